#!/usr/bin/env python
"""Entry point with the reference's name: ``python main_image.py --image_model=... --dataset_folder_name=<name> ...``."""
from garbage_classification_rca_amd.main_image import main

if __name__ == "__main__":
    main()
