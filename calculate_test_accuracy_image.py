#!/usr/bin/env python
"""Entry point with the reference's name: ``python calculate_test_accuracy_image.py ... --model_path=<checkpoint.pth> --dataset_folder_name=<Test folder>``."""
from garbage_classification_rca_amd.calculate_test_accuracy_image import main

if __name__ == "__main__":
    main()
