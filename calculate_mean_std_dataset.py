#!/usr/bin/env python
"""Entry point with the reference's name: ``python calculate_mean_std_dataset.py --dataset_path=<folder>``."""
from garbage_classification_rca_amd.calculate_mean_std_dataset import main

if __name__ == "__main__":
    main()
