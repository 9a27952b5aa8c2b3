"""Per-channel mean / std of an image folder: the reference's standalone ``calculate_mean_std_dataset.py`` on the GPU input path.

    python calculate_mean_std_dataset.py --dataset_path=<folder of class sub-folders> [--width 384 --height 380] [--seed N]

As in the reference: PadToMaintainAR(width / height), resize, batches of 128 shuffled, then ``get_mean_and_std``
(calculate_mean_std_dataset.py:22-38; dataset_stats.pooled_mean_std) and the lines ``mean: ...`` / ``std: ...`` on the 0..1 scale.

Deviations.  The reference resizes bicubically through PIL (``transforms.Resize(..., BICUBIC)``) and keeps the float result of
ToTensor; this tool uses the GPU pipeline's resize, INTER_LINEAR rounded to uint8 -- the images the training pipelines see.  The
reference's folder is a constant in the script; here it is ``--dataset_path``, and the output is ``--width`` wide and ``--height``
high (the reference hands ``(WIDTH, HEIGHT)`` to a function that reads it as (height, width)).
"""
from __future__ import annotations

import argparse
import sys


def args_parser(argv=None):
    p = argparse.ArgumentParser(description="per-channel mean / std of an image dataset, computed on the GPU")
    p.add_argument("--dataset_path", type=str, required=True, help="folder with one sub-folder per class")
    p.add_argument("--width", type=int, default=384, help="resize width (calculate_mean_std_dataset.py:11)")
    p.add_argument("--height", type=int, default=380, help="resize height (calculate_mean_std_dataset.py:12)")
    p.add_argument("--seed", type=int, default=None, help="seed of the shuffle")
    p.add_argument("--num_workers", type=int, default=8, help="decoding workers (calculate_mean_std_dataset.py:48)")
    return p.parse_args(argv)


def main(argv=None):
    args = args_parser(argv)
    import torch
    from . import dataset_stats
    if not torch.cuda.is_available():
        print("GPU not available!!!!  The image pipeline has no CPU fallback.")
        sys.exit(1)
    sums, batch_sizes = dataset_stats.compute(args.dataset_path, args.width, args.height, "cuda:0", pad=True, seed=args.seed,
                                              num_workers=args.num_workers)
    mean, std = dataset_stats.pooled_mean_std(sums, batch_sizes, args.width * args.height)
    print("mean: {}".format(mean))
    print("std: {}".format(std))


if __name__ == "__main__":
    main()
