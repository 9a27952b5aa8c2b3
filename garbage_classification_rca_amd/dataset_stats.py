"""Per-channel mean / std of an image dataset (main_image.py --calculate_dataset_stats, calculate_mean_std_dataset.py).

The GPU reduces every resized uint8 image to six integers -- per channel {sum v, sum v*v}
(``preprocess.GpuImagePipeline.moments``) -- and everything after that is host arithmetic on those integers, in Python
ints / float64.  This module holds that arithmetic and imports without a GPU; only ``compute`` touches one.

Two formulas exist in the reference, and they do not agree:

* ``reference_mean_std``: what ``main_image.py:223-233`` executes and trains with;
* ``pooled_mean_std``: what the standalone ``calculate_mean_std_dataset.py:22-38`` prints.
"""
from __future__ import annotations

import math
from fractions import Fraction
from typing import List, Sequence, Tuple

import numpy as np

STATS_BATCH = 128          # main_image.py:218 / calculate_mean_std_dataset.py:47


def _batches(sums, batch_sizes: Sequence[int]):
    """per batch: (number of images, [(sum v, sum v*v) per channel] as Python ints)"""
    a = sums.cpu().numpy() if hasattr(sums, "cpu") else np.asarray(sums)
    if a.ndim != 3 or a.shape[1:] != (3, 2):
        raise ValueError("dataset_stats: sums must be [N, 3, 2] (per image, per channel: sum v, sum v*v)")
    if any(int(k) <= 0 for k in batch_sizes) or sum(int(k) for k in batch_sizes) != a.shape[0] or len(batch_sizes) == 0:
        raise ValueError("dataset_stats: batch sizes {} do not cover {} images".format(list(batch_sizes), a.shape[0]))
    out, start = [], 0
    for k in batch_sizes:
        k = int(k)
        rows = a[start:start + k].tolist()          # Python ints: no 64-bit overflow in n * sum v*v below
        out.append((k, [(sum(r[c][0] for r in rows), sum(r[c][1] for r in rows)) for c in range(3)]))
        start += k
    return out


def reference_mean_std(sums, batch_sizes: Sequence[int], pixels_per_image: int) -> Tuple[List[float], List[float]]:
    """(mean[3], std[3]) as ``calculate_mean_std_train_dataset`` (main_image.py:223-233) computes them, quirks included:

    * per batch, the mean over the batch's pixels and the unbiased std over the batch's pixels DIVIDED BY THE NUMBER OF
      IMAGES IN THE BATCH (``torch.std(...) / len(images)``);
    * both averaged over the batches with equal weight, so a short last batch counts as much as a full one;
    * both divided by 255.

    The division by the batch length makes the "std" about 1/128 of the real one.  It runs and changes what the network is
    trained with, so it is reproduced: this project reproduces quirks that run and change results, not crashes
    (header and section 8 a8).  ``pooled_mean_std`` gives the conventional figures.

    ``sums``: [N, 3, 2] per-image integer sums in the order the batches were drawn.  The variance numerator
    n * sum v*v - (sum v)**2 is an exact integer (it cancels badly in floating point); one division and one square root follow."""
    mean_sum, std_sum = [0.0] * 3, [0.0] * 3
    batches = _batches(sums, batch_sizes)
    for k, per_channel in batches:
        n = k * int(pixels_per_image)
        for c, (s1, s2) in enumerate(per_channel):
            mean_sum[c] += s1 / n
            num = n * s2 - s1 * s1
            assert num >= 0
            std_sum[c] += (math.sqrt(num / (n * (n - 1))) if n > 1 else float("nan")) / k      # (torch.std of one element is nan)
    nb = len(batches)
    return [m / nb / 255 for m in mean_sum], [s / nb / 255 for s in std_sum]


def pooled_mean_std(sums, batch_sizes: Sequence[int], pixels_per_image: int) -> Tuple[List[float], List[float]]:
    """(mean[3], std[3]) by ``get_mean_and_std`` of the standalone script (calculate_mean_std_dataset.py:22-38), on the 0..1
    scale of ToTensor: the mean of the batch means, and sqrt(mean of the batch E[x^2] - mean^2).  Evaluated in exact
    rationals up to the square root, so a constant dataset gives exactly 0 and never the root of a negative rounding error."""
    batches = _batches(sums, batch_sizes)
    nb = len(batches)
    mean, std = [], []
    for c in range(3):
        m = sum(Fraction(pc[c][0], k * int(pixels_per_image) * 255) for k, pc in batches) / nb
        e2 = sum(Fraction(pc[c][1], k * int(pixels_per_image) * 255 * 255) for k, pc in batches) / nb
        mean.append(float(m))
        std.append(math.sqrt(e2 - m * m))
    return mean, std


def report(sums, batch_sizes: Sequence[int], pixels_per_image: int) -> Tuple[List[float], List[float]]:
    """main_image.py:436-437's line with the reference values (returned: they are what training normalises with), then one more
    with the pooled values, so the reader sees both."""
    mean, std = reference_mean_std(sums, batch_sizes, pixels_per_image)
    print("Mean Train Dataset: {}, STD Train Dataset: {}".format(mean, std))
    pm, ps = pooled_mean_std(sums, batch_sizes, pixels_per_image)
    print("Pooled over the dataset (not used; the STD above is divided by the batch length as in the reference): mean {}, std {}".format(pm, ps))
    return mean, std


def compute(dataset_root, width: int, height: int, device="cuda", pad: bool = False, seed=None, num_workers: int = 0, pipeline=None):
    """One pass over ``CustomImageTextFolder(dataset_root)``: decode in the loader workers, resize to (height, width) and
    reduce on the GPU.  -> (int64 [N, 3, 2] per-image sums on the host, batch sizes).

    The images are drawn shuffled in batches of 128 as in the reference (which images share a batch matters to
    ``reference_mean_std``); the generator is seeded from ``seed``.  The batches are formed here, on the host, from per-image
    sums: a ``pipeline`` with room for fewer than 128 images is fed smaller chunks of the same permutation and the result does
    not change.  pad=False is the reference's STATS_PIPELINE (main_image.py:412-417: a stretch resize), pad=True puts
    PadToMaintainAR in front as the standalone script does."""
    import torch
    from .CustomImageTextFolder import CustomImageTextFolder
    from .main_both import DecodeOnly, collate_decoded
    from .preprocess import GpuImagePipeline
    if pipeline is None or (pipeline.out_h, pipeline.out_w) != (int(height), int(width)):
        pipeline = GpuImagePipeline(height, width, max_batch=STATS_BATCH, max_pixels=640 * 480, device=device)
    data = CustomImageTextFolder(root=dataset_root, transform=DecodeOnly())
    gen = torch.Generator()
    if seed is not None:
        gen.manual_seed(int(seed))
    nw = min(int(num_workers), 16)
    loader = torch.utils.data.DataLoader(data, batch_size=min(STATS_BATCH, pipeline.max_batch), shuffle=True, num_workers=nw, pin_memory=True,
                                         collate_fn=collate_decoded, generator=gen, multiprocessing_context="forkserver" if nw > 0 else None)
    parts = [pipeline.moments(batch["image"]["raw_image"], pad=pad).cpu() for batch, _ in loader]
    n = len(data)
    sums = torch.cat(parts).numpy() if parts else np.zeros((0, 3, 2), dtype=np.int64)
    assert sums.shape[0] == n
    return sums, [min(STATS_BATCH, n - i) for i in range(0, n, STATS_BATCH)]
