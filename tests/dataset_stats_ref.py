"""The two dataset-statistics formulas of the reference, restated on float tensors for the tests.

``reference_formula``: the loop of ``calculate_mean_std_train_dataset`` (main_image.py:223-233) -- per batch the channel mean and
the (unbiased) channel std of the batch divided by the number of images in it, summed, then divided by the number of batches and by 255.
``pooled_formula``: ``get_mean_and_std`` (calculate_mean_std_dataset.py:22-38) on ToTensor's 0..1 scale -- per batch E[x] and E[x^2],
averaged over the batches, std = sqrt(E[x^2] - E[x]^2).

Both take the batches as the DataLoader would deliver them, uint8 [k, 3, H, W], and evaluate in ``dtype``: float32 is what the
reference executes, float64 is the yardstick for the integer implementation.
"""
import torch


def reference_formula(batches, dtype=torch.float64):
    mean_acc = torch.zeros(3, dtype=dtype)
    std_acc = torch.zeros(3, dtype=dtype)
    for images in batches:
        x = images.to(dtype)
        mean_acc = mean_acc + x.mean(dim=(0, 2, 3))
        std_acc = std_acc + x.std(dim=(0, 2, 3)) / x.shape[0]
    n = len(batches)
    return mean_acc / n / 255, std_acc / n / 255


def pooled_formula(batches, dtype=torch.float64):
    first = torch.zeros(3, dtype=dtype)
    second = torch.zeros(3, dtype=dtype)
    for images in batches:
        x = images.to(dtype) / 255
        first = first + x.mean(dim=(0, 2, 3))
        second = second + (x * x).mean(dim=(0, 2, 3))
    n = len(batches)
    mean = first / n
    return mean, torch.sqrt(second / n - mean * mean)


def image_sums(images):
    """uint8 [N, 3, H, W] -> int64 [N, 3, 2]: per image and channel (sum v, sum v*v)"""
    x = images.to(torch.int64)
    return torch.stack([x.sum(dim=(2, 3)), (x * x).sum(dim=(2, 3))], dim=-1)
