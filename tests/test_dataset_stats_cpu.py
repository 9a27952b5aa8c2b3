"""dataset_stats.py (host arithmetic of --calculate_dataset_stats) against the float restatements of the reference's two formulas
(tests/dataset_stats_ref.py), the mean / std arguments of main_both.Transforms, and the command lines.  No GPU."""
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

from garbage_classification_rca_amd import dataset_stats as DS
from tests.dataset_stats_ref import image_sums, pooled_formula, reference_formula

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
H, W = 12, 16


def _images(n, seed, h=H, w=W):
    """uint8 [n, 3, h, w]: channels with different means and spreads (a channel-symmetric input would hide a channel mix-up)"""
    g = torch.Generator().manual_seed(seed)
    x = torch.rand(n, 3, h, w, generator=g) * torch.tensor([255.0, 180.0, 90.0]).view(1, 3, 1, 1) + torch.tensor([0.0, 40.0, 120.0]).view(1, 3, 1, 1)
    return x.clamp_(0, 255).to(torch.uint8)


def _split(images, sizes):
    return list(torch.split(images, sizes))


def _rel(got, ref):
    got, ref = torch.tensor(got, dtype=torch.float64), ref.to(torch.float64)
    return float(((got - ref).abs() / ref.abs()).max())


@pytest.mark.parametrize("sizes", [[128, 128, 44], [5], [128, 1]])
def test_reference_formula_matches_float64(sizes):
    """[128, 1]: a one-image last batch works (its pixel count is far above 1) and counts as much as the full batch."""
    imgs = _images(sum(sizes), seed=len(sizes))
    mean, std = DS.reference_mean_std(image_sums(imgs), sizes, H * W)
    rm, rs = reference_formula(_split(imgs, sizes))
    assert _rel(mean, rm) < 1e-12 and _rel(std, rs) < 1e-12, (_rel(mean, rm), _rel(std, rs))


def test_constant_images_have_exactly_zero_std():
    imgs = torch.full((7, 3, H, W), 37, dtype=torch.uint8)
    imgs[:, 1] = 201
    for fn in (DS.reference_mean_std, DS.pooled_mean_std):
        mean, std = fn(image_sums(imgs), [4, 3], H * W)
        assert std == [0.0, 0.0, 0.0]
        assert mean == pytest.approx([37 / 255, 201 / 255, 37 / 255], rel=1e-15)


def test_all_255_images_at_full_size():
    """the largest sums there are: 128 images of 224 x 256 at 255 (sum v*v = 65025 * 7.3e6 per channel and batch; the variance numerator
    n * sum v*v is ~2.6e25, beyond int64 -- Python ints)"""
    sums = torch.tensor([[[255 * 224 * 256, 65025 * 224 * 256]] * 3] * 129, dtype=torch.int64)
    for fn in (DS.reference_mean_std, DS.pooled_mean_std):
        mean, std = fn(sums, [128, 1], 224 * 256)
        assert mean == [1.0, 1.0, 1.0] and std == [0.0, 0.0, 0.0]


@pytest.mark.parametrize("k", [5, 12])
def test_std_is_divided_by_the_batch_length(k):
    """main_image.py:228 ``torch.std(...) / len(images)``: one batch of k images -> unbiased std over all pixels / k / 255"""
    imgs = _images(k, seed=k)
    _, std = DS.reference_mean_std(image_sums(imgs), [k], H * W)
    x = imgs.to(torch.float64).permute(1, 0, 2, 3).reshape(3, -1)
    n = x.shape[1]
    unbiased = torch.sqrt(((x - x.mean(1, keepdim=True)) ** 2).sum(1) / (n - 1))
    assert _rel(std, unbiased / k / 255) < 1e-12


def test_reference_formula_in_float32_as_the_reference_runs_it():
    """Against the literal float32 evaluation (what the reference executes), one full batch of 128 images of 224 x 256 plus a short
    batch of 6.  Measured on the development CPU: relative difference 9.8e-8 (mean) and 8.4e-8 (std), the same with 1, 4 and 16 threads; the assertion allows
    ten times that for another CPU's summation order, and in any case less than 1e-5."""
    MEAN_F32, STD_F32 = 9.8e-8, 8.4e-8
    sizes = [128, 6]
    imgs = _images(sum(sizes), seed=11, h=224, w=256)
    mean, std = DS.reference_mean_std(image_sums(imgs), sizes, 224 * 256)
    rm, rs = reference_formula(_split(imgs, sizes), torch.float32)
    dm, ds = _rel(mean, rm), _rel(std, rs)
    print("float32 restatement: rel diff mean {:.3e} std {:.3e}".format(dm, ds))
    assert dm <= 10 * MEAN_F32 and ds <= 10 * STD_F32 and max(dm, ds) < 1e-5, (dm, ds)


@pytest.mark.parametrize("sizes", [[128, 128, 44], [5], [128, 1]])
def test_pooled_formula_matches_float64(sizes):
    imgs = _images(sum(sizes), seed=3 + len(sizes))
    mean, std = DS.pooled_mean_std(image_sums(imgs), sizes, H * W)
    rm, rs = pooled_formula(_split(imgs, sizes))
    assert _rel(mean, rm) < 1e-12 and _rel(std, rs) < 1e-12, (_rel(mean, rm), _rel(std, rs))


def test_sums_and_batch_sizes_must_agree():
    sums = image_sums(_images(5, seed=0))
    with pytest.raises(ValueError):
        DS.reference_mean_std(sums, [4], H * W)
    with pytest.raises(ValueError):
        DS.pooled_mean_std(sums[:, :2], [5], H * W)


def test_transforms_normalise_with_the_given_constants():
    from PIL import Image
    from garbage_classification_rca_amd.main_both import Transforms
    rng = np.random.default_rng(4)
    arr = rng.integers(0, 256, (24, 24, 3), dtype=np.uint8)          # square and already the output size: pad + resize is the identity
    img = Image.fromarray(arr)
    m, s = (0.61, 0.52, 0.43), (0.0021, 0.0019, 0.0023)
    x01 = torch.from_numpy(arr).permute(2, 0, 1).double() / 255
    got = Transforms(24, 24, mean=m, std=s)(img)
    want = (x01 - torch.tensor(m, dtype=torch.float64).view(3, 1, 1)) / torch.tensor(s, dtype=torch.float64).view(3, 1, 1)
    assert got.dtype == torch.float32 and float((got.double() - want).abs().max() / want.abs().max()) < 1e-6
    # without them: ImageNet's, and the class constants are untouched by the instance above
    default = Transforms(24, 24)(img)
    inet_m, inet_s = torch.tensor([0.485, 0.456, 0.406]).view(3, 1, 1), torch.tensor([0.229, 0.224, 0.225]).view(3, 1, 1)
    assert torch.equal(default, (x01.float() - inet_m) / inet_s)
    assert torch.equal(Transforms.MEAN, inet_m) and torch.equal(Transforms.STD, inet_s)
    assert torch.equal(default, Transforms(24, 24, False, 0.0)(img))
    # a resized, padded image: the custom constants are an affine map of the default output
    big = Image.fromarray(rng.integers(0, 256, (50, 31, 3), dtype=np.uint8))
    a, b = Transforms(28, 20, mean=m, std=s)(big), Transforms(28, 20)(big)
    want = (b.double() * inet_s.double() + inet_m.double() - torch.tensor(m, dtype=torch.float64).view(3, 1, 1)) / torch.tensor(s, dtype=torch.float64).view(3, 1, 1)
    assert float((a.double() - want).abs().max() / want.abs().max()) < 1e-5


def test_command_lines_parse():
    from garbage_classification_rca_amd.options import args_parser
    assert args_parser(["--calculate_dataset_stats"]).calculate_dataset_stats is True
    assert args_parser([]).calculate_dataset_stats is False
    from garbage_classification_rca_amd.calculate_mean_std_dataset import args_parser as tool_parser
    a = tool_parser(["--dataset_path", "x"])
    assert (a.width, a.height, a.seed) == (384, 380, None)
    r = subprocess.run([sys.executable, os.path.join(ROOT, "calculate_mean_std_dataset.py"), "--help"], capture_output=True, text=True,
                       env=dict(os.environ, PYTHONPATH=ROOT), timeout=120)
    assert r.returncode == 0 and "--dataset_path" in r.stdout and "--width" in r.stdout and "--seed" in r.stdout
