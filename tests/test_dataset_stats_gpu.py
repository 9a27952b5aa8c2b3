"""--calculate_dataset_stats on the MI355X: the integer reduction (csrc/preprocess.hip::image_stats_k, GpuImagePipeline.moments) against
the resize kernel's own output and against the oracle's resize, the mean / std constants of the pipeline, and main_image.py /
calculate_mean_std_dataset.py end to end."""
import glob
import os
import re
import subprocess
import sys

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from garbage_classification_rca_amd import lib as L             # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
OUT_SIZES = [(7, 5), (96, 96), (224, 256)]          # under one block / several blocks / 64 blocks with 3.5 pixels per thread
_pipes, _images = {}, {}


def _pipe(h, w):
    from garbage_classification_rca_amd.preprocess import GpuImagePipeline
    if (h, w) not in _pipes:
        _pipes[(h, w)] = GpuImagePipeline(h, w, max_batch=130, max_pixels=400 * 300)
    return _pipes[(h, w)]


def _smooth(rng, h, w):
    """tests/test_augment_gpu.py::_smooth: a low-frequency image + noise + one flat rectangle"""
    yy, xx = np.mgrid[0:h, 0:w].astype(np.float32)
    base = 127 + 80 * np.sin(xx / (5 + 20 * rng.random())) * np.cos(yy / (7 + 20 * rng.random()))
    img = base[..., None] + rng.normal(0, 25, (h, w, 3))
    img[h // 3: h // 2, w // 4: w // 2] = rng.integers(0, 256, 3)
    return np.clip(img, 0, 255).astype(np.uint8)


def _sources(out_h, out_w):
    """1 x 1, tall-and-narrow, larger than every output (down-scaling), already the output size, and all-255 (the largest sums)"""
    if (out_h, out_w) not in _images:
        rng = np.random.default_rng(out_h * 1000 + out_w)
        _images[(out_h, out_w)] = [np.array([[[13, 200, 77]]], dtype=np.uint8), _smooth(rng, 97, 331), _smooth(rng, 400, 300),
                                   _smooth(rng, out_h, out_w), np.full((300, 400, 3), 255, dtype=np.uint8), _smooth(rng, 300, 400)]
    return _images[(out_h, out_w)]


def _batch(out_h, out_w, B):
    src = _sources(out_h, out_w)
    return [src[i % len(src)] for i in range(B)]


def _np_sums(img):
    x = img.astype(np.int64).reshape(-1, 3)
    return np.stack([x.sum(0), (x * x).sum(0)], axis=-1)


def _resized_by_the_kernel(pipe, B):
    """mmrca_image_resize_u8 on the batch that the last call staged (the slot it used still holds images and descriptors)"""
    k = (pipe._i - 1) & 1
    out = torch.empty(B, pipe.out_h, pipe.out_w, 3, dtype=torch.uint8, device=pipe.device)
    L._check(L.load().mmrca_image_resize_u8(L.ptr(pipe._dev[k]), L.ptr(pipe._dev_desc[k]), L.ptr(out), B, pipe.out_h, pipe.out_w, L.stream_ptr()),
             "mmrca_image_resize_u8")
    return out


@pytest.mark.parametrize("B", [1, 3, 130])
@pytest.mark.parametrize("pad", [True, False])
@pytest.mark.parametrize("out_hw", OUT_SIZES)
def test_moments_equal_the_sums_of_the_resize_kernels_output(out_hw, pad, B):
    """to the integer: both kernels call one sampling function, and integer sums have no order"""
    pipe = _pipe(*out_hw)
    imgs = _batch(*out_hw, B)
    got = pipe.moments(imgs, pad=pad)
    assert got.dtype == torch.int64 and got.shape == (B, 3, 2) and got.device.type == "cuda"
    u8 = _resized_by_the_kernel(pipe, B).to(torch.int64)
    want = torch.stack([u8.sum(dim=(1, 2)), (u8 * u8).sum(dim=(1, 2))], dim=-1)
    assert torch.equal(got, want), (got - want).abs().max().item()
    if B >= 5:          # the all-255 image: 255 * pixels and 65025 * pixels (with padding: of the part the image covers)
        npix = out_hw[0] * out_hw[1]
        assert got[4, :, 0].max().item() <= 255 * npix and got[4, :, 1].max().item() <= 65025 * npix
        if not pad:
            assert got[4].tolist() == [[255 * npix, 65025 * npix]] * 3


@pytest.mark.parametrize("out_hw,pad", [((7, 5), False), ((96, 96), False), ((96, 96), True), ((224, 256), False)])
def test_identity_resize_gives_the_sums_of_the_source(out_hw, pad):
    """sources that already have the output size (and, with padding, its aspect ratio by PadToMaintainAR's reading: square): the
    resize is the identity, in the kernel as in oracle.transforms.resize_linear_u8, so the sums are numpy's sums of the source"""
    from oracle import transforms as T
    rng = np.random.default_rng(7)
    imgs = [_smooth(rng, *out_hw) for _ in range(3)] + [np.full((*out_hw, 3), 255, dtype=np.uint8)]
    assert all(np.array_equal(T.resize_linear_u8(im, *out_hw), im) for im in imgs)
    got = _pipe(*out_hw).moments(imgs, pad=pad).cpu().numpy()
    assert np.array_equal(got, np.stack([_np_sums(im) for im in imgs]))


@pytest.mark.parametrize("pad", [True, False])
@pytest.mark.parametrize("out_hw", [(96, 96), (224, 256)])
def test_moments_against_the_oracles_resize(out_hw, pad):
    """tests/test_augment_gpu.py::test_rotate_crop_then_pad_resize lets a share of 2e-3 of an image's elements differ from the oracle
    by one uint8 step (an x.5 tap sum rounded to the neighbouring step).  Restated for the sums of an image of 3 * H * W elements:
    sum over channels |d sum v| <= 2e-3 * 3HW, and, one step changing v*v by at most 2 * 255 = 510, |d sum v*v| <= 510 * that.
    (7 x 5 is left to the two exact tests: 2e-3 of its 105 elements is less than one element.)"""
    from oracle import transforms as T
    out_h, out_w = out_hw
    imgs = _sources(out_h, out_w)
    got = _pipe(out_h, out_w).moments(imgs, pad=pad).cpu().numpy()
    count = 2e-3 * 3 * out_h * out_w
    for b, img in enumerate(imgs):
        src = T.pad_to_maintain_ar(img, out_w / out_h) if pad else img
        want = _np_sums(T.resize_linear_u8(src, out_h, out_w))
        d1, d2 = np.abs(got[b, :, 0] - want[:, 0]).sum(), np.abs(got[b, :, 1] - want[:, 1]).sum()
        print(out_hw, pad, img.shape, "d sum v", d1, "d sum v*v", d2, "allowed", count, 510 * count)
        assert d1 <= count and d2 <= 510 * count, (img.shape, d1, d2, count)


def test_four_calls_in_a_row_agree_for_every_input_form():
    """four consecutive calls use both staging slots twice; a list of arrays, a packed batch and a pinned packed batch"""
    from garbage_classification_rca_amd.preprocess import pack_images
    pipe = _pipe(96, 96)
    imgs = _batch(96, 96, 7)
    packed = pack_images([torch.from_numpy(i) for i in imgs])
    pinned = {"flat": packed["flat"].pin_memory(), "shapes": packed["shapes"]}
    first = pipe.moments(imgs).clone()
    for form in (imgs, packed, pinned):
        for rep in range(4):
            assert torch.equal(pipe.moments(form), first), (type(form), rep)
    other = pipe.moments(imgs, pad=False)
    assert not torch.equal(other, first)          # (and pad=False is a different resize of the non-square sources)


@pytest.mark.parametrize("launch", ["validation", "aug"])
def test_mean_and_std_reach_the_kernels(launch):
    from garbage_classification_rca_amd.preprocess import MEAN, STD, GpuImagePipeline
    m, s = (0.61, 0.52, 0.43), (0.0021, 0.0019, 0.0023)
    rng = np.random.default_rng(5)
    imgs = [_smooth(rng, 80, 120), _smooth(rng, 150, 90), _smooth(rng, 64, 48)]
    kw = {} if launch == "validation" else dict(aug=[dict(blur_k=3, flip_h=True), dict(angle=20.0, bc=(1.1, -0.05)), dict(scale=0.8, sharpen=(0.3, 0.7))])
    default = GpuImagePipeline(64, 48, max_batch=4, max_pixels=150 * 120)(imgs, **kw).double().cpu()
    custom = GpuImagePipeline(64, 48, max_batch=4, max_pixels=150 * 120, mean=m, std=s)(imgs, **kw).double().cpu()
    col = lambda v: torch.tensor(v, dtype=torch.float64).view(1, 3, 1, 1)      # noqa: E731
    want = (default * col(STD) + col(MEAN) - col(m)) / col(s)
    assert float((custom - want).abs().max() / want.abs().max()) < 1e-5
    assert torch.equal(GpuImagePipeline(64, 48, max_batch=4, max_pixels=150 * 120, mean=MEAN, std=STD)(imgs, **kw).double().cpu(), default)


def _tiny_folder(tmp_path):
    """12 training and 8 validation PNGs of 64 x 64, four classes (tests/test_classifier_gpu.py::_tiny_folder's kind)"""
    from PIL import Image
    rng = np.random.default_rng(0)
    train = []
    for split, per_class in (("Train", 3), ("Val", 2)):
        for ci, c in enumerate(["Black", "Blue", "Green", "TTR"]):
            d = tmp_path / f"Tiny_{split}" / c
            d.mkdir(parents=True)
            for k in range(per_class):
                arr = (rng.random((64, 64, 3)) * 255).astype(np.uint8)
                arr[:, :, ci % 3] = 255 - 40 * ci
                Image.fromarray(arr).save(d / f"{['chip_bag', 'pizza_box', 'banana_peel', 'aa_batteries'][ci]}_{k}.png")
                if split == "Train":
                    train.append(arr)
    return np.stack(train)


def _floats(text):
    return [float(v) for v in re.findall(r"[-+]?\d+\.?\d*(?:[eE][-+]?\d+)?", text)]


def test_main_image_trains_with_the_datasets_own_statistics(tmp_path):
    """main_image.py --calculate_dataset_stats: the statistics pass runs, prints the reference's lines with the values of
    main_image.py:223-233 (one batch of 12, identity resize: computed here from the PNGs with numpy), trains and saves a checkpoint;
    calculate_mean_std_dataset.py prints the pooled values for the same folder."""
    train = _tiny_folder(tmp_path).astype(np.float64)          # [12, 64, 64, 3]
    env = dict(os.environ, PYTHONPATH=ROOT)
    r = subprocess.run([sys.executable, os.path.join(ROOT, "main_image.py"), "--image_model=mb", "--dataset_folder_name=Tiny", "--image_size", "64",
                        "--calculate_dataset_stats", "--epochs", "1", "--ft_epochs", "1", "--num_workers", "0", "--seed", "3"],
                       cwd=tmp_path, env=env, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stdout[-1500:] + r.stderr[-3000:]
    assert "Calculating Train Dataset statistics..." in r.stdout
    assert "accepted for CLI compatibility; the ImageNet mean / std" not in r.stdout
    line = [l for l in r.stdout.splitlines() if l.startswith("Mean Train Dataset:")]
    assert len(line) == 1, r.stdout[-3000:]
    mean_txt, std_txt = line[0].split("STD Train Dataset:")
    px = train.reshape(-1, 3)
    want_mean = px.mean(0) / 255
    want_std = px.std(0, ddof=1) / 12 / 255
    assert np.allclose(_floats(mean_txt), want_mean, rtol=1e-6, atol=0), (mean_txt, want_mean)
    assert np.allclose(_floats(std_txt), want_std, rtol=1e-6, atol=0), (std_txt, want_std)
    assert glob.glob(str(tmp_path / "model_weights" / "mb" / "BEST_model_mb_*.pth")), r.stdout[-3000:]

    r2 = subprocess.run([sys.executable, os.path.join(ROOT, "calculate_mean_std_dataset.py"), "--dataset_path", str(tmp_path / "Tiny_Train"),
                         "--width", "64", "--height", "64", "--seed", "3", "--num_workers", "0"], cwd=tmp_path, env=env, capture_output=True, text=True,
                        timeout=300)
    assert r2.returncode == 0, r2.stdout[-1500:] + r2.stderr[-3000:]
    out = dict(l.split(": ", 1) for l in r2.stdout.splitlines() if l.startswith(("mean: ", "std: ")))
    x = px / 255
    assert np.allclose(_floats(out["mean"]), x.mean(0), rtol=1e-6, atol=0), out
    assert np.allclose(_floats(out["std"]), np.sqrt((x * x).mean(0) - x.mean(0) ** 2), rtol=1e-6, atol=0), out
