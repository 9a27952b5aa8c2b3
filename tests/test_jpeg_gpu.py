"""Baseline-JPEG decode on the MI355X: mmrca_jpeg_idct_rgb (csrc/jpeg.hip) against the NumPy mirror (tests/jpeg_ref.py), byte for
byte -- one launch over a mixed batch, the alignment gaps, single-image launches, a batch large enough for both kernels' stride
loops -- then GpuJpegDecoder + GpuImagePipeline against the pipeline fed with Pillow's pixels, and the drivers' MMRCA_GPU_JPEG=1
loader against the default one.  No tolerance anywhere: every comparison is exact."""
import io
import os

import numpy as np
import pytest
import torch
from PIL import Image

pytestmark = pytest.mark.gpu

from garbage_classification_rca_amd import jpeg as J             # noqa: E402
from tests import jpeg_ref as R                                  # noqa: E402

FX = R.fixtures()
# 4:4:4 one block; 4:2:0 and 4:2:2 at sizes that are no multiple of the MCU; one chroma row (both vertical neighbours replicated);
# restart markers; greyscale; noise at quality 30 (the clamps; 72 blocks = three workgroups of the IDCT kernel); flat = DC only
MIXED = ["8x8_444_smooth_q75", "17x33_420_smooth_q75", "37x53_422_smooth_q75", "2x35_420_smooth_q75", "16x16_420_smooth_q75_rst1",
         "19x23_grey_smooth_q75", "48x60_420_noise_q30", "24x24_420_flat_q75"]
FILL = 0xA7
_mirror = {}


def mirror(name):
    """the mirror's RGB of a fixture (decoded once, never modified)"""
    if name not in _mirror:
        _mirror[name] = R.decode(FX[name])
        _mirror[name].setflags(write=False)
    return _mirror[name]


def launch(records):
    """one mmrca_jpeg_idct_rgb launch over the records -> (the whole output buffer, prefilled with FILL, and the images' offsets)"""
    batch = J.pack_jpeg(records)
    sizes = [(h * w * 3 + 15) // 16 * 16 for h, w in batch["shapes"].tolist()]
    offsets = np.concatenate([[0], np.cumsum(sizes)])
    J.check_descriptors(batch["desc"].numpy().view(J.DESC_DTYPE), batch["coef"].numel(), int(offsets[-1]))
    out = torch.full((int(offsets[-1]),), FILL, dtype=torch.uint8, device="cuda")
    J.idct_rgb(batch["coef"].cuda(), batch["desc"].cuda(), len(records), out)
    return out.cpu().numpy(), offsets, batch["shapes"].tolist()


def check(out, offsets, shapes, wants):
    for i, ((h, w), want) in enumerate(zip(shapes, wants)):
        n = h * w * 3
        got = out[offsets[i]:offsets[i] + n].reshape(h, w, 3)
        assert want.shape == (h, w, 3) and np.array_equal(got, want), (i, int((got != want).sum()))
        assert (out[offsets[i] + n:offsets[i + 1]] == FILL).all(), f"image {i}: alignment gap written"


def test_fixture_is_what_its_name_says():
    flat = R.parse(FX["24x24_420_flat_q75"])
    assert not flat.coef.reshape(-1, 64)[:, 1:].any()                     # DC only
    noise = mirror("48x60_420_noise_q30")
    assert (noise == 0).any() and (noise == 255).any()                    # the clamps are reached
    assert R.parse(FX["16x16_420_smooth_q75_rst1"]).restart == 1 and R.parse(FX["19x23_grey_smooth_q75"]).ncomp == 1
    assert sum(a * b for a, b in zip(R.parse(FX["48x60_420_noise_q30"]).bpr, R.parse(FX["48x60_420_noise_q30"]).bpc)) == 72


def test_one_launch_over_a_mixed_batch_equals_the_mirror_and_leaves_the_gaps():
    out, offsets, shapes = launch([J.entropy_decode(FX[n]) for n in MIXED])
    assert shapes == [[8, 8], [17, 33], [37, 53], [2, 35], [16, 16], [19, 23], [48, 60], [24, 24]]
    assert any((h * w * 3) % 16 for h, w in shapes)                       # there ARE gaps to leave alone
    check(out, offsets, shapes, [mirror(n) for n in MIXED])


@pytest.mark.parametrize("name", MIXED)
def test_single_image_launch_equals_the_mirror(name):
    out, offsets, shapes = launch([J.entropy_decode(FX[name])])
    check(out, offsets, shapes, [mirror(name)])


def test_stride_loops_of_both_kernels():
    """512 images make the launcher pick its smallest grid (16 workgroups per image); a 300 x 260 image then has 1938 blocks > 16 * 32
    and 4875 pixel groups > 16 * 256, so both kernels go round their loops.  The big image's reference is the mirror's arithmetic on
    the host decoder's coefficients (tests/test_jpeg_cpu.py holds those against the mirror's own Huffman decoder)."""
    data = R.encode(R.image(300, 260, "smooth"), 75, "420")
    big = J.entropy_decode(data)
    p = R.Parsed()
    k = J._constants()
    p.height, p.width, p.ncomp = 300, 260, 3
    p.h, p.v = [2, 1, 1], [2, 1, 1]
    p.bpr = big["info"][k["MMRCA_JPEG_INFO_BPR"]:k["MMRCA_JPEG_INFO_BPR"] + 3].tolist()
    p.bpc = big["info"][k["MMRCA_JPEG_INFO_BPC"]:k["MMRCA_JPEG_INFO_BPC"] + 3].tolist()
    assert sum(a * b for a, b in zip(p.bpr, p.bpc)) == 1938
    p.coef, p.qt = big["coef"], big["qt"].reshape(3, 64)
    want_big = R.planes_to_rgb(p, R.idct_planes(p))
    small = J.entropy_decode(FX["8x8_444_smooth_q75"])
    records = [small] * 200 + [big] + [small] * 311
    out, offsets, shapes = launch(records)
    check(out, offsets, shapes, [mirror("8x8_444_smooth_q75")] * 200 + [want_big] + [mirror("8x8_444_smooth_q75")] * 311)


def _progressive():
    buf = io.BytesIO()
    Image.fromarray(R.image(31, 45, "smooth")).save(buf, format="JPEG", quality=85, progressive=True)
    return buf.getvalue()


def pil_rgb(data):
    return np.array(Image.open(io.BytesIO(data)).convert("RGB"))


def test_decoder_then_pipeline_equals_the_pipeline_fed_with_pillow_pixels():
    from garbage_classification_rca_amd.preprocess import GpuImagePipeline
    files = [FX[n] for n in MIXED[:4]] + [_progressive()] + [FX[n] for n in MIXED[4:]]
    load = J.JpegOrDecode()
    items = []
    for data in files:
        rec = J.entropy_decode(data)
        items.append(rec if rec is not None else load(Image.open(io.BytesIO(data))))
    assert sum(not isinstance(it, dict) for it in items) == 1             # the progressive file was declined
    pixels = [pil_rgb(d) for d in files]
    for name, px in zip(MIXED[:4], pixels):
        assert np.array_equal(px, mirror(name))                           # (Pillow == mirror here as well)
    pipe = GpuImagePipeline(32, 32, max_batch=len(files), max_pixels=64 * 64)
    want = pipe(pixels).cpu()
    batch = J.pack_jpeg(items)
    decoded = J.GpuJpegDecoder("cuda")(batch)
    assert decoded["flat"].is_cuda and decoded["shapes"].tolist() == [list(p.shape[:2]) for p in pixels]
    flat = decoded["flat"].cpu().numpy()
    off = 0
    for px in pixels:
        assert np.array_equal(flat[off:off + px.size].reshape(px.shape), px)
        off += (px.size + 15) // 16 * 16
    assert torch.equal(pipe(decoded).cpu(), want)                          # a flat that already lives on the device
    for _ in range(3):                                                     # the collated batch itself, through both of the decoder's slots
        assert torch.equal(pipe(batch).cpu(), want)
    flips = [(i % 2 == 0, i % 3 == 0) for i in range(len(files))]
    assert torch.equal(pipe(batch, flips=flips).cpu(), pipe(pixels, flips=flips).cpu())
    assert torch.equal(pipe.moments(batch).cpu(), pipe.moments(pixels).cpu())


def test_driver_loader_with_gpu_jpeg_gives_the_same_tensors(tmp_path, monkeypatch):
    """single_modality / main_both build their --gpu_preprocess loaders with main_both.decode_only: one epoch over an 8-file folder
    (six baseline JPEGs, one progressive JPEG, one PNG) with MMRCA_GPU_JPEG=1 and without."""
    from garbage_classification_rca_amd.main_both import collate_decoded, decode_only
    from garbage_classification_rca_amd.preprocess import GpuImagePipeline
    from garbage_classification_rca_amd.training import stage_images
    for i, cls in enumerate(["Black", "Blue", "Green", "TTR"]):
        os.makedirs(tmp_path / cls)
        (tmp_path / cls / f"paper cup_{i}.jpg").write_bytes(R.encode(R.image(40 + 9 * i, 70 - 7 * i, "smooth", seed=i), 90, ["420", "422", "444", "420"][i]))
    (tmp_path / "Black" / "glass jar_4.jpg").write_bytes(R.encode(R.image(64, 48, "noise"), 60, "420", restart=2))
    (tmp_path / "Blue" / "tin can_5.jpg").write_bytes(R.encode(R.image(33, 57, "smooth"), 75, grey=True))
    (tmp_path / "Green" / "pizza box_6.jpg").write_bytes(_progressive())
    Image.fromarray(R.image(21, 30, "smooth")).save(tmp_path / "TTR" / "chip bag_7.png")
    pipe = GpuImagePipeline(32, 32, max_batch=4, max_pixels=80 * 80)

    def epoch():
        ds, collate = decode_only(str(tmp_path))
        assert len(ds) == 8
        dl = torch.utils.data.DataLoader(ds, batch_size=3, shuffle=False, num_workers=0, pin_memory=True, collate_fn=collate)
        out = []
        for data, labels in dl:
            out.append((stage_images(data["image"]["raw_image"], "cuda", pipe).cpu(), labels, data["image"]["image_path"]))
        return collate, out

    monkeypatch.delenv("MMRCA_GPU_JPEG", raising=False)
    collate, want = epoch()
    assert collate is collate_decoded
    monkeypatch.setenv("MMRCA_GPU_JPEG", "1")
    collate, got = epoch()
    assert collate is J.collate_jpeg and len(got) == len(want) == 3
    for (a, la, pa), (b, lb, pb) in zip(got, want):
        assert pa == pb and torch.equal(la, lb) and a.shape == b.shape and torch.equal(a, b)
