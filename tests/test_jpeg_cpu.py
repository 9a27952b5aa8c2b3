"""Baseline-JPEG decode without a GPU: the NumPy mirror (tests/jpeg_ref.py) against Pillow and against the committed goldens, the
host entropy decoder (csrc/jpeg_entropy.cpp through garbage_classification_rca_amd/jpeg.py) against the mirror, what it declines,
that damaged input can neither crash it nor make it write past its buffer, collate_jpeg, and the unchanged mmrca.h ABI pins.
All comparisons are exact."""
import io
import os

import numpy as np
import pytest
import torch
from PIL import Image, features

from garbage_classification_rca_amd import abi, jpeg as J, lib as L
from tests import jpeg_ref as R

K = J._constants()
FX = R.fixtures()
_parsed = {}


def parsed(name):
    if name not in _parsed:
        _parsed[name] = R.parse(FX[name])
    return _parsed[name]


def pil_rgb(data):
    return np.array(Image.open(io.BytesIO(data)).convert("RGB"))


def accepted(name):
    return not R.declined_by_rule(*R.fixture_width_sub(name))


def test_fixture_list_covers_what_the_issue_names():
    names = list(FX)
    for h, w in R.SIZES:
        for sub in R.SUBSAMPLINGS:
            assert f"{h}x{w}_{sub}_smooth_q75" in names
    for q in (30, 75, 95, 100):
        assert any(n.endswith(f"_q{q}") for n in names)
    assert any("noise" in n for n in names) and any("rst" in n for n in names) and "19x23_grey_smooth_q75" in names
    # the only fixtures the width rule excludes are the 1 x 1 files with halved chroma (identical either way, see below)
    assert [n for n in names if not accepted(n)] == ["1x1_422_smooth_q75", "1x1_420_smooth_q75"]


def test_mirror_equals_pillow_on_every_fixture():
    if not features.check_feature("libjpeg_turbo"):
        pytest.skip("this Pillow is not built on libjpeg-turbo: another libjpeg upsamples chroma differently")
    for name, data in FX.items():          # (the 1 x 1 files included: one sample, nothing to interpolate)
        assert np.array_equal(R.decode(data), pil_rgb(data)), name


def test_mirror_equals_the_golden_file():
    g = np.load(R.GOLDEN_PATH)
    assert os.path.getsize(R.GOLDEN_PATH) < 100_000
    names = [k[5:] for k in g.files if k.startswith("jpeg/")]
    assert sorted(names) == sorted(R.GOLDEN_NAMES) and len(names) == 12
    for name in names:
        assert np.array_equal(R.decode(g["jpeg/" + name].tobytes()), g["rgb/" + name]), name


def test_c_decoder_equals_the_mirror_on_every_fixture():
    for name, data in FX.items():
        rec, code = J.entropy_decode(data, return_code=True)
        if not accepted(name):
            assert rec is None and code == K["MMRCA_JPEG_THIN_CHROMA"], name
            continue
        assert code == 0, (name, J.decline_reason(code))
        p = parsed(name)
        assert rec["coef"].dtype == np.int16 and np.array_equal(rec["coef"], p.coef), name
        assert np.array_equal(rec["qt"].reshape(3, 64), p.qt), name


def test_probe_equals_the_mirror():
    for name, data in FX.items():
        if not accepted(name):
            continue
        code, info = J.probe(data)
        p = parsed(name)
        assert code == 0 and info.dtype == np.int32 and len(info) == K["MMRCA_JPEG_INFO_LEN"]
        n = p.ncomp
        assert (info[K["MMRCA_JPEG_INFO_WIDTH"]], info[K["MMRCA_JPEG_INFO_HEIGHT"]], info[K["MMRCA_JPEG_INFO_NCOMP"]]) == (p.width, p.height, n)
        for key, want in (("H", p.h), ("V", p.v), ("TQ", p.tq), ("BPR", p.bpr), ("BPC", p.bpc)):
            at = K["MMRCA_JPEG_INFO_" + key]
            assert info[at:at + n].tolist() == want and not info[at + n:at + 3].any(), (name, key)
        assert info[K["MMRCA_JPEG_INFO_NCOEF"]] == p.ncoef == p.coef.size
        assert info[K["MMRCA_JPEG_INFO_RESTART"]] == p.restart
    assert parsed("16x16_420_smooth_q75_rst1").restart == 1 and parsed("48x60_420_noise_q75_rst3").restart == 3


def _png():
    buf = io.BytesIO()
    Image.fromarray(R.image(9, 11, "smooth")).save(buf, format="PNG")
    return buf.getvalue()


def _declined_files():
    smooth = Image.fromarray(R.image(24, 40, "smooth"))
    out = {}
    buf = io.BytesIO()
    smooth.save(buf, format="JPEG", quality=80, progressive=True)
    out["progressive"] = (buf.getvalue(), K["MMRCA_JPEG_NOT_BASELINE"])
    buf = io.BytesIO()
    smooth.convert("CMYK").save(buf, format="JPEG", quality=80)
    out["cmyk"] = (buf.getvalue(), K["MMRCA_JPEG_COMPONENTS"])
    out["35x2_420"] = (R.encode(R.image(35, 2, "smooth"), 75, "420"), K["MMRCA_JPEG_THIN_CHROMA"])
    out["png"] = (_png(), K["MMRCA_JPEG_NOT_JPEG"])
    return out


def _mutations(n=200, seed=20240607):
    """n single-byte mutations, spread over three fixtures: (name, position, mutated bytes)"""
    rng = np.random.default_rng(seed)
    names = ["17x33_420_smooth_q75", "48x60_420_noise_q75_rst3", "19x23_grey_smooth_q75"]
    for i in range(n):
        name = names[i % len(names)]
        data = bytearray(FX[name])
        pos = int(rng.integers(0, len(data)))
        data[pos] ^= int(rng.integers(1, 256))
        yield name, pos, bytes(data)


def test_declined_files_fall_back_to_pillow(tmp_path):
    load = J.JpegOrDecode()
    for name, (data, want) in _declined_files().items():
        code, info = J.probe(data)
        assert code == want and code > 0 and info is None, (name, J.decline_reason(code))
        rec, code = J.entropy_decode(data, return_code=True)
        assert rec is None and code == want, name
        path = tmp_path / (name + (".png" if name == "png" else ".jpg"))
        path.write_bytes(data)
        got = load(load.load(str(path)))
        assert isinstance(got, torch.Tensor) and got.dtype == torch.uint8 and np.array_equal(got.numpy(), pil_rgb(data)), name
    # an accepted file comes back as its coefficient record, untouched by the transform half
    path = tmp_path / "ok.jpg"
    path.write_bytes(FX["17x33_420_smooth_q75"])
    import pickle
    load = pickle.loads(pickle.dumps(load))                 # spawn / forkserver workers receive the pair pickled
    rec = load(pickle.loads(pickle.dumps(load.load))(str(path)))
    assert isinstance(rec, dict) and np.array_equal(rec["coef"], parsed("17x33_420_smooth_q75").coef)


def test_truncated_files_are_declined():
    for name in ("37x53_422_smooth_q75", "48x60_420_noise_q75_rst3"):
        data = FX[name]
        for cut in range(0, len(data), 97):
            rec, code = J.entropy_decode(data[:cut], return_code=True)
            assert rec is None and code > 0, (name, cut)
        assert J.entropy_decode(data[:-2], return_code=True)[1] == K["MMRCA_JPEG_STREAM"]          # no EOI


def _decode_with_canary(data, capacity):
    """mmrca_jpeg_entropy_decode into a buffer of `capacity` coefficients followed by canary words -> (code, coef, canary intact)"""
    canary = 64
    buf = np.full(capacity + canary, 0x5A5A, dtype=np.uint16).view(np.int16)
    qt = np.zeros(192 + canary, dtype=np.uint16)
    qt[192:] = 0xA5A5
    code = J.load_host().mmrca_jpeg_entropy_decode(data, len(data), buf.ctypes.data, capacity, qt.ctypes.data)
    intact = bool((buf[capacity:].view(np.uint16) == 0x5A5A).all() and (qt[192:] == 0xA5A5).all())
    return code, buf[:capacity], qt[:192], intact


def test_mutated_files_return_and_stay_inside_the_buffer(tmp_path):
    load = J.JpegOrDecode()
    outcomes = {"declined": 0, "decoded": 0}
    for i, (name, pos, data) in enumerate(_mutations()):
        capacity = parsed(name).ncoef                    # the ORIGINAL file's size: a mutated header may ask for more
        code, coef, qt, intact = _decode_with_canary(data, capacity)
        assert intact, (name, pos)
        assert code >= 0
        if code == 0:
            _, info = J.probe(data)
            n = int(info[K["MMRCA_JPEG_INFO_NCOEF"]])
            assert n <= capacity
            deq = coef[:n].astype(np.int64).reshape(-1, 64) * np.repeat(qt.reshape(3, 64).astype(np.int64), _blocks(info), axis=0)
            assert deq.min(initial=0) >= -32768 and deq.max(initial=0) <= 32767, (name, pos)
            outcomes["decoded"] += 1
        else:
            assert code in [v for k, v in K.items() if not k.startswith("MMRCA_JPEG_INFO_")]
            outcomes["declined"] += 1
            if i % 10 == 0:          # the loader's fallback: whatever Pillow makes of the file (or Pillow's own error)
                path = tmp_path / f"m{i}.jpg"
                path.write_bytes(data)
                try:
                    want = pil_rgb(data)
                except Exception:
                    with pytest.raises(Exception):
                        load.load(str(path))
                else:
                    assert np.array_equal(load(load.load(str(path))).numpy(), want)
    print("200 mutations:", outcomes)
    assert outcomes["declined"] > 0 and outcomes["decoded"] > 0
    # a buffer that is too small is declined, not overrun
    data = FX["48x60_420_noise_q75_rst3"]
    code, _, _, intact = _decode_with_canary(data, parsed("48x60_420_noise_q75_rst3").ncoef - 64)
    assert code == K["MMRCA_JPEG_CAPACITY"] and intact


def _blocks(info):
    at_r, at_c = K["MMRCA_JPEG_INFO_BPR"], K["MMRCA_JPEG_INFO_BPC"]
    return [int(info[at_r + c]) * int(info[at_c + c]) for c in range(3)]


def test_collate_jpeg_round_trips_a_mixed_batch():
    names = ["17x33_420_smooth_q75", "19x23_grey_smooth_q75", "37x53_422_smooth_q75", "8x8_444_smooth_q75"]
    straggler = torch.from_numpy(pil_rgb(_png()))
    items = [J.entropy_decode(FX[names[0]]), straggler, J.entropy_decode(FX[names[1]]), J.entropy_decode(FX[names[2]]), straggler.clone(),
             J.entropy_decode(FX[names[3]])]
    batch = [({"image": {"raw_image": it, "image_path": f"p{i}"}, "text": {"original_text": "t", "tokens": torch.arange(4), "attention_mask": torch.ones(4)}}, i % 4)
             for i, it in enumerate(items)]
    data, labels = J.collate_jpeg(batch)
    raw = data["image"]["raw_image"]
    assert J.is_jpeg_batch(raw) and labels.tolist() == [0, 1, 2, 3, 0, 1] and data["text"]["tokens"].shape == (6, 4)
    assert raw["shapes"].tolist() == [[17, 33], [9, 11], [19, 23], [37, 53], [9, 11], [8, 8]]
    assert raw["jpeg_index"].tolist() == [0, 2, 3, 5] and raw["straggler_index"].tolist() == [1, 4]
    desc = raw["desc"].numpy().view(J.DESC_DTYPE)
    sizes = [(h * w * 3 + 15) // 16 * 16 for h, w in raw["shapes"].tolist()]
    offsets = np.concatenate([[0], np.cumsum(sizes)])
    J.check_descriptors(desc, raw["coef"].numel(), int(offsets[-1]))
    for d, i, name in zip(desc, raw["jpeg_index"].tolist(), names):
        p = parsed(name)
        assert d["out_offset"] == offsets[i] and (d["width"], d["height"], d["ncomp"], d["hmax"], d["vmax"]) == (p.width, p.height, p.ncomp, p.h[0], p.v[0])
        assert d["bpr"][:p.ncomp].tolist() == p.bpr and d["bpc"][:p.ncomp].tolist() == p.bpc
        assert np.array_equal(raw["coef"].numpy()[d["coef_offset"]:d["coef_offset"] + p.ncoef], p.coef)
        assert np.array_equal(d["qt"].reshape(3, 64), p.qt)
        # the round trip: the descriptor and its slice of the flat tensor decode to the file's pixels
        q = R.Parsed()
        q.width, q.height, q.ncomp, q.h, q.v = p.width, p.height, p.ncomp, p.h, p.v
        q.bpr, q.bpc, q.qt = d["bpr"][:p.ncomp].tolist(), d["bpc"][:p.ncomp].tolist(), d["qt"].reshape(3, 64)
        q.coef = raw["coef"].numpy()[d["coef_offset"]:d["coef_offset"] + p.ncoef]
        assert np.array_equal(R.planes_to_rgb(q, R.idct_planes(q)), R.decode(FX[name]))
    assert raw["straggler_shapes"].tolist() == [[9, 11], [9, 11]]
    n = 9 * 11 * 3
    assert np.array_equal(raw["straggler_flat"].numpy()[:n].reshape(9, 11, 3), straggler.numpy())
    bad = desc.copy()
    bad["coef_offset"][-1] += 64
    with pytest.raises(J.JpegError):
        J.check_descriptors(bad, raw["coef"].numel(), int(offsets[-1]))
    bad = desc.copy()
    bad["width"][0] += 16
    with pytest.raises(J.JpegError):
        J.check_descriptors(bad, raw["coef"].numel(), int(offsets[-1]))


def test_mmrca_h_abi_pins_are_unchanged():
    protos = abi.prototypes()
    lib = L.load()
    assert all(getattr(lib, name).argtypes is not None for name in protos)        # the binding is the header, function for function
    assert not any("jpeg" in name for name in protos)
    jp = abi.prototypes(J.HEADER_PATH)
    assert sorted(jp) == sorted(J.HOST_FUNCTIONS + J.DEVICE_FUNCTIONS)
    assert [n for _, n in jp["mmrca_jpeg_idct_rgb"][1]] == ["coef", "desc", "B", "out", "stream"]
    assert J.header().structs["MmrcaJpegDesc"] == [n for n in J.DESC_DTYPE.names]
