"""NumPy mirror of the baseline-JPEG decoder (include/mmrca_jpeg.h): a table-driven Huffman decoder and the integer arithmetic of
csrc/jpeg.hip in int64 -- "islow" inverse DCT, "fancy" edge-replicated chroma upsampling, 16-bit fixed-point YCbCr -> RGB.
Test code only: slow, and it assumes a well-formed file (the C decoder is the one that faces untrusted bytes).

Also the fixtures shared by tests/test_jpeg_cpu.py and tests/test_jpeg_gpu.py (``fixtures()``: JPEG byte streams encoded with
Pillow) and the writer of tests/golden/jpeg_goldens.npz (``python tests/jpeg_ref.py``)."""
import io
import os

import numpy as np

ZIGZAG = np.array([0, 1, 8, 16, 9, 2, 3, 10, 17, 24, 32, 25, 18, 11, 4, 5, 12, 19, 26, 33, 40, 48, 41, 34, 27, 20, 13, 6, 7, 14, 21, 28,
                   35, 42, 49, 56, 57, 50, 43, 36, 29, 22, 15, 23, 30, 37, 44, 51, 58, 59, 52, 45, 38, 31, 39, 46, 53, 60, 61, 54, 47, 55,
                   62, 63])
GOLDEN_PATH = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "jpeg_goldens.npz")


class Parsed:
    """width, height, ncomp, h/v/tq per component, bpr/bpc (blocks per row / column, whole MCUs), ncoef, restart,
    coef (int16, the C decoder's layout), qt (uint16 [3, 64], natural order, per component)"""


def _huff_table(counts, symbols):
    table, code, k = {}, 0, 0
    for length in range(1, 17):
        for _ in range(counts[length - 1]):
            table[(length, code)] = symbols[k]
            code += 1
            k += 1
        code <<= 1
    return table


class _Bits:
    def __init__(self, data, pos):
        self.d, self.pos, self.acc, self.cnt = data, pos, 0, 0

    def bit(self):
        if self.cnt == 0:
            b = self.d[self.pos]
            self.pos += 1
            if b == 0xFF:
                assert self.d[self.pos] == 0x00, "marker inside the entropy-coded segment"
                self.pos += 1
            self.acc, self.cnt = b, 8
        self.cnt -= 1
        return (self.acc >> self.cnt) & 1

    def bits(self, n):
        v = 0
        for _ in range(n):
            v = (v << 1) | self.bit()
        return v

    def symbol(self, table):
        code = 0
        for length in range(1, 17):
            code = (code << 1) | self.bit()
            if (length, code) in table:
                return table[(length, code)]
        raise ValueError("undefined Huffman code")

    def restart(self, k):
        self.cnt = 0
        while self.d[self.pos] == 0xFF and self.d[self.pos + 1] == 0xFF:
            self.pos += 1
        assert self.d[self.pos] == 0xFF and self.d[self.pos + 1] == 0xD0 + k, "restart marker missing or out of order"
        self.pos += 2


def _extend(v, s):
    return v - (1 << s) + 1 if v < (1 << (s - 1)) else v


def parse(data: bytes) -> Parsed:
    """markers + the entropy-coded scan -> coefficients in the layout of mmrca_jpeg_entropy_decode"""
    d = bytes(data)
    assert d[:2] == b"\xff\xd8"
    p = Parsed()
    qts, huff, p.restart = {}, {}, 0
    pos = 2
    while True:
        assert d[pos] == 0xFF
        while d[pos] == 0xFF:
            pos += 1
        m = d[pos]
        pos += 1
        length = (d[pos] << 8) | d[pos + 1]
        s = d[pos + 2:pos + length]
        if m == 0xC0:
            assert s[0] == 8
            p.height, p.width, p.ncomp = (s[1] << 8) | s[2], (s[3] << 8) | s[4], s[5]
            p.h = [s[7 + 3 * c] >> 4 for c in range(p.ncomp)]
            p.v = [s[7 + 3 * c] & 15 for c in range(p.ncomp)]
            p.tq = [s[8 + 3 * c] for c in range(p.ncomp)]
        elif m == 0xDB:
            for i in range(0, len(s), 65):
                assert s[i] >> 4 == 0
                q = np.zeros(64, dtype=np.uint16)
                q[ZIGZAG] = np.frombuffer(s[i + 1:i + 65], dtype=np.uint8)
                qts[s[i] & 15] = q
        elif m == 0xC4:
            i = 0
            while i < len(s):
                counts = list(s[i + 1:i + 17])
                n = sum(counts)
                huff[(s[i] >> 4, s[i] & 15)] = _huff_table(counts, list(s[i + 17:i + 17 + n]))
                i += 17 + n
        elif m == 0xDD:
            p.restart = (s[0] << 8) | s[1]
        elif m == 0xDA:
            assert s[0] == p.ncomp
            td = [s[2 + 2 * c] >> 4 for c in range(p.ncomp)]
            ta = [s[2 + 2 * c] & 15 for c in range(p.ncomp)]
            pos += length
            break
        else:
            assert m not in (0xC1, 0xC2, 0xC3, 0xC5, 0xC6, 0xC7, 0xC9, 0xCA, 0xCB, 0xCD, 0xCE, 0xCF), "not a baseline file"
        pos += length
    mx = -(-p.width // (8 * p.h[0]))
    my = -(-p.height // (8 * p.v[0]))
    p.bpr = [mx * p.h[c] for c in range(p.ncomp)]
    p.bpc = [my * p.v[c] for c in range(p.ncomp)]
    p.ncoef = 64 * sum(a * b for a, b in zip(p.bpr, p.bpc))
    p.qt = np.zeros((3, 64), dtype=np.uint16)
    for c in range(p.ncomp):
        p.qt[c] = qts[p.tq[c]]
    coef = np.zeros(p.ncoef, dtype=np.int64)
    base = np.concatenate([[0], np.cumsum([64 * a * b for a, b in zip(p.bpr, p.bpc)])])
    bits, pred, rst = _Bits(d, pos), [0] * p.ncomp, 0
    for mcu in range(mx * my):
        if p.restart and mcu and mcu % p.restart == 0:
            bits.restart(rst)
            rst, pred = (rst + 1) & 7, [0] * p.ncomp
        for c in range(p.ncomp):
            for by in range(p.v[c]):
                for bx in range(p.h[c]):
                    blk = ((mcu // mx) * p.v[c] + by) * p.bpr[c] + (mcu % mx) * p.h[c] + bx
                    o = int(base[c]) + 64 * blk
                    s_ = bits.symbol(huff[(0, td[c])])
                    pred[c] += _extend(bits.bits(s_), s_) if s_ else 0
                    coef[o] = pred[c]
                    k = 1
                    while k < 64:
                        rs = bits.symbol(huff[(1, ta[c])])
                        r, s_ = rs >> 4, rs & 15
                        if s_ == 0:
                            if r != 15:
                                break
                            k += 16
                            continue
                        k += r
                        coef[o + ZIGZAG[k]] = _extend(bits.bits(s_), s_)
                        k += 1
    assert np.abs(coef).max(initial=0) < 32768
    p.coef = coef.astype(np.int16)
    return p


A_, B_, C_, D_, E_, F_, G_, H_, I_, J_, K_, L_ = 2446, 3196, 4433, 6270, 7373, 9633, 12299, 15137, 16069, 16819, 20995, 25172


def _idct_1d(v, n):
    """v: int64 [..., 8] -> the 1-D step along the last axis with the final descale D(x, n)"""
    v0, v1, v2, v3, v4, v5, v6, v7 = (v[..., i] for i in range(8))
    z1 = (v2 + v6) * C_
    t2 = z1 - v6 * H_
    t3 = z1 + v2 * D_
    t0 = (v0 + v4) << 13
    t1 = (v0 - v4) << 13
    t10, t13, t11, t12 = t0 + t3, t0 - t3, t1 + t2, t1 - t2
    t0, t1, t2, t3 = v7, v5, v3, v1
    z1, z2, z3, z4 = t0 + t3, t1 + t2, t0 + t2, t1 + t3
    z5 = (z3 + z4) * F_
    t0, t1, t2, t3 = t0 * A_, t1 * J_, t2 * L_, t3 * G_
    z1, z2, z3, z4 = z1 * -E_, z2 * -K_, z3 * -I_ + z5, z4 * -B_ + z5
    t0, t1, t2, t3 = t0 + z1 + z3, t1 + z2 + z4, t2 + z2 + z3, t3 + z1 + z4
    out = np.stack([t10 + t3, t11 + t2, t12 + t1, t13 + t0, t13 - t0, t12 - t1, t11 - t2, t10 - t3], axis=-1)
    return (out + (1 << (n - 1))) >> n


def idct_planes(p: Parsed):
    """one uint8-valued int64 plane [8*bpc, 8*bpr] per component"""
    planes, at = [], 0
    for c in range(p.ncomp):
        nb = p.bpr[c] * p.bpc[c]
        blk = p.coef[at:at + 64 * nb].astype(np.int64).reshape(nb, 8, 8) * p.qt[c].astype(np.int64).reshape(1, 8, 8)
        at += 64 * nb
        ws = _idct_1d(blk.transpose(0, 2, 1), 11).transpose(0, 2, 1)          # down each column
        px = np.clip(_idct_1d(ws, 18) + 128, 0, 255)                          # along each row
        planes.append(px.reshape(p.bpc[c], p.bpr[c], 8, 8).transpose(0, 2, 1, 3).reshape(8 * p.bpc[c], 8 * p.bpr[c]))
    return planes


def _up_h2v1(p):
    n = p.shape[1]
    left = np.concatenate([p[:, :1], p[:, :-1]], axis=1)
    right = np.concatenate([p[:, 1:], p[:, -1:]], axis=1)
    out = np.empty((p.shape[0], 2 * n), dtype=np.int64)
    out[:, 0::2] = (3 * p + left + 1) >> 2
    out[:, 1::2] = (3 * p + right + 2) >> 2
    out[:, 0], out[:, -1] = p[:, 0], p[:, -1]
    return out


def _up_h2v2(p):
    dh, n = p.shape
    out = np.empty((2 * dh, 2 * n), dtype=np.int64)
    for parity in (0, 1):
        nb = np.clip(np.arange(dh) + (1 if parity else -1), 0, dh - 1)
        s = 3 * p + p[nb]
        left = np.concatenate([s[:, :1], s[:, :-1]], axis=1)
        right = np.concatenate([s[:, 1:], s[:, -1:]], axis=1)
        row = np.empty((dh, 2 * n), dtype=np.int64)
        row[:, 0::2] = (3 * s + left + 8) >> 4
        row[:, 1::2] = (3 * s + right + 7) >> 4
        row[:, 0], row[:, -1] = (4 * s[:, 0] + 8) >> 4, (4 * s[:, -1] + 7) >> 4
        out[parity::2] = row
    return out


def planes_to_rgb(p: Parsed, planes) -> np.ndarray:
    H, W = p.height, p.width
    y = planes[0][:H, :W]
    if p.ncomp == 1:
        return np.repeat(y[:, :, None], 3, axis=2).astype(np.uint8)
    hmax, vmax = p.h[0], p.v[0]
    dw, dh = -(-W // hmax), -(-H // vmax)
    ch = []
    for c in (1, 2):
        q = planes[c][:dh, :dw]
        if (hmax, vmax) == (2, 1):
            q = _up_h2v1(q)
        elif (hmax, vmax) == (2, 2):
            q = _up_h2v2(q)
        ch.append(q[:H, :W] - 128)
    cb, cr = ch
    r = y + ((91881 * cr + 32768) >> 16)
    b = y + ((116130 * cb + 32768) >> 16)
    g = y + ((-22554 * cb - 46802 * cr + 32768) >> 16)
    return np.clip(np.stack([r, g, b], axis=2), 0, 255).astype(np.uint8)


def decode(data: bytes) -> np.ndarray:
    p = parse(data)
    return planes_to_rgb(p, idct_planes(p))


# ---------------------------------------------------------------------------------------------------------------- fixtures

SIZES = [(1, 1), (7, 9), (8, 8), (16, 16), (17, 33), (37, 53), (48, 60), (2, 35)]          # (H, W)
SUBSAMPLINGS = {"444": 0, "422": 1, "420": 2}                                               # Pillow's subsampling= values


def declined_by_rule(w, sub):
    """csrc/jpeg_entropy.cpp declines halved chroma planes at most two samples wide (libjpeg does not upsample those 'fancy')"""
    return sub in ("422", "420") and (w + 1) // 2 <= 2


def image(h, w, kind, seed=0):
    rng = np.random.default_rng(seed * 1000 + h * 37 + w)
    if kind == "noise":
        return rng.integers(0, 256, (h, w, 3), dtype=np.uint8)
    if kind == "flat":
        return np.full((h, w, 3), (200, 60, 120), dtype=np.uint8)
    yy, xx = np.mgrid[0:h, 0:w].astype(np.float64)
    base = np.stack([128 + 100 * np.sin(xx / 7.0 + yy / 11.0), 128 + 90 * np.cos(yy / 5.0), 40 + 3.0 * xx + 1.5 * yy], axis=2)
    return np.clip(base + rng.normal(0, 4, (h, w, 3)), 0, 255).astype(np.uint8)


def encode(arr, quality=75, sub="420", restart=0, grey=False, **kw):
    from PIL import Image
    im = Image.fromarray(arr)
    if grey:
        im = im.convert("L")
    else:
        kw["subsampling"] = SUBSAMPLINGS[sub]
    if restart:
        kw["restart_marker_blocks"] = restart
    buf = io.BytesIO()
    im.save(buf, format="JPEG", quality=quality, **kw)
    return buf.getvalue()


_fixtures = None


def fixtures():
    """name -> JPEG bytes: every size x subsampling (smooth content, quality 75), then noise, the other qualities, restart
    markers and the greyscale file on a few sizes.  Encoded once per process."""
    global _fixtures
    if _fixtures is None:
        fx = {}
        for h, w in SIZES:
            for sub in SUBSAMPLINGS:
                fx[f"{h}x{w}_{sub}_smooth_q75"] = encode(image(h, w, "smooth"), 75, sub)
        for h, w in [(17, 33), (48, 60), (7, 9)]:
            for sub in SUBSAMPLINGS:
                fx[f"{h}x{w}_{sub}_noise_q75"] = encode(image(h, w, "noise"), 75, sub)
        for q in (30, 95, 100):
            for sub in SUBSAMPLINGS:
                fx[f"37x53_{sub}_smooth_q{q}"] = encode(image(37, 53, "smooth"), q, sub)
                fx[f"48x60_{sub}_noise_q{q}"] = encode(image(48, 60, "noise"), q, sub)
        for h, w in [(16, 16), (37, 53), (48, 60)]:
            for sub in SUBSAMPLINGS:
                fx[f"{h}x{w}_{sub}_smooth_q75_rst1"] = encode(image(h, w, "smooth"), 75, sub, restart=1)
        fx["48x60_420_noise_q75_rst3"] = encode(image(48, 60, "noise"), 75, "420", restart=3)
        fx["19x23_grey_smooth_q75"] = encode(image(19, 23, "smooth"), 75, grey=True)
        fx["24x24_420_flat_q75"] = encode(image(24, 24, "flat"), 75, "420")
        _fixtures = fx
    return _fixtures


def fixture_width_sub(name):
    size, sub = name.split("_")[:2]
    return int(size.split("x")[1]), sub


GOLDEN_NAMES = ["1x1_444_smooth_q75", "7x9_422_smooth_q75", "8x8_444_smooth_q75", "16x16_420_smooth_q75_rst1", "17x33_420_smooth_q75",
                "37x53_422_smooth_q75", "2x35_420_smooth_q75", "48x60_420_noise_q30", "37x53_444_smooth_q100", "19x23_grey_smooth_q75",
                "24x24_420_flat_q75", "48x60_420_noise_q75_rst3"]


def write_goldens(path=GOLDEN_PATH):
    """the byte streams of GOLDEN_NAMES and Pillow's RGB output for each (a libjpeg-turbo build of Pillow)"""
    from PIL import Image, features
    assert features.check_feature("libjpeg_turbo"), "the goldens record libjpeg-turbo's output"
    out = {}
    for name in GOLDEN_NAMES:
        data = fixtures()[name]
        out["jpeg/" + name] = np.frombuffer(data, dtype=np.uint8)
        out["rgb/" + name] = np.asarray(Image.open(io.BytesIO(data)).convert("RGB"))
    np.savez_compressed(path, **out)


if __name__ == "__main__":
    write_goldens()
    print("wrote", GOLDEN_PATH, os.path.getsize(GOLDEN_PATH), "bytes")
