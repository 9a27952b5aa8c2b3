// Host half of the baseline-JPEG decoder (include/mmrca_jpeg.h): marker parsing and Huffman decoding of ONE interleaved SOF0 scan
// into int16 coefficients.  Plain C++ with no HIP include: libmmrca_jpeg.so is loaded by DataLoader workers that must not touch
// the GPU runtime, and links into a stand-alone program for sanitizer runs.  The bytes are untrusted: the marker parser checks every
// segment against n, the bit reader (Bits) never moves past n, every coefficient write is checked against coef_capacity, and anything this decoder does
// not handle exactly as libjpeg does is DECLINED (positive code) so that the caller falls back to its full decoder.
#include <stdint.h>
#include <string.h>
#include "../../include/mmrca_jpeg.h"

namespace {

const uint8_t ZIGZAG[64] = {0,  1,  8,  16, 9,  2,  3,  10, 17, 24, 32, 25, 18, 11, 4,  5,  12, 19, 26, 33, 40, 48,
                            41, 34, 27, 20, 13, 6,  7,  14, 21, 28, 35, 42, 49, 56, 57, 50, 43, 36, 29, 22, 15, 23,
                            30, 37, 44, 51, 58, 59, 52, 45, 38, 31, 39, 46, 53, 60, 61, 54, 47, 55, 62, 63};
const int MAX_DIM = 16384;

struct Huff {
  bool set;
  uint8_t look_len[256], look_sym[256];   // codes of up to 8 bits, indexed by the next 8 bits of the stream
  int32_t maxcode[18];                    // largest code of each length, -1 = none
  int32_t valoff[17];                     // symbol index = code + valoff[len]
  uint8_t sym[256];
};

struct Frame {
  int width, height, ncomp, restart;
  int id[3], h[3], v[3], tq[3], td[3], ta[3];
  int bpr[3], bpc[3], mcus_x, mcus_y;
  int64_t ncoef;
  bool qt_set[4];
  uint16_t qt[4][64];   // natural order
  Huff dc[4], ac[4];
  int64_t scan;         // first byte of the entropy-coded segment
};

// A canonical Huffman table from the 16 counts and the symbols of a DHT segment; false if the counts over-subscribe the code space.
bool build_huff(Huff& t, const uint8_t* counts, const uint8_t* symbols, int nsym) {
  memset(&t, 0, sizeof(t));
  memcpy(t.sym, symbols, (size_t)nsym);
  int code = 0, k = 0;
  for (int len = 1; len <= 16; ++len) {
    t.valoff[len] = k - code;
    const int cnt = counts[len - 1];
    if (code + cnt > (1 << len)) return false;
    if (len <= 8)
      for (int i = 0; i < cnt; ++i) {
        const int first = (code + i) << (8 - len);
        for (int j = 0; j < (1 << (8 - len)); ++j) {
          t.look_len[first + j] = (uint8_t)len;
          t.look_sym[first + j] = symbols[k + i];
        }
      }
    code += cnt;
    k += cnt;
    t.maxcode[len] = cnt ? code - 1 : -1;
    code <<= 1;
  }
  t.maxcode[17] = 0x7FFFFFFF;
  t.set = true;
  return true;
}

inline int be16(const uint8_t* p) { return (p[0] << 8) | p[1]; }

// Markers up to and including SOS; every table the scan names must have been defined by then.
int parse_headers(const uint8_t* p, int64_t n, Frame& f) {
  memset(&f, 0, sizeof(f));
  if (!p || n < 4 || p[0] != 0xFF || p[1] != 0xD8) return MMRCA_JPEG_NOT_JPEG;
  int64_t pos = 2;
  bool sof = false, adobe = false;
  int adobe_transform = 0;
  for (;;) {
    if (pos >= n || p[pos] != 0xFF) return MMRCA_JPEG_STREAM;
    while (pos < n && p[pos] == 0xFF) ++pos;           // fill bytes
    if (pos >= n) return MMRCA_JPEG_STREAM;
    const int m = p[pos++];
    if (m == 0x01 || m == 0x00) return MMRCA_JPEG_STREAM;
    if (m == 0xD8 || m == 0xD9 || (m >= 0xD0 && m <= 0xD7)) return MMRCA_JPEG_STREAM;   // SOI / EOI / RSTn between the headers
    if (pos + 2 > n) return MMRCA_JPEG_STREAM;
    const int len = be16(p + pos);
    if (len < 2 || pos + len > n) return MMRCA_JPEG_STREAM;
    const uint8_t* s = p + pos + 2;
    const int body = len - 2;
    if (m == 0xC0) {
      if (sof || body < 6) return MMRCA_JPEG_STREAM;
      if (s[0] != 8) return MMRCA_JPEG_PRECISION;
      f.height = be16(s + 1);
      f.width = be16(s + 3);
      f.ncomp = s[5];
      if (f.ncomp != 1 && f.ncomp != 3) return MMRCA_JPEG_COMPONENTS;
      if (body != 6 + 3 * f.ncomp) return MMRCA_JPEG_STREAM;
      if (f.width <= 0 || f.height <= 0 || f.width > MAX_DIM || f.height > MAX_DIM) return MMRCA_JPEG_SIZE;
      for (int c = 0; c < f.ncomp; ++c) {
        f.id[c] = s[6 + 3 * c];
        f.h[c] = s[7 + 3 * c] >> 4;
        f.v[c] = s[7 + 3 * c] & 15;
        f.tq[c] = s[8 + 3 * c];
        if (f.tq[c] > 3) return MMRCA_JPEG_STREAM;
      }
      sof = true;
    } else if ((m >= 0xC1 && m <= 0xCF) && m != 0xC4) {
      return MMRCA_JPEG_NOT_BASELINE;                  // every other SOFn, JPG, DAC (arithmetic conditioning)
    } else if (m == 0xDB) {
      int i = 0;
      while (i < body) {
        const int pq = s[i] >> 4, tq = s[i] & 15;
        if (pq != 0) return MMRCA_JPEG_PRECISION;
        if (tq > 3 || i + 65 > body) return MMRCA_JPEG_STREAM;
        for (int k = 0; k < 64; ++k) f.qt[tq][ZIGZAG[k]] = s[i + 1 + k];
        f.qt_set[tq] = true;
        i += 65;
      }
    } else if (m == 0xC4) {
      int i = 0;
      while (i < body) {
        if (i + 17 > body) return MMRCA_JPEG_STREAM;
        const int tc = s[i] >> 4, th = s[i] & 15;
        if (tc > 1 || th > 3) return MMRCA_JPEG_STREAM;
        int nsym = 0;
        for (int k = 0; k < 16; ++k) nsym += s[i + 1 + k];
        if (nsym > 256 || i + 17 + nsym > body) return MMRCA_JPEG_STREAM;
        if (!build_huff(tc ? f.ac[th] : f.dc[th], s + i + 1, s + i + 17, nsym)) return MMRCA_JPEG_STREAM;
        i += 17 + nsym;
      }
    } else if (m == 0xDD) {
      if (body != 2) return MMRCA_JPEG_STREAM;
      f.restart = be16(s);
    } else if (m == 0xDC) {
      return MMRCA_JPEG_DNL;
    } else if (m == 0xEE) {
      if (body >= 12 && memcmp(s, "Adobe", 5) == 0) {
        adobe = true;
        adobe_transform = s[11];
      }
    } else if (m == 0xDA) {
      if (!sof || body < 1) return MMRCA_JPEG_STREAM;
      const int ns = s[0];
      if (ns != f.ncomp) return MMRCA_JPEG_SCAN;
      if (body != 4 + 2 * ns) return MMRCA_JPEG_STREAM;
      for (int c = 0; c < ns; ++c) {
        if (s[1 + 2 * c] != f.id[c]) return MMRCA_JPEG_SCAN;
        f.td[c] = s[2 + 2 * c] >> 4;
        f.ta[c] = s[2 + 2 * c] & 15;
        if (f.td[c] > 3 || f.ta[c] > 3) return MMRCA_JPEG_STREAM;
      }
      if (s[1 + 2 * ns] != 0 || s[2 + 2 * ns] != 63 || s[3 + 2 * ns] != 0) return MMRCA_JPEG_STREAM;
      f.scan = pos + len;
      break;
    }                                                  // APPn, COM and the rest: skipped
    pos += len;
  }
  if (adobe && adobe_transform != 1) return MMRCA_JPEG_COLOUR;
  if (f.ncomp == 3 && f.id[0] == 'R' && f.id[1] == 'G' && f.id[2] == 'B') return MMRCA_JPEG_COLOUR;
  if (f.ncomp == 1) {
    if (f.h[0] != 1 || f.v[0] != 1) return MMRCA_JPEG_SAMPLING;
  } else {
    const bool luma = (f.h[0] == 1 && f.v[0] == 1) || (f.h[0] == 2 && f.v[0] == 1) || (f.h[0] == 2 && f.v[0] == 2);
    if (!luma || f.h[1] != 1 || f.v[1] != 1 || f.h[2] != 1 || f.v[2] != 1) return MMRCA_JPEG_SAMPLING;
    // libjpeg takes its "fancy" upsampler only for chroma planes more than two samples wide (jdsample.c: downsampled_width > 2)
    // and replicates samples otherwise; this decoder has the fancy rule alone, so images up to four pixels wide with halved
    // chroma are declined.  (One chroma ROW is fine: libjpeg replicates the missing neighbour rows exactly as this decoder does.)
    if (f.h[0] == 2 && (f.width + 1) / 2 <= 2) return MMRCA_JPEG_THIN_CHROMA;
  }
  f.mcus_x = (f.width + 8 * f.h[0] - 1) / (8 * f.h[0]);
  f.mcus_y = (f.height + 8 * f.v[0] - 1) / (8 * f.v[0]);
  f.ncoef = 0;
  for (int c = 0; c < f.ncomp; ++c) {
    f.bpr[c] = f.mcus_x * f.h[c];
    f.bpc[c] = f.mcus_y * f.v[c];
    f.ncoef += (int64_t)64 * f.bpr[c] * f.bpc[c];
  }
  for (int c = 0; c < f.ncomp; ++c)
    if (!f.qt_set[f.tq[c]] || !f.dc[f.td[c]].set || !f.ac[f.ta[c]].set) return MMRCA_JPEG_STREAM;
  return MMRCA_JPEG_OK;
}

// MSB-first bit reader over one entropy-coded segment.  It removes FF00 stuffing and stops in front of a marker (or the end of the
// data); asking for more bits than the segment holds is an error, never a read past n.
struct Bits {
  const uint8_t* p;
  int64_t n, pos;
  uint64_t acc;   // next bit = bit 63
  int cnt;
  bool stop;

  void fill() {
    while (cnt <= 56 && !stop) {
      if (pos >= n) { stop = true; break; }
      const uint8_t b = p[pos];
      if (b == 0xFF) {
        if (pos + 1 >= n || p[pos + 1] != 0x00) { stop = true; break; }
        pos += 2;
      } else {
        pos += 1;
      }
      acc |= (uint64_t)b << (56 - cnt);
      cnt += 8;
    }
  }
  bool get(int k, int& out) {     // 0 <= k <= 16
    if (k == 0) { out = 0; return true; }
    if (cnt < k) { fill(); if (cnt < k) return false; }
    out = (int)(acc >> (64 - k));
    acc <<= k;
    cnt -= k;
    return true;
  }
  bool decode(const Huff& t, int& sym) {
    if (cnt < 16) fill();
    const int look = (int)(acc >> 56);
    int len = t.look_len[look];
    if (len) {
      if (len > cnt) return false;
      sym = t.look_sym[look];
    } else {
      const int code16 = (int)(acc >> 48);
      for (len = 9; len <= 16; ++len)
        if (t.maxcode[len] >= 0 && (code16 >> (16 - len)) <= t.maxcode[len]) break;
      if (len > 16 || len > cnt) return false;
      const int idx = (code16 >> (16 - len)) + t.valoff[len];
      if (idx < 0 || idx > 255) return false;
      sym = t.sym[idx];
    }
    acc <<= len;
    cnt -= len;
    return true;
  }
};

inline int extend(int v, int s) { return v < (1 << (s - 1)) ? v - (1 << s) + 1 : v; }

inline bool fits(int v, int q) {
  const int d = v * q;          // |v| <= 65535 and q <= 255: no overflow
  return v >= -32768 && v <= 32767 && d >= -32768 && d <= 32767;
}

}  // namespace

extern "C" int mmrca_jpeg_probe(const void* bytes, int64_t n, int32_t* info) {
  Frame f;
  const int rc = parse_headers((const uint8_t*)bytes, n, f);
  if (rc != MMRCA_JPEG_OK || !info) return rc ? rc : MMRCA_JPEG_STREAM;
  if (f.ncoef > 0x7FFFFFFF) return MMRCA_JPEG_SIZE;
  memset(info, 0, sizeof(int32_t) * MMRCA_JPEG_INFO_LEN);
  info[MMRCA_JPEG_INFO_WIDTH] = f.width;
  info[MMRCA_JPEG_INFO_HEIGHT] = f.height;
  info[MMRCA_JPEG_INFO_NCOMP] = f.ncomp;
  for (int c = 0; c < f.ncomp; ++c) {
    info[MMRCA_JPEG_INFO_H + c] = f.h[c];
    info[MMRCA_JPEG_INFO_V + c] = f.v[c];
    info[MMRCA_JPEG_INFO_TQ + c] = f.tq[c];
    info[MMRCA_JPEG_INFO_BPR + c] = f.bpr[c];
    info[MMRCA_JPEG_INFO_BPC + c] = f.bpc[c];
  }
  info[MMRCA_JPEG_INFO_NCOEF] = (int32_t)f.ncoef;
  info[MMRCA_JPEG_INFO_RESTART] = f.restart;
  return MMRCA_JPEG_OK;
}

extern "C" int mmrca_jpeg_entropy_decode(const void* bytes, int64_t n, void* coef_out, int64_t coef_capacity, void* qtables) {
  Frame f;
  const uint8_t* p = (const uint8_t*)bytes;
  const int rc = parse_headers(p, n, f);
  if (rc != MMRCA_JPEG_OK) return rc;
  if (!coef_out || !qtables) return MMRCA_JPEG_CAPACITY;
  if (f.ncoef > coef_capacity || f.ncoef > 0x7FFFFFFF) return MMRCA_JPEG_CAPACITY;
  int16_t* coef = (int16_t*)coef_out;
  uint16_t* qout = (uint16_t*)qtables;
  memset(coef, 0, (size_t)f.ncoef * sizeof(int16_t));
  memset(qout, 0, 192 * sizeof(uint16_t));
  int64_t base[3];
  int64_t at = 0;
  for (int c = 0; c < f.ncomp; ++c) {
    memcpy(qout + 64 * c, f.qt[f.tq[c]], 64 * sizeof(uint16_t));
    base[c] = at;
    at += (int64_t)64 * f.bpr[c] * f.bpc[c];
  }
  Bits b = {p, n, f.scan, 0, 0, false};
  int pred[3] = {0, 0, 0};
  const int64_t mcus = (int64_t)f.mcus_x * f.mcus_y;
  int next_rst = 0;
  for (int64_t mcu = 0; mcu < mcus; ++mcu) {
    if (f.restart && mcu && mcu % f.restart == 0) {
      if (b.cnt >= 8) return MMRCA_JPEG_STREAM;         // whole bytes left in front of the marker
      int64_t q = b.pos;
      if (q >= n || p[q] != 0xFF) return MMRCA_JPEG_STREAM;
      while (q < n && p[q] == 0xFF) ++q;
      if (q >= n || p[q] != 0xD0 + next_rst) return MMRCA_JPEG_STREAM;
      next_rst = (next_rst + 1) & 7;
      b.pos = q + 1;
      b.acc = 0;
      b.cnt = 0;
      b.stop = false;
      pred[0] = pred[1] = pred[2] = 0;
    }
    const int mx = (int)(mcu % f.mcus_x), my = (int)(mcu / f.mcus_x);
    for (int c = 0; c < f.ncomp; ++c) {
      const Huff& dc = f.dc[f.td[c]];
      const Huff& ac = f.ac[f.ta[c]];
      const uint16_t* qt = f.qt[f.tq[c]];
      for (int by = 0; by < f.v[c]; ++by)
        for (int bx = 0; bx < f.h[c]; ++bx) {
          const int64_t blk = (int64_t)(my * f.v[c] + by) * f.bpr[c] + (mx * f.h[c] + bx);
          const int64_t o = base[c] + 64 * blk;
          if (o < 0 || o + 64 > f.ncoef || o + 64 > coef_capacity) return MMRCA_JPEG_CAPACITY;
          int16_t* blkp = coef + o;
          int s, bits;
          if (!b.decode(dc, s)) return MMRCA_JPEG_STREAM;
          if (s > 11) return MMRCA_JPEG_STREAM;
          if (!b.get(s, bits)) return MMRCA_JPEG_STREAM;
          pred[c] += s ? extend(bits, s) : 0;
          if (!fits(pred[c], qt[0])) return MMRCA_JPEG_RANGE;
          blkp[0] = (int16_t)pred[c];
          for (int k = 1; k < 64;) {
            int rs;
            if (!b.decode(ac, rs)) return MMRCA_JPEG_STREAM;
            const int r = rs >> 4;
            s = rs & 15;
            if (s == 0) {
              if (r != 15) break;                       // EOB
              k += 16;
              if (k > 64) return MMRCA_JPEG_STREAM;
              continue;
            }
            k += r;
            if (k > 63 || s > 10) return MMRCA_JPEG_STREAM;
            if (!b.get(s, bits)) return MMRCA_JPEG_STREAM;
            const int v = extend(bits, s);
            if (!fits(v, qt[ZIGZAG[k]])) return MMRCA_JPEG_RANGE;
            blkp[ZIGZAG[k]] = (int16_t)v;
            ++k;
          }
        }
    }
  }
  // the scan must be the only one: the next marker is EOI
  if (b.cnt >= 8) return MMRCA_JPEG_STREAM;
  int64_t q = b.pos;
  if (q >= n || p[q] != 0xFF) return MMRCA_JPEG_STREAM;
  while (q < n && p[q] == 0xFF) ++q;
  if (q >= n) return MMRCA_JPEG_STREAM;
  if (p[q] == 0xDC) return MMRCA_JPEG_DNL;
  if (p[q] != 0xD9) return p[q] == 0xDA || p[q] == 0xC4 || p[q] == 0xDB ? MMRCA_JPEG_SCAN : MMRCA_JPEG_STREAM;
  return MMRCA_JPEG_OK;
}
