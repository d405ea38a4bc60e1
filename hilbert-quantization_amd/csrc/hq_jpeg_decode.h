// hq_jpeg_decode.h — the per-frame logic of the grayscale baseline JPEG decoder, shared by the
// kernels of hq_jpeg_decode.hip and the stand-alone host program tools/jpeg_decode_host.cpp: marker walk, Huffman
// table build, bit reader, block decode and the 1-D pass of libjpeg's ISLOW inverse DCT.  Plain C++ over a
// (pointer, begin, end) byte range; every loop is bounded by the range or by a constant and every byte is read
// through jpd_u8, which returns 0 outside [begin, end).
#pragma once

#include <stdint.h>

#if defined(__HIPCC__)
#define JPD_HD __host__ __device__ inline
#else
#define JPD_HD inline
#endif

namespace hq {

// per-payload status (descriptor word 0, and the decode kernel's status output)
enum JpdStatus : int32_t {
  JPD_OK = 0,
  JPD_SHORT = 1,         // fewer than 4 bytes
  JPD_NO_SOI = 2,        // does not start with FF D8
  JPD_BAD_SEGMENT = 3,   // no FF xx where a marker must stand, a length below 2 or past the payload's end
  JPD_SOF_KIND = 4,      // SOF1, SOF2, ...: extended, progressive, lossless, arithmetic
  JPD_BAD_SOF = 5,       // precision != 8, components != 1, sampling != 1 x 1, a zero or > 65500 dimension, two SOFs
  JPD_BAD_DQT = 6,       // 16-bit entries, table id above 3, a segment that does not end on a table
  JPD_BAD_DHT = 7,       // class above 1, id above 3, more than 256 symbols, counts that overflow the code space,
                         // symbols past the segment, a DC symbol above 15
  JPD_RESTART = 8,       // DRI with a non-zero interval
  JPD_BAD_SOS = 9,       // not one component, Ss != 0, Se != 63, Ah Al != 0, another component id
  JPD_MISSING = 10,      // SOS before the SOF, or a table the scan selects was never defined
  JPD_NO_SOS = 11,       // the payload ends before a scan
  JPD_MARKER = 12,       // a marker the decoder does not take (EOI before the scan, DNL, DAC, RSTn, ...)
  JPD_TRUNCATED = 13,    // the scan asked for bits past the payload's end or past a marker
  JPD_CORRUPT = 14,      // a code longer than 16 bits, a coefficient index past 63, a size above 11 (DC) / 10 (AC)
  JPD_NO_EOI = 15,       // the scan is not followed by FF D9 at once
  JPD_SHAPE = 16,        // the payload's H, W are not the launch's
  JPD_RANGE = 17,        // values outside the range in which every libjpeg build computes the same pixel
  JPD_BAD_ID = 18,       // ids[] entry below 0, or offsets that do not bound a payload
};

// descriptor: JPD_DESC int32 words per payload; offsets are relative to the payload's first byte
enum { JPD_STATUS = 0, JPD_H = 1, JPD_W = 2, JPD_DQT = 3, JPD_DC = 4, JPD_AC = 5, JPD_SCAN = 6, JPD_DESC = 8 };
// JPD_DQT: the 64 entries (zigzag order); JPD_DC / JPD_AC: the 16 counts, followed by the symbols

constexpr int kJpdLutBits = 6;
constexpr int kJpdGuard = 16383;  // see jpd_idct_1d

JPD_HD int jpd_u8(const uint8_t* p, int64_t pos, int64_t end) { return pos < end ? (int)p[pos] : 0; }

// zigzag position -> natural (row-major) index
JPD_HD int jpd_zigzag(int k) {
  constexpr uint8_t zz[64] = {0,  1,  8,  16, 9,  2,  3,  10, 17, 24, 32, 25, 18, 11, 4,  5,  12, 19, 26, 33, 40, 48,
                              41, 34, 27, 20, 13, 6,  7,  14, 21, 28, 35, 42, 49, 56, 57, 50, 43, 36, 29, 22, 15, 23,
                              30, 37, 44, 51, 58, 59, 52, 45, 38, 31, 39, 46, 53, 60, 61, 54, 47, 55, 62, 63};
  return zz[k & 63];
}

// Counts at absolute position `at` (16 bytes) + symbols: 0 when libjpeg builds a decoder from them (at most 256
// symbols inside [at + 16, lim), no length whose codes reach 1 << length), else non-zero.
JPD_HD int jpd_check_counts(const uint8_t* p, int64_t at, int64_t lim, int* nsym) {
  int code = 0, total = 0;
  for (int l = 1; l <= 16; ++l) {
    const int c = jpd_u8(p, at + l - 1, lim);
    code += c;
    total += c;
    if (c && code >= (1 << l)) return 1;
    code <<= 1;
  }
  *nsym = total;
  return (total > 256 || at + 16 + total > lim) ? 1 : 0;
}

// Marker walk of payload [begin, end): fills d[JPD_DESC].  Every step moves at least 2 bytes forward.
JPD_HD void jpd_probe(const uint8_t* p, int64_t begin, int64_t end, int32_t* d) {
  for (int i = 0; i < JPD_DESC; ++i) d[i] = 0;
  int32_t dqt[4] = {0, 0, 0, 0}, dc[4] = {0, 0, 0, 0}, ac[4] = {0, 0, 0, 0};  // 0 = not defined (offset 0 is the SOI)
  int tq = -1, comp = -1;
  auto fail = [&](int s) { d[JPD_STATUS] = s; };
  if (end < begin || end - begin > (int64_t)1 << 30) return fail(JPD_BAD_ID);
  if (end - begin < 4) return fail(JPD_SHORT);
  if (p[begin] != 0xFF || p[begin + 1] != 0xD8) return fail(JPD_NO_SOI);
  int64_t pos = begin + 2;
  while (pos + 4 <= end) {
    if (p[pos] != 0xFF) return fail(JPD_BAD_SEGMENT);
    const int m = p[pos + 1];
    const int64_t len = ((int64_t)p[pos + 2] << 8) | p[pos + 3], seg = pos + 4, lim = pos + 2 + len;
    const bool sized = (m >= 0xC0 && m <= 0xCF) || (m >= 0xDA && m <= 0xFE);
    if (!sized || m == 0xDC) return fail(JPD_MARKER);  // no length (RSTn, SOI, EOI, TEM, fill) or DNL
    if (len < 2 || lim > end) return fail(JPD_BAD_SEGMENT);
    if (m == 0xDB) {  // DQT: (Pq Tq, 64 entries) repeated
      int64_t q = seg;
      while (q < lim) {
        const int b = p[q];
        if ((b >> 4) != 0 || (b & 15) > 3 || q + 65 > lim) return fail(JPD_BAD_DQT);
        dqt[b & 15] = (int32_t)(q + 1 - begin);
        q += 65;
      }
    } else if (m == 0xC4) {  // DHT: (Tc Th, 16 counts, symbols) repeated
      int64_t q = seg;
      while (q < lim) {
        const int b = p[q];
        int nsym = 0;
        if ((b >> 4) > 1 || (b & 15) > 3 || q + 17 > lim || jpd_check_counts(p, q + 1, lim, &nsym))
          return fail(JPD_BAD_DHT);
        ((b >> 4) ? ac : dc)[b & 15] = (int32_t)(q + 1 - begin);
        q += 17 + nsym;
      }
    } else if (m == 0xC0) {  // SOF0
      if (d[JPD_H] || len != 11 || p[seg] != 8 || p[seg + 5] != 1 || p[seg + 7] != 0x11 || p[seg + 8] > 3)
        return fail(JPD_BAD_SOF);
      const int H = (p[seg + 1] << 8) | p[seg + 2], W = (p[seg + 3] << 8) | p[seg + 4];
      if (H < 1 || W < 1 || H > 65500 || W > 65500) return fail(JPD_BAD_SOF);
      d[JPD_H] = H;
      d[JPD_W] = W;
      comp = p[seg + 6];
      tq = p[seg + 8];
    } else if (m == 0xDD) {  // DRI
      if (len != 4) return fail(JPD_BAD_SEGMENT);
      if (p[seg] | p[seg + 1]) return fail(JPD_RESTART);
    } else if (m == 0xDA) {  // SOS: the walk ends here
      if (!d[JPD_H]) return fail(JPD_MISSING);
      if (len != 8 || p[seg] != 1 || p[seg + 1] != comp || p[seg + 3] != 0 || p[seg + 4] != 63 || p[seg + 5] != 0)
        return fail(JPD_BAD_SOS);
      const int td = p[seg + 2] >> 4, ta = p[seg + 2] & 15;
      if (td > 3 || ta > 3) return fail(JPD_BAD_SOS);
      if (!dqt[tq] || !dc[td] || !ac[ta]) return fail(JPD_MISSING);
      int ndc = 0;
      for (int l = 0; l < 16; ++l) ndc += p[begin + dc[td] + l];
      for (int i = 0; i < ndc; ++i)
        if (p[begin + dc[td] + 16 + i] > 15) return fail(JPD_BAD_DHT);
      d[JPD_DQT] = dqt[tq];
      d[JPD_DC] = dc[td];
      d[JPD_AC] = ac[ta];
      d[JPD_SCAN] = (int32_t)(lim - begin);
      return;
    } else if (m >= 0xC0 && m <= 0xCF && m != 0xC8 && m != 0xCC) {
      return fail(JPD_SOF_KIND);
    } else if (m == 0xCC || m == 0xC8 || (m >= 0xDE && m <= 0xDF) || (m >= 0xF0 && m <= 0xFD)) {
      return fail(JPD_MARKER);  // DAC, JPG, DHP, EXP, JPGn
    }  // else APPn, COM: skipped by length
    pos = lim;
  }
  fail(JPD_NO_SOS);
}

// Canonical Huffman decoder of one table.  A 16-bit window `peek` of the stream has a code of length l when
// peek < limit[l - 1] for the first time (limit = the left-aligned code after the last of that length, which the
// count check keeps below 1 << 16); its symbol is number first[l - 1] + ((peek - base[l - 1]) >> (16 - l)).
// lut[peek >> (16 - kJpdLutBits)] = length << 8 | symbol for the codes of at most kJpdLutBits bits, else 0.
struct JpdTable {
  uint16_t limit[16], base[16], first[16];
  uint16_t lut[1 << kJpdLutBits];
};

// Builds t from the counts at absolute position `at`; false (and a table that matches nothing) when the counts are
// not a code libjpeg takes or do not lie inside [begin, end).
JPD_HD bool jpd_build_table(const uint8_t* p, int64_t at, int64_t begin, int64_t end, JpdTable& t) {
  for (int l = 0; l < 16; ++l) t.limit[l] = t.base[l] = t.first[l] = 0;
  for (int i = 0; i < (1 << kJpdLutBits); ++i) t.lut[i] = 0;
  int nsym = 0;
  if (at < begin || at + 16 > end || jpd_check_counts(p, at, end, &nsym)) return false;
  int code = 0, k = 0;
  for (int l = 1; l <= 16; ++l) {
    const int c = jpd_u8(p, at + l - 1, end);
    t.base[l - 1] = (uint16_t)(code << (16 - l));
    t.first[l - 1] = (uint16_t)k;
    if (l <= kJpdLutBits)
      for (int i = 0; i < c; ++i) {
        const int sym = jpd_u8(p, at + 16 + k + i, end), lo = (code + i) << (kJpdLutBits - l);
        for (int j = 0; j < (1 << (kJpdLutBits - l)); ++j) t.lut[lo + j] = (uint16_t)((l << 8) | sym);
      }
    code += c;
    k += c;
    t.limit[l - 1] = (uint16_t)(code << (16 - l));
    code <<= 1;
  }
  return true;
}

// MSB-first bit reader over the scan: 64-bit buffer, left-aligned, `n` real bits in it, zeros below them.  Refilled
// bytewise; FF 00 is the data byte FF, FF followed by anything else (or by the end) is a marker: the reader stops
// there for good (pos stays on the FF) and supplies zero bits.  Taking more bits than are real sets `truncated`.
struct JpdBits {
  uint64_t buf;
  int64_t pos, end;
  int n;
  bool stopped, truncated;
};

JPD_HD void jpd_bits_init(JpdBits& b, int64_t pos, int64_t end) {
  b.buf = 0;
  b.pos = pos;
  b.end = end;
  b.n = 0;
  b.stopped = pos >= end;
  b.truncated = false;
}

JPD_HD void jpd_refill(JpdBits& b, const uint8_t* p) {
  while (b.n <= 56 && !b.stopped) {  // at most 8 rounds
    const int c = jpd_u8(p, b.pos, b.end);
    if (b.pos >= b.end || (c == 0xFF && jpd_u8(p, b.pos + 1, b.end) != 0)) {
      b.stopped = true;
      break;
    }
    b.pos += c == 0xFF ? 2 : 1;
    b.buf |= (uint64_t)c << (56 - b.n);
    b.n += 8;
  }
}

JPD_HD void jpd_skip(JpdBits& b, int k) {  // 1 <= k <= 16
  if (k > b.n) {
    b.truncated = true;
    b.buf = 0;
    b.n = 0;
  } else {
    b.buf <<= k;
    b.n -= k;
  }
}

// next symbol of table t (symbols at absolute position `sym`), or -1 when no code of up to 16 bits matches
JPD_HD int jpd_symbol(JpdBits& b, const uint8_t* p, const JpdTable& t, int64_t sym) {
  const uint32_t peek = (uint32_t)(b.buf >> 48);
  const uint32_t e = t.lut[peek >> (16 - kJpdLutBits)];
  if (e) {
    jpd_skip(b, (int)(e >> 8));
    return (int)(e & 255u);
  }
  for (int l = kJpdLutBits + 1; l <= 16; ++l)
    if (peek < t.limit[l - 1]) {
      jpd_skip(b, l);
      return jpd_u8(p, sym + t.first[l - 1] + ((peek - t.base[l - 1]) >> (16 - l)), b.end);
    }
  return -1;
}

// s magnitude bits (1 <= s <= 11) as a signed value: T.81 F.2.2.1 EXTEND
JPD_HD int jpd_receive_extend(JpdBits& b, int s) {
  const int v = (int)(b.buf >> (64 - s));
  jpd_skip(b, s);
  return v < (1 << (s - 1)) ? v - (1 << s) + 1 : v;
}

// One 8 x 8 block: DC difference + prediction, AC (run, size) symbols, ZRL, EOB.  Writes the non-zero coefficients
// into the zeroed natural-order tile; at most 64 symbols.  False = corrupt (the block ends there).
JPD_HD bool jpd_block(JpdBits& b, const uint8_t* p, const JpdTable& dc, int64_t dcsym, const JpdTable& ac,
                      int64_t acsym, int& pred, int16_t* tile) {
  jpd_refill(b, p);
  int s = jpd_symbol(b, p, dc, dcsym);
  if (s < 0 || s > 11) return false;
  if (s) pred += jpd_receive_extend(b, s);
  tile[0] = (int16_t)pred;
  for (int k = 1; k < 64;) {
    jpd_refill(b, p);  // a symbol takes at most 16 + 10 of the >= 57 bits (or the reader has stopped)
    const int rs = jpd_symbol(b, p, ac, acsym);
    if (rs < 0) return false;
    s = rs & 15;
    if (s == 0) {
      if ((rs >> 4) != 15) break;  // EOB
      k += 16;                     // ZRL
      continue;
    }
    k += rs >> 4;
    if (s > 10 || k > 63) return false;
    tile[jpd_zigzag(k)] = (int16_t)jpd_receive_extend(b, s);
    ++k;
  }
  return true;
}

// The scan must end on a byte boundary followed at once by FF D9 (b.n < 8: only pad bits are left).
JPD_HD bool jpd_at_eoi(const JpdBits& b, const uint8_t* p) {
  return b.n < 8 && b.pos + 2 <= b.end && p[b.pos] == 0xFF && p[b.pos + 1] == 0xD9;
}

// One 1-D pass of libjpeg's jidctint.c (ISLOW, CONST_BITS = 13, PASS1_BITS = 2): out = (A x + round) >> shift with
// shift = 11 (pass 1, columns) or 18 (pass 2, rows).  The caller guarantees |x[i]| <= kJpdGuard = 16383.  Then 32-bit
// arithmetic is exact: every intermediate is a linear form of x whose absolute coefficients sum to at most 8192 +
// 7 * 11363 = 87733, so its magnitude stays below 87733 * 16383 + 2^17 < 2^31; no 64-bit operation is needed.  The
// same bound keeps every 16-bit sum and every 32-bit accumulator of libjpeg-turbo's SIMD forms from wrapping, so
// they, the C form (64-bit) and this one agree.
JPD_HD void jpd_idct_1d(const int32_t* x, int32_t* out, int shift) {
  int32_t z1 = (x[2] + x[6]) * 4433;
  const int32_t e2 = z1 - x[6] * 15137, e3 = z1 + x[2] * 6270;
  const int32_t e0 = (x[0] + x[4]) * 8192, e1 = (x[0] - x[4]) * 8192;
  const int32_t t10 = e0 + e3, t13 = e0 - e3, t11 = e1 + e2, t12 = e1 - e2;
  int32_t t0 = x[7], t1 = x[5], t2 = x[3], t3 = x[1];
  z1 = t0 + t3;
  int32_t z2 = t1 + t2, z3 = t0 + t2, z4 = t1 + t3;
  const int32_t z5 = (z3 + z4) * 9633;
  t0 *= 2446;
  t1 *= 16819;
  t2 *= 25172;
  t3 *= 12299;
  z1 *= -7373;
  z2 *= -20995;
  z3 = z3 * -16069 + z5;
  z4 = z4 * -3196 + z5;
  t0 += z1 + z3;
  t1 += z2 + z4;
  t2 += z2 + z3;
  t3 += z1 + z4;
  const int32_t r = 1 << (shift - 1);
  out[0] = (t10 + t3 + r) >> shift;
  out[7] = (t10 - t3 + r) >> shift;
  out[1] = (t11 + t2 + r) >> shift;
  out[6] = (t11 - t2 + r) >> shift;
  out[2] = (t12 + t1 + r) >> shift;
  out[5] = (t12 - t1 + r) >> shift;
  out[3] = (t13 + t0 + r) >> shift;
  out[4] = (t13 - t0 + r) >> shift;
}

// |v| <= kJpdGuard, else 0 and *bad is set
JPD_HD int32_t jpd_guard(int32_t v, bool* bad) {
  if (v > kJpdGuard || v < -kJpdGuard) {
    *bad = true;
    return 0;
  }
  return v;
}

// libjpeg's range-limit table: index (v + 128) & 1023.  Outside -512 <= v <= 511 the table wraps where the SIMD
// forms saturate: *bad is set.
JPD_HD uint8_t jpd_range_limit(int32_t v, bool* bad) {
  if (v < -512 || v > 511) *bad = true;
  const int i = (v + 128) & 1023;
  return (uint8_t)(i < 256 ? i : (i < 640 ? 255 : 0));
}

}  // namespace hq
