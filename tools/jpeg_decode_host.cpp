// jpeg_decode_host.cpp — the device JPEG decoder's per-frame logic (csrc/hq_jpeg_decode.h) on the CPU, one payload
// after the other, with the same steps as k_jpeg_decode: table build, block decode, two ISLOW passes, range limit,
// acceptance.  A stand-alone program, so the logic can run under the host compiler's sanitizers:
//   c++ -std=c++17 -O1 -g -fsanitize=address,undefined -fno-sanitize-recover=all tools/jpeg_decode_host.cpp -o jdh
//   jdh payloads.bin offsets.bin out.bin
// payloads.bin: the payloads back to back; offsets.bin: N + 1 int64; out.bin: per payload int32 status, H, W and,
// when the status is 0, its H x W bytes.  Every payload is decoded at the H, W of its own header.
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>

#include <vector>

#include "../hilbert-quantization_amd/csrc/hq_jpeg_decode.h"

using namespace hq;

static const int kMaxW = 224;           // the device's width cap
static const int64_t kMaxPixels = 1 << 24;

static std::vector<uint8_t> read_file(const char* path) {
  std::vector<uint8_t> v;
  FILE* f = fopen(path, "rb");
  if (!f) {
    fprintf(stderr, "cannot open %s\n", path);
    exit(2);
  }
  uint8_t buf[1 << 16];
  size_t n;
  while ((n = fread(buf, 1, sizeof(buf), f)) > 0) v.insert(v.end(), buf, buf + n);
  fclose(f);
  return v;
}

// one payload; `out` receives H x W bytes when the result is JPD_OK
static int decode(const uint8_t* p, int64_t begin, int64_t end, int32_t* d, std::vector<uint8_t>& out) {
  jpd_probe(p, begin, end, d);
  if (d[JPD_STATUS] != JPD_OK) return d[JPD_STATUS];
  const int H = d[JPD_H], W = d[JPD_W], bw = (W + 7) / 8, bh = (H + 7) / 8;
  if (W > kMaxW || (int64_t)H * W > kMaxPixels) return JPD_SHAPE;
  JpdTable dc, ac;
  bool corrupt = !jpd_build_table(p, begin + d[JPD_DC], begin, end, dc);
  corrupt |= !jpd_build_table(p, begin + d[JPD_AC], begin, end, ac);
  int32_t quant[64];
  for (int k = 0; k < 64; ++k) quant[jpd_zigzag(k)] = jpd_u8(p, begin + d[JPD_DQT] + k, end);
  JpdBits br;
  jpd_bits_init(br, begin + d[JPD_SCAN], end);
  const int64_t dcsym = begin + d[JPD_DC] + 16, acsym = begin + d[JPD_AC] + 16;
  int pred = 0;
  bool range = false;
  out.assign((size_t)H * W, 0);
  for (int by = 0; by < bh; ++by)
    for (int bx = 0; bx < bw; ++bx) {
      int16_t tile[64] = {0};
      corrupt |= !jpd_block(br, p, dc, dcsym, ac, acsym, pred, tile);
      int32_t ws[64];
      for (int c = 0; c < 8; ++c) {
        int32_t x[8], y[8];
        for (int r = 0; r < 8; ++r) x[r] = jpd_guard((int32_t)tile[8 * r + c] * quant[8 * r + c], &range);
        jpd_idct_1d(x, y, 11);
        for (int r = 0; r < 8; ++r) ws[8 * r + c] = jpd_guard(y[r], &range);
      }
      for (int r = 0; r < 8; ++r) {
        int32_t y[8];
        jpd_idct_1d(ws + 8 * r, y, 18);
        for (int c = 0; c < 8; ++c) {
          const uint8_t px = jpd_range_limit(y[c], &range);
          if (8 * by + r < H && 8 * bx + c < W) out[(size_t)(8 * by + r) * W + 8 * bx + c] = px;
        }
      }
    }
  if (corrupt) return JPD_CORRUPT;
  if (br.truncated) return JPD_TRUNCATED;
  if (range) return JPD_RANGE;
  return jpd_at_eoi(br, p) ? JPD_OK : JPD_NO_EOI;
}

int main(int argc, char** argv) {
  if (argc != 4) {
    fprintf(stderr, "usage: %s payloads.bin offsets.bin out.bin\n", argv[0]);
    return 2;
  }
  // exact-size heap copies: a read one byte outside a payload buffer is a sanitizer report
  const std::vector<uint8_t> payload = read_file(argv[1]), ob = read_file(argv[2]);
  const int64_t N = (int64_t)(ob.size() / 8) - 1;
  const int64_t* offsets = reinterpret_cast<const int64_t*>(ob.data());
  FILE* f = fopen(argv[3], "wb");
  if (!f || N < 0) return 2;
  int64_t accepted = 0;
  std::vector<uint8_t> out;
  for (int64_t i = 0; i < N; ++i) {
    if (offsets[i] < 0 || offsets[i + 1] < offsets[i] || offsets[i + 1] > (int64_t)payload.size()) return 2;
    // the payload alone in a buffer of its own length
    const std::vector<uint8_t> one(payload.begin() + offsets[i], payload.begin() + offsets[i + 1]);
    int32_t d[JPD_DESC];
    const int32_t st = decode(one.data(), 0, (int64_t)one.size(), d, out);
    const int32_t head[3] = {st, d[JPD_H], d[JPD_W]};
    fwrite(head, 4, 3, f);
    if (st == JPD_OK) {
      fwrite(out.data(), 1, out.size(), f);
      ++accepted;
    }
  }
  fclose(f);
  printf("%lld payloads, %lld accepted\n", (long long)N, (long long)accepted);
  return 0;
}
