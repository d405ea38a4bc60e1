// hq_jpeg.hip — batched grayscale baseline JPEG encoder on the device.
//
// Replaces the host JPEG stage of the batched ingest (core/compressor.py:71-80 of the reference: PIL on a thread
// pool) for callers that ask for it.  One payload per u8 frame [H, W]: SOI, DQT (libjpeg's quality scaling of the
// Annex K luminance table), SOF0, the two Annex K luminance DHT segments, SOS, one scan without restart markers,
// EOI.  Byte-exactness with libjpeg is not a goal: the payload is a valid baseline JPEG that
// any decoder turns back into the frame with the usual loss.
//
// One 256-thread workgroup encodes one frame; the dynamic LDS is sized by the frame, so small frames (33 x 32:
// 9 KB) share a CU many workgroups at a time without coupling their barriers.  Stages, all inside k_jpeg:
//   1. the frame's bytes go to LDS as 16-byte loads (from the 16-byte boundary below the frame's first byte);
//   2. DCT + quantise: the 2-D DCT of a block is K [64 x 64] . x [64], K = C (x) C with its rows already in zigzag
//      order, so a frame is one [64 x 64] . [64 x blocks] product on v_mfma_f32_16x16x4_f32.  A wave owns tile
//      columns (16 blocks) and all four tile rows: K lives in 64 VGPRs per lane (loaded once, coalesced, from a
//      table laid out in operand order at compile time), every pixel is read and converted once, 64 MFMAs per
//      tile column.  Epilogue on the VALU: true division by Q, round to nearest even, clamp, int16 to LDS as
//      [block][zigzag position];
//   3. entropy coding, one wave per block, lane = zigzag position: __ballot of "non-zero" gives the block's mask,
//      each non-zero lane finds its zero run from the mask and forms its ZRL codes + (run, size) code + magnitude
//      bits in one 64-bit value (at most 59 bits); lane 0 codes the DC difference (the previous block's DC is in
//      LDS, so blocks do not wait for each other), lane 63 the EOB when its coefficient is zero.  Pass A only sums
//      the bit lengths per block; after a prefix sum over the blocks, pass B forms the codes again and ORs them
//      straight into the frame's bit stream in LDS at their final bit position (ds_or_b32: OR commutes, so the
//      result does not depend on the order of the waves).  There is no per-block bit buffer and no shift-and-merge
//      pass: the stream is written once.  It overlays the frame bytes, which are dead after stage 2;
//   4. byte stuffing: every thread counts the 0xFF bytes of its slice of the stream, a workgroup prefix sum gives
//      each slice its output position, and header, stuffed scan and EOI go to the payload.
// Compact output without any wait between workgroups: launch 1 (out == NULL) stops after the count and writes
// lengths[N]; the caller forms offsets = exclusive prefix sum; launch 2 encodes again and writes each payload at
// its offset.  Both launches run the same code on the same data, so the lengths agree.
//
// LDS per frame of B blocks: 1408 bytes of tables, 4 (B + 1) block offsets, 128 B coefficients and the larger of
// the frame bytes (H W + 32) and the worst-case stream (208 B + 16: a block has at most 20 + 63 x 26 = 1658
// bits), under the 160 KB of a gfx950 CU: B <= 477.
#include "hq_common.h"

#include <limits.h>

#include <initializer_list>

namespace hq {

typedef float jpg_f4 __attribute__((ext_vector_type(4)));

constexpr int kJpgThreads = 256;
constexpr int kJpgHdrMax = 320;                 // the header is 310 bytes
constexpr int kJpgQOff = 7;                     // header offset of the 64 DQT entries (zigzag order)
constexpr size_t kJpgBlockBytes = 208;          // ceil(1658 / 8)
constexpr size_t kJpgLdsMax = 160 * 1024;
constexpr uint32_t kJpgOffAc = 256, kJpgOffDc = 1280, kJpgOffRed = 1344, kJpgOffBlk = 1408;

// zigzag position -> natural (row-major) index
constexpr uint8_t kJpgZigzag[64] = {0,  1,  8,  16, 9,  2,  3,  10, 17, 24, 32, 25, 18, 11, 4,  5,
                                    12, 19, 26, 33, 40, 48, 41, 34, 27, 20, 13, 6,  7,  14, 21, 28,
                                    35, 42, 49, 56, 57, 50, 43, 36, 29, 22, 15, 23, 30, 37, 44, 51,
                                    58, 59, 52, 45, 38, 31, 39, 46, 53, 60, 61, 54, 47, 55, 62, 63};
// ITU-T T.81 Annex K.1 luminance quantisation table, natural order
constexpr uint8_t kJpgBaseQ[64] = {16, 11, 10, 16, 24,  40,  51,  61,  12, 12, 14, 19, 26,  58,  60,  55,
                                   14, 13, 16, 24, 40,  57,  69,  56,  14, 17, 22, 29, 51,  87,  80,  62,
                                   18, 22, 37, 56, 68,  109, 103, 77,  24, 35, 55, 64, 81,  104, 113, 92,
                                   49, 64, 78, 87, 103, 121, 120, 101, 72, 92, 95, 98, 112, 100, 103, 99};
// Annex K.3 luminance Huffman tables: codes per length 1 .. 16, then the symbols in code order
constexpr uint8_t kJpgDcBits[16] = {0, 1, 5, 1, 1, 1, 1, 1, 1, 0, 0, 0, 0, 0, 0, 0};
constexpr uint8_t kJpgDcVals[12] = {0, 1, 2, 3, 4, 5, 6, 7, 8, 9, 10, 11};
constexpr uint8_t kJpgAcBits[16] = {0, 2, 1, 3, 3, 2, 4, 3, 5, 5, 4, 4, 0, 0, 1, 0x7d};
constexpr uint8_t kJpgAcVals[162] = {
    0x01, 0x02, 0x03, 0x00, 0x04, 0x11, 0x05, 0x12, 0x21, 0x31, 0x41, 0x06, 0x13, 0x51, 0x61, 0x07, 0x22, 0x71,
    0x14, 0x32, 0x81, 0x91, 0xa1, 0x08, 0x23, 0x42, 0xb1, 0xc1, 0x15, 0x52, 0xd1, 0xf0, 0x24, 0x33, 0x62, 0x72,
    0x82, 0x09, 0x0a, 0x16, 0x17, 0x18, 0x19, 0x1a, 0x25, 0x26, 0x27, 0x28, 0x29, 0x2a, 0x34, 0x35, 0x36, 0x37,
    0x38, 0x39, 0x3a, 0x43, 0x44, 0x45, 0x46, 0x47, 0x48, 0x49, 0x4a, 0x53, 0x54, 0x55, 0x56, 0x57, 0x58, 0x59,
    0x5a, 0x63, 0x64, 0x65, 0x66, 0x67, 0x68, 0x69, 0x6a, 0x73, 0x74, 0x75, 0x76, 0x77, 0x78, 0x79, 0x7a, 0x83,
    0x84, 0x85, 0x86, 0x87, 0x88, 0x89, 0x8a, 0x92, 0x93, 0x94, 0x95, 0x96, 0x97, 0x98, 0x99, 0x9a, 0xa2, 0xa3,
    0xa4, 0xa5, 0xa6, 0xa7, 0xa8, 0xa9, 0xaa, 0xb2, 0xb3, 0xb4, 0xb5, 0xb6, 0xb7, 0xb8, 0xb9, 0xba, 0xc2, 0xc3,
    0xc4, 0xc5, 0xc6, 0xc7, 0xc8, 0xc9, 0xca, 0xd2, 0xd3, 0xd4, 0xd5, 0xd6, 0xd7, 0xd8, 0xd9, 0xda, 0xe1, 0xe2,
    0xe3, 0xe4, 0xe5, 0xe6, 0xe7, 0xe8, 0xe9, 0xea, 0xf1, 0xf2, 0xf3, 0xf4, 0xf5, 0xf6, 0xf7, 0xf8, 0xf9, 0xfa};

// Encoder tables, entry = code << 8 | length (0: the symbol has no code), built as Annex C does.
struct JpgHuff {
  uint32_t ac[256];
  uint32_t dc[16];
};
constexpr JpgHuff make_jpg_huff() {
  JpgHuff h{};
  uint32_t code = 0;
  int k = 0;
  for (int len = 1; len <= 16; ++len, code <<= 1)
    for (int i = 0; i < kJpgDcBits[len - 1]; ++i) h.dc[kJpgDcVals[k++]] = (code++ << 8) | (uint32_t)len;
  code = 0;
  k = 0;
  for (int len = 1; len <= 16; ++len, code <<= 1)
    for (int i = 0; i < kJpgAcBits[len - 1]; ++i) h.ac[kJpgAcVals[k++]] = (code++ << 8) | (uint32_t)len;
  return h;
}
__device__ const JpgHuff kJpgHuff = make_jpg_huff();

// The DCT matrix K[z][k] = C[u][ky] C[v][kx] (zigzag position z = frequencies (u, v), k = 8 ky + kx the pixel of
// the block, C[u][x] = a(u) cos((2x + 1) u pi / 16), a(0) = sqrt(1/8), a(u) = 1/2), computed in float64 at compile
// time, rounded once to float32 and stored in the order the A operand of v_mfma_f32_16x16x4_f32 wants it: entry
// (16 rt + t) * 64 + lane = K[16 rt + (lane & 15)][4 t + (lane >> 4)] for tile row rt and K step t.
struct JpgK {
  float v[4096];
};
constexpr double jpg_cos16(int m) {  // cos(m pi / 16)
  constexpr double c[9] = {1.0,
                           0.98078528040323044913,
                           0.92387953251128675613,
                           0.83146961230254523708,
                           0.70710678118654752440,
                           0.55557023301960222474,
                           0.38268343236508977173,
                           0.19509032201612826785,
                           0.0};
  m &= 31;
  return m <= 8 ? c[m] : (m <= 16 ? -c[16 - m] : (m <= 24 ? -c[m - 16] : c[32 - m]));
}
constexpr double jpg_c(int u, int x) { return (u == 0 ? 0.35355339059327376220 : 0.5) * jpg_cos16((2 * x + 1) * u); }
constexpr JpgK make_jpg_k() {
  JpgK t{};
  for (int rt = 0; rt < 4; ++rt)
    for (int s = 0; s < 16; ++s)
      for (int lane = 0; lane < 64; ++lane) {
        const int nat = kJpgZigzag[16 * rt + (lane & 15)], k = 4 * s + (lane >> 4);
        t.v[(16 * rt + s) * 64 + lane] = (float)(jpg_c(nat >> 3, k >> 3) * jpg_c(nat & 7, k & 7));
      }
  return t;
}
__device__ const JpgK kJpgK = make_jpg_k();

// everything before the scan data, passed to the kernel by value (the DQT entries double as the divisors)
struct JpgHdr {
  int len;
  uint8_t b[kJpgHdrMax];
};

static void jpg_build_header(int H, int W, int q, JpgHdr& h) {
  uint8_t* p = h.b;
  auto put = [&](std::initializer_list<int> v) { for (int x : v) *p++ = (uint8_t)x; };
  put({0xFF, 0xD8, 0xFF, 0xDB, 0x00, 0x43, 0x00});
  const int s = q < 50 ? 5000 / q : 200 - 2 * q;  // libjpeg's jpeg_quality_scaling
  for (int z = 0; z < 64; ++z) {
    const int v = (kJpgBaseQ[kJpgZigzag[z]] * s + 50) / 100;
    *p++ = (uint8_t)(v < 1 ? 1 : (v > 255 ? 255 : v));
  }
  put({0xFF, 0xC0, 0x00, 0x0B, 0x08, H >> 8, H & 255, W >> 8, W & 255, 0x01, 0x01, 0x11, 0x00});
  put({0xFF, 0xC4, 0x00, 0x1F, 0x00});
  for (int i = 0; i < 16; ++i) *p++ = kJpgDcBits[i];
  for (int i = 0; i < 12; ++i) *p++ = kJpgDcVals[i];
  put({0xFF, 0xC4, 0x00, 0xB5, 0x10});
  for (int i = 0; i < 16; ++i) *p++ = kJpgAcBits[i];
  for (int i = 0; i < 162; ++i) *p++ = kJpgAcVals[i];
  put({0xFF, 0xDA, 0x00, 0x08, 0x01, 0x01, 0x00, 0x00, 0x3F, 0x00});
  h.len = (int)(p - h.b);
}

// LDS layout of a frame (bytes): tables at fixed offsets, then block offsets [B + 1], coefficients [B][64] int16,
// then the region shared by the frame bytes (stage 1-2) and the bit stream (stage 3-4)
struct JpgLds {
  uint32_t coef, stream, stream_bytes, total;
};
__host__ __device__ inline JpgLds jpg_lds(int H, int W, int B) {
  JpgLds l;
  l.coef = (kJpgOffBlk + 4u * (uint32_t)(B + 1) + 15u) & ~15u;
  l.stream = l.coef + 128u * (uint32_t)B;
  const uint32_t raw = ((uint32_t)H * (uint32_t)W + 32u + 15u) & ~15u;
  l.stream_bytes = (uint32_t)kJpgBlockBytes * (uint32_t)B + 16u;
  l.total = l.stream + (raw > l.stream_bytes ? raw : l.stream_bytes);
  return l;
}

// wave64 inclusive prefix sum
__device__ __forceinline__ int jpg_wave_scan(int x, int lane) {
#pragma unroll
  for (int d = 1; d < 64; d <<= 1) {
    const int y = __shfl_up(x, d, 64);
    if (lane >= d) x += y;
  }
  return x;
}

// Lane `lane` of the wave that codes block b: its bits (right-aligned in v) and their count.  All 64 lanes call.
__device__ __forceinline__ int jpg_code(const int16_t* __restrict__ cf, int b, int lane,
                                        const uint32_t* __restrict__ ac, const uint32_t* __restrict__ dc,
                                        uint64_t& v) {
  const int c = cf[b * 64 + lane];
  const bool nz = lane > 0 && c != 0;
  const uint64_t mask = __ballot(nz);
  v = 0;
  int nb = 0;
  if (lane == 0) {  // DC: difference to the previous block's DC, category code + magnitude bits
    const int d = c - (b > 0 ? (int)cf[(b - 1) * 64] : 0);
    const int size = 32 - __clz(d < 0 ? -d : d);
    const uint32_t e = dc[size];
    const uint32_t mag = (uint32_t)(d < 0 ? d - 1 : d) & ((1u << size) - 1u);
    v = ((uint64_t)(e >> 8) << size) | mag;
    nb = (int)(e & 255u) + size;
  } else if (nz) {  // AC: zeros since the previous non-zero position (position 0 when there is none)
    const uint64_t lower = mask & ((1ull << lane) - 1ull);
    const int prev = lower ? 63 - __clzll((long long)lower) : 0;
    const int run = lane - prev - 1;
    const int size = 32 - __clz(c < 0 ? -c : c);
    const uint32_t e = ac[((run & 15) << 4) | size], zrl = ac[0xF0];
    const uint32_t mag = (uint32_t)(c < 0 ? c - 1 : c) & ((1u << size) - 1u);
    for (int i = 0; i < (run >> 4); ++i) v = (v << (zrl & 255u)) | (zrl >> 8);
    v = (v << (e & 255u)) | (e >> 8);
    v = (v << size) | mag;
    nb = (run >> 4) * (int)(zrl & 255u) + (int)(e & 255u) + size;
  } else if (lane == 63) {  // the block ends in zeros: EOB
    v = ac[0] >> 8;
    nb = (int)(ac[0] & 255u);
  }
  return nb;
}

// OR the nb <= 59 low bits of v into the MSB-first stream at bit position p (words hold 32 stream bits, first bit
// in bit 31).  Only words that receive a set bit are touched.
__device__ __forceinline__ void jpg_put(uint32_t* stream, uint32_t p, uint64_t v, int nb) {
  const uint32_t w = p >> 5;
  const int sh = 96 - (int)(p & 31u) - nb;  // left shift of v inside the 96-bit window of words w .. w + 2: >= 6
  const uint64_t top = sh >= 32 ? v << (sh - 32) : v >> (32 - sh);
  const uint32_t low = sh >= 32 ? 0u : (uint32_t)(v << sh);
  if ((uint32_t)(top >> 32)) atomicOr(&stream[w], (uint32_t)(top >> 32));
  if ((uint32_t)top) atomicOr(&stream[w + 1], (uint32_t)top);
  if (low) atomicOr(&stream[w + 2], low);
}

__global__ __launch_bounds__(kJpgThreads) void k_jpeg(const uint8_t* __restrict__ frames, int H, int W, JpgHdr hdr,
                                                      const int64_t* __restrict__ offsets,
                                                      int32_t* __restrict__ lengths, uint8_t* __restrict__ out,
                                                      int16_t* __restrict__ coefs, int vec_ok) {
  extern __shared__ __attribute__((aligned(16))) uint8_t jpg_smem[];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int bw = (W + 7) >> 3, B = bw * ((H + 7) >> 3);
  const JpgLds L = jpg_lds(H, W, B);
  float* qz = reinterpret_cast<float*>(jpg_smem);
  uint32_t* ac = reinterpret_cast<uint32_t*>(jpg_smem + kJpgOffAc);
  uint32_t* dc = reinterpret_cast<uint32_t*>(jpg_smem + kJpgOffDc);
  uint32_t* red = reinterpret_cast<uint32_t*>(jpg_smem + kJpgOffRed);
  uint32_t* boff = reinterpret_cast<uint32_t*>(jpg_smem + kJpgOffBlk);
  int16_t* cf = reinterpret_cast<int16_t*>(jpg_smem + L.coef);
  uint8_t* raw = jpg_smem + L.stream;
  uint32_t* stream = reinterpret_cast<uint32_t*>(jpg_smem + L.stream);
  const int64_t f = blockIdx.x, HW = (int64_t)H * W, base = f * HW;

  // ---- stage 1: tables and the frame's bytes to LDS
  if (tid < 64) qz[tid] = (float)hdr.b[kJpgQOff + tid];
  ac[tid] = kJpgHuff.ac[tid];
  if (tid < 16) dc[tid] = kJpgHuff.dc[tid];
  const int shift = vec_ok ? (int)(base & 15) : 0;  // raw[shift + i] = byte i of the frame
  if (vec_ok) {
    const int64_t abase = base - shift, total = (int64_t)gridDim.x * HW;
    const int nchunks = (int)((shift + HW + 15) >> 4);
    for (int c = tid; c < nchunks; c += kJpgThreads) {
      const int64_t g = abase + 16 * (int64_t)c;
      if (g + 16 <= total) {
        *reinterpret_cast<uint4*>(raw + 16 * c) = *reinterpret_cast<const uint4*>(frames + g);
      } else {  // the chunk that holds the batch's last byte
        for (int i = 0; i < 16 && g + i < total; ++i) raw[16 * c + i] = frames[g + i];
      }
    }
  } else {
    for (int i = tid; i < (int)HW; i += kJpgThreads) raw[i] = frames[base + i];
  }
  __syncthreads();

  // ---- stage 2: DCT + quantise.  A: lane = row (lane & 15), k = lane >> 4; B: lane = column (lane & 15), k = lane
  // >> 4; accumulator element r = row 4 (lane >> 4) + r, column lane & 15.
  const int ntc = (B + 15) >> 4;
  if (wave < ntc) {
    float a[4][16];
#pragma unroll
    for (int rt = 0; rt < 4; ++rt)
#pragma unroll
      for (int t = 0; t < 16; ++t) a[rt][t] = kJpgK.v[(16 * rt + t) * 64 + lane];
    for (int tc = wave; tc < ntc; tc += kJpgThreads / 64) {
      const int j = 16 * tc + (lane & 15);
      const bool live = j < B;
      const int jb = live ? j : 0;
      const int y0 = (jb / bw) * 8, x0 = (jb % bw) * 8;
      jpg_f4 acc[4];
#pragma unroll
      for (int rt = 0; rt < 4; ++rt) acc[rt] = jpg_f4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
      for (int t = 0; t < 16; ++t) {
        const int k = 4 * t + (lane >> 4);
        const int y = min(y0 + (k >> 3), H - 1), x = min(x0 + (k & 7), W - 1);  // edge replication
        const float px = (float)((int)raw[shift + y * W + x] - 128);
#pragma unroll
        for (int rt = 0; rt < 4; ++rt) acc[rt] = __builtin_amdgcn_mfma_f32_16x16x4f32(a[rt][t], px, acc[rt], 0, 0, 0);
      }
      if (live) {
#pragma unroll
        for (int rt = 0; rt < 4; ++rt) {
          const int z0 = 16 * rt + 4 * (lane >> 4);
          int c[4];
#pragma unroll
          for (int r = 0; r < 4; ++r) {
            const int v = (int)rintf(acc[rt][r] / qz[z0 + r]);
            const int lo = z0 + r == 0 ? -1024 : -1023;  // DC differences stay inside category 11, AC inside 10
            c[r] = v < lo ? lo : (v > 1023 ? 1023 : v);
          }
          const uint2 pk = make_uint2((uint32_t)(c[0] & 0xFFFF) | ((uint32_t)c[1] << 16),
                                      (uint32_t)(c[2] & 0xFFFF) | ((uint32_t)c[3] << 16));
          *reinterpret_cast<uint2*>(cf + j * 64 + z0) = pk;
          if (coefs) *reinterpret_cast<uint2*>(coefs + (f * B + j) * 64 + z0) = pk;
        }
      }
    }
  }
  __syncthreads();

  // ---- stage 3, pass A: clear the stream (the frame bytes are dead), bit length of every block
  for (uint32_t w = tid; w < L.stream_bytes / 4; w += kJpgThreads) stream[w] = 0u;
  for (int b = wave; b < B; b += kJpgThreads / 64) {
    uint64_t v;
    const int x = jpg_wave_scan(jpg_code(cf, b, lane, ac, dc, v), lane);
    if (lane == 63) boff[b] = (uint32_t)x;
  }
  __syncthreads();
  if (wave == 0) {  // exclusive prefix sum over the blocks: each lane a run of per blocks, then across the lanes
    const int per = (B + 63) >> 6, b0 = lane * per, b1 = min(b0 + per, B);
    int s = 0;
    for (int b = b0; b < b1; ++b) s += (int)boff[b];
    const int incl = jpg_wave_scan(s, lane);
    uint32_t run = (uint32_t)(incl - s);
    for (int b = b0; b < b1; ++b) {
      const uint32_t n = boff[b];
      boff[b] = run;
      run += n;
    }
    if (lane == 63) boff[B] = (uint32_t)incl;
  }
  __syncthreads();

  // ---- stage 3, pass B: the codes again, ORed into the stream at their final position; 1-bits pad the last byte
  const uint32_t T = boff[B], nbytes = (T + 7u) >> 3;
  for (int b = wave; b < B; b += kJpgThreads / 64) {
    uint64_t v;
    const int nb = jpg_code(cf, b, lane, ac, dc, v);
    const int x = jpg_wave_scan(nb, lane);
    if (nb) jpg_put(stream, boff[b] + (uint32_t)(x - nb), v, nb);
  }
  if (tid == 0 && (T & 7u)) jpg_put(stream, T, (1ull << (8u - (T & 7u))) - 1ull, (int)(8u - (T & 7u)));
  __syncthreads();

  // ---- stage 4: count the 0xFF bytes per slice (bytes past nbytes are zero), prefix sum, write
  const uint32_t words = (nbytes + 3u) >> 2, cw = (words + kJpgThreads - 1) / kJpgThreads;
  const uint32_t w0 = min((uint32_t)tid * cw, words), w1 = min(w0 + cw, words);
  int nff = 0;
  for (uint32_t w = w0; w < w1; ++w) {
    const uint32_t x = stream[w];
    nff += ((x >> 24) == 0xFFu) + (((x >> 16) & 0xFFu) == 0xFFu) + (((x >> 8) & 0xFFu) == 0xFFu) + ((x & 0xFFu) == 0xFFu);
  }
  const int incl = jpg_wave_scan(nff, lane);
  if (lane == 63) red[wave] = (uint32_t)incl;
  __syncthreads();
  uint32_t before = (uint32_t)(incl - nff), all = 0;
  for (int w = 0; w < kJpgThreads / 64; ++w) {
    if (w < wave) before += red[w];
    all += red[w];
  }
  const int64_t len = (int64_t)hdr.len + nbytes + all + 2;
  if (!out) {
    if (tid == 0) lengths[f] = (int32_t)len;
    return;
  }
  const int64_t o = offsets[f];
  if (offsets[f + 1] - o != len) {  // not the offsets of these frames: write nothing outside the slot
    if (tid == 0 && lengths) lengths[f] = -1;
    return;
  }
  if (tid == 0 && lengths) lengths[f] = (int32_t)len;
  uint8_t* dst = out + o;
  for (int i = tid; i < hdr.len; i += kJpgThreads) dst[i] = hdr.b[i];
  uint8_t* d = dst + hdr.len + 4 * (int64_t)w0 + before;
  for (uint32_t w = w0; w < w1; ++w) {
    const uint32_t x = stream[w];
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      if (4 * w + i < nbytes) {
        const uint8_t byte = (uint8_t)(x >> (24 - 8 * i));
        *d++ = byte;
        if (byte == 0xFF) *d++ = 0x00;
      }
    }
  }
  if (tid == 0) {
    dst[len - 2] = 0xFF;
    dst[len - 1] = 0xD9;
  }
}

}  // namespace hq

using namespace hq;

extern "C" {

int hq_jpeg_encode(const uint8_t* frames, int64_t N, int H, int W, int q, const int64_t* offsets, int32_t* lengths,
                   uint8_t* out, int16_t* coefs, hq_stream_t stream) {
  if (N < 0 || N > INT_MAX || H < 1 || W < 1)
    return fail(HQ_E_INVALID, "jpeg encode: bad shape %lld x %d x %d", (long long)N, H, W);
  if (q < 1 || q > 95) return fail(HQ_E_UNSUPPORTED, "jpeg encode: quality %d (1 <= q <= 95)", q);
  const int64_t B = ((int64_t)(H + 7) / 8) * ((int64_t)(W + 7) / 8);
  const int64_t max_blocks = (int64_t)((kJpgLdsMax - kJpgOffBlk - 64) / (4 + 128 + kJpgBlockBytes));
  if (H > 65535 || W > 65535 || B > max_blocks || jpg_lds(H, W, (int)B).total > kJpgLdsMax)
    return fail(HQ_E_UNSUPPORTED, "jpeg encode: a frame of %d x %d has %lld 8 x 8 blocks (at most %lld fit the LDS)",
                H, W, (long long)B, (long long)max_blocks);
  if (N == 0) return HQ_OK;
  if (!frames || (!out && !lengths) || (out && !offsets)) return fail(HQ_E_INVALID, "null buffer");
  if (reinterpret_cast<uintptr_t>(coefs) & 7) return fail(HQ_E_INVALID, "jpeg encode: coefs must be 8-byte aligned");
  JpgHdr hdr;
  jpg_build_header(H, W, q, hdr);
  const size_t lds = jpg_lds(H, W, (int)B).total;
  if (lds > 64 * 1024)
    HQ_CHECK_HIP(hipFuncSetAttribute((const void*)k_jpeg, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
  const int vec_ok = (reinterpret_cast<uintptr_t>(frames) & 15) == 0;
  hipLaunchKernelGGL(k_jpeg, dim3((unsigned)N), dim3(kJpgThreads), lds, (hipStream_t)stream, frames, H, W, hdr,
                     offsets, lengths, out, coefs, vec_ok);
  HQ_CHECK_LAUNCH();
  return HQ_OK;
}

}  // extern "C"
