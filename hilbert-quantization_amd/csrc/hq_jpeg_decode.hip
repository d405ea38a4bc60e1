// hq_jpeg_decode.hip — batched grayscale baseline JPEG decoder on the device, bit-identical to
// libjpeg's default decode (Huffman, dequantise, ISLOW integer inverse DCT, range limit), which is what PIL runs.
//
// k_jpeg_probe: one thread per payload walks the marker segments (jpd_probe) and writes a descriptor.
// k_jpeg_decode<F>: a one-wave workgroup owns F frames.  Huffman decoding is sequential per frame, so the
//   parallelism of the hot part is frames: lanes 0 .. F-1 decode one 8 x 8 block each, all F frames in step, into
//   an LDS tile of natural-order int16 coefficients; then all 64 lanes run the inverse DCT of those F blocks in
//   integer VALU code (pass 1: lane = frame x column, pass 2: lane = frame x row; no matrix instructions: an
//   MFMA float IDCT cannot give libjpeg's bytes, and the IDCT is not the bound).  Pixels go to an LDS strip of one
//   block row per frame, flushed at the end of every block row with 16-byte stores where the frames allow it.
//   F < 64 on purpose: a 100,000-frame batch is 6,250 waves at F = 16 against 1,563 at F = 64, for about 8,000
//   wave slots, and the lanes that do not decode are free for the IDCT.
// Safety: the scan loop runs blocks x (1 DC + at most 63 AC) symbols whatever the bytes are; every payload byte
// is read through jpd_u8 inside [offsets[i], offsets[i + 1]); a frame writes only its own H x W bytes.  A frame
// that is refused (any status but 0) keeps running in step on zero bits and its output is zero-filled at the end.
//
// LDS of a workgroup: F x (2 JpdTable + 64 u16 steps) = 576 F, the tile 128 F, the strip 64 F ceil(W / 8), 256
// bytes of flags: 19.25 KB at F = 16, W = 64 (8 waves per CU up to W = 64; 33.25 KB at W = 176).
#include "hq_common.h"
#include "hq_jpeg_decode.h"

#include <limits.h>

namespace hq {

constexpr int kJpdMaxW = 224;  // 64 frames x 28 blocks of strip still fit the 160 KB of a CU
constexpr int kJpdFlagRange = 1, kJpdFlagCorrupt = 2;

__host__ __device__ inline size_t jpd_lds_bytes(int F, int W) {
  return (size_t)F * (2 * sizeof(JpdTable) + 128 + 128 + 64 * (size_t)((W + 7) >> 3)) + 64 * sizeof(int32_t);
}

__global__ __launch_bounds__(256) void k_jpeg_probe(const uint8_t* __restrict__ payload,
                                                    const int64_t* __restrict__ offsets, int64_t N,
                                                    int32_t* __restrict__ desc) {
  const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= N) return;
  int32_t d[JPD_DESC];
  jpd_probe(payload, offsets[i], offsets[i + 1], d);
#pragma unroll
  for (int k = 0; k < JPD_DESC; ++k) desc[i * JPD_DESC + k] = d[k];
}

template <int F>
__global__ __launch_bounds__(64) void k_jpeg_decode(const uint8_t* __restrict__ payload,
                                                    const int64_t* __restrict__ offsets,
                                                    const int32_t* __restrict__ desc, const int64_t* __restrict__ ids,
                                                    int64_t M, int H, int W, uint8_t* __restrict__ frames,
                                                    int32_t* __restrict__ status, int16_t* __restrict__ coefs,
                                                    int vw) {
  extern __shared__ __attribute__((aligned(16))) uint8_t jpd_smem[];
  const int lane = threadIdx.x;
  const int bw = (W + 7) >> 3, bh = (H + 7) >> 3, sw = 8 * bw;  // sw: bytes of a strip row
  JpdTable* tabs = reinterpret_cast<JpdTable*>(jpd_smem);                       // [F][2]: DC, AC
  uint16_t* quant = reinterpret_cast<uint16_t*>(jpd_smem + (size_t)F * 2 * sizeof(JpdTable));  // [F][64] natural
  int16_t* tile = reinterpret_cast<int16_t*>(quant + F * 64);                   // [F][64] natural
  uint8_t* strip = reinterpret_cast<uint8_t*>(tile + F * 64);                   // [F][8][sw]
  int32_t* flags = reinterpret_cast<int32_t*>(strip + (size_t)F * 8 * sw);      // [64], F used
  const int64_t m0 = (int64_t)blockIdx.x * F;
  const int nf = (int)(M - m0 < F ? M - m0 : F);  // frames of this workgroup

  // ---- setup.  Lanes 0 .. F-1 own a frame each for the whole kernel: byte range, descriptor, reader state.
  int64_t begin = 0, end = 0;
  int32_t d[JPD_DESC] = {JPD_BAD_ID, 0, 0, 0, 0, 0, 0, 0};
  if (lane < nf) {
    const int64_t pi = ids ? ids[m0 + lane] : m0 + lane;
    if (pi >= 0) {
      begin = offsets[pi];
      end = offsets[pi + 1];
      if (begin < 0 || end < begin) {
        end = begin = 0;
      } else {
#pragma unroll
        for (int k = 0; k < JPD_DESC; ++k) d[k] = desc[pi * JPD_DESC + k];
      }
    }
    if (d[JPD_STATUS] == JPD_OK && (d[JPD_H] != H || d[JPD_W] != W)) d[JPD_STATUS] = JPD_SHAPE;
    // offsets a caller made up must still point into the payload: 1 <= table < scan <= length
    const int64_t len = end - begin;
    if (d[JPD_STATUS] == JPD_OK && (d[JPD_DQT] < 1 || d[JPD_DQT] + 64 > len || d[JPD_DC] < 1 || d[JPD_AC] < 1 ||
                                    d[JPD_SCAN] < 1 || d[JPD_SCAN] > len))
      d[JPD_STATUS] = JPD_BAD_ID;
  }
  // the frame's state travels to the lanes that build its tables through LDS
  int64_t* xb = reinterpret_cast<int64_t*>(strip);  // [F][2] begin, end; [F][4] int32 status, dqt, dc, ac after it
  int32_t* xd = reinterpret_cast<int32_t*>(xb + 2 * F);
  if (lane < F) {
    xb[2 * lane] = begin;
    xb[2 * lane + 1] = end;
    xd[4 * lane] = lane < nf ? d[JPD_STATUS] : JPD_BAD_ID;
    xd[4 * lane + 1] = d[JPD_DQT];
    xd[4 * lane + 2] = d[JPD_DC];
    xd[4 * lane + 3] = d[JPD_AC];
    flags[lane] = 0;
  }
  __syncthreads();
  for (int t = lane; t < 2 * F; t += 64) {  // one lane per (frame, table)
    const int f = t >> 1;
    const int64_t fb = xb[2 * f], fe = xb[2 * f + 1];
    const bool ok = xd[4 * f] == JPD_OK;
    if (!jpd_build_table(payload, ok ? fb + xd[4 * f + 2 + (t & 1)] : -1, fb, ok ? fe : fb, tabs[t]) && ok)
      atomicOr(&flags[f], kJpdFlagCorrupt);
  }
  for (int f = 0; f < F; ++f) {  // dequantisation steps, de-zigzagged: lane = zigzag position
    const int64_t fb = xb[2 * f], fe = xb[2 * f + 1];
    quant[f * 64 + jpd_zigzag(lane)] = xd[4 * f] == JPD_OK ? (uint16_t)jpd_u8(payload, fb + xd[4 * f + 1] + lane, fe) : 0;
  }
  for (int i = lane; i < F * 64 / 2; i += 64) reinterpret_cast<uint32_t*>(tile)[i] = 0u;
  __syncthreads();  // xb / xd (inside the strip) are dead from here

  JpdBits br;
  const bool live = lane < nf && d[JPD_STATUS] == JPD_OK;
  jpd_bits_init(br, live ? begin + d[JPD_SCAN] : 0, live ? end : 0);  // a refused frame reads zero bits
  const int64_t dcsym = begin + d[JPD_DC] + 16, acsym = begin + d[JPD_AC] + 16;
  int pred = 0;
  bool corrupt = false;
  const int64_t B = (int64_t)bw * bh;

  // ---- blocks in raster order, all frames in step
  for (int by = 0; by < bh; ++by) {
    for (int bx = 0; bx < bw; ++bx) {
      if (lane < nf)
        corrupt |= !jpd_block(br, payload, tabs[2 * lane], dcsym, tabs[2 * lane + 1], acsym, pred, tile + lane * 64);
      __syncthreads();
      if (coefs)  // zigzag order, the encoder's layout: lane = zigzag position
        for (int f = 0; f < nf; ++f)
          coefs[((m0 + f) * B + (int64_t)by * bw + bx) * 64 + lane] = tile[f * 64 + jpd_zigzag(lane)];
      // pass 1, columns: dequantise, ISLOW, (x + 2^10) >> 11, in place
      for (int t = lane; t < 8 * F; t += 64) {
        const int f = t >> 3, c = t & 7;
        int32_t x[8], y[8];
        bool bad = false;
#pragma unroll
        for (int r = 0; r < 8; ++r)
          x[r] = jpd_guard((int32_t)tile[f * 64 + 8 * r + c] * (int32_t)quant[f * 64 + 8 * r + c], &bad);
        jpd_idct_1d(x, y, 11);
#pragma unroll
        for (int r = 0; r < 8; ++r) tile[f * 64 + 8 * r + c] = (int16_t)jpd_guard(y[r], &bad);
        if (bad) atomicOr(&flags[f], kJpdFlagRange);
      }
      __syncthreads();
      // pass 2, rows: ISLOW, (x + 2^17) >> 18, range limit; the tile row is cleared for the next block
      for (int t = lane; t < 8 * F; t += 64) {
        const int f = t >> 3, r = t & 7;
        int32_t x[8], y[8];
        bool bad = false;
        const uint4 row = *reinterpret_cast<const uint4*>(tile + f * 64 + 8 * r);
        const uint32_t w[4] = {row.x, row.y, row.z, row.w};
#pragma unroll
        for (int c = 0; c < 8; ++c) x[c] = (int32_t)(int16_t)(w[c >> 1] >> (16 * (c & 1)));
        *reinterpret_cast<uint4*>(tile + f * 64 + 8 * r) = make_uint4(0u, 0u, 0u, 0u);
        jpd_idct_1d(x, y, 18);
        uint32_t px[2] = {0u, 0u};
#pragma unroll
        for (int c = 0; c < 8; ++c) px[c >> 2] |= (uint32_t)jpd_range_limit(y[c], &bad) << (8 * (c & 3));
        *reinterpret_cast<uint2*>(strip + ((size_t)f * 8 + r) * sw + 8 * bx) = make_uint2(px[0], px[1]);
        if (bad) atomicOr(&flags[f], kJpdFlagRange);
      }
      __syncthreads();
    }
    // ---- flush the block row, clipped to H and W: units of vw bytes (vw = 16, 4 or 1 divides W)
    const int nr = H - 8 * by < 8 ? H - 8 * by : 8, upr = W / vw, total = nf * nr * upr;
    for (int u = lane; u < total; u += 64) {
      const int f = u / (nr * upr), rem = u - f * (nr * upr), r = rem / upr, x = (rem - r * upr) * vw;
      const uint8_t* src = strip + ((size_t)f * 8 + r) * sw + x;
      uint8_t* dst = frames + ((m0 + f) * H + 8 * by + r) * (int64_t)W + x;
      if (vw == 16) {
        *reinterpret_cast<uint4*>(dst) = make_uint4(reinterpret_cast<const uint32_t*>(src)[0],
                                                    reinterpret_cast<const uint32_t*>(src)[1],
                                                    reinterpret_cast<const uint32_t*>(src)[2],
                                                    reinterpret_cast<const uint32_t*>(src)[3]);
      } else if (vw == 4) {
        *reinterpret_cast<uint32_t*>(dst) = *reinterpret_cast<const uint32_t*>(src);
      } else {
        *dst = *src;
      }
    }
    __syncthreads();
  }

  // ---- acceptance: no flag, FF D9 right after the pad bits
  if (lane < nf) {
    int st = d[JPD_STATUS];
    const int fl = flags[lane];
    if (st == JPD_OK) {
      if (corrupt || (fl & kJpdFlagCorrupt)) st = JPD_CORRUPT;
      else if (br.truncated) st = JPD_TRUNCATED;
      else if (fl & kJpdFlagRange) st = JPD_RANGE;
      else if (!jpd_at_eoi(br, payload)) st = JPD_NO_EOI;
    }
    status[m0 + lane] = st;
    flags[lane] = st;
  }
  __syncthreads();
  for (int f = 0; f < nf; ++f) {  // a refused frame leaves zeros
    if (flags[f] == JPD_OK) continue;
    uint8_t* dst = frames + (m0 + f) * (int64_t)H * W;
    for (int64_t i = lane; i < (int64_t)H * W; i += 64) dst[i] = 0;
  }
}

typedef void (*jpd_kernel_t)(const uint8_t*, const int64_t*, const int32_t*, const int64_t*, int64_t, int, int,
                             uint8_t*, int32_t*, int16_t*, int);

}  // namespace hq

using namespace hq;

extern "C" {

int hq_jpeg_probe(const uint8_t* payload, const int64_t* offsets, int64_t N, int32_t* desc, hq_stream_t stream) {
  if (N < 0) return fail(HQ_E_INVALID, "jpeg probe: bad count %lld", (long long)N);
  if (N == 0) return HQ_OK;
  if (!payload || !offsets || !desc) return fail(HQ_E_INVALID, "null buffer");
  hipLaunchKernelGGL(k_jpeg_probe, dim3((unsigned)((N + 255) / 256)), dim3(256), 0, (hipStream_t)stream, payload,
                     offsets, N, desc);
  HQ_CHECK_LAUNCH();
  return HQ_OK;
}

int hq_jpeg_decode(const uint8_t* payload, const int64_t* offsets, const int32_t* desc, const int64_t* ids, int64_t M,
                   int H, int W, uint8_t* frames, int32_t* status, int16_t* coefs, hq_stream_t stream) {
  if (M < 0 || M > INT_MAX || H < 1 || W < 1)
    return fail(HQ_E_INVALID, "jpeg decode: bad shape %lld x %d x %d", (long long)M, H, W);
  if (W > kJpdMaxW || H > 65500)
    return fail(HQ_E_UNSUPPORTED, "jpeg decode: a frame of %d x %d (at most 65500 x %d)", H, W, kJpdMaxW);
  if (M == 0) return HQ_OK;
  if (!payload || !offsets || !desc || !frames || !status) return fail(HQ_E_INVALID, "null buffer");
  const int F = (int)opt(OPT_JPEG_DECODE_F, 16);
  jpd_kernel_t k = F == 8 ? k_jpeg_decode<8> : F == 16 ? k_jpeg_decode<16> : F == 32 ? k_jpeg_decode<32>
                   : F == 64 ? k_jpeg_decode<64> : nullptr;
  if (!k) return fail(HQ_E_INVALID, "jpeg decode: option jpeg_decode_f = %d (8, 16, 32 or 64)", F);
  const size_t lds = jpd_lds_bytes(F, W);
  if (lds > 64 * 1024)
    HQ_CHECK_HIP(hipFuncSetAttribute((const void*)k, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
  const uintptr_t a = reinterpret_cast<uintptr_t>(frames);
  const int vw = (W % 16 == 0 && a % 16 == 0) ? 16 : ((W % 4 == 0 && a % 4 == 0) ? 4 : 1);
  hipLaunchKernelGGL(k, dim3((unsigned)((M + F - 1) / F)), dim3(64), lds, (hipStream_t)stream, payload, offsets, desc,
                     ids, M, H, W, frames, status, coefs, vw);
  HQ_CHECK_LAUNCH();
  return HQ_OK;
}

}  // extern "C"
