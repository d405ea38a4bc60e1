// hq_decode.hip — the decode side of the headline path: u8 frames -> parameters in one kernel
// (hq_dequantize_unmap), and the round-trip error metrics of validate_quantization (hq_roundtrip_error).
//
// Reference sequence replaced (core/pipeline.py:183-235 reconstruct_parameters, after the JPEG codec):
//   _denormalize_from_compression (core/compressor.py:282-303: u8 / 255 * (max - min) + min in float32,
//   a constant frame gives min) -> extract_indices_from_image (core/index_generator.py:255-290: the last
//   row, trailing zeros trimmed, at least one value kept) -> map_from_2d (core/hilbert_mapper.py:176-205)
//   -> [:parameter_count];  and core/pipeline.py:257-259 (mse / mae / max_error of a round trip).
//
// Structure of the fast path (n in {16, 32, 64}; mirrors k_fused_np of hq_fused.hip):
//   * one wave64 per frame, non-persistent, 2 waves per workgroup, each wave with its own LDS frame;
//   * the (n+1) x n frame is read with 16-byte loads, lane j taking pieces j + 64t, into the row-major
//     LDS frame: HBM sees the frame's bytes once, in coalesced 1 KiB wave instructions;
//   * a 2x2 block of the image is one float4 group of the curve (layout invariant): lane j
//     owns groups j + 64t, reads the block's two u16 pairs from LDS, de-normalises the four bytes in curve
//     order (compile-time group LUT of hq_common.h) and writes one coalesced 16-byte store.  Only groups
//     below d are touched: padding is neither decoded nor written;
//   * the index row leaves as 16-byte stores by lanes < n / 4; its kept length comes from one ballot;
//   * every value is ((float)b / 255.0f) * (mx - mn) + mn with the IEEE division (no reciprocal form, no
//     contraction), computed per value: bit-identical to k_dequantize by construction.  At d = 1536 that is
//     24 divisions per lane and frame, the same count as the encoder's exact quantize, which is HBM-bound.
#include "hq_common.h"

namespace hq {

// Q2 arithmetic, exactly k_dequantize's (hq_quant.hip): constant frame -> mn (core/compressor.py:297-298)
__device__ __forceinline__ float denorm1(uint32_t b, float mn, float mx) {
  if (mx == mn) return mn;
  float t = (float)b / 255.0f;
  t = t * (mx - mn);
  return t + mn;
}

typedef float dq_f4v __attribute__((ext_vector_type(4)));
typedef unsigned int dq_u4v __attribute__((ext_vector_type(4)));

template <bool NT>
__device__ __forceinline__ void store_f4(float* p, float a, float b, float c, float d) {
  if constexpr (NT) __builtin_nontemporal_store(dq_f4v{a, b, c, d}, reinterpret_cast<dq_f4v*>(p));
  else *reinterpret_cast<float4*>(p) = make_float4(a, b, c, d);
}

__device__ constexpr GroupLut<16> kDecLut16 = make_group_lut<16, false>();
__device__ constexpr GroupLut<32> kDecLut32 = make_group_lut<32, false>();
__device__ constexpr GroupLut<64> kDecLut64 = make_group_lut<64, false>();
template <int NS>
__device__ __forceinline__ const uint32_t* dec_lut() {
  if constexpr (NS == 16) return kDecLut16.v;
  else if constexpr (NS == 32) return kDecLut32.v;
  else return kDecLut64.v;
}

template <int NS>
struct DecGeo {
  static constexpr int G = NS * NS / 4;        // float4 groups = 2x2 blocks
  static constexpr int NT = (G + 63) / 64;     // groups per lane
  static constexpr int FB = (NS + 1) * NS;     // frame bytes, a multiple of 16 for NS >= 16
  static constexpr int PIECES = FB / 16;
  static constexpr int PT = (PIECES + 63) / 64;
  static_assert(FB % 16 == 0, "frame is not a whole number of 16-byte pieces");
};

// vec_out: every output row starts 16-byte aligned (base aligned, out_stride % 4 == 0); vec_idx: idx_row is
// 16-byte aligned (its rows are n floats).  Without them the same values leave as scalar stores.
template <int NS, int WPB, bool NT>
__global__ __launch_bounds__(64 * WPB) void k_decode_np(const uint8_t* __restrict__ frame_in, int64_t N, int d,
                                                        const float* __restrict__ mm, int mm_shared,
                                                        float* __restrict__ out, int64_t out_stride, bool vec_out,
                                                        float* __restrict__ idx_row, bool vec_idx,
                                                        int32_t* __restrict__ idx_len) {
  using Geo = DecGeo<NS>;
  __shared__ __attribute__((aligned(16))) uint8_t smem[WPB * Geo::FB];
  const int lane = threadIdx.x & 63;
  const int wv = threadIdx.x >> 6;
  uint8_t* frame = smem + wv * Geo::FB;
  const int64_t e = (int64_t)blockIdx.x * WPB + wv;
  const bool live = e < N;
  const int groups = (d + 3) >> 2;
  // this lane's LUT entries (groups lane + 64 t, L2 resident), loaded alongside the frame
  const uint32_t* glut = dec_lut<NS>();
  uint32_t lut_r[Geo::NT];
#pragma unroll
  for (int t = 0; t < Geo::NT; ++t) lut_r[t] = (live && lane + 64 * t < groups) ? glut[lane + 64 * t] : 0u;
  float mn = 0.f, mx = 0.f;
  if (live) {
    const float* p = mm + (mm_shared ? 0 : 2 * e);
    mn = p[0];
    mx = p[1];
    const dq_u4v* src = reinterpret_cast<const dq_u4v*>(frame_in + e * (int64_t)Geo::FB);
#pragma unroll
    for (int t = 0; t < Geo::PT; ++t) {
      const int c = lane + 64 * t;
      if (c < Geo::PIECES) reinterpret_cast<dq_u4v*>(frame)[c] = src[c];
    }
  }
  __syncthreads();
  if (!live) return;

  // ---- parameters: float4 group j = the 2x2 block at lut offset, bytes picked in curve order ----------
  float* dst = out + e * out_stride;
#pragma unroll
  for (int t = 0; t < Geo::NT; ++t) {
    const int j = lane + 64 * t;
    if (j < groups) {
      const uint32_t ent = lut_r[t];
      const uint32_t off = ent & 0xFFFFu, code = ent >> 16;
      const uint32_t w = (uint32_t) * reinterpret_cast<const uint16_t*>(frame + off) |
                         ((uint32_t) * reinterpret_cast<const uint16_t*>(frame + off + NS) << 16);
      const float v0 = denorm1((w >> (8 * (code & 3u))) & 0xFFu, mn, mx);
      const float v1 = denorm1((w >> (8 * ((code >> 2) & 3u))) & 0xFFu, mn, mx);
      const float v2 = denorm1((w >> (8 * ((code >> 4) & 3u))) & 0xFFu, mn, mx);
      const float v3 = denorm1((w >> (8 * ((code >> 6) & 3u))) & 0xFFu, mn, mx);
      if (vec_out && 4 * j + 3 < d) {
        store_f4<NT>(dst + 4 * j, v0, v1, v2, v3);
      } else {  // unaligned rows, and the group that straddles d: never a store at or past d
        dst[4 * j] = v0;
        if (4 * j + 1 < d) dst[4 * j + 1] = v1;
        if (4 * j + 2 < d) dst[4 * j + 2] = v2;
        if (4 * j + 3 < d) dst[4 * j + 3] = v3;
      }
    }
  }

  // ---- index row: lanes < NS / 4 own four values each ------------------------------------------------
  if (idx_row || idx_len) {
    int last = 0;  // 1 + position of this lane's last value != 0.0f (-0.0 == 0.0f, as in np.nonzero)
    if (lane < NS / 4) {
      const uint32_t w = *reinterpret_cast<const uint32_t*>(frame + NS * NS + 4 * lane);
      const float v0 = denorm1(w & 0xFFu, mn, mx), v1 = denorm1((w >> 8) & 0xFFu, mn, mx);
      const float v2 = denorm1((w >> 16) & 0xFFu, mn, mx), v3 = denorm1(w >> 24, mn, mx);
      if (idx_row) {
        float* r = idx_row + e * (int64_t)NS + 4 * lane;
        if (vec_idx) {
          store_f4<NT>(r, v0, v1, v2, v3);
        } else {
          r[0] = v0; r[1] = v1; r[2] = v2; r[3] = v3;
        }
      }
      last = v3 != 0.0f ? 4 * lane + 4 : v2 != 0.0f ? 4 * lane + 3 : v1 != 0.0f ? 4 * lane + 2
                                                                   : v0 != 0.0f ? 4 * lane + 1 : 0;
    }
    if (idx_len) {
      const unsigned long long m = __builtin_amdgcn_ballot_w64(last != 0);
      const int top = m ? 63 - __builtin_clzll(m) : 0;
      const int len = __shfl(last, top, 64);
      if (lane == 0) idx_len[e] = m ? len : 1;
    }
  }
}

// Generic path (every n in 2..128, and frames / rows the fast path's 16-byte accesses cannot take): one
// workgroup per frame, persistent, LDS table of the curve's row-major cell offsets as in k_map_from_2d.
__global__ __launch_bounds__(256) void k_decode_generic(const uint8_t* __restrict__ frame_in, int64_t N, uint32_t n,
                                                        int d, const float* __restrict__ mm, int mm_shared,
                                                        float* __restrict__ out, int64_t out_stride,
                                                        float* __restrict__ idx_row, int32_t* __restrict__ idx_len) {
  extern __shared__ uint16_t dec_cell[];  // d entries: y * n + x < 16384
  __shared__ int s_len;
  for (uint32_t i = threadIdx.x; i < (uint32_t)d; i += blockDim.x) {
    uint32_t x, y;
    d2xy(n, i, x, y);
    dec_cell[i] = (uint16_t)(y * n + x);
  }
  __syncthreads();
  const int64_t fb = (int64_t)(n + 1) * n;
  for (int64_t e = blockIdx.x; e < N; e += gridDim.x) {
    const uint8_t* src = frame_in + e * fb;
    const float* p = mm + (mm_shared ? 0 : 2 * e);
    const float mn = p[0], mx = p[1];
    float* dst = out + e * out_stride;
    for (uint32_t i = threadIdx.x; i < (uint32_t)d; i += blockDim.x) dst[i] = denorm1(src[dec_cell[i]], mn, mx);
    if (idx_row || idx_len) {
      if (threadIdx.x == 0) s_len = 0;
      __syncthreads();
      if (threadIdx.x < n) {
        const float v = denorm1(src[n * n + threadIdx.x], mn, mx);
        if (idx_row) idx_row[e * (int64_t)n + threadIdx.x] = v;
        if (v != 0.0f) atomicMax(&s_len, (int)threadIdx.x + 1);
      }
      __syncthreads();
      if (idx_len && threadIdx.x == 0) idx_len[e] = s_len > 0 ? s_len : 1;
      __syncthreads();
    }
  }
}

template <int NS, bool NT>
static int launch_decode_np(const uint8_t* frame, int64_t N, int d, const float* mm, int mm_shared, float* out,
                            int64_t out_stride, bool vec_out, float* idx_row, bool vec_idx, int32_t* idx_len,
                            hipStream_t s) {
  constexpr int WPB = 2;
  constexpr int64_t kChunk = (int64_t)1 << 30;  // frames per launch: the grid stays below 2^31
  for (int64_t base = 0; base < N; base += kChunk) {
    const int64_t cnt = (N - base) < kChunk ? (N - base) : kChunk;
    const unsigned grid = (unsigned)((cnt + WPB - 1) / WPB);
    hipLaunchKernelGGL((k_decode_np<NS, WPB, NT>), dim3(grid), dim3(64 * WPB), 0, s,
                       frame + base * (int64_t)DecGeo<NS>::FB, cnt, d, mm_shared ? mm : mm + 2 * base, mm_shared,
                       out ? out + base * out_stride : out, out_stride, vec_out,
                       idx_row ? idx_row + base * NS : idx_row, vec_idx, idx_len ? idx_len + base : idx_len);
    HQ_CHECK_LAUNCH();
  }
  return HQ_OK;
}

// store form of the fast path (option decode_nt: 0 plain, 1 non-temporal): the A/B run of tools/ab_decode.py
// decides the default, DESIGN.md §4.1b
constexpr int kDecodeNtDefault = 1;

template <int NS>
static int launch_decode_fast(const uint8_t* frame, int64_t N, int d, const float* mm, int mm_shared, float* out,
                              int64_t out_stride, bool vec_out, float* idx_row, bool vec_idx, int32_t* idx_len,
                              hipStream_t s) {
  if (opt(OPT_DECODE_NT, kDecodeNtDefault) != 0)
    return launch_decode_np<NS, true>(frame, N, d, mm, mm_shared, out, out_stride, vec_out, idx_row, vec_idx, idx_len,
                                      s);
  return launch_decode_np<NS, false>(frame, N, d, mm, mm_shared, out, out_stride, vec_out, idx_row, vec_idx, idx_len,
                                     s);
}

// ------------------------------------------------------------------------------------------------
// round-trip error metrics (core/pipeline.py:257-259) of float32 rows, bit-identical to NumPy:
//   mse = np.mean((o - r) ** 2), mae = np.mean(np.abs(o - r)), max_error = np.max(np.abs(o - r)).
// The differences, squares and absolute values are float32 elementwise; np.mean of a float32 array is
// f32(f64(pairwise f32 sum) / d); np.max has no order.  One thread per row walks NumPy's
// pairwise order serially (np_sum's leaf, split levels deep enough for d <= 2^26): exact, not fast.
// ------------------------------------------------------------------------------------------------
constexpr int kRtMaxD = 1 << 26;

template <typename T, class F>
__device__ __forceinline__ T np_sum_deep(const F& f, int n) {
  if (n <= 128) return T(0) + pw_leaf<T>(f, 0, n);
  return T(0) + pw_rec<20, T>(f, 0, n);  // depth D is exact for n <= 112 * 2^D + 16
}

__global__ __launch_bounds__(64) void k_roundtrip_error(const float* __restrict__ orig, int64_t orig_stride,
                                                        const float* __restrict__ recon, int64_t recon_stride,
                                                        int64_t N, int d, float* __restrict__ out) {
  const int64_t e = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (e >= N) return;
  const float* o = orig + e * orig_stride;
  const float* r = recon + e * recon_stride;
  const Sum2<float> s = np_sum_deep<Sum2<float>>(
      [&](int k) {
        const float df = o[k] - r[k];
        return Sum2<float>(df * df, fabsf(df));
      },
      d);
  float mxe = fabsf(o[0] - r[0]);
  bool nan = mxe != mxe;
  for (int k = 1; k < d; ++k) {
    const float a = fabsf(o[k] - r[k]);
    nan |= a != a;
    mxe = a > mxe ? a : mxe;
  }
  if (nan) mxe = __builtin_nanf("");  // np.max propagates NaN
  out[3 * e + 0] = (float)((double)s.a / (double)d);
  out[3 * e + 1] = (float)((double)s.b / (double)d);
  out[3 * e + 2] = mxe;
}

}  // namespace hq

using namespace hq;

extern "C" {

int hq_dequantize_unmap(const uint8_t* frame, int64_t N, int n, int d, const float* minmax, int mm_shared,
                        float* out, int64_t out_stride, float* idx_row, int32_t* idx_len, hq_stream_t stream) {
  if (!is_pow2(n)) return fail(HQ_E_NOT_POW2, "Dimension must be a power of 2, got %d", n);
  if (n < 2 || n > 128) return fail(HQ_E_UNSUPPORTED, "fused decode supports 2 <= n <= 128, got %d", n);
  if (d < 0 || N < 0 || out_stride < d)
    return fail(HQ_E_INVALID, "bad shape N=%lld d=%d stride=%lld", (long long)N, d, (long long)out_stride);
  if ((int64_t)d > (int64_t)n * n)
    return fail(HQ_E_TOO_MANY, "Too many parameters (%d) for dimensions %dx%d (%d cells)", d, n, n, n * n);
  if (N == 0) return HQ_OK;
  if (d == 0 && !idx_row && !idx_len) return HQ_OK;
  if (!frame || !minmax || (d > 0 && !out)) return fail(HQ_E_INVALID, "null buffer");
  hipStream_t s = (hipStream_t)stream;
  // the fast path's 16-byte frame loads need 16-byte aligned frames; unaligned output rows and index rows
  // stay on it with scalar stores
  const bool fast = !opt_on(OPT_DECODE_GENERIC) && (n == 16 || n == 32 || n == 64) &&
                    (reinterpret_cast<uintptr_t>(frame) & 15) == 0;
  if (fast) {
    const bool vec_out = (reinterpret_cast<uintptr_t>(out) & 15) == 0 && (out_stride % 4 == 0 || N == 1);
    const bool vec_idx = (reinterpret_cast<uintptr_t>(idx_row) & 15) == 0;
    switch (n) {
      case 16: return launch_decode_fast<16>(frame, N, d, minmax, mm_shared, out, out_stride, vec_out, idx_row, vec_idx, idx_len, s);
      case 32: return launch_decode_fast<32>(frame, N, d, minmax, mm_shared, out, out_stride, vec_out, idx_row, vec_idx, idx_len, s);
      case 64: return launch_decode_fast<64>(frame, N, d, minmax, mm_shared, out, out_stride, vec_out, idx_row, vec_idx, idx_len, s);
    }
  }
  const size_t lds = (size_t)(d > 0 ? d : 1) * sizeof(uint16_t);
  const int grid = persistent_grid((const void*)k_decode_generic, 256, lds, N);
  hipLaunchKernelGGL(k_decode_generic, dim3(grid), dim3(256), lds, s, frame, N, (uint32_t)n, d, minmax, mm_shared,
                     out, out_stride, idx_row, idx_len);
  HQ_CHECK_LAUNCH();
  return HQ_OK;
}

int hq_roundtrip_error(const float* orig, int64_t orig_stride, const float* recon, int64_t recon_stride, int64_t N,
                       int d, float* out, hq_stream_t stream) {
  if (N < 0 || d < 1 || orig_stride < d || recon_stride < d)
    return fail(HQ_E_INVALID, "bad shape N=%lld d=%d strides=%lld, %lld", (long long)N, d, (long long)orig_stride,
                (long long)recon_stride);
  if (d > kRtMaxD) return fail(HQ_E_UNSUPPORTED, "round-trip metrics support d <= %d, got %d", kRtMaxD, d);
  if (N == 0) return HQ_OK;
  if (!orig || !recon || !out) return fail(HQ_E_INVALID, "null buffer");
  const int64_t grid = (N + 63) / 64;
  if (grid > 0x7FFFFFFF) return fail(HQ_E_UNSUPPORTED, "too many rows: %lld", (long long)N);
  hipLaunchKernelGGL(k_roundtrip_error, dim3((unsigned)grid), dim3(64), 0, (hipStream_t)stream, orig, orig_stride,
                     recon, recon_stride, N, d, out);
  HQ_CHECK_LAUNCH();
  return HQ_OK;
}

}  // extern "C"
