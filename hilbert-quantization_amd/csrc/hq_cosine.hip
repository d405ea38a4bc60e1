// hq_cosine.hip — dense frame similarity on the matrix cores (north star: "the
// frame similarity as a batched L2/dot over N x (side x side) images — MFMA for the dense
// query x corpus contraction").
//
// Reference: rag/search/engine.py:622-660 _calculate_embedding_cosine_similarity — flatten, truncate
// to the common length, dot / (|a| |b|), (cos + 1) / 2, 0.0 when a norm is 0 — applied to every
// (query, stored frame) pair by the RAG search loops (:503-507, :1025-1051).  The reference computes
// in float32 through BLAS (sdot / snrm2 order), so scores agree within the north star's 1e-5, not bit
// for bit (DESIGN.md §4.5 has the error budget; profiles/cos_error_bounds.txt the error measured per row family:
// up to 3.2e-6 for same-sign rows at K = 16384).  Every finite float32 row gives finite scores, subnormal rows
// included; a row with a NaN or inf gets inv = 0 and scores 0.0 (include/hq_mi355x.h).
//
// Layout (hq_cos_prepare, once per corpus / query batch): every row x is scaled by a power of two s
// (max |s x| in [0.5, 1)) and split as hi = f16(s x), lo = f16(s x - hi), Kp = K rounded up to 32, stored
// as 1 KiB MFMA operand fragments (16-row tile, K step of 32, plane hi / lo: see cos_frag), plus inv[row] =
// 1 / (s |x|) (f64 norm of the original values; 0 for a zero row).  dot(a, b) = (hi_a.hi_b + hi_a.lo_b +
// lo_a.hi_b) / (s_a s_b) + O(2^-22 |a||b|).
//
// GEMM (default k_cos_t<3, 1, 1>): workgroup = 8 waves, tile 128 queries x 384 frames, wave w = all 128
// queries x frames 48 w .. + 47 (8 x 3 tiles of v_mfma_f32_16x16x32_f16 x 3: hi.hi, hi.lo, lo.hi), K steps
// of 32.  Query fragments go through LDS (register-staged, two stages, read by every wave); frame
// fragments, each used by one wave only, go straight from global memory into that wave's VGPRs one K step
// ahead.  Ping-pong: the two waves of every SIMD run one barrier phase apart (memory phase / 72 MFMAs).
// XCD-aware block order: the query tiles of one frame tile run back to back on one XCD, so the frame tile
// is read from HBM once.  Epilogue: (acc * inv_q * inv_c + 1) / 2, f64 stores.  A/B forms (option
// cos_kernel): the LDS-DMA kernel k_cos_g3 (ping-pong / lockstep) and the register-staged
// k_cos_mfma on the row-major layout, and other k_cos_t tiles / prefetch distances / epilogues.
//
// Fused top-k (hq_cos_topk): k_cos_t<3, 1, 1, 4> keeps the K loop and selects the best k
// passing frames of every (query, 384-frame tile) in its epilogue instead of storing scores; k_cos_topk_merge
// reduces the tiles' sorted lists 64 at a time.  Same accumulators, same epilogue expression, same total order
// as hq_select_topk on the dense matrix: identical ids, order and score bits, memory O(Q k N / 384).
//
// Compressed-domain search (hq_cosq_*; the section before the last of this file): the same tile, ping-pong,
// top-k epilogue and merge on the store's own u8 frames + (min, max), contracted exactly by v_mfma_i32_16x16x64_i8.
// Float32 queries against that u8 corpus (hq_cosqf_*; the last section): the query as three int8
// digit planes of a 24-bit fixed-point row, three exact int32 sums per pair, the same epilogue pieces.  Both int8
// routes run one GEMM template, k_cosq_t<NP, EP> (NP query planes), and all three fused routes one host driver
// (cos_topk_run).
#include "hq_common.h"

#include <stdlib.h>
#include <string.h>

namespace hq {

typedef _Float16 h8 __attribute__((ext_vector_type(8)));
typedef float f4 __attribute__((ext_vector_type(4)));
typedef double d2v __attribute__((ext_vector_type(2)));

constexpr int kCosT = 128;                 // tile rows (queries) = tile cols (frames)
constexpr int kCosK = 32;                  // K per step
constexpr int kCosRow = 40;                // LDS halves per tile row (32 + 8 pad: 80 B)

// ---- prepare: scale, split, inverse norm ------------------------------------------------------------
__global__ __launch_bounds__(256) void k_cos_prepare(const float* __restrict__ X, int64_t N, int64_t ld, int K,
                                                     int Kp, int64_t rows_out, _Float16* __restrict__ X16,
                                                     double* __restrict__ inv) {
  // one wave per row
  const int lane = threadIdx.x & 63;
  const int64_t w0 = ((int64_t)blockIdx.x * blockDim.x + threadIdx.x) >> 6;
  const int64_t nw = ((int64_t)gridDim.x * blockDim.x) >> 6;
  for (int64_t r = w0; r < rows_out; r += nw) {
    _Float16* hi = X16 + r * 2 * Kp;
    _Float16* lo = hi + Kp;
    if (r >= N) {  // pad rows: zeros, inv 0
      for (int k = lane; k < Kp; k += 64) hi[k] = lo[k] = (_Float16)0.0f;
      if (lane == 0) inv[r] = 0.0;
      continue;
    }
    const float* x = X + r * ld;
    float amax = 0.0f;
    double ss = 0.0;
    for (int k = lane; k < K; k += 64) {
      const float v = x[k];
      amax = fmaxf(amax, fabsf(v));
      ss = fma((double)v, (double)v, ss);
    }
    for (int o = 32; o > 0; o >>= 1) {
      amax = fmaxf(amax, __shfl_xor(amax, o, 64));
      ss += __shfl_xor(ss, o, 64);
    }
    int e = 0;
    if (amax > 0.0f) frexpf(amax, &e);  // amax = m 2^e, m in [0.5, 1)
    // s x = ldexpf(x, -e) in (-1, 1): exact for every finite row (s = 2^-e itself overflows float32 for a
    // subnormal amax, e <= -128)
    for (int k = lane; k < Kp; k += 64) {
      const float v = k < K ? ldexpf(x[k], -e) : 0.0f;
      const _Float16 h = (_Float16)v;
      hi[k] = h;
      lo[k] = (_Float16)(v - (float)h);
    }
    if (lane == 0) inv[r] = ss > 0.0 ? ldexp(1.0 / sqrt(ss), e) : 0.0;
  }
}

// ---- tiled fragment layout (default) ------------------------------------------------------------------
// Fragment (16-row tile t, K step kb, plane p) = 512 halves (1 KiB) at ((t KB + kb) 2 + p) 512, KB = Kp / 32;
// lane 16 g + j holds row 16 t + j, k = 32 kb + 8 g .. + 7 — exactly the v_mfma_f32_16x16x32_f16 A / B
// operand, so one fragment is one contiguous 1 KiB wave load (16 B per lane) and, staged in LDS
// lane-linearly, one bank-conflict-free ds_read_b128.
__device__ __forceinline__ int64_t cos_frag(int64_t t, int kb, int KB, int p) {
  return ((t * KB + kb) * 2 + p) * 512;
}

__global__ __launch_bounds__(1024) void k_cos_prepare_tiled(const float* __restrict__ X, int64_t N, int64_t ld, int K,
                                                            int Kp, int64_t rows_out, _Float16* __restrict__ X16,
                                                            double* __restrict__ inv) {
  // one 16-wave workgroup per 16-row tile: wave w takes row w's statistics in k_cos_prepare's lane-strided
  // order (same scale and inverse-norm bits), then the waves split the tile's K steps; per K step lane
  // 16 g + j converts row j's values 8 g .. 8 g + 7, so every fragment leaves as one contiguous 1 KiB wave
  // store per plane
  __shared__ int sc[16];  // the rows' scale exponents e (s = 2^-e)
  const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6, j = lane & 15, g = lane >> 4;
  const int KB = Kp / kCosK;
  // blockIdx.y: one of gridDim.y parts of the K steps (small batches: more workgroups per tile, each
  // recomputing the tile's statistics)
  const int per = (KB + gridDim.y - 1) / gridDim.y;
  const int kb0 = blockIdx.y * per, kb1 = kb0 + per < KB ? kb0 + per : KB;
  for (int64_t t = blockIdx.x; t < rows_out / 16; t += gridDim.x) {
    const int64_t r0 = 16 * t + wv;
    if (r0 >= N) {  // pad rows: zeros, inv 0
      if (lane == 0) {
        sc[wv] = 0;
        if (blockIdx.y == 0) inv[r0] = 0.0;
      }
    } else {
      const float* x = X + r0 * ld;
      float amax = 0.0f;
      double ss = 0.0;
      for (int k = lane; k < K; k += 64) {
        const float v = x[k];
        amax = fmaxf(amax, fabsf(v));
        ss = fma((double)v, (double)v, ss);
      }
      for (int o = 32; o > 0; o >>= 1) {
        amax = fmaxf(amax, __shfl_xor(amax, o, 64));
        ss += __shfl_xor(ss, o, 64);
      }
      int e = 0;
      if (amax > 0.0f) frexpf(amax, &e);  // amax = m 2^e, m in [0.5, 1)
      if (lane == 0) {
        sc[wv] = e;
        if (blockIdx.y == 0) inv[r0] = ss > 0.0 ? ldexp(1.0 / sqrt(ss), e) : 0.0;
      }
    }
    __syncthreads();
    const int64_t r = 16 * t + j;
    const int my_e = sc[j];
    const float* x = X + (r < N ? r : 0) * ld;
    for (int kb = kb0 + wv; kb < kb1; kb += 16) {
      h8 hi, lo;
#pragma unroll
      for (int u = 0; u < 8; ++u) {
        const int k = kCosK * kb + 8 * g + u;
        const float v = (r < N && k < K) ? ldexpf(x[k], -my_e) : 0.0f;  // exact (see k_cos_prepare)
        const _Float16 h = (_Float16)v;
        hi[u] = h;
        lo[u] = (_Float16)(v - (float)h);
      }
      _Float16* f = X16 + cos_frag(t, kb, KB, 0) + 8 * lane;
      *reinterpret_cast<h8*>(f) = hi;
      *reinterpret_cast<h8*>(f + 512) = lo;
    }
    __syncthreads();  // sc is rewritten by the next tile
  }
}

// ---- GEMM + epilogue ---------------------------------------------------------------------------------
struct CosArgs {
  const _Float16* A;  // queries [Qp, 2, Kp]
  const _Float16* B;  // frames  [Np, 2, Kp]
  const double* ia;   // [Qp]
  const double* ib;   // [Np]
  int Q;
  int64_t N;
  int Kp;
  int qtiles;
  int64_t ntiles;
  double* out;  // [Q, N]
  float* outf;  // [Q, N] float32 scores (hq_cos_scores_mfma_f32; k_cos_t EP 3): the reference's precision
  // hq_cos_topk (k_cos_t EP 4): the best tk_k passing frames of every (query, frame tile), [Q, ntiles, tk_k]
  double* tk_s;
  int64_t* tk_id;      // frame rows (no id_base), -1 = empty
  uint64_t* tk_hint;   // [Q] running threshold keys (cos_key), or NULL
  double tk_thr;
  int tk_mode;         // 0 none, 1 >= tk_thr, 2 > tk_thr
  int tk_k;
};

// ---- top-k pieces of the fused frame search (hq_cos_topk) ---------------------------------------------
// The total order of hq_select_topk: score descending, id ascending.
__device__ __forceinline__ bool cos_better(double s, int64_t id, double s2, int64_t id2) {
  return s > s2 || (s == s2 && id < id2);
}
// order-preserving u64 key of a score (the sign-flip map: (cs + 1) / 2 can be a hair below 0); 0 is below
// the key of every number, so a zeroed hint is "none"
__device__ __forceinline__ uint64_t cos_key(double s) {
  const uint64_t b = (uint64_t)__double_as_longlong(s);
  return (b >> 63) ? ~b : b | 0x8000000000000000ull;
}
// wave arg-max in the total order (id < 0: empty); every lane ends with the same pair
__device__ __forceinline__ void cos_wave_best(double& bs, int64_t& bi) {
  for (int o = 1; o < 64; o <<= 1) {
    const double s2 = __shfl_xor(bs, o, 64);
    const int64_t i2 = __shfl_xor(bi, o, 64);
    if (i2 >= 0 && (bi < 0 || cos_better(s2, i2, bs, bi))) { bs = s2; bi = i2; }
  }
}
// The same for the epilogue's (score, column) pairs, without LDS round trips (the per-round critical path of
// the top-k epilogue): four DPP steps (xor 1, xor 2, half-row mirror, row mirror) leave every 16-lane row
// with its best pair, four readlanes combine the rows.  The order is total and the columns distinct, so the
// shape of the reduction does not change the result.
__device__ __forceinline__ void cos_take(double& bs, int& bi, double s2, int i2) {
  if (i2 >= 0 && (bi < 0 || s2 > bs || (s2 == bs && i2 < bi))) { bs = s2; bi = i2; }
}
template <int CTRL>
__device__ __forceinline__ void cos_dpp_best(double& bs, int& bi) {
  const int lo = __builtin_amdgcn_update_dpp(0, __double2loint(bs), CTRL, 0xF, 0xF, false);
  const int hi = __builtin_amdgcn_update_dpp(0, __double2hiint(bs), CTRL, 0xF, 0xF, false);
  const int i2 = __builtin_amdgcn_update_dpp(0, bi, CTRL, 0xF, 0xF, false);
  cos_take(bs, bi, __hiloint2double(hi, lo), i2);
}
__device__ __forceinline__ void cos_wave_best(double& bs, int& bi) {
  cos_dpp_best<0xB1>(bs, bi);
  cos_dpp_best<0x4E>(bs, bi);
  cos_dpp_best<0x141>(bs, bi);
  cos_dpp_best<0x140>(bs, bi);
  const int lo = __double2loint(bs), hi = __double2hiint(bs), e = bi;
  bs = __hiloint2double(__builtin_amdgcn_readlane(hi, 0), __builtin_amdgcn_readlane(lo, 0));
  bi = __builtin_amdgcn_readlane(e, 0);
#pragma unroll
  for (int l = 16; l < 64; l += 16)
    cos_take(bs, bi, __hiloint2double(__builtin_amdgcn_readlane(hi, l), __builtin_amdgcn_readlane(lo, l)),
             __builtin_amdgcn_readlane(e, l));
}

// One query of one workgroup tile, one wave: the TN staged scores of row `row` (st: 8 wave slices of
// 16 x TN / 8 f64, the wide epilogue's staging) are TN / 64 per lane, candidate e = lane + 64 u = frame
// nt TN + e.  Frames n >= N (the clamped last tile re-reads real rows) and those failing the threshold test
// are masked; then tk_k arg-max rounds, each pick leaving its lane's set, write (score, frame) to the fixed
// slab position [q][nt][0 .. tk_k), padded with -inf / -1.
// Running threshold (hint != NULL): hint[q] is the key of some tile's k-th pick, so k passing frames score
// at or above it; candidates strictly below it leave the set before the first round (they cannot reach the
// merged top k; ties are kept), the rounds end when the set is empty, and a tile that found all k raises it.
// Relaxed, no ordering: a stale read is only lower, so the merged result does not depend on timing.
template <int TN>
__device__ __forceinline__ void cos_topk_row(const double* __restrict__ st, int row, int64_t q, int64_t nt,
                                             const CosArgs& a) {
  constexpr int C = TN / 64, WC = TN / 8;  // candidates per lane, frames per wave slice
  const int lane = threadIdx.x & 63;
  const int k = a.tk_k;
  uint64_t hint = 0;
  if (a.tk_hint) hint = __hip_atomic_load(a.tk_hint + q, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
  double s[C];
  unsigned live = 0;
#pragma unroll
  for (int u = 0; u < C; ++u) {
    const int e = lane + 64 * u;
    const double v = st[(e / WC) * (16 * WC) + row * WC + e % WC];
    const bool pass = a.tk_mode == 0 || (a.tk_mode == 1 ? v >= a.tk_thr : v > a.tk_thr);
    s[u] = v;
    if (nt * TN + e < a.N && pass && cos_key(v) >= hint) live |= 1u << u;  // strictly below the hint: out
  }
  double* os = a.tk_s + (q * a.ntiles + nt) * k;
  int64_t* oi = a.tk_id + (q * a.ntiles + nt) * k;
  int j = 0;
  double bs = 0.0;
  for (; j < k; ++j) {
    if (__ballot(live != 0) == 0) break;  // nothing left at or above the hint: no reduction for this round
    bs = 0.0;
    int be = -1;
#pragma unroll
    for (int u = 0; u < C; ++u)  // e ascends with u: strict > keeps the lowest frame of a tie
      if (((live >> u) & 1u) && (be < 0 || s[u] > bs)) { bs = s[u]; be = lane + 64 * u; }
    cos_wave_best(bs, be);
    if (lane == 0) {
      os[j] = bs;
      oi[j] = nt * TN + be;
    }
    if ((be & 63) == lane) live &= ~(1u << (be >> 6));
  }
  if (j == k) {
    if (a.tk_hint && lane == 0)
      __hip_atomic_fetch_max(a.tk_hint + q, cos_key(bs), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
  } else {
    for (int jj = j + lane; jj < k; jj += 64) {
      os[jj] = -__builtin_huge_val();
      oi[jj] = -1;
    }
  }
}

// Merge stage of hq_cos_topk: list g of query q (out) = the best k of lists [64 g, 64 g + 64) of the P the
// previous stage left (each sorted in the total order, -1 padded).  One wave per output list, lane l walks
// list 64 g + l: its head is the lane's candidate, the wave arg-max takes the best head, that lane steps to
// its next entry.  ids leave with id_add added (id_base in the last stage, 0 before it).
__global__ __launch_bounds__(64) void k_cos_topk_merge(int Q, int64_t P, int64_t P2, int k, int64_t id_add,
                                                       const double* __restrict__ i_s,
                                                       const int64_t* __restrict__ i_id, double* __restrict__ o_s,
                                                       int64_t* __restrict__ o_id) {
  const int lane = threadIdx.x;
  for (int64_t t = blockIdx.x; t < (int64_t)Q * P2; t += gridDim.x) {
    const int64_t q = t / P2, p = (t % P2) * 64 + lane;
    const double* ls = i_s + (q * P + p) * k;
    const int64_t* li = i_id + (q * P + p) * k;
    int cur = 0;
    double hs = 0.0;
    int64_t hid = -1;
    if (p < P) {
      hid = li[0];
      if (hid >= 0) hs = ls[0];
    }
    double* os = o_s + t * k;
    int64_t* oi = o_id + t * k;
    for (int j = 0; j < k; ++j) {
      double bs = hs;
      int64_t bi = hid;
      cos_wave_best(bs, bi);
      if (bi < 0) {
        for (int jj = j + lane; jj < k; jj += 64) {
          os[jj] = -__builtin_huge_val();
          oi[jj] = -1;
        }
        break;
      }
      if (lane == 0) {
        os[j] = bs;
        oi[j] = bi + id_add;
      }
      if (hid == bi) {  // ids are distinct: exactly one lane
        ++cur;
        hid = cur < k ? li[cur] : -1;
        if (hid >= 0) hs = ls[cur];
      }
    }
  }
}

// Register-staged baseline.  TQ = query rows per workgroup tile; frames per tile kCosT = 128.  LDS per
// buffer: (2 TQ + 2 * 128) rows of 80 B.
template <int TQ>
__global__ __launch_bounds__(256) void k_cos_mfma(CosArgs a) {
  extern __shared__ __attribute__((aligned(16))) uint8_t cos_smem[];
  constexpr int kBuf = (2 * TQ + 2 * kCosT) * kCosRow;  // halves per buffer
  _Float16* lds0 = reinterpret_cast<_Float16*>(cos_smem);
  // plane p of buffer b: A hi / A lo (TQ rows), B hi / B lo (128 rows)
  auto plane = [&](int b, int p) -> _Float16* {
    return lds0 + b * kBuf + (p < 2 ? p * TQ * kCosRow : 2 * TQ * kCosRow + (p - 2) * kCosT * kCosRow);
  };
  const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
  // XCD-aware order: blocks with equal (blockIdx % 8) share an XCD; the query tiles of a frame tile
  // are consecutive within one XCD's sequence
  const int64_t blk = blockIdx.x;
  const int64_t xcd = blk & 7, slot = blk >> 3;
  const int qt = (int)(slot % a.qtiles);
  const int64_t nt = xcd + 8 * (slot / a.qtiles);
  if (nt >= a.ntiles) return;
  const int64_t q0 = (int64_t)qt * TQ, n0 = nt * kCosT;
  const int Kp = a.Kp;
  // global -> register staging: A planes TQ rows, B planes 128 rows, 4 chunks of 16 B per row
  constexpr int CA = TQ * 4 / 256, CB = kCosT * 4 / 256;  // chunks per thread per plane
  h8 sa[2][CA], sb[2][CB];
  auto load_step = [&](int k0) {
#pragma unroll
    for (int p = 0; p < 2; ++p) {
#pragma unroll
      for (int i = 0; i < CA; ++i) {
        const int c = tid + 256 * i, row = c >> 2, seg = c & 3;
        sa[p][i] = *reinterpret_cast<const h8*>(a.A + ((q0 + row) * 2 + p) * (int64_t)Kp + k0 + 8 * seg);
      }
#pragma unroll
      for (int i = 0; i < CB; ++i) {
        const int c = tid + 256 * i, row = c >> 2, seg = c & 3;
        sb[p][i] = *reinterpret_cast<const h8*>(a.B + ((n0 + row) * 2 + p) * (int64_t)Kp + k0 + 8 * seg);
      }
    }
  };
  auto store_step = [&](int buf) {
#pragma unroll
    for (int p = 0; p < 2; ++p) {
#pragma unroll
      for (int i = 0; i < CA; ++i) {
        const int c = tid + 256 * i, row = c >> 2, seg = c & 3;
        *reinterpret_cast<h8*>(plane(buf, p) + row * kCosRow + 8 * seg) = sa[p][i];
      }
#pragma unroll
      for (int i = 0; i < CB; ++i) {
        const int c = tid + 256 * i, row = c >> 2, seg = c & 3;
        *reinterpret_cast<h8*>(plane(buf, 2 + p) + row * kCosRow + 8 * seg) = sb[p][i];
      }
    }
  };
  // wave tile: queries (TQ/2) * (wv >> 1) .. + TQ/2, frames 64 * (wv & 1) .. +64
  constexpr int MI = TQ / 32;  // 16-row query tiles per wave
  const int wr = (TQ / 2) * (wv >> 1), wc = 64 * (wv & 1);
  const int fr = lane & 15, fk = 8 * (lane >> 4);
  f4 acc[MI][4];
#pragma unroll
  for (int i = 0; i < MI; ++i)
#pragma unroll
    for (int j = 0; j < 4; ++j) acc[i][j] = f4{0.f, 0.f, 0.f, 0.f};

  const int steps = Kp / kCosK;
  load_step(0);
  store_step(0);
  __syncthreads();
  for (int s = 0; s < steps; ++s) {
    const int buf = s & 1;
    if (s + 1 < steps) load_step((s + 1) * kCosK);
    h8 bh[4], bl[4];
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      bh[j] = *reinterpret_cast<const h8*>(plane(buf, 2) + (wc + 16 * j + fr) * kCosRow + fk);
      bl[j] = *reinterpret_cast<const h8*>(plane(buf, 3) + (wc + 16 * j + fr) * kCosRow + fk);
    }
#pragma unroll
    for (int i = 0; i < MI; ++i) {
      const h8 ah = *reinterpret_cast<const h8*>(plane(buf, 0) + (wr + 16 * i + fr) * kCosRow + fk);
      const h8 al = *reinterpret_cast<const h8*>(plane(buf, 1) + (wr + 16 * i + fr) * kCosRow + fk);
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        // D[query row][frame col]: A operand = queries, B operand = frames, so each output row's 16
        // frames are 16 consecutive lanes (128-byte stores)
        acc[i][j] = __builtin_amdgcn_mfma_f32_16x16x32_f16(ah, bh[j], acc[i][j], 0, 0, 0);
        acc[i][j] = __builtin_amdgcn_mfma_f32_16x16x32_f16(ah, bl[j], acc[i][j], 0, 0, 0);
        acc[i][j] = __builtin_amdgcn_mfma_f32_16x16x32_f16(al, bh[j], acc[i][j], 0, 0, 0);
      }
    }
    if (s + 1 < steps) store_step(buf ^ 1);
    __syncthreads();
  }
  // epilogue: lane holds queries 4 (lane >> 4) + r of each 16-query tile, frame lane & 15
#pragma unroll
  for (int i = 0; i < MI; ++i)
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      const int64_t q = q0 + wr + 16 * i + 4 * (lane >> 4) + r;
      if (q >= a.Q) continue;
      const double iq = a.ia[q];
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        const int64_t n = n0 + wc + 16 * j + fr;
        if (n >= a.N) continue;
        const double ic = a.ib[n];
        const double cs = (double)acc[i][j][r] * iq * ic;
        a.out[q * a.N + n] = (iq != 0.0 && ic != 0.0) ? (cs + 1.0) / 2.0 : 0.0;
      }
    }
}

// LDS-DMA staging: global_load_lds_dwordx4 writes each staged tile straight into LDS (no staging VGPRs,
// no ds_write).  The DMA destination is lane-linear (one wave instruction = 1 KiB = 16 rows of 64 B),
// so rows are unpadded and the bank spread comes from an XOR swizzle of the 16-byte segment applied
// on the SOURCE address and undone on the fragment read: physical seg = logical seg ^ kSw[(row >> 2) & 3].
// kSw = {0, 2, 3, 1} puts the sixteen rows of every ds_read_b128 lane group (lanes {0-3, 12-15,
// 20-27}, ... — MI355X_MICROARCH.md §LDS) on sixteen distinct 4-bank groups.
__device__ __forceinline__ int cos_sw(int g) { return (0x78 >> (2 * g)) & 3; }  // {0, 2, 3, 1}

// Three-stage LDS-DMA pipeline: tile 128 queries x TN frames, TN / 32 waves (each 64 x 64), K steps of
// 32, three LDS stages so the DMA of step s + 2 is in flight while step s computes (two steps of MFMA
// cover the HBM latency of the streamed frame rows).  The DMAs are inline asm (hipcc would otherwise
// drain them with vmcnt(0) at every barrier); each wave retires its own pieces of a stage with a
// counted vmcnt (the PW pieces of the next stage stay in flight) and an s_barrier publishes it.
// PP = 0: all waves in lockstep, one barrier per K step; PP = 1: ping-pong (below).
template <int TN, int PP, bool NTS = true>
__global__ __launch_bounds__(TN * 2) __attribute__((amdgpu_waves_per_eu(1, 2))) void k_cos_g3(CosArgs a, int64_t np_rows) {
  extern __shared__ __attribute__((aligned(16))) uint8_t cos_smem[];
  constexpr int TQ = 128, NW = TN / 32, kRow = kCosK, ST = 3;
  constexpr int kBuf = (2 * TQ + 2 * TN) * kRow;  // halves per stage
  constexpr int SA = TQ / 16, SB = TN / 16, NP = 2 * SA + 2 * SB, PW = NP / NW;
  static_assert(NP % NW == 0 && PW < 16, "pieces per wave");
  _Float16* lds0 = reinterpret_cast<_Float16*>(cos_smem);
  const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
  const int64_t blk = blockIdx.x;
  const int64_t xcd = blk & 7, slot = blk >> 3;
  const int qt = (int)(slot % a.qtiles);
  const int64_t nt = xcd + 8 * (slot / a.qtiles);
  if (nt >= a.ntiles) return;
  const int64_t q0 = (int64_t)qt * TQ, n0 = nt * TN;
  const int Kp = a.Kp;
  const int lrow = lane >> 2;
  const int lseg = (lane & 3) ^ cos_sw((lane >> 4) & 3);
  const _Float16* src[PW];
  uint32_t dst[PW];  // LDS byte address of the piece in stage 0
  const uint32_t lbase = (uint32_t)(uintptr_t)(__attribute__((address_space(3))) void*)lds0;
#pragma unroll
  for (int t = 0; t < PW; ++t) {
    const int i = wv + NW * t;
    int p, slab;
    if (i < 2 * SA) { p = i / SA; slab = i % SA; }
    else { p = 2 + (i - 2 * SA) / SB; slab = (i - 2 * SA) % SB; }
    const int64_t row = (int64_t)slab * 16 + lrow;
    const _Float16* base;
    if (p < 2) base = a.A + ((q0 + row) * 2 + p) * (int64_t)Kp;
    else {
      const int64_t rg = n0 + row < np_rows ? n0 + row : np_rows - 1;  // last tile may pass the padded rows
      base = a.B + (rg * 2 + (p - 2)) * (int64_t)Kp;
    }
    src[t] = base + 8 * lseg;
    const int off = (p < 2 ? p * TQ * kRow : 2 * TQ * kRow + (p - 2) * TN * kRow) + slab * 16 * kRow;
    dst[t] = __builtin_amdgcn_readfirstlane(lbase + 2 * off);
  }
  auto piece = [&](int t, int k0, int stage) {
    uint32_t keep;
    const _Float16* g = src[t] + k0;
    const uint32_t d = dst[t] + stage * (2 * kBuf);
    asm volatile("s_mov_b32 %0, m0\n\ts_mov_b32 m0, %2\n\ts_nop 0\n\tglobal_load_lds_dwordx4 %1, off\n\ts_mov_b32 m0, %0"
                 : "=&s"(keep) : "v"(g), "s"(d) : "memory");
  };
  auto issue = [&](int k0, int stage) {
#pragma unroll
    for (int t = 0; t < PW; ++t) piece(t, k0, stage);
  };
  const int wr = 64 * (wv & 1), wc = 64 * (wv >> 1);
  const int fr = lane & 15;
  const int rseg = 8 * ((lane >> 4) ^ cos_sw(fr >> 2));
  f4 acc[4][4];
#pragma unroll
  for (int i = 0; i < 4; ++i)
#pragma unroll
    for (int j = 0; j < 4; ++j) acc[i][j] = f4{0.f, 0.f, 0.f, 0.f};

  const int steps = Kp / kCosK;
  issue(0, 0);
  if (steps > 1) issue(kCosK, 1);
  int stage = 0;
  if constexpr (PP) {
    // Ping-pong: waves w and w + 4 share a SIMD; group 1 (waves 4-7) runs one barrier phase behind
    // group 0, so on every SIMD one wave issues its fragment reads + DMA while the other runs MFMAs.
    // Phases per K step: memory (DMA of step s + 2, 16 ds_read_b128, lgkmcnt(0)) then compute (48
    // MFMA), each closed by one block barrier.  Stage s + 1 is published at barrier 2s + 2: group 0
    // reaches it after computing step s, group 1 after its memory phase of step s; both retire it
    // with vmcnt(PW) (only the just-issued stage s + 2 stays in flight).  The lgkmcnt(0) before each
    // memory-phase barrier retires the reads of a stage before the other group's DMA may overwrite it.
    const int grp = __builtin_amdgcn_readfirstlane(wv >> 2);
    if (steps > 1) asm volatile("s_waitcnt vmcnt(%0)\n\ts_barrier" ::"n"(PW) : "memory");
    else asm volatile("s_waitcnt vmcnt(0)\n\ts_barrier" ::: "memory");
    if (grp) asm volatile("s_barrier" ::: "memory");
    for (int s = 0; s < steps; ++s) {
      if (s + 2 < steps) issue((s + 2) * kCosK, stage == 0 ? 2 : stage - 1);
      const _Float16* pA = lds0 + stage * kBuf;
      const _Float16* pB = pA + 2 * TQ * kRow;
      h8 bh[4], bl[4], ah[4], al[4];
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        bh[j] = *reinterpret_cast<const h8*>(pB + (wc + 16 * j + fr) * kRow + rseg);
        bl[j] = *reinterpret_cast<const h8*>(pB + TN * kRow + (wc + 16 * j + fr) * kRow + rseg);
      }
#pragma unroll
      for (int i = 0; i < 4; ++i) {
        ah[i] = *reinterpret_cast<const h8*>(pA + (wr + 16 * i + fr) * kRow + rseg);
        al[i] = *reinterpret_cast<const h8*>(pA + TQ * kRow + (wr + 16 * i + fr) * kRow + rseg);
      }
      __builtin_amdgcn_sched_barrier(0);
      if (grp) {
        if (s + 2 < steps) asm volatile("s_waitcnt vmcnt(%0) lgkmcnt(0)\n\ts_barrier" ::"n"(PW) : "memory");
        else asm volatile("s_waitcnt vmcnt(0) lgkmcnt(0)\n\ts_barrier" ::: "memory");
      } else {
        asm volatile("s_waitcnt lgkmcnt(0)\n\ts_barrier" ::: "memory");
      }
      __builtin_amdgcn_sched_barrier(0);
#pragma unroll
      for (int i = 0; i < 4; ++i) {
#pragma unroll
        for (int j = 0; j < 4; ++j) {
          acc[i][j] = __builtin_amdgcn_mfma_f32_16x16x32_f16(ah[i], bh[j], acc[i][j], 0, 0, 0);
          acc[i][j] = __builtin_amdgcn_mfma_f32_16x16x32_f16(ah[i], bl[j], acc[i][j], 0, 0, 0);
          acc[i][j] = __builtin_amdgcn_mfma_f32_16x16x32_f16(al[i], bh[j], acc[i][j], 0, 0, 0);
        }
      }
      __builtin_amdgcn_sched_barrier(0);
      if (!grp) {
        if (s + 2 < steps) asm volatile("s_waitcnt vmcnt(%0)\n\ts_barrier" ::"n"(PW) : "memory");
        else asm volatile("s_waitcnt vmcnt(0)\n\ts_barrier" ::: "memory");
      } else {
        asm volatile("s_barrier" ::: "memory");
      }
      __builtin_amdgcn_sched_barrier(0);
      stage = stage == ST - 1 ? 0 : stage + 1;
    }
    if (!grp) asm volatile("s_barrier" ::: "memory");  // group 1's extra barrier: equal counts per wave
  } else
  for (int s = 0; s < steps; ++s) {
    // retire this wave's pieces of stage s (those of s + 1 may stay in flight), then publish
    if (s + 1 < steps) asm volatile("s_waitcnt vmcnt(%0)\n\ts_barrier" ::"n"(PW) : "memory");
    else asm volatile("s_waitcnt vmcnt(0)\n\ts_barrier" ::: "memory");
    if (s + 2 < steps) issue((s + 2) * kCosK, stage == 0 ? 2 : stage - 1);
    const _Float16* pl = lds0 + stage * kBuf;
    const _Float16* pA = pl;
    const _Float16* pB = pl + 2 * TQ * kRow;
    // all sixteen fragments first (A rows 0-1 and B, then A rows 2-3 behind the first MFMAs); the
    // scheduling barriers keep the compiler from re-serialising the reads against the MFMAs
    h8 bh[4], bl[4], ah[4], al[4];
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      bh[j] = *reinterpret_cast<const h8*>(pB + (wc + 16 * j + fr) * kRow + rseg);
      bl[j] = *reinterpret_cast<const h8*>(pB + TN * kRow + (wc + 16 * j + fr) * kRow + rseg);
    }
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      ah[i] = *reinterpret_cast<const h8*>(pA + (wr + 16 * i + fr) * kRow + rseg);
      al[i] = *reinterpret_cast<const h8*>(pA + TQ * kRow + (wr + 16 * i + fr) * kRow + rseg);
    }
    __builtin_amdgcn_sched_barrier(0);
#pragma unroll
    for (int i = 0; i < 4; ++i) {
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        acc[i][j] = __builtin_amdgcn_mfma_f32_16x16x32_f16(ah[i], bh[j], acc[i][j], 0, 0, 0);
        acc[i][j] = __builtin_amdgcn_mfma_f32_16x16x32_f16(ah[i], bl[j], acc[i][j], 0, 0, 0);
        acc[i][j] = __builtin_amdgcn_mfma_f32_16x16x32_f16(al[i], bh[j], acc[i][j], 0, 0, 0);
      }
    }
    __builtin_amdgcn_sched_barrier(0);
    stage = stage == ST - 1 ? 0 : stage + 1;
  }
#pragma unroll
  for (int i = 0; i < 4; ++i)
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      const int64_t q = q0 + wr + 16 * i + 4 * (lane >> 4) + r;
      if (q >= a.Q) continue;
      const double iq = a.ia[q];
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        const int64_t n = n0 + wc + 16 * j + fr;
        if (n >= a.N) continue;
        const double ic = a.ib[n];
        const double cs = (double)acc[i][j][r] * iq * ic;
        const double v = (iq != 0.0 && ic != 0.0) ? (cs + 1.0) / 2.0 : 0.0;
        if constexpr (NTS) __builtin_nontemporal_store(v, a.out + q * a.N + n);  // write-once scores
        else a.out[q * a.N + n] = v;
      }
    }
}

// Tiled-layout kernel (default).  Workgroup = 8 waves (2 per SIMD), tile 128 queries x 128 FT frames; wave
// w owns frames 16 FT w .. + 16 FT - 1 against all 128 queries (8 x FT accumulator tiles).  Only the query
// operand goes through LDS (16 fragments = 16 KiB per K step, two stages, register-staged: each wave loads
// and stores two of them), read by all 8 waves; every frame fragment is used by exactly one wave of the
// workgroup, so it goes straight from global memory into that wave's VGPRs (contiguous 1 KiB loads, two
// K steps ahead) and never touches LDS.  Per K step and wave: 16 ds_read_b128 + 2 ds_write_b128, 2 + 2 FT
// global loads, 24 FT MFMAs; one block barrier.  Per output the MFMA sequence is k_cos_g3's (per K step
// hi.hi, hi.lo, lo.hi), so the scores are bit-identical to it.
// X: diagnostics only (wrong scores; make DIAG=1): 1 no MFMAs, 2 no barriers in the K loop, 3 no frame
// loads after the prologue, 4 no query staging after the prologue, 5 no query fragment reads
template <int FT, int PP, int D, int EP, int X = 0>
__global__ __launch_bounds__(512) __attribute__((amdgpu_waves_per_eu(1, 2))) void k_cos_t(CosArgs a, int64_t ftiles) {
  // two query stages (32 KiB); after the K loop the epilogue stages one 16-query row block per wave here
  constexpr int kSm = 2 * 16 * 512 * 2 > 8 * 16 * 16 * FT * 8 ? 2 * 16 * 512 * 2 : 8 * 16 * 16 * FT * 8;
  __shared__ __attribute__((aligned(16))) uint8_t smem[kSm];
  _Float16(*sA)[16 * 512] = reinterpret_cast<_Float16(*)[16 * 512]>(smem);
  constexpr int QT = 8, TN = 8 * 16 * FT;
  const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
  const int64_t blk = blockIdx.x;
  const int64_t xcd = blk & 7, slot = blk >> 3;
  const int qt = (int)(slot % a.qtiles);
  const int64_t nt = xcd + 8 * (slot / a.qtiles);
  if (nt >= a.ntiles) return;
  const int KB = a.Kp / kCosK;
  const int64_t qt0 = (int64_t)qt * QT;
  // this thread's two query pieces per step: fragment f = wv + 8 i -> query tile f >> 1, plane f & 1
  const _Float16* srcA[2];
#pragma unroll
  for (int i = 0; i < 2; ++i) {
    const int f = wv + 8 * i;
    srcA[i] = a.A + cos_frag(qt0 + (f >> 1), 0, KB, f & 1) + 8 * lane;
  }
  const _Float16* srcB[FT];
#pragma unroll
  for (int j = 0; j < FT; ++j) {
    int64_t t = nt * (TN / 16) + wv * FT + j;
    if (t > ftiles - 1) t = ftiles - 1;  // the last frame tile may pass the padded rows
    srcB[j] = a.B + cos_frag(t, 0, KB, 0) + 8 * lane;
  }
  h8 ra[2];
  h8 rb0[FT][2], rb1[FT][2], rb2[FT][2];  // frame fragments of steps s, s + 1, s + 2 (a ring, unrolled by 3)
  auto loadA = [&](int kb) {
#pragma unroll
    for (int i = 0; i < 2; ++i) ra[i] = *reinterpret_cast<const h8*>(srcA[i] + (int64_t)kb * 1024);
  };
  auto loadB = [&](int kb, h8 (&d)[FT][2]) {
#pragma unroll
    for (int j = 0; j < FT; ++j) {
      d[j][0] = *reinterpret_cast<const h8*>(srcB[j] + (int64_t)kb * 1024);
      d[j][1] = *reinterpret_cast<const h8*>(srcB[j] + (int64_t)kb * 1024 + 512);
    }
  };
  auto storeA = [&](int st) {
#pragma unroll
    for (int i = 0; i < 2; ++i) *reinterpret_cast<h8*>(&sA[st][(wv + 8 * i) * 512 + 8 * lane]) = ra[i];
  };
  f4 acc[QT][FT];
#pragma unroll
  for (int i = 0; i < QT; ++i)
#pragma unroll
    for (int j = 0; j < FT; ++j) acc[i][j] = f4{0.f, 0.f, 0.f, 0.f};

  // one K step: b = frame fragments of step s, nb = the ring slot that receives step s + 2
  auto step = [&](int s, const h8 (&b)[FT][2], h8 (&nb)[FT][2]) {
    const int st = s & 1;
    // query pieces of step s + 1 into the other stage (read by every wave in step s - 1, which ended at
    // the last barrier), then the loads for step s + 2: query pieces first, so the wait for them at the
    // next step leaves the frame fragments of s + 2 in flight
    // (branch-free: past the end the loads repeat the last step and the store fills a stage nobody reads
    // again — a conditional load would make the compiler's vmcnt merge wait for the new loads too)
    if constexpr (X != 4) {
      storeA(st ^ 1);
      loadA(s + 2 < KB ? s + 2 : KB - 1);
    }
    if constexpr (X != 3) loadB(s + D < KB ? s + D : KB - 1, nb);
    __builtin_amdgcn_sched_barrier(0);
    if constexpr (PP) {
      // memory phase: every query fragment of the step into registers, then publish; compute phase: 24 FT
      // MFMAs while the SIMD's other wave runs its memory phase
      h8 af[QT][2];
#pragma unroll
      for (int i = 0; i < QT; ++i) {
        if constexpr (X == 5) {  // diagnostics: no fragment reads
          af[i][0] = b[i % FT][0];
          af[i][1] = b[i % FT][1];
        } else {
          af[i][0] = *reinterpret_cast<const h8*>(&sA[st][(2 * i) * 512 + 8 * lane]);
          af[i][1] = *reinterpret_cast<const h8*>(&sA[st][(2 * i + 1) * 512 + 8 * lane]);
        }
      }
      __builtin_amdgcn_sched_barrier(0);
      if constexpr (X == 2) asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
      else asm volatile("s_waitcnt lgkmcnt(0)\n\ts_barrier" ::: "memory");
      __builtin_amdgcn_sched_barrier(0);
      if constexpr (X == 1) {  // keep the fragments live without the matrix cores
#pragma unroll
        for (int i = 0; i < QT; ++i)
#pragma unroll
          for (int j = 0; j < FT; ++j) acc[i][j][0] += (float)af[i][0][0] + (float)af[i][1][0] + (float)b[j][0][0] + (float)b[j][1][0];
      } else {
#pragma unroll
        for (int i = 0; i < QT; ++i)
#pragma unroll
          for (int j = 0; j < FT; ++j) {
            acc[i][j] = __builtin_amdgcn_mfma_f32_16x16x32_f16(af[i][0], b[j][0], acc[i][j], 0, 0, 0);
            acc[i][j] = __builtin_amdgcn_mfma_f32_16x16x32_f16(af[i][0], b[j][1], acc[i][j], 0, 0, 0);
            acc[i][j] = __builtin_amdgcn_mfma_f32_16x16x32_f16(af[i][1], b[j][0], acc[i][j], 0, 0, 0);
          }
      }
      __builtin_amdgcn_sched_barrier(0);
      if constexpr (X != 2) asm volatile("s_barrier" ::: "memory");
      __builtin_amdgcn_sched_barrier(0);
    } else {
#pragma unroll
      for (int i = 0; i < QT; ++i) {
        const h8 ah = *reinterpret_cast<const h8*>(&sA[st][(2 * i) * 512 + 8 * lane]);
        const h8 al = *reinterpret_cast<const h8*>(&sA[st][(2 * i + 1) * 512 + 8 * lane]);
#pragma unroll
        for (int j = 0; j < FT; ++j) {
          acc[i][j] = __builtin_amdgcn_mfma_f32_16x16x32_f16(ah, b[j][0], acc[i][j], 0, 0, 0);
          acc[i][j] = __builtin_amdgcn_mfma_f32_16x16x32_f16(ah, b[j][1], acc[i][j], 0, 0, 0);
          acc[i][j] = __builtin_amdgcn_mfma_f32_16x16x32_f16(al, b[j][0], acc[i][j], 0, 0, 0);
        }
      }
      __builtin_amdgcn_sched_barrier(0);
      asm volatile("s_waitcnt lgkmcnt(0)\n\ts_barrier" ::: "memory");
    }
  };

  loadA(0);
  loadB(0, rb0);
  if constexpr (X == 3) loadB(0, rb2);
  storeA(0);
  loadA(KB > 1 ? 1 : 0);
  if (D == 2) loadB(KB > 1 ? 1 : 0, rb1);
  asm volatile("s_waitcnt lgkmcnt(0)\n\ts_barrier" ::: "memory");
  // ping-pong: waves w and w + 4 share a SIMD; group 1 (waves 4-7) runs one barrier phase behind group 0,
  // so each SIMD alternates one wave's memory phase with the other's MFMAs.  A stage is read in the memory
  // phases of step s (group 0 at phase 2s, group 1 at 2s + 1) and rewritten in those of step s + 1 (2s + 2,
  // 2s + 3); each memory phase ends with lgkmcnt(0) + barrier, so no write overtakes a read and every write
  // is published before its first reader.  Group 0 takes one extra barrier at the end: equal counts.
  const int grp = __builtin_amdgcn_readfirstlane(wv >> 2);
  if (PP && grp) asm volatile("s_barrier" ::: "memory");
  int s = 0;
  if constexpr (D == 2) {  // frame fragments two steps ahead: a ring of three
    for (; s + 3 <= KB; s += 3) {
      step(s, rb0, rb2);
      step(s + 1, rb1, rb0);
      step(s + 2, rb2, rb1);
    }
    if (s < KB) step(s, rb0, rb2);
    if (s + 1 < KB) step(s + 1, rb1, rb0);
  } else {  // one step ahead: a ring of two
    for (; s + 2 <= KB; s += 2) {
      step(s, rb0, rb1);
      step(s + 1, rb1, rb0);
    }
    if (s < KB) step(s, rb0, rb1);
  }
  if (PP && !grp) asm volatile("s_barrier" ::: "memory");
  // epilogue: lane holds queries 16 i + 4 (lane >> 4) + r, frames 16 j + (lane & 15) of its wave's columns;
  // the inverse norms are loaded once (ia / ib cover the padded rows; a frame column past them is clamped
  // for the load and never stored)
  const int64_t q0 = qt0 * 16, n0 = nt * TN + (int64_t)wv * 16 * FT;
  const int64_t nrows = ftiles * 16;
  double ic[FT];
#pragma unroll
  for (int j = 0; j < FT; ++j) {
    const int64_t n = n0 + 16 * j + (lane & 15);
    ic[j] = a.ib[n < nrows ? n : nrows - 1];
  }
  // EP 1 (even N): each 16-query row block goes through the wave's LDS slice (16 x 16 FT f64, row-major)
  // and leaves as 16-byte stores of two adjacent frames; EP 0 (or odd N, whose rows are not all 16-byte
  // aligned): 8-byte stores straight from the accumulator layout
  const bool wide = EP == 1 && (a.N & 1) == 0;
  double* stage = reinterpret_cast<double*>(smem) + wv * 16 * 16 * FT;
#pragma unroll
  for (int i = 0; i < QT; ++i) {
    const int64_t qb = q0 + 16 * i + 4 * (lane >> 4);
    const double4 iq4 = *reinterpret_cast<const double4*>(a.ia + qb);
    const double iqv[4] = {iq4.x, iq4.y, iq4.z, iq4.w};
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      const int64_t q = qb + r;
      const double iq = iqv[r];
#pragma unroll
      for (int j = 0; j < FT; ++j) {
        const int64_t n = n0 + 16 * j + (lane & 15);
        const double cs = (double)acc[i][j][r] * iq * ic[j];
        const double v = (iq != 0.0 && ic[j] != 0.0) ? (cs + 1.0) / 2.0 : 0.0;
        if constexpr (EP == 2) {  // diagnostics: no stores (wrong output; A/B of the epilogue's cost)
          if (v == -1.0) a.out[0] = v;
        } else if constexpr (EP == 3) {  // float32 scores: the f64 value rounded once
          if (q < a.Q && n < a.N) __builtin_nontemporal_store((float)v, a.outf + q * a.N + n);
        } else if constexpr (EP == 4) {  // top-k: every value is staged, rows and columns are masked below
          stage[(4 * (lane >> 4) + r) * 16 * FT + 16 * j + (lane & 15)] = v;
        } else if (wide) {
          stage[(4 * (lane >> 4) + r) * 16 * FT + 16 * j + (lane & 15)] = v;
        } else if (q < a.Q && n < a.N) {
          __builtin_nontemporal_store(v, a.out + q * a.N + n);  // write-once scores
        }
      }
    }
    if (wide) {
      // 16 rows x 8 FT pairs of frames; lane c takes pairs c, c + 64, ...
#pragma unroll
      for (int u = 0; u < (16 * 8 * FT + 63) / 64; ++u) {
        const int c = lane + 64 * u;
        if (c >= 16 * 8 * FT) break;
        const int row = c / (8 * FT), pr = c % (8 * FT);
        const int64_t q = q0 + 16 * i + row, n = n0 + 2 * pr;
        const d2v v2 = *reinterpret_cast<const d2v*>(stage + row * 16 * FT + 2 * pr);
        if (q < a.Q) {
          if (n + 1 < a.N) __builtin_nontemporal_store(v2, reinterpret_cast<d2v*>(a.out + q * a.N + n));
          else if (n < a.N) __builtin_nontemporal_store(v2.x, a.out + q * a.N + n);
        }
      }
    }
    if constexpr (EP == 4) {
      // EP 4 (hq_cos_topk): the 16 queries of the row block against the tile's TN frames are now staged in
      // the eight wave slices; wave w selects for queries 2 w and 2 w + 1 (padded query rows write nothing).
      // Every wave of the workgroup reaches both barriers of every row block.
      __syncthreads();
#pragma unroll 1
      for (int h = 0; h < 2; ++h) {
        const int row = 2 * wv + h;
        const int64_t q = q0 + 16 * i + row;
        if (q < a.Q) cos_topk_row<TN>(reinterpret_cast<const double*>(smem), row, q, nt, a);
      }
      __syncthreads();  // the next row block overwrites the stage
    }
  }
}

template <int FT, int PP, int D = 2, int EP = 0, int X = 0>
static int launch_t(CosArgs a, hipStream_t s) {
  constexpr int TN = 8 * 16 * FT;
  const int64_t np_rows = a.ntiles * kCosT;
  a.qtiles = (int)(hq_cos_padded_rows(a.Q) / 128);
  a.ntiles = (np_rows + TN - 1) / TN;
  const int64_t nt8 = ((a.ntiles + 7) / 8) * 8;
  const int64_t blocks = nt8 * a.qtiles;
  if (blocks > 0x7FFFFFFF) return fail(HQ_E_UNSUPPORTED, "too many tiles");
  auto kern = k_cos_t<FT, PP, D, EP, X>;
  hipLaunchKernelGGL(kern, dim3((unsigned)blocks), dim3(512), 0, s, a, np_rows / 16);
  HQ_CHECK_LAUNCH();
  return HQ_OK;
}

template <int TN, int PP, bool NTS = true>
static int launch_g3(CosArgs a, hipStream_t s) {
  const int64_t np_rows = a.ntiles * kCosT;
  a.qtiles = (int)(hq_cos_padded_rows(a.Q) / 128);
  a.ntiles = (np_rows + TN - 1) / TN;
  const int64_t nt8 = ((a.ntiles + 7) / 8) * 8;
  const int64_t blocks = nt8 * a.qtiles;
  if (blocks > 0x7FFFFFFF) return fail(HQ_E_UNSUPPORTED, "too many tiles");
  const size_t lds = sizeof(_Float16) * 3 * (2 * 128 + 2 * TN) * kCosK;
  auto kern = k_cos_g3<TN, PP, NTS>;
  HQ_CHECK_HIP(hipFuncSetAttribute((const void*)kern, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
  hipLaunchKernelGGL(kern, dim3((unsigned)blocks), dim3(TN * 2), lds, s, a, np_rows);
  HQ_CHECK_LAUNCH();
  return HQ_OK;
}

template <int TQ>
static int launch_cos(CosArgs a, hipStream_t s) {
  a.qtiles = (int)((hq_cos_padded_rows(a.Q) + TQ - 1) / TQ);
  const int64_t nt8 = ((a.ntiles + 7) / 8) * 8;
  const int64_t blocks = nt8 * a.qtiles;
  if (blocks > 0x7FFFFFFF) return fail(HQ_E_UNSUPPORTED, "too many tiles");
  const size_t lds = sizeof(_Float16) * 2 * (2 * TQ + 2 * kCosT) * kCosRow;
  HQ_CHECK_HIP(hipFuncSetAttribute((const void*)k_cos_mfma<TQ>, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
  hipLaunchKernelGGL(k_cos_mfma<TQ>, dim3((unsigned)blocks), dim3(256), lds, s, a);
  HQ_CHECK_LAUNCH();
  return HQ_OK;
}

}  // namespace hq

using namespace hq;

extern "C" {

int hq_cos_padded_k(int K) { return K <= 0 ? 0 : ((K + kCosK - 1) / kCosK) * kCosK; }
int64_t hq_cos_padded_rows(int64_t N) { return N <= 0 ? 0 : ((N + kCosT - 1) / kCosT) * kCosT; }

int hq_cos_prepare(const float* X, int64_t N, int64_t ld, int K, void* X16, double* inv, hq_stream_t stream) {
  if (N < 0 || K <= 0 || ld < K) return fail(HQ_E_INVALID, "bad shape N=%lld K=%d ld=%lld", (long long)N, K, (long long)ld);
  if (N == 0) return HQ_OK;
  if (!X || !X16 || !inv) return fail(HQ_E_INVALID, "null buffer");
  const int Kp = hq_cos_padded_k(K);
  const int64_t rows = hq_cos_padded_rows(N);
  // the row-major layout only for the superseded A/B kernels (option cos_kernel 1-3): one wave per row;
  // the tiled layout: one wave per 16-row tile
  const int64_t ek = opt(OPT_COS_KERNEL, 0);
  const bool rowmajor = ek >= 1 && ek <= 3;
  int64_t blocks = rowmajor ? (rows + 3) / 4 : rows / 16;
  if (blocks > 65536) blocks = 65536;
  // tiled: split the K steps over up to 8 workgroups per tile while there are fewer than 1024 tiles
  int parts = 1;
  while (!rowmajor && parts < 8 && blocks * parts < 1024 && (Kp / kCosK) / (2 * parts) >= 16) parts *= 2;
  if (rowmajor)
    hipLaunchKernelGGL(k_cos_prepare, dim3((unsigned)blocks), dim3(256), 0, (hipStream_t)stream, X, N, ld, K, Kp, rows,
                       reinterpret_cast<_Float16*>(X16), inv);
  else
    hipLaunchKernelGGL(k_cos_prepare_tiled, dim3((unsigned)blocks, (unsigned)parts), dim3(1024), 0, (hipStream_t)stream,
                       X, N, ld, K, Kp, rows, reinterpret_cast<_Float16*>(X16), inv);
  HQ_CHECK_LAUNCH();
  return HQ_OK;
}

int hq_cos_scores_mfma_f32(const void* A16, const double* inv_a, int Q, const void* B16, const double* inv_b, int64_t N,
                           int K, float* out, hq_stream_t stream) {
  if (Q < 0 || N < 0 || K <= 0) return fail(HQ_E_INVALID, "bad shape");
  if (Q == 0 || N == 0) return HQ_OK;
  if (!A16 || !inv_a || !B16 || !inv_b || !out) return fail(HQ_E_INVALID, "null buffer");
  CosArgs a;
  a.A = reinterpret_cast<const _Float16*>(A16);
  a.B = reinterpret_cast<const _Float16*>(B16);
  a.ia = inv_a;
  a.ib = inv_b;
  a.Q = Q;
  a.N = N;
  a.Kp = hq_cos_padded_k(K);
  a.ntiles = hq_cos_padded_rows(N) / kCosT;
  a.out = nullptr;
  a.outf = out;
  return launch_t<3, 1, 1, 3>(a, (hipStream_t)stream);  // the default kernel, float32 score stores
}

int hq_cos_scores_mfma(const void* A16, const double* inv_a, int Q, const void* B16, const double* inv_b, int64_t N,
                       int K, double* out, hq_stream_t stream) {
  if (Q < 0 || N < 0 || K <= 0) return fail(HQ_E_INVALID, "bad shape");
  if (Q == 0 || N == 0) return HQ_OK;
  if (!A16 || !inv_a || !B16 || !inv_b || !out) return fail(HQ_E_INVALID, "null buffer");
  CosArgs a;
  a.A = reinterpret_cast<const _Float16*>(A16);
  a.B = reinterpret_cast<const _Float16*>(B16);
  a.ia = inv_a;
  a.ib = inv_b;
  a.Q = Q;
  a.N = N;
  a.Kp = hq_cos_padded_k(K);
  a.ntiles = hq_cos_padded_rows(N) / kCosT;
  a.out = out;
  a.outf = nullptr;
  // A/B (option cos_kernel): 1 register-staged two-buffer kernel, 2 lockstep (the DMA kernel without the
  // ping-pong stagger), 3 temporal score stores; DESIGN.md §4.5 has the measurements
  const int64_t ek = opt(OPT_COS_KERNEL, 0);
  if (ek == 1) return launch_cos<128>(a, (hipStream_t)stream);
  if (ek == 2) return launch_g3<256, 0>(a, (hipStream_t)stream);
  if (ek == 3) return launch_g3<256, 1>(a, (hipStream_t)stream);
  // tiled-layout forms: 4 lockstep 128 x 256, 5 ping-pong 128 x 128, 6 ping-pong 128 x 256
  // with frame fragments two steps ahead, 7 the same one step ahead, 8 the default with 16-byte score
  // stores through LDS
  if (ek == 4) return launch_t<2, 0>(a, (hipStream_t)stream);
  if (ek == 5) return launch_t<1, 1>(a, (hipStream_t)stream);
  if (ek == 6) return launch_t<2, 1, 2>(a, (hipStream_t)stream);
  if (ek == 7) return launch_t<2, 1, 1>(a, (hipStream_t)stream);
  if (ek == 8) return launch_t<3, 1, 1, 1>(a, (hipStream_t)stream);
#ifdef HQ_DIAG
  if (ek == 90) return launch_t<3, 1, 1, 2>(a, (hipStream_t)stream);  // no score stores (wrong output)
  // diagnostics (wrong output): 91 no MFMAs, 92 no K-loop barriers, 93 no frame loads, 94 no query
  // staging, 95 no query fragment reads
  if (ek == 91) return launch_t<3, 1, 1, 0, 1>(a, (hipStream_t)stream);
  if (ek == 92) return launch_t<3, 1, 1, 0, 2>(a, (hipStream_t)stream);
  if (ek == 93) return launch_t<3, 1, 1, 0, 3>(a, (hipStream_t)stream);
  if (ek == 94) return launch_t<3, 1, 1, 0, 4>(a, (hipStream_t)stream);
  if (ek == 95) return launch_t<3, 1, 1, 0, 5>(a, (hipStream_t)stream);
#endif
  return launch_t<3, 1, 1>(a, (hipStream_t)stream);
}

}  // extern "C"

// ---- fused top-k ---------------------------------------------------------------------------------------
// Workspace of hq_cos_topk: [Q] hint keys, the stage-1 slab [Q, P, k] (f64 scores, i64 frames; P = frame
// tiles of 384) and two merge buffers [Q, ceil(P / 64), k], [Q, ceil(P / 4096), k]; every piece 256-aligned.
// hq_cosq_topk and hq_cosqf_topk use the same layout, checks and driver around their own first stage.
namespace hq {

static int64_t cos_topk_tiles(int64_t N) { return (hq_cos_padded_rows(N) + 383) / 384; }
static size_t cos_topk_al(size_t b) { return (b + 255) & ~(size_t)255; }

// The argument checks the three fused routes share, in the order that decides which error wins: shape, empty
// problem (HQ_OK, *run stays false), k, the route's own limit (route(), HQ_OK to go on), buffers, workspace.
template <class Route>
static int cos_topk_check(int Q, int64_t N, int K, int k, bool buffers, size_t workspace_bytes, bool* run,
                          Route route) {
  *run = false;
  if (Q < 0 || N < 0 || K <= 0 || k < 1) return fail(HQ_E_INVALID, "bad shape Q=%d N=%lld K=%d k=%d", Q, (long long)N, K, k);
  if (Q == 0 || N == 0) return HQ_OK;
  if (k > 64) return fail(HQ_E_UNSUPPORTED, "k=%d: the fused frame top-k keeps lists of at most 64", k);
  const int rc = route();
  if (rc != HQ_OK) return rc;
  if (!buffers) return fail(HQ_E_INVALID, "null buffer");
  if (workspace_bytes < hq_cos_topk_workspace_size(Q, N, k)) return fail(HQ_E_INVALID, "workspace too small");
  *run = true;
  return HQ_OK;
}

// The fused top-k around a route's first stage: carve the workspace, point tk's top-k fields at the hint and the
// stage-1 slab, zero the hint, launch() the GEMM whose epilogue fills the slab (the caller's lambda reads tk),
// then merge 64 lists at a time until one is left: slab -> buffer 1 -> buffer 2 -> buffer 1 ...
template <class Launch>
static int cos_topk_run(int Q, int64_t N, int k, double threshold, int thr_mode, int64_t id_base, void* workspace,
                        double* out_score, int64_t* out_id, hipStream_t s, CosArgs& tk, Launch launch) {
  const int64_t P = cos_topk_tiles(N);
  uint8_t* w = reinterpret_cast<uint8_t*>(workspace);
  auto take = [&](size_t bytes) { uint8_t* p = w; w += cos_topk_al(bytes); return p; };
  uint64_t* hint = reinterpret_cast<uint64_t*>(take((size_t)Q * 8));
  double* bs[3];
  int64_t* bi[3];
  int64_t cap = P;  // lists per query a buffer holds: P, ceil(P / 64), ceil(P / 4096)
  for (int i = 0; i < 3; ++i) {
    bs[i] = reinterpret_cast<double*>(take((size_t)Q * cap * k * 8));
    bi[i] = reinterpret_cast<int64_t*>(take((size_t)Q * cap * k * 8));
    cap = (cap + 63) / 64;
  }
  tk.tk_s = bs[0];
  tk.tk_id = bi[0];
  tk.tk_hint = opt(OPT_COS_TOPK_HINT, 1) ? hint : nullptr;
  tk.tk_thr = threshold;
  tk.tk_mode = thr_mode;
  tk.tk_k = k;
  if (tk.tk_hint) HQ_CHECK_HIP(hipMemsetAsync(hint, 0, (size_t)Q * 8, s));
  const int rc = launch();
  if (rc != HQ_OK) return rc;
  int64_t Pc = P;
  int cur = 0;
  for (;;) {
    const int64_t P2 = (Pc + 63) / 64;
    const bool last = P2 == 1;
    const int nxt = cur == 1 ? 2 : 1;
    const int64_t g = (int64_t)Q * P2 < 65536 ? (int64_t)Q * P2 : 65536;
    hipLaunchKernelGGL(k_cos_topk_merge, dim3((unsigned)g), dim3(64), 0, s, Q, Pc, P2, k, last ? id_base : (int64_t)0,
                       (const double*)bs[cur], (const int64_t*)bi[cur], last ? out_score : bs[nxt], last ? out_id : bi[nxt]);
    HQ_CHECK_LAUNCH();
    if (last) break;
    Pc = P2;
    cur = nxt;
  }
  return HQ_OK;
}

}  // namespace hq

extern "C" {

size_t hq_cos_topk_workspace_size(int Q, int64_t N, int k) {
  if (Q <= 0 || N <= 0 || k <= 0) return 0;
  const size_t P = (size_t)cos_topk_tiles(N), P1 = (P + 63) / 64, P2 = (P1 + 63) / 64;
  return cos_topk_al((size_t)Q * 8) + 2 * cos_topk_al((size_t)Q * P * k * 8) + 2 * cos_topk_al((size_t)Q * P1 * k * 8) +
         2 * cos_topk_al((size_t)Q * P2 * k * 8);
}

int hq_cos_topk(const void* A16, const double* inv_a, int Q, const void* B16, const double* inv_b, int64_t N, int K,
                int k, double threshold, int thr_mode, int64_t id_base, void* workspace, size_t workspace_bytes,
                double* out_score, int64_t* out_id, hq_stream_t stream) {
  bool run;
  const int rc = cos_topk_check(Q, N, K, k, A16 && inv_a && B16 && inv_b && workspace && out_score && out_id,
                                workspace_bytes, &run, [] {
    const int64_t ek = opt(OPT_COS_KERNEL, 0);
    if (ek >= 1 && ek <= 3)
      return fail(HQ_E_UNSUPPORTED, "cos_kernel=%lld prepares the row-major layout; the fused frame top-k needs the tiled one",
                  (long long)ek);
    return HQ_OK;
  });
  if (!run) return rc;
  const hipStream_t s = (hipStream_t)stream;
  CosArgs a;
  a.A = reinterpret_cast<const _Float16*>(A16);
  a.B = reinterpret_cast<const _Float16*>(B16);
  a.ia = inv_a;
  a.ib = inv_b;
  a.Q = Q;
  a.N = N;
  a.Kp = hq_cos_padded_k(K);
  a.ntiles = hq_cos_padded_rows(N) / kCosT;
  a.out = nullptr;
  a.outf = nullptr;
  // the default kernel's K loop, top-k epilogue
  return cos_topk_run(Q, N, k, threshold, thr_mode, id_base, workspace, out_score, out_id, s, a,
                      [&] { return launch_t<3, 1, 1, 4>(a, s); });
}

}  // extern "C"

// ======== compressed-domain frame search: exact cosine of u8 frames (hq_cosq_*) ==========
// A stored frame is K bytes u plus float32 (mn, mx), x_i = mn + (mx - mn) u_i / 255.  With w = u - 128,
// S = sum w, T = sum w^2 (exact integers), s = (mx - mn) / 255, m = mn + s (128 + S / K) (the row mean),
// V = K T - S^2 and n^2 = K m^2 + s^2 V / K, the cosine of two dequantised frames is
//   cos = K a_q a_c + b_q b_c t / K,   a = m / n, b = s / n, t = K P - S_q S_c, P = sum w_q w_c
// (include/hq_mi355x.h has the contract).  P is what v_mfma_i32_16x16x64_i8 accumulates, exactly, so the score
// does not depend on tile shape, K order or kernel form.  hq_cosq_prepare stores, per row, the signed bytes in
// 1 KiB operand fragments and the pre-scaled pair A = m / sqrt(n^2 / K), B = s / (K sqrt(n^2 / K)), so that
// cos = A_q A_c + (B_q B_c) t: four float64 roundings per pair after exact integer work.
// Operand map: fragment (16-row tile t, K step kb of 64) = 1024 bytes at (t KB + kb) 1024, lane 16 g + j holds
// row 16 t + j, bytes 64 kb + 16 g .. + 15.  Queries and frames use the same fragment layout and the A and B
// operands of the instruction pair up the same (lane group, byte) positions, so P sums over every k of the step
// whatever order the hardware gives them inside it; only "lane & 15 = row" is relied on.
namespace hq {

typedef int i4v __attribute__((ext_vector_type(4)));

constexpr int kCosqK = 64;        // K per step
constexpr int kCosqMaxK = 65536;  // |P| <= 2^30, K T and S_q S_c below 2^48
constexpr int kCosqfQ = 64;       // queries per workgroup of k_cosq_t<3, EP> = the row padding of hq_cosqf_* queries

struct CosqArgs {
  CosArgs c;         // Q, N, qtiles, ntiles, out, tk_*: what the shared epilogue pieces read (the rest unused)
  const int8_t* A8;  // query fragments
  const int8_t* B8;  // frame fragments
  const double* sa;  // [Qp, 4]: A, B, S, ok (1.0 / 0.0)
  const double* sb;  // [Np, 4]
  int K;             // the true K (the formulas never see the padded one)
  int KB;            // K steps
};

// The one pair expression of every epilogue (dense and fused agree bit for bit).  K P and S_q S_c are integers
// below 2^48, so both products and their difference are exact in float64: t is the int64 value K P - S_q S_c.
__device__ __forceinline__ double cosq_score(int P, double Kd, double Aq, double Bq, double Sq, double okq, double Ac,
                                             double Bc, double Sc, double okc) {
  const double t = Kd * (double)P - Sq * Sc;
  const double cs = Aq * Ac + (Bq * Bc) * t;
  return (okq != 0.0 && okc != 0.0) ? (cs + 1.0) / 2.0 : 0.0;
}

// The one pair expression of every hq_cosqf_* epilogue (D, Sv, A_q, B_q: the banner of the file's last section, three
// query planes P0 .. P2 against one frame).  The integer part wraps nowhere that matters: K D and
// Sv S_c reach 2^62 each, their difference is at most 2^62 in magnitude (Cauchy-Schwarz on the two centred rows),
// and unsigned arithmetic gives that difference whatever the intermediate carries do.
__device__ __forceinline__ double cosqf_score(int P0, int P1, int P2, int64_t K, double Aq, double Bq, int64_t Sv,
                                              double okq, double Ac, double Bc, int64_t Sc, double okc) {
  const int64_t D = 65536 * (int64_t)P2 + 256 * (int64_t)P1 + (int64_t)P0 + 32896 * Sc;
  const int64_t t = (int64_t)((uint64_t)K * (uint64_t)D - (uint64_t)Sv * (uint64_t)Sc);
  const double cs = Aq * Ac + (Bq * Bc) * (double)t;
  return (okq != 0.0 && okc != 0.0) ? (cs + 1.0) / 2.0 : 0.0;
}

// Piece (kb, g) of a frame x of K bytes as k_cosq_prepare forms it: u ^ 0x80, zero past K (and for live = false).
__device__ __forceinline__ uint4 cosq_piece(const uint8_t* __restrict__ x, int k0, int K, int fast, bool live) {
  uint32_t w[4] = {0u, 0u, 0u, 0u};
  if (live && k0 < K) {
    if (fast && k0 + 16 <= K) {
      const uint4 v = *reinterpret_cast<const uint4*>(x + k0);
      w[0] = v.x ^ 0x80808080u;
      w[1] = v.y ^ 0x80808080u;
      w[2] = v.z ^ 0x80808080u;
      w[3] = v.w ^ 0x80808080u;
    } else {
#pragma unroll
      for (int u = 0; u < 16; ++u)
        if (k0 + u < K) w[u >> 2] |= (uint32_t)(x[k0 + u] ^ 0x80u) << (8 * (u & 3));
    }
  }
  return make_uint4(w[0], w[1], w[2], w[3]);
}

__device__ __forceinline__ void cosq_piece_sums(uint4 p, int& S, int& T) {
  const uint32_t w[4] = {p.x, p.y, p.z, p.w};
#pragma unroll
  for (int d = 0; d < 4; ++d)
#pragma unroll
    for (int b = 0; b < 4; ++b) {
      const int v = (int)(int8_t)(w[d] >> (8 * b));
      S += v;
      T += v * v;
    }
}

// The row statistics of the contract (include/hq_mi355x.h) from the exact sums S and T: (A, B, S, ok) at o.  mm: the
// row's float32 (mn, mx), nullptr for a pad row, which gets (0, 0, S, 0) with S = 0.  The one copy of the expression:
// k_cosq_prepare and the writers of the mutable store (k_cosq_append, k_cosq_replace) call it.
__device__ __forceinline__ void cosq_row_stats(int K, int64_t Si, int64_t Ti, const float* __restrict__ mm,
                                               double* __restrict__ o) {
  double A = 0.0, B = 0.0, ok = 0.0;
  if (mm) {
    const float fmn = mm[0], fmx = mm[1];
    if (isfinite(fmn) && isfinite(fmx)) {
      const double mn = fmn, mx = fmx, Kd = K;
      const double s = mx == mn ? 0.0 : (mx - mn) / 255.0;
      const double m = mn + s * (128.0 + (double)Si / Kd);
      const int64_t V = (int64_t)K * Ti - Si * Si;  // >= 0 (Cauchy-Schwarz), below 2^47
      const double n2 = m * m + (s * s) * ((double)V / (Kd * Kd));  // n^2 / K
      if (n2 > 0.0) {
        const double inv = 1.0 / sqrt(n2);
        A = m * inv;
        B = (s * inv) / Kd;
        ok = 1.0;
      }
    }
  }
  o[0] = A;
  o[1] = B;
  o[2] = (double)Si;
  o[3] = ok;
}

// One 16-wave workgroup per 16-row tile, one pass over the bytes: the waves split the tile's K steps, lane
// 16 g + j flips (u ^ 0x80) row j's bytes 64 kb + 16 g .. + 15 and stores them at its place in the fragment
// (one contiguous 1 KiB wave store), keeping int32 partial sums of w and w^2 (|S| <= 2^23, T <= 2^30); the
// partials meet in LDS and sixteen threads write the rows' statistics (V in int64).  fast: base and ld are
// multiples of 16, so a whole 16-byte piece inside K is one load; every other piece goes byte by byte.
__global__ __launch_bounds__(1024) void k_cosq_prepare(const uint8_t* __restrict__ X, int64_t N, int64_t ld, int K,
                                                       int KB, int64_t rows_out, const float* __restrict__ mm,
                                                       int8_t* __restrict__ X8, double* __restrict__ st, int fast) {
  __shared__ int sS[16], sT[16];
  const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6, j = lane & 15, g = lane >> 4;
  for (int64_t t = blockIdx.x; t < rows_out / 16; t += gridDim.x) {
    if (threadIdx.x < 16) sS[threadIdx.x] = sT[threadIdx.x] = 0;
    __syncthreads();
    const int64_t r = 16 * t + j;
    const uint8_t* x = X + (r < N ? r : 0) * ld;
    int S = 0, T = 0;
    for (int kb = wv; kb < KB; kb += 16) {
      const uint4 p = cosq_piece(x, kCosqK * kb + 16 * g, K, fast, r < N);  // pad rows and pad positions: w = 0
      cosq_piece_sums(p, S, T);
      *reinterpret_cast<uint4*>(X8 + ((t * KB + kb) * 1024 + 16 * lane)) = p;
    }
    S += __shfl_xor(S, 16, 64);
    T += __shfl_xor(T, 16, 64);
    S += __shfl_xor(S, 32, 64);
    T += __shfl_xor(T, 32, 64);
    if (g == 0) {
      atomicAdd(&sS[j], S);
      atomicAdd(&sT[j], T);
    }
    __syncthreads();
    if (threadIdx.x < 16) {
      const int64_t row = 16 * t + threadIdx.x;
      cosq_row_stats(K, sS[threadIdx.x], sT[threadIdx.x], row < N ? mm + 2 * row : nullptr, st + 4 * row);
    }
    __syncthreads();  // sS / sT are cleared for the next tile
  }
}

// ---- the mutable store: hq_cosq_append / hq_cosq_replace / hq_cosq_gather ----------------------
// A row's bytes are 4 KB pieces of 16 bytes, piece (kb, g) at (t KB + kb) 1024 + 16 (16 g + j), and 32 bytes of
// statistics; no piece holds bytes of two rows and the search kernels mask every row >= N, so rows can be written
// behind N, in place, or copied to another place one by one, and the result is what k_cosq_prepare writes.

// k_cosq_prepare's tile pass over rows [N0, N1) of a resident operand, tiles N0 / 16 .. rows_out / 16: frame
// r - N0 of X becomes row r.  Rows below N0 (the leading rows of N0's tile) are neither loaded nor stored, rows
// [N1, rows_out) are pad rows.  The store is predicated per lane on r >= N0, so every tile but N0's gets
// k_cosq_prepare's contiguous 1 KiB wave store; a lane sums its own row only, so S and T never see a resident row.
__global__ __launch_bounds__(1024) void k_cosq_append(const uint8_t* __restrict__ X, int64_t N0, int64_t N1, int64_t ld,
                                                      int K, int KB, int64_t rows_out, const float* __restrict__ mm,
                                                      int8_t* __restrict__ X8, double* __restrict__ st, int fast) {
  __shared__ int sS[16], sT[16];
  const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6, j = lane & 15, g = lane >> 4;
  for (int64_t t = N0 / 16 + blockIdx.x; t < rows_out / 16; t += gridDim.x) {
    if (threadIdx.x < 16) sS[threadIdx.x] = sT[threadIdx.x] = 0;
    __syncthreads();
    const int64_t r = 16 * t + j;
    const bool live = r >= N0 && r < N1;
    const uint8_t* x = X + (live ? r - N0 : 0) * ld;
    int S = 0, T = 0;
    for (int kb = wv; kb < KB; kb += 16) {
      const uint4 p = cosq_piece(x, kCosqK * kb + 16 * g, K, fast, live);
      cosq_piece_sums(p, S, T);
      if (r >= N0) *reinterpret_cast<uint4*>(X8 + ((t * KB + kb) * 1024 + 16 * lane)) = p;
    }
    S += __shfl_xor(S, 16, 64);
    T += __shfl_xor(T, 16, 64);
    S += __shfl_xor(S, 32, 64);
    T += __shfl_xor(T, 32, 64);
    if (g == 0) {
      atomicAdd(&sS[j], S);
      atomicAdd(&sT[j], T);
    }
    __syncthreads();
    if (threadIdx.x < 16) {
      const int64_t row = 16 * t + threadIdx.x;
      if (row >= N0)
        cosq_row_stats(K, sS[threadIdx.x], sT[threadIdx.x], row < N1 ? mm + 2 * (row - N0) : nullptr, st + 4 * row);
    }
    __syncthreads();  // sS / sT are cleared for the next tile
  }
}

// One 4-wave workgroup per replaced row: thread p takes the row's pieces p, p + 256, .. (piece 4 kb + g: the
// frame's bytes 16 p .. + 15, read contiguously across the workgroup) and stores each at its lane position of
// fragment kb; the other 15 rows of the tile are not touched.  A row id outside [0, N) is skipped.
__global__ __launch_bounds__(256) void k_cosq_replace(const uint8_t* __restrict__ X, int64_t M, int64_t ld, int K, int KB,
                                                      const float* __restrict__ mm, const int64_t* __restrict__ rows,
                                                      int64_t N, int8_t* __restrict__ X8, double* __restrict__ st,
                                                      int fast) {
  __shared__ int sS, sT;
  for (int64_t i = blockIdx.x; i < M; i += gridDim.x) {
    const int64_t row = rows[i];
    if (row < 0 || row >= N) continue;  // the whole workgroup
    if (threadIdx.x == 0) sS = sT = 0;
    __syncthreads();
    const int64_t t = row >> 4;
    const int j = (int)(row & 15);
    const uint8_t* x = X + i * ld;
    int S = 0, T = 0;
    for (int p = threadIdx.x; p < 4 * KB; p += 256) {
      const int kb = p >> 2, g = p & 3;
      const uint4 v = cosq_piece(x, 16 * p, K, fast, true);
      cosq_piece_sums(v, S, T);
      *reinterpret_cast<uint4*>(X8 + ((t * KB + kb) * 1024 + 16 * (16 * g + j))) = v;
    }
#pragma unroll
    for (int o = 1; o < 64; o <<= 1) {
      S += __shfl_xor(S, o, 64);
      T += __shfl_xor(T, o, 64);
    }
    if ((threadIdx.x & 63) == 0) {
      atomicAdd(&sS, S);
      atomicAdd(&sT, T);
    }
    __syncthreads();
    if (threadIdx.x == 0) cosq_row_stats(K, sS, sT, mm + 2 * i, st + 4 * row);
    __syncthreads();  // sS / sT are cleared for the next row
  }
}

// One 16-wave workgroup per destination tile, tiles 0 .. rows_out / 16: lane 16 g + j of wave w copies, for the
// K steps kb = w, w + 16, .., piece (kb, g) of source row src_row[16 t + j] (clamped into [0, N_src) for the
// load) to its own position: a 16-byte gather load and k_cosq_prepare's contiguous 1 KiB wave store.  Rows
// [M, rows_out) are pad rows.  Wave 0 copies the sixteen rows' statistics, one float64 per lane.
__global__ __launch_bounds__(1024) void k_cosq_gather(const int64_t* __restrict__ src_row, int64_t M, int64_t N_src,
                                                      int KB, int64_t rows_out, const int8_t* __restrict__ X8s,
                                                      const double* __restrict__ sts, int8_t* __restrict__ X8,
                                                      double* __restrict__ st) {
  const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6, j = lane & 15, g = lane >> 4;
  for (int64_t t = blockIdx.x; t < rows_out / 16; t += gridDim.x) {
    const int64_t r = 16 * t + j;
    int64_t s = 0;  // pad rows load nothing (M > 0 implies N_src > 0: hq_cosq_gather's check)
    if (r < M) s = min(max(src_row[r], (int64_t)0), N_src - 1);
    const int64_t src = (s >> 4) * KB * 1024 + 16 * (16 * g + (int)(s & 15));
    for (int kb = wv; kb < KB; kb += 16) {
      uint4 p = make_uint4(0u, 0u, 0u, 0u);
      if (r < M) p = *reinterpret_cast<const uint4*>(X8s + (src + (int64_t)kb * 1024));
      *reinterpret_cast<uint4*>(X8 + ((t * KB + kb) * 1024 + 16 * lane)) = p;
    }
    if (threadIdx.x < 64) {  // wave 0, thread 4 i + c: value c of the statistics of the tile's row i
      const int64_t row = 16 * t + (threadIdx.x >> 2);
      double v = 0.0;
      if (row < M) v = sts[4 * min(max(src_row[row], (int64_t)0), N_src - 1) + (threadIdx.x & 3)];
      st[4 * row + (threadIdx.x & 3)] = v;
    }
  }
}

// The GEMM of hq_cosq_* (NP = 1 query plane) and hq_cosqf_* (NP = 3): k_cos_t<3, 1, 1>'s structure (384 frames per
// 8-wave workgroup, wave w = every query x frames 48 w .. + 47, frame fragments straight from global memory one K
// step ahead, query fragments through two LDS stages, ping-pong: the two waves of a SIMD one barrier phase apart,
// XCD-aware block order) with K steps of 64 and v_mfma_i32_16x16x64_i8 into int32 accumulators.  A workgroup takes
// QT query tiles of 16 x NP planes = NF fragments of 1 KiB per step and stage; fragment f = (query tile f / NP,
// plane f % NP), wave w stages f = w and, where NF > 8, waves 0 .. NF - 9 also f = w + 8.
//   NP 1: 128 queries, 8 fragments, 8 x 3 accumulators of 4 = 96 VGPRs; per K step and wave 8 ds_read_b128,
//         1 ds_write_b128, 1 + 3 global loads of 1 KiB, 24 MFMAs.
//   NP 3: 64 queries, 4 x 3 = 12 fragments, 4 x 3 x 3 accumulators of 4 = 144 VGPRs; per K step and wave
//         12 ds_read_b128, 1 or 2 ds_write_b128, 1 or 2 + 3 global loads of 1 KiB, 36 MFMAs.
// EP 0: float64 score stores; EP 4: the staged top-k epilogue of hq_cos_topk (cos_topk_row on the same slab layout,
// running-threshold hint included).
template <int NP, int EP>
__global__ __launch_bounds__(512) __attribute__((amdgpu_waves_per_eu(1, 2))) void k_cosq_t(CosqArgs a, int64_t ftiles) {
  constexpr int FT = 3, QT = NP == 1 ? 8 : 4, NF = QT * NP, TN = 8 * 16 * FT;
  // the epilogue's stage (8 wave slices of 16 x 48 f64); during the K loop its first 2 NF KiB hold the two query stages
  __shared__ __attribute__((aligned(16))) uint8_t smem[8 * 16 * 16 * FT * 8];
  int8_t(*sA)[NF * 1024] = reinterpret_cast<int8_t(*)[NF * 1024]>(smem);
  const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
  const int64_t blk = blockIdx.x;
  const int64_t xcd = blk & 7, slot = blk >> 3;
  const int qt = (int)(slot % a.c.qtiles);
  const int64_t nt = xcd + 8 * (slot / a.c.qtiles);
  if (nt >= a.c.ntiles) return;
  const int KB = a.KB;
  const int64_t qt0 = (int64_t)qt * QT;
  const bool two = NF > 8 && __builtin_amdgcn_readfirstlane(wv) < NF - 8;
  const int f1 = wv + 8;
  const int8_t* srcA0 = a.A8 + ((qt0 + wv / NP) * KB * NP + wv % NP) * 1024 + 16 * lane;
  const int8_t* srcA1 = a.A8 + ((qt0 + (two ? f1 / NP : 0)) * KB * NP + f1 % NP) * 1024 + 16 * lane;
  const int8_t* srcB[FT];
#pragma unroll
  for (int j = 0; j < FT; ++j) {
    int64_t t = nt * (TN / 16) + wv * FT + j;
    if (t > ftiles - 1) t = ftiles - 1;  // the last frame tile may pass the padded rows
    srcB[j] = a.B8 + t * KB * 1024 + 16 * lane;
  }
  i4v ra0, ra1 = i4v{0, 0, 0, 0};
  i4v rb0[FT], rb1[FT];  // frame fragments of steps s, s + 1
  auto loadA = [&](int kb) {
    ra0 = *reinterpret_cast<const i4v*>(srcA0 + (int64_t)kb * (NP * 1024));
    if (two) ra1 = *reinterpret_cast<const i4v*>(srcA1 + (int64_t)kb * (NP * 1024));
  };
  auto loadB = [&](int kb, i4v (&d)[FT]) {
#pragma unroll
    for (int j = 0; j < FT; ++j) d[j] = *reinterpret_cast<const i4v*>(srcB[j] + (int64_t)kb * 1024);
  };
  auto storeA = [&](int st) {
    *reinterpret_cast<i4v*>(&sA[st][wv * 1024 + 16 * lane]) = ra0;
    if (two) *reinterpret_cast<i4v*>(&sA[st][f1 * 1024 + 16 * lane]) = ra1;
  };
  i4v acc[QT][NP][FT];
#pragma unroll
  for (int i = 0; i < QT; ++i)
#pragma unroll
    for (int p = 0; p < NP; ++p)
#pragma unroll
      for (int j = 0; j < FT; ++j) acc[i][p][j] = i4v{0, 0, 0, 0};

  // one K step: b = frame fragments of step s, nb receives step s + 1 (k_cos_t's step, PP = 1, D = 1; past the
  // end the loads repeat the last step and the store fills a stage nobody reads again)
  auto step = [&](int s, const i4v (&b)[FT], i4v (&nb)[FT]) {
    const int st = s & 1;
    storeA(st ^ 1);
    loadA(s + 2 < KB ? s + 2 : KB - 1);
    loadB(s + 1 < KB ? s + 1 : KB - 1, nb);
    __builtin_amdgcn_sched_barrier(0);
    i4v af[NF];
#pragma unroll
    for (int f = 0; f < NF; ++f) af[f] = *reinterpret_cast<const i4v*>(&sA[st][f * 1024 + 16 * lane]);
    __builtin_amdgcn_sched_barrier(0);
    asm volatile("s_waitcnt lgkmcnt(0)\n\ts_barrier" ::: "memory");
    __builtin_amdgcn_sched_barrier(0);
#pragma unroll
    for (int i = 0; i < QT; ++i)
#pragma unroll
      for (int p = 0; p < NP; ++p)
#pragma unroll
        for (int j = 0; j < FT; ++j)
          acc[i][p][j] = __builtin_amdgcn_mfma_i32_16x16x64_i8(af[NP * i + p], b[j], acc[i][p][j], 0, 0, 0);
    __builtin_amdgcn_sched_barrier(0);
    asm volatile("s_barrier" ::: "memory");
    __builtin_amdgcn_sched_barrier(0);
  };

  loadA(0);
  loadB(0, rb0);
  storeA(0);
  loadA(KB > 1 ? 1 : 0);
  asm volatile("s_waitcnt lgkmcnt(0)\n\ts_barrier" ::: "memory");
  // ping-pong as in k_cos_t: group 1 (waves 4-7) one barrier phase behind, group 0 one extra barrier at the end
  const int grp = __builtin_amdgcn_readfirstlane(wv >> 2);
  if (grp) asm volatile("s_barrier" ::: "memory");
  int s = 0;
  for (; s + 2 <= KB; s += 2) {
    step(s, rb0, rb1);
    step(s + 1, rb1, rb0);
  }
  if (s < KB) step(s, rb0, rb1);
  if (!grp) asm volatile("s_barrier" ::: "memory");
  // epilogue: lane holds queries 16 i + 4 (lane >> 4) + r, frames 16 j + (lane & 15) of its wave's columns (the
  // C / D map does not depend on the operand type); sa / sb cover the padded rows, a frame column past them is
  // clamped for the load and never stored.  NP 3 takes the integer sums S_c, Sv as int64, converted here, once
  // per frame column and query row (at the use site the conversion would repeat for every pair).
  const int64_t q0 = qt0 * 16, n0 = nt * TN + (int64_t)wv * 16 * FT;
  const int64_t nrows = ftiles * 16;
  const double Kd = (double)a.K;
  const int64_t Ki = a.K;
  double Ac[FT], Bc[FT], Sd[FT], okc[FT];
  int64_t Sc[FT];
#pragma unroll
  for (int j = 0; j < FT; ++j) {
    const int64_t n = n0 + 16 * j + (lane & 15);
    const double4 c = *reinterpret_cast<const double4*>(a.sb + 4 * (n < nrows ? n : nrows - 1));
    Ac[j] = c.x;
    Bc[j] = c.y;
    Sd[j] = c.z;
    Sc[j] = (int64_t)c.z;
    okc[j] = c.w;
  }
  double* stage = reinterpret_cast<double*>(smem) + wv * 16 * 16 * FT;
#pragma unroll
  for (int i = 0; i < QT; ++i) {
    const int64_t qb = q0 + 16 * i + 4 * (lane >> 4);
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      const int64_t q = qb + r;
      const double4 sq = *reinterpret_cast<const double4*>(a.sa + 4 * q);
      const int64_t Sv = (int64_t)sq.z;
#pragma unroll
      for (int j = 0; j < FT; ++j) {
        const int64_t n = n0 + 16 * j + (lane & 15);
        double v;
        if constexpr (NP == 1)
          v = cosq_score(acc[i][0][j][r], Kd, sq.x, sq.y, sq.z, sq.w, Ac[j], Bc[j], Sd[j], okc[j]);
        else
          v = cosqf_score(acc[i][0][j][r], acc[i][1][j][r], acc[i][2][j][r], Ki, sq.x, sq.y, Sv, sq.w, Ac[j], Bc[j],
                          Sc[j], okc[j]);
        if constexpr (EP == 4) {  // top-k: every value is staged, rows and columns are masked in cos_topk_row
          stage[(4 * (lane >> 4) + r) * 16 * FT + 16 * j + (lane & 15)] = v;
        } else if (q < a.c.Q && n < a.c.N) {
          __builtin_nontemporal_store(v, a.c.out + q * a.c.N + n);  // write-once scores
        }
      }
    }
    if constexpr (EP == 4) {
      // as k_cos_t's EP 4: wave w selects for queries 2 w and 2 w + 1 of the row block; every wave of the
      // workgroup reaches both barriers of every row block
      __syncthreads();
#pragma unroll 1
      for (int h = 0; h < 2; ++h) {
        const int row = 2 * wv + h;
        const int64_t q = q0 + 16 * i + row;
        if (q < a.c.Q) cos_topk_row<TN>(reinterpret_cast<const double*>(smem), row, q, nt, a.c);
      }
      __syncthreads();  // the next row block overwrites the stage
    }
  }
}

// Query rows are padded to the workgroup's QT tiles: 128 for one plane, kCosqfQ for three.
template <int NP, int EP>
static int launch_cosq(CosqArgs a, hipStream_t s) {
  const int64_t np_rows = hq_cosq_padded_rows(a.c.N);
  a.c.qtiles = (int)(NP == 1 ? hq_cosq_padded_rows(a.c.Q) / 128 : hq_cosqf_padded_rows(a.c.Q) / kCosqfQ);
  a.c.ntiles = (np_rows + 383) / 384;
  const int64_t nt8 = ((a.c.ntiles + 7) / 8) * 8;
  const int64_t blocks = nt8 * a.c.qtiles;
  if (blocks > 0x7FFFFFFF) return fail(HQ_E_UNSUPPORTED, "too many tiles");
  hipLaunchKernelGGL((k_cosq_t<NP, EP>), dim3((unsigned)blocks), dim3(512), 0, s, a, np_rows / 16);
  HQ_CHECK_LAUNCH();
  return HQ_OK;
}

static CosqArgs cosq_args(const void* A8, const double* sa, int Q, const void* B8, const double* sb, int64_t N, int K) {
  CosqArgs a;
  memset(&a, 0, sizeof(a));
  a.A8 = reinterpret_cast<const int8_t*>(A8);
  a.B8 = reinterpret_cast<const int8_t*>(B8);
  a.sa = sa;
  a.sb = sb;
  a.K = K;
  a.KB = hq_cosq_padded_k(K) / kCosqK;
  a.c.Q = Q;
  a.c.N = N;
  return a;
}

}  // namespace hq

extern "C" {

int hq_cosq_padded_k(int K) { return K <= 0 ? 0 : ((K + kCosqK - 1) / kCosqK) * kCosqK; }
int64_t hq_cosq_padded_rows(int64_t N) { return N <= 0 ? 0 : ((N + kCosT - 1) / kCosT) * kCosT; }

int hq_cosq_prepare(const uint8_t* frames, int64_t N, int64_t ld, int K, const float* minmax, void* X8, double* stats,
                    hq_stream_t stream) {
  if (N < 0 || K <= 0 || ld < K) return fail(HQ_E_INVALID, "bad shape N=%lld K=%d ld=%lld", (long long)N, K, (long long)ld);
  if (N == 0) return HQ_OK;
  if (K > kCosqMaxK) return fail(HQ_E_UNSUPPORTED, "K=%d: the int32 accumulator holds K <= %d", K, kCosqMaxK);
  if (!frames || !minmax || !X8 || !stats) return fail(HQ_E_INVALID, "null buffer");
  const int64_t rows = hq_cosq_padded_rows(N);
  int64_t blocks = rows / 16;
  if (blocks > 65536) blocks = 65536;
  const int fast = ((uintptr_t)frames % 16 == 0 && ld % 16 == 0) ? 1 : 0;
  hipLaunchKernelGGL(k_cosq_prepare, dim3((unsigned)blocks), dim3(1024), 0, (hipStream_t)stream, frames, N, ld, K,
                     hq_cosq_padded_k(K) / kCosqK, rows, minmax, reinterpret_cast<int8_t*>(X8), stats, fast);
  HQ_CHECK_LAUNCH();
  return HQ_OK;
}

// cap_rows of a resident operand: whole 128-row units, at least need's padded rows
static bool cosq_cap_ok(int64_t cap_rows, int64_t need) {
  return cap_rows >= 0 && cap_rows % kCosT == 0 && need <= cap_rows && hq_cosq_padded_rows(need) <= cap_rows;
}

int hq_cosq_append(const uint8_t* frames, int64_t M, int64_t ld, int K, const float* minmax, int64_t N0, int64_t cap_rows,
                   void* X8, double* stats, hq_stream_t stream) {
  if (M < 0 || N0 < 0 || K <= 0 || ld < K || M > INT64_MAX - N0 || !cosq_cap_ok(cap_rows, N0 + M))
    return fail(HQ_E_INVALID, "bad shape M=%lld K=%d ld=%lld N0=%lld cap_rows=%lld", (long long)M, K, (long long)ld,
                (long long)N0, (long long)cap_rows);
  if (M == 0) return HQ_OK;
  if (K > kCosqMaxK) return fail(HQ_E_UNSUPPORTED, "K=%d: the int32 accumulator holds K <= %d", K, kCosqMaxK);
  if (!frames || !minmax || !X8 || !stats) return fail(HQ_E_INVALID, "null buffer");
  const int64_t rows = hq_cosq_padded_rows(N0 + M);
  int64_t blocks = rows / 16 - N0 / 16;
  if (blocks > 65536) blocks = 65536;
  const int fast = ((uintptr_t)frames % 16 == 0 && ld % 16 == 0) ? 1 : 0;
  hipLaunchKernelGGL(k_cosq_append, dim3((unsigned)blocks), dim3(1024), 0, (hipStream_t)stream, frames, N0, N0 + M, ld, K,
                     hq_cosq_padded_k(K) / kCosqK, rows, minmax, reinterpret_cast<int8_t*>(X8), stats, fast);
  HQ_CHECK_LAUNCH();
  return HQ_OK;
}

int hq_cosq_replace(const uint8_t* frames, int64_t M, int64_t ld, int K, const float* minmax, const int64_t* rows,
                    int64_t N, void* X8, double* stats, hq_stream_t stream) {
  if (M < 0 || N < 0 || K <= 0 || ld < K)
    return fail(HQ_E_INVALID, "bad shape M=%lld K=%d ld=%lld N=%lld", (long long)M, K, (long long)ld, (long long)N);
  if (M == 0) return HQ_OK;
  if (K > kCosqMaxK) return fail(HQ_E_UNSUPPORTED, "K=%d: the int32 accumulator holds K <= %d", K, kCosqMaxK);
  if (!frames || !minmax || !rows || !X8 || !stats) return fail(HQ_E_INVALID, "null buffer");
  const int64_t blocks = M < 65536 ? M : 65536;
  const int fast = ((uintptr_t)frames % 16 == 0 && ld % 16 == 0) ? 1 : 0;
  hipLaunchKernelGGL(k_cosq_replace, dim3((unsigned)blocks), dim3(256), 0, (hipStream_t)stream, frames, M, ld, K,
                     hq_cosq_padded_k(K) / kCosqK, minmax, rows, N, reinterpret_cast<int8_t*>(X8), stats, fast);
  HQ_CHECK_LAUNCH();
  return HQ_OK;
}

int hq_cosq_gather(const int64_t* src_row, int64_t M, int64_t N_src, int K, const void* X8_src, const double* stats_src,
                   int64_t cap_rows, void* X8, double* stats, hq_stream_t stream) {
  if (M < 0 || N_src < 0 || K <= 0 || (M > 0 && N_src == 0) || !cosq_cap_ok(cap_rows, M))
    return fail(HQ_E_INVALID, "bad shape M=%lld N_src=%lld K=%d cap_rows=%lld", (long long)M, (long long)N_src, K,
                (long long)cap_rows);
  if (M == 0 && cap_rows == 0) return HQ_OK;
  if (K > kCosqMaxK) return fail(HQ_E_UNSUPPORTED, "K=%d: the int32 accumulator holds K <= %d", K, kCosqMaxK);
  if ((M > 0 && (!src_row || !X8_src || !stats_src)) || !X8 || !stats) return fail(HQ_E_INVALID, "null buffer");
  const int64_t rows = M ? hq_cosq_padded_rows(M) : kCosT;  // an empty result: one unit of pad rows
  int64_t blocks = rows / 16;
  if (blocks > 65536) blocks = 65536;
  hipLaunchKernelGGL(k_cosq_gather, dim3((unsigned)blocks), dim3(1024), 0, (hipStream_t)stream, src_row, M, N_src,
                     hq_cosq_padded_k(K) / kCosqK, rows, reinterpret_cast<const int8_t*>(X8_src), stats_src,
                     reinterpret_cast<int8_t*>(X8), stats);
  HQ_CHECK_LAUNCH();
  return HQ_OK;
}

int hq_cosq_scores(const void* A8, const double* stats_a, int Q, const void* B8, const double* stats_b, int64_t N, int K,
                   double* out, hq_stream_t stream) {
  if (Q < 0 || N < 0 || K <= 0) return fail(HQ_E_INVALID, "bad shape Q=%d N=%lld K=%d", Q, (long long)N, K);
  if (Q == 0 || N == 0) return HQ_OK;
  if (K > kCosqMaxK) return fail(HQ_E_UNSUPPORTED, "K=%d: the int32 accumulator holds K <= %d", K, kCosqMaxK);
  if (!A8 || !stats_a || !B8 || !stats_b || !out) return fail(HQ_E_INVALID, "null buffer");
  CosqArgs a = cosq_args(A8, stats_a, Q, B8, stats_b, N, K);
  a.c.out = out;
  return launch_cosq<1, 0>(a, (hipStream_t)stream);
}

// The workspace layout, the shared checks and the merge stage are hq_cos_topk's (cos_topk_check, cos_topk_run).
size_t hq_cosq_topk_workspace_size(int Q, int64_t N, int k) { return hq_cos_topk_workspace_size(Q, N, k); }

int hq_cosq_topk(const void* A8, const double* stats_a, int Q, const void* B8, const double* stats_b, int64_t N, int K,
                 int k, double threshold, int thr_mode, int64_t id_base, void* workspace, size_t workspace_bytes,
                 double* out_score, int64_t* out_id, hq_stream_t stream) {
  bool run;
  const int rc = cos_topk_check(Q, N, K, k, A8 && stats_a && B8 && stats_b && workspace && out_score && out_id,
                                workspace_bytes, &run, [&] {
    if (K > kCosqMaxK) return fail(HQ_E_UNSUPPORTED, "K=%d: the int32 accumulator holds K <= %d", K, kCosqMaxK);
    return HQ_OK;
  });
  if (!run) return rc;
  const hipStream_t s = (hipStream_t)stream;
  CosqArgs a = cosq_args(A8, stats_a, Q, B8, stats_b, N, K);
  return cos_topk_run(Q, N, k, threshold, thr_mode, id_base, workspace, out_score, out_id, s, a.c,
                      [&] { return launch_cosq<1, 4>(a, s); });
}

}  // extern "C"

// ======== float32 queries against the u8 frame store: exact asymmetric cosine (hq_cosqf_*) ======
// The corpus operands are hq_cosq_prepare's, untouched.  A query row of K float32 values is scaled by a power of
// two and rounded to 24-bit fixed point: amax = f 2^e (f in [0.5, 1)), v_i = min(rint(q_i 2^(23 - e)), 2^23 - 1),
// an integer vector that plays "a row with s = 1" in the closed form of hq_cosq_*: with Sv = sum v, Nv = sum v^2,
// B_q = 1 / sqrt(K Nv), A_q = Sv B_q and D = sum v_i w_i,
//   cos = A_q A_c + (B_q B_c) t,   t = K D - Sv S_c   (an exact int64, |t| <= 2^62).
// D comes from three int8 digit planes of v contracted with the corpus's signed bytes by v_mfma_i32_16x16x64_i8:
// with the two's-complement bytes of v (b2 signed, b1 and b0 unsigned), plane 2 = b2, plane 1 = b1 ^ 0x80 =
// b1 - 128, plane 0 = b0 ^ 0x80 = b0 - 128, so v = 65536 p2 + 256 p1 + p0 + 32896 and
//   D = 65536 P2 + 256 P1 + P0 + 32896 S_c,   |P_j| <= 2^30 for K <= 65536.
// Pad rows and pad K positions hold 0 in all three planes (the corpus's pad bytes are w = 0 as well, and S_c is
// the true-K sum, so the identity holds on the padded operands).
// Operand map: query tile t (16 rows), K step kb, plane p = the 1 KiB fragment at ((t KB + kb) 3 + p) 1024 in the
// corpus's fragment layout (lane 16 g + j = row 16 t + j, bytes 64 kb + 16 g .. + 15): a step's query operands are
// one contiguous 3 KiB.  stats [padded rows, 4] = (A_q, B_q, Sv, ok); Sv is an integer below 2^39, exact as f64.
namespace hq {

// One 16-wave workgroup per 16-row query tile, two passes over the floats (the second one hits the cache).
// Pass 1: the largest |q| bit pattern of every row (a NaN or inf is above every finite pattern, so one integer
// max finds amax and the non-finite rows).  Pass 2: lane 16 g + j rounds row j's values 64 kb + 16 g .. + 15 to v
// (the scaling in float64 is exact: 2^(23 - e) overflows float32 for subnormal rows), stores the three digit
// pieces at its place in the step's three fragments and keeps int64 partial sums of v and v^2; the partials meet
// in LDS and sixteen threads write the rows' statistics.  fast: base and ld are multiples of 16 bytes, so a whole
// 16-value piece inside K is four 16-byte loads; every other piece goes element by element.
__global__ __launch_bounds__(1024) void k_cosqf_prepare(const float* __restrict__ X, int64_t Q, int64_t ld, int K,
                                                        int KB, int64_t rows_out, int8_t* __restrict__ Q8,
                                                        double* __restrict__ st, int fast) {
  __shared__ unsigned sM[16];
  __shared__ unsigned long long sS[16], sN[16];
  const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6, j = lane & 15, g = lane >> 4;
  for (int64_t t = blockIdx.x; t < rows_out / 16; t += gridDim.x) {
    if (threadIdx.x < 16) {
      sM[threadIdx.x] = 0u;
      sS[threadIdx.x] = sN[threadIdx.x] = 0ull;
    }
    __syncthreads();
    const int64_t r = 16 * t + j;
    const float* x = X + (r < Q ? r : 0) * ld;
    auto piece = [&](int k0, float (&f)[16]) {  // values k0 .. k0 + 15 of the row, 0 past K
      if (fast && k0 + 16 <= K) {
#pragma unroll
        for (int u = 0; u < 4; ++u) {
          const float4 v = *reinterpret_cast<const float4*>(x + k0 + 4 * u);
          f[4 * u] = v.x;
          f[4 * u + 1] = v.y;
          f[4 * u + 2] = v.z;
          f[4 * u + 3] = v.w;
        }
      } else {
#pragma unroll
        for (int u = 0; u < 16; ++u) f[u] = k0 + u < K ? x[k0 + u] : 0.0f;
      }
    };
    unsigned m = 0u;
    if (r < Q)
      for (int kb = wv; kb < KB; kb += 16) {
        const int k0 = kCosqK * kb + 16 * g;
        if (k0 < K) {
          float f[16];
          piece(k0, f);
#pragma unroll
          for (int u = 0; u < 16; ++u) {
            const unsigned b = __float_as_uint(f[u]) & 0x7FFFFFFFu;
            m = b > m ? b : m;
          }
        }
      }
    {
      const unsigned m2 = (unsigned)__shfl_xor((int)m, 16, 64);
      m = m2 > m ? m2 : m;
      const unsigned m3 = (unsigned)__shfl_xor((int)m, 32, 64);
      m = m3 > m ? m3 : m;
    }
    if (g == 0) atomicMax(&sM[j], m);
    __syncthreads();
    const unsigned am = sM[j];
    const bool ok = r < Q && am != 0u && am < 0x7F800000u;
    // amax = f 2^e, f in [0.5, 1): amax is a normal float64 whatever it was in float32
    const int e = (int)((__double_as_longlong((double)__uint_as_float(am)) >> 52) & 0x7FF) - 1022;
    const double scale = __longlong_as_double((long long)(1023 + 23 - e) << 52);  // 2^(23 - e), 23 - e in [-105, 172]
    int64_t S = 0, Nn = 0;
    for (int kb = wv; kb < KB; kb += 16) {
      const int k0 = kCosqK * kb + 16 * g;
      uint32_t d[3][4] = {{0u, 0u, 0u, 0u}, {0u, 0u, 0u, 0u}, {0u, 0u, 0u, 0u}};  // pad rows, pad positions: 0
      if (ok && k0 < K) {
        float f[16];
        piece(k0, f);
#pragma unroll
        for (int u = 0; u < 16; ++u)
          if (k0 + u < K) {
            int v = (int)rint((double)f[u] * scale);  // round to nearest even, |.| <= 2^23
            v = v > 8388607 ? 8388607 : v;
            S += v;
            Nn += (int64_t)v * v;
            const uint32_t b = (uint32_t)v ^ 0x8080u;
            d[0][u >> 2] |= (b & 0xFFu) << (8 * (u & 3));
            d[1][u >> 2] |= ((b >> 8) & 0xFFu) << (8 * (u & 3));
            d[2][u >> 2] |= ((b >> 16) & 0xFFu) << (8 * (u & 3));
          }
      }
#pragma unroll
      for (int p = 0; p < 3; ++p)
        *reinterpret_cast<uint4*>(Q8 + (((t * KB + kb) * 3 + p) * 1024 + 16 * lane)) =
            make_uint4(d[p][0], d[p][1], d[p][2], d[p][3]);
    }
    S += __shfl_xor(S, 16, 64);
    Nn += __shfl_xor(Nn, 16, 64);
    S += __shfl_xor(S, 32, 64);
    Nn += __shfl_xor(Nn, 32, 64);
    if (g == 0) {
      atomicAdd(&sS[j], (unsigned long long)S);
      atomicAdd(&sN[j], (unsigned long long)Nn);
    }
    __syncthreads();
    if (threadIdx.x < 16) {
      const int64_t row = 16 * t + threadIdx.x;
      const unsigned a2 = sM[threadIdx.x];
      const int64_t Si = (int64_t)sS[threadIdx.x], Ni = (int64_t)sN[threadIdx.x];
      double A = 0.0, B = 0.0, Sd = 0.0, okd = 0.0;
      if (row < Q && a2 != 0u && a2 < 0x7F800000u) {  // Ni >= 2^44: the row maximum rounds to at least 2^22
        B = 1.0 / sqrt((double)K * (double)Ni);
        A = (double)Si * B;
        Sd = (double)Si;
        okd = 1.0;
      }
      double* o = st + 4 * row;
      o[0] = A;
      o[1] = B;
      o[2] = Sd;
      o[3] = okd;
    }
    __syncthreads();  // sM / sS / sN are cleared for the next tile
  }
}

}  // namespace hq

extern "C" {

int64_t hq_cosqf_padded_rows(int64_t Q) { return Q <= 0 ? 0 : ((Q + kCosqfQ - 1) / kCosqfQ) * kCosqfQ; }

int hq_cosqf_prepare(const float* X, int64_t Q, int64_t ld, int K, void* Q8, double* stats, hq_stream_t stream) {
  if (Q < 0 || K <= 0 || ld < K) return fail(HQ_E_INVALID, "bad shape Q=%lld K=%d ld=%lld", (long long)Q, K, (long long)ld);
  if (Q == 0) return HQ_OK;
  if (K > kCosqMaxK) return fail(HQ_E_UNSUPPORTED, "K=%d: the int32 accumulators hold K <= %d", K, kCosqMaxK);
  if (!X || !Q8 || !stats) return fail(HQ_E_INVALID, "null buffer");
  const int64_t rows = hq_cosqf_padded_rows(Q);
  int64_t blocks = rows / 16;
  if (blocks > 65536) blocks = 65536;
  const int fast = ((uintptr_t)X % 16 == 0 && ld % 4 == 0) ? 1 : 0;
  hipLaunchKernelGGL(k_cosqf_prepare, dim3((unsigned)blocks), dim3(1024), 0, (hipStream_t)stream, X, Q, ld, K,
                     hq_cosq_padded_k(K) / kCosqK, rows, reinterpret_cast<int8_t*>(Q8), stats, fast);
  HQ_CHECK_LAUNCH();
  return HQ_OK;
}

int hq_cosqf_scores(const void* Q8, const double* stats_q, int Q, const void* B8, const double* stats_b, int64_t N, int K,
                    double* out, hq_stream_t stream) {
  if (Q < 0 || N < 0 || K <= 0) return fail(HQ_E_INVALID, "bad shape Q=%d N=%lld K=%d", Q, (long long)N, K);
  if (Q == 0 || N == 0) return HQ_OK;
  if (K > kCosqMaxK) return fail(HQ_E_UNSUPPORTED, "K=%d: the int32 accumulators hold K <= %d", K, kCosqMaxK);
  if (!Q8 || !stats_q || !B8 || !stats_b || !out) return fail(HQ_E_INVALID, "null buffer");
  CosqArgs a = cosq_args(Q8, stats_q, Q, B8, stats_b, N, K);
  a.c.out = out;
  return launch_cosq<3, 0>(a, (hipStream_t)stream);
}

// Workspace layout and merge stage: hq_cos_topk's, as hq_cosq_topk.
size_t hq_cosqf_topk_workspace_size(int Q, int64_t N, int k) { return hq_cos_topk_workspace_size(Q, N, k); }

int hq_cosqf_topk(const void* Q8, const double* stats_q, int Q, const void* B8, const double* stats_b, int64_t N, int K,
                  int k, double threshold, int thr_mode, int64_t id_base, void* workspace, size_t workspace_bytes,
                  double* out_score, int64_t* out_id, hq_stream_t stream) {
  bool run;
  const int rc = cos_topk_check(Q, N, K, k, Q8 && stats_q && B8 && stats_b && workspace && out_score && out_id,
                                workspace_bytes, &run, [&] {
    if (K > kCosqMaxK) return fail(HQ_E_UNSUPPORTED, "K=%d: the int32 accumulators hold K <= %d", K, kCosqMaxK);
    return HQ_OK;
  });
  if (!run) return rc;
  const hipStream_t s = (hipStream_t)stream;
  CosqArgs a = cosq_args(Q8, stats_q, Q, B8, stats_b, N, K);
  return cos_topk_run(Q, N, k, threshold, thr_mode, id_base, workspace, out_score, out_id, s, a.c,
                      [&] { return launch_cosq<3, 4>(a, s); });
}

}  // extern "C"
