// hq_hier.hip — the RAG engine's progressive hierarchical search (rag/search/engine.py:51-95, 97-162, 178-287) over
// a resident frame corpus: the candidate cascade that runs before the comprehensive score.
//
//   hq_hier_prepare   frames [N, H, W] + hq_comp_describe descriptors -> the compacted, trimmed index rows as float64
//                     [N, max_levels, W] (zero beyond each trimmed length) and their lengths int32 [N, max_levels]
//                     (0: the frame has no such level).  One launch, one wave per frame.
//   hq_hier_filter    a query batch against the prepared corpus, no host round trip between levels:
//                       k_hier_scores   S[l][q][i] = s_l(q, i), every level, float64, into the workspace;
//                       k_hier_cascade  one workgroup per query: per level the cut, then the first kout of the list.
//
// The level score s_l(q, c) is 0.0 when c has no level l, else (cos + 1) / 2 over the first m = min(len_q, len_c)
// values of the two trimmed rows, 0.0 when a truncated norm is 0.  Dot product and both prefix square norms are
// float64 sums in element order, so a score depends on the two rows only: bit-identical frames score bit-identically
// against every query, which the id tie-break below relies on.
//
// The reference sorts the survivors stably by s_l at every level and keeps, in order, those with s_l >= thr_l until
// cap_l = max(1, int(n_prev ratio_l)) are kept.  Since a stable sort of a list ordered by (s_{l-1}, ..., s_0, id) gives
// the order (s_l desc, s_{l-1} desc, ..., s_0 desc, id asc), the survivors of level l are the first cap_l elements of
// that lexicographic order among the alive entries with s_l >= thr_l, and the final list is one such order.  Per query
// and level this is ONE cut key, found by an MSD radix select (11-bit digits, an LDS histogram per digit) over the
// multi-word key
//     [ord(s_l), ord(s_{l-1}), ..., ord(s_0), N - 1 - id]      ord = the monotone map of a double onto uint64
// which stops as soon as the bucket holding the cap-th element is taken whole.  Keys are distinct (the id word), so
// ties at any level, and whole stores of duplicates, need no special case.  A NaN score fails s_l >= thr_l and never
// enters a key.
#include "hq_common.h"

#include <math.h>

namespace hq {

constexpr int kHierMaxLevels = 8;
constexpr int kHierMaxK = 64;
constexpr int kHierTQ = 16;        // queries one k_hier_scores workgroup stages
constexpr int kHierMaxW = 512;     // 16 (2 W + 1) float64 in LDS
constexpr int kHierBits = 11;      // radix digit
constexpr int kHierBins = 1 << kHierBits;
constexpr int kHierDigits = 6;     // 5 x 11 + 9 bits
constexpr int kHierThreads = 1024;

struct HierTables {
  double thr[kHierMaxLevels];
  double ratio[kHierMaxLevels];
};

// ---- prepare ------------------------------------------------------------------------------------------------
template <typename T>
__global__ __launch_bounds__(64) void k_hier_prepare(const T* __restrict__ imgs, int64_t N, int64_t ld, int H, int W,
                                                     const int* __restrict__ desc, int ML, double* __restrict__ rows,
                                                     int* __restrict__ lens, int* __restrict__ flag) {
  const int lane = threadIdx.x;
  for (int64_t i = blockIdx.x; i < N; i += gridDim.x) {
    const T* img = imgs + i * ld;
    // the height is clamped to [1, H]: a descriptor this library did not write cannot steer a read outside a frame
    const int h = min(max(desc[4 * i], 1), H);
    unsigned mask = (unsigned)desc[4 * i + 3];
    double* out = rows + i * (int64_t)ML * W;
    int l = 0;
    while (mask) {
      const int r = h + __ffs(mask) - 1;
      mask &= mask - 1;
      if (r >= H) break;
      if (l >= ML) {
        if (lane == 0 && flag) *flag = 1;
        break;
      }
      int last = -1;
      for (int c = lane; c < W; c += 64) {
        const T v = img[(int64_t)r * W + c];
        out[(int64_t)l * W + c] = (double)v;
        if (v != (T)0) last = c;
      }
      for (int o = 32; o > 0; o >>= 1) {
        const int other = __shfl_xor(last, o, 64);
        last = other > last ? other : last;
      }
      if (lane == 0) lens[i * ML + l] = last + 1;  // (a row of the mask is non-zero: last >= 0)
      ++l;
    }
    for (; l < ML; ++l) {
      for (int c = lane; c < W; c += 64) out[(int64_t)l * W + c] = 0.0;
      if (lane == 0) lens[i * ML + l] = 0;
    }
  }
}

// ---- level scores -------------------------------------------------------------------------------------------
// Workgroup (x, y): candidates 256 x .. 256 x + 255 (one per thread) against queries 16 y .. 16 y + 15, level by
// level.  LDS: the 16 query rows of the level [16][W] and their prefix square norms [16][W + 1] (element order).
// A thread walks its candidate row once per level and query tile: the dot products of the 16 queries stay in
// registers, the candidate's prefix norm is latched where a shorter query ends.
__global__ __launch_bounds__(256) void k_hier_scores(const double* __restrict__ qr, const int* __restrict__ ql,
                                                     const int* __restrict__ Lq, int Q, const double* __restrict__ cr,
                                                     const int* __restrict__ cl, int64_t N, int W, int ML,
                                                     double* __restrict__ S) {
  extern __shared__ double sm[];
  double* qs = sm;                          // [16][W]
  double* qp = sm + (size_t)kHierTQ * W;    // [16][W + 1]
  __shared__ int qlen[kHierTQ];
  const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
  for (int q0 = blockIdx.y * kHierTQ; q0 < Q; q0 += gridDim.y * kHierTQ) {
    const int nq = Q - q0 < kHierTQ ? Q - q0 : kHierTQ;
    for (int l = 0; l < ML; ++l) {
      __syncthreads();  // the previous level's readers are done
      for (int e = threadIdx.x; e < kHierTQ * W; e += 256) {
        const int t = e / W, k = e - t * W;
        qs[e] = t < nq ? qr[((int64_t)(q0 + t) * ML + l) * W + k] : 0.0;
      }
      if (threadIdx.x < kHierTQ) {
        const int t = threadIdx.x;
        int len = 0;
        if (t < nq && l < Lq[q0 + t]) len = min(max(ql[(int64_t)(q0 + t) * ML + l], 0), W);
        qlen[t] = len;
      }
      __syncthreads();
      if (threadIdx.x < kHierTQ) {
        const int t = threadIdx.x;
        double acc = 0.0;
        qp[t * (W + 1)] = 0.0;
        for (int k = 0; k < W; ++k) {
          const double x = qs[t * W + k];
          acc = fma(x, x, acc);
          qp[t * (W + 1) + k + 1] = acc;
        }
      }
      __syncthreads();
      if (i < N) {
        const int lc = min(max(cl[i * ML + l], 0), W);
        const double* y = cr + (i * ML + l) * (int64_t)W;
        double dot[kHierTQ], ncs[kHierTQ];
        int lqv[kHierTQ];
#pragma unroll
        for (int t = 0; t < kHierTQ; ++t) {
          dot[t] = ncs[t] = 0.0;
          lqv[t] = qlen[t];
        }
        double nc = 0.0;
        for (int k = 0; k < lc; ++k) {
          const double v = y[k];
          nc = fma(v, v, nc);
#pragma unroll
          for (int t = 0; t < kHierTQ; ++t) {
            if (k < lqv[t]) dot[t] = fma(qs[t * W + k], v, dot[t]);
            if (k + 1 == lqv[t]) ncs[t] = nc;
          }
        }
#pragma unroll
        for (int t = 0; t < kHierTQ; ++t) {
          if (t < nq) {
            const int lq = lqv[t];
            double s = 0.0;
            if (lq > 0 && lc > 0) {
              const int m = lq < lc ? lq : lc;
              const double na = qp[t * (W + 1) + m], nb = lq < lc ? ncs[t] : nc;
              if (na != 0.0 && nb != 0.0) s = (dot[t] / (sqrt(na) * sqrt(nb)) + 1.0) / 2.0;
            }
            S[((int64_t)l * Q + q0 + t) * N + i] = s;
          }
        }
      }
    }
  }
}

// ---- cascade ------------------------------------------------------------------------------------------------
// monotone map of a double onto uint64 (negative values below positive ones; a score is (cos + 1) / 2, which
// rounding can leave a hair below zero)
__device__ __forceinline__ uint64_t hier_ord(double s) {
  const uint64_t u = (uint64_t)__double_as_longlong(s);
  return (u >> 63) ? ~u : (u | 0x8000000000000000ull);
}

struct HierSel {
  uint64_t cut[kHierMaxLevels + 1];  // the cut key's words; words past `words` are 0
  int words;                          // words the select fixed (0: every eligible entry passes)
};

// shared state of one cascade workgroup
struct HierShared {
  unsigned hist[kHierBins];
  HierSel sel;
  int64_t krem;       // elements still to take inside the current bucket
  int64_t bucket;     // size of the bucket the cut lies in
  int64_t total;      // eligible entries (first pass)
  int done;
  int lcount;
  int64_t list[kHierMaxK];
};

// word w of entry i's key with top level T: the scores of levels T, T - 1, ..., 0, then N - 1 - i
__device__ __forceinline__ uint64_t hier_word(const double* __restrict__ Sq, int64_t QN, int64_t N, int T, int w,
                                              int64_t i) {
  return w <= T ? hier_ord(Sq[(int64_t)(T - w) * QN + i]) : (uint64_t)(N - 1 - i);
}

__device__ __forceinline__ int hier_shift(int d) {
  const int s = 64 - kHierBits * (d + 1);
  return s < 0 ? 0 : s;
}
__device__ __forceinline__ int hier_width(int d) { return d < kHierDigits - 1 ? kHierBits : 64 - kHierBits * (kHierDigits - 1); }

// key(i) >= the cut key
__device__ __forceinline__ bool hier_passes(const HierSel& sel, const double* __restrict__ Sq, int64_t QN, int64_t N,
                                            int T, int64_t i) {
  for (int w = 0; w < sel.words; ++w) {
    const uint64_t k = hier_word(Sq, QN, N, T, w, i);
    if (k != sel.cut[w]) return k > sel.cut[w];
  }
  return true;
}

// The cut key of the first `k` entries (k >= 1), by key descending, among the eligible ones: alive[i] == need and
// (thr_on: S_T[i] >= thr).  Returns the number taken, min(k, eligible); sh.sel holds the key (words = 0 when every
// eligible entry is taken).  Called by the whole workgroup; uniform control flow.
__device__ int64_t hier_select(HierShared& sh, const double* __restrict__ Sq, int64_t QN, int64_t N, int T,
                               const uint8_t* __restrict__ alive, int need, bool thr_on, double thr, int64_t k) {
  const int tid = threadIdx.x;
  if (tid == 0) {
    sh.sel.words = 0;
    for (int w = 0; w <= kHierMaxLevels; ++w) sh.sel.cut[w] = 0;
    sh.krem = k;
    sh.done = 0;
  }
  for (int w = 0; w <= T + 1; ++w) {
    for (int d = 0; d < kHierDigits; ++d) {
      for (int b = tid; b < kHierBins; b += kHierThreads) sh.hist[b] = 0;
      __syncthreads();
      const int shift = hier_shift(d), width = hier_width(d);
      const uint64_t cur = sh.sel.cut[w];
      for (int64_t i = tid; i < N; i += kHierThreads) {
        if (alive[i] != need) continue;
        if (thr_on && !(Sq[(int64_t)T * QN + i] >= thr)) continue;
        bool match = true;
        for (int v = 0; v < w && match; ++v) match = hier_word(Sq, QN, N, T, v, i) == sh.sel.cut[v];
        if (!match) continue;
        const uint64_t key = hier_word(Sq, QN, N, T, w, i);
        if (d > 0 && (key >> (shift + width)) != (cur >> (shift + width))) continue;
        atomicAdd(&sh.hist[(unsigned)((key >> shift) & ((1u << width) - 1))], 1u);
      }
      __syncthreads();
      if (tid < 64) {
        // lane j owns the 32 bins 2047 - 32 j .. 2016 - 32 j (from the top); an exclusive scan over the lanes finds
        // the lane whose chunk holds the krem-th element, which then walks its bins
        const int top = kHierBins - 1 - 32 * tid;
        int64_t c = 0;
        for (int b = 0; b < 32; ++b) c += sh.hist[top - b];
        int64_t inc = c;
        for (int o = 1; o < 64; o <<= 1) {
          const int64_t up = __shfl_up(inc, o, 64);
          if (tid >= o) inc += up;
        }
        const int64_t tot = __shfl(inc, 63, 64);
        const bool first = (w == 0 && d == 0);
        const int64_t kr = sh.krem;
        if (first && tid == 0) sh.total = tot;
        if (first && tot <= kr) {
          if (tid == 0) sh.done = 2;  // every eligible entry is taken
        } else {
          int64_t above = inc - c;
          if (above < kr && kr <= inc) {
            int b = 0;
            for (; b < 32; ++b) {
              const int64_t n = sh.hist[top - b];
              if (kr <= above + n) break;
              above += n;
            }
            if (b > 31) b = 31;  // (cannot happen: the chunk holds the krem-th element)
            const int64_t n = sh.hist[top - b];
            sh.sel.cut[w] = cur | ((uint64_t)(top - b) << shift);
            sh.sel.words = w + 1;
            sh.krem = kr - above;
            sh.bucket = n;
            if (kr - above == n) sh.done = 1;  // the bucket is taken whole: the key so far is the cut
          }
        }
      }
      __syncthreads();
      if (sh.done) break;
    }
    if (sh.done) break;
  }
  const int64_t taken = sh.done == 2 ? sh.total : k;
  __syncthreads();
  return taken;
}

__global__ __launch_bounds__(kHierThreads) void k_hier_cascade(const double* __restrict__ S, const int* __restrict__ Lq,
                                                               int Q, int64_t N, int ML, HierTables tab, int kout,
                                                               uint8_t* __restrict__ alive_all,
                                                               int64_t* __restrict__ out_count,
                                                               int64_t* __restrict__ out_ids,
                                                               double* __restrict__ out_scores) {
  __shared__ HierShared sh;
  const int tid = threadIdx.x;
  const int64_t QN = (int64_t)Q * N;
  for (int q = blockIdx.x; q < Q; q += gridDim.x) {
    const double* Sq = S + (int64_t)q * N;  // level l of this query: Sq + l QN
    uint8_t* alive = alive_all + (int64_t)q * N;
    const int L = Lq[q];
    const int levels = L < ML ? (L < 0 ? 0 : L) : ML;
    for (int64_t i = tid; i < N; i += kHierThreads) alive[i] = 0;
    __syncthreads();
    int64_t n = N;
    for (int l = 0; l < ML; ++l) {
      if (l >= levels || n == 0) {
        if (tid == 0) out_count[(int64_t)q * ML + l] = 0;  // the cascade has ended (l >= L_q) or stopped (nobody left)
        continue;
      }
      int64_t cap = (int64_t)((double)n * tab.ratio[l]);  // int(n * ratio), the same IEEE product as Python's
      if (cap < 1) cap = 1;
      const double thr = tab.thr[l];
      n = hier_select(sh, Sq, QN, N, l, alive, l, true, thr, cap);
      // each thread rewrites only the entries it reads in every pass (i = tid mod 1024): no fence is needed
      for (int64_t i = tid; i < N; i += kHierThreads)
        if (alive[i] == l && Sq[(int64_t)l * QN + i] >= thr && hier_passes(sh.sel, Sq, QN, N, l, i))
          alive[i] = (uint8_t)(l + 1);
      if (tid == 0) out_count[(int64_t)q * ML + l] = n;
      __syncthreads();
    }
    // a query with more levels than the corpus rows hold: no frame has level ML, nothing survives it
    if (L > ML || levels == 0) n = 0;
    // the first kout of the final list
    int cnt = 0;
    if (n > 0 && kout > 0) {
      const int T = levels - 1;
      const int64_t taken = hier_select(sh, Sq, QN, N, T, alive, levels, false, 0.0, kout);
      if (tid == 0) sh.lcount = 0;
      __syncthreads();
      for (int64_t i = tid; i < N; i += kHierThreads)
        if (alive[i] == levels && hier_passes(sh.sel, Sq, QN, N, T, i)) {
          const int p = atomicAdd(&sh.lcount, 1);
          if (p < kHierMaxK) sh.list[p] = i;
        }
      __syncthreads();
      cnt = (int)taken < kHierMaxK ? (int)taken : kHierMaxK;
      if (tid < cnt) {
        const int64_t me = sh.list[tid];
        int rank = 0;
        for (int u = 0; u < cnt; ++u) {
          const int64_t other = sh.list[u];
          if (other == me) continue;
          bool greater = other < me;  // every score word equal: the smaller id comes first
          for (int w = 0; w <= T; ++w) {
            const uint64_t a = hier_word(Sq, QN, N, T, w, other), b = hier_word(Sq, QN, N, T, w, me);
            if (a != b) { greater = a > b; break; }
          }
          rank += greater ? 1 : 0;
        }
        out_ids[(int64_t)q * kout + rank] = me;
        for (int l = 0; l < ML; ++l)
          out_scores[((int64_t)q * kout + rank) * ML + l] = l < levels ? Sq[(int64_t)l * QN + me] : 0.0;
      }
    }
    for (int p = cnt + tid; p < kout; p += kHierThreads) {
      out_ids[(int64_t)q * kout + p] = -1;
      for (int l = 0; l < ML; ++l) out_scores[((int64_t)q * kout + p) * ML + l] = 0.0;
    }
    __syncthreads();  // sh is reused by the next query
  }
}

static size_t hier_align(size_t n) { return (n + 255) & ~(size_t)255; }

}  // namespace hq

using namespace hq;

extern "C" {

int hq_hier_prepare(int dtype, const void* imgs, int64_t N, int64_t ld, int H, int W, const int32_t* desc,
                    int max_levels, double* rows, int32_t* lens, hq_stream_t stream) {
  if (N < 0 || H <= 0 || W <= 0 || ld < (int64_t)H * W) return fail(HQ_E_INVALID, "bad shape");
  if (max_levels < 1 || max_levels > kHierMaxLevels)
    return fail(HQ_E_INVALID, "max_levels %d (1 .. %d)", max_levels, kHierMaxLevels);
  if (dtype != HQ_F32 && dtype != HQ_F64) return fail(HQ_E_UNSUPPORTED, "dtype %d (float32 / float64)", dtype);
  if (N == 0) return HQ_OK;
  if (!imgs || !desc || !rows || !lens) return fail(HQ_E_INVALID, "null buffer");
  const hipStream_t s = (hipStream_t)stream;
  // only frames of more than max_levels + 1 rows can have more than max_levels index rows: those launches carry a
  // flag that is read back (one 4-byte copy and a stream synchronisation)
  int* flag = nullptr;
  if (H - 1 > max_levels) {
    HQ_CHECK_HIP(hipMalloc((void**)&flag, sizeof(int)));
    hipError_t e = hipMemsetAsync(flag, 0, sizeof(int), s);
    if (e != hipSuccess) {
      (void)hipFree(flag);
      return fail(HQ_E_HIP, "hipMemsetAsync: %s", hipGetErrorString(e));
    }
  }
  const int g = (int)(N < 65536 ? N : 65536);
  if (dtype == HQ_F32)
    hipLaunchKernelGGL(k_hier_prepare<float>, dim3(g), dim3(64), 0, s, (const float*)imgs, N, ld, H, W, desc, max_levels,
                       rows, lens, flag);
  else
    hipLaunchKernelGGL(k_hier_prepare<double>, dim3(g), dim3(64), 0, s, (const double*)imgs, N, ld, H, W, desc,
                       max_levels, rows, lens, flag);
  hipError_t le = hipGetLastError();
  int over = 0;
  if (flag) {
    if (le == hipSuccess) le = hipMemcpyAsync(&over, flag, sizeof(int), hipMemcpyDeviceToHost, s);
    if (le == hipSuccess) le = hipStreamSynchronize(s);
    (void)hipFree(flag);
  }
  if (le != hipSuccess) return fail(HQ_E_HIP, "hq_hier_prepare: %s", hipGetErrorString(le));
  if (over) return fail(HQ_E_UNSUPPORTED, "a frame has more than %d non-zero index rows", max_levels);
  return HQ_OK;
}

size_t hq_hier_workspace_size(int Q, int64_t N, int max_levels) {
  if (Q <= 0 || N <= 0 || max_levels <= 0) return 0;
  return hier_align((size_t)max_levels * (size_t)Q * (size_t)N * 8) + hier_align((size_t)Q * (size_t)N);
}

int hq_hier_filter(const double* q_rows, const int32_t* q_lens, const int32_t* Lq, int Q, const double* c_rows,
                   const int32_t* c_lens, int64_t N, int W, int max_levels, const double* thr, const double* ratio,
                   int kout, void* ws, int64_t* out_count, int64_t* out_top_ids, double* out_top_scores,
                   uint8_t* out_alive, hq_stream_t stream) {
  if (Q < 0 || N < 0 || W <= 0 || kout < 0) return fail(HQ_E_INVALID, "bad shape");
  if (max_levels < 1 || max_levels > kHierMaxLevels)
    return fail(HQ_E_INVALID, "max_levels %d (1 .. %d)", max_levels, kHierMaxLevels);
  if (kout > kHierMaxK) return fail(HQ_E_UNSUPPORTED, "kout %d (at most %d)", kout, kHierMaxK);
  if (W > kHierMaxW) return fail(HQ_E_UNSUPPORTED, "index rows of %d values (at most %d)", W, kHierMaxW);
  if (Q == 0) return HQ_OK;
  if (!out_count) return fail(HQ_E_INVALID, "null buffer");
  const hipStream_t s = (hipStream_t)stream;
  if (N == 0) {
    HQ_CHECK_HIP(hipMemsetAsync(out_count, 0, (size_t)Q * max_levels * sizeof(int64_t), s));
    return HQ_OK;
  }
  if (!q_rows || !q_lens || !Lq || !c_rows || !c_lens || !thr || !ratio || !ws || (kout > 0 && (!out_top_ids || !out_top_scores)))
    return fail(HQ_E_INVALID, "null buffer");
  if (N > 0x7FFFFFFF) return fail(HQ_E_UNSUPPORTED, "too many frames");  // 32-bit histogram counts
  HierTables tab;
  for (int l = 0; l < kHierMaxLevels; ++l) {
    tab.thr[l] = l < max_levels ? thr[l] : 0.0;
    tab.ratio[l] = l < max_levels ? ratio[l] : 0.0;
  }
  double* S = (double*)ws;
  uint8_t* alive = out_alive ? out_alive
                             : (uint8_t*)ws + hier_align((size_t)max_levels * (size_t)Q * (size_t)N * 8);
  const size_t lds = (size_t)kHierTQ * (2 * (size_t)W + 1) * 8;
  HQ_CHECK_HIP(hipFuncSetAttribute((const void*)k_hier_scores, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
  const int qt = (Q + kHierTQ - 1) / kHierTQ;
  hipLaunchKernelGGL(k_hier_scores, dim3((unsigned)((N + 255) / 256), (unsigned)(qt < 65535 ? qt : 65535)), dim3(256),
                     lds, s, q_rows, q_lens, Lq, Q, c_rows, c_lens, N, W, max_levels, S);
  HQ_CHECK_LAUNCH();
  hipLaunchKernelGGL(k_hier_cascade, dim3((unsigned)(Q < 65536 ? Q : 65536)), dim3(kHierThreads), 0, s, S, Lq, Q, N,
                     max_levels, tab, kout, alive, out_count, out_top_ids, out_top_scores);
  HQ_CHECK_LAUNCH();
  return HQ_OK;
}

}  // extern "C"
