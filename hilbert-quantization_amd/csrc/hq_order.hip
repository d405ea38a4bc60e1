// hq_order.hip — greedy frame ordering of a video store on the device (DESIGN.md §frame ordering).
//
// Reference: core/video_storage.py
//   :762-781   _calculate_hierarchical_similarity   (np.std branches, np.allclose, (np.corrcoef + 1) / 2)
//   :1203-1277 _sort_frames_by_hierarchical_indices (start nearest the centroid, then greedy nearest neighbour)
//   :1445-1522 get_frame_ordering_metrics, _calculate_ordering_efficiency
//   :1751-1803 _find_optimal_insertion_position
//
// The reference evaluates one np.corrcoef per pair from a Python loop (N^2 / 2 calls per sort).  Here the rows
// are centred and normalised once (k_order_prepare), all pair similarities are one f64 MFMA contraction
// (k_order_sims, v_mfma_f64_16x16x4f64) into a resident matrix S, and the sequential greedy chain reads one row
// of S per step from a single workgroup (k_order_walk).  Neighbour metrics (k_order_pairs, k_order_stats) and
// insertion positions (k_order_insert) use the same pair similarity.
//
// Pair similarity of query row a and candidate row b: a row is constant when np.std is exactly 0 in NumPy's
// summation order (np_sum16 below follows pairwise_sum like hq_common.h np_sum); a pair with a constant row
// scores 1.0 / 0.0 by np.allclose(a, b) on the raw rows, every other pair min(1, max(0, (r + 1) / 2)) with r the
// dot product of the two centred unit rows, clipped to [-1, 1].
#include "hq_common.h"

#include <limits.h>

namespace hq {

typedef double ord_d4 __attribute__((ext_vector_type(4)));

constexpr int kOrdMaxL = 256;      // longest index row
constexpr int kOrdMaxN = 16384;    // greedy: the matrix S is 8 Np^2 bytes (2 GiB here)
constexpr int kOrdTile = 64;       // k_order_sims: S tile side of one workgroup
constexpr int kOrdKC = 32;         // K values staged per round
constexpr int kOrdRS = kOrdKC + 2; // LDS row stride in doubles (2 mod 32: rows 16 B apart in the banks)
constexpr int kOrdWalkT = 1024;    // walker workgroup
constexpr uint8_t kOrdConst = 1, kOrdPad = 2, kOrdBad = 4;

// ------------------------------------------------------------------------------------------------
// 16 lanes per row.  np_sum16: np.add.reduce over f(0 .. n-1), n <= 256, in NumPy's pairwise order, by the 16
// lanes of an aligned group (every lane returns the sum).  n < 8: sequential from -0.0 (each lane alone).
// n <= 128 is one leaf: lane j of each half keeps accumulator r_j over k = j, j + 8, ...; xor-shuffles 1, 2, 4
// form ((r0+r1)+(r2+r3))+((r4+r5)+(r6+r7)) (+ is commutative, so both partners of a shuffle hold the same
// bits); the tail is added sequentially (np_leaf8).  n > 128 splits at n/2 rounded down to a multiple of 8: lanes
// 0-7 take the first half, lanes 8-15 the second, one more shuffle adds them.  For n = 249 .. 255 the second half
// holds 129 .. 135 values and NumPy splits it once more (64 + the rest): lanes 8-15 then run its two leaves one
// after the other and add them (lanes 0-7 only take part in the shuffles).  The identity 0 is added first.
// ------------------------------------------------------------------------------------------------
// one pairwise leaf of m >= 8 values from f(off) by the eight lanes j = 0 .. 7 of a half group; !live: shuffles only
template <class F>
__device__ __forceinline__ double np_leaf8(const F& f, int off, int m, int j, bool live) {
  const int lim = live ? m - (m % 8) : 0;
  double r = live ? f(off + j) : 0.0;
  for (int i = 8; i < lim; i += 8) r = r + f(off + i + j);
  r = r + __shfl_xor(r, 1, 64);
  r = r + __shfl_xor(r, 2, 64);
  r = r + __shfl_xor(r, 4, 64);
  if (live)
    for (int i = lim; i < m; ++i) r = r + f(off + i);
  return r;
}

template <class F>
__device__ __forceinline__ double np_sum16(const F& f, int n, int l) {
  if (n < 8) {
    double r = -0.0;
    for (int i = 0; i < n; ++i) r = r + f(i);
    return 0.0 + r;
  }
  const int j = l & 7;
  if (n <= 128) return 0.0 + np_leaf8(f, 0, n, j, true);
  const bool hi = (l & 8) != 0;
  int n2 = n / 2;
  n2 -= n2 % 8;
  const int off = hi ? n2 : 0;
  int m = hi ? n - n2 : n2;
  const bool split2 = n - n2 > 128;  // uniform: only the second half can exceed a leaf (n <= 256)
  int mb = 0;
  if (split2 && hi) {
    mb = m;
    m = m / 2;
    m -= m % 8;
    mb -= m;
  }
  double r = np_leaf8(f, off, m, j, true);
  if (split2) {
    const double rb = np_leaf8(f, off + m, mb, j, hi);
    if (hi) r = r + rb;
  }
  r = r + __shfl_xor(r, 8, 64);
  return 0.0 + r;
}

// sum over the 16 lanes of a group in a fixed order (xor 1, 2, 4, 8); every lane returns it
__device__ __forceinline__ double sum16(double v) {
  v = v + __shfl_xor(v, 1, 64);
  v = v + __shfl_xor(v, 2, 64);
  v = v + __shfl_xor(v, 4, 64);
  v = v + __shfl_xor(v, 8, 64);
  return v;
}
__device__ __forceinline__ int and16(int v) {
  v &= __shfl_xor(v, 1, 64);
  v &= __shfl_xor(v, 2, 64);
  v &= __shfl_xor(v, 4, 64);
  v &= __shfl_xor(v, 8, 64);
  return v;
}

// np.allclose(a, b) element: |a - b| <= 1e-8 + 1e-5 |b| (asymmetric in the candidate b)
__device__ __forceinline__ bool ord_close(double a, double b) { return fabs(a - b) <= 1e-8 + 1e-5 * fabs(b); }

// r (dot of two centred unit rows) -> similarity (:778-781)
__device__ __forceinline__ double ord_sim(double r) {
  r = r > 1.0 ? 1.0 : (r < -1.0 ? -1.0 : r);
  const double s = (r + 1.0) / 2.0;
  return s < 1.0 ? (s > 0.0 ? s : 0.0) : 1.0;
}

// ------------------------------------------------------------------------------------------------
// k_order_prepare: rows X [N, L] (row stride ldx) -> Z [Np, Lp] centred unit rows and flags [Np].
// 16 rows per 256-thread workgroup, 16 lanes per row.  mean = np.mean, the deviation sum ss in NumPy's order
// too: np.std = sqrt(ss / L), and the row is constant exactly when that is 0.0.  z = (x - mean) / sqrt(ss).
// Constant rows, rows holding a NaN or inf (kOrdBad) and the pad rows N .. Np-1 (kOrdPad) are written as zeros,
// as are the columns L .. Lp-1.
// ------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void k_order_prepare(const double* __restrict__ X, int N, int64_t ldx, int L, int Lp,
                                                       double* __restrict__ Z, uint8_t* __restrict__ flags) {
  const int l = threadIdx.x & 15;
  const int row = blockIdx.x * 16 + (threadIdx.x >> 4);  // < Np: the grid is Np / 16
  const bool live = row < N;
  const double* x = X + (int64_t)(live ? row : 0) * ldx;
  int fin = 1;
  for (int k = l; k < L; k += 16) fin &= (fabs(x[k]) <= 1.79769313486231570815e308) ? 1 : 0;  // false for NaN, inf
  fin = and16(fin);
  const double mean = np_sum16([=](int k) { return x[k]; }, L, l) / (double)L;
  const double ss = np_sum16([=](int k) { const double d = x[k] - mean; return d * d; }, L, l);
  const bool constant = sqrt(ss / (double)L) == 0.0;
  const bool zero = !live || !fin || constant;
  const double nrm = sqrt(ss);
  for (int k = l; k < Lp; k += 16) Z[(int64_t)row * Lp + k] = (zero || k >= L) ? 0.0 : (x[k] - mean) / nrm;
  if (l == 0) flags[row] = !live ? kOrdPad : (!fin ? kOrdBad : (constant ? kOrdConst : 0));
}

// ------------------------------------------------------------------------------------------------
// k_order_sims: S[i][j] = similarity of query row i (Za, fa, Xa) and candidate row j (Zb, fb, Xb), i < M, j < N.
// One 256-thread workgroup owns a 64 x 64 tile of S.  Per round of kOrdKC = 32 K values both operand panels
// (64 rows x 32 doubles each) go through LDS once, as 16-byte pieces, rows kOrdRS = 34 doubles apart; wave w
// owns the 16 query rows 16 w .. 16 w + 15 and all four 16-column blocks: per K step of 4 one A read, four B
// reads and four v_mfma_f64_16x16x4f64 into four accumulators (32 VGPRs).  Operand layout (as hq_search.hip):
// A lane = row (lane & 15), k = lane >> 4; B lane = column (lane & 15), k = lane >> 4; accumulator element r
// = row (lane >> 4) + 4 r, column lane & 15.  Every column sees the K steps in the same order 0 .. Lp/4 - 1, so
// two bit-identical candidate rows get bit-identical similarities against any query row (the walker's tie rule
// needs that).  Epilogue: clip, affine map, clamp; an entry whose row or column is constant is replaced by
// np.allclose on the raw rows (rare: the loop over L runs only there).  Only i < M, j < N is stored.
// ------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void k_order_sims(const double* __restrict__ Za, const uint8_t* __restrict__ fa,
                                                    const double* __restrict__ Xa, int64_t lda, int M, int Mp,
                                                    const double* __restrict__ Zb, const uint8_t* __restrict__ fb,
                                                    const double* __restrict__ Xb, int64_t ldb, int N, int Np, int L,
                                                    int Lp, double* __restrict__ S, int64_t ldS) {
  __shared__ __attribute__((aligned(16))) double pa[kOrdTile * kOrdRS];
  __shared__ __attribute__((aligned(16))) double pb[kOrdTile * kOrdRS];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int i0 = blockIdx.y * kOrdTile, j0 = blockIdx.x * kOrdTile;
  ord_d4 acc[4];
#pragma unroll
  for (int cb = 0; cb < 4; ++cb) acc[cb] = ord_d4{0.0, 0.0, 0.0, 0.0};
  const double* arow = pa + (wave * 16 + (lane & 15)) * kOrdRS + (lane >> 4);
  const double* brow = pb + (lane & 15) * kOrdRS + (lane >> 4);
  for (int k0 = 0; k0 < Lp; k0 += kOrdKC) {
    const int kc = min(kOrdKC, Lp - k0);  // a multiple of 4
    const int ppr = kc >> 1;              // 16-byte pieces per row
    for (int p = tid; p < kOrdTile * ppr; p += 256) {
      const int r = p / ppr, kk = p - r * ppr;
      double2 va = make_double2(0.0, 0.0), vb = make_double2(0.0, 0.0);
      if (i0 + r < Mp) va = *reinterpret_cast<const double2*>(Za + (int64_t)(i0 + r) * Lp + k0 + 2 * kk);
      if (j0 + r < Np) vb = *reinterpret_cast<const double2*>(Zb + (int64_t)(j0 + r) * Lp + k0 + 2 * kk);
      *reinterpret_cast<double2*>(pa + r * kOrdRS + 2 * kk) = va;
      *reinterpret_cast<double2*>(pb + r * kOrdRS + 2 * kk) = vb;
    }
    __syncthreads();
    for (int t = 0; t < (kc >> 2); ++t) {
      const double a = arow[4 * t];
#pragma unroll
      for (int cb = 0; cb < 4; ++cb)
        acc[cb] = __builtin_amdgcn_mfma_f64_16x16x4f64(a, brow[cb * 16 * kOrdRS + 4 * t], acc[cb], 0, 0, 0);
    }
    __syncthreads();
  }
  const int ib = i0 + wave * 16 + (lane >> 4), jb = j0 + (lane & 15);
  uint32_t patch = 0u;  // bit 4 cb + r: the entry has a constant row or column
#pragma unroll
  for (int cb = 0; cb < 4; ++cb) {
    const int j = jb + cb * 16;
    if (j >= N) continue;
    const bool cconst = (fb[j] & kOrdConst) != 0;
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      const int i = ib + 4 * r;
      if (i >= M) continue;
      if (cconst || (fa[i] & kOrdConst)) patch |= 1u << (4 * cb + r);
      S[(int64_t)i * ldS + j] = ord_sim(acc[cb][r]);
    }
  }
  for (; patch; patch &= patch - 1) {
    const int e = __builtin_ctz(patch);
    const int i = ib + 4 * (e & 3), j = jb + 16 * (e >> 2);
    const double* a = Xa + (int64_t)i * lda;
    const double* b = Xb + (int64_t)j * ldb;
    bool close = true;
    for (int k = 0; k < L; ++k) close &= ord_close(a[k], b[k]);
    S[(int64_t)i * ldS + j] = close ? 1.0 : 0.0;
  }
}

// ------------------------------------------------------------------------------------------------
// Workgroup arg-max of (value, index): larger value first, lower index on equal values.  Wave stage: DPP
// butterfly (xor 1, xor 2, half-row mirror, row mirror) then the four row results by readlane; workgroup stage:
// lane 0 of every wave stores its pair to LDS slot set `par`, one barrier, every thread folds the slots in wave
// order — all threads return the same winner without a second barrier (callers alternate par between
// consecutive calls).  The rule is a total order, so any fold order gives the same winner.
// ------------------------------------------------------------------------------------------------
struct OrdSlots {
  double s[2][16];
  int i[2][16];
};
__device__ __forceinline__ bool ord_better(double os, int oi, double s, int i) {
  return os > s || (os == s && oi < i);
}
template <int CTRL>
__device__ __forceinline__ void ord_dpp_step(double& s, int& i) {
  const double os = __hiloint2double(dppi<CTRL>(__double2hiint(s)), dppi<CTRL>(__double2loint(s)));
  const int oi = dppi<CTRL>(i);
  if (ord_better(os, oi, s, i)) { s = os; i = oi; }
}
__device__ __forceinline__ void ord_wg_argmax(double& s, int& i, OrdSlots& sl, int par) {
  ord_dpp_step<0xB1>(s, i);
  ord_dpp_step<0x4E>(s, i);
  ord_dpp_step<0x141>(s, i);
  ord_dpp_step<0x140>(s, i);
  double ws = 0.0;
  int wi = INT_MAX;
#pragma unroll
  for (int q = 0; q < 4; ++q) {
    const double os = __hiloint2double(__builtin_amdgcn_readlane(__double2hiint(s), 16 * q),
                                       __builtin_amdgcn_readlane(__double2loint(s), 16 * q));
    const int oi = __builtin_amdgcn_readlane(i, 16 * q);
    if (q == 0 || ord_better(os, oi, ws, wi)) { ws = os; wi = oi; }
  }
  const int wave = threadIdx.x >> 6, nw = blockDim.x >> 6;
  if ((threadIdx.x & 63) == 0) { sl.s[par][wave] = ws; sl.i[par][wave] = wi; }
  __syncthreads();
  s = sl.s[par][0];
  i = sl.i[par][0];
  for (int w = 1; w < nw; ++w) {
    const double os = sl.s[par][w];
    const int oi = sl.i[par][w];
    if (ord_better(os, oi, s, i)) { s = os; i = oi; }
  }
}

// ------------------------------------------------------------------------------------------------
// k_order_start (:1220-1247): the row nearest the centroid.  One 1024-thread workgroup.  Centroid: thread
// (slice, column) adds rows slice, slice + nsl, ... of its column in order (nsl = 1024 / L slices), then one
// thread per column adds the nsl partials in order and divides by N.  Distances: 16 lanes per row, squared
// differences summed per lane then by sum16; sqrt as np.linalg.norm.  Strict <, the lowest index wins a tie.
// ------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(kOrdWalkT) void k_order_start(const double* __restrict__ X, int64_t ldx, int N, int L,
                                                           int64_t* __restrict__ start) {
  __shared__ double part[kOrdWalkT];
  __shared__ double cen[kOrdMaxL];
  __shared__ OrdSlots sl;
  const int tid = threadIdx.x;
  const int nsl = kOrdWalkT / L;
  if (tid < nsl * L) {
    const int c = tid % L, s0 = tid / L;
    double a = 0.0;
    for (int r = s0; r < N; r += nsl) a = a + X[(int64_t)r * ldx + c];
    part[tid] = a;
  }
  __syncthreads();
  if (tid < L) {
    double a = 0.0;
    for (int s = 0; s < nsl; ++s) a = a + part[s * L + tid];
    cen[tid] = a / (double)N;
  }
  __syncthreads();
  const int l = tid & 15;
  double bs = -INFINITY;
  int bi = INT_MAX;
  for (int r0 = 0; r0 < N; r0 += kOrdWalkT / 16) {  // uniform trip count: the shuffles need whole groups
    const int r = r0 + (tid >> 4);
    double d2 = 0.0;
    if (r < N)
      for (int k = l; k < L; k += 16) {
        const double d = X[(int64_t)r * ldx + k] - cen[k];
        d2 = d2 + d * d;
      }
    const double nd = -sqrt(sum16(d2));
    if (r < N && nd > bs) { bs = nd; bi = r; }
  }
  ord_wg_argmax(bs, bi, sl, 0);
  if (tid == 0) start[0] = bi == INT_MAX ? 0 : bi;
}

// ------------------------------------------------------------------------------------------------
// k_order_walk (:1249-1271): the greedy chain on the resident matrix, ONE workgroup of 1024 threads (no grid
// barrier, no waiting on other workgroups).  Thread t owns the column pairs p = t, t + 1024, ... (columns 2p,
// 2p + 1): per step it reads them from row `last` of S as 16-byte loads (four in flight per round, the pair
// index clamped so the loads are unconditional), skips visited columns (bitmap in LDS) and columns >= N, and
// keeps the best (similarity, column) with strict > from -1.0 — its columns ascend, so the lowest index wins
// inside a thread, and ord_wg_argmax keeps the lower index between threads: the reference's scan of
// remaining_frames in original order with `similarity > best_similarity`.  The winner's bit is set by the
// thread that owns the column (the only one that reads it, in program order), so a step costs one barrier.
// Ranks the final similarities, not r: rounding of (r + 1) / 2 and the clamp create ties that r does not have.
// A row of S holding no value above -1.0 (NaN: outside the contract) ends the chain with -1 entries.
// ------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(kOrdWalkT) void k_order_walk(const double* __restrict__ S, int64_t ldS, int N,
                                                          const int64_t* __restrict__ start,
                                                          int64_t* __restrict__ order, double* __restrict__ step_sims) {
  __shared__ uint32_t vis[kOrdMaxN / 32];
  __shared__ OrdSlots sl;
  const int tid = threadIdx.x;
  for (int w = tid; w < kOrdMaxN / 32; w += kOrdWalkT) vis[w] = 0u;
  __syncthreads();
  int last = (int)start[0];
  if (last < 0 || last >= N) last = 0;
  if (((last >> 1) & (kOrdWalkT - 1)) == tid) atomicOr(&vis[last >> 5], 1u << (last & 31));
  if (tid == 0) order[0] = last;
  const int npairs = (N + 1) >> 1;
  for (int t = 1; t < N; ++t) {
    const double* row = S + (int64_t)last * ldS;
    double bs = -1.0;
    int bi = INT_MAX;
    for (int p0 = 0; p0 < npairs; p0 += 4 * kOrdWalkT) {
      double2 v[4];
      uint32_t w[4];
#pragma unroll
      for (int u = 0; u < 4; ++u) {
        const int p = min(p0 + u * kOrdWalkT + tid, npairs - 1);
        v[u] = *reinterpret_cast<const double2*>(row + 2 * p);
        w[u] = vis[p >> 4] >> ((2 * p) & 31);
      }
#pragma unroll
      for (int u = 0; u < 4; ++u) {
        const int p = p0 + u * kOrdWalkT + tid;
        const int j = 2 * p;
        if (p < npairs) {
          if (!(w[u] & 1u) && v[u].x > bs) { bs = v[u].x; bi = j; }
          if (j + 1 < N && !(w[u] & 2u) && v[u].y > bs) { bs = v[u].y; bi = j + 1; }
        }
      }
    }
    ord_wg_argmax(bs, bi, sl, t & 1);
    if (bi == INT_MAX) {  // uniform: every thread holds the same winner
      for (int q = t + tid; q < N; q += kOrdWalkT) { order[q] = -1; step_sims[q - 1] = bs; }
      return;
    }
    if (((bi >> 1) & (kOrdWalkT - 1)) == tid) atomicOr(&vis[bi >> 5], 1u << (bi & 31));
    if (tid == 0) { order[t] = bi; step_sims[t - 1] = bs; }
    last = bi;
  }
}

// ------------------------------------------------------------------------------------------------
// k_order_pairs (:1470-1476, :1508-1516): similarities of the N - 1 neighbour pairs (order[q], order[q + 1]), or
// (q, q + 1) when order is NULL.  16 lanes per pair, 16 pairs per workgroup, straight from Z and the raw rows:
// each lane multiplies its columns l, l + 16, ... in order, sum16 adds the lanes.  An index outside [0, N)
// gives NaN for its pairs and is never dereferenced.
// k_order_stats: one workgroup over the n = N - 1 pair similarities: per-thread strided sums in order, then a
// fixed LDS tree.  stats = average, population variance (two passes, as np.var), coherence avg (1 - min(var, 1)),
// efficiency max(0, 1 - mean(1 - s)); n = 0 writes 1, 0, 1, 1 (:1461-1467).
// ------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void k_order_pairs(const double* __restrict__ Z, const uint8_t* __restrict__ flags,
                                                     const double* __restrict__ X, int64_t ldx, int N, int L, int Lp,
                                                     const int64_t* __restrict__ order, double* __restrict__ pair_sims) {
  const int l = threadIdx.x & 15;
  const int q = blockIdx.x * 16 + (threadIdx.x >> 4);
  const bool live = q < N - 1;
  int64_t a = q, b = q + 1;
  if (live && order) { a = order[q]; b = order[q + 1]; }
  const bool ok = live && a >= 0 && a < N && b >= 0 && b < N;
  double dot = 0.0;
  int close = 1;
  bool constant = false;
  if (ok) {
    const double* za = Z + a * Lp;
    const double* zb = Z + b * Lp;
    for (int k = l; k < Lp; k += 16) dot = dot + za[k] * zb[k];
    constant = ((flags[a] | flags[b]) & kOrdConst) != 0;
    if (constant)
      for (int k = l; k < L; k += 16) close &= ord_close(X[a * ldx + k], X[b * ldx + k]) ? 1 : 0;
  }
  dot = sum16(dot);
  close = and16(close);
  if (live && l == 0) pair_sims[q] = !ok ? NAN : (constant ? (close ? 1.0 : 0.0) : ord_sim(dot));
}

__device__ __forceinline__ double ord_block_sum(double v, double* red) {
  const int tid = threadIdx.x;
  red[tid] = v;
  __syncthreads();
  for (int s = 128; s > 0; s >>= 1) {
    if (tid < s) red[tid] = red[tid] + red[tid + s];
    __syncthreads();
  }
  const double r = red[0];
  __syncthreads();
  return r;
}

__global__ __launch_bounds__(256) void k_order_stats(const double* __restrict__ pair_sims, int n,
                                                     double* __restrict__ stats) {
  __shared__ double red[256];
  const int tid = threadIdx.x;
  if (n <= 0) {
    if (tid == 0) { stats[0] = 1.0; stats[1] = 0.0; stats[2] = 1.0; stats[3] = 1.0; }
    return;
  }
  double a = 0.0, pen = 0.0;
  for (int q = tid; q < n; q += 256) { a = a + pair_sims[q]; pen = pen + (1.0 - pair_sims[q]); }
  const double avg = ord_block_sum(a, red) / (double)n;
  const double apen = ord_block_sum(pen, red) / (double)n;
  double v = 0.0;
  for (int q = tid; q < n; q += 256) { const double d = pair_sims[q] - avg; v = v + d * d; }
  const double var = ord_block_sum(v, red) / (double)n;
  if (tid == 0) {
    const double eff = 1.0 - apen;
    stats[0] = avg;
    stats[1] = var;
    stats[2] = avg * (1.0 - (var < 1.0 ? var : 1.0));
    stats[3] = eff > 0.0 ? eff : 0.0;
  }
}

// ------------------------------------------------------------------------------------------------
// k_order_insert (:1772-1803): one workgroup per query row s = S[q][0 .. N-1].  Position 0 scores s[0], position
// i = 1 .. N-1 scores (s[i-1] + s[i]) / 2, position N scores s[N-1]; visited in that order with strict > from
// -1.0, so the first maximum wins: per thread ascending positions, ord_wg_argmax keeps the lower one.
// ------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void k_order_insert(const double* __restrict__ S, int64_t ldS, int N,
                                                      int64_t* __restrict__ pos, double* __restrict__ score) {
  __shared__ OrdSlots sl;
  const double* s = S + (int64_t)blockIdx.x * ldS;
  double bs = -1.0;
  int bi = INT_MAX;
  for (int p = threadIdx.x; p <= N; p += 256) {
    const double v = p == 0 ? s[0] : (p == N ? s[N - 1] : (s[p - 1] + s[p]) / 2.0);
    if (v > bs) { bs = v; bi = p; }
  }
  ord_wg_argmax(bs, bi, sl, 0);
  if (threadIdx.x == 0) {
    pos[blockIdx.x] = bi == INT_MAX ? 0 : bi;
    score[blockIdx.x] = bs;
  }
}

static inline int64_t ord_pad_rows(int64_t N) { return (N + 15) & ~(int64_t)15; }
static inline int ord_pad_len(int L) { return (L + 3) & ~3; }

static int ord_check(int64_t N, int L, const char* what) {
  if (N < 0 || N > INT_MAX - 64) return fail(HQ_E_INVALID, "%s: bad row count %lld", what, (long long)N);
  if (L < 1 || L > kOrdMaxL)
    return fail(HQ_E_UNSUPPORTED, "%s: index rows of %d values (1 <= L <= %d)", what, L, kOrdMaxL);
  return HQ_OK;
}

}  // namespace hq

using namespace hq;

extern "C" {

int64_t hq_order_padded_rows(int64_t N) { return N <= 0 ? 0 : ord_pad_rows(N); }

int hq_order_padded_len(int L) { return L <= 0 ? 0 : ord_pad_len(L); }

int hq_order_prepare(const double* X, int64_t N, int64_t ldx, int L, double* Z, uint8_t* flags, hq_stream_t stream) {
  if (int rc = ord_check(N, L, "order prepare")) return rc;
  if (ldx < L) return fail(HQ_E_INVALID, "order prepare: row stride %lld < L = %d", (long long)ldx, L);
  if (N == 0) return HQ_OK;
  if (!X || !Z || !flags) return fail(HQ_E_INVALID, "null buffer");
  const int64_t Np = ord_pad_rows(N);
  hipLaunchKernelGGL(k_order_prepare, dim3((unsigned)(Np / 16)), dim3(256), 0, (hipStream_t)stream, X, (int)N, ldx, L,
                     ord_pad_len(L), Z, flags);
  HQ_CHECK_LAUNCH();
  return HQ_OK;
}

int hq_order_sims(const double* Za, const uint8_t* fa, const double* Xa, int64_t lda, int64_t M, const double* Zb,
                  const uint8_t* fb, const double* Xb, int64_t ldb, int64_t N, int L, double* S, int64_t ldS,
                  hq_stream_t stream) {
  if (int rc = ord_check(N, L, "order sims")) return rc;
  if (M < 0 || M > INT_MAX - 64) return fail(HQ_E_INVALID, "order sims: bad query count %lld", (long long)M);
  if (lda < L || ldb < L || ldS < N) return fail(HQ_E_INVALID, "order sims: row stride below the row length");
  if (M == 0 || N == 0) return HQ_OK;
  if (!Za || !fa || !Xa || !Zb || !fb || !Xb || !S) return fail(HQ_E_INVALID, "null buffer");
  const unsigned gy = (unsigned)((M + kOrdTile - 1) / kOrdTile);
  if (gy > 65535u) return fail(HQ_E_UNSUPPORTED, "order sims: %lld query rows (at most %d per call)", (long long)M,
                               65535 * kOrdTile);
  hipLaunchKernelGGL(k_order_sims, dim3((unsigned)((N + kOrdTile - 1) / kOrdTile), gy), dim3(256), 0,
                     (hipStream_t)stream, Za, fa, Xa, lda, (int)M, (int)ord_pad_rows(M), Zb, fb, Xb, ldb, (int)N,
                     (int)ord_pad_rows(N), L, ord_pad_len(L), S, ldS);
  HQ_CHECK_LAUNCH();
  return HQ_OK;
}

int hq_order_start(const double* X, int64_t ldx, int64_t N, int L, int64_t* start, hq_stream_t stream) {
  if (int rc = ord_check(N, L, "order start")) return rc;
  if (ldx < L) return fail(HQ_E_INVALID, "order start: row stride %lld < L = %d", (long long)ldx, L);
  if (N == 0) return HQ_OK;
  if (!X || !start) return fail(HQ_E_INVALID, "null buffer");
  hipLaunchKernelGGL(k_order_start, dim3(1), dim3(kOrdWalkT), 0, (hipStream_t)stream, X, ldx, (int)N, L, start);
  HQ_CHECK_LAUNCH();
  return HQ_OK;
}

size_t hq_order_greedy_workspace_size(int64_t N) {
  if (N <= 0 || N > kOrdMaxN) return 0;
  const size_t Np = (size_t)ord_pad_rows(N);
  return 8 * Np * Np + 16;  // S [Np, Np], then the start row
}

int hq_order_greedy(const double* Z, const uint8_t* flags, const double* X, int64_t ldx, int64_t N, int L,
                    void* workspace, size_t workspace_bytes, int64_t* order, double* step_sims, hq_stream_t stream) {
  if (int rc = ord_check(N, L, "order greedy")) return rc;
  if (N > kOrdMaxN)
    return fail(HQ_E_UNSUPPORTED, "order greedy: %lld frames (at most %d: the similarity matrix takes 8 N^2 bytes)",
                (long long)N, kOrdMaxN);
  if (ldx < L) return fail(HQ_E_INVALID, "order greedy: row stride %lld < L = %d", (long long)ldx, L);
  if (N == 0) return HQ_OK;
  if (!Z || !flags || !X || !workspace || !order || (N > 1 && !step_sims)) return fail(HQ_E_INVALID, "null buffer");
  if (workspace_bytes < hq_order_greedy_workspace_size(N) || (reinterpret_cast<uintptr_t>(workspace) & 15))
    return fail(HQ_E_INVALID, "order greedy: workspace of %zu bytes (needs %zu, 16-byte aligned)", workspace_bytes,
                hq_order_greedy_workspace_size(N));
  const int64_t Np = ord_pad_rows(N);
  double* S = static_cast<double*>(workspace);
  int64_t* start = reinterpret_cast<int64_t*>(S + Np * Np);
  if (int rc = hq_order_sims(Z, flags, X, ldx, N, Z, flags, X, ldx, N, L, S, Np, stream)) return rc;
  if (int rc = hq_order_start(X, ldx, N, L, start, stream)) return rc;
  hipLaunchKernelGGL(k_order_walk, dim3(1), dim3(kOrdWalkT), 0, (hipStream_t)stream, S, Np, (int)N, start, order,
                     step_sims);
  HQ_CHECK_LAUNCH();
  return HQ_OK;
}

int hq_order_pairs(const double* Z, const uint8_t* flags, const double* X, int64_t ldx, int64_t N, int L,
                   const int64_t* order, double* pair_sims, double* stats, hq_stream_t stream) {
  if (int rc = ord_check(N, L, "order pairs")) return rc;
  if (ldx < L) return fail(HQ_E_INVALID, "order pairs: row stride %lld < L = %d", (long long)ldx, L);
  if (N == 0) return HQ_OK;
  if (!stats || (N > 1 && (!Z || !flags || !X || !pair_sims))) return fail(HQ_E_INVALID, "null buffer");
  if (N > 1) {
    hipLaunchKernelGGL(k_order_pairs, dim3((unsigned)((N - 1 + 15) / 16)), dim3(256), 0, (hipStream_t)stream, Z, flags,
                       X, ldx, (int)N, L, ord_pad_len(L), order, pair_sims);
    HQ_CHECK_LAUNCH();
  }
  hipLaunchKernelGGL(k_order_stats, dim3(1), dim3(256), 0, (hipStream_t)stream, pair_sims, (int)(N - 1), stats);
  HQ_CHECK_LAUNCH();
  return HQ_OK;
}

int hq_order_insert(const double* S, int64_t ldS, int Q, int64_t N, int64_t* pos, double* score, hq_stream_t stream) {
  if (Q < 0 || N < 0 || N > INT_MAX - 64) return fail(HQ_E_INVALID, "order insert: bad shape");
  if (Q == 0 || N == 0) return HQ_OK;
  if (ldS < N) return fail(HQ_E_INVALID, "order insert: row stride %lld < N", (long long)ldS);
  if (!S || !pos || !score) return fail(HQ_E_INVALID, "null buffer");
  hipLaunchKernelGGL(k_order_insert, dim3((unsigned)Q), dim3(256), 0, (hipStream_t)stream, S, ldS, (int)N, pos, score);
  HQ_CHECK_LAUNCH();
  return HQ_OK;
}

}  // extern "C"
