// hq_vfeat.hip — per-frame video features and their weighted clamped-cosine scorer (gfx950).
//
// The reference's `video_features` and `hybrid` searches (core/video_search.py: _extract_comprehensive_features
// :1347, _extract_texture_features :1390, _calculate_feature_similarity :1499, _hybrid_search_optimized :1576)
// describe every gray u8 frame g [H, W] (n = H W) by
//   histogram [32]  counts of g >> 3 (cv2.calcHist, 32 bins over [0, 256))
//   texture   [16]  gx, gy = the 3 x 3 Sobel derivatives with mirrored borders (p[-1] = p[1]), m = sqrt(gx^2 + gy^2):
//                   mean m, std m, mean gx, std gx, mean gy, std gy, mean |gx|, mean |gy|, then np.histogram(m, 8)
//   stats     [7]   mean, std, min, max, median, 25th and 75th percentile of g (linear interpolation)
// and score a pair by sum over the parts of w_part max(0, a.b / (|a| |b|)), weights 0.3, 0.2, 0.1.  The ORB part
// (weight 0.4) is not computed.
//
//   hq_vfeat_extract        frames u8 [N, H, W] -> rows f64 [N, 64]
//   hq_vfeat_scores         rows x rows -> [Q, N]
//   hq_vfeat_scores_listed  the same pairs through an id list -> [Q, C], bit for bit the dense entries, and the
//                           hybrid search's blend with a hierarchical score
//
// Row layout (512 bytes): [0, 32) histogram, [32, 48) texture, [48, 55) stats, [55] 0 (pads the stats part to 8),
// [56, 59) the Euclidean norms of the three parts, [59, 64) 0.
//
// Extraction: one wave per frame, four frames per 256-thread workgroup, no block barrier.  The frame is copied once
// into LDS as u8 (16-byte loads over its aligned body); pass A builds a 256-bin LDS histogram from which the 32 bins,
// both integer moments, min, max and the order statistics follow (64-lane prefix scan over the bins); pass B runs the
// Sobel stencil out of LDS with integer accumulators and sums sqrt(gx^2 + gy^2) in float64; pass C repeats the
// stencil for the 8-bin magnitude histogram and the two-pass std of m.  Every integer quantity is exact, variances
// are (n sum x^2 - (sum x)^2) / n^2 from int64.
//
// Scoring: a workgroup owns 64 corpus rows in LDS and walks the queries in tiles of 64; a lane keeps a 4 x 4
// register tile (register-tiled VALU form: on gfx950 the f64 MFMA peak equals the f64 VALU peak, and with K = 32, 16
// and 8 per part the kernel is bound by its Q x N store and its three divisions per pair, not by the contraction).
// Each part's dot product is one fma chain over k ascending from 0.0 in both kernels, and both call vfeat_total.
#include "hq_common.h"

#include <math.h>

namespace hq {

constexpr int kVfNt = 256;               // threads per workgroup: four waves, one frame each
constexpr int kVfMinSide = 4;
constexpr int kVfMaxPx = 131 * 128;      // 16768 pixels: per-lane 32-bit sums hold, four frames fit 72 KiB of LDS
constexpr int kVfRow = 64;               // doubles per row
constexpr int kVfK = 56;                 // contracted slots: 32 + 16 + 8
constexpr int kVfNormSlot = 56;
constexpr int kVfWaveFixed = 256 * 4 + kVfRow * 8;  // per wave: 256-bin histogram + one output row

__device__ __forceinline__ void vf_wave_sync() {
  __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
  __builtin_amdgcn_wave_barrier();
  __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
}

__device__ __forceinline__ int vf_wsum(int v) {
  for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o);
  return v;
}
__device__ __forceinline__ long long vf_wsum(long long v) {
  for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o);
  return v;
}
__device__ __forceinline__ double vf_wsum(double v) {
  for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o);
  return v;
}
__device__ __forceinline__ int vf_wmax(int v) {
  for (int o = 32; o > 0; o >>= 1) v = max(v, __shfl_xor(v, o));
  return v;
}
__device__ __forceinline__ int vf_wmin(int v) {
  for (int o = 32; o > 0; o >>= 1) v = min(v, __shfl_xor(v, o));
  return v;
}

static __host__ __device__ inline size_t vfeat_px_bytes(int n) { return ((size_t)n + 15 + 15) & ~(size_t)15; }
static inline size_t vfeat_lds_bytes(int n) { return 4 * (kVfWaveFixed + vfeat_px_bytes(n)); }

// Sobel derivatives at (r, c) of the H x W frame P, borders mirrored without the edge pixel
__device__ __forceinline__ void vf_sobel(const uint8_t* P, int H, int W, int r, int c, int& gx, int& gy) {
  const uint8_t* a = P + (r == 0 ? 1 : r - 1) * W;
  const uint8_t* b = P + r * W;
  const uint8_t* d = P + (r == H - 1 ? H - 2 : r + 1) * W;
  const int cm = c == 0 ? 1 : c - 1, cp = c == W - 1 ? W - 2 : c + 1;
  const int am = a[cm], ac = a[c], ap = a[cp], bm = b[cm], bp = b[cp], dm = d[cm], dc = d[c], dp = d[cp];
  gx = (ap + 2 * bp + dp) - (am + 2 * bm + dm);
  gy = (dm + 2 * dc + dp) - (am + 2 * ac + ap);
}

// the value of 0-based rank k in the sorted frame: the lane whose four bins [exc, exc + c0 + .. + c3) hold k knows it
__device__ __forceinline__ int vf_rank(int k, int lane, int exc, const int (&c)[4]) {
  int v = -1, cum = exc;
#pragma unroll
  for (int j = 0; j < 4; ++j) {
    if (v < 0 && k >= cum && k < cum + c[j]) v = 4 * lane + j;
    cum += c[j];
  }
  return vf_wmax(v);
}

// np.percentile's linear rule at virtual index q (n - 1) / 4 (q = 1, 2, 3: exact in float64)
__device__ __forceinline__ double vf_quartile(int q, int n, int lane, int exc, const int (&c)[4]) {
  const int num = q * (n - 1), lo = num >> 2, hi = min(lo + 1, n - 1);
  const int a = vf_rank(lo, lane, exc, c), b = vf_rank(hi, lane, exc, c);
  return (double)a + (double)(b - a) * ((double)(num & 3) * 0.25);
}

__global__ __launch_bounds__(kVfNt) void k_vfeat_extract(const uint8_t* frames, int64_t N, int H, int W,
                                                         double* rows) {
  extern __shared__ __attribute__((aligned(16))) unsigned char vf_smem[];
  const int n = H * W;
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  unsigned char* base = vf_smem + (size_t)wave * (kVfWaveFixed + vfeat_px_bytes(n));
  int* hist = reinterpret_cast<int*>(base);
  double* row = reinterpret_cast<double*>(base + 1024);
  uint8_t* px = base + kVfWaveFixed;
  const double dn = (double)n;
  for (int64_t idx = (int64_t)blockIdx.x * 4 + wave; idx < N; idx += (int64_t)gridDim.x * 4) {
    // ---- stage: pixel p lives at px[m + p], m = the frame's misalignment, so the 16-byte body is aligned on both sides
    const uint8_t* f = frames + idx * n;
    const int m = (int)((uintptr_t)f & 15);
    const int head = (16 - m) & 15;  // < 16 <= n
    if (lane < head) px[m + lane] = f[lane];
    const int nv = (n - head) >> 4;
    const uint4* src = reinterpret_cast<const uint4*>(f + head);
    uint4* dst = reinterpret_cast<uint4*>(px + m + head);
    for (int i = lane; i < nv; i += 64) dst[i] = src[i];
    const int t0 = head + (nv << 4);
    if (t0 + lane < n) px[m + t0 + lane] = f[t0 + lane];  // fewer than 16 bytes
    for (int i = lane; i < 256; i += 64) hist[i] = 0;
    vf_wave_sync();
    // ---- pass A: 256-bin histogram, four pixels per LDS read
    const uint32_t* pw = reinterpret_cast<const uint32_t*>(px);
    const int nd = (m + n + 3) >> 2;
    for (int d = lane; d < nd; d += 64) {
      const uint32_t w = pw[d];
#pragma unroll
      for (int b = 0; b < 4; ++b) {
        const int e = 4 * d + b - m;
        if (e >= 0 && e < n) atomicAdd(&hist[(w >> (8 * b)) & 255u], 1);
      }
    }
    vf_wave_sync();
    int c[4];
    int t = 0, vmin = 256, vmax = -1;
    long long sv = 0, svv = 0;
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      const int v = 4 * lane + j;
      c[j] = hist[v];
      t += c[j];
      sv += (long long)v * c[j];
      svv += (long long)(v * v) * c[j];
      if (c[j] > 0) {
        vmin = min(vmin, v);
        vmax = v;
      }
    }
    int inc = t;
    for (int o = 1; o < 64; o <<= 1) {
      const int u = __shfl_up(inc, o);
      if (lane >= o) inc += u;
    }
    const int exc = inc - t;
    sv = vf_wsum(sv);
    svv = vf_wsum(svv);
    vmin = vf_wmin(vmin);
    vmax = vf_wmax(vmax);
    const double p25 = vf_quartile(1, n, lane, exc, c);
    const double med = vf_quartile(2, n, lane, exc, c);
    const double p75 = vf_quartile(3, n, lane, exc, c);
    const int h32 = t + __shfl_xor(t, 1);  // bins 8 (lane / 2) .. + 7
    if ((lane & 1) == 0) row[lane >> 1] = (double)h32;
    const long long sh2 = vf_wsum((lane & 1) == 0 ? (long long)h32 * h32 : 0ll);
    // ---- pass B: Sobel, integer sums, sum of magnitudes
    const uint8_t* P = px + m;
    const int dr = 64 / W, dc = 64 % W;
    int sgx = 0, sgy = 0, smin = 0x7fffffff, smax = 0;
    unsigned sgx2 = 0, sgy2 = 0, sax = 0, say = 0;
    double sm = 0.0;
    {
      int r = lane / W, cc = lane - r * W;
      for (int p = lane; p < n; p += 64) {
        int gx, gy;
        vf_sobel(P, H, W, r, cc, gx, gy);
        const int s = gx * gx + gy * gy;
        sgx += gx;
        sgy += gy;
        sgx2 += (unsigned)(gx * gx);
        sgy2 += (unsigned)(gy * gy);
        sax += (unsigned)abs(gx);
        say += (unsigned)abs(gy);
        smin = min(smin, s);
        smax = max(smax, s);
        sm += sqrt((double)s);
        cc += dc;
        r += dr;
        if (cc >= W) {
          cc -= W;
          ++r;
        }
      }
    }
    const long long SGX = vf_wsum((long long)sgx), SGY = vf_wsum((long long)sgy);
    const long long SGX2 = vf_wsum((long long)sgx2), SGY2 = vf_wsum((long long)sgy2);
    const long long SAX = vf_wsum((long long)sax), SAY = vf_wsum((long long)say);
    smin = vf_wmin(smin);
    smax = vf_wmax(smax);
    const double mean_m = vf_wsum(sm) / dn;
    // ---- pass C: the 8 bins of np.histogram(m, bins=8) and sum (m - mean)^2
    double lo = sqrt((double)smin), hi = sqrt((double)smax);
    if (lo == hi) {
      lo -= 0.5;
      hi += 0.5;
    }
    const double step = (hi - lo) / 8.0;
    double edge[7];
#pragma unroll
    for (int j = 0; j < 7; ++j) edge[j] = (double)(j + 1) * step + lo;
    int ge[7] = {0, 0, 0, 0, 0, 0, 0};  // pixels with m >= edge j
    double sq = 0.0;
    {
      int r = lane / W, cc = lane - r * W;
      for (int p = lane; p < n; p += 64) {
        int gx, gy;
        vf_sobel(P, H, W, r, cc, gx, gy);
        const double x = sqrt((double)(gx * gx + gy * gy));
        const double dv = x - mean_m;
        sq += dv * dv;
#pragma unroll
        for (int j = 0; j < 7; ++j) ge[j] += x >= edge[j] ? 1 : 0;
        cc += dc;
        r += dr;
        if (cc >= W) {
          cc -= W;
          ++r;
        }
      }
    }
#pragma unroll
    for (int j = 0; j < 7; ++j) ge[j] = vf_wsum(ge[j]);
    sq = vf_wsum(sq);
    if (lane == 0) {
      const long long ln = n;
      const double n2 = dn * dn;
      double tx[16];
      tx[0] = mean_m;
      tx[1] = sqrt(sq / dn);
      tx[2] = (double)SGX / dn;
      tx[3] = sqrt((double)(ln * SGX2 - SGX * SGX) / n2);
      tx[4] = (double)SGY / dn;
      tx[5] = sqrt((double)(ln * SGY2 - SGY * SGY) / n2);
      tx[6] = (double)SAX / dn;
      tx[7] = (double)SAY / dn;
      tx[8] = (double)(n - ge[0]);
#pragma unroll
      for (int j = 1; j < 7; ++j) tx[8 + j] = (double)(ge[j - 1] - ge[j]);
      tx[15] = (double)ge[6];
      double st[8];
      st[0] = (double)sv / dn;
      st[1] = sqrt((double)(ln * svv - sv * sv) / n2);
      st[2] = (double)vmin;
      st[3] = (double)vmax;
      st[4] = med;
      st[5] = p25;
      st[6] = p75;
      st[7] = 0.0;
      double nt = 0.0, ns = 0.0;
#pragma unroll
      for (int j = 0; j < 16; ++j) {
        row[32 + j] = tx[j];
        nt += tx[j] * tx[j];
      }
#pragma unroll
      for (int j = 0; j < 8; ++j) {
        row[48 + j] = st[j];
        ns += st[j] * st[j];
      }
      row[kVfNormSlot + 0] = sqrt((double)sh2);
      row[kVfNormSlot + 1] = sqrt(nt);
      row[kVfNormSlot + 2] = sqrt(ns);
#pragma unroll
      for (int j = kVfNormSlot + 3; j < kVfRow; ++j) row[j] = 0.0;
    }
    vf_wave_sync();
    rows[idx * kVfRow + lane] = row[lane];
    vf_wave_sync();  // the row and the pixels are rewritten by the next frame
  }
}

// ---------------------------------------------------------------------------------------------- scoring
struct VfWeights {
  double w[3];
};

// one pair from its three dot products and part norms
__device__ __forceinline__ double vfeat_total(const double (&d)[3], const double (&na)[3], const double (&nb)[3],
                                              const VfWeights& w) {
  double tot = 0.0;
#pragma unroll
  for (int p = 0; p < 3; ++p) {
    const double c = (na[p] > 0.0 && nb[p] > 0.0) ? fmax(0.0, d[p] / (na[p] * nb[p])) : 0.0;
    tot = p == 0 ? w.w[0] * c : tot + w.w[p] * c;
  }
  return tot;
}

constexpr int kVsT = 64;      // rows per tile on both sides
constexpr int kVsPitch = 66;  // doubles between the k-planes of a staged tile: 16-byte aligned, spreads the banks
constexpr size_t kVsLds = (size_t)2 * (kVfK * kVsPitch + 3 * kVsT) * sizeof(double);  // 62,208 bytes

// rows r0 .. r0 + 63 of `rows` (zeros past R), transposed: tile[k][row], nrm[part][row]
__device__ __forceinline__ void vs_stage(const double* rows, int64_t r0, int64_t R, double* tile, double* nrm) {
  for (int e = threadIdx.x; e < kVsT * kVfK; e += kVfNt) {
    const int r = e / kVfK, k = e - r * kVfK;
    tile[k * kVsPitch + r] = r0 + r < R ? rows[(r0 + r) * kVfRow + k] : 0.0;
  }
  if (threadIdx.x < 3 * kVsT) {
    const int r = threadIdx.x / 3, p = threadIdx.x - 3 * r;
    nrm[p * kVsT + r] = r0 + r < R ? rows[(r0 + r) * kVfRow + kVfNormSlot + p] : 0.0;
  }
}

// grid: corpus tiles of 64 rows.  Thread (ty, tx) = (tid / 16, tid % 16) owns queries 4 ty .. + 3 x frames 4 tx .. + 3.
__global__ __launch_bounds__(kVfNt) void k_vfeat_scores(const double* qrows, int Q, const double* crows, int64_t N,
                                                        VfWeights w, double* out) {
  extern __shared__ __attribute__((aligned(16))) unsigned char vf_smem[];
  double* ct = reinterpret_cast<double*>(vf_smem);
  double* qt = ct + kVfK * kVsPitch;
  double* cn = qt + kVfK * kVsPitch;
  double* qn = cn + 3 * kVsT;
  const int tx = threadIdx.x & 15, ty = threadIdx.x >> 4;
  for (int64_t c0 = (int64_t)blockIdx.x * kVsT; c0 < N; c0 += (int64_t)gridDim.x * kVsT) {
    vs_stage(crows, c0, N, ct, cn);
    for (int q0 = 0; q0 < Q; q0 += kVsT) {
      vs_stage(qrows, q0, Q, qt, qn);
      __syncthreads();
      double d[3][4][4];
#pragma unroll
      for (int p = 0; p < 3; ++p) {
        const int k0 = p == 0 ? 0 : (p == 1 ? 32 : 48), k1 = p == 0 ? 32 : (p == 1 ? 48 : 56);
#pragma unroll
        for (int i = 0; i < 4; ++i)
#pragma unroll
          for (int j = 0; j < 4; ++j) d[p][i][j] = 0.0;
#pragma unroll 4
        for (int k = k0; k < k1; ++k) {
          const double2 qa = *reinterpret_cast<const double2*>(qt + k * kVsPitch + 4 * ty);
          const double2 qb = *reinterpret_cast<const double2*>(qt + k * kVsPitch + 4 * ty + 2);
          const double2 ca = *reinterpret_cast<const double2*>(ct + k * kVsPitch + 4 * tx);
          const double2 cb = *reinterpret_cast<const double2*>(ct + k * kVsPitch + 4 * tx + 2);
          const double qv[4] = {qa.x, qa.y, qb.x, qb.y}, cv[4] = {ca.x, ca.y, cb.x, cb.y};
#pragma unroll
          for (int i = 0; i < 4; ++i)
#pragma unroll
            for (int j = 0; j < 4; ++j) d[p][i][j] = fma(qv[i], cv[j], d[p][i][j]);
        }
      }
#pragma unroll
      for (int i = 0; i < 4; ++i) {
        const int a = 4 * ty + i;
        if (q0 + a >= Q) continue;
        const double na[3] = {qn[a], qn[kVsT + a], qn[2 * kVsT + a]};
#pragma unroll
        for (int j = 0; j < 4; ++j) {
          const int b = 4 * tx + j;
          if (c0 + b >= N) continue;
          const double nb[3] = {cn[b], cn[kVsT + b], cn[2 * kVsT + b]};
          const double dd[3] = {d[0][i][j], d[1][i][j], d[2][i][j]};
          out[(int64_t)(q0 + a) * N + c0 + b] = vfeat_total(dd, na, nb, w);
        }
      }
      __syncthreads();  // the query tile is restaged
    }
  }
}

// grid (chunks of 64 list entries, queries); one wave per (query, chunk), a lane per entry
__global__ __launch_bounds__(64) void k_vfeat_scores_listed(const double* qrows, int Q, const double* crows, int64_t N,
                                                            VfWeights w, const int64_t* ids, int C,
                                                            const double* hier, double* video, double* combined) {
  __shared__ double qrow[kVfRow];
  const int lane = threadIdx.x;
  const int j = blockIdx.x * 64 + lane;
  for (int a = blockIdx.y; a < Q; a += gridDim.y) {
    qrow[lane] = qrows[(int64_t)a * kVfRow + lane];
    __syncthreads();
    if (j < C) {
      const int64_t o = (int64_t)a * C + j;
      const int64_t id = ids[o];
      double v = -INFINITY, cmb = -INFINITY;
      if (id >= 0 && id < N) {
        const double* cr = crows + id * kVfRow;
        double d[3];
#pragma unroll
        for (int p = 0; p < 3; ++p) {
          const int k0 = p == 0 ? 0 : (p == 1 ? 32 : 48), k1 = p == 0 ? 32 : (p == 1 ? 48 : 56);
          double acc = 0.0;
          for (int k = k0; k < k1; ++k) acc = fma(qrow[k], cr[k], acc);
          d[p] = acc;
        }
        const double na[3] = {qrow[kVfNormSlot], qrow[kVfNormSlot + 1], qrow[kVfNormSlot + 2]};
        const double nb[3] = {cr[kVfNormSlot], cr[kVfNormSlot + 1], cr[kVfNormSlot + 2]};
        v = vfeat_total(d, na, nb, w);
        if (combined) {
          const double h = hier[o];
          cmb = v > 0.5 ? 0.3 * h + 0.7 * v : 0.8 * h + 0.2 * v;
        }
      }
      video[o] = v;
      if (combined) combined[o] = cmb;
    }
    __syncthreads();  // qrow is rewritten by the next query
  }
}

// ---------------------------------------------------------------------------------------------- host side
static bool vf_aligned8(const void* p) { return ((uintptr_t)p & 7) == 0; }

static int vf_weights(const double* w, VfWeights& out) {
  if (!w) return fail(HQ_E_INVALID, "null buffer");
  for (int p = 0; p < 3; ++p) {
    if (!(w[p] >= 0.0) || isinf(w[p])) return fail(HQ_E_INVALID, "weights must be finite and >= 0");
    out.w[p] = w[p];
  }
  return HQ_OK;
}

}  // namespace hq

using namespace hq;

extern "C" {

int hq_vfeat_extract(const uint8_t* frames, int64_t N, int H, int W, double* rows, hq_stream_t stream) {
  if (N < 0 || H <= 0 || W <= 0) return fail(HQ_E_INVALID, "bad shape");
  if (H < kVfMinSide || W < kVfMinSide || (int64_t)H * W > kVfMaxPx)
    return fail(HQ_E_UNSUPPORTED, "video-feature frames have sides >= %d and at most %d pixels, got %d x %d",
                kVfMinSide, kVfMaxPx, H, W);
  if (N == 0) return HQ_OK;
  if (!frames || !rows) return fail(HQ_E_INVALID, "null buffer");
  if (!vf_aligned8(rows)) return fail(HQ_E_INVALID, "rows must be 8-byte aligned");
  const size_t lds = vfeat_lds_bytes(H * W);
  if (lds > 64 * 1024)
    HQ_CHECK_HIP(hipFuncSetAttribute((const void*)k_vfeat_extract, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
  const int64_t groups = (N + 3) / 4;
  hipLaunchKernelGGL(k_vfeat_extract, dim3((unsigned)(groups < 65536 ? groups : 65536)), dim3(kVfNt), lds,
                     (hipStream_t)stream, frames, N, H, W, rows);
  HQ_CHECK_LAUNCH();
  return HQ_OK;
}

int hq_vfeat_scores(const double* qrows, int Q, const double* crows, int64_t N, const double* w, double* out,
                    hq_stream_t stream) {
  if (Q < 0 || N < 0) return fail(HQ_E_INVALID, "bad shape");
  VfWeights vw;
  if (int rc = vf_weights(w, vw)) return rc;
  if (Q == 0 || N == 0) return HQ_OK;
  if (!qrows || !crows || !out) return fail(HQ_E_INVALID, "null buffer");
  if (!vf_aligned8(qrows) || !vf_aligned8(crows) || !vf_aligned8(out))
    return fail(HQ_E_INVALID, "rows and outputs must be 8-byte aligned");
  const int64_t tiles = (N + kVsT - 1) / kVsT;
  hipLaunchKernelGGL(k_vfeat_scores, dim3((unsigned)(tiles < (1 << 20) ? tiles : (1 << 20))), dim3(kVfNt), kVsLds,
                     (hipStream_t)stream, qrows, Q, crows, N, vw, out);
  HQ_CHECK_LAUNCH();
  return HQ_OK;
}

int hq_vfeat_scores_listed(const double* qrows, int Q, const double* crows, int64_t N, const double* w,
                           const int64_t* ids, int C, const double* hier, double* video, double* combined,
                           hq_stream_t stream) {
  if (Q < 0 || N < 0) return fail(HQ_E_INVALID, "bad shape");
  if (C < 1 || C > 65535) return fail(HQ_E_INVALID, "a list holds 1 .. 65535 entries, got C = %d", C);
  VfWeights vw;
  if (int rc = vf_weights(w, vw)) return rc;
  if ((hier == nullptr) != (combined == nullptr))
    return fail(HQ_E_INVALID, "hier and combined are given together or not at all");
  if (Q == 0) return HQ_OK;
  // (N = 0: every entry is a pad, crows is never read)
  if (!qrows || !ids || !video || (N > 0 && !crows)) return fail(HQ_E_INVALID, "null buffer");
  if (!vf_aligned8(qrows) || !vf_aligned8(crows) || !vf_aligned8(ids) || !vf_aligned8(hier) || !vf_aligned8(video) ||
      !vf_aligned8(combined))
    return fail(HQ_E_INVALID, "rows, ids and outputs must be 8-byte aligned");
  hipLaunchKernelGGL(k_vfeat_scores_listed, dim3((unsigned)((C + 63) / 64), (unsigned)(Q < 65535 ? Q : 65535)),
                     dim3(64), 0, (hipStream_t)stream, qrows, Q, crows, N, vw, ids, C, hier, video, combined);
  HQ_CHECK_LAUNCH();
  return HQ_OK;
}

}  // extern "C"
