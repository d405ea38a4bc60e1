// hq_ssim.hip — Gaussian-window SSIM and template correlation of u8 frame pairs (gfx950).
//
// The reference's image similarity (core/cv_features.py:386-457 calculate_ssim, :657-704 _calculate_ssim_manual):
// each frame min-max normalised in float64, x' = (x - min) / (max - min + 1e-8); F = the separable 7 x 7 Gaussian
// (sigma 1.5) correlation with mirrored borders (BORDER_REFLECT_101); mu = F(x'), var = F(x'^2) - mu^2,
// cov = F(x'y') - mu1 mu2; the score is the mean over all pixels of
//   (2 mu1 mu2 + C1)(2 cov + C2) / ((mu1^2 + mu2^2 + C1)(var1 + var2 + C2) + 1e-8),  C1 = 1e-4, C2 = 9e-4.
// The second output is the Pearson correlation of the raw pixels (cv2.matchTemplate TM_CCOEFF_NORMED of two frames of
// one size), from exact integer sums; 0.0 when a frame is constant.
//
//   hq_ssim_prepare        frames -> maps (mu, var of the normalised frame, float64) and stats (min, max, sum, sum sq)
//   hq_ssim_scores         prepared queries x raw corpus frames -> [Q, N]
//   hq_ssim_scores_listed  the same pairs through an id list -> [Q, C], bit for bit the dense entries
//
// Arithmetic.  Pixels are centred on the frame minimum as integers (xi = x - min, 0 .. 255), so a constant frame is
// all zeros and every filter of it is exactly 0, as in the model.  F is linear and the division by the range is a
// per-frame constant, so the filters run on the integers xi, xi^2 and xi yi (exact, at most 65,025) in float64 and
// the ranges are applied afterwards: mu = F(xi) / r, var = (F(xi^2) - F(xi)^2) / r^2, cov = F(xi yi) / (rx ry) -
// mu1 mu2.  Everything after the integer product is float64: the float32 form loses var to cancellation on nearly
// flat frames.  Only F(xi yi) is per-pair filter work.
//
// Work split.  A 256-thread workgroup owns one corpus frame and a tile of queries.  The frame is walked in strips
// of S = min(H, 4352 / W) rows (17 pixels per thread): the strip with a 3-pixel halo, mirrored at load time, is
// staged as u8 in LDS, the strip's mu2 / var2 are filtered once and stay in registers, then each query of the tile
// is staged (the next one while the current one's vertical pass runs, two LDS buffers), multiplied, filtered
// (horizontal pass into an LDS tile of doubles, vertical pass out of it) and evaluated against its prepared maps
// read from L2.  Strip sums are reduced per wave and added per (query, wave) in LDS in strip order; the four
// wave sums are combined in one fixed order at the end, so a pair's value does not depend on where it is computed.
#include "hq_common.h"

#include <math.h>

namespace hq {

constexpr int kSsimNt = 256;                      // threads per workgroup
constexpr int kSsimPpt = 17;                      // pixels per thread and strip (65 x 64 frames are one strip)
constexpr int kSsimStripPx = kSsimNt * kSsimPpt;  // 4352
constexpr int kSsimMinSide = 4;                   // one reflection reaches every halo pixel
constexpr int kSsimMaxH = 131, kSsimMaxW = 128;
constexpr int kSsimQt = 32;                       // most queries one workgroup walks per corpus frame
constexpr size_t kSsimLdsMax = 64 * 1024;

struct SsimTaps {
  double g[7];
};

struct SsimGeom {
  int H, W, S, pitch;  // S rows per strip, pitch = W + 6 (u8 tile row)
  float rcpW, rcpP;
};

// floor(e / d) for 0 <= e < 2^16 through the float reciprocal, corrected by one either way
__device__ __forceinline__ int ssim_div(int e, int d, float rcp) {
  int q = (int)((float)e * rcp);
  q -= (q * d > e) ? 1 : 0;
  q += ((q + 1) * d <= e) ? 1 : 0;
  return q;
}

__device__ __forceinline__ int ssim_mirror(int i, int n) { return i < 0 ? -i : (i >= n ? 2 * n - 2 - i : i); }

struct SsimStats {
  int mn, mx;
  long long s, ss;
};

// min, max, sum and sum of squares of one frame (n <= 16768 pixels: both sums fit 32 bits), on every thread
__device__ SsimStats ssim_frame_stats(const uint8_t* f, int n, int* red) {
  int mn = 255, mx = 0;
  unsigned s = 0, ss = 0;
  for (int i = threadIdx.x; i < n; i += kSsimNt) {
    const int v = f[i];
    mn = min(mn, v);
    mx = max(mx, v);
    s += (unsigned)v;
    ss += (unsigned)(v * v);
  }
  for (int o = 32; o > 0; o >>= 1) {
    mn = min(mn, __shfl_xor(mn, o));
    mx = max(mx, __shfl_xor(mx, o));
    s += (unsigned)__shfl_xor((int)s, o);
    ss += (unsigned)__shfl_xor((int)ss, o);
  }
  const int wave = threadIdx.x >> 6;
  if ((threadIdx.x & 63) == 0) {
    red[wave * 4 + 0] = mn;
    red[wave * 4 + 1] = mx;
    red[wave * 4 + 2] = (int)s;
    red[wave * 4 + 3] = (int)ss;
  }
  __syncthreads();
  SsimStats r;
  r.mn = min(min(red[0], red[4]), min(red[8], red[12]));
  r.mx = max(max(red[1], red[5]), max(red[9], red[13]));
  r.s = (long long)(unsigned)red[2] + (unsigned)red[6] + (unsigned)red[10] + (unsigned)red[14];
  r.ss = (long long)(unsigned)red[3] + (unsigned)red[7] + (unsigned)red[11] + (unsigned)red[15];
  __syncthreads();
  return r;
}

// rows r0 - 3 .. r0 + Sr + 2, columns -3 .. W + 2 of frame f, mirrored into the frame, minus mn -> tile
__device__ __forceinline__ void ssim_stage(const SsimGeom& g, const uint8_t* f, int r0, int Sr, int mn, uint8_t* tile) {
  const int n = (Sr + 6) * g.pitch;
  for (int e = threadIdx.x; e < n; e += kSsimNt) {
    const int rr = ssim_div(e, g.pitch, g.rcpP);
    const int r = ssim_mirror(r0 + rr - 3, g.H);
    const int c = ssim_mirror(e - rr * g.pitch - 3, g.W);
    tile[e] = (uint8_t)((int)f[r * g.W + c] - mn);
  }
}

// horizontal pass: hp[rr, c] = sum_k g[k] prod(tile offset of (rr, c + k)) over the strip's Sr + 6 rows; returns this
// thread's sum of the products of the strip's own pixels (halo rows left out)
template <class P>
__device__ __forceinline__ int ssim_hpass(const SsimGeom& g, int Sr, const SsimTaps& w, double* hp, P prod) {
  const int nh = (Sr + 6) * g.W;
  int own = 0;
  for (int e = threadIdx.x; e < nh; e += kSsimNt) {
    const int rr = ssim_div(e, g.W, g.rcpW);
    const int o = e + 6 * rr;  // rr * pitch + c
    const int p3 = prod(o + 3);
    double a = w.g[0] * (double)prod(o);
    a = fma(w.g[1], (double)prod(o + 1), a);
    a = fma(w.g[2], (double)prod(o + 2), a);
    a = fma(w.g[3], (double)p3, a);
    a = fma(w.g[4], (double)prod(o + 4), a);
    a = fma(w.g[5], (double)prod(o + 5), a);
    a = fma(w.g[6], (double)prod(o + 6), a);
    hp[e] = a;
    own += (rr >= 3 && rr < Sr + 3) ? p3 : 0;
  }
  return own;
}

// vertical pass: pixel p = thread + 256 i of the strip (row-major, Sr x W) from hp rows p / W .. p / W + 6
__device__ __forceinline__ void ssim_vpass(const SsimGeom& g, int Sr, const SsimTaps& w, const double* hp,
                                           double (&out)[kSsimPpt]) {
  const int np = Sr * g.W;
#pragma unroll
  for (int i = 0; i < kSsimPpt; ++i) {
    const int p = threadIdx.x + kSsimNt * i;
    double a = 0.0;
    if (p < np) {
      a = w.g[0] * hp[p];
#pragma unroll
      for (int k = 1; k < 7; ++k) a = fma(w.g[k], hp[p + k * g.W], a);
    }
    out[i] = a;
  }
}

// mu and var of the normalised frame over one staged strip (the tile is visible to every thread on entry; hp is
// free again on return)
__device__ __forceinline__ void ssim_self_maps(const SsimGeom& g, int Sr, const SsimTaps& w, const uint8_t* t,
                                               double inv_r, double* hp, double (&mu)[kSsimPpt],
                                               double (&var)[kSsimPpt]) {
  ssim_hpass(g, Sr, w, hp, [&](int o) { return (int)t[o]; });
  __syncthreads();
  ssim_vpass(g, Sr, w, hp, mu);
  __syncthreads();
  ssim_hpass(g, Sr, w, hp, [&](int o) { const int v = t[o]; return v * v; });
  __syncthreads();
  ssim_vpass(g, Sr, w, hp, var);
  __syncthreads();
  const double inv_r2 = inv_r * inv_r;
#pragma unroll
  for (int i = 0; i < kSsimPpt; ++i) {
    var[i] = (var[i] - mu[i] * mu[i]) * inv_r2;
    mu[i] = mu[i] * inv_r;
  }
}

struct SsimLds {
  double* hp;
  double* acc;       // [kSsimQt, 4] strip sums of the SSIM map per (query, wave)
  long long* accxy;  // [kSsimQt, 4] sums of xi yi
  int* red;          // [16]
  uint8_t* ty;
  uint8_t* tx[2];
};

static __host__ __device__ inline size_t ssim_hp_elems(int S, int W) { return (size_t)(S + 6) * W; }
static __host__ __device__ inline size_t ssim_tile_bytes(int S, int W) {
  return ((size_t)(S + 6) * (W + 6) + 7) & ~(size_t)7;
}
static __host__ __device__ inline size_t ssim_lds_bytes(int S, int W) {
  return ssim_hp_elems(S, W) * 8 + (size_t)kSsimQt * 4 * 16 + 64 + 3 * ssim_tile_bytes(S, W);
}

__device__ __forceinline__ SsimLds ssim_carve(const SsimGeom& g, double* smem) {
  SsimLds l;
  l.hp = smem;
  l.acc = l.hp + ssim_hp_elems(g.S, g.W);
  l.accxy = reinterpret_cast<long long*>(l.acc + kSsimQt * 4);
  l.red = reinterpret_cast<int*>(l.accxy + kSsimQt * 4);
  l.ty = reinterpret_cast<uint8_t*>(l.red + 16);
  l.tx[0] = l.ty + ssim_tile_bytes(g.S, g.W);
  l.tx[1] = l.tx[0] + ssim_tile_bytes(g.S, g.W);
  return l;
}

// One corpus frame y against queries q0 .. q0 + nq - 1 (nq <= kSsimQt): the per-pair routine of both score
// kernels.  Entry t is written at out[base + t * stride].  Block-cooperative; every branch is uniform.
__device__ void ssim_frame_vs_queries(const SsimGeom& g, const SsimTaps& w, const SsimLds& l, const uint8_t* y,
                                      const uint8_t* q, const double* q_maps, const double* q_stats, int q0, int nq,
                                      double* out_ssim, double* out_ncc, int64_t base, int64_t stride) {
  const int HW = g.H * g.W;
  const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63;
  const SsimStats sy = ssim_frame_stats(y, HW, l.red);
  if (tid < nq * 4) {
    l.acc[tid] = 0.0;
    l.accxy[tid] = 0;
  }
  const double inv_ry = 1.0 / ((double)(sy.mx - sy.mn) + 1e-8);
  double mu2[kSsimPpt], var2[kSsimPpt];
  for (int r0 = 0; r0 < g.H; r0 += g.S) {
    const int Sr = min(g.S, g.H - r0);
    const int np = Sr * g.W;
    ssim_stage(g, y, r0, Sr, sy.mn, l.ty);
    ssim_stage(g, q + (int64_t)q0 * HW, r0, Sr, (int)q_stats[4 * (int64_t)q0], l.tx[0]);
    __syncthreads();
    ssim_self_maps(g, Sr, w, l.ty, inv_ry, l.hp, mu2, var2);
    for (int j = 0; j < nq; ++j) {
      const int64_t a = q0 + j;
      const double* st = q_stats + 4 * a;
      const uint8_t* tx = l.tx[j & 1];
      const uint8_t* ty = l.ty;
      const int own = ssim_hpass(g, Sr, w, l.hp, [&](int o) { return (int)tx[o] * (int)ty[o]; });
      __syncthreads();
      // the next query's strip lands in the other buffer while this one's vertical pass runs
      if (j + 1 < nq) ssim_stage(g, q + (a + 1) * HW, r0, Sr, (int)st[4], l.tx[(j + 1) & 1]);
      const double inv_rx = 1.0 / ((st[1] - st[0]) + 1e-8);
      const double inv_rr = inv_rx * inv_ry;
      const double* xm = q_maps + a * 2 * HW + (int64_t)r0 * g.W;
      double pxy[kSsimPpt];
      ssim_vpass(g, Sr, w, l.hp, pxy);
      double part = 0.0;
#pragma unroll
      for (int i = 0; i < kSsimPpt; ++i) {
        const int p = tid + kSsimNt * i;
        if (p < np) {
          const double m1 = xm[p], v1 = xm[HW + p];
          const double m12 = m1 * mu2[i];
          const double cov = pxy[i] * inv_rr - m12;
          const double num = (2.0 * m12 + 1e-4) * (2.0 * cov + 9e-4);
          const double den = (m1 * m1 + mu2[i] * mu2[i] + 1e-4) * (v1 + var2[i] + 9e-4) + 1e-8;
          part += num / den;
        }
      }
      int sxy = own;
      for (int o = 32; o > 0; o >>= 1) {
        part += __shfl_xor(part, o);
        sxy += __shfl_xor(sxy, o);
      }
      if (lane == 0) {
        l.acc[j * 4 + wave] += part;
        l.accxy[j * 4 + wave] += sxy;
      }
      __syncthreads();
    }
  }
  if (tid < nq) {
    const int64_t a = q0 + tid;
    const double* st = q_stats + 4 * a;
    const double* ac = l.acc + tid * 4;
    out_ssim[base + tid * stride] = ((ac[0] + ac[1]) + (ac[2] + ac[3])) / (double)HW;
    if (out_ncc) {
      // Pearson is shift invariant: the sums of the centred integers xi, yi, all exact in int64
      const long long n = HW, ax = (long long)st[0];
      const long long sx = (long long)st[2] - n * ax;
      const long long sxx = (long long)st[3] - 2 * ax * (long long)st[2] + n * ax * ax;
      const long long sy1 = sy.s - n * sy.mn;
      const long long syy = sy.ss - 2 * sy.mn * sy.s + n * (long long)sy.mn * sy.mn;
      const long long* xy = l.accxy + tid * 4;
      const long long sxy = xy[0] + xy[1] + xy[2] + xy[3];
      const long long vx = n * sxx - sx * sx, vy = n * syy - sy1 * sy1;
      const long long cv = n * sxy - sx * sy1;
      out_ncc[base + tid * stride] = (vx == 0 || vy == 0) ? 0.0 : (double)cv / sqrt((double)vx * (double)vy);
    }
  }
  __syncthreads();  // acc is cleared by the next frame
}

__global__ __launch_bounds__(kSsimNt) void k_ssim_prepare(const uint8_t* frames, int64_t N, SsimGeom g, SsimTaps w,
                                                          double* maps, double* stats) {
  extern __shared__ double ssim_smem[];
  const SsimLds l = ssim_carve(g, ssim_smem);
  const int HW = g.H * g.W;
  for (int64_t n = blockIdx.x; n < N; n += gridDim.x) {
    const uint8_t* x = frames + n * HW;
    const SsimStats sx = ssim_frame_stats(x, HW, l.red);
    if (threadIdx.x == 0) {
      stats[4 * n + 0] = (double)sx.mn;
      stats[4 * n + 1] = (double)sx.mx;
      stats[4 * n + 2] = (double)sx.s;
      stats[4 * n + 3] = (double)sx.ss;
    }
    const double inv_r = 1.0 / ((double)(sx.mx - sx.mn) + 1e-8);
    double mu[kSsimPpt], var[kSsimPpt];
    for (int r0 = 0; r0 < g.H; r0 += g.S) {
      const int Sr = min(g.S, g.H - r0);
      ssim_stage(g, x, r0, Sr, sx.mn, l.ty);
      __syncthreads();
      ssim_self_maps(g, Sr, w, l.ty, inv_r, l.hp, mu, var);
      double* m = maps + n * 2 * HW + (int64_t)r0 * g.W;
#pragma unroll
      for (int i = 0; i < kSsimPpt; ++i) {
        const int p = threadIdx.x + kSsimNt * i;
        if (p < Sr * g.W) {
          m[p] = mu[i];
          m[HW + p] = var[i];
        }
      }
    }
  }
}

// grid (corpus frames, query tiles of qt)
__global__ __launch_bounds__(kSsimNt) void k_ssim_scores(const uint8_t* q, const double* q_maps, const double* q_stats,
                                                         int Q, int qt, const uint8_t* c, int64_t N, SsimGeom g,
                                                         SsimTaps w, double* out_ssim, double* out_ncc) {
  extern __shared__ double ssim_smem[];
  const SsimLds l = ssim_carve(g, ssim_smem);
  const int q0 = blockIdx.y * qt;
  const int nq = min(qt, Q - q0);
  for (int64_t n = blockIdx.x; n < N; n += gridDim.x)
    ssim_frame_vs_queries(g, w, l, c + n * g.H * g.W, q, q_maps, q_stats, q0, nq, out_ssim, out_ncc,
                          (int64_t)q0 * N + n, N);
}

// grid (list entries, queries)
__global__ __launch_bounds__(kSsimNt) void k_ssim_scores_listed(const uint8_t* q, const double* q_maps,
                                                                const double* q_stats, int Q, const uint8_t* c,
                                                                int64_t N, const int64_t* ids, int C, SsimGeom g,
                                                                SsimTaps w, double* out_ssim, double* out_ncc) {
  extern __shared__ double ssim_smem[];
  const SsimLds l = ssim_carve(g, ssim_smem);
  const int j = blockIdx.x;
  for (int a = blockIdx.y; a < Q; a += gridDim.y) {
    const int64_t o = (int64_t)a * C + j;
    const int64_t id = ids[o];
    if (id < 0 || id >= N) {  // a pad: no frame is read
      if (threadIdx.x == 0) {
        out_ssim[o] = -INFINITY;
        if (out_ncc) out_ncc[o] = -INFINITY;
      }
      continue;
    }
    ssim_frame_vs_queries(g, w, l, c + id * g.H * g.W, q, q_maps, q_stats, a, 1, out_ssim, out_ncc, o, 0);
  }
}

// ---------------------------------------------------------------------------------------------- host side
static SsimTaps ssim_taps() {  // cv2.getGaussianKernel(7, 1.5)
  SsimTaps t;
  double s = 0.0;
  for (int i = 0; i < 7; ++i) {
    t.g[i] = exp(-(double)((i - 3) * (i - 3)) / (2.0 * 1.5 * 1.5));
    s += t.g[i];
  }
  for (int i = 0; i < 7; ++i) t.g[i] /= s;
  return t;
}

// the one argument check of the three entries: shape, then the frame limits
static int ssim_check_shape(int64_t Q, int64_t N, int H, int W) {
  if (Q < 0 || N < 0 || H <= 0 || W <= 0) return fail(HQ_E_INVALID, "bad shape");
  if (H < kSsimMinSide || W < kSsimMinSide || H > kSsimMaxH || W > kSsimMaxW)
    return fail(HQ_E_UNSUPPORTED, "SSIM frames are %d x %d to %d x %d (window 7), got %d x %d", kSsimMinSide,
                kSsimMinSide, kSsimMaxH, kSsimMaxW, H, W);
  return HQ_OK;
}

static bool ssim_aligned8(const void* p) { return ((uintptr_t)p & 7) == 0; }

static SsimGeom ssim_geom(int H, int W) {
  SsimGeom g;
  g.H = H;
  g.W = W;
  g.S = kSsimStripPx / W < H ? kSsimStripPx / W : H;
  g.pitch = W + 6;
  g.rcpW = 1.0f / (float)W;
  g.rcpP = 1.0f / (float)g.pitch;
  return g;
}

static int ssim_grid(int64_t work) { return (int)(work < 65536 ? work : 65536); }

}  // namespace hq

using namespace hq;

extern "C" {

size_t hq_ssim_maps_bytes(int H, int W) {
  if (H < kSsimMinSide || W < kSsimMinSide || H > kSsimMaxH || W > kSsimMaxW) return 0;
  return (size_t)H * W * 2 * sizeof(double);
}

int hq_ssim_prepare(const uint8_t* frames, int64_t N, int H, int W, void* maps, double* stats, hq_stream_t stream) {
  if (int rc = ssim_check_shape(0, N, H, W)) return rc;
  if (N == 0) return HQ_OK;
  if (!frames || !maps || !stats) return fail(HQ_E_INVALID, "null buffer");
  if (!ssim_aligned8(maps) || !ssim_aligned8(stats)) return fail(HQ_E_INVALID, "maps and stats must be 8-byte aligned");
  const SsimGeom g = ssim_geom(H, W);
  const size_t lds = ssim_lds_bytes(g.S, W);
  if (lds > kSsimLdsMax) return fail(HQ_E_UNSUPPORTED, "frame %dx%d: strip exceeds 64 KiB of LDS", H, W);
  hipLaunchKernelGGL(k_ssim_prepare, dim3(ssim_grid(N)), dim3(kSsimNt), lds, (hipStream_t)stream, frames, N, g,
                     ssim_taps(), (double*)maps, stats);
  HQ_CHECK_LAUNCH();
  return HQ_OK;
}

int hq_ssim_scores(const uint8_t* q, const void* q_maps, const double* q_stats, int Q, const uint8_t* c, int64_t N,
                   int H, int W, double* out_ssim, double* out_ncc, hq_stream_t stream) {
  if (int rc = ssim_check_shape(Q, N, H, W)) return rc;
  if (Q == 0 || N == 0) return HQ_OK;
  if (!q || !q_maps || !q_stats || !c || !out_ssim) return fail(HQ_E_INVALID, "null buffer");
  if (!ssim_aligned8(q_maps) || !ssim_aligned8(q_stats) || !ssim_aligned8(out_ssim) || !ssim_aligned8(out_ncc))
    return fail(HQ_E_INVALID, "maps, stats and outputs must be 8-byte aligned");
  const SsimGeom g = ssim_geom(H, W);
  const size_t lds = ssim_lds_bytes(g.S, W);
  if (lds > kSsimLdsMax) return fail(HQ_E_UNSUPPORTED, "frame %dx%d: strip exceeds 64 KiB of LDS", H, W);
  // query tiles of equal size, at most kSsimQt each
  const int nt = (Q + kSsimQt - 1) / kSsimQt;
  if (nt > 65535) return fail(HQ_E_UNSUPPORTED, "too many queries");
  const int qt = (Q + nt - 1) / nt;
  hipLaunchKernelGGL(k_ssim_scores, dim3(ssim_grid(N), (unsigned)((Q + qt - 1) / qt)), dim3(kSsimNt), lds,
                     (hipStream_t)stream, q, (const double*)q_maps, q_stats, Q, qt, c, N, g, ssim_taps(), out_ssim,
                     out_ncc);
  HQ_CHECK_LAUNCH();
  return HQ_OK;
}

int hq_ssim_scores_listed(const uint8_t* q, const void* q_maps, const double* q_stats, int Q, const uint8_t* c,
                          int64_t N, int H, int W, const int64_t* ids, int C, double* out_ssim, double* out_ncc,
                          hq_stream_t stream) {
  if (int rc = ssim_check_shape(Q, N, H, W)) return rc;
  if (C < 1 || C > 65535) return fail(HQ_E_INVALID, "a list holds 1 .. 65535 entries, got C = %d", C);
  if (Q == 0) return HQ_OK;
  // (N = 0: every entry is a pad, c is never read)
  if (!q || !q_maps || !q_stats || !ids || !out_ssim || (N > 0 && !c)) return fail(HQ_E_INVALID, "null buffer");
  if (!ssim_aligned8(q_maps) || !ssim_aligned8(q_stats) || !ssim_aligned8(ids) || !ssim_aligned8(out_ssim) ||
      !ssim_aligned8(out_ncc))
    return fail(HQ_E_INVALID, "maps, stats, ids and outputs must be 8-byte aligned");
  const SsimGeom g = ssim_geom(H, W);
  const size_t lds = ssim_lds_bytes(g.S, W);
  if (lds > kSsimLdsMax) return fail(HQ_E_UNSUPPORTED, "frame %dx%d: strip exceeds 64 KiB of LDS", H, W);
  hipLaunchKernelGGL(k_ssim_scores_listed, dim3((unsigned)C, (unsigned)(Q < 65535 ? Q : 65535)), dim3(kSsimNt), lds,
                     (hipStream_t)stream, q, (const double*)q_maps, q_stats, Q, c, N, ids, C, g, ssim_taps(), out_ssim,
                     out_ncc);
  HQ_CHECK_LAUNCH();
  return HQ_OK;
}

}  // extern "C"
