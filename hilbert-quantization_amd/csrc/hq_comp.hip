// hq_comp.hip — the RAG engine's comprehensive frame similarity (rag/search/engine.py:478-727,
// 994-1138): score = 0.5 hierarchical + 0.3 embedding + 0.2 spatial of two enhanced frames [H, W].
//
//   hq_comp_describe   per frame (h, L, width, row_mask): detected original height, number of non-zero index rows
//                      among h .. H - 1, their largest trimmed length, their bit set (one launch).
//   hq_comp_scores     the exact float64 score of every (query, frame) pair from the frames and their descriptors:
//                      any pair (different heights, different L, dropped rows, zero blocks and windows, ws < 2).
//                      One wave per pair, the windows spread over its lanes, the query frame and its window norms
//                      staged in LDS once per workgroup for the 32 frames the workgroup walks.
//   hq_comp_scores_listed  the same score through an id list [Q, C]: the frames are read in place, both kernels call
//                      one per-pair function (comp_pair), so an entry is bit for bit the dense kernel's value.
//   hq_list_topk       the first k of a scored list by (score desc, list position asc): the engine's stable sort,
//                      threshold and cut (engine.py:512, 777-781), one workgroup per query.
//   hq_list_windows    every candidate widened to its window of consecutive frames (frame_cache.py:66-72), first
//                      appearances in order, one workgroup per query.
//   hq_comp_prepare    frames of one profile (h, L = H - h, every index row non-zero) -> "composite" rows in
//                      hq_cos_prepare's tiled split-f16 fragment layout, so that hq_cos_scores_mfma / hq_cos_topk,
//                      unchanged, return the comprehensive score: for such frames the score is an affine function
//                      of ONE dot product:
//                        2 score - 1 = sum_l 2 a_l cos_l + 2 b (cos_o + I_o) + sum_w 2 g (cos_w + I_w) + (2 sum a_l - 1)
//                      with a_l = 0.5 (w_l / sum w) / 2, b = 0.3 / 2, g = 0.2 / (2 n_windows), I = [both norms != 0].
//                      Row = [sqrt(2 g) x_w / |x_w|]_w, sqrt(2 b) o / |o|, [sqrt(2 a_l) r_l / |r_l|]_l, c,
//                            sqrt(2 b) [|o| != 0], [sqrt(2 g) [|x_w| != 0]]_w  (c = 2 sum a_l - 1 on the query side,
//                      1 on the corpus side; comp_layout has the reason for this order).  Every entry is at most 1
//                      in magnitude and is stored unscaled (hq_cos_prepare's own range), inv = 1, and the cosine
//                      epilogue (acc inv_q inv_c + 1) / 2 is the score.  Scaling the rows up so that the lo halves
//                      of the small window entries stay normal f16 numbers was measured and is worse (DESIGN.md
//                      §4.15, profiles/comp_error_bounds.txt).
// Dot products and norms accumulate in float64 (hq_rag.hip's contract: < 1e-12 for f64 frames, < 1e-6 against the
// reference's float32 arithmetic); the window mean follows NumPy's pairwise order.
#include "hq_common.h"

#include <math.h>

namespace hq {

typedef _Float16 ch8 __attribute__((ext_vector_type(8)));

constexpr int kCompCand = 32;      // frames one hq_comp_scores workgroup walks per staged query (8 per wave)
constexpr size_t kCompLds = 160 * 1024;

// window geometry of _calculate_spatial_locality_similarity for an original block h x W.  ws < 2 (one cosine over
// the block) is one h x W "window".
struct CompWin {
  int ws;                  // the reference's window_size (0 when it is below 2)
  int wr, wc, st, ni, nj;  // window rows / cols, stride, windows down / across
  __host__ __device__ int count() const { return ni * nj; }
  __host__ __device__ int elems() const { return wr * wc; }
};
__host__ __device__ inline CompWin comp_windows(int h, int W) {
  int ws = 4;
  if (h / 4 < ws) ws = h / 4;
  if (W / 4 < ws) ws = W / 4;
  CompWin g;
  if (ws < 2) {
    g.ws = 0; g.wr = h; g.wc = W; g.st = 1; g.ni = 1; g.nj = 1;
  } else {
    g.ws = g.wr = g.wc = ws;
    g.st = ws / 2;
    g.ni = (h - ws) / g.st + 1;
    g.nj = (W - ws) / g.st + 1;
  }
  return g;
}

template <typename V>
__device__ __forceinline__ V wave_sum(V v) {
  for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
  return v;
}

// ---- describe -----------------------------------------------------------------------------------------------
template <typename T>
__global__ __launch_bounds__(64) void k_comp_describe(const T* __restrict__ imgs, int64_t N, int H, int W,
                                                      int* __restrict__ desc, int* __restrict__ flag) {
  __shared__ int slot;
  const int lane = threadIdx.x;
  for (int64_t i = blockIdx.x; i < N; i += gridDim.x) {
    const T* img = imgs + i * (int64_t)H * W;
    const int h = detect_height(img, H, W, &slot);
    int L = 0, width = 0;
    unsigned mask = 0;
    if (H - h > 31) {
      L = -1;
      if (lane == 0 && flag) *flag = 1;
    } else {
      for (int r = h; r < H; ++r) {
        int last = -1;
        for (int c = lane; c < W; c += 64)
          if (img[(int64_t)r * W + c] != (T)0) last = c;
        for (int o = 32; o > 0; o >>= 1) {
          const int other = __shfl_xor(last, o, 64);
          last = other > last ? other : last;
        }
        if (last >= 0) {
          ++L;
          mask |= 1u << (r - h);
          if (last + 1 > width) width = last + 1;
        }
      }
    }
    if (lane == 0) {
      desc[4 * i + 0] = h;
      desc[4 * i + 1] = L;
      desc[4 * i + 2] = width;
      desc[4 * i + 3] = (int)mask;
    }
  }
}

// ---- exact scores -------------------------------------------------------------------------------------------
// (cos + 1) / 2 from the three sums, 0.0 for a zero norm (engine.py:654-660)
__device__ __forceinline__ double comp_cos01(double dot, double na, double nb) {
  return (na != 0.0 && nb != 0.0) ? (dot / (sqrt(na) * sqrt(nb)) + 1.0) / 2.0 : 0.0;
}

// One (query, frame) pair by one wave: the staged query frame qf with its descriptor (hq_, Lq, maskq), window geometry
// gq / nwq and window square norms qn, against frame b (hc clamped by the caller, Lc, maskc).  wsc: the wave's window
// score list.  Returns the score on every lane; pt[3] = the components.  Shared by k_comp_scores and
// k_comp_scores_listed, so that both write the same bits for a pair.
template <typename T>
__device__ __forceinline__ double comp_pair(const T* qf, int hq_, int Lq, unsigned maskq, const CompWin& gq, int nwq,
                                            const double* qn, double* wsc, const T* __restrict__ b, int hc, int Lc,
                                            unsigned maskc, int H, int W, const double* __restrict__ wt, int ML,
                                            int lane, double* pt) {
  // hierarchical: the non-zero index rows of each frame in order, zero-padded to M = max(L_q, L_c) levels,
  // weights of M levels, accumulated left to right (engine.py:535-551, 1053-1099)
  double hier = 0.0;
  if (Lq > 0 && Lc > 0) {
    const int M = Lq > Lc ? Lq : Lc;
    if (M > ML) {
      hier = nan("");  // outside the caller's weight table: never read past it
    } else {
      const double* w = wt + (size_t)M * ML;
      unsigned mq = maskq, mc = maskc;
      double tot = 0.0, tw = 0.0;
      for (int l = 0; l < M; ++l) {
        int rq = -1, rc = -1;
        if (mq) { rq = hq_ + __ffs(mq) - 1; mq &= mq - 1; }
        if (mc) { rc = hc + __ffs(mc) - 1; mc &= mc - 1; }
        double s = 0.0;
        if (rq >= 0 && rc >= 0 && rq < H && rc < H) {
          double dot = 0.0, na = 0.0, nb = 0.0;
          for (int c = lane; c < W; c += 64) {
            const double x = (double)qf[rq * W + c], y = (double)b[rc * W + c];
            dot = fma(x, y, dot);
            na = fma(x, x, na);
            nb = fma(y, y, nb);
          }
          s = comp_cos01(wave_sum(dot), wave_sum(na), wave_sum(nb));
        }
        tot += s * w[l];
        tw += w[l];
      }
      hier = tw != 0.0 ? tot / tw : 0.0;
    }
  }
  // embedding: the original blocks flattened, truncated to the common length (engine.py:604-660)
  double emb;
  {
    const int m = (hq_ < hc ? hq_ : hc) * W;
    double dot = 0.0, na = 0.0, nb = 0.0;
    for (int i = lane; i < m; i += 64) {
      const double x = (double)qf[i], y = (double)b[i];
      dot = fma(x, y, dot);
      na = fma(x, x, na);
      nb = fma(y, y, nb);
    }
    emb = comp_cos01(wave_sum(dot), wave_sum(na), wave_sum(nb));
  }
  // spatial (engine.py:662-714): 0.0 for different heights; ws < 2: the embedding cosine
  double spa = 0.0;
  if (hq_ == hc) {
    if (gq.ws < 2) {
      spa = emb;
    } else {
      for (int w = lane; w < nwq; w += 64) {
        const int off = (w / gq.nj) * gq.st * W + (w % gq.nj) * gq.st;
        double dot = 0.0, nb = 0.0;
        for (int r = 0; r < gq.wr; ++r)
          for (int c = 0; c < gq.wc; ++c) {
            const double x = (double)qf[off + r * W + c], y = (double)b[off + r * W + c];
            dot = fma(x, y, dot);
            nb = fma(y, y, nb);
          }
        wsc[w] = comp_cos01(dot, qn[w], nb);
      }
      __threadfence_block();
      __builtin_amdgcn_wave_barrier();
      double mean = 0.0;
      if (lane == 0) {
        auto f = [&](int k) -> double { return wsc[k]; };
        mean = np_sum<double>(f, nwq) / (double)nwq;
      }
      spa = __shfl(mean, 0, 64);
      __threadfence_block();
      __builtin_amdgcn_wave_barrier();  // lane 0 has read the list before the next pair rewrites it
    }
  }
  pt[0] = hier;
  pt[1] = emb;
  pt[2] = spa;
  return 0.5 * hier + 0.3 * emb + 0.2 * spa;
}

// Stage query q for its workgroup: the frame into qf, its window square norms into qn; the clamped height, level
// count, row mask and window geometry come back by reference.  Every thread of the workgroup calls it.
template <typename T>
__device__ __forceinline__ void comp_stage_query(const T* __restrict__ Qi, const int* __restrict__ dq, int q, int H,
                                                 int W, T* qf, double* qn, int& hq_, int& Lq, unsigned& maskq,
                                                 CompWin& gq) {
  const int img = H * W;
  __syncthreads();  // the previous query's readers are done
  const T* a = Qi + (int64_t)q * img;
  for (int i = threadIdx.x; i < img; i += 256) qf[i] = a[i];
  // heights are clamped to [1, H]: a descriptor this library did not write cannot steer a read outside a frame
  hq_ = min(max(dq[4 * q], 1), H);
  Lq = dq[4 * q + 1];
  maskq = (unsigned)dq[4 * q + 3];
  gq = comp_windows(hq_, W);
  const int nwq = gq.count();  // <= nw_cap (the host sizes nw_cap over every height)
  __syncthreads();
  for (int w = threadIdx.x; w < nwq; w += 256) {
    const T* x = qf + (w / gq.nj) * gq.st * W + (w % gq.nj) * gq.st;
    double na = 0.0;
    for (int r = 0; r < gq.wr; ++r)
      for (int c = 0; c < gq.wc; ++c) {
        const double v = (double)x[r * W + c];
        na = fma(v, v, na);
      }
    qn[w] = na;
  }
  __syncthreads();
}

// LDS: window scores [4 waves][nw_cap] f64, the staged query's window square norms [nw_cap] f64, the query frame
// [H W] T.  Workgroup (x, y): frames 32 x .. 32 x + 31 against queries y, y + gridDim.y, ...
template <typename T>
__global__ __launch_bounds__(256) void k_comp_scores(const T* __restrict__ Qi, const int* __restrict__ dq, int Qn,
                                                     const T* __restrict__ Ci, const int* __restrict__ dc, int64_t N,
                                                     int H, int W, const double* __restrict__ wt, int ML, int nw_cap,
                                                     double* __restrict__ out, double* __restrict__ parts) {
  extern __shared__ double sm[];
  const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
  double* wsc = sm + (size_t)wv * nw_cap;
  double* qn = sm + (size_t)4 * nw_cap;
  T* qf = reinterpret_cast<T*>(sm + (size_t)5 * nw_cap);
  const int img = H * W;
  const int64_t c0 = (int64_t)blockIdx.x * kCompCand;
  const int64_t c1 = c0 + kCompCand < N ? c0 + kCompCand : N;
  for (int q = blockIdx.y; q < Qn; q += gridDim.y) {
    int hq_, Lq;
    unsigned maskq;
    CompWin gq;
    comp_stage_query(Qi, dq, q, H, W, qf, qn, hq_, Lq, maskq, gq);
    for (int64_t cand = c0 + wv; cand < c1; cand += 4) {
      const int hc = min(max(dc[4 * cand], 1), H);
      double pt[3];
      const double score = comp_pair(qf, hq_, Lq, maskq, gq, gq.count(), qn, wsc, Ci + cand * img, hc,
                                     dc[4 * cand + 1], (unsigned)dc[4 * cand + 3], H, W, wt, ML, lane, pt);
      if (lane == 0) {
        const int64_t o = (int64_t)q * N + cand;
        out[o] = score;
        if (parts) {
          parts[3 * o + 0] = pt[0];
          parts[3 * o + 1] = pt[1];
          parts[3 * o + 2] = pt[2];
        }
      }
    }
  }
}

// The same pairs through an id list: workgroup (x, y) walks entries 32 x .. 32 x + 31 of ids[q] for queries y,
// y + gridDim.y, ...; the frame of entry j is read in place at Ci + ids[q, j] H W.  An id outside [0, N) is a pad:
// -inf, parts 0.0, nothing read.
template <typename T>
__global__ __launch_bounds__(256) void k_comp_scores_listed(const T* __restrict__ Qi, const int* __restrict__ dq, int Qn,
                                                            const T* __restrict__ Ci, const int* __restrict__ dc,
                                                            int64_t N, int H, int W, const int64_t* __restrict__ ids,
                                                            int C, const double* __restrict__ wt, int ML, int nw_cap,
                                                            double* __restrict__ out, double* __restrict__ parts) {
  extern __shared__ double sm[];
  const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
  double* wsc = sm + (size_t)wv * nw_cap;
  double* qn = sm + (size_t)4 * nw_cap;
  T* qf = reinterpret_cast<T*>(sm + (size_t)5 * nw_cap);
  const int img = H * W;
  const int j0 = (int)blockIdx.x * kCompCand;
  const int j1 = j0 + kCompCand < C ? j0 + kCompCand : C;
  for (int q = blockIdx.y; q < Qn; q += gridDim.y) {
    int hq_, Lq;
    unsigned maskq;
    CompWin gq;
    comp_stage_query(Qi, dq, q, H, W, qf, qn, hq_, Lq, maskq, gq);
    for (int j = j0 + wv; j < j1; j += 4) {
      const int64_t o = (int64_t)q * C + j;
      const int64_t cand = ids[o];  // wave-uniform
      double pt[3] = {0.0, 0.0, 0.0};
      double score = -INFINITY;
      if (cand >= 0 && cand < N) {
        const int hc = min(max(dc[4 * cand], 1), H);
        score = comp_pair(qf, hq_, Lq, maskq, gq, gq.count(), qn, wsc, Ci + cand * img, hc, dc[4 * cand + 1],
                          (unsigned)dc[4 * cand + 3], H, W, wt, ML, lane, pt);
      }
      if (lane == 0) {
        out[o] = score;
        if (parts) {
          parts[3 * o + 0] = pt[0];
          parts[3 * o + 1] = pt[1];
          parts[3 * o + 2] = pt[2];
        }
      }
    }
  }
}

// ---- list ranking and neighbour windows ---------------------------------------------------------------------
constexpr int kListMax = 1024;  // entries of one list: one per thread of the workgroup

// One workgroup per query: entry j's rank = the eligible entries that precede it in (score desc, position asc);
// ranks below k are written at their rank, the rest of the row is padded.  Ineligible entries sit in LDS as NaN.
__global__ __launch_bounds__(kListMax) void k_list_topk(const double* __restrict__ scores,
                                                        const int64_t* __restrict__ ids, int C, int k, double thr,
                                                        int mode, double* __restrict__ out_score,
                                                        int64_t* __restrict__ out_id, int* __restrict__ out_count) {
  __shared__ double s[kListMax];
  __shared__ int total;
  const int q = blockIdx.x, j = threadIdx.x;
  if (j == 0) total = 0;
  double v = nan("");
  int64_t id = -1;
  if (j < C) {
    const double x = scores[(int64_t)q * C + j];
    id = ids[(int64_t)q * C + j];
    const bool ok = id >= 0 && x == x && (mode == 0 || (mode == 1 ? x >= thr : x > thr));
    if (ok) v = x;
    s[j] = v;
  }
  __syncthreads();
  const bool mine = v == v;
  if (mine) {
    int rank = 0;
    for (int i = 0; i < C; ++i) {
      const double o = s[i];  // NaN compares false both ways
      rank += (o > v || (o == v && i < j)) ? 1 : 0;
    }
    if (rank < k) {
      out_score[(int64_t)q * k + rank] = v;
      out_id[(int64_t)q * k + rank] = id;
    }
    atomicAdd(&total, 1);
  }
  __syncthreads();
  const int n = total < k ? total : k;
  for (int r = n + j; r < k; r += kListMax) {
    out_score[(int64_t)q * k + r] = -INFINITY;
    out_id[(int64_t)q * k + r] = -1;
  }
  if (j == 0) out_count[q] = n;
}

// One workgroup per query: thread j = window slot j % window of head j / window -> its frame (or -1) in LDS; a
// slot is dropped when an earlier slot holds the same frame; the kept slots are compacted by a prefix count.
__global__ __launch_bounds__(kListMax) void k_list_windows(const int64_t* __restrict__ heads, int C0, int64_t N,
                                                           int window, int64_t* __restrict__ out,
                                                           int* __restrict__ out_count) {
  __shared__ int64_t f[kListMax];
  __shared__ int keep[kListMax];
  __shared__ int total;
  const int q = blockIdx.x, j = threadIdx.x, n = C0 * window;
  int64_t mine = -1;
  if (j < n) {
    const int64_t h = heads[(int64_t)q * C0 + j / window];
    if (h >= 0) {
      const int64_t half = window / 2;
      const int64_t start = h - half > 0 ? h - half : 0;
      const int64_t end = start + window < h + half + 1 ? start + window : h + half + 1;
      const int64_t x = start + j % window;
      if (x < end && x < N) mine = x;
    }
    f[j] = mine;
  }
  __syncthreads();
  int kept = 0;
  if (mine >= 0) {
    kept = 1;
    for (int i = 0; i < j; ++i)
      if (f[i] == mine) { kept = 0; break; }
  }
  if (j < n) keep[j] = kept;
  __syncthreads();
  int pos = 0;
  if (j < n) {
    for (int i = 0; i < j; ++i) pos += keep[i];
    if (kept) out[(int64_t)q * n + pos] = mine;
  }
  if (j == n - 1) total = pos + kept;
  __syncthreads();
  if (j >= total && j < n) out[(int64_t)q * n + j] = -1;
  if (j == 0) out_count[q] = total;
}

// ---- composite rows -----------------------------------------------------------------------------------------
// Section order (the dot product does not care, its float32 accumulation does: the matrix cores' accumulate
// truncates, so the error of a pair grows with the partial sum it carries through the K steps): the windows first
// (most of the row, 0.2 of the weight), then the original block (0.3), the levels (0.5, a few steps), and the
// columns that are constants for a valid pair last and next to each other (-0.5, +0.3, +0.2 spread over the
// window indicators), so that they cancel within the last K steps.
struct CompLayout {
  int K, L, off_win, off_orig, off_lev, off_const, off_oind, off_wind;
  CompWin g;
};
__host__ __device__ inline CompLayout comp_layout(int H, int W, int h) {
  CompLayout y;
  y.g = comp_windows(h, W);
  y.L = H - h;
  y.off_win = 0;
  y.off_orig = y.g.count() * y.g.elems();
  y.off_lev = y.off_orig + h * W;
  y.off_const = y.off_lev + y.L * W;
  y.off_oind = y.off_const + 1;
  y.off_wind = y.off_oind + 1;
  y.K = y.off_wind + y.g.count();
  return y;
}

// One 16-wave workgroup per 16-frame tile.  Phase 1: wave w takes frame 16 t + w and leaves, in LDS, one
// coefficient per section (weight / float64 norm, 0 for a zero norm; every coefficient 0 for a pad row and for a
// frame holding a NaN or inf).  Phase 2: the waves split the tile's K steps; lane 16 g + j converts frame j's
// entries 32 kb + 8 g .. + 7, so every fragment leaves as one contiguous 1 KiB wave store per plane.
// LDS: coef [16][S] f64, S = L + 1 + n_windows (levels, original block, windows).
__global__ __launch_bounds__(1024) void k_comp_prepare(const float* __restrict__ X, int64_t N, int64_t ld, int H, int W,
                                                       int h, int side, const double* __restrict__ level_coef, int Kp,
                                                       int64_t rows_out, _Float16* __restrict__ X16,
                                                       double* __restrict__ inv) {
  extern __shared__ double coef[];
  const CompLayout y = comp_layout(H, W, h);
  const int nw = y.g.count(), S = y.L + 1 + nw;
  const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6, j = lane & 15, g = lane >> 4;
  const int KB = Kp / 32;
  const double sb = sqrt(0.3), sg = sqrt(0.2 / (double)nw);  // sqrt(2 b), sqrt(2 g)
  double cq = -1.0;  // the query side's constant column: 2 sum a_l - 1 = sum level_coef^2 - 1
  for (int l = 0; l < y.L; ++l) cq += level_coef[l] * level_coef[l];
  for (int64_t t = blockIdx.x; t < rows_out / 16; t += gridDim.x) {
    double* cf = coef + (size_t)wv * S;
    const int64_t r0 = 16 * t + wv;
    if (r0 >= N) {
      for (int s = lane; s < S; s += 64) cf[s] = 0.0;
      if (lane == 0) inv[r0] = 0.0;
    } else {
      const float* x = X + r0 * ld;
      int bad = 0;
      double so = 0.0;
      for (int i = lane; i < H * W; i += 64) {
        const float v = x[i];
        bad |= !(fabsf(v) <= 3.4028234663852886e38f);
        if (i < h * W) so = fma((double)v, (double)v, so);
      }
      bad = __any(bad);
      so = wave_sum(so);
      for (int l = 0; l < y.L; ++l) {
        double s = 0.0;
        for (int c = lane; c < W; c += 64) {
          const double v = (double)x[(h + l) * W + c];
          s = fma(v, v, s);
        }
        s = wave_sum(s);
        if (lane == 0) cf[l] = (!bad && s > 0.0) ? level_coef[l] / sqrt(s) : 0.0;
      }
      if (lane == 0) cf[y.L] = (!bad && so > 0.0) ? sb / sqrt(so) : 0.0;
      for (int w = lane; w < nw; w += 64) {
        const float* p = x + (w / y.g.nj) * y.g.st * W + (w % y.g.nj) * y.g.st;
        double s = 0.0;
        for (int r = 0; r < y.g.wr; ++r)
          for (int c = 0; c < y.g.wc; ++c) {
            const double v = (double)p[r * W + c];
            s = fma(v, v, s);
          }
        cf[y.L + 1 + w] = (!bad && s > 0.0) ? sg / sqrt(s) : 0.0;
      }
      if (lane == 0) inv[r0] = bad ? 0.0 : 1.0;
    }
    __syncthreads();
    const int64_t r = 16 * t + j;
    const bool live = r < N;
    const float* x = X + (live ? r : 0) * ld;
    const double* cj = coef + (size_t)j * S;
    const int we = y.g.elems();
    for (int kb = wv; kb < KB; kb += 16) {
      ch8 hi, lo;
#pragma unroll
      for (int u = 0; u < 8; ++u) {
        const int k = 32 * kb + 8 * g + u;
        double val = 0.0;
        if (live && k < y.K) {
          int i;
          if ((i = k - y.off_win) >= 0 && i < nw * we) {
            const int w = i / we, e = i - w * we;
            const int off = ((w / y.g.nj) * y.g.st + e / y.g.wc) * W + (w % y.g.nj) * y.g.st + e % y.g.wc;
            val = (double)x[off] * cj[y.L + 1 + w];
          } else if ((i = k - y.off_orig) >= 0 && i < h * W) {
            val = (double)x[i] * cj[y.L];
          } else if ((i = k - y.off_lev) >= 0 && i < y.L * W) {
            val = (double)x[h * W + i] * cj[i / W];
          } else if (k == y.off_const) {
            // (a frame holding a NaN or inf keeps this column too: its inv = 0 gives 0.0 against everything)
            val = side == 0 ? cq : 1.0;
          } else if (k == y.off_oind) {
            val = cj[y.L] != 0.0 ? sb : 0.0;
          } else if ((i = k - y.off_wind) >= 0 && i < nw) {
            val = cj[y.L + 1 + i] != 0.0 ? sg : 0.0;
          }
        }
        const float v = (float)val;
        const _Float16 hh = (_Float16)v;
        hi[u] = hh;
        lo[u] = (_Float16)(v - (float)hh);
      }
      _Float16* f = X16 + ((t * KB + kb) * 2) * 512 + 8 * lane;
      *reinterpret_cast<ch8*>(f) = hi;
      *reinterpret_cast<ch8*>(f + 512) = lo;
    }
    __syncthreads();  // coef is rewritten by the next tile
  }
}

static int comp_grid(int64_t work) {
  if (work > 65536) work = 65536;
  return (int)(work < 1 ? 1 : work);
}

static int comp_max_windows(int H, int W) {
  int m = 1;
  for (int h = 1; h <= H; ++h) {
    const int n = comp_windows(h, W).count();
    if (n > m) m = n;
  }
  return m;
}

}  // namespace hq

using namespace hq;

extern "C" {

int hq_comp_describe(int dtype, const void* imgs, int64_t N, int H, int W, int32_t* desc, hq_stream_t stream) {
  if (N < 0 || H <= 0 || W <= 0) return fail(HQ_E_INVALID, "bad shape");
  if (dtype != HQ_F32 && dtype != HQ_F64) return fail(HQ_E_UNSUPPORTED, "dtype %d (float32 / float64)", dtype);
  if (N == 0) return HQ_OK;
  if (!imgs || !desc) return fail(HQ_E_INVALID, "null buffer");
  const hipStream_t s = (hipStream_t)stream;
  // only frames of more than 32 rows can have more than 31 index rows: those launches carry a flag that is read
  // back (one 4-byte copy and a stream synchronisation)
  int* flag = nullptr;
  if (H > 32) {
    HQ_CHECK_HIP(hipMalloc((void**)&flag, sizeof(int)));
    hipError_t e = hipMemsetAsync(flag, 0, sizeof(int), s);
    if (e != hipSuccess) {
      (void)hipFree(flag);
      return fail(HQ_E_HIP, "hipMemsetAsync: %s", hipGetErrorString(e));
    }
  }
  const int g = comp_grid(N);
  if (dtype == HQ_F32)
    hipLaunchKernelGGL(k_comp_describe<float>, dim3(g), dim3(64), 0, s, (const float*)imgs, N, H, W, desc, flag);
  else
    hipLaunchKernelGGL(k_comp_describe<double>, dim3(g), dim3(64), 0, s, (const double*)imgs, N, H, W, desc, flag);
  hipError_t le = hipGetLastError();
  int over = 0;
  if (flag) {
    if (le == hipSuccess) le = hipMemcpyAsync(&over, flag, sizeof(int), hipMemcpyDeviceToHost, s);
    if (le == hipSuccess) le = hipStreamSynchronize(s);
    (void)hipFree(flag);
  }
  if (le != hipSuccess) return fail(HQ_E_HIP, "hq_comp_describe: %s", hipGetErrorString(le));
  if (over) return fail(HQ_E_UNSUPPORTED, "a frame has more than 31 index rows below its detected height");
  return HQ_OK;
}

int hq_comp_scores(int dtype, const void* q, const int32_t* desc_q, int Q, const void* c, const int32_t* desc_c,
                   int64_t N, int H, int W, const double* weights, int max_levels, double* out, double* parts,
                   hq_stream_t stream) {
  if (Q < 0 || N < 0 || H <= 0 || W <= 0 || max_levels < 0) return fail(HQ_E_INVALID, "bad shape");
  if (dtype != HQ_F32 && dtype != HQ_F64) return fail(HQ_E_UNSUPPORTED, "dtype %d (float32 / float64)", dtype);
  if (Q == 0 || N == 0) return HQ_OK;
  if (!q || !desc_q || !c || !desc_c || !out || (max_levels > 0 && !weights)) return fail(HQ_E_INVALID, "null buffer");
  if ((int64_t)H * W > (1 << 24)) return fail(HQ_E_UNSUPPORTED, "frame %dx%d too large", H, W);
  const int nw_cap = comp_max_windows(H, W);
  const size_t lds = (size_t)5 * nw_cap * 8 + (size_t)H * W * (dtype == HQ_F32 ? 4 : 8);
  if (lds > kCompLds) return fail(HQ_E_UNSUPPORTED, "frame %dx%d: query and window lists exceed 160 KiB of LDS", H, W);
  const int64_t bx = (N + kCompCand - 1) / kCompCand;
  if (bx > 0x7FFFFFFF) return fail(HQ_E_UNSUPPORTED, "too many frames");
  const dim3 grid((unsigned)bx, (unsigned)(Q < 65535 ? Q : 65535));
  const hipStream_t s = (hipStream_t)stream;
  if (dtype == HQ_F32) {
    HQ_CHECK_HIP(hipFuncSetAttribute((const void*)k_comp_scores<float>, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
    hipLaunchKernelGGL(k_comp_scores<float>, grid, dim3(256), lds, s, (const float*)q, desc_q, Q, (const float*)c,
                       desc_c, N, H, W, weights, max_levels, nw_cap, out, parts);
  } else {
    HQ_CHECK_HIP(hipFuncSetAttribute((const void*)k_comp_scores<double>, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
    hipLaunchKernelGGL(k_comp_scores<double>, grid, dim3(256), lds, s, (const double*)q, desc_q, Q, (const double*)c,
                       desc_c, N, H, W, weights, max_levels, nw_cap, out, parts);
  }
  HQ_CHECK_LAUNCH();
  return HQ_OK;
}

int hq_comp_scores_listed(int dtype, const void* q, const int32_t* desc_q, int Q, const void* c, const int32_t* desc_c,
                          int64_t N, int H, int W, const int64_t* ids, int C, const double* weights, int max_levels,
                          double* out, double* parts, hq_stream_t stream) {
  if (Q < 0 || N < 0 || C < 0 || H <= 0 || W <= 0 || max_levels < 0) return fail(HQ_E_INVALID, "bad shape");
  if (dtype != HQ_F32 && dtype != HQ_F64) return fail(HQ_E_UNSUPPORTED, "dtype %d (float32 / float64)", dtype);
  if (Q == 0 || C == 0) return HQ_OK;
  // (N = 0: every entry is a pad, c and desc_c are never read)
  if (!q || !desc_q || !ids || !out || (N > 0 && (!c || !desc_c)) || (max_levels > 0 && !weights))
    return fail(HQ_E_INVALID, "null buffer");
  if ((int64_t)H * W > (1 << 24)) return fail(HQ_E_UNSUPPORTED, "frame %dx%d too large", H, W);
  const int nw_cap = comp_max_windows(H, W);
  const size_t lds = (size_t)5 * nw_cap * 8 + (size_t)H * W * (dtype == HQ_F32 ? 4 : 8);
  if (lds > kCompLds) return fail(HQ_E_UNSUPPORTED, "frame %dx%d: query and window lists exceed 160 KiB of LDS", H, W);
  const dim3 grid((unsigned)((C + kCompCand - 1) / kCompCand), (unsigned)(Q < 65535 ? Q : 65535));
  const hipStream_t s = (hipStream_t)stream;
  if (dtype == HQ_F32) {
    HQ_CHECK_HIP(hipFuncSetAttribute((const void*)k_comp_scores_listed<float>, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
    hipLaunchKernelGGL(k_comp_scores_listed<float>, grid, dim3(256), lds, s, (const float*)q, desc_q, Q, (const float*)c,
                       desc_c, N, H, W, ids, C, weights, max_levels, nw_cap, out, parts);
  } else {
    HQ_CHECK_HIP(hipFuncSetAttribute((const void*)k_comp_scores_listed<double>, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
    hipLaunchKernelGGL(k_comp_scores_listed<double>, grid, dim3(256), lds, s, (const double*)q, desc_q, Q,
                       (const double*)c, desc_c, N, H, W, ids, C, weights, max_levels, nw_cap, out, parts);
  }
  HQ_CHECK_LAUNCH();
  return HQ_OK;
}

int hq_list_topk(const double* scores, const int64_t* ids, int Q, int C, int k, double threshold, int thr_mode,
                 double* out_score, int64_t* out_id, int32_t* out_count, hq_stream_t stream) {
  if (Q < 0 || thr_mode < 0 || thr_mode > 2) return fail(HQ_E_INVALID, "bad shape");
  if (C < 1 || C > kListMax || k < 1) return fail(HQ_E_UNSUPPORTED, "list of %d entries, k = %d (1 .. %d, k >= 1)", C, k, kListMax);
  if (Q == 0) return HQ_OK;
  if (!scores || !ids || !out_score || !out_id || !out_count) return fail(HQ_E_INVALID, "null buffer");
  hipLaunchKernelGGL(k_list_topk, dim3((unsigned)Q), dim3(kListMax), 0, (hipStream_t)stream, scores, ids, C, k, threshold,
                     thr_mode, out_score, out_id, out_count);
  HQ_CHECK_LAUNCH();
  return HQ_OK;
}

int hq_list_windows(const int64_t* heads, int Q, int C0, int64_t N, int window, int64_t* out, int32_t* out_count,
                    hq_stream_t stream) {
  if (Q < 0 || C0 < 0 || N < 0) return fail(HQ_E_INVALID, "bad shape");
  if (window < 1 || window > 64 || (int64_t)C0 * window > kListMax)
    return fail(HQ_E_UNSUPPORTED, "window %d over %d heads (1 .. 64, at most %d entries)", window, C0, kListMax);
  if (Q == 0 || C0 == 0) return HQ_OK;
  if (!heads || !out || !out_count) return fail(HQ_E_INVALID, "null buffer");
  hipLaunchKernelGGL(k_list_windows, dim3((unsigned)Q), dim3(kListMax), 0, (hipStream_t)stream, heads, C0, N, window, out,
                     out_count);
  HQ_CHECK_LAUNCH();
  return HQ_OK;
}

int hq_comp_layout(int H, int W, int h, int32_t* out) {
  if (H <= 0 || W <= 0 || h <= 0 || h > H || H - h > 31) return fail(HQ_E_INVALID, "bad profile H=%d W=%d h=%d", H, W, h);
  const CompWin g = comp_windows(h, W);
  const int64_t k = (int64_t)H * W + 1 + (int64_t)g.ni * g.nj * ((int64_t)g.wr * g.wc + 1) + 1;
  if (k > (1 << 24)) return fail(HQ_E_UNSUPPORTED, "composite row of %lld entries", (long long)k);
  const CompLayout y = comp_layout(H, W, h);
  if (out) {
    out[0] = y.K;
    out[1] = y.L;
    out[2] = y.g.ws;  // 0: ws < 2, one cosine over the block
    out[3] = y.g.st;
    out[4] = y.g.ni;
    out[5] = y.g.nj;
    out[6] = y.off_win;
    out[7] = y.off_orig;
    out[8] = y.off_lev;
    out[9] = y.off_const;
    out[10] = y.off_oind;
    out[11] = y.off_wind;
  }
  return y.K;
}

int hq_comp_padded_k(int H, int W, int h) {
  const int k = hq_comp_layout(H, W, h, nullptr);
  return k < 0 ? k : hq_cos_padded_k(k);
}

int hq_comp_prepare(const float* imgs, int64_t N, int64_t ld, int H, int W, int h, int side, const double* level_coef,
                    void* X16, double* inv, hq_stream_t stream) {
  if (N < 0 || H <= 0 || W <= 0 || ld < (int64_t)H * W || (side != 0 && side != 1)) return fail(HQ_E_INVALID, "bad shape");
  const int K = hq_comp_layout(H, W, h, nullptr);
  if (K < 0) return K;
  if (N == 0) return HQ_OK;
  if (!imgs || !X16 || !inv || (H > h && !level_coef)) return fail(HQ_E_INVALID, "null buffer");
  const int Kp = hq_cos_padded_k(K);
  const int64_t rows = hq_cos_padded_rows(N);
  const size_t lds = (size_t)16 * ((H - h) + 1 + comp_windows(h, W).count()) * 8;
  if (lds > kCompLds) return fail(HQ_E_UNSUPPORTED, "frame %dx%d: section coefficients exceed 160 KiB of LDS", H, W);
  HQ_CHECK_HIP(hipFuncSetAttribute((const void*)k_comp_prepare, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
  hipLaunchKernelGGL(k_comp_prepare, dim3((unsigned)comp_grid(rows / 16)), dim3(1024), lds, (hipStream_t)stream, imgs, N,
                     ld, H, W, h, side, level_coef, Kp, rows, reinterpret_cast<_Float16*>(X16), inv);
  HQ_CHECK_LAUNCH();
  return HQ_OK;
}

}  // extern "C"
