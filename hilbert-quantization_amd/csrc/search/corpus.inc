// search/corpus.inc: part of hq_search.hip (one translation unit: included there, inside namespace hq, between
// k_packov and the overall scan's kernels; no include guard and no #include of its own).
// The corpus mutation kernels: k_seg_append, k_seg_gather and k_seg_replace keep a resident corpus's prepared
// rows and split copies in step with its rows, one launch each.  The reference rebuilds its index instead
// (core/search_engine.py has no counterpart); the rows written are those of the preparation kernels.
// Uses, from the text above its #include: SegInfo, seg_prepare_one, seg_prepare_coop, z16_rows, pack0_elem,
// flag_row, OvLayout, packov_elem.  Has guarded loads: DIAG part 1.
#undef HQ_PART
#define HQ_PART 1

// Appending M rows to a resident corpus of N0 (hq_seg_append), one launch: one wave per new row N0 + i runs
// k_seg_prepare_pack0's steps (the row's segments from an LDS copy, then its split level-0 copy), then the
// row's split overall copy (packov_elem) and its entry of the flagged-row list (flag_row); the blocks past
// N1 = N0 + M write the pad rows up to z16_rows(N1).  Every write lands in rows >= N0 (the layouts address by
// row: z16_elem, ov_frag, the 4-row statistics groups), so resident rows sharing a tile or a group with N0
// keep their bytes; the copies are those of the packing kernels run on the N1 rows.  COOP: the
// lane-cooperative statistics (k_seg_prepare_pack0_coop's shapes).  Z16 / Zo / flags may be null.
template <bool COOP>
__global__ __launch_bounds__(64) void k_seg_append(const double* __restrict__ idx, int64_t M, int64_t N0, SegInfo si,
                                                   int all_f32, const uint8_t* __restrict__ row_f32, double* Z,
                                                   double* stats, _Float16* Z16, float* S32, OvLayout o,
                                                   _Float16* Zo, float* So, int* flags) {
  extern __shared__ double xs[];  // L values
  const int lane = threadIdx.x;
  const int64_t N1 = N0 + M, rows = z16_rows(N1);
  const int per = o.nkb * 32;
  for (int64_t row = N0 + blockIdx.x; row < rows; row += gridDim.x) {
    if (row < N1) {
      const int64_t i = row - N0;
      const double* src = idx + i * si.L;
      HQ_GUARD(src, idx, M * si.L - (si.L - 1));
      const bool is32 = row_f32 ? row_f32[i] != 0 : all_f32 != 0;
      for (int k = lane; k < si.L; k += 64) xs[k] = src[k];
      __syncthreads();
      if (COOP) {
        for (int sg = lane >> 3; sg < si.nseg; sg += 8) seg_prepare_coop(xs, row, sg, si, is32, Z, stats, lane & 7);
      } else {
        for (int sg = lane; sg < si.nseg; sg += 64) seg_prepare_one(xs, row, sg, si, is32, Z, stats);
      }
      __threadfence_block();
      __syncthreads();
    }
    if (Z16 && lane < 32) pack0_elem(Z, stats, N1, si.Lp, si.plen[0], si.nseg, Z16, S32, row, lane);
    if (Zo)
      for (int c = lane; c < per; c += 64) packov_elem(Z, stats, N1, si.Lp, o, Zo, So, row, c);
    // lane 0 wrote the row's flag word (pack0_elem, value 0) just above
    if (flags && lane == 0 && row < N1) flag_row(S32, row, flags + 1, flags);
    __syncthreads();
  }
}

// n values of one row, copied by the nl lanes l = 0 .. nl - 1 of a wave: up to four loads per lane issued
// before the first store, so a row of <= 4 nl values costs one round trip
template <typename T>
__device__ __forceinline__ void row_copy_t(T* dst, const T* src, int n, int l, int nl) {
  for (int k0 = l; k0 < n; k0 += 4 * nl) {
    T v[4];
#pragma unroll
    for (int u = 0; u < 4; ++u)
      if (k0 + u * nl < n) v[u] = src[k0 + u * nl];
#pragma unroll
    for (int u = 0; u < 4; ++u)
      if (k0 + u * nl < n) dst[k0 + u * nl] = v[u];
  }
}

// n doubles of one row: 16-byte loads and stores where the row allows them (an even count at 16-byte aligned
// addresses: every Z and statistics row of allocator-aligned buffers, R for even L)
__device__ __forceinline__ void row_copy(double* dst, const double* src, int n, int l, int nl) {
  if (!(n & 1) && !(((uintptr_t)dst | (uintptr_t)src) & 15))
    row_copy_t(reinterpret_cast<f64x2*>(dst), reinterpret_cast<const f64x2*>(src), n >> 1, l, nl);
  else
    row_copy_t(dst, src, n, l, nl);
}

// Selecting M rows of a resident corpus into a second set of buffers (hq_seg_gather), one launch: one wave
// per group of 4 destination rows (a statistics group of the split copies), 16 lanes per row.  The lanes of
// destination row i copy source row src_row[i] (raw values when R is given, Z, statistics: functions of the
// row alone, so nothing is recomputed); then the wave packs its 4 rows as k_seg_append packs one (pack0_elem,
// packov_elem, flag_row, behind the same fence).  The groups past M write the pad rows up to z16_rows(M).
// Four rows per wave keep four rows' loads in flight through the chain row number -> row -> fence -> pack,
// which is latency, not bandwidth (DESIGN.md 4.10).  R / Z16 / Zo / flags may be null.
__global__ __launch_bounds__(64) void k_seg_gather(const int64_t* __restrict__ src_row, int64_t M, int64_t N_src,
                                                   SegInfo si, const double* __restrict__ R_src,
                                                   const double* __restrict__ Z_src,
                                                   const double* __restrict__ S_src, double* R, double* Z,
                                                   double* stats, _Float16* Z16, float* S32, OvLayout o,
                                                   _Float16* Zo, float* So, int* flags, int64_t groups) {
  const int lane = threadIdx.x, rr = lane >> 4, ql = lane & 15;
  const int per = o.nkb * 32, ns4 = si.nseg * 4;
  for (int64_t g = blockIdx.x; g < groups; g += gridDim.x) {
    const int64_t row0 = g * 4, row = row0 + rr;
    if (row0 < M) {  // wave-uniform
      if (row < M) {
        int64_t sr = src_row[row];
#ifdef HQ_DIAG
        sr = diag_bound(sr, N_src, HQ_DIAG_LINE);
#endif
        row_copy(Z + row * si.Lp, Z_src + sr * si.Lp, si.Lp, ql, 16);
        row_copy(stats + row * ns4, S_src + sr * ns4, ns4, ql, 16);
        if (R) row_copy(R + row * si.L, R_src + sr * si.L, si.L, ql, 16);
      }
      __threadfence_block();
      __syncthreads();
    }
    if (Z16)
      for (int t = lane; t < 4 * 32; t += 64) {
        const int64_t r = row0 + (t >> 5);
        pack0_elem(Z, stats, M, si.Lp, si.plen[0], si.nseg, Z16, S32, r, t & 31);
        // this lane wrote the row's flag word (pack0_elem, value 0) just above
        if (flags && (t & 31) == 0 && r < M) flag_row(S32, r, flags + 1, flags);
      }
    if (Zo)
      for (int t = lane; t < 4 * per; t += 64) packov_elem(Z, stats, M, si.Lp, o, Zo, So, row0 + t / per, t % per);
  }
}

// Overwriting M resident rows in place (hq_seg_replace): k_seg_append's steps per row (the segments from an
// LDS copy, then the row's split level-0 and overall copies) for destination row rows[i] of the N resident
// ones.  The layouts address by row, so every other row keeps its bytes; no pad row is written, and the
// flagged-row list is rebuilt by k_flag_rows afterwards (a replaced row may enter or leave it).
template <bool COOP>
__global__ __launch_bounds__(64) void k_seg_replace(const double* __restrict__ idx, int64_t M,
                                                    const int64_t* __restrict__ rows, int64_t N, SegInfo si,
                                                    int all_f32, const uint8_t* __restrict__ row_f32, double* Z,
                                                    double* stats, _Float16* Z16, float* S32, OvLayout o,
                                                    _Float16* Zo, float* So) {
  extern __shared__ double xs[];  // L values
  const int lane = threadIdx.x;
  const int per = o.nkb * 32;
  for (int64_t i = blockIdx.x; i < M; i += gridDim.x) {
    int64_t row = rows[i];
#ifdef HQ_DIAG
    row = diag_bound(row, N, HQ_DIAG_LINE);
#endif
    const double* src = idx + i * si.L;
    const bool is32 = row_f32 ? row_f32[i] != 0 : all_f32 != 0;
    for (int k = lane; k < si.L; k += 64) xs[k] = src[k];
    __syncthreads();
    if (COOP) {
      for (int sg = lane >> 3; sg < si.nseg; sg += 8) seg_prepare_coop(xs, row, sg, si, is32, Z, stats, lane & 7);
    } else {
      for (int sg = lane; sg < si.nseg; sg += 64) seg_prepare_one(xs, row, sg, si, is32, Z, stats);
    }
    __threadfence_block();
    __syncthreads();
    if (Z16 && lane < 32) pack0_elem(Z, stats, N, si.Lp, si.plen[0], si.nseg, Z16, S32, row, lane);
    if (Zo)
      for (int c = lane; c < per; c += 64) packov_elem(Z, stats, N, si.Lp, o, Zo, So, row, c);
    __syncthreads();
  }
}
