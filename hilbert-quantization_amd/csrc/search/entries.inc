// search/entries.inc: part of hq_search.hip (one translation unit: included there last, inside extern "C", after
// `using namespace hq`; no include guard and no #include of its own).
// The exported C entries (include/hq_mi355x.h states their contracts): argument tests, workspace carving and the
// launches, through the launchers above its #include (launch_scan, scan0_run, ov_launch, refine_run,
// empty_lists) or directly for the preparation, dense-score and selection kernels.  Host code only.

int hq_diag_violations(int64_t* count, int* first_line) {
  unsigned long long c = 0;
  int line = 0;
#ifdef HQ_DIAG
  HQ_CHECK_HIP(hipDeviceSynchronize());
  HQ_CHECK_HIP(hipMemcpyFromSymbol(&c, HIP_SYMBOL(g_diag_count), sizeof(c)));
  HQ_CHECK_HIP(hipMemcpyFromSymbol(&line, HIP_SYMBOL(g_diag_line), sizeof(line)));
#endif
  if (count) *count = (int64_t)c;
  if (first_line) *first_line = line;
  return HQ_OK;
}

int hq_scan0_geometry(int Q, int64_t N, int* nqb, int* nchunks, int64_t* chunk_len, int64_t* z_rows,
                      int64_t* s_rows) {
  if (Q <= 0 || N <= 0) return fail(HQ_E_INVALID, "bad shape Q=%d N=%lld", Q, (long long)N);
  int a = 0, b = 0;
  int64_t c = 0;
  scan0_geometry(Q, N, a, b, c);
  if (nqb) *nqb = a;
  if (nchunks) *nchunks = b;
  if (chunk_len) *chunk_len = c;
  if (z_rows) *z_rows = z16_rows(N);
  if (s_rows) *s_rows = pack0_rows(N);
  return HQ_OK;
}

int hq_seg_count(int L) {
  SegInfo si;
  seg_info(L, si);
  return si.nseg;
}

int hq_seg_padded_len(int L) {
  SegInfo si;
  seg_info(L, si);
  return si.Lp;
}

int hq_seg_prepare(const double* idx, int64_t N, int L, double* Z, double* stats, hq_stream_t stream) {
  return hq_seg_prepare_src(idx, N, L, 0, Z, stats, stream);
}

int hq_seg_prepare_src(const double* idx, int64_t N, int L, int src_f32, double* Z, double* stats,
                       hq_stream_t stream) {
  return hq_seg_prepare_rows(idx, N, L, src_f32, nullptr, Z, stats, stream);
}

int hq_seg_prepare_rows(const double* idx, int64_t N, int L, int src_f32, const uint8_t* row_f32, double* Z,
                        double* stats, hq_stream_t stream) {
  if (L <= 0 || N < 0) return fail(HQ_E_INVALID, "bad shape N=%lld L=%d", (long long)N, L);
  if (N == 0) return HQ_OK;
  if (!idx || !Z || !stats) return fail(HQ_E_INVALID, "null buffer");
  SegInfo si;
  seg_info(L, si);
  if (si.nseg == 0) return fail(HQ_E_INVALID, "no level structure for L=%d", L);
  if (N <= 16384 && si.L <= 4096) {
    hipLaunchKernelGGL(k_seg_prepare_lds, dim3((unsigned)N), dim3(64), (size_t)8 * si.L, (hipStream_t)stream, idx, N,
                       si, src_f32 ? 1 : 0, row_f32, Z, stats);
  } else {
    hipLaunchKernelGGL(k_seg_prepare, dim3(grid_for(N * si.nseg, 256, 16384)), dim3(256), 0, (hipStream_t)stream, idx,
                       N, si, src_f32 ? 1 : 0, row_f32, Z, stats);
  }
  HQ_CHECK_LAUNCH();
  return HQ_OK;
}

int hq_level_scores(const double* Rq, const double* Zq, const double* Sq, int Q, const double* Rc, const double* Zc,
                    const double* Sc, int64_t N, int L, int level, double* scores, hq_stream_t stream) {
  if (Q < 0 || N < 0 || L <= 0) return fail(HQ_E_INVALID, "bad shape");
  if (Q == 0 || N == 0) return HQ_OK;
  if (!Rq || !Zq || !Sq || !Rc || !Zc || !Sc || !scores) return fail(HQ_E_INVALID, "null buffer");
  SegInfo si;
  seg_info(L, si);
  if (level >= 0 && level < si.nseg && si.len[level] <= 128 && !opt_on(OPT_LEVEL_SCORES_V1) &&
      (N + kLsTile - 1) / kLsTile < (int64_t(1) << 31) && (Q + kLsQ - 1) / kLsQ < 65536) {
    const size_t lds = (size_t)kLsTile * (si.len[level] | 1) * 8;
    // segments of 65..128 values stage up to 132 KB: above the 64 KB default, so opt in (one block per CU)
    if (lds > 65536)
      HQ_CHECK_HIP(hipFuncSetAttribute((const void*)k_level_scores_lds, hipFuncAttributeMaxDynamicSharedMemorySize,
                                       (int)lds));
    hipLaunchKernelGGL(k_level_scores_lds, dim3((unsigned)((N + kLsTile - 1) / kLsTile), (Q + kLsQ - 1) / kLsQ),
                       dim3(kLsTile), lds, (hipStream_t)stream, VecSet{Rq, Zq, Sq}, Q, VecSet{Rc, Zc, Sc}, N, si, level,
                       scores);
    HQ_CHECK_LAUNCH();
    return HQ_OK;
  }
  auto kern = seg_small(si) ? k_level_scores<true> : k_level_scores<false>;
  hipLaunchKernelGGL(kern, dim3(grid_for((int64_t)Q * N, 256, 16384)), dim3(256), 0, (hipStream_t)stream,
                     VecSet{Rq, Zq, Sq}, Q, VecSet{Rc, Zc, Sc}, N, si, level, scores);
  HQ_CHECK_LAUNCH();
  return HQ_OK;
}

int hq_refine_topk(const double* Rq, const double* Zq, const double* Sq, int Q, const double* Rc, const double* Zc,
                   const double* Sc, int64_t N, int L, int mode, const double* cand_score, const int64_t* cand_id,
                   int kp, int k, double threshold, int thr_mode, double eps, int64_t id_base, double* out_score,
                   int64_t* out_id, int* out_count, int* out_resolved, int count_empty, int* out_redo,
                   hq_stream_t stream) {
  const RefineCall c{{Rq, Zq, Sq}, Q, {Rc, Zc, Sc}, N, L, mode, cand_score, cand_id, kp, k, threshold, thr_mode, eps,
                     id_base, out_score, out_id, out_count, out_resolved, count_empty, out_redo, stream};
  return refine_run(c, 0);
}

int hq_refine_rescore_topk_pp(const double* Rq, const double* Zq, const double* Sq, int Q, const double* Rc,
                              const double* Zc, const double* Sc, int64_t N, int L, int mode,
                              const double* cand_score, const int64_t* cand_id, int kp, int k, double threshold,
                              int thr_mode, double eps, int64_t id_base, double* out_score, int64_t* out_id,
                              int* out_count, int* out_resolved, int count_empty, int* out_redo, int* next_redo,
                              double* out_det, hq_stream_t stream) {
  const RefineCall c{{Rq, Zq, Sq}, Q, {Rc, Zc, Sc}, N, L, mode, cand_score, cand_id, kp, k, threshold, thr_mode, eps,
                     id_base, out_score, out_id, out_count, out_resolved, count_empty, out_redo, stream, out_det,
                     next_redo};
  return refine_run(c, kNeedDet | kNeedCounters);
}

int hq_refine_rescore_topk(const double* Rq, const double* Zq, const double* Sq, int Q, const double* Rc,
                           const double* Zc, const double* Sc, int64_t N, int L, int mode, const double* cand_score,
                           const int64_t* cand_id, int kp, int k, double threshold, int thr_mode, double eps,
                           int64_t id_base, double* out_score, int64_t* out_id, int* out_count, int* out_resolved,
                           int count_empty, int* out_redo, double* out_det, hq_stream_t stream) {
  const RefineCall c{{Rq, Zq, Sq}, Q, {Rc, Zc, Sc}, N, L, mode, cand_score, cand_id, kp, k, threshold, thr_mode, eps,
                     id_base, out_score, out_id, out_count, out_resolved, count_empty, out_redo, stream, out_det};
  return refine_run(c, kNeedDet);
}

size_t hq_refine_workspace_size(int Q, int kp, int L) { return refine_ws_bytes(Q, kp, L); }

int hq_refine_topk_ws(const double* Rq, const double* Zq, const double* Sq, int Q, const double* Rc, const double* Zc,
                      const double* Sc, int64_t N, int L, int mode, const double* cand_score, const int64_t* cand_id,
                      int kp, int k, double threshold, int thr_mode, double eps, int64_t id_base, double* out_score,
                      int64_t* out_id, int* out_count, int* out_resolved, int count_empty, int* out_redo,
                      int* next_redo, double* out_det, void* workspace, size_t workspace_bytes, hq_stream_t stream) {
  const RefineCall c{{Rq, Zq, Sq}, Q, {Rc, Zc, Sc}, N, L, mode, cand_score, cand_id, kp, k, threshold, thr_mode, eps,
                     id_base, out_score, out_id, out_count, out_resolved, count_empty, out_redo, stream, out_det,
                     next_redo, workspace, workspace_bytes};
  return refine_run(c, 0);
}

int hq_refine_final_ws(const double* Rq, const double* Zq, const double* Sq, int Q, const double* Rc, const double* Zc,
                       const double* Sc, int64_t N, int L, const double* cand_score, const int64_t* cand_id, int kp,
                       int k, double threshold, int thr_mode, double eps, int64_t id_base, double* out_score,
                       int64_t* out_id, int* out_count, int* out_resolved, int* out_redo, int* next_redo, int K_out,
                       int64_t* fin_id, double* fin_det, int* fin_count, void* workspace, size_t workspace_bytes,
                       hq_stream_t stream) {
  const FinalOut fin{K_out, fin_id, fin_det, fin_count, 1};
  // mode 0; count_empty on (nothing passed: redo); out_det set (fin_det stands in): records on, the final
  // ranking reads them from the workspace.  out_score / out_id may both be null: the level-0 lists are then
  // not written
  const RefineCall c{{Rq, Zq, Sq}, Q, {Rc, Zc, Sc}, N, L, 0, cand_score, cand_id, kp, k, threshold, thr_mode, eps,
                     id_base, out_score, out_id, out_count, out_resolved, 1, out_redo, stream, fin_det, next_redo,
                     workspace, workspace_bytes, &fin};
  return refine_run(c, kListsOptional);
}

size_t hq_scan_workspace_size(int Q, int64_t N, int k) {
  if (k > kMaxTopK) return scan0_ws_bytes(Q, N, k);  // long lists: the split level-0 scan only
  int nqb, nchunks;
  int64_t chunk_len;
  scan_geometry(Q, N, nqb, nchunks, chunk_len);
  const size_t w1 = (size_t)nchunks * Q * k * 16 + (size_t)nchunks * Q * 16 + 256;
  const size_t w0 = scan0_ws_bytes(Q, N, k);
  return w0 > w1 ? w0 : w1;
}

int hq_scan_topk(const double* Zq, const double* Sq, int Q, const double* Zc, const double* Sc, int64_t N, int L,
                 int mode, int k, double threshold, int thr_mode, int64_t id_base, void* workspace,
                 size_t workspace_bytes, double* out_score, int64_t* out_id, double* out_best,
                 int64_t* out_best_id, hq_stream_t stream) {
  if (Q < 0 || N < 0 || L <= 0) return fail(HQ_E_INVALID, "bad shape");
  if (k <= 0 || k > kMaxTopK) return fail(HQ_E_UNSUPPORTED, "k=%d (1..%d)", k, kMaxTopK);
  if (mode != 0 && mode != 1) return fail(HQ_E_INVALID, "mode %d", mode);
  if (Q == 0) return HQ_OK;
  if (!out_score || !out_id) return fail(HQ_E_INVALID, "null buffer");
  hipStream_t s = (hipStream_t)stream;
  if (N == 0) return empty_lists(out_score, out_id, Q, k, out_best, out_best_id, s);
  if (!Zq || !Sq || !Zc || !Sc || !workspace) return fail(HQ_E_INVALID, "null buffer");
  if (workspace_bytes < hq_scan_workspace_size(Q, N, k)) return fail(HQ_E_INVALID, "workspace too small");
  ScanArgs a;
  a.Zq = Zq; a.Sq = Sq; a.Q = Q; a.Zc = Zc; a.Sc = Sc; a.N = N;
  seg_info(L, a.si);
  const int kp = mode == 0 ? a.si.plen[0] : a.si.Lp;
  a.ks = kp / 4;
  a.nseg_used = mode == 0 ? 1 : a.si.nseg;
  a.rs = rs_for(kp);
  a.K = k;
  a.thr = threshold;
  a.thr_mode = thr_mode;
  a.id_base = id_base;
  scan_geometry(Q, N, a.nqb, a.nchunks, a.chunk_len);
  uint8_t* ws = reinterpret_cast<uint8_t*>(workspace);
  a.ws_score = reinterpret_cast<double*>(ws);
  a.ws_id = reinterpret_cast<int64_t*>(ws + (size_t)a.nchunks * Q * k * 8);
  a.ws_best = reinterpret_cast<double*>(ws + (size_t)a.nchunks * Q * k * 16);
  a.ws_best_id = reinterpret_cast<int64_t*>(ws + (size_t)a.nchunks * Q * k * 16 + (size_t)a.nchunks * Q * 8);
  int rc;
  if (mode == 0) {
    if (a.ks <= 8) rc = launch_scan<8, false>(a, s);
    else if (a.ks <= 16) rc = launch_scan<16, false>(a, s);
    else if (a.ks <= 32) rc = launch_scan<32, false>(a, s);
    else if (a.ks <= 64) rc = launch_scan<64, false>(a, s);
    else return fail(HQ_E_UNSUPPORTED, "level-0 segment too long (%d)", kp);
  } else {
    if (a.ks <= 8) rc = launch_scan<8, true>(a, s);
    else if (a.ks <= 16) rc = launch_scan<16, true>(a, s);
    else if (a.ks <= 32) rc = launch_scan<32, true>(a, s);
    else if (a.ks <= 64) rc = launch_scan<64, true>(a, s);
    else return fail(HQ_E_UNSUPPORTED, "index too long for the fused scan (Lp=%d)", kp);
  }
  if (rc) return rc;
  hipLaunchKernelGGL(k_merge, dim3(query_grid(Q, 4096)), dim3(64), 0, s, a.ws_score, a.ws_id, a.ws_best, a.ws_best_id, a.nchunks, Q,
                     k, out_score, out_id, out_best, out_best_id);
  HQ_CHECK_LAUNCH();
  return HQ_OK;
}

int hq_seg_level0_len(int L) {
  SegInfo si;
  seg_info(L, si);
  return si.nseg > 0 ? si.plen[0] : 0;
}

int hq_seg_prepare_pack0(const double* idx, int64_t N, int L, int src_f32, const uint8_t* row_f32, double* Z,
                         double* stats, void* Z16, float* S32, hq_stream_t stream) {
  if (L <= 0 || N < 0) return fail(HQ_E_INVALID, "bad shape N=%lld L=%d", (long long)N, L);
  if ((N > 0 && (!idx || !Z || !stats)) || !Z16 || !S32) return fail(HQ_E_INVALID, "null buffer");
  SegInfo si;
  seg_info(L, si);
  if (si.nseg == 0) return fail(HQ_E_INVALID, "no level structure for L=%d", L);
  if (si.plen[0] > 32) return fail(HQ_E_UNSUPPORTED, "level-0 segment of %d values (<= 32)", si.plen[0]);
  if (si.L > 4096) return fail(HQ_E_UNSUPPORTED, "L=%d (<= 4096)", L);
  auto kern = prep_coop(si) ? k_seg_prepare_pack0_coop : k_seg_prepare_pack0;
  hipLaunchKernelGGL(kern, dim3(grid_for(z16_rows(N), 1, 65536)), dim3(64), (size_t)8 * si.L, (hipStream_t)stream, idx,
                     N, si, src_f32 ? 1 : 0, row_f32, Z, stats, reinterpret_cast<_Float16*>(Z16), S32);
  HQ_CHECK_LAUNCH();
  return HQ_OK;
}

int hq_seg_pack0_split(const double* Z, const double* S, int64_t N, int L, void* Z16, float* S32,
                       hq_stream_t stream) {
  if (L <= 0 || N < 0) return fail(HQ_E_INVALID, "bad shape N=%lld L=%d", (long long)N, L);
  if ((N > 0 && (!Z || !S)) || !Z16 || !S32) return fail(HQ_E_INVALID, "null buffer");
  SegInfo si;
  seg_info(L, si);
  if (si.nseg == 0) return fail(HQ_E_INVALID, "no level structure for L=%d", L);
  if (si.plen[0] > 32) return fail(HQ_E_UNSUPPORTED, "level-0 segment of %d values (<= 32)", si.plen[0]);
  hipLaunchKernelGGL(k_pack0, dim3(grid_for(z16_rows(N) * 32, 256, 16384)), dim3(256), 0, (hipStream_t)stream, Z, S, N,
                     si.Lp, si.plen[0], si.nseg, reinterpret_cast<_Float16*>(Z16), S32);
  HQ_CHECK_LAUNCH();
  return HQ_OK;
}

int hq_seg_flag_rows(const float* S32, int64_t N, int* flags, hq_stream_t stream) {
  if (N < 0) return fail(HQ_E_INVALID, "bad shape N=%lld", (long long)N);
  if (!flags || (N > 0 && !S32)) return fail(HQ_E_INVALID, "null buffer");
  hipStream_t s = (hipStream_t)stream;
  HQ_CHECK_HIP(hipMemsetAsync(flags, 0, sizeof(int), s));
  if (N == 0) return HQ_OK;
  hipLaunchKernelGGL(k_flag_rows, dim3(grid_for(N, 256, 4096)), dim3(256), 0, s, S32, N, flags + 1, flags);
  HQ_CHECK_LAUNCH();
  return HQ_OK;
}

int hq_scan0_topk_split(const void* Zq16, const float* Sq32, const double* Sq, int Q, const void* Zc16,
                        const float* Sc32, const double* Sc, int64_t N, int L, int k, double threshold, int thr_mode,
                        int64_t id_base, void* workspace, size_t workspace_bytes, double* out_score,
                        int64_t* out_id, hq_stream_t stream) {
  return hq_scan0_topk_split_fl(Zq16, Sq32, Sq, Q, Zc16, Sc32, Sc, N, L, k, threshold, thr_mode, id_base, workspace,
                                workspace_bytes, out_score, out_id, nullptr, stream);
}

int hq_scan0_topk_split_fl(const void* Zq16, const float* Sq32, const double* Sq, int Q, const void* Zc16,
                           const float* Sc32, const double* Sc, int64_t N, int L, int k, double threshold,
                           int thr_mode, int64_t id_base, void* workspace, size_t workspace_bytes, double* out_score,
                           int64_t* out_id, const int* corpus_flags, hq_stream_t stream) {
  if (Q < 0 || N < 0 || L <= 0) return fail(HQ_E_INVALID, "bad shape");
  if (k <= 0 || k > kMaxTopKBig) return fail(HQ_E_UNSUPPORTED, "k=%d (1..%d)", k, kMaxTopKBig);
  if (Q == 0) return HQ_OK;
  if (!out_score || !out_id) return fail(HQ_E_INVALID, "null buffer");
  hipStream_t s = (hipStream_t)stream;
  if (N == 0) return empty_lists(out_score, out_id, Q, k, nullptr, nullptr, s);
  if (N >= 0x7FFFFFFF) return fail(HQ_E_UNSUPPORTED, "N=%lld rows (int32 row ids)", (long long)N);
  if (!Zq16 || !Sq32 || !Sq || !Zc16 || !Sc32 || !Sc || !workspace) return fail(HQ_E_INVALID, "null buffer");
  if (workspace_bytes < hq_scan_workspace_size(Q, N, k)) return fail(HQ_E_INVALID, "workspace too small");
  SegInfo si;
  seg_info(L, si);
  const int ks = si.nseg > 0 ? si.plen[0] / 4 : 0;
  if (ks < 1 || ks > 8) return fail(HQ_E_UNSUPPORTED, "level-0 segment of %d values (1..32)", si.plen[0]);
  return scan0_run(Sq, reinterpret_cast<const _Float16*>(Zq16), Sq32, Q, Sc, reinterpret_cast<const _Float16*>(Zc16),
                   Sc32, N, si, k, threshold, thr_mode, id_base, workspace, out_score, out_id, s, corpus_flags);
}

int hq_rescore(const double* Rq, const double* Zq, const double* Sq, int Q, const double* Rc, const double* Zc,
               const double* Sc, int64_t N, int L, const int64_t* ids, int k, int64_t id_base, double* out,
               hq_stream_t stream) {
  if (Q < 0 || N < 0 || L <= 0 || k < 0) return fail(HQ_E_INVALID, "bad shape");
  if (Q == 0 || k == 0) return HQ_OK;
  if (!Rq || !Zq || !Sq || !ids || !out || (N > 0 && (!Rc || !Zc || !Sc))) return fail(HQ_E_INVALID, "null buffer");
  SegInfo si;
  seg_info(L, si);
  const int64_t total = (int64_t)Q * k;
  const int G = si.nseg <= 8 ? 8 : 16;
  const bool sm = seg_small(si);
  auto kern = G == 8 ? (sm ? k_rescore<8, true> : k_rescore<8, false>) : (sm ? k_rescore<16, true> : k_rescore<16, false>);
  hipLaunchKernelGGL(kern, dim3(grid_for(total * G, 256, 16384)), dim3(256), 0, (hipStream_t)stream, VecSet{Rq, Zq, Sq},
                     Q, VecSet{Rc, Zc, Sc}, N, si, ids, k, id_base, out);
  HQ_CHECK_LAUNCH();
  return HQ_OK;
}

int hq_progressive_final(int R, int Q, int M, int nseg, const double* s0, const int64_t* ids, const double* det,
                         const double* best, const int64_t* best_id, const double* best_det, int K,
                         int64_t* out_id, double* out_det, int* out_count, hq_stream_t stream) {
  return hq_progressive_final_ex(R, Q, M, nseg, s0, ids, det, best, best_id, best_det, K, out_id, out_det, out_count,
                                 0, stream);
}

int hq_progressive_final_ex(int R, int Q, int M, int nseg, const double* s0, const int64_t* ids, const double* det,
                            const double* best, const int64_t* best_id, const double* best_det, int K,
                            int64_t* out_id, double* out_det, int* out_count, int flags, hq_stream_t stream) {
  if (R <= 0 || R > 16 || Q < 0 || M <= 0 || M > kMaxTopKBig || K <= 0 || nseg < 0 || nseg >= kMaxSeg)
    return fail(HQ_E_INVALID, "bad sizes R=%d Q=%d M=%d K=%d", R, Q, M, K);
  if (Q == 0) return HQ_OK;
  if (!s0 || !ids || !det || !best || !best_id || !best_det || !out_id || !out_det || !out_count)
    return fail(HQ_E_INVALID, "null buffer");
  const int W = 1 + nseg;
  const int grid = query_grid(Q);
  if (M <= kMaxTopK)
    hipLaunchKernelGGL(k_progressive_final, dim3(grid), dim3(64), 0, (hipStream_t)stream, R, Q, M, W, s0, ids, det,
                       best, best_id, best_det, K, out_id, out_det, out_count, flags);
  else
    hipLaunchKernelGGL(k_progressive_final_big, dim3(grid), dim3(256), 0, (hipStream_t)stream, R, Q, M, W, s0, ids,
                       det, best, best_id, best_det, K, out_id, out_det, out_count,
                       flags & 1);
  HQ_CHECK_LAUNCH();
  return HQ_OK;
}

// parts of the two-stage select: ~8192 entries each, <= 1024 per query
static void select_parts(int Q, int64_t N, int& P, int64_t& plen) {
  int64_t p = (N + 8191) / 8192;
  if (p > 1024) p = 1024;
  if (p < 1) p = 1;
  P = (int)p;
  plen = (N + P - 1) / P;
}

// the register-resident multi-stage select runs when the two-stage form would have few waves
static bool select_reg_ok(int Q, int64_t N, int k) {
  return N > 0 && k >= 16 && k <= 64 && (int64_t)Q * ((N + 8191) / 8192) < 4096 && !opt_on(OPT_SELECT_2STAGE);
}
static int64_t select_reg_parts(int64_t N) { return (N + kRegSel - 1) / kRegSel; }

// the sort-based select (k > 64): stage-1 parts of the row and their ping-pong stage buffers
static bool select_sort_ok(int64_t N, int k) {
  return N > 0 && k > kMaxTopK && k <= kSortPart / 4 && !opt_on(OPT_SELECT_2STAGE);
}
static int64_t select_sort_parts(int64_t N) { return (N + kSortPart - 1) / kSortPart; }

size_t hq_select_workspace_size(int Q, int64_t N, int k) {
  if (Q <= 0 || N <= 0 || k <= 0) return 0;
  if (select_sort_ok(N, k)) {  // two k-list stage buffers + the stage-1 arg-maxes
    const size_t P1 = (size_t)select_sort_parts(N);
    return 2 * (size_t)Q * P1 * k * 16 + (size_t)Q * P1 * 16 + 512;
  }
  int P;
  int64_t plen;
  select_parts(Q, N, P, plen);
  size_t two = (size_t)Q * P * ((size_t)k + 1) * 16 + 256;
  if (select_reg_ok(Q, N, k)) {  // two ping-pong stage buffers of the stage-1 size
    const size_t reg = 2 * (size_t)Q * select_reg_parts(N) * ((size_t)k + 1) * 16 + 256;
    if (reg > two) two = reg;
  }
  return two;
}

int hq_select_topk_ws(const double* scores, int Q, int64_t N, int k, double threshold, int thr_mode,
                      int64_t id_base, void* workspace, size_t workspace_bytes, double* out_score, int64_t* out_id,
                      double* out_best, int64_t* out_best_id, hq_stream_t stream) {
  if (Q < 0 || N < 0 || k <= 0) return fail(HQ_E_INVALID, "bad shape");
  if (Q == 0) return HQ_OK;
  if (workspace && out_score && out_id && scores && select_sort_ok(N, k)) {
    if (workspace_bytes < hq_select_workspace_size(Q, N, k)) return fail(HQ_E_INVALID, "workspace too small");
    const hipStream_t s = (hipStream_t)stream;
    const int64_t P1 = select_sort_parts(N);
    const size_t cap = (size_t)Q * P1 * k;
    uint8_t* w = reinterpret_cast<uint8_t*>(workspace);
    double* bs[2] = {reinterpret_cast<double*>(w), reinterpret_cast<double*>(w + cap * 16)};
    int64_t* bi[2] = {reinterpret_cast<int64_t*>(w + cap * 8), reinterpret_cast<int64_t*>(w + cap * 24)};
    double* pb = reinterpret_cast<double*>(w + cap * 32);
    int64_t* pbi = reinterpret_cast<int64_t*>(w + cap * 32 + (size_t)Q * P1 * 8);
    // stage 1: parts of the row (the arg-maxes per part, or straight to the outputs when one part)
    const int64_t part1 = (N + P1 - 1) / P1;
    bool last = P1 == 1;
    hipLaunchKernelGGL(k_select_sort, dim3(grid_for(Q * P1, 1, 65536)), dim3(512), 0, s, scores,
                       (const int64_t*)nullptr, Q, N, part1,
                       (int)P1, k, threshold, thr_mode, last ? 1 : 0, id_base, last ? out_score : bs[0],
                       last ? out_id : bi[0], last ? out_best : pb, last ? out_best_id : pbi, (const double*)nullptr,
                       (const int64_t*)nullptr, 0);
    HQ_CHECK_LAUNCH();
    int64_t P = P1;
    int cur = 0;
    const int64_t F = kSortPart / k;  // k-lists merged per part (>= 4)
    while (P > 1) {
      const int64_t P2 = (P + F - 1) / F;
      last = P2 == 1;
      hipLaunchKernelGGL(k_select_sort, dim3(grid_for(Q * P2, 1, 65536)), dim3(512), 0, s, (const double*)bs[cur],
                         (const int64_t*)bi[cur], Q, P * k, F * k, (int)P2, k, threshold, thr_mode, last ? 1 : 0,
                         id_base, last ? out_score : bs[cur ^ 1], last ? out_id : bi[cur ^ 1],
                         last ? out_best : (double*)nullptr, last ? out_best_id : (int64_t*)nullptr,
                         (const double*)pb, (const int64_t*)pbi, (int)P1);
      HQ_CHECK_LAUNCH();
      P = P2;
      cur ^= 1;
    }
    return HQ_OK;
  }
  int P;
  int64_t plen;
  select_parts(Q, N, P, plen);
  if (workspace && out_score && out_id && scores && select_reg_ok(Q, N, k) && P > 1) {
    if (workspace_bytes < hq_select_workspace_size(Q, N, k)) return fail(HQ_E_INVALID, "workspace too small");
    const hipStream_t s = (hipStream_t)stream;
    const int64_t P1 = select_reg_parts(N);
    const int F = kRegSel / k < 64 ? kRegSel / k : 64;  // fan-in: F k <= kRegSel candidates, F <= 64 arg-maxes
    const size_t cap = (size_t)Q * P1;                   // parts a stage buffer holds
    uint8_t* w = reinterpret_cast<uint8_t*>(workspace);
    auto region = [&](int r, double*& rs, int64_t*& ri, double*& rb, int64_t*& rbi) {
      uint8_t* b = w + (size_t)r * cap * ((size_t)k + 1) * 16;
      rs = reinterpret_cast<double*>(b);
      ri = reinterpret_cast<int64_t*>(b + cap * k * 8);
      rb = reinterpret_cast<double*>(b + cap * k * 16);
      rbi = reinterpret_cast<int64_t*>(b + cap * k * 16 + cap * 8);
    };
    double *as, *bs_, *ab, *bb;
    int64_t *ai, *bi, *abi, *bbi;
    region(0, as, ai, ab, abi);
    region(1, bs_, bi, bb, bbi);
    // every stage keeps the arg-maxes (the final one writes them only when requested)
    int64_t P = P1;
    const bool last1 = P == 1;
    hipLaunchKernelGGL(k_select_reg1, dim3(grid_for(Q * P, 1, 65536)), dim3(64), 0, s, scores, Q, N, (int)P, k,
                       threshold, thr_mode,
                       last1 ? id_base : 0, last1 ? out_score : as, last1 ? out_id : ai, last1 ? out_best : ab,
                       last1 ? out_best_id : abi);
    HQ_CHECK_LAUNCH();
    int cur = 0;
    while (P > 1) {
      const int64_t P2 = (P + F - 1) / F;
      const bool last = P2 == 1;
      double *is_, *ib, *os_, *ob;
      int64_t *ii, *ibi, *oi, *obi;
      if (cur == 0) { is_ = as; ii = ai; ib = ab; ibi = abi; os_ = bs_; oi = bi; ob = bb; obi = bbi; }
      else { is_ = bs_; ii = bi; ib = bb; ibi = bbi; os_ = as; oi = ai; ob = ab; obi = abi; }
      hipLaunchKernelGGL(k_select_regm, dim3(grid_for(Q * P2, 1, 65536)), dim3(64), 0, s, Q, (int)P, F, (int)P2, k,
                         last ? id_base : 0, (const double*)is_, (const int64_t*)ii, (const double*)ib,
                         (const int64_t*)ibi, last ? out_score : os_, last ? out_id : oi, last ? out_best : ob,
                         last ? out_best_id : obi);
      HQ_CHECK_LAUNCH();
      P = P2;
      cur ^= 1;
    }
    return HQ_OK;
  }
  if (P == 1 || !workspace)
    return hq_select_topk(scores, Q, N, k, threshold, thr_mode, id_base, out_score, out_id, out_best, out_best_id,
                          stream);
  if (!out_score || !out_id || !scores) return fail(HQ_E_INVALID, "null buffer");
  if (workspace_bytes < hq_select_workspace_size(Q, N, k)) return fail(HQ_E_INVALID, "workspace too small");
  uint8_t* ws = reinterpret_cast<uint8_t*>(workspace);
  const size_t nk = (size_t)Q * P * k;
  double* ws_s = reinterpret_cast<double*>(ws);
  int64_t* ws_id = reinterpret_cast<int64_t*>(ws + nk * 8);
  double* ws_b = reinterpret_cast<double*>(ws + nk * 16);
  int64_t* ws_bid = reinterpret_cast<int64_t*>(ws + nk * 16 + (size_t)Q * P * 8);
  hipLaunchKernelGGL(k_select_part, dim3(grid_for((int64_t)Q * P, 1, 65536)), dim3(64), 0, (hipStream_t)stream, scores,
                     Q, N, P, plen, k, threshold, thr_mode, ws_s, ws_id, ws_b, ws_bid);
  HQ_CHECK_LAUNCH();
  hipLaunchKernelGGL(k_select_merge, dim3(query_grid(Q, 4096)), dim3(64), 0, (hipStream_t)stream, Q, P, k, threshold, thr_mode, id_base,
                     (const double*)ws_s, (const int64_t*)ws_id, (const double*)ws_b, (const int64_t*)ws_bid,
                     out_score, out_id, out_best, out_best_id);
  HQ_CHECK_LAUNCH();
  return HQ_OK;
}

int hq_select_topk(const double* scores, int Q, int64_t N, int k, double threshold, int thr_mode, int64_t id_base,
                   double* out_score, int64_t* out_id, double* out_best, int64_t* out_best_id, hq_stream_t stream) {
  if (Q < 0 || N < 0 || k <= 0) return fail(HQ_E_INVALID, "bad shape");
  if (Q == 0) return HQ_OK;
  if (!out_score || !out_id || (N > 0 && !scores)) return fail(HQ_E_INVALID, "null buffer");
  hipLaunchKernelGGL(k_select, dim3(query_grid(Q, 4096)), dim3(64), 0, (hipStream_t)stream, scores, Q, N, k, threshold, thr_mode,
                     id_base, out_score, out_id, out_best, out_best_id);
  HQ_CHECK_LAUNCH();
  return HQ_OK;
}

int hq_pair_scores_raw(const double* q, const double* C, int64_t N, int m, double* out, hq_stream_t stream) {
  return hq_pair_scores_raw_src(q, C, N, m, 0, 0, out, stream);
}

int hq_pair_scores_raw_src(const double* q, const double* C, int64_t N, int m, int q_f32, int c_f32, double* out,
                           hq_stream_t stream) {
  if (N < 0 || m <= 0) return fail(HQ_E_INVALID, "bad shape");
  if (N == 0) return HQ_OK;
  if (!q || !C || !out) return fail(HQ_E_INVALID, "null buffer");
  hipLaunchKernelGGL(k_pair_raw, dim3(grid_for(N, 256, 8192)), dim3(256), 0, (hipStream_t)stream, q, C, N, m,
                     q_f32 ? 1 : 0, c_f32 ? 1 : 0, out);
  HQ_CHECK_LAUNCH();
  return HQ_OK;
}

int hq_cosine_scores(const float* a, int Q, const float* b, int64_t N, int K, double* out, hq_stream_t stream) {
  if (Q < 0 || N < 0 || K < 0) return fail(HQ_E_INVALID, "bad shape");
  if (Q == 0 || N == 0) return HQ_OK;
  if ((K > 0 && (!a || !b)) || !out) return fail(HQ_E_INVALID, "null buffer");  // K = 0: rows are never read
  hipLaunchKernelGGL(k_cosine, dim3(grid_for((int64_t)Q * N, 256, 16384)), dim3(256), 0, (hipStream_t)stream, a, Q, b,
                     N, K, out);
  HQ_CHECK_LAUNCH();
  return HQ_OK;
}


/* ---- overall-mode scan (split-f16 copies of every level segment) ------------------------------ */
int hq_seg_packov_info(int L, int* nkb, int* ng, int* nc, int* group_floats) {
  OvLayout o;
  if (L <= 0 || !ov_layout(L, o)) return fail(HQ_E_UNSUPPORTED, "no split overall layout for L=%d", L);
  if (nkb) *nkb = o.nkb;
  if (ng) *ng = o.ng;
  if (nc) *nc = o.nc;
  if (group_floats) *group_floats = ov_gsize(o.ng, o.nc);
  return HQ_OK;
}

int hq_seg_packov_split(const double* Z, const double* S, int64_t N, int L, void* Zo16, float* So32,
                        hq_stream_t stream) {
  if (L <= 0 || N < 0) return fail(HQ_E_INVALID, "bad shape N=%lld L=%d", (long long)N, L);
  if ((N > 0 && (!Z || !S)) || !Zo16 || !So32) return fail(HQ_E_INVALID, "null buffer");
  if (N >= 0x7FFFFFFF) return fail(HQ_E_UNSUPPORTED, "N=%lld rows (int32 row ids)", (long long)N);
  OvLayout o;
  if (!ov_layout(L, o)) return fail(HQ_E_UNSUPPORTED, "no split overall layout for L=%d", L);
  SegInfo si;
  seg_info(L, si);
  hipLaunchKernelGGL(k_packov, dim3(grid_for(z16_rows(N) * o.nkb * 32, 256, 16384)), dim3(256), 0, (hipStream_t)stream,
                     Z, S, N, si.Lp, o, reinterpret_cast<_Float16*>(Zo16), So32);
  HQ_CHECK_LAUNCH();
  return HQ_OK;
}

int hq_seg_append(const double* idx, int64_t M, int L, int src_f32, const uint8_t* row_f32, int64_t N0, double* Z,
                  double* stats, void* Z16, float* S32, void* Zov16, float* Sov32, int* flags, hq_stream_t stream) {
  if (L <= 0 || M < 0 || N0 < 0) return fail(HQ_E_INVALID, "bad shape N0=%lld M=%lld L=%d", (long long)N0, (long long)M, L);
  if (L > 4096) return fail(HQ_E_UNSUPPORTED, "L=%d (<= 4096)", L);
  if (M == 0) return HQ_OK;
  if (!idx || !Z || !stats) return fail(HQ_E_INVALID, "null buffer");
  const SplitCopies c = split_copies(Z16, S32, Zov16, Sov32, flags);
  if (int rc = split_copies_paired(c)) return rc;
  if (N0 + M >= 0x7FFFFFFF) return fail(HQ_E_UNSUPPORTED, "N=%lld rows (int32 row ids)", (long long)(N0 + M));
  SegInfo si;
  OvLayout o;
  if (int rc = split_copies_check(L, c, si, o)) return rc;
  hipStream_t s = (hipStream_t)stream;
  if (flags && N0 == 0) HQ_CHECK_HIP(hipMemsetAsync(flags, 0, sizeof(int), s));  // an empty corpus lists no rows
  // one workgroup per new row, then per pad row
  auto kern = prep_coop(si) ? k_seg_append<true> : k_seg_append<false>;
  hipLaunchKernelGGL(kern, dim3(grid_for(z16_rows(N0 + M) - N0, 1, 65536)), dim3(64), (size_t)8 * si.L, s, idx, M, N0,
                     si, src_f32 ? 1 : 0, row_f32, Z, stats, c.Z16, c.S32, o, c.Zov16, c.Sov32, c.flags);
  HQ_CHECK_LAUNCH();
  return HQ_OK;
}

int hq_seg_gather(const int64_t* src_row, int64_t M, int64_t N_src, int L, const double* R_src, const double* Z_src,
                  const double* S_src, double* R, double* Z, double* stats, void* Z16, float* S32, void* Zov16,
                  float* Sov32, int* flags, hq_stream_t stream) {
  if (L <= 0 || M < 0 || N_src < 0 || (M > 0 && N_src == 0))
    return fail(HQ_E_INVALID, "bad shape N_src=%lld M=%lld L=%d", (long long)N_src, (long long)M, L);
  if (M >= 0x7FFFFFFF) return fail(HQ_E_UNSUPPORTED, "M=%lld rows (int32 row ids)", (long long)M);
  if (M > 0 && (!src_row || !Z_src || !S_src || !Z || !stats)) return fail(HQ_E_INVALID, "null buffer");
  if ((R_src == nullptr) != (R == nullptr)) return fail(HQ_E_INVALID, "the raw rows need both of their buffers");
  const SplitCopies c = split_copies(Z16, S32, Zov16, Sov32, flags);
  if (int rc = split_copies_paired(c)) return rc;
  SegInfo si;
  OvLayout o;
  if (int rc = split_copies_check(L, c, si, o)) return rc;
  if ((R && R == R_src) || (Z && Z == Z_src) || (stats && stats == S_src))
    return fail(HQ_E_INVALID, "a destination buffer is its source");
  hipStream_t s = (hipStream_t)stream;
  if (flags) HQ_CHECK_HIP(hipMemsetAsync(flags, 0, sizeof(int), s));
  // groups of 4 rows: the selected rows, then the pad rows of the copies (z16_rows is a multiple of 16)
  const int64_t groups = ((Z16 || Zov16) ? z16_rows(M) : M + 3) / 4;
  if (groups == 0) return HQ_OK;
  // one wave per group, dispatched by the hardware (a grid-stride loop only past 2^22 groups)
  hipLaunchKernelGGL(k_seg_gather, dim3(grid_for(groups, 1, 1 << 22)), dim3(64), 0, s, src_row, M, N_src, si, R_src,
                     Z_src, S_src, R, Z, stats, c.Z16, c.S32, o, c.Zov16, c.Sov32, c.flags, groups);
  HQ_CHECK_LAUNCH();
  return HQ_OK;
}

int hq_seg_replace(const double* idx, int64_t M, const int64_t* rows, int L, int src_f32, const uint8_t* row_f32,
                   int64_t N, double* Z, double* stats, void* Z16, float* S32, void* Zov16, float* Sov32, int* flags,
                   hq_stream_t stream) {
  if (L <= 0 || M < 0 || N < 0 || M > N) return fail(HQ_E_INVALID, "bad shape N=%lld M=%lld L=%d", (long long)N, (long long)M, L);
  if (L > 4096) return fail(HQ_E_UNSUPPORTED, "L=%d (<= 4096)", L);
  if (M == 0) return HQ_OK;
  if (!idx || !rows || !Z || !stats) return fail(HQ_E_INVALID, "null buffer");
  const SplitCopies c = split_copies(Z16, S32, Zov16, Sov32, flags);
  if (int rc = split_copies_paired(c)) return rc;
  if (N >= 0x7FFFFFFF) return fail(HQ_E_UNSUPPORTED, "N=%lld rows (int32 row ids)", (long long)N);
  SegInfo si;
  OvLayout o;
  if (int rc = split_copies_check(L, c, si, o)) return rc;
  hipStream_t s = (hipStream_t)stream;
  auto kern = prep_coop(si) ? k_seg_replace<true> : k_seg_replace<false>;
  hipLaunchKernelGGL(kern, dim3(grid_for(M, 1, 65536)), dim3(64), (size_t)8 * si.L, s, idx, M, rows, N, si,
                     src_f32 ? 1 : 0, row_f32, Z, stats, c.Z16, c.S32, o, c.Zov16, c.Sov32);
  HQ_CHECK_LAUNCH();
  // a replaced row may enter or leave the list: listed again from the N rows' flag words
  if (flags) return hq_seg_flag_rows(S32, N, flags, stream);
  return HQ_OK;
}

size_t hq_scanov_workspace_size(int Q, int64_t N, int k) {
  if (Q <= 0 || N <= 0 || k <= 0) return 256;
  return ov_plan(Q, N, k).total;
}

int hq_scanov_topk_split(const void* Zq16, const float* Sq32, const double* Sq, const double* Zq, int Q,
                         const void* Zc16, const float* Sc32, const double* Sc, const double* Zc, int64_t N, int L,
                         int k, double threshold, int thr_mode, int64_t id_base, void* workspace,
                         size_t workspace_bytes, double* out_score, int64_t* out_id, hq_stream_t stream) {
  if (Q < 0 || N < 0 || L <= 0) return fail(HQ_E_INVALID, "bad shape");
  if (k <= 0 || k > kMaxTopKBig) return fail(HQ_E_UNSUPPORTED, "k=%d (1..%d)", k, kMaxTopKBig);
  if (Q == 0) return HQ_OK;
  if (!out_score || !out_id) return fail(HQ_E_INVALID, "null buffer");
  hipStream_t s = (hipStream_t)stream;
  if (N == 0) return empty_lists(out_score, out_id, Q, k, nullptr, nullptr, s);
  if (N >= 0x7FFFFFFF) return fail(HQ_E_UNSUPPORTED, "N=%lld rows (int32 row ids)", (long long)N);
  if (!Zq16 || !Sq32 || !Sq || !Zq || !Zc16 || !Sc32 || !Sc || !Zc || !workspace) return fail(HQ_E_INVALID, "null buffer");
  if (workspace_bytes < hq_scanov_workspace_size(Q, N, k)) return fail(HQ_E_INVALID, "workspace too small");
  OvArgs a;
  if (!ov_layout(L, a.o)) return fail(HQ_E_UNSUPPORTED, "no split overall layout for L=%d", L);
  SegInfo si;
  seg_info(L, si);
  const OvPlan p = ov_plan(Q, N, k);
  a.Zq = reinterpret_cast<const _Float16*>(Zq16); a.Sq32 = Sq32; a.Sq = Sq; a.Q = Q;
  a.Zc = reinterpret_cast<const _Float16*>(Zc16); a.Sc32 = Sc32; a.Sc = Sc; a.N = N;
  a.Zq64 = Zq; a.Zc64 = Zc; a.Lp = si.Lp;
  a.nqb = p.nqb; a.nchunks = p.nchunks; a.chunk_len = p.chunk_len;
  a.stride = p.stride; a.S = p.S; a.top = nullptr; a.qc = nullptr;
  const int sample_kth = scan_kprime(k, p.stride);
  const double thr0 = thr_mode == 0 ? -__builtin_huge_val() : threshold;
  uint8_t* ws = reinterpret_cast<uint8_t*>(workspace);
  if (a.o.lid == 0) return ov_launch<0>(a, p, si, k, thr0, sample_kth, id_base, ws, out_score, out_id, s);
  return ov_launch<1>(a, p, si, k, thr0, sample_kth, id_base, ws, out_score, out_id, s);
}
