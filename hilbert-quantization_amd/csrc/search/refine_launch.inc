// search/refine_launch.inc: part of hq_search.hip (one translation unit: included there, inside namespace hq, after
// launch_scan; no include guard and no #include of its own).
// The host side of the exact re-rank: RefineCall (what the five hq_refine_* entries pass on), refine_check (their
// argument tests), refine_launch (which kernel a list length and an index length get) and refine_run.  Host code
// only; the reference has no counterpart.
// Uses, from the text above its #include: SegInfo, seg_info, VecSet, kMaxTopK, kMaxTopKBig, the k_refine*,
// k_refine_big* and k_rank_* kernels, RankArgs, FinalOut, seg_small, coop_ppl, coop_lid, refine_ws_bytes, query_grid.

// One exact re-rank call: what the five hq_refine_* entries pass on.  The entries' optional arguments are
// null / 0 where an entry has none.
struct RefineCall {
  VecSet q; int Q;
  VecSet c; int64_t N;
  int L, mode;
  const double* cand_score; const int64_t* cand_id; int kp, k;
  double threshold; int thr_mode; double eps; int64_t id_base;
  double* out_score; int64_t* out_id; int* out_count; int* out_resolved;
  int count_empty; int* out_redo;
  hq_stream_t stream;
  double* out_det = nullptr;
  int* next_redo = nullptr;
  void* workspace = nullptr; size_t workspace_bytes = 0;
  const FinalOut* fin = nullptr;  // hq_refine_final_ws: the fused final ranking
};

// what an entry requires beyond the common buffers
enum : unsigned {
  kNeedDet = 1,       // out_det
  kNeedCounters = 2,  // out_redo and next_redo
  kListsOptional = 4  // out_score and out_id may both be null
};

// The entries' argument tests, in their order: sizes, (fused final ranking: a cooperative shape), Q = 0, null
// buffers, workspace size.  HQ_OK with Q = 0: nothing is to be launched.
static int refine_check(const RefineCall& c, unsigned need) {
  const bool bad = c.Q < 0 || c.N < 0 || c.L <= 0 || c.kp <= 0 || c.kp > kMaxTopKBig || c.k <= 0 || c.k > c.kp;
  if (c.fin) {
    if (bad || c.fin->K <= 0) return fail(HQ_E_INVALID, "bad sizes kp=%d k=%d K=%d", c.kp, c.k, c.fin->K);
  } else if (bad) {
    return fail(HQ_E_INVALID, "bad sizes kp=%d k=%d", c.kp, c.k);
  }
  bool ws = c.workspace != nullptr;  // whether the workspace is used, so its size tested
  if (c.fin) {
    SegInfo si;
    seg_info(c.L, si);
    // the fused form exists on the lane-cooperative paths only (k_rank_small for lists <= 64, k_rank_pairs +
    // k_rank_sort above; the caller keeps the two-step form otherwise: hq_refine_topk_ws + hq_progressive_final_ex)
    const bool small = c.kp <= kMaxTopK && coop_ppl(si) && opt(OPT_REFINE_SMALL, 1) != 0;
    ws = c.kp > kMaxTopK && coop_ppl(si) && opt(OPT_REFINE_COOP, 1) != 0 && c.Q <= 65535;
    if (!small && !ws) return fail(HQ_E_UNSUPPORTED, "fused final ranking: kp=%d L=%d", c.kp, c.L);
  }
  if (c.Q == 0) {  // no kernel runs: the next batch's counter is still cleared
    if (c.next_redo) HQ_CHECK_HIP(hipMemsetAsync(c.next_redo, 0, sizeof(int), (hipStream_t)c.stream));
    return HQ_OK;
  }
  const bool lists = (need & kListsOptional) ? !c.out_score == !c.out_id : c.out_score && c.out_id;
  if (!c.q.raw || !c.q.Z || !c.q.S || !c.cand_score || !c.cand_id || !lists || !c.out_count || !c.out_resolved ||
      ((need & kNeedDet) && !c.out_det) || ((need & kNeedCounters) && (!c.out_redo || !c.next_redo)) ||
      (c.next_redo && (!c.out_redo || c.out_redo == c.next_redo)) ||
      (c.fin && (!c.fin->id || !c.fin->det || !c.fin->count)) || (ws && !c.workspace) ||
      (c.N > 0 && (!c.c.raw || !c.c.Z || !c.c.S)))
    return fail(HQ_E_INVALID, "null buffer");
  if (ws && c.workspace_bytes < refine_ws_bytes(c.Q, c.kp, c.L)) return fail(HQ_E_INVALID, "workspace too small");
  return HQ_OK;
}

// exact re-rank launcher: the LDS-staged kernel when the staged rows fit (<= 96 KiB), else k_refine
// (which has no re-score output: odet then takes hq_rescore's kernel afterwards)
static int refine_launch(const RefineCall& c) {
  SegInfo si;
  seg_info(c.L, si);
  const hipStream_t s = (hipStream_t)c.stream;
  const int Q = c.Q, kp = c.kp;
  const dim3 grid(query_grid(Q));
  const int ce = c.count_empty ? 1 : 0;
  // next_redo (hq_refine_rescore_topk_pp): out_redo arrives zeroed (cleared by the previous batch's kernel),
  // the kernel clears next_redo for the next batch; otherwise one 4-byte memset here
  if (c.out_redo && !c.next_redo) HQ_CHECK_HIP(hipMemsetAsync(c.out_redo, 0, sizeof(int), s));
  const bool sm = seg_small(si);
  auto rank_args = [&]() {
    RankArgs ra;
    ra.Rq = c.q.raw; ra.Zq = c.q.Z; ra.Sq = c.q.S; ra.Q = Q; ra.Rc = c.c.raw; ra.Sc = c.c.S; ra.N = c.N;
    ra.cs.nseg = si.nseg; ra.cs.L = si.L; ra.cs.Lp = si.Lp;
    for (int i = 0; i < kCoopMaxW - 1; ++i) {
      ra.cs.src[i] = i < si.nseg ? si.src[i] : 0;
      ra.cs.len[i] = i < si.nseg ? si.len[i] : 0;
      ra.cs.poff[i] = i < si.nseg ? si.poff[i] : 0;
    }
    ra.mode = c.mode; ra.kp = kp; ra.k = c.k; ra.thr_mode = c.thr_mode; ra.det = c.out_det ? 1 : 0;
    ra.thr = c.threshold; ra.id_base = c.id_base; ra.cid = c.cand_id;
    ra.ws_sc = nullptr; ra.ws_id = nullptr; ra.ws_rec = nullptr;
    ra.win = (int)opt(OPT_RANK_WIN, 1);
    return ra;
  };
  // the cooperative kernels' final ranking (hq_refine_final_ws) writes the records itself
  const FinalOut fo = c.fin ? *c.fin : FinalOut{0, nullptr, nullptr, nullptr, 0};
  double* odet = c.fin ? nullptr : c.out_det;
  // short lists: the fused lane-cooperative re-rank (k_rank_small) where its shapes hold; option
  // refine_small = 0 keeps k_refine_lds below (A/B, parity)
  if (kp <= kMaxTopK && coop_ppl(si) && opt(OPT_REFINE_SMALL, 1) != 0) {
    const RankArgs ra = rank_args();
    const int ng = kp <= 32 ? 32 : 64, W = 1 + si.nseg;
    const size_t lds = 8 * ((size_t)coop_qw(ra.cs) + (size_t)ng * coop_rw(ra.cs) + (size_t)ng * (2 + W)) + 8 * (size_t)ng;
    const int ppl = coop_ppl(si);
    auto kern = ng == 32 ? (ppl == 6 ? k_rank_small<6, 32> : k_rank_small<10, 32>)
                         : (ppl == 6 ? k_rank_small<6, 64> : k_rank_small<10, 64>);
    // compile-time level structures (L = 64, 32) here only with option rank_ct 2: at the 128-VGPR cap of this
    // kernel the unrolled scorer spills (28 VGPRs for L = 64)
    const int lid = ppl == 6 && opt(OPT_RANK_CT, 1) == 2 ? coop_lid(ra.cs) : 0;
    if (lid && ng == 32) kern = lid == 1 ? k_rank_small<6, 32, 1> : k_rank_small<6, 32, 2>;
    else if (lid) kern = lid == 1 ? k_rank_small<6, 64, 1> : k_rank_small<6, 64, 2>;
    if (lds > 65536)
      HQ_CHECK_HIP(hipFuncSetAttribute((const void*)kern, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
    hipLaunchKernelGGL(kern, grid, dim3(8 * ng), lds, s, ra, c.cand_score, c.eps, c.out_score, c.out_id, c.out_count,
                       c.out_resolved, ce, c.out_redo, odet, c.next_redo, fo);
    HQ_CHECK_LAUNCH();
    return HQ_OK;
  }
  if (kp > kMaxTopK) {  // long lists: rows read from global memory, one workgroup per query
    // with a workspace (hq_refine_topk_ws): the lane-cooperative pair scoring (k_rank_pairs: 8 lanes per
    // entry, rows staged per group, every level in one pass) + the per-query ranking (k_rank_sort) where
    // its shapes hold; option refine_coop = 0 keeps the one-thread-per-entry kernels below (A/B, parity)
    const int ppl = coop_ppl(si);
    if (c.workspace && ppl && opt(OPT_REFINE_COOP, 1) != 0 && Q <= 65535) {  // (its size: refine_check)
      RankArgs ra = rank_args();
      uint8_t* w = reinterpret_cast<uint8_t*>(c.workspace);
      ra.ws_sc = reinterpret_cast<double*>(w);
      ra.ws_id = reinterpret_cast<int64_t*>(w + (size_t)Q * kp * 8);
      ra.ws_rec = reinterpret_cast<double*>(w + (size_t)Q * kp * 16);
      const size_t lds = 8 * ((size_t)coop_qw(ra.cs) + (size_t)kCoopGroups * coop_rw(ra.cs));
      // (round 6: two or four entries per group with the next row in flight measured 5-10% slower at M = 100 /
      // 1000 — profiles/r06_ab_count_read.txt, rank_e rows — the kernel was dropped)
      const int lid = ppl == 6 ? coop_lid(ra.cs) : 0;  // compile-time level structures (L = 64, 32)
      auto pairs = k_rank_pairs<6, 1>;
      if (lid == 2) pairs = k_rank_pairs<6, 2>;
      else if (lid != 1) pairs = ppl == 6 ? k_rank_pairs<6> : k_rank_pairs<10>;
      hipLaunchKernelGGL(pairs, dim3((kp + kCoopGroups - 1) / kCoopGroups, Q), dim3(256), lds, s, ra);
      HQ_CHECK_LAUNCH();
      // lists > 512: 256 threads, four entries each (4 queries per CU at 118 VGPRs: M = 1000 1.70 -> 1.76M QPS,
      // profiles/r06_ab_rank_win.txt); option rank_sort_nt 512: one compare-exchange per thread and stage
      const bool narrow = pow2_at_least(kp) <= 128 && opt(OPT_RANK_SORT_SMALL, 1) != 0;
      const bool wide = !narrow && kp > 512 && opt(OPT_RANK_SORT_NT, 256) == 512;
      auto sort = k_rank_sort<128, 128>;
      if (!narrow) sort = wide ? k_rank_sort<512> : k_rank_sort<256>;
      hipLaunchKernelGGL(sort, grid, dim3(narrow ? 128 : wide ? 512 : 256), 0, s, ra, c.cand_score, c.eps, c.out_score, c.out_id, c.out_count,
                         c.out_resolved, ce, c.out_redo, odet, c.next_redo, fo);
      HQ_CHECK_LAUNCH();
      return HQ_OK;
    }
    // lists of >= 512: the candidates' raw rows only (refine_big_body's ZB)
    const bool raw = kp >= 512;
    auto kern = sm ? (raw ? k_refine_big_sm_raw : k_refine_big_sm) : (raw ? k_refine_big_raw : k_refine_big);
    hipLaunchKernelGGL(kern, grid, dim3(256), 0, s, c.q, Q, c.c, c.N, si, c.mode, c.cand_score, c.cand_id, kp, c.k,
                       c.threshold, c.thr_mode, c.eps, c.id_base, c.out_score, c.out_id, c.out_count, c.out_resolved,
                       ce, c.out_redo, c.out_det, c.next_redo, 0);
    HQ_CHECK_LAUNCH();
    return HQ_OK;
  }
  const size_t lds = ((size_t)refine_qw(si) + (size_t)kp * refine_rw(si) + (size_t)kp * (1 + si.nseg)) * 8;
  if (lds <= 96 * 1024 && c.L % 2 == 0 && !opt_on(OPT_REFINE_GLOBAL)) {  // 16-B pieces: L even
    auto kern = sm ? k_refine_lds_sm : k_refine_lds;
    HQ_CHECK_HIP(hipFuncSetAttribute((const void*)kern, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
    hipLaunchKernelGGL(kern, grid, dim3(256), lds, s, c.q, Q, c.c, c.N, si, c.mode, c.cand_score, c.cand_id, kp, c.k,
                       c.threshold, c.thr_mode, c.eps, c.id_base, c.out_score, c.out_id, c.out_count, c.out_resolved,
                       ce, c.out_redo, c.out_det, c.next_redo);
    HQ_CHECK_LAUNCH();
    return HQ_OK;
  }
  auto kern = sm ? k_refine<true> : k_refine<false>;
  hipLaunchKernelGGL(kern, grid, dim3(64), 0, s, c.q, Q, c.c, c.N, si, c.mode, c.cand_score, c.cand_id, kp, c.k,
                     c.threshold, c.thr_mode, c.eps, c.id_base, c.out_score, c.out_id, c.out_count, c.out_resolved, ce,
                     c.out_redo, c.next_redo);
  HQ_CHECK_LAUNCH();
  if (c.out_det)
    return hq_rescore(c.q.raw, c.q.Z, c.q.S, Q, c.c.raw, c.c.Z, c.c.S, c.N, c.L, c.out_id, c.k, c.id_base, c.out_det,
                      c.stream);
  return HQ_OK;
}

// an entry's body after it has filled the call: the tests, then the launch unless nothing is to run
static int refine_run(const RefineCall& c, unsigned need) {
  const int rc = refine_check(c, need);
  return rc != HQ_OK || c.Q == 0 ? rc : refine_launch(c);
}
