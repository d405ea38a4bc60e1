/* hq_mi355x.h — C-ABI of libhq_mi355x.so, the MI355X (gfx950) hot path of hilbert_quantization.
 *
 * The reference (Tylerlhess/hilbert-quantization v1.3.0) is pure Python/NumPy and has no FFI: its
 * plugin boundary is a set of Python ABCs injected into the pipelines.  Each entry
 * point below replaces the arithmetic behind one of those ABC methods; the Python package
 * `hq_mi355x` (hilbert-quantization_amd/hq_mi355x) binds them with ctypes and keeps the reference's
 * method names, argument meaning, exceptions and messages.  Replaced reference interfaces are cited
 * as file:line in the reference's `hilbert_quantization/` tree.
 *
 * Conventions (all entry points):
 *   - every buffer argument is a caller-owned DEVICE pointer; nothing here allocates device memory
 *     (hq_scan_topk takes a caller-sized workspace: hq_scan_workspace_size);
 *   - `stream` is a hipStream_t (NULL = default stream); calls are asynchronous on that stream;
 *   - return HQ_OK (0) or a negative HQ_E_* code; hq_last_error() is thread-local;
 *   - no global mutable state: calls are re-entrant from any host thread.
 */
#ifndef HQ_MI355X_H
#define HQ_MI355X_H

#include <stdint.h>
#include <stddef.h>

#ifdef __cplusplus
extern "C" {
#endif

typedef void* hq_stream_t; /* hipStream_t */

/* error codes */
#define HQ_OK 0
#define HQ_E_INVALID (-1)     /* bad argument (shape, pointer, size) */
#define HQ_E_NOT_POW2 (-2)    /* grid side is not a positive power of two */
#define HQ_E_TOO_MANY (-3)    /* more values than n*n cells */
#define HQ_E_HIP (-4)         /* HIP runtime / launch error */
#define HQ_E_UNSUPPORTED (-5) /* valid request outside what this build implements */

/* dtype codes (element type of copy-only buffers) */
#define HQ_F32 0
#define HQ_F64 1
#define HQ_F16 2
#define HQ_BF16 3
#define HQ_I8 4
#define HQ_U8 5
#define HQ_I16 6
#define HQ_I32 7
#define HQ_I64 8

int hq_version(void);
const char* hq_last_error(void);

/* ---- kernel-variant options (parity tests and A/B only) ------------------------------------------
 * Every entry point runs its tuned kernel by default and a default build never reads the environment.
 * hq_set_option selects an alternative form of a kernel (same results, checked by the parity tests):
 * e.g. "fused_v" (fused-kernel variant bits), "fused_generic", "chunk_generic", "chunk_exactdiv",
 * "chunk_wpb", "chunk_cpw", "precomp_grid", "precomp_tree_lds", "cos_kernel" (1 register-staged,
 * 2 lockstep), "refine_global", "select_2stage", "level_scores_v1" (the one-thread-per-pair dense scorer),
 * "sample_kth" (0 = provable bound), "scan_v1" (the LDS-tiled f64 scans instead of the split-f16 ones),
 * "rank_ct" (0: the long-list re-rank's runtime level structure; 2: the compile-time one in the short-list kernel too),
 * "rank_win" (0: the long-list ranking by the bitonic sort alone, no window ranking), "rank_sort_nt" (512: lists
 * > 512 in 512-thread workgroups), "rank_sort_small" (0: lists <= 128 in the 1024-entry workgroup), "decode_nt"
 * (0: plain instead of non-temporal stores in hq_dequantize_unmap), "decode_generic" (1: its generic kernel
 * for every n), "cos_topk_hint" (0: hq_cos_topk without the running threshold between tiles).  Options are
 * process-wide: set them before launching, not
 * while other host threads launch.  hq_reset_option restores the default; hq_get_option returns 1 when
 * the option is set (value in *value), 0 when it is at its default, HQ_E_INVALID for an unknown name.
 * hq_diag_build() = 1 for a `make DIAG=1` library (diagnostics kernels; HQ_<NAME> environment variables
 * are read once at load).                                                                         */
int hq_set_option(const char* name, int64_t value);
int hq_reset_option(const char* name);
int hq_get_option(const char* name, int64_t* value);
int hq_diag_build(void);
/* DIAG builds: bounds violations counted by the guarded row loads of the level-0 scan (k_scan0g,
 * k_sample_topg, k_pool_select) and of the corpus mutation kernels (k_seg_append, k_seg_gather,
 * k_seg_replace) since the library loaded (the load is clamped instead of faulting), and where the
 * first was seen: *first_line = part * 10000 + line, part 0 being csrc/hq_search.hip itself
 * and part n the file under csrc/search/ that sets HQ_PART n at its top, line the line in that file.
 * Synchronises the device.  Default builds report 0.                                               */
int hq_diag_violations(int64_t* count, int* first_line);
/* Launch geometry of the level-0 scan k_scan0g, exactly as launched (host only): query blocks of 64, corpus chunks (a multiple
 * of 8: XCD map) of chunk_len rows (a multiple of 16), and the row counts of the split copies it reads
 * (Z16: z_rows = round_up(N, 16) + 48 rows of 64 halves in the tiled fragment layout, S32: s_rows =
 * round_up(N, 4) + 48).  A C caller of hq_seg_pack0_split allocates z_rows x 64 halves and s_rows x 4
 * floats; hq_scan0_geometry(1, N, ...) returns both.  Exported for the bounds test.                 */
int hq_scan0_geometry(int Q, int64_t N, int* nqb, int* nchunks, int64_t* chunk_len, int64_t* z_rows,
                      int64_t* s_rows);

/* ---- M1/M2/M4: coordinate tables ------------------------------------------------------------
 * replaces core/hilbert_mapper.py:17-40 generate_hilbert_coordinates (+ :42-113 d2xy/xy2d/rotate)
 * and rag/embedding_generation/hilbert_mapper.py:122-204.
 * xs, ys: int32[n*n] in curve order (d2xy); xy2d: int32[n*n] row-major (index of cell (x,y) at
 * y*n+x).  Any of the three may be NULL.                                                        */
int hq_hilbert_table(int n, int32_t* xs, int32_t* ys, int32_t* xy2d, hq_stream_t stream);

/* ---- M5: 1-D -> 2-D scatter ---------------------------------------------------------------
 * replaces core/hilbert_mapper.py:115-174 map_to_2d (and rag/.../hilbert_mapper.py:16-75).
 * in: N rows of d elements (row stride in_stride elements); out: N x n x n row-major (row = y),
 * out[y][x] = in[i] for the i with d2xy(i) = (x,y), i < d; zero elsewhere.  Bit copy, any dtype.  */
int hq_map_to_2d(int dtype, const void* in, int64_t N, int64_t in_stride, int d, int n, void* out,
                 hq_stream_t stream);

/* ---- M6: 2-D -> 1-D gather ----------------------------------------------------------------
 * replaces core/hilbert_mapper.py:176-205 map_from_2d (and rag/.../hilbert_mapper.py:77-120,
 * rag/embedding_generation/reconstructor.py:100-131).  img: N x n x n; out: N x d_out with
 * out[i] = img[y_i][x_i], d_out <= n*n (callers truncate, core/pipeline.py:219).               */
int hq_map_from_2d(int dtype, const void* img, int64_t N, int n, int d_out, void* out,
                   hq_stream_t stream);

/* ---- I1: streaming hierarchical index ------------------------------------------------------
 * replaces core/streaming_index_builder.py:315-343 StreamingHilbertIndexGenerator.
 * generate_optimized_indices(image, L) (default index of HilbertQuantizer, core/pipeline.py:59-63).
 * img: N x n x n (dtype HQ_F32 or HQ_F64); the tree is built over the first stream_len values of
 * the Hilbert-ordered stream (n*n for generate_optimized_indices; len(parameters) for
 * generate_indices_during_mapping, :287-313, where partial groups of 4 never promote).
 * idx_out: float64 N x L.                                                                       */
int hq_index_streaming(int dtype, const void* img, int64_t N, int n, int stream_len, int L,
                       double* idx_out, hq_stream_t stream);

/* ---- I2: traditional index -----------------------------------------------------------------
 * replaces core/index_generator.py:313-356 _generate_traditional_indices (used by the chunk
 * encoder, core/streaming_processor.py:858-860,897-899).  img: f32 N x n x n; out: f32 N x L.   */
int hq_index_traditional_f32(const float* img, int64_t N, int n, int L, float* out,
                             hq_stream_t stream);
/* The same index for images of dtype HQ_F32 or HQ_F64.  A float64 image keeps the reference's
 * arithmetic: block means are np.mean in float64 (pairwise sum / count), samples are read in
 * float64, and every slot is rounded to float32 once, at the store (:346).                      */
int hq_index_traditional(int dtype, const void* img, int64_t N, int n, int L, float* out,
                         hq_stream_t stream);

/* ---- I2/I4 building block: block means ---------------------------------------------------------
 * np.mean of each (n/grid)^2 block of N x n x n images (dtype HQ_F32 or HQ_F64, NumPy pairwise
 * order in that dtype, result in that dtype):
 * order 0 = row-major sections (core/index_generator.py:100-144 calculate_spatial_averages);
 * order 1 = the RAG generator's Hilbert order (hierarchical_index_generator.py:204-244).
 * out: N x cnt with cnt = grid*grid (1 = whole-image mean when grid > n).                       */
int hq_block_means(int dtype, const void* img, int64_t N, int n, int grid, int order, void* out,
                   hq_stream_t stream);

/* ---- I4: RAG multi-row index ---------------------------------------------------------------
 * replaces rag/embedding_generation/hierarchical_index_generator.py:103-146
 * generate_multi_level_indices.  img: f32 N x n x n; out: f32 N x (n + R) x n where
 * R = hq_rag_index_rows(n) (image copied, one row per granularity appended, zero filled).       */
int hq_rag_index_rows(int n);
int hq_index_rag_f32(const float* img, int64_t N, int n, float* out, hq_stream_t stream);

/* ---- Q1/Q2: uint8 quantize / de-normalise ---------------------------------------------------
 * replaces core/compressor.py:256-280 _normalize_for_compression and :282-303
 * _denormalize_from_compression.  enh: f32 N x rows x cols; out u8 same shape;
 * minmax: f32 N x 2 (min, max) written.  Constant images give 128 everywhere.
 *
 * Input domain of every quantizer here (Q1, Q2, the fused kernel, the chunk encoder): all values are
 * finite and max - min of an image is finite (it does not overflow float32).  Inside that domain the
 * bytes are bit-identical to the reference's float32 trunc((x - min) / (max - min) * 255), subnormal
 * values and ranges included (float32 and f16 subnormals are kept, not flushed).  A NaN or Inf in an
 * image, or a range whose difference overflows, gives unspecified bytes and min / max, as in the
 * reference, whose astype(uint8) of NaN is undefined.  Q2 likewise takes finite min <= max with a
 * finite difference.                                                                            */
int hq_quantize_u8(const float* enh, int64_t N, int rows, int cols, uint8_t* out, float* minmax,
                   hq_stream_t stream);
int hq_dequantize_u8(const uint8_t* u8, int64_t N, int rows, int cols, const float* minmax,
                     float* out, hq_stream_t stream);

/* ---- fused map + streaming index + embed + uint8 quantize (the north-star kernel) -----------
 * replaces the component sequence of core/pipeline.py:97-146 quantize_model up to the codec:
 * pad (:325-349) -> map_to_2d -> streaming index (L) -> embed_indices_in_image
 * (core/index_generator.py:221-253) -> _normalize_for_compression.
 * in: f32 N x d (row stride in_stride elements), d <= n*n, 2 <= n <= 128;
 * frame: u8 N x (n+1) x n; idx: f64 N x L (may be NULL); minmax: f32 N x 2 (may be NULL).
 * Input domain: as for Q1 (finite values, finite max - min over the padded row and its index row). */
int hq_map_index_quantize(const float* in, int64_t N, int64_t in_stride, int d, int n, int L,
                          uint8_t* frame, double* idx, float* minmax, hq_stream_t stream);

/* ---- fused de-normalise + index-row extract + 2-D -> 1-D gather (the decode of the kernel above) ----
 * replaces the component sequence of core/pipeline.py:183-235 reconstruct_parameters after the codec:
 * _denormalize_from_compression (core/compressor.py:282-303) -> extract_indices_from_image
 * (core/index_generator.py:255-290) -> map_from_2d (core/hilbert_mapper.py:176-205) -> [:d].
 * frame: u8 N x (n+1) x n contiguous, index row last; minmax: f32 N x 2, or ONE (min, max) pair applied to
 * every frame when mm_shared != 0 (the compressor instance's state, core/compressor.py:282-303; (0, 1) is
 * the stateless u8 / 255).  out: f32 N rows of d values, rows out_stride >= d floats apart:
 * out[e][i] = the de-normalised cell at curve position i, i < d <= n*n (d = 0 allowed); floats d ..
 * out_stride - 1 of a row are not written.  idx_row (f32 N x n, may be NULL): the de-normalised last row;
 * idx_len (int32 N, may be NULL): the length extract_indices_from_image keeps, 1 + the position of the
 * last value != 0.0f (-0.0 counts as zero, as in np.nonzero), 1 when there is none.
 * Every value is (mx == mn) ? mn : ((float)b / 255.0f) * (mx - mn) + mn in float32 with the IEEE division:
 * bit-identical to hq_dequantize_u8.  2 <= n <= 128; n in {16, 32, 64} with 16-byte aligned frames runs one
 * wave per frame with 16-byte loads and stores (rows that are not 16-byte aligned: scalar stores).
 * Input domain: as for Q2 (finite min <= max with a finite difference).                              */
int hq_dequantize_unmap(const uint8_t* frame, int64_t N, int n, int d, const float* minmax, int mm_shared,
                        float* out, int64_t out_stride, float* idx_row, int32_t* idx_len, hq_stream_t stream);

/* ---- round-trip error metrics ------------------------------------------------------------------
 * replaces the three expressions of core/pipeline.py:257-259 validate_quantization for N row pairs of d
 * float32 values (row strides in floats): out f32 N x 3 = np.mean((o - r) ** 2), np.mean(np.abs(o - r)),
 * np.max(np.abs(o - r)), bit-identical to NumPy on float32 arrays (elementwise float32, the means as
 * f32(f64(pairwise f32 sum) / d) in NumPy's pairwise order).  1 <= d <= 2^26.  One thread per row walks
 * that order serially: exact, not a throughput path.                                               */
int hq_roundtrip_error(const float* orig, int64_t orig_stride, const float* recon, int64_t recon_stride,
                       int64_t N, int d, float* out /* [N, 3]: mse, mae, max_error */, hq_stream_t stream);

/* ---- config 5: f16 parameter stream, chunked (core/streaming_processor.py:539-582,877-972) ---
 * Consecutive chunks of `chunk` fp16 values (the last may be shorter, >= chunk/2) are each padded
 * to n*n (n = side of chunk), Hilbert-mapped, given the TRADITIONAL index (L = min(chunk, n)),
 * embedded and quantized: frame u8 nchunks x (n+1) x n, idx f32 nchunks x L, minmax f32 x 2.
 * A shorter last chunk gets the geometry of its own length (side ts <= n): its frame is the first
 * (ts+1)*ts bytes of the last slot and its index the first ts values; the rest of that slot is not
 * written.  A `chunk` of 5..64 values (side 4 or 8) has frames that are no multiple of 16 bytes:
 * HQ_E_UNSUPPORTED, nothing written (a tail of that size inside a larger slot is fine).  Input domain: finite f16 values (as for Q1; every finite f16
 * range is inside it).                                                                            */
int hq_chunk_encode_f16(const uint16_t* in, int64_t total, int chunk, uint8_t* frame, float* idx,
                        float* minmax, hq_stream_t stream);

/* ---- S2: level structure of an index vector of length L (host function) -------------------
 * replaces core/search_engine.py:42-109 _parse_index_structure.  Writes up to max_levels rows of
 * (grid, start, end, is_offset) into out[4*max_levels]; returns the number of levels.           */
int hq_parse_structure(int L, int32_t* out, int max_levels);

/* ---- S3 support: per-segment statistics of index vectors -----------------------------------
 * Level segments are those of hq_parse_structure(L).  Vectors are stored "segment padded": segment s
 * starts at a multiple of 4 and is zero-filled to a multiple of 4, Lp = hq_seg_padded_len(L)
 * columns, nseg = hq_seg_count(L).  For every row of idx (f64 N x L):
 *   Z[row][poff_s + j] = (c_j - mean_s) / std_s   (0 where std_s == 0)     f64 N x Lp
 *   stats[row][s]      = {mean_s, std_s, mean(c^2)_s, aux}                f64 N x nseg x 4
 * mean/std follow NumPy's pairwise summation order so the std == 0 branches of
 * core/search_engine.py:137-147 match bit-for-bit.  aux = 0 for f64 sources.                     */
int hq_seg_count(int L);
int hq_seg_padded_len(int L);
int hq_seg_prepare(const double* idx, int64_t N, int L, double* Z, double* stats, hq_stream_t stream);
/* As hq_seg_prepare; src_f32 != 0 marks rows that hold float32 index vectors (widened to f64).  The
 * reference then runs np.mean / np.std / the normalisation (and, when both sides are float32, the
 * whole score) in float32 (core/search_engine.py:137-189 keep the array dtype).  For such rows
 *   Z = f32((c - mean32) / std32), std = std32 (float32 NumPy order), mean = the f64 mean (the sum of
 *   the float32 z is not 0; with the exact mean, sum q*c = std_q std_c G + m mean_q mean_c holds),
 *   aux = 1 (float32 source; the exact scores recompute the float32 statistics), + 2 when the mean of
 *   squares is outside [2^-100, 2^100] (float32 squares under/overflow: the scans' model does not
 *   hold; callers score such rows on the dense exact path).
 * A segment whose float32 std is 0 stores the float32 mean and std 0 (the reference's constant
 * branch, whose mean comparison is float32).                                                     */
int hq_seg_prepare_src(const double* idx, int64_t N, int L, int src_f32, double* Z, double* stats,
                       hq_stream_t stream);
/* As hq_seg_prepare_src with a per-row flag (pools mixing float32 and float64 index vectors):
 * row_f32 (device u8[N], may be NULL: src_f32 applies to every row) != 0 marks float32 rows.      */
int hq_seg_prepare_rows(const double* idx, int64_t N, int L, int src_f32, const uint8_t* row_f32, double* Z,
                        double* stats, hq_stream_t stream);

/* ---- S3/S4: dense EXACT scores ---------------------------------------------------------------
 * replaces core/search_engine.py:111-189 compare_indices_at_level (level >= 0) and :191-230
 * _calculate_overall_similarity (level == -1) for Q queries against N candidates of equal L.
 * Scores are evaluated in the reference's operation order (products and squared differences
 * summed in NumPy's pairwise order), so they are bit-identical to the reference.  Inputs per side:
 * the raw index vectors R (f64 x L) and their hq_seg_prepare outputs (Z, S).  scores: f64 Q x N. */
int hq_level_scores(const double* Rq, const double* Zq, const double* Sq, int Q, const double* Rc,
                    const double* Zc, const double* Sc, int64_t N, int L, int level, double* scores,
                    hq_stream_t stream);

/* ---- S5/S6: fused MFMA scan with per-query top-k (APPROXIMATE scores) ------------------------
 * One pass over the corpus: f64 MFMA contraction (v_mfma_f64_16x16x4f64) of the normalised
 * vectors + algebraic score epilogue (|score - exact| < 1e-12 for L <= 64) + per-query top-k by
 * (score desc, id asc).  mode 0: level-0 score (progressive filter, search_engine.py:232-300;
 * video hierarchical scan, core/video_search.py:215-264); mode 1: overall score
 * (brute_force_search :302-338).  thr_mode 0: keep all; 1: score >= threshold; 2: > threshold.
 * Also the first arg-max of the approximate score (out_best, may be NULL).  id_base is added to
 * local row ids (sharding).  out_score/out_id: Q x k (-inf / -1 in empty slots), 1 <= k <= 64, and no
 * longer than the workgroup's 160 KiB of LDS hold next to the candidate tile: 64 for level-0 segments of
 * up to 64 values, 57 for the overall mode of L = 64 and the 128-value level 0 of L = 256, 25 for the
 * overall mode of L = 128 (a longer list: HQ_E_UNSUPPORTED; callers take the dense exact path).
 * Measured |score - exact| <= 2.2e-15 for L <= 256 (profiles/scan_error_bounds.txt).
 * The exact ranking is obtained with hq_refine_topk on a slightly larger list.  Vectors with an aux
 * bit 2 (unsafe) segment are outside the model: callers use the dense exact path for them.  Mode 0
 * without the arg-max and with a level-0 segment of <= 32 values runs an f64 wave-level kernel for
 * f64 sources only (float32 rows: hq_scan0_topk_split).
 * workspace: hq_scan_workspace_size(Q, N, k) bytes of device memory.                            */
size_t hq_scan_workspace_size(int Q, int64_t N, int k);
int hq_scan_topk(const double* Zq, const double* Sq, int Q, const double* Zc, const double* Sc,
                 int64_t N, int L, int mode, int k, double threshold, int thr_mode, int64_t id_base,
                 void* workspace, size_t workspace_bytes, double* out_score, int64_t* out_id,
                 double* out_best, int64_t* out_best_id, hq_stream_t stream);

/* ---- S5/S6 level-0 scan on the matrix cores (the progressive search's filtering stage) ----------
 * Same result contract as hq_scan_topk(mode 0, no arg-max), but the contraction G = sum zq*zc runs as
 * a split-f16 product (z = hi + lo, G ~= hi.hi + hi.lo + lo.hi with f32 accumulation, three
 * v_mfma_f32_16x16x32_f16 per 16x16 tile) and the filter and list scores in f32.
 * |approx - exact| <= ~5.5e-6 (measured: 4.5e-7 on adversarial inputs, profiles/scan_error_bounds.txt), so
 * callers re-rank with hq_refine_topk at eps >= 2e-5.
 * hq_seg_pack0_split builds, from hq_seg_prepare's Z and S, Z16: f16 hi[32], lo[32] of the
 * zero-padded level-0 segment for round_up(N, 16) + 48 rows (128 B per row), in 16-row tiles of 2 KiB:
 * [hi: 64 x 8][lo: 64 x 8] halves, the 8 at (16 g + j) * 8 being row 16 t + j, values 8 g .. 8 g + 7
 * (one MFMA operand fragment per lane: a wave loads 1 KiB of consecutive bytes), and S32, f32 statistics (std, mean, msq, flag bits) in SoA
 * groups of 4 rows (std[4], mean[4], msq[4], flags[4]) for round_up(N, 4) + 48 rows (16 B per row);
 * Sq/Sc are the f64 statistics of hq_seg_prepare.  Level-0 segments of up to 32 values, N < 2^31. */
/* Starting threshold of hq_scan0_topk_split: the K'-th best score of a 1/16 sample (every 16th tile of
 * 16 rows) minus the error
 * margin, K' = the smallest count with P(Binomial(k, 1/16) >= K') <= 1e-7 (12 at k = 28, 24 at k = 108,
 * 107 at k = 1008; option sample_kth overrides; K' = k, a provable lower bound of the k-th best, for
 * corpora below 16 x 4096 rows).  k up to 1024: lists longer than 64 (the reference engine's default
 * max_candidates_per_level = 100, SearchConfig's 1000) are reduced by a per-query LDS sort of the pool,
 * whose capacity is sized from the sample (an overflowing pool marks its query unresolved).  With K' < k a query can end with fewer than k listed candidates although more pass
 * the caller's threshold: its empty slots then carry score +inf (id -1), which hq_refine_topk /
 * hq_refine_rescore_topk report as unresolved (the caller's dense exact path answers the query).    */
/* hq_seg_prepare_pack0: hq_seg_prepare_rows + hq_seg_pack0_split in one launch (query batches: one wave
 * per row, the same arithmetic and outputs as the two calls; L <= 4096, level-0 segment <= 32 values).  */
int hq_seg_prepare_pack0(const double* idx, int64_t N, int L, int src_f32, const uint8_t* row_f32, double* Z,
                         double* stats, void* Z16, float* S32, hq_stream_t stream);
/* The level-0 segment's PADDED length (its values rounded up to a multiple of 4: the columns the scans
 * contract over), 0 when L has no level structure (L = 1). */
int hq_seg_level0_len(int L);
int hq_seg_pack0_split(const double* Z, const double* S, int64_t N, int L, void* Z16, float* S32,
                       hq_stream_t stream);
int hq_scan0_topk_split(const void* Zq16, const float* Sq32, const double* Sq, int Q, const void* Zc16,
                        const float* Sc32, const double* Sc, int64_t N, int L, int k, double threshold,
                        int thr_mode, int64_t id_base, void* workspace, size_t workspace_bytes,
                        double* out_score, int64_t* out_id, hq_stream_t stream);
/* hq_seg_flag_rows: the rows of a split copy (S32 of hq_seg_pack0_split) whose zero-variance / f32-unsafe
 *   flag is set, listed once per corpus into flags [1 + N] int32: flags[0] = count, then the rows (any
 *   order).  hq_scan0_topk_split_fl: hq_scan0_topk_split with that list of the corpus (the plain entry
 *   lists the flagged rows on every call: one memset and one pass over S32 per query batch).           */
int hq_seg_flag_rows(const float* S32, int64_t N, int* flags, hq_stream_t stream);
int hq_scan0_topk_split_fl(const void* Zq16, const float* Sq32, const double* Sq, int Q, const void* Zc16,
                           const float* Sc32, const double* Sc, int64_t N, int L, int k, double threshold,
                           int thr_mode, int64_t id_base, void* workspace, size_t workspace_bytes,
                           double* out_score, int64_t* out_id, const int* corpus_flags, hq_stream_t stream);

/* ---- S5 brute force: split-f16 overall scan ----------------------------------------------------
 * Replaces the per-candidate _calculate_overall_similarity loop of brute_force_search
 * (core/search_engine.py:302-338, :191-230) with one scan over all levels: approximate overall scores
 * (|approx - exact| <= ~6e-6; measured 1.8e-7) -> per-query top k, re-ranked exactly by hq_refine_topk
 * (mode 1).  A query with an f32-unsafe segment is not scanned, and a query whose passing pairs overflow a
 * wave's append buffer or its pool is given up: either list is (+inf, -1) throughout (unresolved).
 * hq_seg_packov_info: the layout of L's level segments (K-blocks of 32 values, segments of >= 2 values,
 * one-value segments, floats per statistics group of 4 rows); HQ_E_UNSUPPORTED when L has none (a
 * segment longer than 32 values, more than 4 / 2 of either kind, or another block pattern than the
 * L = 64 and L = 32 structures): callers keep hq_scan_topk.
 * hq_seg_packov_split builds from hq_seg_prepare's Z and S: Zo16, f16 hi / lo of every segment's
 * normalised values packed into the K-blocks, round_up(N, 16) + 48 rows of nkb x 128 B in 16-row
 * tiles of nkb x 2 KiB (hq_seg_pack0_split's fragment order per block), and So32, f32 statistics in
 * groups of 4 rows (per one-value segment value[4], row flags[4], pre-filter offsets[4], then per row
 * and segment (std, mean, msq, zero-std flag)) for (round_up(N, 4) + 48) / 4 groups.
 * hq_scanov_topk_split: Zq/Zc are hq_seg_prepare's f64 Z (rows with an f32-unsafe statistic are scored
 * from them in f64); the starting threshold comes from a 1/16 tile sample (K' as
 * hq_scan0_topk_split: short lists carry +inf, which hq_refine_topk reports as unresolved).  k <= 1024. */
int hq_seg_packov_info(int L, int* nkb, int* ng, int* nc, int* group_floats);
int hq_seg_packov_split(const double* Z, const double* S, int64_t N, int L, void* Zo16, float* So32,
                        hq_stream_t stream);
/* hq_seg_append: grow a resident corpus of N0 rows by the M rows of idx (f64 [M, L]; src_f32 / row_f32 [M] as
 *   hq_seg_prepare_rows) in ONE launch, without moving a resident row.  Z, stats, Z16, S32, Zov16, Sov32 and
 *   flags are the BASES of the corpus's buffers, each with room for N1 = N0 + M rows and its padding
 *   (round_up(N1, 16) + 48 rows of Z16 / Zov16, round_up(N1, 4) + 48 rows of S32 / Sov32, 1 + N1 ints of flags).
 *   One wave per new row writes its Z, stats, split level-0 copy, split overall copy and flag-list entry
 *   (flags[0] grows by an atomic add; N0 = 0 clears it first); further workgroups write the pad rows after
 *   N1.  Afterwards every buffer equals, byte for byte, what hq_seg_prepare_rows, hq_seg_pack0_split,
 *   hq_seg_packov_split and hq_seg_flag_rows (as a set: the list has no order) write for the N1 rows; only rows
 *   >= N0 are written, so rows below N0 in N0's 16-row tile or 4-row group keep their bytes.  Z16 / S32 may be
 *   NULL (level-0 segment longer than 32 values), Zov16 / Sov32 too (no hq_seg_packov_info layout), flags too.
 *   L <= 4096 (else HQ_E_UNSUPPORTED); M = 0 writes nothing.  The caller orders the call after every scan
 *   that reads the corpus (stream order or an event): readers of N0 rows treat [N0, ...) as pad rows.        */
int hq_seg_append(const double* idx, int64_t M, int L, int src_f32, const uint8_t* row_f32, int64_t N0, double* Z,
                  double* stats, void* Z16, float* S32, void* Zov16, float* Sov32, int* flags, hq_stream_t stream);
/* hq_seg_gather: select M rows of a resident corpus of N_src rows into a SECOND set of buffers in ONE launch:
 *   destination row i becomes source row src_row[i] (device int64 [M], every value in [0, N_src): any order,
 *   repeats allowed; the range is the caller's precondition).  Removing rows is the gather of the survivors.
 *   R, Z, stats, Z16, S32, Zov16, Sov32 and flags are the bases of the destination buffers, each with room for
 *   M rows and its padding (round_up(M, 16) + 48 rows of Z16 / Zov16, round_up(M, 4) + 48 rows of S32 / Sov32,
 *   1 + M ints of flags); no destination may alias a source.  One wave per 4 destination rows copies their raw
 *   values (R_src and R may both be NULL), Z and stats (nothing is recomputed: they are functions of the row
 *   alone), then writes their split level-0 copies, split overall copies and flag-list entries from the copy;
 *   further workgroups write the pad rows after M; flags[0] is cleared on the stream first.  Afterwards every buffer
 *   equals, byte for byte, what hq_seg_prepare_rows (with the rows' float32 flags), hq_seg_pack0_split,
 *   hq_seg_packov_split and hq_seg_flag_rows (as a set) write for the M selected rows.  Z16 / S32, Zov16 /
 *   Sov32 and flags may be NULL as for hq_seg_append.  Any L with a level structure (nothing is recomputed, so
 *   no L <= 4096 limit); M = 0 writes the pad rows of an empty corpus and flags[0] = 0; M >= 2^31 - 1:
 *   HQ_E_UNSUPPORTED (int32 row ids).  Order the call after the writers of the source, as a scan.            */
int hq_seg_gather(const int64_t* src_row, int64_t M, int64_t N_src, int L, const double* R_src, const double* Z_src,
                  const double* S_src, double* R, double* Z, double* stats, void* Z16, float* S32, void* Zov16,
                  float* Sov32, int* flags, hq_stream_t stream);
/* hq_seg_replace: overwrite M resident rows of a corpus of N rows IN PLACE with the rows of idx (f64 [M, L];
 *   src_f32 / row_f32 [M] as hq_seg_prepare_rows): row rows[i] (device int64 [M], distinct values in [0, N): the
 *   caller's precondition) takes idx row i.  One launch runs hq_seg_append's per-row steps (Z, stats, split
 *   level-0 copy, split overall copy) on those rows; every other row and every pad row keeps its bytes.  A
 *   replaced row may enter or leave the flagged-row list, so flags (when given) is then cleared and listed
 *   again from the N rows' flag words (hq_seg_flag_rows's kernel) on the same stream.  Afterwards every buffer
 *   equals, byte for byte, a fresh build of the updated rows (flags as a set).  The raw rows are the caller's
 *   to update.  NULL pairs as for hq_seg_append; L <= 4096 (else HQ_E_UNSUPPORTED); M = 0 writes nothing.  A
 *   writer: order it after every scan that reads the corpus.                                                 */
int hq_seg_replace(const double* idx, int64_t M, const int64_t* rows, int L, int src_f32, const uint8_t* row_f32,
                   int64_t N, double* Z, double* stats, void* Z16, float* S32, void* Zov16, float* Sov32, int* flags,
                   hq_stream_t stream);
size_t hq_scanov_workspace_size(int Q, int64_t N, int k);
int hq_scanov_topk_split(const void* Zq16, const float* Sq32, const double* Sq, const double* Zq, int Q,
                         const void* Zc16, const float* Sc32, const double* Sc, const double* Zc, int64_t N, int L,
                         int k, double threshold, int thr_mode, int64_t id_base, void* workspace,
                         size_t workspace_bytes, double* out_score, int64_t* out_id, hq_stream_t stream);

/* ---- S5/S6: exact re-rank of a scan list -----------------------------------------------------
 * cand_score/cand_id: Q x kp list from hq_scan_topk (approximate, sorted).  Re-scores every listed
 * candidate exactly (as hq_level_scores), applies the threshold test exactly and writes the exact
 * top-k (score desc, id asc): out_score/out_id Q x k, out_count Q, and out_resolved Q = 1 when the
 * result is provably the exact top-k over the whole corpus given |approx - exact| <= eps (else the
 * caller re-runs that query on the dense exact path).  kp <= 1024 (lists longer than 64 are staged in
 * tiles and ranked by an LDS sort), k <= kp.  Any L with a level structure (L >= 2): the lane-cooperative
 * kernels take even L <= 140 (every segment <= 128 values, at most six levels), the LDS-staged kernel even L
 * whose kp rows fit 96 KiB (L <= 160 at kp = 64), every other length - odd L included - kernels that read
 * the rows from global memory; the outputs are the same, bit for bit (tests/test_gpu_scorer_sweep.py runs
 * every one of them against the CPU oracle).  out_redo (device int, may
 * be NULL): the number of queries that need the dense path — unresolved, or (count_empty != 0) with
 * no candidate passing — so the caller syncs on one int.                                          */
int hq_refine_topk(const double* Rq, const double* Zq, const double* Sq, int Q, const double* Rc,
                   const double* Zc, const double* Sc, int64_t N, int L, int mode,
                   const double* cand_score, const int64_t* cand_id, int kp, int k,
                   double threshold, int thr_mode, double eps, int64_t id_base, double* out_score,
                   int64_t* out_id, int* out_count, int* out_resolved, int count_empty, int* out_redo,
                   hq_stream_t stream);
/* hq_refine_topk + the exact re-score of its output (core/search_engine.py:191-230 for each output
 * pair, as hq_rescore computes it): out_det [Q, k, 1 + nseg] = [overall, level 0, level 1, ...] of
 * every output entry, zeros for empty slots.  The candidates' rows are staged once per query in LDS,
 * so the progressive search needs no separate hq_rescore launch for its survivors.                  */
int hq_refine_rescore_topk(const double* Rq, const double* Zq, const double* Sq, int Q, const double* Rc,
                           const double* Zc, const double* Sc, int64_t N, int L, int mode,
                           const double* cand_score, const int64_t* cand_id, int kp, int k,
                           double threshold, int thr_mode, double eps, int64_t id_base,
                           double* out_score, int64_t* out_id, int* out_count, int* out_resolved,
                           int count_empty, int* out_redo, double* out_det, hq_stream_t stream);
/* hq_refine_rescore_topk with a ping-pong pair of redo counters (no memset launch per batch): out_redo
 * must be zero on entry (fresh, or cleared by the previous call as its next_redo); the kernel clears
 * next_redo for the next batch.  Alternate the two counters between consecutive batches of a stream and
 * copy out_redo to the host behind the batch (the next batch's kernels run after that copy).          */
int hq_refine_rescore_topk_pp(const double* Rq, const double* Zq, const double* Sq, int Q, const double* Rc,
                              const double* Zc, const double* Sc, int64_t N, int L, int mode,
                              const double* cand_score, const int64_t* cand_id, int kp, int k,
                              double threshold, int thr_mode, double eps, int64_t id_base,
                              double* out_score, int64_t* out_id, int* out_count, int* out_resolved,
                              int count_empty, int* out_redo, int* next_redo, double* out_det,
                              hq_stream_t stream);
/* The three entries above in one, with a device workspace (hq_refine_workspace_size bytes; may be NULL):
 * out_det and next_redo nullable (NULL out_det = hq_refine_topk's outputs; a non-NULL next_redo = the
 * ping-pong counters of hq_refine_rescore_topk_pp).  Lists longer than 64 then run the lane-cooperative
 * re-rank: 8 lanes score one list entry (NumPy's eight pairwise accumulators one per lane, the row staged
 * with 16-byte loads), every level of the entry in one pass over its row, the exact scores, ids and records
 * to the workspace, then one workgroup per query ranks them.  Same outputs, bit for bit.
 * Replaces the re-rank arithmetic of core/search_engine.py:232-300 (level-0 filter) and :340-388
 * (overall re-score of the survivors) for the reference's default lists (M = 100, :31; 1000, config.py:181). */
size_t hq_refine_workspace_size(int Q, int kp, int L);
int hq_refine_topk_ws(const double* Rq, const double* Zq, const double* Sq, int Q, const double* Rc,
                      const double* Zc, const double* Sc, int64_t N, int L, int mode,
                      const double* cand_score, const int64_t* cand_id, int kp, int k,
                      double threshold, int thr_mode, double eps, int64_t id_base,
                      double* out_score, int64_t* out_id, int* out_count, int* out_resolved,
                      int count_empty, int* out_redo, int* next_redo, double* out_det,
                      void* workspace, size_t workspace_bytes, hq_stream_t stream);
/* The level-0 re-rank of one progressive search (mode 0, records on, count_empty on) with its final
 * ranking fused in: the level-0 outputs and the proof as hq_refine_topk_ws (out_det not produced), and
 * fin_id [Q, K_out], fin_det [Q, K_out, 1 + nseg], fin_count [Q] = hq_progressive_final_ex's outputs for
 * R = 1 and no arg-max fallback (best id -1: a query where nothing passed gets count 0 and is counted in
 * out_redo).  The final order is core/search_engine.py:387's stable sort by the overall score over the
 * level-0 order (key32: thr_mode | HQ_THR_KEY32 ranks by float32-rounded keys).  On the lane-cooperative
 * paths only (the cooperative shapes; kp > 64 needs the workspace); HQ_E_UNSUPPORTED otherwise, and the
 * caller keeps the two-step form.  out_score and out_id may both be NULL: the level-0 lists are then not
 * written (the final outputs, count, resolved flag and redo count are the same). */
int hq_refine_final_ws(const double* Rq, const double* Zq, const double* Sq, int Q, const double* Rc,
                       const double* Zc, const double* Sc, int64_t N, int L, const double* cand_score,
                       const int64_t* cand_id, int kp, int k, double threshold, int thr_mode, double eps,
                       int64_t id_base, double* out_score, int64_t* out_id, int* out_count,
                       int* out_resolved, int* out_redo, int* next_redo, int K_out, int64_t* fin_id,
                       double* fin_det, int* fin_count, void* workspace, size_t workspace_bytes,
                       hq_stream_t stream);

/* ---- S4 on candidate lists: EXACT overall + per-level scores of selected pairs ---------------
 * ids: int64 Q x k GLOBAL ids (row = id - id_base; out of range / < 0 -> zeros);
 * out: f64 Q x k x (1 + nseg) = [overall, level_0 .. level_{nseg-1}] (search_engine.py:191-230). */
int hq_rescore(const double* Rq, const double* Zq, const double* Sq, int Q, const double* Rc,
               const double* Zc, const double* Sc, int64_t N, int L, const int64_t* ids, int k,
               int64_t id_base, double* out, hq_stream_t stream);

/* ---- S5 final stage, R-way (R = number of corpus shards) -------------------------------------
 * Inputs per shard r: level-0 top-M lists s0/ids (R x Q x M, sorted), their rescored rows det
 * (R x Q x M x (1+nseg)), and the shard's level-0 arg-max best/best_id (R x Q) with its row
 * best_det (R x Q x (1+nseg)).  Forms the global level-0 top-M, falls back to the global first
 * arg-max when no candidate passed (search_engine.py:295-298), stable-sorts the survivors by the
 * overall score (:386-388) and writes the top K: out_id (Q x K, -1 padded), out_det
 * (Q x K x (1+nseg)), out_count (Q).  M <= 1024, R <= 16.                                        */
int hq_progressive_final(int R, int Q, int M, int nseg, const double* s0, const int64_t* ids,
                         const double* det, const double* best, const int64_t* best_id,
                         const double* best_det, int K, int64_t* out_id, double* out_det,
                         int* out_count, hq_stream_t stream);
/* hq_progressive_final with flags: 1 = float32 sort keys (every vector float32: the reference's sort
 * compares a numpy float32 score with a Python-float one in float32 under NumPy 2 / NEP 50, so the merge
 * and the stable sort rank by the float32-rounded values; core/search_engine.py:291, :387).  The re-rank
 * takes the same mode as thr_mode | 8 (HQ_THR_KEY32) on hq_refine_topk / hq_refine_rescore_topk.      */
#define HQ_THR_KEY32 8
int hq_progressive_final_ex(int R, int Q, int M, int nseg, const double* s0, const int64_t* ids,
                            const double* det, const double* best, const int64_t* best_id,
                            const double* best_det, int K, int64_t* out_id, double* out_det,
                            int* out_count, int flags, hq_stream_t stream);

/* ---- S5 support: top-k of a dense score matrix (k > 64, e.g. max_candidates_per_level = 100) -----
 * scores f64 Q x N -> out_score/out_id Q x k ordered (score desc, id asc) among candidates passing
 * thr_mode (0 none, 1 >=, 2 >); out_best/out_best_id (may be NULL): first arg-max.               */
int hq_select_topk(const double* scores, int Q, int64_t N, int k, double threshold, int thr_mode,
                   int64_t id_base, double* out_score, int64_t* out_id, double* out_best,
                   int64_t* out_best_id, hq_stream_t stream);
/* Two-stage form of hq_select_topk for long rows (the dense exact fallback: few queries x a 1M-row
 * corpus): parts of ~8192 entries select their own top-k and arg-max in parallel (one wave each), then
 * one wave per query merges the parts' candidates in the same total order - identical results.
 * workspace: hq_select_workspace_size(Q, N, k) bytes (0 / NULL -> the one-stage kernel).           */
size_t hq_select_workspace_size(int Q, int64_t N, int k);
int hq_select_topk_ws(const double* scores, int Q, int64_t N, int k, double threshold, int thr_mode,
                      int64_t id_base, void* workspace, size_t workspace_bytes, double* out_score,
                      int64_t* out_id, double* out_best, int64_t* out_best_id, hq_stream_t stream);

/* ---- S3 on raw segments (candidate pools of mixed index length) -------------------------------
 * compare_indices_at_level for the level segments already sliced and truncated to a common length
 * m (search_engine.py:122-135): q f64[m] against C f64 N x m -> out f64[N].                      */
int hq_pair_scores_raw(const double* q, const double* C, int64_t N, int m, double* out,
                       hq_stream_t stream);
/* As hq_pair_scores_raw; q_f32 / c_f32 != 0: that side holds float32 values, whose statistics and
 * normalised values the reference computes in float32 (the whole score when both are float32).   */
int hq_pair_scores_raw_src(const double* q, const double* C, int64_t N, int m, int q_f32, int c_f32,
                           double* out, hq_stream_t stream);

/* ---- S7: RAG cosine scores (rag/search/engine.py:622-660, 1025-1051) --------------------------
 * a: f32 Q x K, b: f32 N x K -> out f64 Q x N of (cos + 1) / 2 (0 if a norm is 0).               */
int hq_cosine_scores(const float* a, int Q, const float* b, int64_t N, int K, double* out,
                     hq_stream_t stream);

/* ---- §8f row 3: pre-computed overlapping-square index ---------------------------------------
 * replaces core/precomputed_hilbert_index.py:65-212 PrecomputedHilbertIndexer.
 * create_precomputed_index (built for every model by HilbertQuantizer.quantize, api.py:162-173).
 * hq_precomputed_layout: levels of _calculate_granularity_levels (:121-149) as int32 quadruples
 *   (grid, square, count, first output) into levels_out[4*max_out]; returns the level count.
 * hq_precomputed_index: N inputs -> float32 averages [N, T] (row stride out_stride >= T), levels
 *   finest first, each level = grid squares row-major then the half-offset squares; every value is
 *   float32(np.mean(square)) bit for bit.  kind 0: n x n images (dtype HQ_F32 / HQ_F64, image
 *   stride in_stride elements); kind 1: 1-D Hilbert-ordered streams of d <= n*n values, zero
 *   padded (core/pipeline.py:298-319 _get_2d_representation).  n: power of two <= 128 (f64: <= 64);
 *   max_levels / min_square_size as PrecomputedHilbertIndexer's constructor (defaults 6, 2).        */
int hq_precomputed_layout(int n, int max_levels, int min_square_size, int32_t* levels_out, int max_out);
int hq_precomputed_index(int dtype, int kind, const void* in, int64_t N, int64_t in_stride, int d, int n,
                         int max_levels, int min_square_size, float* out, int64_t out_stride, hq_stream_t stream);
/* hq_precomputed_stats: per vector and level l (averages [offsets[l], offsets[l] + counts[l]) of
 *   each row of avgs, row stride `stride`): stats [N, nlev, 3] float32 = (np.mean, np.std,
 *   np.mean(a**2)) in NumPy's order, and norm (same layout as avgs) = (a - mean) / std where std != 0.
 *   Call it with counts = min(query count, candidate count) per level (the reference truncates,
 *   :427-431).
 * hq_precomputed_similarity: replaces :358-466 (_calculate_precomputed_similarity over
 *   _compare_precomputed_levels) for Q x N pairs: out_overall [Q, N] (float64 holding the exact
 *   value), out_type [Q, N] (0: the reference returns a numpy float32, 1: a Python float — decides
 *   the `>= similarity_threshold` comparison, :342), out_levels [Q, N, nlev] (nullable).  weights:
 *   the normalised level weights (Python floats, :390-404).                                      */
/* hq_pearson_f64: replaces :468-496 (PrecomputedSimilaritySearchEngine.compare_indices_at_level, the
 *   legacy np.corrcoef comparison) for one query q[m] against N rows of C [N, m] -> out [N] f64;
 *   np.std branches and np.allclose exact, the correlation within ~1e-15 (BLAS order in np.cov). */
int hq_pearson_f64(const double* q, const double* C, int64_t N, int m, double* out, hq_stream_t stream);
int hq_precomputed_stats(const float* avgs, int64_t N, int64_t stride, int nlev, const int32_t* offsets,
                         const int32_t* counts, float* stats, float* norm, hq_stream_t stream);
int hq_precomputed_similarity(const float* q_avgs, const float* q_norm, const float* q_stats, int Q, int64_t q_stride,
                              const float* c_avgs, const float* c_norm, const float* c_stats, int64_t N,
                              int64_t c_stride, int nlev, const int32_t* q_offsets, const int32_t* c_offsets,
                              const int32_t* counts, const double* weights, double* out_overall, uint8_t* out_type,
                              double* out_levels, hq_stream_t stream);

/* ---- S7 dense frame similarity on the matrix cores ------------------------------------------
 * replaces rag/search/engine.py:622-660 (_calculate_embedding_cosine_similarity) for Q query x N
 * frame pairs of K values (e.g. 64 x 64 images, K = 4096).
 * hq_cos_prepare: f32 rows X [N, K] (row stride ld) -> split-f16 copies X16 of hq_cos_padded_rows(N) x 2 x
 *   hq_cos_padded_k(K) halves (power-of-two scaled hi / lo halves in 1 KiB MFMA operand fragments: 16-row
 *   tile t, K step kb of 32, plane p at ((t KB + kb) 2 + p) x 512 halves, lane 16 g + j = row 16 t + j,
 *   k = 32 kb + 8 g .. + 7; the superseded kernels of option cos_kernel 1-3 use rows [N, 2, Kp]) and
 *   inv [padded rows] = 1 / (scale |x|) (0 for a zero row).  Prepare a corpus once, each query batch per
 *   call, under the same cos_kernel option as the scoring call.
 * hq_cos_scores_mfma: out [Q, N] f64 = (cos + 1) / 2 (0 when a norm is 0), split-f16 MFMA contraction
 *   (v_mfma_f32_16x16x32_f16 x 3), within 1e-5 of the exact cosine and of the reference's float32 BLAS result
 *   for K <= 16384.  The error depends on the rows (profiles/cos_error_bounds.txt, measured per row family):
 *   5e-8 where the products cancel (zero-mean rows, any K); same-sign rows (images, decoded u8 frames, post-ReLU
 *   embeddings) grow with K, up to 1.4e-6 at K = 4096 and 3.2e-6 at K = 16384.
 *   Input domain: every finite float32 row, subnormal rows (max |x| < 2^-126) and rows up to FLT_MAX included,
 *   gives finite scores: the row is scaled by an exact power of two (ldexpf) and its norm is taken in float64.
 *   Known, intended difference: a row so small that the reference's float32 norm underflows to 0 (all |x|
 *   below about 3e-23) scores 0.0 there; here it is scored from its float64 norm like any other row, as
 *   hq_cosine_scores does.  A row holding a NaN or an inf is outside the domain: its inverse norm is stored as
 *   0, so all its scores are 0.0 and no other row's score changes (hq_cosine_scores / hq_cosine_scores_dt
 *   return NaN for such a row, as the reference does).
 * hq_cos_scores_mfma_f32: the same scores rounded once to float32 (the reference's own score dtype; half
 *   the output bytes).                                                                           */
int hq_cos_padded_k(int K);
int64_t hq_cos_padded_rows(int64_t N);
int hq_cos_prepare(const float* X, int64_t N, int64_t ld, int K, void* X16, double* inv, hq_stream_t stream);
int hq_cos_scores_mfma(const void* A16, const double* inv_a, int Q, const void* B16, const double* inv_b, int64_t N,
                       int K, double* out, hq_stream_t stream);
int hq_cos_scores_mfma_f32(const void* A16, const double* inv_a, int Q, const void* B16, const double* inv_b, int64_t N,
                           int K, float* out, hq_stream_t stream);

/* hq_cos_topk: the nearest k frames of every query without the Q x N score matrix.  Operands as for
 *   hq_cos_scores_mfma in the default tiled layout (option cos_kernel 1-3: HQ_E_UNSUPPORTED).  out_score /
 *   out_id [Q, k]: the best k frames among those passing thr_mode (0 none, 1 >= threshold, 2 > threshold), in
 *   (score descending, id ascending) order, ids = frame + id_base, empty slots -inf / -1.  The scores are the
 *   float64 values hq_cos_scores_mfma writes for those pairs, bit for bit, and the lists equal
 *   hq_select_topk_ws of that matrix.  The GEMM's epilogue selects k frames per (query, 384-frame tile) into
 *   the workspace and merge launches reduce the tiles' lists 64 at a time; option "cos_topk_hint" (default 1)
 *   lets tiles skip candidates below a k-th score another tile has already published (same result).
 *   1 <= k <= 64 (larger: HQ_E_UNSUPPORTED).  workspace: hq_cos_topk_workspace_size(Q, N, k) bytes, about
 *   16 Q k N / 384.                                                                               */
size_t hq_cos_topk_workspace_size(int Q, int64_t N, int k);
int hq_cos_topk(const void* A16, const double* inv_a, int Q, const void* B16, const double* inv_b, int64_t N,
                int K, int k, double threshold, int thr_mode, int64_t id_base,
                void* workspace, size_t workspace_bytes,
                double* out_score, int64_t* out_id, hq_stream_t stream);

/* ---- compressed-domain frame search: exact cosine top-k on u8 frames ------------------------------
 * The store's own format (hq_map_index_quantize / hq_quantize_u8: K bytes u and float32 (mn, mx) per frame,
 * x_i = mn + (mx - mn) u_i / 255) is searched without decoding: the cosine of two dequantised frames is a
 * closed form of exact integers and the two (mn, mx) pairs.  Queries of hq_cosq_* are u8 rows too (quantise them
 * with hq_map_index_quantize / hq_quantize_u8); float32 queries against the same prepared corpus, without
 * quantising them to 8 bits, go through hq_cosqf_* below.
 * The contract, everything in float64 from the float32 (mn, mx):
 *   row:  w_i = u_i - 128;  S = sum w_i, T = sum w_i^2 (exact integers);  s = (mx - mn) / 255 (0 when mx == mn);
 *         m = mn + s (128 + S / K) (the row mean);  V = K T - S^2 (exact in int64, >= 0);  n^2 = K m^2 + s^2 V / K;
 *         inv = 1 / sqrt(n^2), 0 when n^2 == 0 and 0 when mn or mx is not finite;  a = m inv, b = s inv.
 *   pair: P = sum w_q,i w_c,i (the int32 accumulator of v_mfma_i32_16x16x64_i8);  t = K P - S_q S_c (exact);
 *         cos = K a_q a_c + b_q b_c t / K;  score = (cos + 1) / 2, and 0.0 when either inv is 0.
 *   A row with a non-finite mn or mx is outside the input domain: it scores 0.0 against everything and changes
 *   no other score.  Every finite float32 (mn, mx), subnormal and near-FLT_MAX ranges included, is in the domain.
 *   The integer part is exact, so the score does not depend on tile shape, K order or kernel form: it is within
 *   a few float64 roundings (1e-13 is tested) of the cosine of the dequantised frames in extended precision.
 *   Limits: 1 <= K <= 65536 (|P| <= 2^30; K T and S_q S_c below 2^48); a larger K: HQ_E_UNSUPPORTED.  Padded K
 *   positions and padded rows hold w = 0 and the formulas use the true K.
 * hq_cosq_prepare: frames u8 [N, K] (ld bytes between frames, ld >= K: a store of (n + 1) x n frames searched on
 *   its n leading rows has ld = (n + 1) n, K = n n), minmax f32 [N, 2] -> X8: hq_cosq_padded_rows(N) x
 *   hq_cosq_padded_k(K) signed bytes u ^ 0x80 in 1 KiB MFMA operand fragments (16-row tile t, K step kb of 64 at
 *   (t KB + kb) 1024; lane 16 g + j = row 16 t + j, bytes 64 kb + 16 g .. + 15), and stats f64 [padded rows, 4] =
 *   (m / sqrt(n^2 / K), s / (K sqrt(n^2 / K)), S, inv != 0), the pre-scaled a and b with which
 *   cos = A_q A_c + (B_q B_c) t.  One launch, no host round trip.  16-byte loads when the base and ld are
 *   multiples of 16, byte loads otherwise.
 * hq_cosq_scores: out [Q, N] f64, the dense scores.
 * hq_cosq_topk: arguments and semantics of hq_cos_topk on these operands (threshold, thr_mode 0 / 1 / 2, id_base,
 *   -inf / -1 padding, 1 <= k <= 64 else HQ_E_UNSUPPORTED, (score descending, id ascending)); the lists equal
 *   hq_select_topk_ws of hq_cosq_scores bit for bit, so duplicated frames tie exactly and list by id.
 *   workspace: hq_cosq_topk_workspace_size(Q, N, k) bytes.
 * Zero Q or N: HQ_OK before any pointer is looked at; negative sizes, K < 1, ld < K, NULL operands: HQ_E_INVALID. */
int hq_cosq_padded_k(int K);
int64_t hq_cosq_padded_rows(int64_t N);
int hq_cosq_prepare(const uint8_t* frames, int64_t N, int64_t ld, int K, const float* minmax, void* X8, double* stats,
                    hq_stream_t stream);
int hq_cosq_scores(const void* A8, const double* stats_a, int Q, const void* B8, const double* stats_b, int64_t N,
                   int K, double* out, hq_stream_t stream);
size_t hq_cosq_topk_workspace_size(int Q, int64_t N, int k);
int hq_cosq_topk(const void* A8, const double* stats_a, int Q, const void* B8, const double* stats_b, int64_t N,
                 int K, int k, double threshold, int thr_mode, int64_t id_base,
                 void* workspace, size_t workspace_bytes,
                 double* out_score, int64_t* out_id, hq_stream_t stream);
/* The mutable store.  A resident operand (X8, stats) may hold more rows than its N frames need: cap_rows rows, a
 *   multiple of 128 and >= hq_cosq_padded_rows(N).  hq_cosq_scores / hq_cosq_topk / hq_cosqf_scores / hq_cosqf_topk
 *   read only the first hq_cosq_padded_rows(N) rows and mask every frame >= N, so such a buffer is a valid operand
 *   as it stands.  A row's bytes are 4 KB pieces of 16 bytes (KB = hq_cosq_padded_k(K) / 64), piece (kb, g) at
 *   (t KB + kb) 1024 + 16 (16 g + j) for row 16 t + j, and 32 bytes of stats: no piece holds bytes of two rows.
 *   The contract of the three calls below: afterwards the first hq_cosq_padded_rows(N) rows of X8 and of stats,
 *   N the resulting number of frames, equal bit for bit what hq_cosq_prepare writes for those N frames (pad rows
 *   [N, padded rows) included: bytes 0, stats (0, 0, 0, 0)); nothing past them is written and no row the call
 *   does not name changes.  All three are writers of (X8, stats): the caller orders them after every search
 *   that reads the corpus (stream order or an event), as for hq_seg_append.
 * hq_cosq_append: grow a resident operand of N0 frames by the M frames of `frames` (u8, ld bytes apart, minmax f32
 *   [M, 2], as hq_cosq_prepare) in ONE launch: frame i becomes row N0 + i.  In N0's 16-row tile only the pieces
 *   and stats of rows >= N0 are written and the sums S and T run over the new rows alone; every further tile is
 *   hq_cosq_prepare's contiguous 1 KiB wave store per fragment (16-byte loads when the base and ld are multiples
 *   of 16, byte loads otherwise).  Rows [N0 + M, hq_cosq_padded_rows(N0 + M)) are written as pad rows (after a
 *   reallocation they are uninitialised memory).  cap_rows >= hq_cosq_padded_rows(N0 + M).
 * hq_cosq_replace: overwrite M resident rows of a corpus of N frames IN PLACE in ONE launch: frame i takes row
 *   rows[i] (device int64 [M], distinct values in [0, N): the caller's precondition), bytes and stats; the other
 *   rows of its tile keep their bytes.  A row id outside [0, N) is skipped, not written.
 * hq_cosq_gather: row i of a SECOND operand (X8, stats; cap_rows rows; it may not alias the source) becomes row
 *   src_row[i] of the source of N_src frames (device int64 [M], any order, repeats allowed) in ONE launch.
 *   Nothing is recomputed: the 4 KB pieces move to their new lane positions (destination tiles as whole 1 KiB
 *   wave stores) and the 32 stats bytes with them; rows [M, hq_cosq_padded_rows(M)) are written as pad rows.  An
 *   id outside [0, N_src) is clamped for the load: that row's content is unspecified, no read leaves the source.
 *   Removing, selecting, inserting and re-ordering frames are all this call.  cap_rows >= hq_cosq_padded_rows(M).
 * Return codes, in hq_cosq_prepare's order: negative sizes, K < 1, ld < K, cap_rows not a multiple of 128 or
 *   smaller than the result's padded rows, M > 0 with N_src = 0: HQ_E_INVALID; then M = 0: HQ_OK and nothing is
 *   touched (hq_cosq_gather with M = 0 and cap_rows > 0 goes on and writes rows [0, 128) as the pad rows of an
 *   empty corpus); K > 65536: HQ_E_UNSUPPORTED; a NULL buffer: HQ_E_INVALID.                                  */
int hq_cosq_append(const uint8_t* frames, int64_t M, int64_t ld, int K, const float* minmax, int64_t N0,
                   int64_t cap_rows, void* X8, double* stats, hq_stream_t stream);
int hq_cosq_replace(const uint8_t* frames, int64_t M, int64_t ld, int K, const float* minmax, const int64_t* rows,
                    int64_t N, void* X8, double* stats, hq_stream_t stream);
int hq_cosq_gather(const int64_t* src_row, int64_t M, int64_t N_src, int K, const void* X8_src,
                   const double* stats_src, int64_t cap_rows, void* X8, double* stats, hq_stream_t stream);

/* ---- float32 queries against the u8 frame store: exact asymmetric cosine top-k --------------------
 * The corpus stays compressed (exactly what hq_cosq_prepare wrote: one resident corpus serves both query kinds),
 * the query keeps its float32 precision: a query row is rounded to 24-bit fixed point, stored as three int8 digit
 * planes, and every plane is contracted exactly with the corpus's signed bytes by v_mfma_i32_16x16x64_i8.
 * The contract:
 *   query row: K float32 values q_i (ld floats between rows, ld >= K).
 *         amax = max |q_i|.  If amax == 0, or any q_i is NaN or inf, the row has ok = 0: it scores 0.0 against
 *         every frame and changes no other score.
 *         e: amax = f 2^e with f in [0.5, 1) (frexp).
 *         v_i = clamp(rint(q_i 2^(23 - e)), -2^23, 2^23 - 1), rint = round to nearest even, the scaling exact (ldexp,
 *         or in float64: 2^(23 - e) itself overflows float32 for subnormal rows).  The clamp only ever acts on
 *         +2^23.  v is an integer vector; subnormal rows and rows up to FLT_MAX are in the domain.
 *         Sv = sum v_i, Nv = sum v_i^2: exact int64 values (|Sv| < 2^39, Nv < 2^62).
 *         B_q = 1 / sqrt(K Nv), A_q = Sv B_q, in float64.
 *   pair: D = sum v_i w_i with w = u - 128, exact, from three int32 accumulators of int8 digit planes of v against
 *         the corpus's signed bytes.  Digits here: bytes 1 and 0 of the two's-complement v with the top bit flipped
 *         (b - 128), byte 2 as it is, so D = 65536 P2 + 256 P1 + P0 + 32896 S_c, |P_j| <= 2^30 for K <= 65536 (the
 *         encoding is the implementation's choice; the definition of v is not).
 *         t = K D - Sv S_c, the exact integer (|t| <= 2^62, each term up to 2^62: 64-bit integer arithmetic, since
 *         float64 products round both terms past 2^53 before they cancel; on a frame of one 255 among zeros and a
 *         same-sign query at K = 65536 the float64 t is off by several units, which moves a score by 1e-15, and by
 *         up to 2.4e-13 on a frame of one 1 among zeros), converted to float64 once.
 *         cos = A_q A_c + (B_q B_c) t with the (A_c, B_c, S_c, ok_c) hq_cosq_prepare stores;
 *         score = (cos + 1) / 2, and 0.0 when either ok is 0.
 *   The epilogues are compiled with -ffp-contract=off and use one pair function, so the dense and the fused
 *   route agree bit for bit.  Limits: 1 <= K <= 65536 (larger: HQ_E_UNSUPPORTED), 1 <= k <= 64 in hq_cosqf_topk.
 *   What the score means: it is the cosine of (v, dequantised frame) to a few float64 roundings (a NumPy model of
 *   the formula stays within 3e-16 of the long-double value over K = 1 .. 65536; 1e-13 is tested).  Against the
 *   query's own float32 values, |delta score| <= 2^(e-24) sqrt(K) / |q|: the per-element rounding is at most
 *   2^(e-24), and with 2^e <= 2 amax that is at most 2^-23 sqrt(K) amax / |q| -- below 7e-7 for gaussian and
 *   post-ReLU rows at any K (amax / |q| about 4 / sqrt(K)); the worst adversarial row found reached 3.2e-6 at
 *   K = 65536.
 * hq_cosqf_prepare: X f32 [Q, K] (ld floats between rows) -> Q8: hq_cosqf_padded_rows(Q) x hq_cosq_padded_k(K) x 3
 *   bytes, the three digit planes in the corpus's fragment layout (16-row tile t, K step kb of 64, plane p: the
 *   1 KiB fragment at ((t KB + kb) 3 + p) 1024; lane 16 g + j = row 16 t + j, bytes 64 kb + 16 g .. + 15; a step's
 *   query operands are one contiguous 3 KiB), pad rows and pad K positions 0, and stats f64 [padded rows, 4] =
 *   (A_q, B_q, Sv, ok).  One launch, no host round trip.  16-byte loads when the base is a multiple of 16 bytes and
 *   ld a multiple of 4 floats, element loads otherwise.
 * hq_cosqf_scores: out [Q, N] f64, the dense scores.  B8 / stats_b: hq_cosq_prepare's outputs.
 * hq_cosqf_topk: arguments and semantics of hq_cosq_topk (threshold, thr_mode 0 / 1 / 2, id_base, -inf / -1
 *   padding, 1 <= k <= 64 else HQ_E_UNSUPPORTED, (score descending, id ascending)); the lists equal
 *   hq_select_topk_ws of hq_cosqf_scores bit for bit.  workspace: hq_cosqf_topk_workspace_size(Q, N, k) bytes.
 * Zero Q or N: HQ_OK before any pointer is looked at; negative sizes, K < 1, ld < K, NULL operands: HQ_E_INVALID. */
int64_t hq_cosqf_padded_rows(int64_t Q);
int hq_cosqf_prepare(const float* X, int64_t Q, int64_t ld, int K, void* Q8, double* stats, hq_stream_t stream);
int hq_cosqf_scores(const void* Q8, const double* stats_q, int Q, const void* B8, const double* stats_b, int64_t N,
                    int K, double* out, hq_stream_t stream);
size_t hq_cosqf_topk_workspace_size(int Q, int64_t N, int k);
int hq_cosqf_topk(const void* Q8, const double* stats_q, int Q, const void* B8, const double* stats_b, int64_t N,
                  int K, int k, double threshold, int thr_mode, int64_t id_base,
                  void* workspace, size_t workspace_bytes,
                  double* out_score, int64_t* out_id, hq_stream_t stream);

/* ---- S7: the rest of the RAG scorer (rag/search/engine.py) --------------------------------------
 * hq_cosine_scores_dt: as hq_cosine_scores for float32 (HQ_F32) or float64 (HQ_F64) rows; float64
 *   inputs are not narrowed (engine.py:622-660 computes in the input dtype).
 * hq_detect_heights: _detect_original_embedding_height (engine.py:134-162) of N images [N, H, W]: the
 *   first row from the bottom with fewer than half zeros ends the original embedding (height = row + 1,
 *   H when none) -> out int32 [N].  _extract_original_embedding (:604-620) is the image's first rows.
 * hq_spatial_locality: _calculate_spatial_locality_similarity (engine.py:662-714) of every query image
 *   q [Q, H, W] against every stored image c [N, H, W] -> out f64 [Q, N]: original heights detected on
 *   both (different -> 0.0), ws = min(4, h / 4, W / 4), one cosine over the block when ws < 2, else the
 *   mean (NumPy pairwise order) of the (cos + 1) / 2 of ws x ws windows at stride ws / 2.  H * W <= 8192.
 * hq_threshold_select: _apply_progressive_threshold (engine.py:243-287) for Q rows of candidate scores
 *   [Q, N] in the caller's order: the first `cap` candidates with score >= threshold -> out_ids [Q, cap]
 *   (ids[q, i] when ids is given, else the position i; -1 padded), out_count [Q].  The caller computes
 *   the level's threshold and cap exactly as the reference (Python float arithmetic).  A NaN score never
 *   passes.  cap = 0: every out_count[q] is written as 0 and out_ids, which then has no columns, is neither
 *   read nor written (it may be NULL).
 * hq_cosine_scores / hq_cosine_scores_dt with K = 0: every score is 0.0 (both norms are 0); a and b are not
 *   read and may be NULL.                                                                            */
int hq_cosine_scores_dt(int dtype, const void* a, int Q, const void* b, int64_t N, int K, double* out,
                        hq_stream_t stream);
int hq_detect_heights(int dtype, const void* imgs, int64_t N, int H, int W, int* out, hq_stream_t stream);
int hq_spatial_locality(int dtype, const void* q, int Q, const void* c, int64_t N, int H, int W, double* out,
                        hq_stream_t stream);
int hq_threshold_select(const double* scores, const int64_t* ids, int Q, int64_t N, double threshold, int64_t cap,
                        int64_t* out_ids, int64_t* out_count, hq_stream_t stream);

/* ---- S7: the comprehensive frame similarity (rag/search/engine.py:478-727, hq_comp.hip) -----------
 * score = 0.5 hierarchical + 0.3 embedding + 0.2 spatial of two enhanced frames [H, W] (float32 or float64):
 * hierarchical = compare_hierarchical_indices of the frames' non-zero index rows (the rows below the detected
 * height, all-zero rows dropped, zero-padded to M = max(L_q, L_c) levels, weights of M levels; 0.0 when a frame
 * has none), embedding = the cosine of the original blocks (flattened, truncated to the common length), spatial =
 * hq_spatial_locality's windowed cosine.
 * hq_comp_describe: per frame desc[4 i ..] = (h, L, width, row_mask): detected height, number of non-zero rows
 *   among h .. H - 1, their largest length without trailing zeros, their bit set (bit r - h).  One launch.  A
 *   frame with more than 31 rows below its height: HQ_E_UNSUPPORTED (its L is written as -1; for H > 32 the call
 *   reads one flag back and synchronises the stream).
 * hq_comp_scores: out [Q, N] f64 = the score of every pair from the frames and their descriptors (heights are
 *   not detected again); parts [Q, N, 3] (or NULL) = the three components.  weights: the host table of
 *   calculate_granularity_weights, (max_levels + 1) rows of max_levels, row M = the weights of M levels; every
 *   max(L_q, L_c) must be <= max_levels (a pair above it gets a NaN hierarchical part).  The caller checks that
 *   pairs with L_q, L_c >= 1 share `width` (the reference raises ValueError otherwise).  One wave per pair, the
 *   query frame staged in LDS: (5 max_windows + H W) values must fit 160 KiB.  |err| < 1e-12 for float64 frames,
 *   < 1e-6 against the reference's float32 arithmetic.
 * hq_comp_layout: the composite row of profile (h, L = H - h): returns its length K (< 0: error) and, when out
 *   is not NULL, out[12] = (K, L, ws (0 when < 2), stride, windows down, windows across, and the offsets of the
 *   sections in row order: the windows, the original block, the levels, the constant column, the block's
 *   indicator, the windows' indicators).  hq_comp_padded_k = K rounded up as hq_cos_padded_k rounds.
 * hq_comp_prepare: float32 frames imgs [N, H, W] (frame stride ld) of that profile (the caller has checked
 *   desc == (h, H - h, ., full mask)) -> composite rows in hq_cos_prepare's tiled layout: X16 of
 *   hq_cos_padded_rows(N) x 2 x hq_comp_padded_k halves and inv [hq_cos_padded_rows(N)].  level_coef[l] =
 *   sqrt(0.5 w_l / sum w) for the H - h levels; side 0 = queries, 1 = corpus (the constant column).  Rows are
 *   stored unscaled (every entry is at most 1), inv = 1 (0 for a pad row and for a frame holding a NaN or inf: it
 *   scores 0.0), so
 *   hq_cos_scores_mfma / _f32 / hq_cos_topk on two such operands return the comprehensive score (within 1e-5;
 *   profiles/comp_error_bounds.txt has the measured error, up to K = 20,627).  A tile's 16 frames keep one float64
 *   coefficient per section in LDS: 16 (H - h + 1 + n_windows) values must fit 160 KiB, i.e. at most
 *   1279 - (H - h) windows (67 x 64 frames: 961).  A profile beyond that, such as the RAG generator's 131 x 128
 *   frames (3969 windows, K = 84,243), is HQ_E_UNSUPPORTED: it cannot be fused, and since hq_comp_scores cannot
 *   stage such a frame either, callers refuse it (ComprehensiveFrameCorpus passes the message on).
 * hq_comp_scores_listed: the same score through an id list.  ids int64 [Q, C], out f64 [Q, C], parts [Q, C, 3] or
 *   NULL: out[a, j] is the value hq_comp_scores writes for the pair (query a, frame ids[a, j]), bit for bit,
 *   whatever N, C or the entry's position (both kernels call one per-pair device function).  An entry with
 *   ids[a, j] < 0 or >= N is a pad: out = -inf, its parts are 0.0, and no frame is read for it.  Repeated ids are
 *   allowed and are scored independently.  No frames are copied: the kernel reads c + id H W.  LDS rule, refusal
 *   message and argument checks are hq_comp_scores' (c and desc_c may be NULL when N = 0: every entry is a pad);
 *   Q = 0 or C = 0 returns HQ_OK before any pointer is looked at.  One launch, no host synchronisation.
 * hq_list_topk: scores f64 [Q, C] and ids int64 [Q, C] -> the first k entries of every row in (score descending,
 *   list position ascending) order: out_score / out_id [Q, k], padded with -inf / -1, out_count int32 [Q] = the
 *   number written.  An entry is eligible when its id is >= 0, its score is not NaN, and it passes thr_mode (0
 *   none, 1 >=, 2 >, as hq_select_topk).  -0.0 and 0.0 compare equal, so position decides between them.  This is
 *   the reference's stable sort by score over a list whose order carries meaning (the cascade's), then the
 *   threshold and the cut; hq_select_topk breaks ties by id and does not specify NaN.  1 <= C <= 1024 and 1 <= k,
 *   anything beyond is HQ_E_UNSUPPORTED.  One workgroup per query, O(C^2) rank counting in LDS, one launch.
 * hq_list_windows: heads int64 [Q, C0] (-1 allowed anywhere) -> out int64 [Q, C0 window]: each head f >= 0 widened
 *   to its window of consecutive frames (FrameCacheManager.cache_consecutive_frames, rag/search/frame_cache.py:
 *   66-72): half = window / 2, start = max(0, f - half), end = min(start + window, f + half + 1), frames start ..
 *   end - 1, those >= N dropped.  The row is the windows' frames in head order, each window ascending, keeping only
 *   a frame's first appearance, compacted to the front and -1 padded; out_count int32 [Q] = its length.  window = 1
 *   returns the heads, deduplicated.  1 <= window <= 64 and C0 window <= 1024, anything else is HQ_E_UNSUPPORTED.
 *   One workgroup per query, one launch.                                                                       */
int hq_comp_describe(int dtype, const void* imgs, int64_t N, int H, int W, int32_t* desc, hq_stream_t stream);
int hq_comp_scores(int dtype, const void* q, const int32_t* desc_q, int Q, const void* c, const int32_t* desc_c,
                   int64_t N, int H, int W, const double* weights, int max_levels, double* out, double* parts,
                   hq_stream_t stream);
int hq_comp_scores_listed(int dtype, const void* q, const int32_t* desc_q, int Q, const void* c, const int32_t* desc_c,
                          int64_t N, int H, int W, const int64_t* ids, int C, const double* weights, int max_levels,
                          double* out, double* parts, hq_stream_t stream);
int hq_list_topk(const double* scores, const int64_t* ids, int Q, int C, int k, double threshold, int thr_mode,
                 double* out_score, int64_t* out_id, int32_t* out_count, hq_stream_t stream);
int hq_list_windows(const int64_t* heads, int Q, int C0, int64_t N, int window, int64_t* out, int32_t* out_count,
                    hq_stream_t stream);
int hq_comp_layout(int H, int W, int h, int32_t* out);
int hq_comp_padded_k(int H, int W, int h);
int hq_comp_prepare(const float* imgs, int64_t N, int64_t ld, int H, int W, int h, int side, const double* level_coef,
                    void* X16, double* inv, hq_stream_t stream);

/* ---- S7: the progressive hierarchical search (rag/search/engine.py:51-95, 178-287, hq_hier.hip) ---
 * The candidate cascade the engine runs before the comprehensive score, for a query batch against a prepared,
 * resident corpus.  A frame's levels are its non-zero index rows below the detected height, in order (all-zero rows
 * dropped, later rows move up), each cut after its last non-zero value.  Level score s_l(q, c), l < L_q: 0.0 when c
 * has no level l, else (cos + 1) / 2 over the first min(len_q, len_c) values of the two rows, 0.0 when either
 * truncated norm is 0; float64 sums in element order, so bit-identical frames score bit-identically.  At level l the
 * survivors (every frame at level 0) are ordered by (s_l desc, s_{l-1} desc, ..., s_0 desc, id asc) — what the
 * reference's stable sort per level amounts to — and the first cap_l = max(1, (int64)(n_prev * ratio[l])) of those
 * with s_l >= thr[l] survive (n_prev: survivors entering the level, N at level 0).  A NaN score never passes.
 * hq_hier_prepare: frames imgs [N, H, W] (float32 / float64, frame stride ld) and their hq_comp_describe
 *   descriptors -> rows f64 [N, max_levels, W] (zero beyond each length and for missing levels) and lens int32
 *   [N, max_levels] (0: no such level).  One launch.  1 <= max_levels <= 8; a frame with more non-zero index rows:
 *   HQ_E_UNSUPPORTED (for H - 1 > max_levels the call reads one flag back and synchronises the stream).
 * hq_hier_workspace_size: bytes hq_hier_filter needs: max_levels * Q * N float64 scores and Q * N bytes.
 * hq_hier_filter: Lq int32 [Q] = the queries' level counts; thr, ratio: host tables of max_levels doubles.  Two
 *   launches (all level scores; one workgroup per query for the cuts and the list head), no host round trip.
 *   out_count [Q, max_levels] int64: survivors after each level, 0 for the levels the cascade did not run (l >= L_q,
 *   or nobody was left).  out_top_ids [Q, kout] int64: the first kout of the final list in its order, -1 padded;
 *   out_top_scores [Q, kout, max_levels]: their level scores (0.0 for l >= L_q and for pad entries).  out_alive
 *   [Q, N] uint8 (NULL allowed): the number of levels each frame survived (the final list: == L_q).  A query with
 *   L_q = 0 returns nothing; one with L_q > max_levels returns nothing either (no frame has level max_levels), its
 *   counts are those of the max_levels levels run.  kout <= 64, W <= 512 (HQ_E_UNSUPPORTED beyond).  Q = 0 or N = 0:
 *   returns 0 and writes only counts.                                                                        */
int hq_hier_prepare(int dtype, const void* imgs, int64_t N, int64_t ld, int H, int W, const int32_t* desc,
                    int max_levels, double* rows, int32_t* lens, hq_stream_t stream);
size_t hq_hier_workspace_size(int Q, int64_t N, int max_levels);
int hq_hier_filter(const double* q_rows, const int32_t* q_lens, const int32_t* Lq, int Q, const double* c_rows,
                   const int32_t* c_lens, int64_t N, int W, int max_levels, const double* thr, const double* ratio,
                   int kout, void* ws, int64_t* out_count, int64_t* out_top_ids, double* out_top_scores,
                   uint8_t* out_alive, hq_stream_t stream);

/* ---- §8e: the sharded search's one collective (RCCL over xGMI) ----------------------------------
 * The corpus is split into contiguous global-id ranges, one per GPU (one process per GPU); each rank
 * answers the whole query batch against its shard and packs fixed-size top-k records, and ONE
 * all-gather lets every rank merge them with hq_progressive_final (the reference's analogue: the
 * thread fan-out + list-concatenation merge of core/video_search.py:722-875).
 * hq_comm_unique_id: rank 0 creates the communicator id (HQ_COMM_ID_BYTES opaque bytes) and hands it
 *   to every rank out of band (hq_mi355x.distributed uses the torch.distributed store / broadcast);
 * hq_comm_init_rank: collective over the nranks processes, on the calling thread's current HIP device;
 * hq_allgather_topk: recv [nranks x bytes] = every rank's send [bytes], in rank order, on `stream`;
 *   bytes must be equal on all ranks.  Asynchronous like every other entry point.                   */
#define HQ_COMM_ID_BYTES 128
int hq_comm_unique_id(void* id_out);
int hq_comm_init_rank(void** comm, int nranks, const void* id, int rank);
int hq_comm_size(void* comm, int* nranks, int* rank);
int hq_comm_destroy(void* comm);
int hq_allgather_topk(void* comm, const void* send, void* recv, size_t bytes, hq_stream_t stream);

#ifdef __cplusplus
}
#endif
#endif /* HQ_MI355X_H */
