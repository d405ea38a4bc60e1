#!/usr/bin/env python3
"""Comprehensive frame ranking: the fused composite route against the unfused and the exact routes, and the fused
route's error, device resident, one process.

timing (--what timing, written to profiles/comp_vs_unfused.txt):
(a)  ComprehensiveFrameCorpus.search: hq_comp_describe + hq_comp_prepare of the queries + hq_cos_topk on the
     resident composite operand;
(b)  the exact route: hq_comp_describe of the queries + hq_comp_scores ([Q, N] float64) + hq_select_topk;
(c)  the unfused route, what the reference's ranking cost before hq_comp.hip: spatial_locality_scores (one
     workgroup per pair, heights detected per pair) + the embedding cosine + one cosine per index level, combined
     on the device, + hq_select_topk.
(b) and (c) need the dense matrices and (c) one workgroup per pair, so they run on a slice of the problem (--exact-q
queries; --unfused-q queries x --unfused-n frames) and their times are scaled to Q x N by the pair count; the file
says so next to every scaled number.  Every variant runs between two HIP events after a warm-up call.

errors (--what errors, written to profiles/comp_error_bounds.txt): the largest and the mean |fused - exact| per
row family (gaussian, same-sign, near-duplicate, negated: queries that are the negation of a stored frame) and shape:
the RAG generator's four square profiles, then hand-built profiles (H, W, h) that reach the other window geometries
(ws < 2 with index rows, ws 3 at stride 1, odd and wide W, 31 index rows), and a line for the generator's 131 x 128
frames, which hq_comp_prepare does not take.

usage: ab_comp.py --what timing|errors [--out FILE] [--queries 1000] [--reps 3]
Needs an MI355X."""
import argparse
import os
import statistics
import sys

ap = argparse.ArgumentParser()
ap.add_argument("--what", choices=("timing", "errors"), required=True)
ap.add_argument("--out", default=None)
ap.add_argument("--queries", type=int, default=1000)
ap.add_argument("--k", type=int, nargs="+", default=[10, 64])
ap.add_argument("--reps", type=int, default=3)
ap.add_argument("--exact-q", type=int, default=50)
ap.add_argument("--unfused-q", type=int, default=4)
ap.add_argument("--unfused-n", type=int, default=20000)
ap.add_argument("--shapes", type=str, nargs="+", default=["32:250000", "64:50000"], help="n:N (n x n images)")
args = ap.parse_args()
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "hilbert-quantization_amd")]

import torch  # noqa: E402
from hq_mi355x import kernels as K  # noqa: E402
from hq_mi355x.rag import similarity as S  # noqa: E402

assert torch.cuda.is_available(), "ab_comp.py needs the GPU"
OUT = args.out or os.path.join(ROOT, "profiles", "comp_vs_unfused.txt" if args.what == "timing" else
                               "comp_error_bounds.txt")
LINES = []
GRAN = {8: (2,), 16: (4, 2), 32: (4, 2), 64: (8, 4, 2)}   # the RAG generator's index rows, finest first
HEIGHT = {8: 8, 16: 17, 32: 32, 64: 65}                  # detected height of an enhanced n x n frame
# (H, W, h): ws < 2 with index rows; ws 2; ws 3 (stride 1) twice; ws 4; W > 64; odd W; 945 windows; 31 index rows
BUILT_PROFILES = ((6, 4, 4), (9, 8, 8), (13, 12, 12), (15, 16, 14), (18, 16, 17), (12, 100, 10), (20, 65, 17),
                  (35, 128, 32), (40, 8, 9))


def say(s=""):
    print(s, flush=True)
    LINES.append(s)


def enhance(img, gran=None):
    """[M, n, n] float32 images -> [M, n + rows, n] enhanced frames (block means per granularity, one row each)."""
    M, n, _ = img.shape
    rows = []
    for g in gran or GRAN[n]:
        r = torch.zeros((M, n), dtype=img.dtype, device=img.device)
        r[:, :g * g] = img.reshape(M, g, n // g, g, n // g).mean(dim=(2, 4)).reshape(M, g * g)
        rows.append(r)
    return torch.cat([img, torch.stack(rows, dim=1)], dim=1).contiguous()


def timed(fn):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    r = fn()
    e1.record()
    e1.synchronize()
    del r
    return e0.elapsed_time(e1) * 1e-3


def unfused_topk(qs, fr, h, k):
    Q, H, W = qs.shape
    N = fr.shape[0]
    w = S.calculate_granularity_weights(H - h)
    spa = S.spatial_locality_scores(qs, fr)
    emb = K.cosine_scores(qs[:, :h].reshape(Q, -1), fr[:, :h].reshape(N, -1))
    hier = sum(float(w[l] / w.sum()) * K.cosine_scores(qs[:, h + l].contiguous(), fr[:, h + l].contiguous())
               for l in range(H - h))
    return K.select_topk(0.5 * hier + 0.3 * emb + 0.2 * spa, k)[:2]


def exact_topk(qs, fr, k):
    return K.select_topk(S.comprehensive_scores(qs, fr), k)[:2]


def timing():
    Q = args.queries
    say(f"== comprehensive frame ranking, {torch.cuda.get_device_name(0)}: {Q} queries, {args.reps} repetitions after one "
        f"warm-up call, HIP events ==")
    say("(a) ComprehensiveFrameCorpus.search (describe + prepare of the queries + hq_cos_topk), whole problem")
    say(f"(b) comp_scores + select_topk on {args.exact_q} queries x all frames, SCALED to {Q} queries by the pair count")
    say(f"(c) unfused: spatial_locality_scores + embedding cosine + per-level cosines + select_topk on "
        f"{args.unfused_q} queries x {args.unfused_n} frames, SCALED to the whole problem by the pair count")
    for spec in args.shapes:
        n, N = (int(v) for v in spec.split(":"))
        h = HEIGHT[n]
        g = torch.Generator(device="cuda").manual_seed(0)
        frames = torch.cat([enhance(torch.randn((min(50000, N - i), n, n), generator=g, dtype=torch.float32,
                                                device="cuda")) for i in range(0, N, 50000)])
        pick = torch.randint(0, N, (Q,), generator=g, device="cuda")
        qimg = frames[pick, :n] + 0.5 * torch.randn((Q, n, n), generator=g, dtype=torch.float32, device="cuda")
        queries = enhance(qimg)
        corpus = S.ComprehensiveFrameCorpus(frames)
        assert corpus.fused
        raw = frames.numel() * 4
        say(f"-- frames {frames.shape[1]} x {n}, N = {N}: composite K = {corpus.K}; resident {corpus.resident_bytes} B = "
            f"{corpus.resident_bytes / N:.0f} B per frame against {raw // N} B per raw float32 frame "
            f"({corpus.resident_bytes / raw:.2f}x)")
        for k in args.k:
            fa = lambda: corpus.search(queries, k)                                      # noqa: E731
            fb = lambda: exact_topk(queries[:args.exact_q], frames, k)                  # noqa: E731
            fc = lambda: unfused_topk(queries[:args.unfused_q], frames[:args.unfused_n], h, k)  # noqa: E731
            got, want = fa(), fb()
            same = float((got[1][:args.exact_q] == want[1]).double().mean())
            err = float((got[0][:args.exact_q] - want[0]).abs().max())
            scale = {"a": 1.0, "b": Q / args.exact_q, "c": Q * N / (args.unfused_q * args.unfused_n)}
            fc()
            ts = {"a": [], "b": [], "c": []}
            for _ in range(args.reps):
                for key, fn in (("a", fa), ("b", fb), ("c", fc)):
                    ts[key].append(timed(fn) * scale[key])
            med = {key: statistics.median(v) for key, v in ts.items()}
            say(f"k = {k}: fused list vs exact list on the first {args.exact_q} queries: {100 * same:.2f}% of the places "
                f"equal, largest score difference {err:.2e}")
            for key, name in (("a", "(a) fused, measured"), ("b", "(b) exact, scaled"), ("c", "(c) unfused, scaled")):
                say(f"  {name:<22} median {med[key]:10.3f} s  (min {min(ts[key]):10.3f} - max {max(ts[key]):10.3f})")
            say(f"  (c) / (a): {med['c'] / med['a']:.1f}x   (b) / (a): {med['b'] / med['a']:.1f}x   (c) / (b): "
                f"{med['c'] / med['b']:.1f}x")
        del corpus, frames, queries
        torch.cuda.empty_cache()


def errors():
    say(f"== fused composite route against hq_comp_scores, {torch.cuda.get_device_name(0)}: |fused - exact| over "
        f"16 queries x 256 frames per family ==")
    say("# The composite rows are stored unscaled (entries <= 1).  The error is the float32 accumulation of the matrix")
    say("# cores over K / 32 steps; it grows with the partial sum a pair carries, so the row holds the windows first and")
    say("# the columns that are constant for a valid pair (-0.5, +0.3, +0.2) last, next to each other.  The largest")
    say("# errors belong to pairs with a score near 0 (negated frames): the negative partial sums of the window and")
    say("# original-block sections.  The 1e-5 of the tests is the project's contract, these are the measurements.")
    g = torch.Generator(device="cuda").manual_seed(1)
    for n in (8, 16, 32, 64):
        h = HEIGHT[n]

        def rnd(*shape):
            return torch.randn(shape, generator=g, dtype=torch.float32, device="cuda")

        base = rnd(256, n, n)
        fams = {
            "gaussian": (rnd(16, n, n), base),
            "same-sign": (rnd(16, n, n).abs() + 1.0, base.abs() + 1.0),
            "near-duplicate": (base[:1] + 1e-3 * rnd(16, n, n), base[:1] + 1e-3 * rnd(256, n, n)),
            "negated": (-base[:16] + 0.05 * rnd(16, n, n), base),
        }
        for name, (qi, ci) in fams.items():
            qs, fr = enhance(qi), enhance(ci)
            corpus = S.ComprehensiveFrameCorpus(fr)
            assert corpus.fused and corpus.profile[0] == h
            d = (corpus.scores(qs) - S.comprehensive_scores(qs, fr)).abs()
            say(f"frames {fr.shape[1]:>2} x {n:<2} K = {corpus.K:>5}  {name:<15} max {float(d.max()):.3e}  mean "
                f"{float(d.mean()):.3e}")
    say("# hand-built profiles (H x W, detected height h): a gaussian block of h rows, then H - h index rows that are")
    say("# non-zero in their first W / 2 - 1 columns and in the last one")
    for H, W, h in BUILT_PROFILES:

        def rnd(*shape):
            return torch.randn(shape, generator=g, dtype=torch.float32, device="cuda")

        def built(x):
            x = x.clone()
            x[:, h:, max(W // 2, 1) - 1:W - 1] = 0.0
            return x.contiguous()

        base = rnd(256, H, W)
        fams = {
            "gaussian": (rnd(16, H, W), base),
            "same-sign": (rnd(16, H, W).abs() + 1.0, base.abs() + 1.0),
            "near-duplicate": (base[:1] + 1e-3 * rnd(16, H, W), base[:1] + 1e-3 * rnd(256, H, W)),
            "negated": (-base[:16] + 0.05 * rnd(16, H, W), base),
        }
        for name, (qi, ci) in fams.items():
            qs, fr = built(qi), built(ci)
            corpus = S.ComprehensiveFrameCorpus(fr)
            assert corpus.fused and corpus.profile[:2] == (h, H - h), (H, W, h, corpus.profile)
            d = (corpus.scores(qs) - S.comprehensive_scores(qs, fr)).abs()
            say(f"frames {H:>2} x {W:<3} h = {h:<2} K = {corpus.K:>5}  {name:<15} max {float(d.max()):.3e}  mean "
                f"{float(d.mean()):.3e}")
    # the generator's 128 x 128 images: 131 x 128 frames, h = 128, three index rows (g = 8, 4, 2)
    lay = K.comp_layout(131, 128, 128)
    fr = enhance(torch.randn((16, 128, 128), generator=g, dtype=torch.float32, device="cuda"), (8, 4, 2))
    corpus = S.ComprehensiveFrameCorpus(fr)
    say(f"frames 131 x 128 K = {lay['K']}: not measured.  {lay['ni'] * lay['nj']} windows: hq_comp_prepare keeps 16 x "
        f"(L + 1 + windows) float64 coefficients in LDS, {16 * 8 * (lay['L'] + 1 + lay['ni'] * lay['nj'])} B > 160 KiB "
        f"(comp_prepare_fits = {K.comp_prepare_fits(131, 128, 128)}, corpus.fused = {corpus.fused}); hq_comp_scores "
        f"cannot stage the frame either, so the store is refused")


(timing if args.what == "timing" else errors)()
os.makedirs(os.path.dirname(OUT), exist_ok=True)
with open(OUT, "w") as f:
    f.write("\n".join(LINES) + "\n")
print(f"wrote {OUT}")
