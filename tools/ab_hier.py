#!/usr/bin/env python3
"""Progressive hierarchical search: HierarchicalFrameCorpus.filter against the route a user had before hq_hier.hip,
device resident, one process (written to profiles/hier_vs_unfused.txt).

(a)  HierarchicalFrameCorpus.filter: hq_comp_describe + hq_hier_prepare of the queries + hq_hier_filter on the
     resident packed rows, the whole query batch (split under the default 1 GiB workspace);
(b)  the unfused route: the store's index rows extracted once (not timed with the queries), then per query and level
     the query's row extracted on the host, cosine_scores_dt against the surviving rows, a stable torch sort,
     hq_threshold_select (progressive_threshold_batch), the count read back, the survivors gathered for the next
     level.  It runs on --unfused-q queries and its time is scaled to the whole batch by the query count; the file
     says so next to the number.
(s)  HierarchicalFrameCorpus.search (k = 10: the cascade, then hq_comp_scores on the first 20 candidates, one scoring
     launch per query) on --search-q queries, reported per query.
Every variant runs between two HIP events after a warm-up call, the variants alternate inside each repetition.

usage: ab_hier.py [--out FILE] [--queries 1000] [--reps 5] [--shapes 32:250000 64:50000]
Needs an MI355X."""
import argparse
import os
import statistics
import sys

ap = argparse.ArgumentParser()
ap.add_argument("--out", default=None)
ap.add_argument("--queries", type=int, default=1000)
ap.add_argument("--kout", type=int, nargs="+", default=[20, 64])
ap.add_argument("--reps", type=int, default=5)
ap.add_argument("--unfused-q", type=int, default=100)
ap.add_argument("--search-q", type=int, default=100)
ap.add_argument("--clusters", type=int, default=4)
ap.add_argument("--shapes", type=str, nargs="+", default=["32:250000", "64:50000"], help="n:N (n x n images)")
args = ap.parse_args()
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "hilbert-quantization_amd")]

import numpy as np  # noqa: E402
import torch  # noqa: E402
from hq_mi355x import kernels as K  # noqa: E402
from hq_mi355x._dev import to_np  # noqa: E402
from hq_mi355x.rag import similarity as S  # noqa: E402

assert torch.cuda.is_available(), "ab_hier.py needs the GPU"
OUT = args.out or os.path.join(ROOT, "profiles", "hier_vs_unfused.txt")
LINES = []
GRAN = {8: (2,), 16: (4, 2), 32: (4, 2), 64: (8, 4, 2)}   # the RAG generator's index rows, finest first


def say(s=""):
    print(s, flush=True)
    LINES.append(s)


def enhance(img):
    """[M, n, n] float32 images -> [M, n + rows, n] enhanced frames (block means per granularity, one row each)."""
    M, n, _ = img.shape
    rows = []
    for g in GRAN[n]:
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


def store_levels(frames):
    """The store's levels for the unfused route, once: per level the trimmed rows [N, len] on the device (a store
    written by one generator: every frame the same heights and lengths, checked)."""
    desc = to_np(K.comp_describe(frames))
    assert (desc == desc[0]).all(), "the unfused route of this tool takes a uniform store"
    h, L = int(desc[0, 0]), int(desc[0, 1])
    out = []
    for l in range(L):
        row = frames[:, h + l]
        length = int((row != 0).any(dim=0).nonzero().max()) + 1
        out.append(row[:, :length].contiguous())
    return out


def query_levels(q):
    """engine.py:97-162 on one host frame."""
    H, W = q.shape
    h = H
    for r in range(H - 1, -1, -1):
        if np.sum(q[r] == 0) / W < 0.5:
            h = r + 1
            break
    rows = []
    for r in range(h, H):
        nz = np.nonzero(q[r])[0]
        if len(nz):
            rows.append(q[r, :nz[-1] + 1])
    return rows


def unfused(queries_host, levels):
    """The candidate lists of the queries, one query and one level at a time."""
    lists = []
    dev = levels[0].device
    for q in queries_host:
        cand = None
        for l, qrow in enumerate(query_levels(q)):
            if l >= len(levels):
                cand = cand[:0]
                break
            rows = levels[l] if cand is None else levels[l][cand]
            m = min(len(qrow), rows.shape[1])
            s = K.cosine_scores_dt(torch.as_tensor(qrow[None, :m], device=dev), rows[:, :m].contiguous())
            order = torch.sort(s[0], descending=True, stable=True).indices
            ids = order if cand is None else cand[order]
            out, cnt = S.progressive_threshold_batch(s[0][order][None], l, ids[None])
            cand = out[0, :int(cnt[0])]
            if not len(cand):
                break
        lists.append(cand if cand is not None else torch.zeros(0, dtype=torch.int64, device=dev))
    return lists


def main():
    Q = args.queries
    say(f"== progressive hierarchical search, {torch.cuda.get_device_name(0)}: {Q} queries, {args.reps} repetitions "
        f"after one warm-up call, HIP events, variants alternating ==")
    say("(a) HierarchicalFrameCorpus.filter (describe + prepare of the queries + hq_hier_filter), whole batch")
    say(f"(b) unfused: per query and level host extraction + cosine_scores_dt + stable sort + hq_threshold_select, on "
        f"{args.unfused_q} queries, SCALED to {Q} queries by the query count")
    say(f"(s) HierarchicalFrameCorpus.search, k = 10, on {args.search_q} queries, per query")
    for spec in args.shapes:
        n, N = (int(v) for v in spec.split(":"))
        g = torch.Generator(device="cuda").manual_seed(0)
        centres = torch.randn((args.clusters, n, n), generator=g, dtype=torch.float32, device="cuda")
        frames = torch.cat([enhance(
            centres[torch.randint(0, args.clusters, (min(50000, N - i),), generator=g, device="cuda")] +
            torch.randn((min(50000, N - i), n, n), generator=g, dtype=torch.float32, device="cuda"))
            for i in range(0, N, 50000)])
        pick = torch.randint(0, N, (Q,), generator=g, device="cuda")
        queries = enhance(frames[pick, :n] + 0.5 * torch.randn((Q, n, n), generator=g, dtype=torch.float32,
                                                                device="cuda"))
        t_prep = timed(lambda: S.HierarchicalFrameCorpus(frames, keep_frames=False))
        corpus = S.HierarchicalFrameCorpus(frames)
        packed = corpus.resident_bytes - frames.numel() * 4 - 16 * N
        t_old_prep = timed(lambda: store_levels(frames))
        levels = store_levels(frames)
        uq = min(args.unfused_q, Q)
        q_host = to_np(queries[:uq])
        say(f"-- frames {frames.shape[1]} x {n}, N = {N}: {corpus.max_levels} levels of lengths "
            f"{[int(x.shape[1]) for x in levels]}; packed rows {packed} B = {packed / N:.0f} B per frame against "
            f"{frames.numel() * 4 // N} B per raw float32 frame")
        say(f"   one-off: describe + hq_hier_prepare of the store {t_prep * 1e3:.1f} ms; the unfused route's row "
            f"extraction {t_old_prep * 1e3:.1f} ms")
        want = unfused(q_host, levels)
        ids, _, counts = corpus.filter(queries, 64)
        ids, counts = to_np(ids), to_np(counts)
        same = sum(int(np.array_equal(ids[a][ids[a] >= 0], to_np(want[a])[:64])) for a in range(uq))
        final = counts[:, -1]   # every query has the store's level count
        say(f"   lists: mean survivors per level {counts.mean(axis=0).round(1).tolist()}, final list length min "
            f"{int(final.min())} / median {int(np.median(final))} / max {int(final.max())}; first 64 places equal to the "
            f"unfused route's list on {same} of {uq} queries")
        fb = lambda: unfused(q_host, levels)                                                  # noqa: E731
        fns = [(f"a{k}", (lambda k=k: corpus.filter(queries, k)), 1.0) for k in args.kout] + [("b", fb, Q / uq)]
        ts = {key: [] for key, _, _ in fns}
        for key, fn, _ in fns:
            fn()
        for _ in range(args.reps):
            for key, fn, scale in fns:
                ts[key].append(timed(fn) * scale)
        med = {key: statistics.median(v) for key, v in ts.items()}
        for k in args.kout:
            key = f"a{k}"
            say(f"  (a) filter, kout = {k:<3} measured  median {med[key]:9.4f} s  (min {min(ts[key]):9.4f} - max "
                f"{max(ts[key]):9.4f})")
        say(f"  (b) unfused, scaled             median {med['b']:9.4f} s  (min {min(ts['b']):9.4f} - max "
            f"{max(ts['b']):9.4f})")
        say("  (b) / (a): " + "   ".join(f"kout = {k}: {med['b'] / med[f'a{k}']:.1f}x" for k in args.kout))
        sq = min(args.search_q, Q)
        corpus.search(queries[:sq], 10)
        tsr = [timed(lambda: corpus.search(queries[:sq], 10)) / sq for _ in range(args.reps)]
        say(f"  (s) search, k = 10, per query   median {statistics.median(tsr) * 1e3:9.4f} ms (min {min(tsr) * 1e3:9.4f} - "
            f"max {max(tsr) * 1e3:9.4f})")
        del corpus, frames, queries, levels
        torch.cuda.empty_cache()
    os.makedirs(os.path.dirname(OUT), exist_ok=True)
    with open(OUT, "w") as f:
        f.write("\n".join(LINES) + "\n")


if __name__ == "__main__":
    main()
