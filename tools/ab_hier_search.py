#!/usr/bin/env python3
"""The engine's search workflow: HierarchicalFrameCorpus.search (the batch on the device: hq_hier_filter, hq_list_windows
when window > 0, hq_comp_scores_listed, hq_list_topk) against its per-query route (_search_per_query: the list heads
copied to the host, then per query a gather of the raw frames, one hq_comp_scores launch and a NumPy sort), device
resident, one process (written to profiles/hier_search_vs_per_query.txt).

Every variant runs between two HIP events after a warm-up call, the two routes alternate inside each repetition; the
file gives medians with the spread (min - max).  The lists of the two routes are compared on every timed query: ids
and score bits.

usage: ab_hier_search.py [--out FILE] [--queries 1 1000] [--windows 0 10] [--k 10] [--reps 5]
                         [--shapes 32:250000 64:50000]
Needs an MI355X."""
import argparse
import os
import statistics
import sys

ap = argparse.ArgumentParser()
ap.add_argument("--out", default=None)
ap.add_argument("--queries", type=int, nargs="+", default=[1, 1000])
ap.add_argument("--windows", type=int, nargs="+", default=[0, 10])
ap.add_argument("--k", type=int, default=10)
ap.add_argument("--reps", type=int, default=5)
ap.add_argument("--clusters", type=int, default=4)
ap.add_argument("--shapes", type=str, nargs="+", default=["32:250000", "64:50000"], help="n:N (n x n images)")
args = ap.parse_args()
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "hilbert-quantization_amd")]

import torch  # noqa: E402
from hq_mi355x.rag import similarity as S  # noqa: E402

assert torch.cuda.is_available(), "ab_hier_search.py needs the GPU"
OUT = args.out or os.path.join(ROOT, "profiles", "hier_search_vs_per_query.txt")
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


def main():
    k = args.k
    say(f"== engine search workflow, {torch.cuda.get_device_name(0)}: k = {k} (2 k = {2 * k} candidates), "
        f"threshold 0.1, {args.reps} repetitions after one warm-up call, HIP events, routes alternating ==")
    say("(a) HierarchicalFrameCorpus.search: the batch on the device, launches and host copies independent of Q")
    say("(b) _search_per_query: per query a frame gather, one hq_comp_scores launch, a host sort")
    for spec in args.shapes:
        n, N = (int(v) for v in spec.split(":"))
        g = torch.Generator(device="cuda").manual_seed(0)
        centres = torch.randn((args.clusters, n, n), generator=g, dtype=torch.float32, device="cuda")
        frames = torch.cat([enhance(
            centres[torch.randint(0, args.clusters, (min(50000, N - i),), generator=g, device="cuda")] +
            torch.randn((min(50000, N - i), n, n), generator=g, dtype=torch.float32, device="cuda"))
            for i in range(0, N, 50000)])
        Qmax = max(args.queries)
        pick = torch.randint(0, N, (Qmax,), generator=g, device="cuda")
        queries = enhance(frames[pick, :n] + 0.5 * torch.randn((Qmax, n, n), generator=g, dtype=torch.float32,
                                                                device="cuda"))
        corpus = S.HierarchicalFrameCorpus(frames)
        say(f"-- frames {frames.shape[1]} x {n}, N = {N}")
        for w in args.windows:
            for Q in args.queries:
                qs = queries[:Q]
                fa = lambda: corpus.search(qs, k, 0.1, window=w)                  # noqa: E731
                fb = lambda: corpus._search_per_query(qs, k, 0.1, window=w)       # noqa: E731
                (sa, ia), (sb, ib) = fa(), fb()                                   # the warm-up calls
                same = bool(torch.equal(ia, ib)) and bool(torch.equal(sa.view(torch.int64), sb.view(torch.int64)))
                found = float((ia >= 0).sum()) / Q
                ta, tb = [], []
                for _ in range(args.reps):
                    ta.append(timed(fa))
                    tb.append(timed(fb))
                ma, mb = statistics.median(ta), statistics.median(tb)
                say(f"  window = {w:<2} Q = {Q:<5} (a) batched   median {ma * 1e3:9.3f} ms  (min {min(ta) * 1e3:9.3f} - "
                    f"max {max(ta) * 1e3:9.3f})")
                say(f"  {'':11} {'':9} (b) per query median {mb * 1e3:9.3f} ms  (min {min(tb) * 1e3:9.3f} - "
                    f"max {max(tb) * 1e3:9.3f})   (b) / (a) = {mb / ma:.2f}x")
                say(f"  {'':11} {'':9} lists of the two routes (ids and score bits) equal on all {Q} queries: {same}; "
                    f"{found:.1f} results per query")
        del corpus, frames, queries
        torch.cuda.empty_cache()
    os.makedirs(os.path.dirname(OUT), exist_ok=True)
    with open(OUT, "w") as f:
        f.write("\n".join(LINES) + "\n")


if __name__ == "__main__":
    main()
