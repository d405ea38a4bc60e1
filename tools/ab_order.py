#!/usr/bin/env python3
"""Greedy frame ordering: FrameOrdering.greedy_order (hq_order_greedy: one f64 MFMA similarity matrix, the start
row, then the chain walked by one resident workgroup) against the route the library offered before it: per step one
hq_pearson_f64 launch of the last row against all rows, the scores copied to the host, a NumPy masked arg-max
(written to profiles/order_vs_per_step.txt).

Rows are resident on the device for both routes.  Every variant runs after a warm-up call; the device route between
two HIP events around as many back-to-back calls as fill --window seconds (time per call = window / calls), the
per-step route (which ends every step in a device-to-host copy) on the host clock around a final synchronise; the
two alternate inside each repetition.  The file gives medians with the spread (min - max),
the similarity matrix alone (hq_order_sims into a preallocated matrix) and from it the time per chain step,
(greedy - matrix) / (N - 1).  The per-step route runs whole unless --slice S is given: then its first S steps are
timed and scaled by (N - 1) / S (every step costs the same: one launch over all N rows, one copy of N scores), and
the file says so.  The two orders are compared.

usage: ab_order.py [--out FILE] [--sizes 1000 10000] [--L 64] [--reps 10] [--window 0.2] [--slice 0]
Needs an MI355X."""
import argparse
import os
import statistics
import sys
import time

ap = argparse.ArgumentParser()
ap.add_argument("--out", default=None)
ap.add_argument("--sizes", type=int, nargs="+", default=[1000, 10000])
ap.add_argument("--L", type=int, default=64)
ap.add_argument("--reps", type=int, default=10)
ap.add_argument("--window", type=float, default=0.2, help="seconds of device work per timed window")
ap.add_argument("--slice", type=int, default=0, help="per-step route: time this many steps and scale (0 = all)")
args = ap.parse_args()
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "hilbert-quantization_amd")]

import numpy as np  # noqa: E402
import torch  # noqa: E402
from hq_mi355x import kernels as K  # noqa: E402
from hq_mi355x.core.frame_order import FrameOrdering  # noqa: E402

assert torch.cuda.is_available(), "ab_order.py needs the GPU"
OUT = args.out or os.path.join(ROOT, "profiles", "order_vs_per_step.txt")
LINES = []


def say(s=""):
    print(s, flush=True)
    LINES.append(s)


def events(fn, calls=1):
    """Seconds per call of `calls` back-to-back calls between two HIP events."""
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(calls):
        fn()
    e1.record()
    e1.synchronize()
    return e0.elapsed_time(e1) * 1e-3 / calls


def calls_for(fn):
    """Calls that fill the timed window, from one timed call after the warm-up."""
    return max(1, int(args.window / max(events(fn), 1e-7)))


def per_step(rows, start, steps):
    """The chain by one hq_pearson_f64 launch and one host arg-max per step -> (seconds, order of steps + 1 rows)."""
    N = rows.shape[0]
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    left = np.ones(N, bool)
    left[start] = False
    order = [start]
    for _ in range(steps):
        s = K.pearson_f64(rows[order[-1]], rows).cpu().numpy()
        b = int(np.argmax(np.where(left, s, -1.0)))
        left[b] = False
        order.append(b)
    torch.cuda.synchronize()
    return time.perf_counter() - t0, order


def spread(ts, unit=1e3):
    return f"median {statistics.median(ts) * unit:10.3f} ms  (min {min(ts) * unit:10.3f} - max {max(ts) * unit:10.3f})"


def main():
    say(f"== greedy frame ordering, {torch.cuda.get_device_name(0)}: gaussian index rows, L = {args.L}, "
        f"{args.reps} repetitions after one warm-up call, routes alternating ==")
    say("(a) FrameOrdering.greedy_order: hq_order_greedy (similarity matrix + start row + chain walk), HIP events")
    say("(b) per step: hq_pearson_f64 of the last row against all rows, copy to the host, masked arg-max; host clock")
    for N in args.sizes:
        rng = np.random.default_rng(N)
        x = rng.standard_normal((N, args.L)) + 3.0 * rng.uniform(-1, 1, (N, 1))
        fo = FrameOrdering(x)
        rows = fo.rows.X
        steps = N - 1 if args.slice <= 0 else min(args.slice, N - 1)
        S = torch.empty((N, N), dtype=torch.float64, device=rows.device)
        r = fo.rows

        def sims():
            K._chk(K._L().hq_order_sims(K.ptr(r.Z), K.ptr(r.flags), K.ptr(r.X), r.L, N, K.ptr(r.Z), K.ptr(r.flags),
                                        K.ptr(r.X), r.L, N, r.L, K.ptr(S), N, K.stream()))

        order = fo.greedy_order()[0].cpu().numpy()            # the warm-up calls
        sims()
        _, ref = per_step(rows, int(order[0]), min(steps, 50))
        ca, cm = calls_for(fo.greedy_order), calls_for(sims)
        ta, tb, tm = [], [], []
        for _ in range(args.reps):
            ta.append(events(fo.greedy_order, ca))
            tm.append(events(sims, cm))
            tb_, ref = per_step(rows, int(order[0]), steps)
            tb.append(tb_ * (N - 1) / steps)
        ma, mb, mm = statistics.median(ta), statistics.median(tb), statistics.median(tm)
        say(f"-- N = {N}: {ca} chain calls and {cm} matrix calls per timed window")
        say(f"  (a) device chain     {spread(ta)}")
        say(f"      matrix alone     {spread(tm)}   ({2.0 * N * N * args.L / mm * 1e-12:.2f} TFLOP/s f64 from shapes"
            f"{'; launch and latency dominate at this size: not a kernel rate' if mm < 1e-4 else ''})")
        say(f"      per chain step   {(ma - mm) / (N - 1) * 1e6:10.3f} us  = (chain - matrix) / (N - 1), start row included")
        how = "run whole" if steps == N - 1 else f"first {steps} steps timed, scaled by (N - 1) / {steps}"
        say(f"  (b) per-step route   {spread(tb)}   ({how}; {mb / (N - 1) * 1e6:.1f} us per step)")
        say(f"      (b) / (a) = {mb / ma:.1f}x; first {len(ref)} rows of the two orders equal: "
            f"{ref == order[:len(ref)].tolist()}")
        del S, fo
        torch.cuda.empty_cache()
    os.makedirs(os.path.dirname(OUT), exist_ok=True)
    with open(OUT, "w") as f:
        f.write("\n".join(LINES) + "\n")


if __name__ == "__main__":
    main()
