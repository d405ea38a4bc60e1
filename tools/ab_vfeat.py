#!/usr/bin/env python3
"""Video features of u8 frames: hq_vfeat_extract against the NumPy model on host threads, and hq_vfeat_scores /
hq_vfeat_scores_listed against the route a user has without them on the same device: torch float64, the three parts
normalised, three matmuls, clamp, weighted sum.  Written to profiles/vfeat_vs_host.txt.

Device variants run between two HIP events after a warm-up call, the routes alternate inside each repetition; the
file gives medians with the spread (min - max).  The host model is timed on --host-frames frames spread over
--threads threads (wall clock) and scaled to the frame count.  The extraction rate is also given as a share of the
6.27 TB/s the project's float4 copy kernel moved, counting the frame bytes read.

With --errors the largest feature and score errors of every frame family of tests/vfeat_cases.py (the float64 model
the tests assert against) are written to profiles/vfeat_error_bounds.txt.

usage: ab_vfeat.py [--out FILE] [--errors] [--reps 5] [--shapes 65x64 33x32] [--frames 100000] [--Q 1000]
                   [--N 250000] [--C 64] [--host-frames 1600] [--threads 16]
Needs an MI355X."""
import argparse
import os
import statistics
import sys
import time
from concurrent.futures import ThreadPoolExecutor

ap = argparse.ArgumentParser()
ap.add_argument("--out", default=None)
ap.add_argument("--errors", action="store_true")
ap.add_argument("--reps", type=int, default=5)
ap.add_argument("--shapes", nargs="+", default=["65x64", "33x32"])
ap.add_argument("--frames", type=int, default=100000)
ap.add_argument("--Q", type=int, default=1000)
ap.add_argument("--N", type=int, default=250000)
ap.add_argument("--C", type=int, default=64)
ap.add_argument("--host-frames", type=int, default=1600)
ap.add_argument("--threads", type=int, default=16)
args = ap.parse_args()
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "hilbert-quantization_amd"), os.path.join(ROOT, "tests")]

import numpy as np  # noqa: E402
import torch  # noqa: E402
import vfeat_cases as V  # noqa: E402
from hq_mi355x import kernels as K  # noqa: E402

assert torch.cuda.is_available(), "ab_vfeat.py needs the GPU"
DEV = torch.device("cuda:0")
COPY_TBS = 6.27
LINES = []


def say(s=""):
    print(s, flush=True)
    LINES.append(s)


def write(path):
    with open(path, "w") as f:
        f.write("\n".join(LINES) + "\n")


def timed(fn):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    r = fn()
    e1.record()
    e1.synchronize()
    return e0.elapsed_time(e1), r


def alternate(routes):
    """{tag: fn} -> ({tag: result of the warm-up call}, {tag: [ms] * reps})"""
    res = {k: fn() for k, fn in routes.items()}
    torch.cuda.synchronize()
    ts = {k: [] for k in routes}
    for _ in range(args.reps):
        for k, fn in routes.items():
            ts[k].append(timed(fn)[0])
    return res, ts


def line(tag, ts):
    return f"  {tag} median {statistics.median(ts):10.3f} ms  (min {min(ts):10.3f} - max {max(ts):10.3f})"


def extraction(H, W):
    gen = torch.Generator(device=DEV).manual_seed(H * 1000 + W)
    fr = torch.randint(0, 256, (args.frames, H, W), dtype=torch.uint8, device=DEV, generator=gen)
    _, ts = alternate({"hq": lambda: K.vfeat_extract(fr)})
    host = fr[:args.host_frames].cpu().numpy()
    with ThreadPoolExecutor(args.threads) as ex:
        t0 = time.perf_counter()
        list(ex.map(lambda part: [V.features(g) for g in part], np.array_split(host, args.threads)))
        th = (time.perf_counter() - t0) * 1e3 * args.frames / len(host)
    med = statistics.median(ts["hq"])
    say(f"-- extraction, {args.frames} frames of {H} x {W}")
    say(line("hq_vfeat_extract            ", ts["hq"]) + f"   {args.frames / med / 1e3:.2f}M frames/s, "
        f"{args.frames * H * W / med / 1e9:.3f} TB/s of frame bytes = {args.frames * H * W / med / 1e9 / COPY_TBS:.3f} "
        f"of the copy kernel's {COPY_TBS} TB/s")
    say(f"  NumPy model, {args.threads} host threads: {th:10.1f} ms scaled from {len(host)} frames   host / hq = {th / med:.0f}x")


def torch_rows(rows):
    """The three parts of rows [R, 64], each scaled to unit norm (zero where the norm is zero)."""
    out = []
    for p, (a, b) in enumerate(((0, 32), (32, 48), (48, 56))):
        n = rows[:, 56 + p:57 + p]
        out.append(torch.where(n > 0, rows[:, a:b] / n, torch.zeros_like(n)))
    return out


def torch_dense(q, c):
    s = None
    for w, a, b in zip(K.VFEAT_WEIGHTS, torch_rows(q), torch_rows(c)):
        t = (a @ b.T).clamp_(min=0).mul_(w)
        s = t if s is None else s.add_(t)
    return s


def torch_listed(q, c, ids):
    s = None
    for w, a, b in zip(K.VFEAT_WEIGHTS, torch_rows(q), torch_rows(c)):
        t = torch.einsum("qk,qck->qc", a, b[ids]).clamp_(min=0).mul_(w)
        s = t if s is None else s.add_(t)
    return s


def scoring():
    gen = torch.Generator(device=DEV).manual_seed(7)
    Q, N, C = args.Q, args.N, args.C
    c = K.vfeat_extract(torch.randint(0, 256, (N, 33, 32), dtype=torch.uint8, device=DEV, generator=gen))
    q = K.vfeat_extract(torch.randint(0, 256, (Q, 33, 32), dtype=torch.uint8, device=DEV, generator=gen))
    ids = torch.randint(0, N, (Q, C), dtype=torch.int64, device=DEV, generator=gen)
    res, ts = alternate({"dense  hq_vfeat_scores       ": lambda: K.vfeat_scores(q, c),
                         "dense  torch f64 3 matmuls   ": lambda: torch_dense(q.rows, c.rows),
                         "listed hq_vfeat_scores_listed": lambda: K.vfeat_scores_listed(q, c, ids),
                         "listed torch f64 gather+einsum": lambda: torch_listed(q.rows, c.rows, ids)})
    say(f"-- scoring, Q = {Q} queries x N = {N} rows (features of 33 x 32 random frames); listed C = {C}")
    keys = list(ts)
    for k in keys:
        say(line(k, ts[k]))
    for hq, th in ((keys[0], keys[1]), (keys[2], keys[3])):
        say(f"  {hq.split()[0]}: torch / hq = {statistics.median(ts[th]) / statistics.median(ts[hq]):.2f}x; "
            f"max |hq - torch| = {(res[hq] - res[th]).abs().max().item():.3e}")
    med = statistics.median(ts[keys[0]])
    say(f"  dense: {Q * N * 8 / med / 1e9:.2f} TB/s of scores written, {Q * N * 56 * 2 / med / 1e9:.1f} TFLOP/s of "
        "float64 contraction")


def errors():
    say(f"== hq_vfeat_extract / hq_vfeat_scores against the float64 model of tests/vfeat_cases.py, "
        f"{torch.cuda.get_device_name(0)}: largest errors over 3 queries x 5 frames per shape ==")
    say("(asserted: exact slots equal; other features <= 4 H W 2.2e-16 max(1, |want|); scores <= 1e-10, and <= 1e-5 "
        "to the float32-histogram typing)")
    shapes = [(4, 4), (7, 9), (33, 32), (65, 64), (131, 128)]
    for fam in V.FAMILIES:
        ef, es, e32, exact = [], [], [], True
        for H, W in shapes:
            fr = V.make(fam, H, W)
            want = np.stack([V.features(g) for g in fr])
            rows = K.vfeat_extract(torch.from_numpy(fr).to(DEV))
            got = rows.rows.cpu().numpy()[:, :55]
            exact &= got[:, V.EXACT].tolist() == want[:, V.EXACT].tolist()
            ef.append((np.abs(got - want) / np.maximum(1, np.abs(want))).max())
            s = K.vfeat_scores(K.VfeatRows(rows.rows[:3]), K.VfeatRows(rows.rows[3:])).cpu().numpy()
            es.append(max(abs(s[a, b] - V.score(want[a], want[3 + b])) for a in range(3) for b in range(5)))
            e32.append(max(abs(s[a, b] - V.score(want[a], want[3 + b], hist32=True)) for a in range(3) for b in range(5)))
        say(f"  {fam:8s} exact slots {'equal' if exact else 'DIFFER'}; features "
            + " ".join(f"{H}x{W}: {e:.2e}" for (H, W), e in zip(shapes, ef))
            + f"; score max {max(es):.2e}; to float32 typing max {max(e32):.2e}")


if args.errors:
    errors()
    write(args.out or os.path.join(ROOT, "profiles", "vfeat_error_bounds.txt"))
else:
    say(f"== video features of u8 frames, {torch.cuda.get_device_name(0)}: {args.reps} repetitions after one warm-up "
        "call, HIP events, routes alternating ==")
    for s in args.shapes:
        extraction(*(int(v) for v in s.split("x")))
    scoring()
    write(args.out or os.path.join(ROOT, "profiles", "vfeat_vs_host.txt"))
