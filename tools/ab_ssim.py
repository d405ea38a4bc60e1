#!/usr/bin/env python3
"""Gaussian-window SSIM of u8 frame pairs: hq_ssim_scores (dense [Q, N]) and hq_ssim_scores_listed ([Q, C] through an
id list into a resident store) against the route a user has without them on the same device: the same formula with
torch.nn.functional.conv2d in float64 over reflect-padded frames, batched per query (the corpus side's maps computed
once per call, as the kernel does per frame).  Written to profiles/ssim_vs_torch.txt.

Every variant runs between two HIP events after a warm-up call, the routes alternate inside each repetition; the file
gives medians with the spread (min - max).  The torch route is timed on --torch-queries of the Q queries (it is linear
in Q: one batch per query) and the figure is scaled to Q; the two routes' scores are compared on those queries.

With --errors the largest |score - model| of every frame family of tests/ssim_cases.py (the float64 NumPy / SciPy
model the tests assert against) is written to profiles/ssim_error_bounds.txt.

usage: ab_ssim.py [--out FILE] [--errors] [--reps 5] [--shapes 65x64 33x32] [--Q 100] [--N 10000] [--C 64]
                  [--resident 250000] [--torch-queries 10]
Needs an MI355X."""
import argparse
import os
import statistics
import sys

ap = argparse.ArgumentParser()
ap.add_argument("--out", default=None)
ap.add_argument("--errors", action="store_true")
ap.add_argument("--reps", type=int, default=5)
ap.add_argument("--shapes", nargs="+", default=["65x64", "33x32"])
ap.add_argument("--Q", type=int, default=100)
ap.add_argument("--N", type=int, default=10000)
ap.add_argument("--C", type=int, default=64)
ap.add_argument("--resident", type=int, default=250000)
ap.add_argument("--torch-queries", type=int, default=10)
args = ap.parse_args()
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "hilbert-quantization_amd"), os.path.join(ROOT, "tests")]

import numpy as np  # noqa: E402
import torch  # noqa: E402
import torch.nn.functional as F  # noqa: E402
from hq_mi355x import kernels as K  # noqa: E402

assert torch.cuda.is_available(), "ab_ssim.py needs the GPU"
DEV = torch.device("cuda:0")
LINES = []


def say(s=""):
    print(s, flush=True)
    LINES.append(s)


def write(path):
    with open(path, "w") as f:
        f.write("\n".join(LINES) + "\n")
    del LINES[:]


def timed(fn):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    r = fn()
    e1.record()
    e1.synchronize()
    return e0.elapsed_time(e1), r


G = torch.exp(-(torch.arange(7, dtype=torch.float64, device=DEV) - 3) ** 2 / 4.5)
G = G / G.sum()
G2 = torch.outer(G, G)[None, None]


def gauss(a):
    """[B, H, W] float64 -> the 7 x 7 Gaussian correlation with mirrored borders."""
    return F.conv2d(F.pad(a[:, None], (3, 3, 3, 3), mode="reflect"), G2)[:, 0]


def normalise(u8):
    a = u8.to(torch.float64)
    mn, mx = a.amin((1, 2), keepdim=True), a.amax((1, 2), keepdim=True)
    return (a - mn) / (mx - mn + 1e-8)


def torch_ssim(q_u8, c_u8, ids=None, chunk=2048):
    """The formula in float64 torch ops: [Q, N], or [Q, C] when ids [Q, C] lists frames of c_u8 per query."""
    xs = normalise(q_u8)
    m1s = gauss(xs)
    v1s = gauss(xs * xs) - m1s * m1s
    n_out = c_u8.shape[0] if ids is None else ids.shape[1]
    out = torch.empty((q_u8.shape[0], n_out), dtype=torch.float64, device=DEV)
    for a in range(q_u8.shape[0]):
        for j0 in range(0, n_out, chunk):
            y = normalise(c_u8[j0:j0 + chunk] if ids is None else c_u8[ids[a, j0:j0 + chunk]])
            m2 = gauss(y)
            v2 = gauss(y * y) - m2 * m2
            cov = gauss(xs[a:a + 1] * y) - m1s[a:a + 1] * m2
            num = (2 * m1s[a:a + 1] * m2 + 1e-4) * (2 * cov + 9e-4)
            den = (m1s[a:a + 1] ** 2 + m2 * m2 + 1e-4) * (v1s[a:a + 1] + v2 + 9e-4) + 1e-8
            out[a, j0:j0 + chunk] = (num / den).mean((1, 2))
    return out


def line(tag, ts):
    return f"{tag} median {statistics.median(ts):10.3f} ms  (min {min(ts):10.3f} - max {max(ts):10.3f})"


def compare(H, W):
    gen = torch.Generator(device=DEV).manual_seed(H * 1000 + W)
    Q, N, C, R, Qt = args.Q, args.N, args.C, args.resident, min(args.torch_queries, args.Q)
    q = torch.randint(0, 256, (Q, H, W), dtype=torch.uint8, device=DEV, generator=gen)
    store = torch.randint(0, 256, (R, H, W), dtype=torch.uint8, device=DEV, generator=gen)
    ids = torch.randint(0, R, (Q, C), dtype=torch.int64, device=DEV, generator=gen)
    c = store[:N]
    routes = {
        "dense  hq_ssim_scores       ": lambda: K.ssim_scores(K.ssim_prepare(q), c),
        "dense  torch conv2d f64     ": lambda: torch_ssim(q[:Qt], c),
        "listed hq_ssim_scores_listed": lambda: K.ssim_scores_listed(K.ssim_prepare(q), store, ids),
        "listed torch conv2d f64     ": lambda: torch_ssim(q[:Qt], store, ids[:Qt]),
    }
    res, ts = {}, {k: [] for k in routes}
    for k, fn in routes.items():
        res[k] = fn()  # warm-up
    torch.cuda.synchronize()
    for _ in range(args.reps):
        for k, fn in routes.items():
            ts[k].append(timed(fn)[0])
    say(f"-- frames {H} x {W}, Q = {Q}; dense N = {N}; listed C = {C} of {R} resident frames; torch timed on {Qt} queries")
    keys = list(routes)
    for k in keys:
        say("  " + line(k, ts[k]) + (f"   x {Q / Qt:g} for Q = {Q}: {statistics.median(ts[k]) * Q / Qt:10.3f} ms"
                                     if "torch" in k else f"   (includes hq_ssim_prepare of the {Q} queries)"))
    for hq, th in ((keys[0], keys[1]), (keys[2], keys[3])):
        say(f"  {hq.split()[0]}: torch / hq = {statistics.median(ts[th]) * Q / Qt / statistics.median(ts[hq]):.1f}x; "
            f"max |hq - torch| on the {Qt} compared queries = {(res[hq][:Qt] - res[th]).abs().max().item():.3e}")


def errors():
    import ssim_cases as S
    say(f"== hq_ssim_scores against the float64 model of tests/ssim_cases.py, {torch.cuda.get_device_name(0)}: "
        "largest |score - model| over 3 queries x 5 frames per shape ==")
    say("(asserted bound: 1e-5 for ssim, 1e-12 for the template correlation)")
    shapes = [(4, 4), (7, 9), (33, 32), (65, 64), (131, 128)]
    for fam in S.FAMILIES:
        es, en = [], []
        for H, W in shapes:
            q, c = S.make(fam, H, W)
            got, ncc = (t.cpu().numpy() for t in K.ssim_scores(K.ssim_prepare(torch.from_numpy(q).to(DEV)),
                                                               torch.from_numpy(c).to(DEV), ncc=True))
            es.append(max(abs(got[a, b] - S.ssim_model(q[a], c[b])) for a in range(len(q)) for b in range(len(c))))
            en.append(max(abs(ncc[a, b] - S.ncc_model(q[a], c[b])) for a in range(len(q)) for b in range(len(c))))
        say(f"  {fam:13s} ssim " + " ".join(f"{H}x{W}: {e:.2e}" for (H, W), e in zip(shapes, es))
            + f"   ncc max {max(en):.2e}")


if args.errors:
    errors()
    write(os.path.join(ROOT, "profiles", "ssim_error_bounds.txt"))
else:
    say(f"== SSIM of u8 frame pairs, {torch.cuda.get_device_name(0)}: {args.reps} repetitions after one warm-up call, "
        "HIP events, routes alternating ==")
    for s in args.shapes:
        H, W = (int(v) for v in s.split("x"))
        compare(H, W)
    write(args.out or os.path.join(ROOT, "profiles", "ssim_vs_torch.txt"))
