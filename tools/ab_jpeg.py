#!/usr/bin/env python3
"""The JPEG stage of the batched ingest: core.compressor.encode_jpeg_batch (hq_jpeg_encode: two launches of one
kernel, the payloads back in one copy, sliced into bytes on the host) against the host route of api._ingest (the
frames copied to the host, core.compressor.encode_jpeg = PIL with optimize=True on a pool of min(32, cpus)
threads), in the same run (written to profiles/jpeg_vs_host.txt).

The frames are resident on the device for both routes, as quantize_batch leaves them; both routes end with a list
of bytes objects on the host, which is what the ingest needs, so both are timed on the host clock around whole
calls (they end in a device-to-host copy).  The two alternate inside each repetition after one warm-up call each.
The kernel launches alone (measure + prefix sum + write, no copy) are timed between two HIP events.  The file gives
medians with the spread, the total payload size of both routes, and the mean squared error of the PIL-decoded
payloads against the frames for a sample of each route.

Frames: the fused map + quantise kernel's output for gaussian parameter vectors (a u8 Hilbert image plus its index
row), the ingest's own frames.

usage: ab_jpeg.py [--out FILE] [--counts 10000 100000] [--reps 5] [--quality 0.8]
Needs an MI355X."""
import argparse
import concurrent.futures as cf
import os
import statistics
import sys
import time

ap = argparse.ArgumentParser()
ap.add_argument("--out", default=None)
ap.add_argument("--counts", type=int, nargs="+", default=[10_000, 100_000])
ap.add_argument("--reps", type=int, default=5)
ap.add_argument("--quality", type=float, default=0.8)
args = ap.parse_args()
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "hilbert-quantization_amd")]

import numpy as np  # noqa: E402
import torch  # noqa: E402
from hq_mi355x import kernels as K  # noqa: E402
from hq_mi355x._dev import to_np  # noqa: E402
from hq_mi355x.core.compressor import decode_jpeg, encode_jpeg, encode_jpeg_batch, jpeg_quality  # noqa: E402

assert torch.cuda.is_available(), "ab_jpeg.py needs the GPU"
OUT = args.out or os.path.join(ROOT, "profiles", "jpeg_vs_host.txt")
WORKERS = min(32, os.cpu_count() or 1)
LINES = []


def say(s=""):
    print(s, flush=True)
    LINES.append(s)


def host_route(frames, pool):
    fr_h = to_np(frames)
    return list(pool.map(lambda k: encode_jpeg(fr_h[k], args.quality), range(len(fr_h))))


def clock(fn):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    r = fn()
    torch.cuda.synchronize()
    return time.perf_counter() - t0, r


def events(fn):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    fn()
    e1.record()
    e1.synchronize()
    return e0.elapsed_time(e1) * 1e-3


def spread(ts):
    return f"median {statistics.median(ts) * 1e3:10.2f} ms  (min {min(ts) * 1e3:10.2f} - max {max(ts) * 1e3:10.2f})"


def mse(payloads, fr_h, sample):
    return float(np.mean([(decode_jpeg(payloads[i]).astype(np.float64) - fr_h[i].astype(np.float64)) ** 2
                          for i in sample]))


def main():
    q = jpeg_quality(args.quality)
    say(f"== JPEG stage of the batched ingest, {torch.cuda.get_device_name(0)}: quality {args.quality} (libjpeg q = {q}), "
        f"{args.reps} repetitions after one warm-up call, routes alternating ==")
    say("(a) encode_jpeg_batch: hq_jpeg_encode twice (measure, write), one payload copy, slicing; host clock")
    say(f"(b) host route: frames to the host, PIL optimize=True on {WORKERS} threads; host clock")
    with cf.ThreadPoolExecutor(max_workers=WORKERS) as pool:
        for d, n in ((4096, 64), (1024, 32)):
            for N in args.counts:
                g = torch.Generator(device="cuda").manual_seed(N + d)
                X = torch.randn((N, d), generator=g, device="cuda", dtype=torch.float32)
                frames = K.map_index_quantize(X, n, n)[0]
                del X
                H, W = int(frames.shape[1]), int(frames.shape[2])
                a = encode_jpeg_batch(frames, args.quality)       # warm-up calls
                b = host_route(frames[:min(N, 2000)], pool)
                ta, tb, tk = [], [], []
                for _ in range(args.reps):
                    t, a = clock(lambda: encode_jpeg_batch(frames, args.quality))
                    ta.append(t)
                    tk.append(events(lambda: K.jpeg_encode(frames, q)))
                    t, b = clock(lambda: host_route(frames, pool))
                    tb.append(t)
                ma, mb, mk = statistics.median(ta), statistics.median(tb), statistics.median(tk)
                fr_h = to_np(frames)
                sample = range(0, N, max(1, N // 500))
                sa, sb = sum(map(len, a)), sum(map(len, b))
                say(f"-- {N} frames of {H} x {W}")
                say(f"  (a) device codec   {spread(ta)}   {N / ma:12.0f} frames/s")
                say(f"      launches alone {spread(tk)}   {N / mk:12.0f} frames/s (HIP events; the total is read back "
                    f"between the two launches)")
                say(f"  (b) host codec     {spread(tb)}   {N / mb:12.0f} frames/s")
                say(f"      (b) / (a) = {mb / ma:.1f}x")
                say(f"      payload bytes: device {sa} ({sa / N:.1f} per frame), host {sb} ({sb / N:.1f} per frame), "
                    f"device / host = {sa / sb:.3f}")
                ea, eb = mse(a, fr_h, sample), mse(b, fr_h, sample)
                say(f"      decoded-frame MSE over {len(sample)} frames: device {ea:.4f}, host {eb:.4f}, "
                    f"device / host = {ea / eb:.5f}")
                del frames, a, b
                torch.cuda.empty_cache()
    os.makedirs(os.path.dirname(OUT), exist_ok=True)
    with open(OUT, "w") as f:
        f.write("\n".join(LINES) + "\n")


if __name__ == "__main__":
    main()
