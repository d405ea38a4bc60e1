#!/usr/bin/env python3
"""The JPEG stage of the batched reconstruct: HilbertQuantizer.reconstruct_many(codec="device") (hq_jpeg_probe +
hq_jpeg_decode, the frames handed to hq_dequantize_unmap on the device) against codec="host" (PIL on 16 threads,
the frames uploaded), in the same run (written to profiles/jpeg_decode_vs_host.txt).

Both routes start from a list of QuantizedModels whose payloads are bytes on the host and end with float32 vectors
on the host, so both are timed on the host clock around whole calls, alternating inside each repetition after a
warm-up call each; their results are compared bit for bit.  core.compressor.decode_jpeg_batch alone (join, upload,
probe, read-back of the shapes, decode, read-back of the statuses) is timed the same way, and the two launches
alone (payload resident, no copy) between two HIP events for 8, 16, 32 and 64 frames per wave (option
jpeg_decode_f), the four alternating.

Payloads: the fused map + quantise kernel's frames for gaussian parameter vectors, encoded by the host codec (PIL,
optimize=True: a Huffman table pair per payload) and by the device codec (hq_jpeg_encode: the Annex K tables).

usage: ab_jpeg_decode.py [--out FILE] [--count 100000] [--reps 3] [--quality 0.8]
Needs an MI355X."""
import argparse
import concurrent.futures as cf
import dataclasses
import os
import statistics
import sys
import time

ap = argparse.ArgumentParser()
ap.add_argument("--out", default=None)
ap.add_argument("--count", type=int, default=100_000)
ap.add_argument("--reps", type=int, default=3)
ap.add_argument("--quality", type=float, default=0.8)
args = ap.parse_args()
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "hilbert-quantization_amd")]

import numpy as np  # noqa: E402
import torch  # noqa: E402
from hq_mi355x import _lib, kernels as K  # noqa: E402
from hq_mi355x._dev import to_dev, to_np  # noqa: E402
from hq_mi355x.api import HilbertQuantizer  # noqa: E402
from hq_mi355x.core.compressor import decode_jpeg_batch, encode_jpeg, encode_jpeg_batch  # noqa: E402

assert torch.cuda.is_available(), "ab_jpeg_decode.py needs the GPU"
OUT = args.out or os.path.join(ROOT, "profiles", "jpeg_decode_vs_host.txt")
LINES = []


def say(s=""):
    print(s, flush=True)
    LINES.append(s)


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


def main():
    N = args.count
    say(f"== JPEG stage of the batched reconstruct, {torch.cuda.get_device_name(0)}: {N} payloads, quality "
        f"{args.quality}, {args.reps} repetitions after one warm-up call, routes alternating ==")
    say('(a) reconstruct_many(codec="device"): join, upload, probe, decode, hq_dequantize_unmap, vectors to the host')
    say('(b) reconstruct_many(codec="host"): PIL on 16 threads, upload, hq_dequantize_unmap, vectors to the host')
    say("(c) decode_jpeg_batch alone: join, upload, probe, shapes back, decode, statuses back; frames stay on the device")
    say("(d) hq_jpeg_probe + hq_jpeg_decode alone, payload resident: HIP events, per frames-per-wave F")
    for d, n in ((4096, 64), (1024, 32)):
        hq = HilbertQuantizer()
        g = torch.Generator(device="cuda").manual_seed(N + d)
        X = torch.randn((N, d), generator=g, device="cuda", dtype=torch.float32)
        template = hq.quantize_many([to_np(X[0])])[0]
        frames = K.map_index_quantize(X, n, n)[0]
        del X
        H, W = int(frames.shape[1]), int(frames.shape[2])
        fr_h = to_np(frames)
        with cf.ThreadPoolExecutor(max_workers=16) as pool:
            sources = {"host": list(pool.map(lambda k: encode_jpeg(fr_h[k], args.quality), range(N))),
                       "device": encode_jpeg_batch(frames, args.quality)}
        del frames
        for codec, payloads in sources.items():
            models = [dataclasses.replace(template, compressed_data=p) for p in payloads]
            hq.reconstruct_many(models, codec="device")  # warm-up calls
            hq.reconstruct_many(models[:2000])
            ta, tb, tc = [], [], []
            for _ in range(args.reps):
                t, a = clock(lambda: hq.reconstruct_many(models, codec="device"))
                ta.append(t)
                t, b = clock(lambda: hq.reconstruct_many(models))
                tb.append(t)
                t, (groups, refused) = clock(lambda: decode_jpeg_batch(payloads))
                tc.append(t)
            same = all(x.tobytes() == y.tobytes() for x, y in zip(a, b))
            total = sum(map(len, payloads))
            offs = np.zeros(N + 1, np.int64)
            np.cumsum([len(p) for p in payloads], out=offs[1:])
            payload, offsets = to_dev(np.frombuffer(bytearray(b"".join(payloads)), np.uint8)), to_dev(offs)
            tk = {F: [] for F in (8, 16, 32, 64)}
            for rep in range(args.reps + 1):  # the first round warms every F up
                for F in tk:
                    with _lib.option("jpeg_decode_f", F):
                        t = events(lambda: K.jpeg_decode(payload, offsets, K.jpeg_probe(payload, offsets), None, H, W))
                    if rep:
                        tk[F].append(t)
            ma, mb, mc = statistics.median(ta), statistics.median(tb), statistics.median(tc)
            say(f"-- {N} payloads of {H} x {W} from the {codec} encoder ({total / N:.1f} bytes per payload); refused by the "
                f"device: {len(refused)}; (a) and (b) bit-identical: {same}")
            say(f"  (a) device codec   {spread(ta)}   {N / ma:12.0f} models/s")
            say(f"  (b) host codec     {spread(tb)}   {N / mb:12.0f} models/s      (b) / (a) = {mb / ma:.1f}x")
            say(f"  (c) decode_jpeg_batch {spread(tc)}   {N / mc:12.0f} frames/s")
            for F, ts in tk.items():
                say(f"  (d) F = {F:2d} launches {spread(ts)}   {N / statistics.median(ts):12.0f} frames/s")
            del models, a, b, groups, payload
            torch.cuda.empty_cache()
    os.makedirs(os.path.dirname(OUT), exist_ok=True)
    with open(OUT, "w") as f:
        f.write("\n".join(LINES) + "\n")


if __name__ == "__main__":
    main()
