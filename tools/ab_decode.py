#!/usr/bin/env python3
"""Fused decode against the unfused sequence: u8 frames -> parameters, device resident, one process.

(a) the unfused path: K.dequantize_u8 (f32 [N, n+1, n]) -> enh[:, :-1, :].contiguous() -> K.map_from_2d (all
    n * n cells; the host used to truncate to parameter_count) — what core.pipeline.reconstruct_batch ran before
    hq_dequantize_unmap;
(b) K.dequantize_unmap (one kernel, d floats per frame), with non-temporal and with plain stores (option
    decode_nt), and the generic kernel (option decode_generic) for comparison.

Every variant runs once per repetition, in turn (a, b-nt, b-plain, b-generic, a, ...), each between two HIP
events on the launch stream, after warm-up runs of every variant; outputs are compared bit for bit first.
Prints the medians, (a) / (b), and (b)'s share of the 8 TB/s spec peak at (n+1) n + 8 + 4 d algorithmic bytes
per frame (10,312 B at n = 64, d = 1536).

usage: ab_decode.py [--frames 1000000] [--n 64] [--d 1536] [--reps 15] [--warmup 3]
Needs an MI355X."""
import argparse
import os
import statistics
import sys

ap = argparse.ArgumentParser()
ap.add_argument("--frames", type=int, default=1_000_000)
ap.add_argument("--n", type=int, default=64)
ap.add_argument("--d", type=int, default=1536)
ap.add_argument("--reps", type=int, default=15)
ap.add_argument("--warmup", type=int, default=3)
args = ap.parse_args()
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "hilbert-quantization_amd")]

import torch  # noqa: E402
from hq_mi355x import _lib, kernels as K  # noqa: E402

assert torch.cuda.is_available(), "ab_decode.py needs the GPU"
N, n, d = args.frames, args.n, args.d
PEAK = 8.0e12
BYTES = (n + 1) * n + 8 + 4 * d

g = torch.Generator(device="cuda").manual_seed(0)
frames = torch.randint(0, 256, (N, n + 1, n), generator=g, dtype=torch.uint8, device="cuda")
lo = torch.rand((N, 1), generator=g, device="cuda") * 2 - 1.5
mm = torch.cat([lo, lo + 0.5 + torch.rand((N, 1), generator=g, device="cuda")], 1).contiguous()
out_b = torch.empty((N, d), dtype=torch.float32, device="cuda")


def unfused():
    enh = K.dequantize_u8(frames, mm)
    return K.map_from_2d(enh[:, :-1, :].contiguous(), None)


def fused(nt, generic=0):
    def run():
        with _lib.option("decode_nt", nt), _lib.option("decode_generic", generic):
            return K.dequantize_unmap(frames, mm, d, out=out_b)
    return run


VARIANTS = [("a  unfused (dequantize_u8 + contiguous + map_from_2d)", unfused),
            ("b  dequantize_unmap, non-temporal stores", fused(1)),
            ("b  dequantize_unmap, plain stores", fused(0)),
            ("b' dequantize_unmap, generic kernel", fused(1, 1))]

# same bits first (and the first launches: code objects, allocator blocks)
ref = unfused()[:, :d]
for name, fn in VARIANTS[1:]:
    out_b.fill_(-1.0)
    assert torch.equal(fn(), ref), name
del ref
for _ in range(args.warmup):
    for _, fn in VARIANTS:
        fn()
torch.cuda.synchronize()

times = {name: [] for name, _ in VARIANTS}
for _ in range(args.reps):
    for name, fn in VARIANTS:
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        r = fn()
        e1.record()
        e1.synchronize()
        del r
        times[name].append(e0.elapsed_time(e1) * 1e-3)

print(f"== decode A/B: {N} frames of {n + 1} x {n}, d = {d}, {args.reps} alternating repetitions after "
      f"{args.warmup} warm-up rounds, HIP events; {torch.cuda.get_device_name(0)} ==")
med = {}
for name, _ in VARIANTS:
    ts = times[name]
    med[name] = statistics.median(ts)
    print(f"{name:<58} median {med[name] * 1e3:8.3f} ms  (min {min(ts) * 1e3:8.3f}, max {max(ts) * 1e3:8.3f})  "
          f"{N / med[name] / 1e6:7.1f} M frames/s")
a = med[VARIANTS[0][0]]
for name, _ in VARIANTS[1:]:
    share = BYTES * N / med[name] / PEAK
    print(f"(a) / ({name.split(',')[-1].strip()}): {a / med[name]:5.2f}x   {BYTES * N / med[name] / 1e12:5.2f} TB/s "
          f"= {share:5.3f} of the 8 TB/s spec peak at {BYTES} B per frame")
print(f"(b) non-temporal / plain stores: {med[VARIANTS[2][0]] / med[VARIANTS[1][0]]:5.3f}x "
      f"(> 1: non-temporal is faster)")
