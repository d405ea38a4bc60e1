"""Shared inputs of the fused decode tests (test_decode_cpu.py, test_gpu_decode.py).

Plain NumPy plus the CPU oracle; nothing here touches the GPU package.  A decoded value is
((float)b / 255.0f) * (mx - mn) + mn in float32 (oracle.denormalize_u8), a function of one byte and one
(mn, mx) pair, so 256 bytes x the ranges of quant_edges.RANGES_F32 is the whole domain of the arithmetic; the
kept length of an index row (oracle.extract_index_row) depends only on where the row's last value != 0 is.
test_decode_cpu.py shows on the CPU that these inputs tell a reciprocal de-normalise from the exact one and
that the index-row cases reach the lengths 1, a middle value and n.
"""
import numpy as np

from oracle import hq_oracle as O

import quant_edges as Q

F32 = np.float32


def every_byte_frame(n=16):
    """u8 [n+1, n] whose first 256 cells hold every byte value once (37 is odd, so k -> 37 k + 11 mod 256 is
    a permutation); the cells after them repeat the sequence, so for n = 16 the image has all 256 values and
    the index row sixteen different ones."""
    cells = (n + 1) * n
    assert cells >= 256
    return ((np.arange(cells, dtype=np.int64) * 37 + 11) % 256).astype(np.uint8).reshape(n + 1, n)


def pairs():
    """[(mn, mx)]: every family of RANGES_F32, then the flat pair (mn, mn) of every family."""
    return list(Q.RANGES_F32.values()) + [(mn, mn) for mn, _ in Q.RANGES_F32.values()]


def oracle_decode(frames, mn, mx, d):
    """map_from_2d(denormalize_u8(frame)[:-1])[:d] per frame; mn, mx scalars (shared) or one per frame."""
    frames = np.asarray(frames)
    if frames.ndim == 2:
        frames = frames[None]
    mn = np.broadcast_to(np.asarray(mn, F32), (len(frames),))
    mx = np.broadcast_to(np.asarray(mx, F32), (len(frames),))
    enh = np.stack([O.denormalize_u8(f, a, b) for f, a, b in zip(frames, mn, mx)])
    assert enh.dtype == F32
    return np.ascontiguousarray(O.map_from_2d(enh[:, :-1])[:, :d])


def oracle_index(frames, mn, mx):
    """(last rows f32 [N, n], kept lengths int32 [N]) of oracle.extract_index_row on the de-normalised frames."""
    frames = np.asarray(frames)
    if frames.ndim == 2:
        frames = frames[None]
    mn = np.broadcast_to(np.asarray(mn, F32), (len(frames),))
    mx = np.broadcast_to(np.asarray(mx, F32), (len(frames),))
    rows, lens = [], []
    for f, a, b in zip(frames, mn, mx):
        enh = O.denormalize_u8(f, a, b)
        rows.append(enh[-1])
        lens.append(len(O.extract_index_row(enh)[1]))
    return np.stack(rows).astype(F32, copy=False), np.array(lens, np.int32)


def recip_denormalize(u8, mn, mx):
    """The de-normalise a kernel must NOT use: the byte times fl(1 / 255) instead of the division."""
    mn, mx = F32(mn), F32(mx)
    u = np.asarray(u8).astype(F32)
    if mx == mn:
        return np.full_like(u, mn)
    with np.errstate(all="ignore"):
        return ((u * (F32(1.0) / F32(255.0))).astype(F32) * (mx - mn) + mn).astype(F32)


def index_cases(n):
    """[(name, frame u8 [n+1, n], mn, mx)]: the index-row cases of the issue.  The image part is random."""
    rng = np.random.default_rng(100 + n)

    def frame(row):
        f = rng.integers(0, 256, (n + 1, n), dtype=np.uint8)
        f[-1] = row
        return f

    mid = np.zeros(n, np.uint8)
    mid[: n // 2 - 1] = rng.integers(1, 256, n // 2 - 1, dtype=np.uint8)   # ends in zero bytes
    last_only = np.zeros(n, np.uint8)
    last_only[-1] = 7
    first_only = np.zeros(n, np.uint8)
    first_only[0] = 200
    zeros = np.zeros(n, np.uint8)
    varied = rng.integers(1, 256, n, dtype=np.uint8)
    return [
        ("trimmed", frame(mid), F32(0.0), F32(2.5)),                 # trailing zeros with mn = 0: n / 2 - 1
        ("untrimmed", frame(mid), F32(-1.0), F32(2.5)),              # same bytes, mn != 0: n
        ("all_zero", frame(zeros), F32(0.0), F32(1.0)),              # nothing != 0: 1
        ("flat_zero", frame(varied), F32(0.0), F32(0.0)),            # mn = mx = 0: every value 0.0 -> 1
        ("neg_zero", frame(mid), F32(-0.0), F32(3.0)),               # zero bytes give -0.0 + ... : trimmed
        ("flat_neg_zero", frame(varied), F32(-0.0), F32(-0.0)),      # every value -0.0, which counts as zero: 1
        ("last_column", frame(last_only), F32(0.0), F32(1.0)),       # n
        ("first_column", frame(first_only), F32(0.0), F32(1.0)),     # 1, with a value
        ("flat_nonzero", frame(zeros), F32(0.25), F32(0.25)),        # every value 0.25: n
    ]
