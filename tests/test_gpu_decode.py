"""GPU parity of the fused decode (hq_dequantize_unmap), the round-trip metrics (hq_roundtrip_error) and the
layers above them.  Bit-exact against the CPU oracle's map_from_2d(denormalize_u8(frame, mn, mx)[:-1])[:d]
throughout; inputs come from decode_cases.py / quant_edges.py, and test_decode_cpu.py shows on the CPU that
they discriminate.

Input domain (include/hq_mi355x.h): finite min <= max with a finite difference."""
import dataclasses

import numpy as np
import pytest

from oracle import hq_oracle as O

import decode_cases as D
import quant_edges as Q

pytestmark = pytest.mark.gpu

N_LONG = 41_000     # as test_gpu_quant_edges.py: longer than any persistent grid
N_ROWS = 97         # distinct frames of the long batch
SENTINEL = np.float32(-12345.678)


def _t(x):
    from hq_mi355x._dev import to_dev
    return to_dev(x)


def _np(x):
    from hq_mi355x._dev import to_np
    return to_np(x)


def _same(got, ref, what=""):
    """Bitwise equality of two arrays; on failure name the first differing element."""
    got, ref = np.ascontiguousarray(got), np.ascontiguousarray(ref)
    assert got.shape == ref.shape and got.dtype == ref.dtype, (what, got.shape, ref.shape, got.dtype, ref.dtype)
    if got.tobytes() == ref.tobytes():
        return
    a, b = got.reshape(-1).view(np.uint8), ref.reshape(-1).view(np.uint8)
    i = int(np.flatnonzero(a != b)[0]) // got.dtype.itemsize
    idx = np.unravel_index(i, got.shape)
    n = int(np.sum(got.reshape(-1).view(np.uint32) != ref.reshape(-1).view(np.uint32))) if got.dtype.itemsize == 4 \
        else int(np.sum(got.reshape(-1) != ref.reshape(-1)))
    raise AssertionError(f"{what}: {n} of {got.size} differ, first at {tuple(int(k) for k in idx)}: "
                         f"got {got[idx]!r}, expected {ref[idx]!r}")


def _tiled(ref, n):
    reps = -(-n // len(ref))
    return np.tile(ref, (reps,) + (1,) * (ref.ndim - 1))[:n]


def _generic(hq_option, on):
    if on:
        hq_option("decode_generic", 1)


# ------------------------------------------------------------------------------ 1. every byte x every range


@pytest.mark.parametrize("generic", [0, 1])
def test_every_byte_every_range(hq_lib, generic, hq_option):
    """All 256 bytes (image and index row) under every range family and every flat pair: per-row (min, max),
    then one shared-mode launch per pair, which must equal the per-row result with the pair repeated."""
    from hq_mi355x import kernels as K
    _generic(hq_option, generic)
    pairs = D.pairs()
    f = D.every_byte_frame(16)
    frames = np.tile(f, (len(pairs), 1, 1))
    mm = np.array(pairs, np.float32)
    ref = D.oracle_decode(frames, mm[:, 0], mm[:, 1], 256)
    rrow, rlen = D.oracle_index(frames, mm[:, 0], mm[:, 1])
    dev = _t(frames)
    got, row, ln = K.dequantize_unmap(dev, _t(mm), 256, want_index=True)
    got, row, ln = _np(got), _np(row), _np(ln)
    _same(got, ref, "per-row parameters")
    _same(row, rrow, "per-row index row")
    _same(ln, rlen, "per-row index length")
    three = _t(np.tile(f, (3, 1, 1)))
    for i, (mn, mx) in enumerate(pairs):
        for pair in (_t(np.array([mn, mx], np.float32)), _t(np.array([[mn, mx]], np.float32))):   # [2] and [1, 2]
            g, r, l = K.dequantize_unmap(three, pair, 256, want_index=True)
            _same(_np(g), np.tile(got[i], (3, 1)), f"shared parameters, pair {i}")
            _same(_np(r), np.tile(row[i], (3, 1)), f"shared index row, pair {i}")
            _same(_np(l), np.tile(ln[i], 3), f"shared index length, pair {i}")


# -------------------------------------------------------------------------------------------------- 2. shapes

_SHAPE_N = 130
_SHAPE_REF = {}


def _shape_ref(n):
    """Random frames and per-frame ranges of side n with their oracle decode at d = n * n, computed once.  Two
    frames get an index row with a zero tail under mn = 0, so the generic kernel's lengths are not all n."""
    if n not in _SHAPE_REF:
        rng = np.random.default_rng(1000 + n)
        frames = rng.integers(0, 256, (_SHAPE_N, n + 1, n), dtype=np.uint8)
        lo = rng.uniform(-3, 1, _SHAPE_N).astype(np.float32)
        mm = np.stack([lo, lo + rng.uniform(0.1, 5, _SHAPE_N).astype(np.float32)], 1)
        frames[0, -1, :n // 2] |= 1
        frames[0, -1, n // 2:] = 0
        frames[1, -1, :] = 0
        mm[0] = (0.0, 1.5)
        mm[1] = (0.0, 2.0)
        mm[2] = (0.75, 0.75)                                       # a flat frame among the others
        ref = D.oracle_decode(frames, mm[:, 0], mm[:, 1], n * n)
        rrow, rlen = D.oracle_index(frames, mm[:, 0], mm[:, 1])
        for a in (ref, rrow, rlen):
            a.setflags(write=False)
        _SHAPE_REF[n] = (frames, mm, ref, rrow, rlen)
    return _SHAPE_REF[n]


def _shape_ds(n):
    ds = [0, 1, 3, 13, n * n - 1, n * n] + ({64: [1536], 16: [255]}.get(n, []))
    return sorted({d for d in ds if 0 <= d <= n * n})


@pytest.mark.parametrize("n", [2, 4, 8, 16, 32, 64, 128])
def test_shapes(hq_lib, n):
    """Every d, batch size, row stride and start alignment: the parameters match, and no float of the output
    buffer outside [row start, row start + d) is written (sentinel check over the whole buffer, the float in
    front of an offset view included)."""
    import torch
    from hq_mi355x import kernels as K
    frames, mm, ref, rrow, rlen = _shape_ref(n)
    assert rlen[0] == n // 2 and rlen[1] == 1 and (rlen[3:] == n).sum() > 100
    dev_f, dev_mm = _t(frames), _t(mm)
    for N in (1, 3, _SHAPE_N):
        fN, mN = dev_f[:N], dev_mm[:N]
        for d in _shape_ds(n):
            for stride in (d, d + 1, (d + 4) // 4 * 4 + 4):
                for offset in (0, 1):                              # 1: rows start 4 bytes off 16-byte alignment
                    flat = torch.full((N * stride + offset + 1,), float(SENTINEL), dtype=torch.float32,
                                      device=fN.device)
                    assert flat.data_ptr() % 16 == 0
                    view = flat[offset:offset + N * stride].view(N, stride)
                    want_index = stride == d + 1
                    res = K.dequantize_unmap(fN, mN, d, want_index=want_index, out=view)
                    what = f"n={n} N={N} d={d} stride={stride} offset={offset}"
                    if want_index:
                        res, row, ln = res
                        _same(_np(row), rrow[:N], what + " index row")
                        _same(_np(ln), rlen[:N], what + " index length")
                    assert tuple(res.shape) == (N, d)
                    host = _np(flat)
                    body = host[offset:offset + N * stride].reshape(N, stride)
                    _same(body[:, :d], ref[:N, :d], what)
                    assert np.all(body[:, d:] == SENTINEL), what + ": wrote past d"
                    assert np.all(host[:offset] == SENTINEL) and host[-1] == SENTINEL, what + ": wrote outside"


def test_unaligned_frames_take_the_generic_kernel(hq_lib):
    """Frames that do not start 16-byte aligned cannot be read in 16-byte pieces: same results."""
    import torch
    from hq_mi355x import kernels as K
    frames, mm, ref, rrow, rlen = _shape_ref(16)
    raw = torch.zeros(5 * 17 * 16 + 16, dtype=torch.uint8, device="cuda")
    view = raw[4:4 + 5 * 17 * 16].view(5, 17, 16)
    view.copy_(_t(frames[:5]))
    assert view.data_ptr() % 16 == 4 and view.is_contiguous()
    got, row, ln = K.dequantize_unmap(view, _t(mm[:5]), 255, want_index=True)
    _same(_np(got), ref[:5, :255], "parameters")
    _same(_np(row), rrow[:5], "index row")
    _same(_np(ln), rlen[:5], "index length")


@pytest.mark.parametrize("n", [16, 32, 64])
def test_plain_store_form(hq_lib, n, hq_option):
    """Option decode_nt = 0 (plain instead of non-temporal stores, the A/B form of tools/ab_decode.py): same bits."""
    from hq_mi355x import kernels as K
    hq_option("decode_nt", 0)
    frames, mm, ref, rrow, rlen = _shape_ref(n)
    for d in (n * n - 1, n * n, 3 * n * n // 8):
        got, row, ln = K.dequantize_unmap(_t(frames), _t(mm), d, want_index=True)
        _same(_np(got), ref[:, :d], f"n={n} d={d}")
        _same(_np(row), rrow, f"n={n} d={d} index row")
        _same(_np(ln), rlen, f"n={n} d={d} index length")


# ----------------------------------------------------------------------------------------------- 3. long batch


@pytest.mark.parametrize("generic", [0, 1])
def test_long_batch(hq_lib, generic, hq_option):
    from hq_mi355x import kernels as K
    _generic(hq_option, generic)
    rng = np.random.default_rng(77)
    frames = rng.integers(0, 256, (N_ROWS, 17, 16), dtype=np.uint8)
    lo = rng.uniform(-2, 2, N_ROWS).astype(np.float32)
    mm = np.stack([lo, lo + rng.uniform(0.01, 9, N_ROWS).astype(np.float32)], 1)
    ref = D.oracle_decode(frames, mm[:, 0], mm[:, 1], 255)
    rrow, rlen = D.oracle_index(frames, mm[:, 0], mm[:, 1])
    got, row, ln = K.dequantize_unmap(_t(_tiled(frames, N_LONG)), _t(_tiled(mm, N_LONG)), 255, want_index=True)
    _same(_np(got), _tiled(ref, N_LONG), "parameters")
    _same(_np(row), _tiled(rrow, N_LONG), "index row")
    _same(_np(ln), _tiled(rlen, N_LONG), "index length")


# ------------------------------------------------------------------------------------------------ 4. index row


@pytest.mark.parametrize("generic", [0, 1])
@pytest.mark.parametrize("n", [16, 64])
def test_index_row_cases(hq_lib, n, generic, hq_option):
    from hq_mi355x import kernels as K
    _generic(hq_option, generic)
    cases = D.index_cases(n)
    frames = np.stack([f for _, f, _, _ in cases])
    mm = np.array([[mn, mx] for _, _, mn, mx in cases], np.float32)
    assert np.signbit(mm[[c[0] for c in cases].index("neg_zero"), 0])
    rrow, rlen = D.oracle_index(frames, mm[:, 0], mm[:, 1])
    assert {1, n // 2 - 1, n} <= set(rlen.tolist())
    ref = D.oracle_decode(frames, mm[:, 0], mm[:, 1], 13)
    got, row, ln = K.dequantize_unmap(_t(frames), _t(mm), 13, want_index=True)
    _same(_np(got), ref, "per-row parameters")
    _same(_np(row), rrow, "per-row index row")
    _same(_np(ln), rlen, "per-row index length")
    # index outputs alone (d = 0): extract_indices_device
    from hq_mi355x.api import BatchQuantizer
    row0, ln0 = BatchQuantizer.extract_indices_device(_t(frames), _t(mm))
    _same(_np(row0), rrow, "d = 0 index row")
    _same(_np(ln0), rlen, "d = 0 index length")
    for i, (name, f, mn, mx) in enumerate(cases):                 # shared mode: one launch per case
        three = _t(np.tile(f, (3, 1, 1)))
        _, r, l = K.dequantize_unmap(three, _t(mm[i]), 13, want_index=True)
        _same(_np(r), np.tile(rrow[i], (3, 1)), f"shared index row, {name}")
        _same(_np(l), np.tile(rlen[i], 3), f"shared index length, {name}")


# ----------------------------------------------------------------------------------------------- 5. round trip


def _edge_rows(names, d):
    """[N, d] rows holding every quantiser edge value of the families `names`, each row starting with its
    family's mn, mx (test_gpu_quant_edges.py builds its fused inputs the same way)."""
    rows = []
    for name in names:
        mn, mx = Q.RANGES_F32[name]
        e = Q.edges(name)
        per = d - 2
        nrow = -(-len(e) // per)
        r = np.empty((nrow, d), np.float32)
        r[:, 0], r[:, 1] = mn, mx
        r[:, 2:] = Q.cycled(e, nrow * per).reshape(nrow, per)
        rows.append(r)
    return np.concatenate(rows)


@pytest.mark.parametrize("n,d,names", [(16, 256, tuple(Q.RANGES_F32)), (64, 1536, Q.HOLDS_ZERO)])
def test_round_trip_of_edge_rows(hq_lib, n, d, names):
    """Encode (hq_map_index_quantize) then decode with the returned min / max == the oracle's decode of the
    oracle's frames: pins the two kernels together at the quantiser's edges."""
    from hq_mi355x import kernels as K
    P = _edge_rows(names, d)
    img = O.map_to_2d(O.pad_parameters(P, n), n)
    enh = O.embed_index_row(img, O.streaming_index(O.map_from_2d(img), n))
    u8, mn, mx = O.normalize_u8(enh)
    ref = D.oracle_decode(u8, mn, mx, d)
    stride = d + 4                                                # 16-byte aligned rows: the fast encoder
    wide = np.zeros((len(P), stride), np.float32)
    wide[:, :d] = P
    fr, _, mm = K.map_index_quantize(_t(wide)[:, :d], n, n)
    _same(_np(fr), u8, "frames")
    _same(_np(K.dequantize_unmap(fr, mm, d)), ref, "round trip")


# ------------------------------------------------------------------------------------------ 6. roundtrip_error


def _np_metrics(o, r):
    return np.array([[np.mean((a - b) ** 2), np.mean(np.abs(a - b)), np.max(np.abs(a - b))] for a, b in zip(o, r)],
                    np.float32)


@pytest.mark.parametrize("d", [1, 7, 8, 9, 128, 129, 255, 1536, 4095])
def test_roundtrip_error_matches_numpy(hq_lib, d):
    from hq_mi355x import kernels as K
    rng = np.random.default_rng(d)
    o = (rng.standard_normal((7, d)) * rng.uniform(0.1, 10, (7, 1))).astype(np.float32)
    r = (o + rng.standard_normal((7, d)).astype(np.float32) * np.float32(0.01)).astype(np.float32)
    r[5] = o[5]
    r[5, d // 2] += np.float32(0.5)                               # one element differs
    r[6] = o[6]                                                   # identical: all zeros
    ref = _np_metrics(o, r)
    assert ref.dtype == np.float32 and np.all(ref[6] == 0) and ref[5, 2] > 0
    _same(_np(K.roundtrip_error(_t(o), _t(r))), ref, f"d={d}")
    _same(_np(K.roundtrip_error(_t(o[0]), _t(r[0]))), ref[0], f"d={d}, one row")
    wide = np.zeros((7, d + 3), np.float32)                       # strided rows
    wide[:, :d] = o
    _same(_np(K.roundtrip_error(_t(wide)[:, :d], _t(r))), ref, f"d={d}, strided")


# ------------------------------------------------------------------------------------------------------ 7. API


def test_reconstruct_device_inverts_quantize_device(hq_lib):
    from hq_mi355x.api import BatchQuantizer
    rng = np.random.default_rng(5)
    X = rng.standard_normal((33, 1536)).astype(np.float32)
    bq = BatchQuantizer()
    bq.quantizer.config.quantization.min_efficiency_ratio = 0.2   # 1536 of 4096 cells
    frames, _, mm = bq.quantize_device(X)
    img = O.map_to_2d(O.pad_parameters(X, 64), 64)
    u8, mn, mx = O.normalize_u8(O.embed_index_row(img, O.streaming_index(O.map_from_2d(img), 64)))
    _same(_np(frames), u8, "frames")
    got = bq.reconstruct_device(frames, mm, 1536)
    assert got.is_cuda and tuple(got.shape) == (33, 1536)
    _same(_np(got), D.oracle_decode(u8, mn, mx, 1536), "reconstruct_device")
    rows, lens = bq.extract_indices_device(frames, mm)
    rrow, rlen = D.oracle_index(u8, mn, mx)
    _same(_np(rows), rrow, "index rows")
    _same(_np(lens), rlen, "index lengths")
    from hq_mi355x.exceptions import HilbertQuantizationError
    with pytest.raises(HilbertQuantizationError, match="Reconstructed parameter count 4096 doesn't match original 4097"):
        bq.reconstruct_device(frames, mm, 4097)


def test_reconstruct_many_mixed_lengths_in_one_group(hq_lib):
    """Two parameter counts that share the 65 x 64 frame shape decode in one fused launch of the larger count;
    every vector equals the per-model reconstruct bytewise."""
    pytest.importorskip("PIL")
    from hq_mi355x.api import HilbertQuantizer
    rng = np.random.default_rng(6)
    sets = [rng.standard_normal(k).astype(np.float32) for k in (4096, 2500, 1024, 2500, 4096, 3001)]
    hq = HilbertQuantizer()
    models = hq.quantize_many(sets, model_ids=[f"m{i}" for i in range(len(sets))])
    want = [hq.reconstruct(m) for m in models]
    got = hq.reconstruct_many(models)
    for a, b, p in zip(got, want, sets):
        assert a.dtype == b.dtype == np.float32 and a.shape == b.shape == p.shape
        assert a.tobytes() == b.tobytes()
    from hq_mi355x.exceptions import ReconstructionError
    bad = dataclasses.replace(models[1], parameter_count=5000)
    with pytest.raises(ReconstructionError, match="Reconstructed parameter count 4096 doesn't match original 5000"):
        hq.reconstruct_many([models[0], bad])
    with pytest.raises(ReconstructionError, match="Reconstructed parameter count 4096 doesn't match original 5000"):
        hq.reconstruct(bad)


REFERENCE_KEYS = {"is_valid", "mse", "mae", "max_error", "tolerance", "parameter_count_match", "compression_ratio",
                  "original_size_bytes", "compressed_size_bytes"}


def test_validate_quantization(hq_lib):
    pytest.importorskip("PIL")
    from hq_mi355x.api import HilbertQuantizer
    rng = np.random.default_rng(8)
    p = rng.standard_normal(3000).astype(np.float32)
    hq = HilbertQuantizer()
    m = hq.quantize(p, model_id="v")
    pipe = hq.quantization_pipeline
    res = pipe.validate_quantization(p, m)
    assert set(res) == REFERENCE_KEYS                             # the compressor drop-in keeps no metrics
    rec = hq.reconstruct(m)
    assert rec.dtype == np.float32
    want = (float(np.mean((p - rec) ** 2)), float(np.mean(np.abs(p - rec))), float(np.max(np.abs(p - rec))))
    assert (res["mse"], res["mae"], res["max_error"]) == want
    assert all(type(res[k]) is float for k in ("mse", "mae", "max_error"))
    assert res["is_valid"] == (want[0] <= 1e-3) and res["tolerance"] == 1e-3 and res["parameter_count_match"] is True
    assert res["compression_ratio"] == m.metadata.compression_ratio
    assert res["original_size_bytes"] == 12000 and res["compressed_size_bytes"] == len(m.compressed_data)
    assert pipe.validate_quantization(p, m, tolerance=0.0)["is_valid"] == (want[0] <= 0.0)
    bad = dataclasses.replace(m, compressed_data=b"\x00\x01not a jpeg")
    fail = pipe.validate_quantization(p, bad)
    assert set(fail) == {"is_valid", "error", "mse", "mae", "max_error"}
    assert fail["is_valid"] is False and "Failed to decompress image" in fail["error"]
    assert fail["mse"] == fail["mae"] == fail["max_error"] == float("inf")
