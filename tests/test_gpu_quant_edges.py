"""GPU parity of the ingest kernels where a quantiser can be wrong: both sides of every byte boundary, subnormal
and near-FLT_MAX ranges, every f16 value of a range, the shapes the dispatchers accept, and batches long
enough for every persistent or grid-stride loop to run several iterations.  Bit-exact against the CPU oracle
throughout.  Inputs come from quant_edges.py; test_quant_edges_cpu.py shows on the CPU that they discriminate.

Input domain (include/hq_mi355x.h): finite values with a finite max - min.  Nothing here feeds NaN, Inf or a
range whose difference overflows."""
import numpy as np
import pytest

from oracle import hq_oracle as O

import quant_edges as Q

pytestmark = pytest.mark.gpu

N_LONG = 41_000     # > 5 x 8192: the largest persistent grid is 256 CUs x 32 one-wave workgroups
N_ROWS = 97         # distinct rows of a long batch (the oracle runs on these, the batch tiles them)


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
    n = int(np.sum(got.reshape(-1) != ref.reshape(-1)))
    raise AssertionError(f"{what}: {n} of {got.size} differ, first at {tuple(int(k) for k in idx)}: "
                         f"got {got[idx]!r}, expected {ref[idx]!r}")


def _same_minmax(mm, mn, mx):
    """min / max by value: the sign of a zero minimum depends on the order of the reduction."""
    mm = np.asarray(mm)
    assert mm.dtype == np.float32 and mm.shape == (len(mn), 2)
    for col, ref, what in ((0, mn, "min"), (1, mx, "max")):
        bad = np.flatnonzero(mm[:, col] != np.asarray(ref, np.float32))
        assert bad.size == 0, f"{what}: {bad.size} rows differ, first row {bad[0]}: got {mm[bad[0], col]!r}, " \
                              f"expected {ref[bad[0]]!r}"


def _tiled(ref, n):
    """The expected output of a batch that tiles the rows `ref` was computed from."""
    reps = -(-n // len(ref))
    return np.tile(ref, (reps,) + (1,) * (ref.ndim - 1))[:n]


def _oracle_fused(P, n, L):
    img = O.map_to_2d(O.pad_parameters(P, n), n)
    idx = O.streaming_index(O.map_from_2d(img), L)
    enh = O.embed_index_row(img, idx)
    u8, mn, mx = O.normalize_u8(enh)
    return u8, idx, mn, mx


def _rows_view(P, d):
    """Device view [N, d] of the first d columns of P, in rows whose stride is a multiple of 4 floats (the
    fast fused path takes 16-byte aligned rows only; a plain [N, d] array with d % 4 != 0 would decline it)."""
    stride = (d + 3) // 4 * 4 + 4
    wide = np.zeros((P.shape[0], stride), np.float32)
    wide[:, :d] = P[:, :d]
    return _t(wide)[:, :d]


def _check_fused(P, n, L, view=False, oracle=None):
    from hq_mi355x import kernels as K
    u8, ridx, mn, mx = oracle if oracle is not None else _oracle_fused(P, n, L)
    fr, idx, mm = K.map_index_quantize(_rows_view(P, P.shape[1]) if view else _t(P), n, L)
    _same_minmax(_np(mm), mn, mx)
    _same(_np(idx), ridx, "index")
    _same(_np(fr), u8, "frame")


# ------------------------------------------------------------------- 1. hq_quantize_u8 / hq_dequantize_u8


def _edge_images(cells):
    """[N, cells] images that between them hold every edge value of every family; every image of three or
    more cells starts with its family's mn, mx.  One-cell images are flat."""
    imgs = []
    for name, (mn, mx) in Q.RANGES_F32.items():
        e = Q.edges(name)
        if cells < 3:
            imgs.append(Q.cycled(e, -(-len(e) // cells) * cells).reshape(-1, cells))
            continue
        per = cells - 2
        nimg = -(-len(e) // per)
        im = np.empty((nimg, cells), np.float32)
        im[:, 0], im[:, 1] = mn, mx
        im[:, 2:] = Q.cycled(e, nimg * per).reshape(nimg, per)
        imgs.append(im)
    return np.concatenate(imgs)


@pytest.mark.parametrize("rows,cols", [(1, 1), (1, 5), (1, 255), (1, 256), (1, 257), (65, 64)])
def test_quantize_edges(hq_lib, rows, cols):
    from hq_mi355x import kernels as K
    E = _edge_images(rows * cols).reshape(-1, rows, cols)
    ru8, rmn, rmx = O.normalize_u8(E)
    if rows * cols >= 3:
        fam_mn = {mn.tobytes() for mn, _ in Q.RANGES_F32.values()}
        assert {v.tobytes() for v in rmn} == fam_mn          # the edges are live: every image has its range
    u8, mm = K.quantize_u8(_t(E))
    _same_minmax(_np(mm), rmn, rmx)
    _same(_np(u8), ru8, "frame")


def test_dequantize_every_byte(hq_lib):
    from hq_mi355x import kernels as K
    pairs = list(Q.RANGES_F32.values()) + [(mn, mn) for mn, _ in Q.RANGES_F32.values()]
    u8 = np.tile(np.arange(256, dtype=np.uint8), (len(pairs), 1)).reshape(len(pairs), 16, 16)
    mm = np.array(pairs, np.float32)
    got = _np(K.dequantize_u8(_t(u8), _t(mm)))
    ref = np.stack([O.denormalize_u8(u8[i], mm[i, 0], mm[i, 1]) for i in range(len(pairs))])
    _same(got, ref, "dequantize")


# --------------------------------------------------------------------------------------- 2. fused kernel


def _edge_rows(names, d):
    """[N, d] rows that between them hold every edge value of the families `names`; each row starts with its
    family's mn, mx.  Returns (rows, per-row mn, per-row mx)."""
    rows, mns, mxs = [], [], []
    for name in names:
        mn, mx = Q.RANGES_F32[name]
        e = Q.edges(name)
        if d < 3:
            continue
        per = d - 2
        nrow = -(-len(e) // per)
        r = np.empty((nrow, d), np.float32)
        r[:, 0], r[:, 1] = mn, mx
        r[:, 2:] = Q.cycled(e, nrow * per).reshape(nrow, per)
        rows.append(r)
        mns += [mn] * nrow
        mxs += [mx] * nrow
    return np.concatenate(rows), np.array(mns, np.float32), np.array(mxs, np.float32)


def _fused_edges(n, d, L, names):
    P, mn, mx = _edge_rows(names, d)
    oracle = _oracle_fused(P, n, L)
    # the edges are live only if padding and index row leave every row's range alone: checked before any launch
    _same(oracle[2], mn, "oracle min")
    _same(oracle[3], mx, "oracle max")
    _check_fused(P, n, L, view=True, oracle=oracle)


ALL_F32 = tuple(Q.RANGES_F32)


@pytest.mark.parametrize("n", [16, 32, 64])
def test_fused_default_edges(hq_lib, n):
    _fused_edges(n, n * n, n, ALL_F32)
    _fused_edges(n, n * n - 57, n, Q.HOLDS_ZERO)           # d % 4 == 3: a straddling group, zero padding


@pytest.mark.parametrize("n,forced", [(16, True), (8, False), (128, False)])
def test_fused_generic_edges(hq_lib, n, forced, hq_option):
    if forced:
        hq_option("fused_generic", 1)
    _fused_edges(n, n * n, n, ALL_F32)
    _fused_edges(n, n * n - 9, n, Q.HOLDS_ZERO)


@pytest.mark.parametrize("variant", [2, 322, 706])
def test_fused_reciprocal_variants_edges(hq_lib, variant, hq_option):
    """The reciprocal quantize (fused_v bit 2) exists for n = 64 with 6 groups per lane only: d = 1536.  The
    row is zero padded, so only the families that hold 0 keep their range; those include `huge` and the four
    ranges in which fl(fl(1 / rng) * 255) overflows (exact division there: recip_ok, hq_common.h)."""
    hq_option("fused_v", variant)
    _fused_edges(64, 1536, 64, Q.HOLDS_ZERO)


# --------------------------------------------------------------------------- 3. chunk encoder, exhaustive


def _oracle_chunks(X, n):
    """Frames, index rows, min, max of the f16 chunks X [nch, cnt] in an n x n geometry."""
    img = O.map_to_2d(X.astype(np.float32), n)              # astype(float32), then zero padded
    ridx = O.traditional_index(img, n)
    u8, mn, mx = O.normalize_u8(O.embed_index_row(img, ridx))
    return u8, ridx, mn, mx


_SWEEPS = {}


def _sweep(name, chunk):
    """(f16 stream, oracle) of a pair's sweep: computed once, shared by the launch forms, never written to."""
    key = (name, chunk)
    if key not in _SWEEPS:
        mn, mx = Q.RANGES_F16[name]
        x = Q.f16_sweep(mn, mx, chunk)
        ref = _oracle_chunks(x.reshape(-1, chunk), O.optimal_dimensions(chunk)[0])
        lo, hi = Q.chunk_frame_range(mn, mx)                       # the index row adds nothing but its 0.0 fill
        assert np.all(ref[2] == lo) and np.all(ref[3] == hi)
        for a in (x,) + ref:
            a.setflags(write=False)
        _SWEEPS[key] = (x, ref)
    return _SWEEPS[key]


def _chunk_mode(mode, hq_option):
    if mode == "generic":
        hq_option("chunk_generic", 1)
    if mode == "exactdiv":
        hq_option("chunk_exactdiv", 1)
    if mode in ("cpw1", "cpw4"):
        hq_option("chunk_cpw", int(mode[-1]))
    if mode == "wpb2":
        hq_option("chunk_wpb", 2)


@pytest.mark.parametrize("chunk", [1024, 4096])
@pytest.mark.parametrize("mode", ["fast", "exactdiv", "generic", "cpw1", "cpw4", "wpb2"])
@pytest.mark.parametrize("name", list(Q.RANGES_F16))
def test_chunk_encoder_every_f16_value(hq_lib, name, mode, chunk, hq_option):
    from hq_mi355x import kernels as K
    _chunk_mode(mode, hq_option)
    x, (u8, ridx, mn, mx) = _sweep(name, chunk)
    fr, idx, mm = K.chunk_encode_f16(_t(x.copy()), chunk)      # the shared sweep is read-only
    _same_minmax(_np(mm), mn, mx)
    _same(_np(idx), ridx, "index")
    _same(_np(fr), u8, "frame")


# ----------------------------------------------------------------------------------------------- 4. shapes


@pytest.mark.parametrize("n,d,L", [(16, 256, 64), (32, 1024, 64), (16, 200, 33), (64, 4096, 1), (16, 1, 16),
                                   (64, 258, 33), (64, 4095, 64), (32, 1022, 32)])
def test_fused_default_shapes(hq_lib, n, d, L):
    rng = np.random.default_rng(n * 100000 + d * 10 + L)
    P = (rng.standard_normal((37, d)) * rng.uniform(0.1, 10)).astype(np.float32)
    P[3] = 0.0                          # all zero
    P[4] = 2.5                          # constant
    P[5] = np.abs(P[5]) + 1.0           # strictly positive
    _check_fused(P, n, L, view=True)


@pytest.mark.parametrize("chunk,nfull,tail", [(256, 70, 128), (300, 5, 200), (100, 9, 64), (4, 50, 2),
                                              (4096, 3, 2048)])
def test_chunk_encoder_other_geometries(hq_lib, chunk, nfull, tail):
    """Chunks other than 1024 / 4096 (the generic kernel), a chunk padded inside its frame, and a tail whose
    geometry is smaller than its slot: the tail is the first (ts + 1) * ts bytes of the slot and the first ts
    index values; the rest of a caller-provided slot is left alone."""
    from hq_mi355x import kernels as K
    import torch
    rng = np.random.default_rng(chunk * 1000 + nfull)
    total = chunk * nfull + tail
    x = (rng.standard_normal(total) * 0.02).astype(np.float16)
    x[chunk:2 * chunk] = np.float16(0.5)                     # constant chunk
    x[2 * chunk:3 * chunk] = np.abs(x[2 * chunk:3 * chunk]) + np.float16(1.0)   # strictly positive
    n = O.optimal_dimensions(chunk)[0]
    ts = O.optimal_dimensions(tail)[0]
    out = (torch.full((nfull + 1, n + 1, n), 7, dtype=torch.uint8, device="cuda"),
           torch.full((nfull + 1, n), 7.0, dtype=torch.float32, device="cuda"),
           torch.full((nfull + 1, 2), 7.0, dtype=torch.float32, device="cuda"))
    fr, idx, mm = (_np(a) for a in K.chunk_encode_f16(_t(x), chunk, out=out))
    u8, ridx, mn, mx = _oracle_chunks(x[:chunk * nfull].reshape(nfull, chunk), n)
    _same_minmax(mm[:nfull], mn, mx)
    _same(idx[:nfull], ridx, "index")
    _same(fr[:nfull], u8, "frame")
    tu8, tidx, tmn, tmx = _oracle_chunks(x[chunk * nfull:][None], ts)
    slot = fr[nfull].reshape(-1)
    nb = (ts + 1) * ts
    _same(slot[:nb].reshape(1, ts + 1, ts), tu8, "tail frame")
    _same(idx[nfull][None, :ts], tidx, "tail index")
    assert mm[nfull, 0] == tmn[0] and mm[nfull, 1] == tmx[0]
    assert np.all(slot[nb:] == 7) and np.all(idx[nfull, ts:] == 7.0)


@pytest.mark.parametrize("chunk", [16, 64, 9, 50])
def test_chunk_encoder_sides_4_and_8_unsupported(hq_lib, chunk):
    """A chunk whose frame side is 4 or 8 has frames that are no multiple of 16 bytes: refused, nothing written."""
    from hq_mi355x import kernels as K
    from hq_mi355x._lib import NativeLibraryError
    import torch
    n = O.optimal_dimensions(chunk)[0]
    assert n in (4, 8)
    x = (np.random.default_rng(chunk).standard_normal(chunk * 5 + 1) * 0.02).astype(np.float16)
    out = (torch.full((6, n + 1, n), 7, dtype=torch.uint8, device="cuda"),
           torch.full((6, n), 7.0, dtype=torch.float32, device="cuda"),
           torch.full((6, 2), 7.0, dtype=torch.float32, device="cuda"))
    with pytest.raises(NativeLibraryError, match=r"error -5: frame stride"):
        K.chunk_encode_f16(_t(x), chunk, out=out)
    torch.cuda.synchronize()
    assert all(bool((a == 7).all()) for a in out)


# ----------------------------------------------------------------------------------------- 5. long batches


def _rows97(shape, seed):
    """97 distinct float32 rows with a constant, an all-zero and a strictly positive row among them."""
    rng = np.random.default_rng(seed)
    R = (rng.standard_normal((N_ROWS,) + shape) * rng.uniform(0.1, 10.0, (N_ROWS,) + (1,) * len(shape))).astype(np.float32)
    R[11] = 0.0
    R[12] = -2.5
    R[13] = np.abs(R[13]) + 1.0
    return R


def test_long_batch_maps(hq_lib):
    from hq_mi355x import kernels as K
    P = _rows97((13,), 1)                                   # 13 of 16 cells: padded rows
    img = K.map_to_2d(_t(_tiled(P, N_LONG)), 4)
    ref = O.map_to_2d(P, 4)
    _same(_np(img), _tiled(ref, N_LONG), "map_to_2d")
    _same(_np(K.map_from_2d(img, 13)), _tiled(P, N_LONG), "map_from_2d")
    _same(_np(K.map_from_2d(img)), _tiled(O.map_from_2d(ref), N_LONG), "map_from_2d full")


def test_long_batch_indices(hq_lib):
    from hq_mi355x import kernels as K
    imgs = _rows97((8, 8), 2)
    dev = _t(_tiled(imgs, N_LONG))
    _same(_np(K.index_streaming(dev, 8)), _tiled(O.streaming_index(O.map_from_2d(imgs), 8), N_LONG), "streaming")
    _same(_np(K.index_traditional(dev, 8)), _tiled(O.traditional_index(imgs, 8), N_LONG), "traditional")
    _same(_np(K.index_rag(dev)), _tiled(O.rag_multi_level_indices(imgs), N_LONG), "rag")


def test_long_batch_block_means(hq_lib):
    """One thread per block mean, at most 8192 x 256 threads: 41,000 images of 16 x 16 one-cell blocks are
    10,496,000 means, five grids and a bit."""
    from hq_mi355x import kernels as K
    imgs = _rows97((16, 16), 3)
    assert N_LONG * 256 > 5 * 8192 * 256
    got = _np(K.block_means(_t(_tiled(imgs, N_LONG)), 16))
    _same(got, _tiled(O.spatial_averages(imgs, 16), N_LONG), "block means")
    small = _rows97((8, 8), 4)                              # 2 x 2 blocks of 4 x 4: a real mean per thread
    got = _np(K.block_means(_t(_tiled(small, N_LONG)), 2))
    _same(got, _tiled(O.spatial_averages(small, 2), N_LONG), "block means 2 x 2")


def test_long_batch_quantize_dequantize(hq_lib):
    from hq_mi355x import kernels as K
    E = _rows97((4, 4), 5)
    u8, mm = K.quantize_u8(_t(_tiled(E, N_LONG)))
    ru8, rmn, rmx = O.normalize_u8(E)
    _same_minmax(_np(mm), _tiled(rmn, N_LONG), _tiled(rmx, N_LONG))
    _same(_np(u8), _tiled(ru8, N_LONG), "frame")
    # de-quantize: 41,000 x 256 elements, more than five times the 8192 x 256 threads of its grid
    B = np.random.default_rng(6).integers(0, 256, (N_ROWS, 16, 16), dtype=np.uint8)
    M = np.stack([rmn, rmx], 1)                             # row 11 and 12 are flat (mn == mx)
    assert N_LONG * 256 > 5 * 8192 * 256
    de = _np(K.dequantize_u8(_t(_tiled(B, N_LONG)), _t(_tiled(M, N_LONG))))
    ref = np.stack([O.denormalize_u8(B[i], M[i, 0], M[i, 1]) for i in range(N_ROWS)])
    _same(de, _tiled(ref, N_LONG), "dequantize")


@pytest.mark.parametrize("n,d,forced", [(4, 13, False), (8, 64, False), (16, 250, True)])
def test_long_batch_fused_generic(hq_lib, n, d, forced, hq_option):
    from hq_mi355x import kernels as K
    if forced:
        hq_option("fused_generic", 1)
    P = _rows97((d,), 7 + n)
    u8, ridx, mn, mx = _oracle_fused(P, n, n)
    fr, idx, mm = K.map_index_quantize(_t(_tiled(P, N_LONG)), n, n)
    _same_minmax(_np(mm), _tiled(mn, N_LONG), _tiled(mx, N_LONG))
    _same(_np(idx), _tiled(ridx, N_LONG), "index")
    _same(_np(fr), _tiled(u8, N_LONG), "frame")


@pytest.mark.parametrize("chunk", [4, 1024])
def test_long_batch_chunk_generic(hq_lib, chunk, hq_option):
    from hq_mi355x import kernels as K
    hq_option("chunk_generic", 1)
    rng = np.random.default_rng(chunk)
    X = (rng.standard_normal((N_ROWS, chunk)) * 0.02).astype(np.float16)
    X[11] = np.float16(0.0)
    X[12] = np.float16(0.5)
    X[13] = np.abs(X[13]) + np.float16(1.0)
    u8, ridx, mn, mx = _oracle_chunks(X, O.optimal_dimensions(chunk)[0])
    fr, idx, mm = K.chunk_encode_f16(_t(_tiled(X, N_LONG).reshape(-1)), chunk)
    _same_minmax(_np(mm), _tiled(mn, N_LONG), _tiled(mx, N_LONG))
    _same(_np(idx), _tiled(ridx, N_LONG), "index")
    _same(_np(fr), _tiled(u8, N_LONG), "frame")
