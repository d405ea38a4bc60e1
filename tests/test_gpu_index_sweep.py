"""GPU parity of the index generators over every branch of the slot plan: `k_trad_image`, `k_stream_index`,
`k_rag` and `k_block_means` against the CPU oracle, byte for byte with dtype and shape, for n = 1 .. 128, float32
and float64 images, L = 1 .. 130 plus the plan's edge lengths, padded streams, and batches long enough for the
persistent loops.  tests/test_index_sweep_cpu.py pins the oracle to the real reference over the same sweep
(tests/golden/index_sweep.npz), so the oracle is the only expectation needed here; the drop-in classes are also
compared with the reference's own recorded arrays."""
from unittest import mock

import numpy as np
import pytest

import index_sweep_cases as S
from oracle import hq_oracle as O

pytestmark = pytest.mark.gpu

N_LONG = 41_000     # > 5 x 8192 workgroups of the persistent one-wave kernels
N_ROWS = 97


def _t(x):
    from hq_mi355x._dev import to_dev
    return to_dev(x)


def _np(x):
    from hq_mi355x._dev import to_np
    return to_np(x)


def _same(got, ref, what=""):
    got, ref = np.ascontiguousarray(got), np.ascontiguousarray(ref)
    assert got.shape == ref.shape and got.dtype == ref.dtype, (what, got.shape, ref.shape, got.dtype, ref.dtype)
    if got.tobytes() == ref.tobytes():
        return
    a, b = got.reshape(-1).view(np.uint8), ref.reshape(-1).view(np.uint8)
    i = int(np.flatnonzero(a != b)[0]) // got.dtype.itemsize
    idx = np.unravel_index(i, got.shape)
    n = int(np.any(a.reshape(-1, got.dtype.itemsize) != b.reshape(-1, got.dtype.itemsize), axis=1).sum())
    raise AssertionError(f"{what}: {n} of {got.size} differ, first at {tuple(int(k) for k in idx)}: "
                         f"got {got[idx]!r}, expected {ref[idx]!r}")


def _tiled(ref, n):
    reps = -(-n // len(ref))
    return np.tile(ref, (reps,) + (1,) * (ref.ndim - 1))[:n]


@pytest.fixture(scope="module")
def g(golden):
    return golden("index_sweep")


def _memo_block_means():
    """O.spatial_averages memoised per (batch, grid): the traditional oracle asks for the same grids at every L.
    Results are the oracle's own, computed once."""
    real, cache = O.spatial_averages, {}

    def cached(img, grid):
        key = (id(img), img.shape, img.dtype.str, grid)
        if key not in cache:
            cache[key] = real(img, grid)
        return cache[key]

    return mock.patch.object(O, "spatial_averages", cached)


def _sweep(K, batch, lengths, what):
    dev = _t(batch)
    stream = O.map_from_2d(batch)
    with _memo_block_means():
        for L in lengths:
            _same(_np(K.index_traditional(dev, L)), O.traditional_index(batch, L), f"{what} traditional L={L}")
            _same(_np(K.index_streaming(dev, L)), O.streaming_index(stream, L), f"{what} streaming L={L}")


@pytest.mark.parametrize("n", S.SIDES_F32)
def test_sweep_float32(hq_lib, g, n):
    from hq_mi355x import kernels as K
    batch = S.gpu_batch(g[f"img_f32_n{n}"])
    assert batch.dtype == np.float32 and np.isfinite(batch).all()
    assert n == 1 or np.signbit(batch[2][batch[2] == 0]).any()
    _sweep(K, batch, S.LS_GPU, f"f32 n={n}")
    _same(_np(K.index_rag(_t(batch))), O.rag_multi_level_indices(batch), f"rag n={n}")


@pytest.mark.parametrize("n", S.SIDES_F64)
def test_sweep_float64(hq_lib, g, n):
    """Float64 images: means and samples in float64, one rounding to float32 at the store.  (The float32-cast
    route differs from the reference in 9 of 10 (n, L) cases tried.)"""
    from hq_mi355x import kernels as K
    batch = S.gpu_batch(g[f"img_f64_n{n}"])
    assert batch.dtype == np.float64
    _sweep(K, batch, S.LS_GPU, f"f64 n={n}")


def test_other_dtypes_widen_to_float64(hq_lib):
    from hq_mi355x import kernels as K
    img = np.random.default_rng(5).integers(-2 ** 30, 2 ** 30, (2, 16, 16)).astype(np.int32)   # not exact in float32
    for L in (5, 16, 40):
        _same(_np(K.index_traditional(_t(img), L)), O.traditional_index(img.astype(np.float64), L), f"int32 L={L}")


@pytest.mark.parametrize("kind,n", S.BLOCK_IMAGES)
def test_block_means_both_orders(hq_lib, g, kind, n):
    """Dividing, non-dividing (3, 5) and too-large grids; order 1 (the RAG generator's Hilbert order) is defined
    for power-of-two grids only."""
    from hq_mi355x import kernels as K
    batch = S.gpu_batch(g[f"img_{kind}_n{n}"])
    dev = _t(batch)
    for grid in S.GRIDS:
        got = _np(K.block_means(dev, grid, 0))
        _same(got, O.spatial_averages(batch, grid), f"{kind} n={n} grid={grid} row-major")
        want = g[f"block_{kind}_n{n}_g{grid}"]                      # the reference's list of Python floats
        assert got[0].astype(np.float64).tobytes() == want.tobytes(), (kind, n, grid)
        if grid & (grid - 1) == 0:
            _same(_np(K.block_means(dev, grid, 1)), O.rag_hilbert_order_averages(batch, grid),
                  f"{kind} n={n} grid={grid} hilbert")


def test_dropin_traditional_matches_reference_arrays(hq_lib, g):
    """generate_optimized_indices returns the reference's dtype, shape and bytes, including the empty float64
    array of an empty allocation (L = 1) and of L = 0, for float32 and float64 images."""
    from hq_mi355x.core.index_generator import HierarchicalIndexGeneratorImpl, QuantizationConfig
    from hq_mi355x.core.streaming_index_builder import StreamingHilbertIndexGenerator
    gen = HierarchicalIndexGeneratorImpl()
    sgen = HierarchicalIndexGeneratorImpl(QuantizationConfig(use_streaming_optimization=True))
    for kind, n in [("f32", 8), ("f64", 8), ("f64", 32), ("f32", 1), ("f32", 64)]:
        img = g[f"img_{kind}_n{n}"]
        for L in S.LS_FULL:
            _same(gen.generate_optimized_indices(img, L), g[f"trad_{kind}_n{n}_L{L}"], f"trad {kind} n={n} L={L}")
            _same(sgen.generate_optimized_indices(img, L), g[f"strm_{kind}_n{n}_L{L}"], f"strm {kind} n={n} L={L}")
            _same(StreamingHilbertIndexGenerator().generate_optimized_indices(img, L), g[f"strm_{kind}_n{n}_L{L}"])
        for L in (0, -3):                                            # core/index_generator.py:303-304
            _same(gen.generate_optimized_indices(img, L), np.array([]), f"trad {kind} n={n} L={L}")
        assert g[f"trad_{kind}_n{n}_L1"].dtype == np.float64 and g[f"trad_{kind}_n{n}_L1"].shape == (0,)
        assert g[f"trad_{kind}_n{n}_L2"].dtype == np.float32 and g[f"trad_{kind}_n{n}_L2"].shape == (2,)


@pytest.mark.parametrize("n,d", S.PADDED)
def test_dropin_padded_streams(hq_lib, g, n, d):
    """generate_indices_during_mapping with d < n * n: the tree covers d values, partial groups never promote."""
    from hq_mi355x.core.streaming_index_builder import StreamingHilbertIndexGenerator
    p = g[f"pad_params_n{n}_d{d}"]
    sg = StreamingHilbertIndexGenerator()
    for i, L in enumerate(S.padded_ls(n)):
        img, idx, stats = sg.generate_indices_during_mapping(p, (n, n), L)
        want_img = O.map_to_2d(p, n)
        _same(np.asarray(img), want_img, f"image n={n} d={d}")
        _same(np.asarray(idx), O.streaming_index(O.map_from_2d(want_img)[:d], L), f"index n={n} d={d} L={L}")
        assert S.digest(np.asarray(idx)) == g[f"pad_dig_n{n}_d{d}"][i].tobytes(), (n, d, L)
        assert stats["total_values_processed"] == d


def test_long_batch_sampling_level(hq_lib):
    """41,000 images through the persistent loops at L = 11: a non-power-of-two length whose plan has two
    block-mean levels, a corner / centre sampling level and a zero slot."""
    from hq_mi355x import kernels as K
    rng = np.random.default_rng(11)
    imgs = (rng.standard_normal((N_ROWS, 8, 8)) * rng.uniform(0.1, 10.0, (N_ROWS, 1, 1))).astype(np.float32)
    imgs[11] = 0.0
    imgs[12] = -2.5
    assert O.traditional_allocation(11) == [(2, 4), (1, 1), (2, 6)]
    dev = _t(_tiled(imgs, N_LONG))
    _same(_np(K.index_traditional(dev, 11)), _tiled(O.traditional_index(imgs, 11), N_LONG), "traditional")
    _same(_np(K.index_streaming(dev, 11)), _tiled(O.streaming_index(O.map_from_2d(imgs), 11), N_LONG), "streaming")
    dev64 = _t(_tiled(imgs.astype(np.float64) * 1.1, N_LONG))
    _same(_np(K.index_traditional(dev64, 11)), _tiled(O.traditional_index(imgs.astype(np.float64) * 1.1, 11), N_LONG),
          "traditional f64")
