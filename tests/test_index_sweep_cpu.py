"""The oracle's index generators against the real reference over the whole slot-plan sweep
(tests/golden/index_sweep.npz, written by tests/golden/make_golden.py from tests/index_sweep_cases.py).

Every recorded case is compared by dtype, shape and bytes (an 8-byte digest, full arrays at a few lengths), so
the GPU tests of tests/test_gpu_index_sweep.py need only the oracle.  Runs anywhere: no reference, no GPU."""
import numpy as np
import pytest

import index_sweep_cases as S
from oracle import hq_oracle as O


@pytest.fixture(scope="module")
def g(golden):
    return golden("index_sweep")


def ref_traditional(img, L):
    """What the reference's generate_optimized_indices returns for one image: the oracle's row, or the empty
    float64 array where the level allocation is empty (L = 1, core/index_generator.py:318-319)."""
    if not O.traditional_allocation(L):
        return np.array([])
    return O.traditional_index(img, L)


def ref_streaming(img, L):
    return O.streaming_index(O.map_from_2d(img), L)


def ref_padded(p, n, L):
    img = O.map_to_2d(O.pad_parameters(p, n), n)
    return img, O.streaming_index(O.map_from_2d(img)[: len(p)], L)


def test_case_tables_match_the_golden(g):
    assert list(g["LS"]) == S.LS and list(g["LS_FULL"]) == S.LS_FULL
    assert set(S.LS_FULL) <= set(S.LS) and set(S.LS_GPU) <= set(S.LS)
    for (kind, n), img in S.make_images().items():
        stored = g[f"img_{kind}_n{n}"]
        assert stored.dtype == img.dtype and stored.shape == (n, n)
    raised = [(k, str(e)) for k in g if "_err_" in k for e in g[k] if str(e)]
    assert raised == [], "the reference raises in none of the recorded cases"


def test_digest_scheme_on_full_arrays(g):
    """The digest of every fully stored array is the recorded digest, and it tells dtype and shape apart."""
    for kind, n in S.image_tags():
        for name in ("trad", "strm"):
            for L in S.LS_FULL:
                full = g[f"{name}_{kind}_n{n}_L{L}"]
                assert S.digest(full) == g[f"{name}_dig_{kind}_n{n}"][S.LS.index(L)].tobytes(), (name, kind, n, L)
    z32, z64 = np.zeros(1, np.float32), np.zeros(1, np.float64)
    assert len({S.digest(z32), S.digest(z64), S.digest(np.zeros(2, np.float32)), S.digest(np.zeros((1, 1), np.float32)),
                S.digest(np.array([])), S.digest(-z32)}) == 6


@pytest.mark.parametrize("kind,n", S.image_tags())
def test_traditional_and_streaming_digests(g, kind, n):
    img = g[f"img_{kind}_n{n}"]
    for name, fn in (("trad", ref_traditional), ("strm", ref_streaming)):
        dig = g[f"{name}_dig_{kind}_n{n}"]
        bad = [L for i, L in enumerate(S.LS) if S.digest(fn(img, L)) != dig[i].tobytes()]
        assert not bad, f"{name} {kind} n={n}: oracle differs from the reference at L={bad[:10]}"
        for L in S.LS_FULL:
            got, want = fn(img, L), g[f"{name}_{kind}_n{n}_L{L}"]
            assert got.dtype == want.dtype and got.shape == want.shape and got.tobytes() == want.tobytes(), (name, L)


def test_traditional_empty_allocation(g):
    """L = 1 leaves the allocation empty: the reference returns np.array([]) (float64, shape (0,))."""
    assert O.traditional_allocation(1) == [] and O.traditional_allocation(2) != []
    want = g["trad_f32_n8_L1"]
    assert want.dtype == np.float64 and want.shape == (0,)


def test_float64_images_differ_from_their_float32_cast(g):
    """The float64 cases are worth having: rounding the image to float32 first changes the index."""
    changed = 0
    for n in S.SIDES_F64:
        img = g[f"img_f64_n{n}"]
        for L in (5, 16, 32, 100, 300):
            changed += O.traditional_index(img, L).tobytes() != O.traditional_index(img.astype(np.float32), L).tobytes()
    assert changed >= 5


@pytest.mark.parametrize("n,d", S.PADDED)
def test_padded_streams(g, n, d):
    p = g[f"pad_params_n{n}_d{d}"]
    assert S.digest(S.make_padded_params()[(n, d)]) == S.digest(p)
    for i, L in enumerate(S.padded_ls(n)):
        img, idx = ref_padded(p, n, L)
        assert S.digest(idx) == g[f"pad_dig_n{n}_d{d}"][i].tobytes(), (n, d, L)
    assert S.digest(img) == g[f"pad_img_dig_n{n}_d{d}"].tobytes()


def test_rag_rows(g):
    for kind, sides in (("f32", S.RAG_SIDES_F32), ("f64", S.SIDES_F64)):
        for n in sides:
            img = g[f"img_{kind}_n{n}"] if n <= 128 else S.image_256(g["img_f32_n128"])
            want = g[f"rag_rows_{kind}_n{n}"]
            got = O.rag_multi_level_indices(img)[n:]
            assert got.dtype == want.dtype and got.shape == want.shape and got.tobytes() == want.tobytes(), (kind, n)


def test_block_averages(g):
    for kind, n in S.BLOCK_IMAGES:
        img = g[f"img_{kind}_n{n}"]
        for grid in S.GRIDS:
            want = g[f"block_{kind}_n{n}_g{grid}"]
            got = O.spatial_averages(img[None], grid)[0].astype(np.float64)   # the reference's float(np.mean(...))
            assert got.shape == want.shape and got.tobytes() == want.tobytes(), (kind, n, grid)
