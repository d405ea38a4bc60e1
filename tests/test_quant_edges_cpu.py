"""The quantiser edge inputs have teeth (no GPU): the values test_gpu_quant_edges.py feeds the kernels sit on
both sides of every byte boundary, the fast kernels' reciprocal form without its fallback is wrong on them,
and the fallback as designed repairs it, except in the ranges where fl(fl(1 / rng) * 255) overflows."""
import numpy as np
import pytest

from oracle import hq_oracle as O

import quant_edges as Q

FULL = [k for k in Q.RANGES_F32 if k not in ("big_offset", "few_ulps")]
FORMS = ("qfast", "packed")


def test_families_are_in_the_input_domain():
    for name, (mn, mx) in Q.RANGES_F32.items():
        assert mn.dtype == np.float32 and mx.dtype == np.float32
        assert np.isfinite(mn) and np.isfinite(mx) and mn < mx and np.isfinite(mx - mn), name
    assert [k for k in Q.RANGES_F32 if Q.full_range(k)] == FULL
    assert set(Q.RECIP_OVERFLOW) == {k for k, (mn, mx) in Q.RANGES_F32.items() if mx - mn < 7.5e-37}
    assert len(Q.RECIP_OVERFLOW) == 4
    with np.errstate(over="ignore"):
        for name, (mn, mx) in Q.RANGES_F32.items():
            c255 = np.float32(np.float32(1.0) / (mx - mn)) * np.float32(255.0)
            assert np.isinf(c255) == (name in Q.RECIP_OVERFLOW), name
    assert len(Q.RANGES_F16) == 8
    for name, (mn, mx) in Q.RANGES_F16.items():
        assert mn.dtype == np.float16 and mx.dtype == np.float16 and np.isfinite(mn) and np.isfinite(mx) and mn < mx


@pytest.mark.parametrize("name", list(Q.RANGES_F32))
def test_level_edges_straddle_every_boundary(name):
    mn, mx = Q.RANGES_F32[name]
    b = Q.boundaries(mn, mx)
    e = Q.edges(name)
    assert e.dtype == np.float32 and e[0] == mn and e[-1] == mx and np.all(np.diff(e) > 0)
    by = Q.oracle_bytes(e, mn, mx)
    if name in FULL:
        assert [k for k, _ in b] == list(range(1, 256))
        assert np.array_equal(np.unique(by), np.arange(256))
    else:
        assert 0 < len(b) < 255
        assert np.array_equal(np.unique(by), np.unique(Q.oracle_bytes(_all_f32(mn, mx), mn, mx)))
    where = {x.tobytes(): i for i, x in enumerate(e)}
    for k, x in b:
        lo = np.nextafter(x, np.float32(-np.inf))
        assert mn <= lo < x <= mx
        i = where[x.tobytes()]
        assert e[i - 1] == lo                                   # both sides of the boundary are fed ...
        assert by[i] >= k and by[i - 1] == k - 1                # ... and the byte changes between them
        # one more neighbour on each side (clipped to the range)
        assert i < 2 or e[i - 2] == np.nextafter(lo, np.float32(-np.inf))
        assert x == mx or e[i + 1] == np.nextafter(x, np.float32(np.inf))


def _all_f32(mn, mx):
    o = np.arange(Q._ordinal(mn), Q._ordinal(mx) + 1)
    return Q._from_ordinal(o)


def test_ordinals_walk_the_float32_line():
    x = np.array([-1.0, -1e-45, -0.0, 0.0, 1e-45, 1.0, 3.0e38], np.float32)
    o = Q._ordinal(x)
    assert np.all(np.diff(o) >= 0) and o[2] == o[3] == 0 and o[4] == 1 and o[1] == -1
    assert Q._from_ordinal(o).tobytes() == np.where(x == 0, np.float32(0), x).astype(np.float32).tobytes()
    assert Q._from_ordinal(Q._ordinal(np.float32(1.0)) + 1) == np.nextafter(np.float32(1.0), np.float32(2.0))
    assert Q._from_ordinal(Q._ordinal(np.float32(-1.0)) + 1) == np.nextafter(np.float32(-1.0), np.float32(0.0))


@pytest.mark.parametrize("name", ["wide", "huge"])
def test_unguarded_reciprocal_is_wrong_on_the_edges(name):
    """At least 100 edge values get the wrong byte from the packed form without its fallback (correctly
    rounded reciprocal): 116 of 1020 for `wide`, 223 of 1021 for `huge`."""
    mn, mx = Q.RANGES_F32[name]
    e = Q.edges(name)
    ref = Q.oracle_bytes(e, mn, mx)
    for form in FORMS:
        got, _ = Q.recip_model(e, mn, mx, 0, form)
        wrong = int(np.sum(got != ref))
        print(name, form, wrong, "of", len(e))
        assert wrong >= 100, (name, form, wrong)


def test_searched_f16_pairs():
    """The four searched pairs come from the seeded search, and each holds an f16 value that both unguarded
    forms quantize wrongly for every rounding of the reciprocal."""
    found = Q.search_f16_pairs()
    assert [(a.tobytes(), b.tobytes()) for a, b in found] == \
        [(Q.RANGES_F16[k][0].tobytes(), Q.RANGES_F16[k][1].tobytes()) for k in Q.SEARCHED_F16]
    for k in Q.SEARCHED_F16:
        mn, mx = Q.RANGES_F16[k]
        v = Q.f16_values(mn, mx).astype(np.float32)
        ref = Q.oracle_bytes(v, mn, mx)
        for form in FORMS:
            for ulp in (-1, 0, 1):
                assert np.any(Q.recip_model(v, mn, mx, ulp, form)[0] != ref), (k, form, ulp)


def test_f16_sweep_holds_every_value_in_every_chunk_range():
    for name, (mn, mx) in Q.RANGES_F16.items():
        vals = Q.f16_values(mn, mx)
        assert vals[0] == mn and vals[-1] == mx
        bits = np.sort(vals.view(np.uint16))
        for chunk in (1024, 4096):
            x = Q.f16_sweep(mn, mx, chunk)
            assert x.dtype == np.float16 and x.size % chunk == 0 and np.all(np.isfinite(x))
            c = x.reshape(-1, chunk)
            assert np.all(c.min(axis=1) == mn) and np.all(c.max(axis=1) == mx)
            assert np.array_equal(np.unique(x.view(np.uint16)), bits), name
    n_all = Q.f16_values(*Q.RANGES_F16["full"]).size
    assert n_all == 2 * (0x7C00)                       # every finite f16 bit pattern, both zeros
    sub = Q.f16_values(*Q.RANGES_F16["subnormal"])
    assert sub.size == 1025 and np.all(np.abs(sub.astype(np.float32)) < 2.0 ** -14)   # -0, +0, 1023 subnormals


@pytest.mark.parametrize("name", list(Q.RANGES_F32))
def test_guarded_model_f32(name):
    """With the fallback the reciprocal forms agree with the oracle on every edge value, except where the
    design's assumptions fail: the packed form where fl(fl(1 / rng) * 255) is inf (the four ranges below
    7.5e-37), qfast where fl(1 / rng) itself is inf (the two subnormal ranges).  There they must disagree:
    y is inf or NaN, the guard compares false, nothing asks for the exact division.  The kernels therefore
    take the reciprocal form only for rng in [2^-100, 2^100] (hq_common.h: recip_ok)."""
    mn, mx = Q.RANGES_F32[name]
    e = Q.edges(name)
    ref = Q.oracle_bytes(e, mn, mx)
    # a reciprocal one ulp off only where 1 / rng is a normal number (1 ulp of a subnormal is not 2^-23)
    ulps = (0,) if name == "huge" else (-1, 0, 1)
    for form in FORMS:
        broken = name in Q.RECIP_OVERFLOW if form == "packed" else name in ("subnormal", "subnormal_signed")
        for ulp in ulps:
            wrong = int(np.sum(Q.guarded_model(e, mn, mx, ulp, form) != ref))
            print(name, form, ulp, wrong, "of", len(e))
            if broken:
                assert wrong > len(e) // 2, (name, form, ulp, wrong)
            else:
                assert wrong == 0, (name, form, ulp, wrong)


def test_guarded_model_f16_exhaustive():
    """Every f16 value of every f16 range: the guarded forms agree with the oracle (f16 data keeps rng in
    [2^-24, 131008], well inside the reciprocal form's domain)."""
    for name, (mn, mx) in Q.RANGES_F16.items():
        v = Q.f16_values(mn, mx).astype(np.float32)
        mn, mx = Q.chunk_frame_range(mn, mx)               # the index row's zero fill belongs to the frame
        ref = Q.oracle_bytes(v, mn, mx)
        assert 2.0 ** -24 <= mx - mn <= 131008
        for form in FORMS:
            for ulp in (-1, 0, 1):
                assert np.array_equal(Q.guarded_model(v, mn, mx, ulp, form), ref), (name, form, ulp)


def test_recip_ok_window():
    """rng in [2^-100, 2^100] keeps 1 / rng and fl(1 / rng) * 255 normal float32 numbers, with room to
    spare; every family outside the window is one of `huge` and the overflow ranges."""
    tiny = np.finfo(np.float32).tiny
    for rng in (np.float32(2.0 ** -100), np.float32(2.0 ** 100)):
        r = np.float32(1.0) / rng
        assert tiny <= r and np.isfinite(r * np.float32(255.0)) and tiny <= r * np.float32(255.0)
    outside = {k for k, (mn, mx) in Q.RANGES_F32.items() if not 2.0 ** -100 <= float(mx - mn) <= 2.0 ** 100}
    assert outside == set(Q.RECIP_OVERFLOW) | {"huge"}


def test_oracle_bytes_is_the_oracle():
    mn, mx = Q.RANGES_F32["wide"]
    e = Q.edges("wide")
    u8, rmn, rmx = O.normalize_u8(e.reshape(1, 1, -1))
    assert rmn[0] == mn and rmx[0] == mx
    assert np.array_equal(u8.reshape(-1), Q.oracle_bytes(e, mn, mx))
    assert np.array_equal(Q.cycled(np.arange(3), 8, first=(9, 9)), [9, 9, 0, 1, 2, 0, 1, 2])
