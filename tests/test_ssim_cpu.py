"""Argument checks of the SSIM entries (hq_ssim.hip): every refusal returns before any launch, with the library's
message.  No GPU is needed."""
import pytest


@pytest.fixture(scope="module")
def lib():
    from hq_mi355x import _lib
    return _lib.load()


def _calls(lib, H, W, N=5, Q=3, C=4, p=8):
    """The three entries with every pointer = p (never dereferenced: the checks refuse first)."""
    return [lambda: lib.hq_ssim_prepare(p, N, H, W, p, p, None),
            lambda: lib.hq_ssim_scores(p, p, p, Q, p, N, H, W, p, p, None),
            lambda: lib.hq_ssim_scores_listed(p, p, p, Q, p, N, H, W, p, C, p, p, None)]


@pytest.mark.parametrize("H,W", [(3, 8), (8, 3), (132, 64), (64, 129)])
def test_frame_limits(lib, H, W):
    from hq_mi355x import _lib
    assert lib.hq_ssim_maps_bytes(H, W) == 0
    for call in _calls(lib, H, W):
        assert call() == _lib.HQ_E_UNSUPPORTED
        assert _lib.last_error() == f"SSIM frames are 4 x 4 to 131 x 128 (window 7), got {H} x {W}"


def test_null_misaligned_and_empty_list(lib):
    from hq_mi355x import _lib
    for call in _calls(lib, 33, 32, p=None):
        assert call() == _lib.HQ_E_INVALID and _lib.last_error() == "null buffer"
    assert lib.hq_ssim_scores(8, 8, 8, 3, 8, 5, 33, 32, None, None, None) == _lib.HQ_E_INVALID  # null output
    assert _lib.last_error() == "null buffer"
    for call in _calls(lib, 33, 32, p=12):
        assert call() == _lib.HQ_E_INVALID and "8-byte aligned" in _lib.last_error()
    assert _calls(lib, 33, 32, C=0)[2]() == _lib.HQ_E_INVALID
    assert _lib.last_error() == "a list holds 1 .. 65535 entries, got C = 0"
    assert lib.hq_ssim_scores(None, None, None, 0, None, 5, 33, 32, None, None, None) == 0  # nothing to do


def test_maps_bytes(lib):
    assert lib.hq_ssim_maps_bytes(65, 64) == 16 * 65 * 64
    assert lib.hq_ssim_maps_bytes(4, 4) == 256 and lib.hq_ssim_maps_bytes(131, 128) == 16 * 131 * 128
