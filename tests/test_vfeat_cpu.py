"""Video features without a GPU: the header's rule for the 8 magnitude bins equals np.histogram on every frame family,
the library's argument checks return before any launch, and the package refuses to run without a device."""
import numpy as np
import pytest

import vfeat_cases as V


@pytest.mark.parametrize("H,W", [(4, 4), (7, 9), (33, 32), (65, 64)])
@pytest.mark.parametrize("family", V.FAMILIES)
def test_bin_rule_is_np_histogram(family, H, W):
    for g in V.make(family, H, W):
        m = V.sobel(g)[2]
        assert V.bin_rule(m).tolist() == np.histogram(m.ravel(), bins=8)[0].tolist()


def test_argument_checks():
    from hq_mi355x import _lib
    lib = _lib.load()
    w = (_lib.ctypes.c_double * 3)(0.3, 0.2, 0.1)
    for H, W in [(3, 8), (8, 3), (132, 128), (4, 4193)]:
        assert lib.hq_vfeat_extract(8, 5, H, W, 8, None) == _lib.HQ_E_UNSUPPORTED
        assert _lib.last_error() == f"video-feature frames have sides >= 4 and at most 16768 pixels, got {H} x {W}"
    assert lib.hq_vfeat_extract(None, 5, 8, 8, None, None) == _lib.HQ_E_INVALID and _lib.last_error() == "null buffer"
    assert lib.hq_vfeat_extract(None, 0, 8, 8, None, None) == _lib.HQ_OK
    assert lib.hq_vfeat_scores(8, 3, 8, 5, w, 12, None) == _lib.HQ_E_INVALID and "8-byte" in _lib.last_error()
    assert lib.hq_vfeat_scores(8, 3, 8, 5, None, 8, None) == _lib.HQ_E_INVALID
    assert lib.hq_vfeat_scores(None, 0, None, 5, w, None, None) == _lib.HQ_OK
    bad = (_lib.ctypes.c_double * 3)(0.3, -0.2, 0.1)
    assert lib.hq_vfeat_scores(8, 3, 8, 5, bad, 8, None) == _lib.HQ_E_INVALID and "weights" in _lib.last_error()
    assert lib.hq_vfeat_scores_listed(8, 3, 8, 5, w, 8, 0, None, 8, None, None) == _lib.HQ_E_INVALID
    assert _lib.last_error() == "a list holds 1 .. 65535 entries, got C = 0"
    assert lib.hq_vfeat_scores_listed(8, 3, 8, 5, w, 8, 4, 8, 8, None, None) == _lib.HQ_E_INVALID
    assert "together" in _lib.last_error()


def test_no_gpu_no_fallback():
    import torch
    if torch.cuda.is_available():
        return
    from hq_mi355x._lib import NativeLibraryError
    from hq_mi355x.core import VideoFeatureIndex, extract_video_features
    frames = V.make("random", 8, 8)
    with pytest.raises(NativeLibraryError):
        VideoFeatureIndex(frames)
    with pytest.raises(NativeLibraryError):
        extract_video_features(frames[0])
    with pytest.raises(TypeError):
        extract_video_features(frames[0].astype(np.float64))
