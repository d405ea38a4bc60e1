"""hq_jpeg_encode without a GPU: the export, its argument checks (which return before any device work) and the
ingest API's codec switch."""
import numpy as np
import pytest


def test_export_and_argument_rules():
    from hq_mi355x import _lib
    lib = _lib.load()
    assert hasattr(lib, "hq_jpeg_encode") and len(_lib.SIGNATURES["hq_jpeg_encode"][1]) == 10
    enc = lambda N, H, W, q: lib.hq_jpeg_encode(None, N, H, W, q, None, None, None, None, None)
    assert enc(0, 65, 64, 76) == _lib.HQ_OK                                    # empty batch: no launch
    assert enc(3, 65, 64, 76) == _lib.HQ_E_INVALID and _lib.last_error() == "null buffer"
    assert enc(-1, 65, 64, 76) == _lib.HQ_E_INVALID and enc(3, 0, 64, 76) == _lib.HQ_E_INVALID
    for q in (0, 96, -5):
        assert enc(3, 65, 64, q) == _lib.HQ_E_UNSUPPORTED and "1 <= q <= 95" in _lib.last_error()
    assert enc(3, 131, 128, 1) == _lib.HQ_E_INVALID and enc(3, 168, 176, 95) == _lib.HQ_E_INVALID  # 272, 462 blocks fit
    for H, W in ((8, 3832), (257, 256), (70000, 8)):                            # 479, 1056, 8750 blocks
        assert enc(3, H, W, 76) == _lib.HQ_E_UNSUPPORTED and "at most 477 fit the LDS" in _lib.last_error()


def test_unknown_codec_is_refused():
    from hq_mi355x.api import BatchQuantizer, HilbertQuantizer
    x = [np.zeros(1024, dtype=np.float32)]
    with pytest.raises(ValueError, match="codec must be 'host' or 'device', got 'bogus'"):
        HilbertQuantizer().quantize_many(x, codec="bogus")
    with pytest.raises(ValueError, match="codec must be"):
        BatchQuantizer().quantize_batch(x, codec="bogus")
