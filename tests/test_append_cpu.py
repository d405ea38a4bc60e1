"""CPU-side checks of the appendable corpus: hq_seg_append is exported and validates its arguments before
any device work, and HilbertQuantizer's registry add / remove methods behave like the reference's
(api.py:299-325, :542-551).  No kernel is launched here."""
import ctypes

import numpy as np
import pytest


@pytest.fixture(scope="module")
def lib():
    from hq_mi355x import _lib
    return _lib.load()


def _append(lib, idx, M, L, Z, stats, N0=0):
    return lib.hq_seg_append(idx, M, L, 0, None, N0, Z, stats, None, None, None, None, None, None)


def test_symbol_exported(lib):
    from hq_mi355x._lib import SIGNATURES
    assert hasattr(lib, "hq_seg_append")
    assert "hq_seg_append" in SIGNATURES


def test_argument_validation(lib):
    from hq_mi355x import _lib
    buf = (ctypes.c_double * 64)()
    p = ctypes.cast(buf, ctypes.c_void_p)
    assert _append(lib, None, 0, 64, None, None) == _lib.HQ_OK                  # M == 0: nothing to write
    assert _append(lib, None, 0, 64, None, None, N0=17) == _lib.HQ_OK
    assert _append(lib, p, 1, 64, None, p) == _lib.HQ_E_INVALID                 # null Z with M > 0
    assert _lib.last_error() == "null buffer"
    assert _append(lib, p, 1, 64, p, None) == _lib.HQ_E_INVALID                 # null stats
    assert _append(lib, None, 1, 64, p, p) == _lib.HQ_E_INVALID                 # null rows
    assert _append(lib, p, -1, 64, p, p) == _lib.HQ_E_INVALID                   # bad shapes
    assert _append(lib, p, 1, 0, p, p) == _lib.HQ_E_INVALID
    assert _append(lib, p, 1, 64, p, p, N0=-1) == _lib.HQ_E_INVALID
    assert _append(lib, p, 1, 4097, p, p) == _lib.HQ_E_UNSUPPORTED              # as hq_seg_prepare_pack0
    assert _append(lib, p, 1, 8192, None, None) == _lib.HQ_E_UNSUPPORTED
    # a split copy comes as a pair, and the flagged-row list needs the level-0 statistics
    assert lib.hq_seg_append(p, 1, 64, 0, None, 0, p, p, p, None, None, None, None, None) == _lib.HQ_E_INVALID
    assert lib.hq_seg_append(p, 1, 64, 0, None, 0, p, p, None, None, p, None, None, None) == _lib.HQ_E_INVALID
    assert lib.hq_seg_append(p, 1, 64, 0, None, 0, p, p, None, None, None, None, p, None) == _lib.HQ_E_INVALID


def _model(name, count=16, data=b"\xff\xd8jpeg"):
    from hq_mi355x.models import ModelMetadata, QuantizedModel
    md = ModelMetadata(model_name=name, original_size_bytes=4 * count, compressed_size_bytes=len(data),
                       compression_ratio=1.0, quantization_timestamp="2024-01-01 00:00:00")
    return QuantizedModel(compressed_data=data, original_dimensions=(4, 4), parameter_count=count,
                          compression_quality=0.8, hierarchical_indices=np.arange(8, dtype=np.float64), metadata=md)


def test_registry_add_remove_like_reference():
    from hq_mi355x.api import HilbertQuantizer
    hq = HilbertQuantizer()
    a, b, c =_model("a"), _model("b"), _model("c")
    for m in (a, b, c):
        assert hq.add_model_to_registry(m) is None
    assert hq.get_registry_info() == {"total_models": 3, "model_ids": ["a", "b", "c"]}
    assert hq._model_registry[1] is b                                   # appended in order, the objects themselves
    assert hq.remove_model_from_registry("b") is True
    assert hq.get_registry_info()["model_ids"] == ["a", "c"]
    assert hq.remove_model_from_registry("b") is False                  # not found
    hq.add_model_to_registry(_model("a"))                               # names may repeat: the first one goes
    assert hq.remove_model_from_registry("a") is True
    assert [m.metadata.model_name for m in hq._model_registry] == ["c", "a"] and hq._model_registry[0] is c


def test_registry_add_validates_like_reference():
    from hq_mi355x.api import HilbertQuantizer
    from hq_mi355x.exceptions import ValidationError
    hq = HilbertQuantizer()
    with pytest.raises(ValidationError, match="Invalid quantized model type"):
        hq.add_model_to_registry({"not": "a model"})
    with pytest.raises(ValidationError, match="Quantized model has no compressed data"):
        hq.add_model_to_registry(_model("empty", data=b""))
    m = _model("none")
    m.compressed_data = None
    with pytest.raises(ValidationError, match="Quantized model has no compressed data"):
        hq.add_model_to_registry(m)
    m = _model("count")
    m.parameter_count = 0                                               # the dataclass itself refuses it at creation
    with pytest.raises(ValidationError, match="Invalid parameter count in quantized model"):
        hq.add_model_to_registry(m)
    assert hq.get_registry_info()["total_models"] == 0
