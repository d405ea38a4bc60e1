"""CPU-side checks of the fused decode (hq_dequantize_unmap) and the round-trip metrics (hq_roundtrip_error):
the library exports and binds them, their argument validation returns before any device work, and the inputs
of test_gpu_decode.py discriminate (shown with the oracle alone).  No kernel is launched here."""
import numpy as np

from oracle import hq_oracle as O

import decode_cases as D
import quant_edges as Q


def _lib():
    from hq_mi355x import _lib
    return _lib, _lib.load()


def test_exports_and_signatures():
    _l, lib = _lib()
    for name, nargs in (("hq_dequantize_unmap", 11), ("hq_roundtrip_error", 8)):
        assert hasattr(lib, name), name
        assert name in _l.SIGNATURES and len(_l.SIGNATURES[name][1]) == nargs
    from hq_mi355x import kernels as K
    from hq_mi355x.api import BatchQuantizer
    from hq_mi355x.core import pipeline as P
    assert callable(K.dequantize_unmap) and callable(K.roundtrip_error)
    assert callable(P.reconstruct_frames_batch) and callable(P.QuantizationPipeline.validate_quantization)
    assert callable(BatchQuantizer.reconstruct_device) and callable(BatchQuantizer.extract_indices_device)


def test_dequantize_unmap_validation():
    """Same codes and message style as hq_map_index_quantize, decided on the host: every call passes null
    pointers."""
    _l, lib = _lib()

    def call(N, n, d, stride, shared=0):
        return lib.hq_dequantize_unmap(None, N, n, d, None, shared, None, stride, None, None, None)

    assert call(1, 6, 4, 4) == _l.HQ_E_NOT_POW2
    assert _l.last_error() == "Dimension must be a power of 2, got 6"
    assert call(1, 256, 4, 4) == _l.HQ_E_UNSUPPORTED
    assert _l.last_error() == "fused decode supports 2 <= n <= 128, got 256"
    assert call(1, 1, 1, 1) == _l.HQ_E_UNSUPPORTED
    assert call(1, 16, 257, 257) == _l.HQ_E_TOO_MANY
    assert _l.last_error() == "Too many parameters (257) for dimensions 16x16 (256 cells)"
    assert call(1, 16, 200, 199) == _l.HQ_E_INVALID          # out_stride < d
    assert call(-1, 16, 200, 200) == _l.HQ_E_INVALID         # N < 0
    assert call(1, 16, -1, 200) == _l.HQ_E_INVALID           # d < 0
    assert call(0, 16, 200, 200) == _l.HQ_OK                 # nothing to do
    assert call(0, 16, 200, 200, shared=1) == _l.HQ_OK
    assert call(1, 16, 200, 200) == _l.HQ_E_INVALID          # work with null buffers
    assert _l.last_error() == "null buffer"
    assert call(1, 64, 1536, 1536, shared=1) == _l.HQ_E_INVALID
    assert call(1, 128, 0, 0) == _l.HQ_OK                    # d = 0 and no index output: nothing to do


def test_roundtrip_error_validation():
    _l, lib = _lib()

    def call(N, d, so, sr):
        return lib.hq_roundtrip_error(None, so, None, sr, N, d, None, None)

    assert call(0, 8, 8, 8) == _l.HQ_OK
    assert call(-1, 8, 8, 8) == _l.HQ_E_INVALID
    assert call(1, 0, 0, 0) == _l.HQ_E_INVALID               # np.max of an empty row has no value
    assert call(1, 8, 7, 8) == _l.HQ_E_INVALID and call(1, 8, 8, 7) == _l.HQ_E_INVALID
    assert call(1, 8, 8, 8) == _l.HQ_E_INVALID               # null buffers
    assert call(1, (1 << 26) + 1, 1 << 27, 1 << 27) == _l.HQ_E_UNSUPPORTED


def test_decode_options_exist():
    _l, _ = _lib()
    for name in ("decode_nt", "decode_generic"):
        assert _l.get_option(name) is None
        with _l.option(name, 1):
            assert _l.get_option(name) == 1
        assert _l.get_option(name) is None


def test_every_byte_frames_discriminate():
    """The every-byte frame holds all 256 values in its image and varied bytes in its index row, and decoding
    it with fl(1 / 255) instead of the division gives different bits in at least one family."""
    f = D.every_byte_frame(16)
    assert f.shape == (17, 16) and len(np.unique(f[:-1])) == 256 and len(np.unique(f[-1])) == 16
    differs = []
    for name, (mn, mx) in Q.RANGES_F32.items():
        ref = O.denormalize_u8(f, mn, mx)
        assert ref.dtype == np.float32
        if D.recip_denormalize(f, mn, mx).tobytes() != ref.tobytes():
            differs.append(name)
    assert differs, "no family tells the reciprocal form from the division"
    # and a flat pair decodes to mn whatever the byte
    for mn, _ in Q.RANGES_F32.values():
        assert np.all(O.denormalize_u8(f, mn, mn) == mn)


def test_index_cases_reach_every_length():
    for n in (16, 64):
        cases = D.index_cases(n)
        lens = {}
        for name, f, mn, mx in cases:
            rows, ln = D.oracle_index(f, mn, mx)
            lens[name] = int(ln[0])
            assert rows.shape == (1, n) and 1 <= lens[name] <= n
        assert lens["trimmed"] == n // 2 - 1 and lens["neg_zero"] == n // 2 - 1
        assert lens["untrimmed"] == n and lens["last_column"] == n and lens["flat_nonzero"] == n
        assert lens["all_zero"] == lens["flat_zero"] == lens["flat_neg_zero"] == lens["first_column"] == 1
        assert {1, n // 2 - 1, n} <= set(lens.values())


def test_oracle_decode_is_the_reference_sequence():
    """decode_cases.oracle_decode == the reference's component sequence on one frame (truncation included)."""
    rng = np.random.default_rng(3)
    f = rng.integers(0, 256, (9, 8), dtype=np.uint8)
    enh = O.denormalize_u8(f, -0.5, 2.0)
    img, _ = O.extract_index_row(enh)
    want = O.map_from_2d(img)[:13]
    got = D.oracle_decode(f, -0.5, 2.0, 13)
    assert got.shape == (1, 13) and got[0].tobytes() == want.tobytes()
