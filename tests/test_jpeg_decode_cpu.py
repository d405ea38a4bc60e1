"""The device JPEG decoder without a GPU: the two exports and their argument checks (which return before any device
work), the reconstruct API's codec switch, and the decoder's per-frame logic (csrc/hq_jpeg_decode.h) run on the
CPU by tools/jpeg_decode_host.cpp against PIL."""
import io
import os
import shutil
import struct
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_exports_and_argument_rules():
    from hq_mi355x import _lib
    lib = _lib.load()
    assert len(_lib.SIGNATURES["hq_jpeg_probe"][1]) == 5 and len(_lib.SIGNATURES["hq_jpeg_decode"][1]) == 11
    one = 1  # any non-NULL address: the checks below return before it is used
    assert lib.hq_jpeg_probe(None, None, 0, None, None) == _lib.HQ_OK
    assert lib.hq_jpeg_probe(None, None, -1, None, None) == _lib.HQ_E_INVALID
    assert lib.hq_jpeg_probe(None, one, 3, one, None) == _lib.HQ_E_INVALID and _lib.last_error() == "null buffer"
    dec = lambda M, H, W, p=None: lib.hq_jpeg_decode(p, p, p, None, M, H, W, p, p, None, None)
    assert dec(0, 65, 64) == _lib.HQ_OK
    assert dec(3, 65, 64) == _lib.HQ_E_INVALID and _lib.last_error() == "null buffer"
    assert dec(-1, 65, 64) == _lib.HQ_E_INVALID and dec(3, 0, 64) == _lib.HQ_E_INVALID
    assert dec(3, 65, 0) == _lib.HQ_E_INVALID and dec(0, 0, 64) == _lib.HQ_E_INVALID
    assert dec(3, 168, 224) == _lib.HQ_E_INVALID                                # the widest frame: on to the NULL check
    for M in (0, 3):
        assert dec(M, 65, 225, one) == _lib.HQ_E_UNSUPPORTED and "at most 65500 x 224" in _lib.last_error()


def test_unknown_codec_is_refused():
    from hq_mi355x.api import BatchQuantizer, HilbertQuantizer
    from hq_mi355x.core.pipeline import reconstruct_batch
    with pytest.raises(ValueError, match="codec must be 'host' or 'device', got 'bogus'"):
        HilbertQuantizer().reconstruct_many([], codec="bogus")
    with pytest.raises(ValueError, match="codec must be 'host' or 'device', got 'gpu'"):
        BatchQuantizer().reconstruct_batch([], codec="gpu")
    with pytest.raises(ValueError, match="codec must be"):
        reconstruct_batch([], None, codec="bogus")


def test_host_program_equals_pil(tmp_path):
    Image = pytest.importorskip("PIL.Image")
    cxx = shutil.which("c++") or shutil.which("g++") or shutil.which("clang++")
    if cxx is None:
        pytest.skip("no host C++ compiler")
    exe = str(tmp_path / "jpeg_decode_host")
    subprocess.run([cxx, "-std=c++17", "-O1", os.path.join(ROOT, "tools", "jpeg_decode_host.cpp"), "-o", exe], check=True)
    rng = np.random.default_rng(3)

    def encode(frame, q, optimize):
        buf = io.BytesIO()
        Image.fromarray(frame, "L").save(buf, format="JPEG", quality=q, optimize=optimize)
        return buf.getvalue()

    whole = [encode(rng.integers(0, 256, s, dtype=np.uint8) if k % 2 else np.full(s, 23 * k, np.uint8), q, bool(k % 3))
             for k, (s, q) in enumerate([(s, q) for s in [(8, 8), (9, 8), (5, 4), (33, 32)] for q in (1, 76, 95)])]
    small = encode(rng.integers(0, 256, (9, 8), dtype=np.uint8), 76, True)
    payloads = whole + [small[:k] for k in range(len(small) + 1)]
    offs = np.zeros(len(payloads) + 1, np.int64)
    offs[1:] = np.cumsum([len(p) for p in payloads])
    (tmp_path / "p.bin").write_bytes(b"".join(payloads))
    offs.tofile(tmp_path / "o.bin")
    subprocess.run([exe, str(tmp_path / "p.bin"), str(tmp_path / "o.bin"), str(tmp_path / "out.bin")], check=True)
    out, pos, accepted = (tmp_path / "out.bin").read_bytes(), 0, 0
    for k, p in enumerate(payloads):
        status, H, W = struct.unpack_from("<iii", out, pos)
        pos += 12
        assert status == 0 or k >= len(whole), (k, status)       # a prefix may be refused, a whole payload not
        if status == 0:
            got = np.frombuffer(out, np.uint8, H * W, pos).reshape(H, W)
            pos += H * W
            np.testing.assert_array_equal(got, np.array(Image.open(io.BytesIO(p))))
            accepted += 1
    assert pos == len(out) and accepted >= len(whole) + 1        # the last prefix is the whole payload
