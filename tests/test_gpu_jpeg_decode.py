"""The device JPEG decoder (csrc/hq_jpeg_decode.hip) against PIL, byte for byte: the kernels, decode_jpeg_batch on
a mixed batch, refusals inside a wave group, and reconstruct_many(codec="device") against codec="host"."""
import dataclasses
import io

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
Image = pytest.importorskip("PIL.Image")


def make_frame(i, H, W, rng):
    """Family i % 4: random bytes, constant 0 / 128 / 255, checkerboard, clipped gaussian."""
    if i % 4 == 0:
        return rng.integers(0, 256, (H, W), dtype=np.uint8)
    if i % 4 == 1:
        return np.full((H, W), (0, 128, 255)[(i // 4) % 3], np.uint8)
    if i % 4 == 2:
        y, x = np.ogrid[:H, :W]
        return (((y + x + i) & 1) * 255).astype(np.uint8)
    return np.clip(rng.normal(128, 60, (H, W)), 0, 255).astype(np.uint8)


def pil_encode(frame, q, **kw):
    buf = io.BytesIO()
    Image.fromarray(frame, "L").save(buf, format="JPEG", quality=q, **kw)
    return buf.getvalue()


def pil_decode(data):
    return np.array(Image.open(io.BytesIO(data)))


def upload(payloads):
    from hq_mi355x._dev import to_dev
    offs = np.zeros(len(payloads) + 1, np.int64)
    offs[1:] = np.cumsum([len(p) for p in payloads])
    return to_dev(np.frombuffer(bytearray(b"".join(payloads) or b"\0"), np.uint8)), to_dev(offs)


CASES = [(H, W, N) for H, W in [(8, 8), (9, 8), (5, 4), (33, 32), (65, 64), (131, 128)]
         for N in ((3,) if H == 131 else (1, 70))]


@pytest.mark.parametrize("source", ["pil_optimize", "pil_standard", "device"])
@pytest.mark.parametrize("q", [1, 76, 95])
@pytest.mark.parametrize("H,W,N", CASES)
def test_decode_equals_pil(hq_lib, H, W, N, q, source):
    from hq_mi355x import kernels as K
    from hq_mi355x._dev import to_dev, to_np
    rng = np.random.default_rng([H, W, N, q])
    frames = np.stack([make_frame(i, H, W, rng) for i in range(N)])
    if source == "device":
        payload, offsets = K.jpeg_encode(to_dev(frames), q)
        data, offs = to_np(payload), to_np(offsets)
        payloads = [data[offs[i]:offs[i + 1]].tobytes() for i in range(N)]
    else:
        payloads = [pil_encode(f, q, optimize=source == "pil_optimize") for f in frames]
        payload, offsets = upload(payloads)
    desc = K.jpeg_probe(payload, offsets)
    got, status, coefs = K.jpeg_decode(payload, offsets, desc, None, H, W, want_coefs=True)
    assert not to_np(status).any() and not to_np(desc)[:, 0].any()
    np.testing.assert_array_equal(to_np(got), np.stack([pil_decode(p) for p in payloads]))
    if source == "device":
        np.testing.assert_array_equal(to_np(coefs), to_np(K.jpeg_coefficients(to_dev(frames), q)))


def test_mixed_batch_in_caller_order(hq_lib):
    from hq_mi355x._dev import to_np
    from hq_mi355x.core.compressor import decode_jpeg_batch
    rng = np.random.default_rng(5)
    shapes = [(33, 32), (65, 64), (9, 8)]
    payloads = [pil_encode(make_frame(i, *shapes[i % 3], rng), (30, 76)[(i // 3) % 2], optimize=bool((i // 6) % 2))
                for i in range(60)]
    groups, refused = decode_jpeg_batch(payloads)
    assert refused == [] and sorted(tuple(f.shape[1:]) for f, _ in groups) == sorted(shapes)
    got = {int(i): fr for f, ids in groups for fr, i in zip(to_np(f), ids)}
    assert sorted(got) == list(range(60))
    for i, p in enumerate(payloads):
        np.testing.assert_array_equal(got[i], pil_decode(p))


def test_refusals_do_not_disturb_neighbours(hq_lib):
    """Planted inside the first 16-frame wave group of a 33 x 32 batch: each gets a status and zero rows, every
    other payload PIL's pixels."""
    from hq_mi355x import kernels as K
    from hq_mi355x._dev import to_np
    rng = np.random.default_rng(11)
    valid = [pil_encode(make_frame(i, 33, 32, rng), 76, optimize=bool(i % 2)) for i in range(20)]
    rgb = io.BytesIO()
    Image.fromarray(rng.integers(0, 256, (33, 32, 3), dtype=np.uint8), "RGB").save(rgb, format="JPEG")
    fr = make_frame(0, 33, 32, rng)
    planted = {1: valid[1][:int(0.6 * len(valid[1]))], 3: valid[3][:-2], 4: pil_encode(fr, 76, progressive=True),
               6: rgb.getvalue(), 7: pil_encode(fr, 76, restart_marker_blocks=2), 9: b"",
               10: np.random.default_rng(0).integers(0, 256, 200, dtype=np.uint8).tobytes(),
               12: pil_encode(make_frame(0, 65, 64, rng), 76)}
    payloads = [planted.get(i, p) for i, p in enumerate(valid)]
    payload, offsets = upload(payloads)
    got, status = K.jpeg_decode(payload, offsets, K.jpeg_probe(payload, offsets), None, 33, 32)
    got, status = to_np(got), to_np(status)
    for i, p in enumerate(payloads):
        if i in planted:
            assert status[i] != 0 and not got[i].any(), (i, status[i])
        else:
            assert status[i] == 0, (i, status[i])
            np.testing.assert_array_equal(got[i], pil_decode(p))


@pytest.mark.parametrize("d,eff", [(1024, None), (1536, 0.2)])
def test_reconstruct_many_device_codec(hq_lib, d, eff):
    from hq_mi355x.api import HilbertQuantizer
    from hq_mi355x.exceptions import HilbertQuantizationError
    rng = np.random.default_rng(d)
    sets = [rng.standard_normal(d).astype(np.float32) for _ in range(70)]
    for codec in ("host", "device"):
        hq = HilbertQuantizer(min_efficiency_ratio=eff)
        models = hq.quantize_many(sets, codec=codec)
        want, got = hq.reconstruct_many(models), hq.reconstruct_many(models, codec="device")
        assert len(got) == 70
        for a, b in zip(got, want):
            assert a.dtype == b.dtype and a.shape == b.shape == (d,) and a.tobytes() == b.tobytes()
        cut = models[5].compressed_data
        models[5] = dataclasses.replace(models[5], compressed_data=cut[:len(cut) // 2])
        errors = []
        for route in ("host", "device"):
            with pytest.raises(HilbertQuantizationError) as e:
                hq.reconstruct_many(models, codec=route)
            errors.append((type(e.value), str(e.value)))
        assert errors[0] == errors[1]
