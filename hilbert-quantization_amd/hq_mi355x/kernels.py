"""Tensor-level entry points: one function per C-ABI call of libhq_mi355x (include/hq_mi355x.h).

Inputs and outputs are device tensors (torch on ROCm, used only as HBM buffers); every function
launches HIP kernels on the current stream and never computes on the host.  These are the batched
entry points the reference lacks (`map_to_2d_batch`, `quantize_batch`, `search_batch` in
SURVEY.md §7); the reference-shaped classes in `hq_mi355x.core` / `hq_mi355x.rag` wrap them.
"""
from __future__ import annotations

import functools
import threading

import ctypes
from typing import Optional, Tuple

import numpy as np

from . import _lib
from ._dev import device, dtype_code, ptr, stream, torch


def _L():
    return _lib.lib()


def _chk(rc, exc=None):
    _lib.check(rc, exc)


def _contig(x):
    return x if x.is_contiguous() else x.contiguous()


# ---------------------------------------------------------------------------------------------- M


def hilbert_table(n: int, exc=None):
    """(xs, ys, xy2d) int32 device tensors for an n x n grid (core/hilbert_mapper.py:17-113)."""
    t = torch()
    if n <= 0 or (n & (n - 1)) != 0:
        _chk(_L().hq_hilbert_table(n, None, None, None, None), exc)
    xs = t.empty(n * n, dtype=t.int32, device=device())
    ys = t.empty_like(xs)
    tab = t.empty_like(xs)
    _chk(_L().hq_hilbert_table(n, ptr(xs), ptr(ys), ptr(tab), stream()), exc)
    return xs, ys, tab.view(n, n)


def map_to_2d(x, n: int, exc=None):
    """[N, d] (or [d]) -> [N, n, n]: out[y][x] = in[d2xy^-1(x, y)] (core/hilbert_mapper.py:115-174)."""
    t = torch()
    squeeze = x.dim() == 1
    x2 = x.view(1, -1) if squeeze else x
    if x2.stride(-1) != 1:
        x2 = x2.contiguous()
    N, d = x2.shape
    out = t.empty((N, n, n), dtype=x.dtype, device=x.device)
    _chk(_L().hq_map_to_2d(dtype_code(x.dtype), ptr(x2), N, x2.stride(0) if N > 1 else d, d, n, ptr(out),
                           stream()), exc)
    return out[0] if squeeze else out


def map_from_2d(img, d_out: Optional[int] = None, exc=None):
    """[N, n, n] (or [n, n]) -> [N, d_out] in curve order (core/hilbert_mapper.py:176-205)."""
    t = torch()
    squeeze = img.dim() == 2
    im = _contig(img.unsqueeze(0) if squeeze else img)
    N, n, _ = im.shape
    if d_out is None:
        d_out = n * n
    out = t.empty((N, d_out), dtype=img.dtype, device=img.device)
    _chk(_L().hq_map_from_2d(dtype_code(img.dtype), ptr(im), N, n, d_out, ptr(out), stream()), exc)
    return out[0] if squeeze else out


# ---------------------------------------------------------------------------------------------- I


def index_streaming(img, L: int, stream_len: Optional[int] = None, exc=None):
    """Streaming index of [N, n, n] f32/f64 images -> f64 [N, L] (core/streaming_index_builder.py:315-343).
    The tree covers the first `stream_len` curve positions (default n*n)."""
    t = torch()
    squeeze = img.dim() == 2
    im = _contig(img.unsqueeze(0) if squeeze else img)
    N, n, _ = im.shape
    if stream_len is None:
        stream_len = n * n
    out = t.zeros((N, L), dtype=t.float64, device=im.device)
    _chk(_L().hq_index_streaming(dtype_code(im.dtype), ptr(im), N, n, int(stream_len), L, ptr(out), stream()), exc)
    return out[0] if squeeze else out


def index_traditional(img, L: int, exc=None):
    """Traditional index of [N, n, n] f32/f64 images -> f32 [N, L] (core/index_generator.py:313-356).
    Float64 images are averaged and sampled in float64 and rounded to float32 once per slot, as the
    reference does; any other dtype is widened to float64 first.  Slots the level allocation does not
    fill stay 0.0: at L = 1 the allocation is empty, so the row is [0.0] (the reference returns an empty
    array there; core.HierarchicalIndexGeneratorImpl.generate_optimized_indices reproduces that)."""
    t = torch()
    squeeze = img.dim() == 2
    im = img.unsqueeze(0) if squeeze else img
    if im.dtype not in (t.float32, t.float64):
        im = im.to(t.float64)
    im = _contig(im)
    N, n, _ = im.shape
    out = t.zeros((N, L), dtype=t.float32, device=im.device)
    _chk(_L().hq_index_traditional(dtype_code(im.dtype), ptr(im), N, n, L, ptr(out), stream()), exc)
    return out[0] if squeeze else out


def block_means(img, grid: int, order: int = 0, exc=None):
    """np.mean of each block: order 0 row-major sections, 1 RAG Hilbert order -> f32 [N, cnt]."""
    t = torch()
    squeeze = img.dim() == 2
    im = _contig(img.unsqueeze(0) if squeeze else img)
    if im.dtype not in (t.float32, t.float64):
        im = im.to(t.float32)
    N, n, _ = im.shape
    cnt = 1 if n // grid == 0 else grid * grid
    out = t.empty((N, cnt), dtype=im.dtype, device=im.device)
    _chk(_L().hq_block_means(dtype_code(im.dtype), ptr(im), N, n, int(grid), int(order), ptr(out), stream()), exc)
    return out[0] if squeeze else out


def rag_index_rows(n: int) -> int:
    return _lib.load().hq_rag_index_rows(n)


def index_rag(img, exc=None):
    """RAG multi-row index: [N, n, n] f32 -> [N, n + R, n] (hierarchical_index_generator.py:103-146)."""
    t = torch()
    squeeze = img.dim() == 2
    im = _contig(img.unsqueeze(0) if squeeze else img)
    if im.dtype != t.float32:
        raise TypeError("index_rag: float32 images only")
    N, n, _ = im.shape
    R = rag_index_rows(n)
    out = t.empty((N, n + R, n), dtype=t.float32, device=im.device)
    _chk(_L().hq_index_rag_f32(ptr(im), N, n, ptr(out), stream()), exc)
    return out[0] if squeeze else out


# ---------------------------------------------------------------------------------------------- Q


def quantize_u8(enh, exc=None):
    """[N, r, c] f32 -> (u8 [N, r, c], minmax f32 [N, 2]) (core/compressor.py:256-280)."""
    t = torch()
    squeeze = enh.dim() == 2
    e = _contig(enh.unsqueeze(0) if squeeze else enh)
    N, r, c = e.shape
    out = t.empty((N, r, c), dtype=t.uint8, device=e.device)
    mm = t.empty((N, 2), dtype=t.float32, device=e.device)
    _chk(_L().hq_quantize_u8(ptr(e), N, r, c, ptr(out), ptr(mm), stream()), exc)
    return (out[0], mm[0]) if squeeze else (out, mm)


def dequantize_u8(u8, minmax, exc=None):
    """u8 [N, r, c] with minmax [N, 2] -> f32 (core/compressor.py:282-303)."""
    t = torch()
    squeeze = u8.dim() == 2
    u = _contig(u8.unsqueeze(0) if squeeze else u8)
    mm = _contig(minmax.view(-1, 2).to(t.float32))
    N, r, c = u.shape
    out = t.empty((N, r, c), dtype=t.float32, device=u.device)
    _chk(_L().hq_dequantize_u8(ptr(u), N, r, c, ptr(mm), ptr(out), stream()), exc)
    return out[0] if squeeze else out


def map_index_quantize(x, n: int, L: Optional[int] = None, want_idx: bool = True, want_minmax: bool = True,
                       out: Optional[Tuple] = None, exc=None):
    """The fused north-star kernel: f32 [N, d] -> (u8 frames [N, n+1, n], f64 idx [N, L], f32 minmax [N, 2]).
    Equivalent to pad -> map_to_2d -> streaming index(L) -> embed -> normalise of core/pipeline.py:97-146."""
    t = torch()
    if L is None:
        L = n
    x2 = x if x.dim() == 2 else x.view(1, -1)
    if x2.dtype != t.float32:
        raise TypeError("map_index_quantize expects float32 parameters")
    if x2.stride(-1) != 1:
        x2 = x2.contiguous()
    N, d = x2.shape
    if out is not None:
        frames, idx, mm = out
    else:
        frames = t.empty((N, n + 1, n), dtype=t.uint8, device=x2.device)
        idx = t.empty((N, L), dtype=t.float64, device=x2.device) if want_idx else None
        mm = t.empty((N, 2), dtype=t.float32, device=x2.device) if want_minmax else None
    _chk(_L().hq_map_index_quantize(ptr(x2), N, x2.stride(0) if N > 1 else d, d, n, L, ptr(frames), ptr(idx),
                                    ptr(mm), stream()), exc)
    return frames, idx, mm


def dequantize_unmap(frames, minmax, d: Optional[int] = None, want_index: bool = False, out=None, exc=None):
    """The fused decode: u8 frames [N, n+1, n] (or [n+1, n]) -> f32 parameters [N, d] in curve order, i.e.
    map_from_2d(dequantize_u8(frames)[:, :-1])[:, :d] in ONE kernel (core/pipeline.py:183-235 after the codec).

    minmax: f32 device tensor [N, 2], or ONE pair of shape [2] / [1, 2] applied to every frame (shared mode:
    the compressor-state semantics of core/compressor.py:282-303).  d defaults to n * n.  out: an f32 device
    tensor [N, >= d] with unit column stride to write into (its columns from d on are left as they are).
    want_index: also return the de-normalised index rows f32 [N, n] and the lengths int32 [N] that
    extract_indices_from_image keeps (core/index_generator.py:255-290)."""
    t = torch()
    squeeze = frames.dim() == 2
    fr = _contig(frames.unsqueeze(0) if squeeze else frames)
    if fr.dtype != t.uint8:
        raise TypeError("dequantize_unmap expects uint8 frames")
    N, r, n = fr.shape
    if r != n + 1:
        raise ValueError(f"dequantize_unmap expects (n + 1) x n frames, got {r} x {n}")
    if d is None:
        d = n * n
    d = int(d)
    mm = minmax if minmax.dtype == t.float32 else minmax.to(t.float32)
    shared = mm.dim() == 1 or (mm.shape[0] == 1 and N != 1)
    mm = _contig(mm.reshape(-1, 2))
    if not shared and mm.shape[0] != N:
        raise ValueError(f"minmax must be [2], [1, 2] or [{N}, 2], got {tuple(minmax.shape)}")
    if out is None:
        out = t.empty((N, d), dtype=t.float32, device=fr.device)
    elif (out.dtype != t.float32 or out.dim() != 2 or out.shape[0] != N or out.shape[1] < d
          or (out.shape[1] > 1 and out.stride(1) != 1)):
        raise ValueError(f"out must be a float32 [{N}, >= {d}] tensor with unit column stride")
    stride = out.stride(0) if N > 1 else max(int(out.shape[1]), d)
    idx_row = t.empty((N, n), dtype=t.float32, device=fr.device) if want_index else None
    idx_len = t.empty((N,), dtype=t.int32, device=fr.device) if want_index else None
    _chk(_L().hq_dequantize_unmap(ptr(fr), N, n, d, ptr(mm), 1 if shared else 0, ptr(out), stride, ptr(idx_row),
                                  ptr(idx_len), stream()), exc)
    params = out if out.shape[1] == d else out[:, :d]
    if squeeze:
        return (params[0], idx_row[0], idx_len[0]) if want_index else params[0]
    return (params, idx_row, idx_len) if want_index else params


def roundtrip_error(orig, recon, exc=None):
    """f32 [N, d] (or [d]) original and reconstructed rows -> f32 [N, 3] (or [3]) = (mse, mae, max_error) per
    row: np.mean((o - r) ** 2), np.mean(np.abs(o - r)), np.max(np.abs(o - r)) bit for bit
    (core/pipeline.py:257-259 validate_quantization)."""
    t = torch()
    squeeze = orig.dim() == 1
    o = orig.view(1, -1) if squeeze else orig
    r = recon.view(1, -1) if recon.dim() == 1 else recon
    if o.dtype != t.float32 or r.dtype != t.float32:
        raise TypeError("roundtrip_error expects float32 rows")
    if tuple(o.shape) != tuple(r.shape):
        raise ValueError(f"shapes differ: {tuple(o.shape)} and {tuple(r.shape)}")
    if o.stride(-1) != 1:
        o = o.contiguous()
    if r.stride(-1) != 1:
        r = r.contiguous()
    N, d = o.shape
    out = t.empty((N, 3), dtype=t.float32, device=o.device)
    _chk(_L().hq_roundtrip_error(ptr(o), o.stride(0) if N > 1 else d, ptr(r), r.stride(0) if N > 1 else d, N, d,
                                 ptr(out), stream()), exc)
    return out[0] if squeeze else out


def chunk_encode_f16(x, chunk: int = 1024, exc=None, out=None):
    """Config 5: flat f16 stream -> per-chunk (u8 frame, f32 traditional index, minmax)
    (core/streaming_processor.py:539-582, 877-913).  The last (shorter) chunk uses its own
    geometry inside its slot; unused slot bytes are zero (when `out` is given, the caller's
    buffers are written in place and unused tail-slot bytes are left as they are)."""
    t = torch()
    x1 = _contig(x.reshape(-1))
    if x1.dtype != t.float16:
        raise TypeError("chunk_encode_f16 expects float16")
    total = x1.numel()
    from .core.dimension_calculator import _optimal_side
    ns = _optimal_side(chunk)
    nch = (total + chunk - 1) // chunk
    if out is not None:
        frames, idx, mm = out
        if (tuple(frames.shape) != (nch, ns + 1, ns) or tuple(idx.shape) != (nch, ns) or tuple(mm.shape) != (nch, 2)
                or frames.dtype != t.uint8 or idx.dtype != t.float32 or mm.dtype != t.float32
                or not (frames.is_contiguous() and idx.is_contiguous() and mm.is_contiguous())):
            raise ValueError(f"out buffers must be contiguous u8 [{nch}, {ns + 1}, {ns}], f32 [{nch}, {ns}], "
                             f"f32 [{nch}, 2]")
    else:
        frames = t.zeros((nch, ns + 1, ns), dtype=t.uint8, device=x1.device)
        idx = t.zeros((nch, ns), dtype=t.float32, device=x1.device)
        mm = t.zeros((nch, 2), dtype=t.float32, device=x1.device)
    _chk(_L().hq_chunk_encode_f16(ptr(x1), total, chunk, ptr(frames), ptr(idx), ptr(mm), stream()), exc)
    return frames, idx, mm


# ---------------------------------------------------------------------------------------------- S


def parse_structure(L: int):
    """[(grid, start, end, is_offset)] (core/search_engine.py:42-109), computed by the library."""
    buf = (ctypes.c_int32 * 64)()
    n = _lib.load().hq_parse_structure(int(L), buf, 16)
    return [(buf[4 * i], buf[4 * i + 1], buf[4 * i + 2], bool(buf[4 * i + 3])) for i in range(min(n, 16))]


@functools.lru_cache(maxsize=None)
def seg_count(L: int) -> int:
    return _lib.load().hq_seg_count(int(L))


@functools.lru_cache(maxsize=None)
def seg_level0_len(L: int) -> int:
    return int(_lib.load().hq_seg_level0_len(int(L)))


@functools.lru_cache(maxsize=None)
def seg_padded_len(L: int) -> int:
    return _lib.load().hq_seg_padded_len(int(L))


class Prepared:
    """Device-resident prepared index vectors: raw R [N, L] f64, Z [N, Lp] f64 (segment padded,
    normalised) and stats S [N, nseg, 4] (mean, std, mean of squares, aux).  Built once per corpus.
    f32: some rows are float32 index vectors (aux bit 1; hq_seg_prepare_src / _rows).

    cap: the rows the buffers behind R / Z / S hold (seg_reserve / seg_append); R, Z, S are then the
    length-N prefix views of `base` = (R, Z, S) capacity buffers, and Z16 / S32 / Zov16 / Sov32 / F0 are
    sized for cap rows (their valid extents are those of N rows).  cap == N, base None: built to size."""

    __slots__ = ("R", "Z", "S", "L", "N", "nseg", "Lp", "Z16", "S32", "F0", "Zov16", "Sov32", "f32", "all32", "cap",
                 "base")

    def __init__(self, R, Z, S, L, f32: bool = False, all32: bool = False):
        self.R, self.Z, self.S, self.L = R, Z, S, int(L)
        self.N = Z.shape[0]
        self.nseg = S.shape[1]
        self.Lp = Z.shape[1]
        self.f32 = bool(f32)      # some rows are float32 sources
        self.all32 = bool(all32)  # every row is
        self.Z16 = self.S32 = None  # split-f16 level-0 copies for the level-0 scan (pack0)
        self.F0 = None  # a corpus's flagged rows of the level-0 copies, listed once (flag_rows)
        self.Zov16 = self.Sov32 = None  # split-f16 copies of every level for the overall scan (packov)
        self.cap, self.base = self.N, None

    def rows(self, sel):
        """Sub-set of rows (device index tensor) as a new Prepared (level-0 copies re-packed on demand)."""
        p = Prepared(self.R.index_select(0, sel), self.Z.index_select(0, sel), self.S.index_select(0, sel), self.L,
                     self.f32, self.all32)
        p = pack0(p) if self.Z16 is not None else p
        return packov(p) if self.Zov16 is not None else p

    def unsafe_rows(self):
        """Device bool [N]: float32 rows outside the scans' model (aux bit 2, hq_mi355x.h) -> dense exact path."""
        return (self.S[:, :, 3] >= 2.0).any(dim=1)


def _row_flags(src_f32: bool, row_f32, n: int, dev, all_needs_rows: bool = True):
    """(rf, any32, all32) of a batch of n rows: the device uint8 flag per row for the library (None when
    src_f32 covers every row or no flags were given), and whether any / every row is a float32 index vector.
    all_needs_rows: per-row flags of an empty batch do not make it all-float32 (seg_append passes False: its
    empty batch changes nothing)."""
    any32 = all32 = bool(src_f32)
    if row_f32 is None or src_f32:
        return None, any32, all32
    flags = np.asarray(row_f32, dtype=bool).reshape(-1)
    if flags.size != n:
        raise ValueError("row_f32 needs one flag per row")
    any32, all32 = bool(flags.any()), bool(flags.all()) and (n > 0 or not all_needs_rows)
    return _contig(torch().from_numpy(flags.astype(np.uint8)).to(dev)), any32, all32


def seg_prepare(idx, exc=None, src_f32: bool = False, row_f32=None) -> Prepared:
    """src_f32: every row is a float32 index vector; row_f32 (bool per row, host or device): some are
    (hq_seg_prepare_rows).  The reference computes those rows' statistics and scores in float32."""
    t = torch()
    i2 = _contig((idx if idx.dim() == 2 else idx.view(1, -1)).to(t.float64))
    N, L = i2.shape
    Lp, ns = seg_padded_len(L), seg_count(L)
    Z = t.empty((N, Lp), dtype=t.float64, device=i2.device)
    S = t.empty((N, ns, 4), dtype=t.float64, device=i2.device)
    rf, any32, all32 = _row_flags(src_f32, row_f32, N, i2.device)
    if N:
        _chk(_L().hq_seg_prepare_rows(ptr(i2), N, L, 1 if src_f32 else 0, ptr(rf), ptr(Z), ptr(S), stream()), exc)
    return Prepared(i2, Z, S, L, any32, all32)


PAD0 = 48  # pad rows of the level-0 copies (hq_mi355x.h: hq_seg_pack0_split)


def _rows16(n: int) -> int:
    return (n + 15) // 16 * 16 + PAD0


def _rows4(n: int) -> int:
    return (n + 3) // 4 * 4 + PAD0


@functools.lru_cache(maxsize=None)
def packov_info(L: int):
    """(K-blocks, G segments, one-value segments, floats per 4-row statistics group) of the split
    overall layout (hq_seg_packov_info), or None when the level structure of L has none."""
    v = [ctypes.c_int() for _ in range(4)]
    if _lib.load().hq_seg_packov_info(int(L), *[ctypes.byref(x) for x in v]) != 0:
        return None
    return tuple(x.value for x in v)


def _alloc_split(p: Prepared, cap: int, level0: bool = False, overall: bool = False, flags: bool = False) -> Prepared:
    """Give p uninitialised split layouts sized for cap rows: the level-0 copies (Z16, S32), the overall copies
    (Zov16, Sov32; L must have a split overall layout) and the flagged-row list (F0), each where asked."""
    t = torch()
    dev = p.Z.device
    if level0:
        p.Z16 = t.empty((_rows16(cap), 64), dtype=t.float16, device=dev)  # tiled rows
        p.S32 = t.empty((_rows4(cap), 4), dtype=t.float32, device=dev)  # SoA groups of 4 rows
    if overall:
        nkb, _, _, gs = packov_info(p.L)
        p.Zov16 = t.empty((_rows16(cap), nkb * 64), dtype=t.float16, device=dev)  # tiled: 16-row tiles of nkb x 2 KiB
        p.Sov32 = t.empty((_rows4(cap) // 4, gs), dtype=t.float32, device=dev)  # SoA groups of 4 rows
    if flags:
        p.F0 = t.empty(1 + cap, dtype=t.int32, device=dev)  # the count, then the listed rows
    return p


def packov(p: Prepared, exc=None) -> Prepared:
    """Attach the split-f16 copies of every level segment (hq_seg_packov_split) used by the overall
    (brute-force) scan; level structures without a split layout keep the f64 scan."""
    if packov_info(p.L) is None:
        return p
    _alloc_split(p, p.N, overall=True)
    _chk(_L().hq_seg_packov_split(ptr(p.Z), ptr(p.S), p.N, p.L, ptr(p.Zov16), ptr(p.Sov32), stream()), exc)
    return p


def pack0(p: Prepared, exc=None) -> Prepared:
    """Attach the split-f16 level-0 copies (hq_seg_pack0_split) used by the level-0 scan; indexes whose
    level-0 segment is longer than 32 values keep the f64 scan."""
    if seg_level0_len(p.L) > 32:
        return p
    _alloc_split(p, p.N, level0=True)
    _chk(_L().hq_seg_pack0_split(ptr(p.Z), ptr(p.S), p.N, p.L, ptr(p.Z16), ptr(p.S32), stream()), exc)
    return p


def seg_prepare_pack0(idx, exc=None, src_f32: bool = False, row_f32=None) -> Prepared:
    """seg_prepare + pack0 in one launch (hq_seg_prepare_pack0): a query batch's statistics, normalised
    rows and split level-0 copies (level-0 segments of <= 32 values; else seg_prepare alone)."""
    t = torch()
    i2 = _contig((idx if idx.dim() == 2 else idx.view(1, -1)).to(t.float64))
    N, L = i2.shape
    if seg_level0_len(L) > 32 or L > 4096:
        return pack0(seg_prepare(i2, exc, src_f32, row_f32), exc)
    Lp, ns = seg_padded_len(L), seg_count(L)
    Z = t.empty((N, Lp), dtype=t.float64, device=i2.device)
    S = t.empty((N, ns, 4), dtype=t.float64, device=i2.device)
    rf, any32, all32 = _row_flags(src_f32, row_f32, N, i2.device)
    p = _alloc_split(Prepared(i2, Z, S, L, any32, all32), N, level0=True)
    _chk(_L().hq_seg_prepare_pack0(ptr(i2), N, L, 1 if src_f32 else 0, ptr(rf), ptr(Z), ptr(S), ptr(p.Z16),
                                   ptr(p.S32), stream()), exc)
    return p


def flag_rows(p: Prepared, exc=None) -> Prepared:
    """List a corpus's flagged level-0 rows once (hq_seg_flag_rows: int32 [1 + N], count first), so the
    level-0 scan of every query batch skips that pass over the statistics."""
    if p.S32 is None:
        return p
    _alloc_split(p, p.N, flags=True)
    _chk(_L().hq_seg_flag_rows(ptr(p.S32), p.N, ptr(p.F0), stream()), exc)
    return p


def _carry(q: Prepared, p: Prepared) -> Prepared:
    """q, a new view of p's rows, takes over p's capacity buffers and split layouts."""
    q.cap, q.base = p.cap, p.base
    q.Z16, q.S32, q.Zov16, q.Sov32, q.F0 = p.Z16, p.S32, p.Zov16, p.Sov32, p.F0
    return q


def seg_reserve(p: Prepared, capacity: int) -> Prepared:
    """A Prepared of the same N rows whose buffers hold `capacity` rows (p itself when they already do):
    new buffers, device-to-device copies of the valid extents of every layout p carries.  The rows past N
    are written by seg_append."""
    cap = int(capacity)
    if cap <= p.cap and p.base is not None:
        return p
    cap = max(cap, p.cap)
    t = torch()
    dev, N = p.Z.device, p.N
    Rb = t.empty((cap, p.L), dtype=t.float64, device=dev)
    Zb = t.empty((cap, p.Lp), dtype=t.float64, device=dev)
    Sb = t.empty((cap, p.nseg, 4), dtype=t.float64, device=dev)
    Rb[:N].copy_(p.R)
    Zb[:N].copy_(p.Z)
    Sb[:N].copy_(p.S)
    q = Prepared(Rb[:N], Zb[:N], Sb[:N], p.L, p.f32, p.all32)
    q.cap, q.base = cap, (Rb, Zb, Sb)
    _alloc_split(q, cap, p.Z16 is not None, p.Zov16 is not None, p.F0 is not None)
    if p.Z16 is not None:
        q.Z16[:_rows16(N)].copy_(p.Z16[:_rows16(N)])
        q.S32[:_rows4(N)].copy_(p.S32[:_rows4(N)])
    if p.Zov16 is not None:
        q.Zov16[:_rows16(N)].copy_(p.Zov16[:_rows16(N)])
        q.Sov32[:_rows4(N) // 4].copy_(p.Sov32[:_rows4(N) // 4])
    if p.F0 is not None:
        q.F0[:1 + N].copy_(p.F0[:1 + N])  # the count and (at most N) listed rows
    return q


def seg_append(p: Prepared, rows, src_f32: bool = False, row_f32=None, exc=None) -> Prepared:
    """p grown by `rows` [M, L] (src_f32 / row_f32 as seg_prepare): one hq_seg_append launch writes the new
    rows' R / Z / S and every split layout p carries (pack0, packov, flag_rows) behind the resident rows, which
    do not move.  Beyond the capacity the buffers grow geometrically (x 2, at least the need: seg_reserve).
    Returns a new Prepared over the same buffers; p must not be scanned afterwards (what it took for pad rows
    are real rows now), and scans of p still running on other streams must have finished before the call."""
    t = torch()
    r2 = _contig((rows if rows.dim() == 2 else rows.view(1, -1)).to(t.float64))
    M, L = r2.shape
    if L != p.L:
        raise ValueError(f"appended index length {L} != corpus index length {p.L}")
    rf, any32, all32 = _row_flags(src_f32, row_f32, M, r2.device, all_needs_rows=False)
    if M == 0:
        return p
    N0, N1 = p.N, p.N + M
    if N1 > p.cap or p.base is None:
        p = seg_reserve(p, max(N1, 2 * p.cap))
    Rb, Zb, Sb = p.base
    Rb[N0:N1].copy_(r2)
    _chk(_L().hq_seg_append(ptr(r2), M, L, 1 if src_f32 else 0, ptr(rf), N0, ptr(Zb), ptr(Sb), ptr(p.Z16), ptr(p.S32),
                            ptr(p.Zov16), ptr(p.Sov32), ptr(p.F0), stream()), exc)
    return _carry(Prepared(Rb[:N1], Zb[:N1], Sb[:N1], L, p.f32 or any32, all32 and (p.all32 or N0 == 0)), p)


def _row_ids(rows, n: int, dev, what: str, checked: bool = False):
    """Row numbers (sequence, NumPy array or tensor) as a contiguous device int64 [M]; every value must lie in
    [0, n): IndexError otherwise, before anything is launched (a device tensor costs one host sync; checked:
    the caller has done it)."""
    t = torch()
    if isinstance(rows, t.Tensor):
        sel = _contig(rows.reshape(-1).to(device=dev, dtype=t.int64))
        if not checked and sel.numel():
            lo, hi = (int(v) for v in sel.aminmax())
            if lo < 0 or hi >= n:
                raise IndexError(f"{what}: row {lo if lo < 0 else hi} outside [0, {n})")
        return sel
    a = np.asarray(rows).reshape(-1)
    if a.size and a.dtype.kind not in "iu":
        raise TypeError(f"{what}: row numbers must be integers")
    a = a.astype(np.int64)
    if not checked and a.size and (a.min() < 0 or a.max() >= n):
        raise IndexError(f"{what}: row {int(a.min()) if a.min() < 0 else int(a.max())} outside [0, {n})")
    return t.from_numpy(np.ascontiguousarray(a)).to(dev)


def _f32_state(p: Prepared, S):
    """(f32, all32) of the rows whose statistics are S, taken from a corpus p: what a fresh build of those rows
    reports.  An all-float32 or all-float64 corpus needs no look; a mixed one reads aux bit 1 of S[:, 0, 3]
    (one host sync)."""
    if not p.f32:
        return False, False
    if p.all32:
        return True, True
    if S.shape[0] == 0:
        return False, False
    t = torch()
    bits = (S[:, 0, 3].to(t.int64) & 1).to(t.float64)
    n32 = int(bits.sum())
    return n32 > 0, n32 == S.shape[0]


def seg_gather(p: Prepared, src_rows, cap: Optional[int] = None, exc=None, checked: bool = False) -> Prepared:
    """A new Prepared of the rows p[src_rows] (row numbers in [0, p.N), any order, repeats allowed), in a second
    set of buffers with room for max(cap or p.cap, M) rows: one hq_seg_gather launch copies each row's R / Z / S
    and writes every split layout p carries (pack0, packov, flag_rows), byte-identical to a fresh build of the
    selected rows.  p is only read.  IndexError for a row out of range, before the launch."""
    t = torch()
    dev = p.Z.device
    sel = _row_ids(src_rows, p.N, dev, "seg_gather", checked)
    M = int(sel.numel())
    cap = max(int(cap) if cap else p.cap, M)
    Rb = t.empty((cap, p.L), dtype=t.float64, device=dev)
    Zb = t.empty((cap, p.Lp), dtype=t.float64, device=dev)
    Sb = t.empty((cap, p.nseg, 4), dtype=t.float64, device=dev)
    q = Prepared(Rb[:M], Zb[:M], Sb[:M], p.L)
    q.cap, q.base = cap, (Rb, Zb, Sb)
    _alloc_split(q, cap, p.Z16 is not None, p.Zov16 is not None, p.F0 is not None)
    _chk(_L().hq_seg_gather(ptr(sel), M, p.N, p.L, ptr(p.R), ptr(p.Z), ptr(p.S), ptr(Rb), ptr(Zb), ptr(Sb), ptr(q.Z16),
                            ptr(q.S32), ptr(q.Zov16), ptr(q.Sov32), ptr(q.F0), stream()), exc)
    q.f32, q.all32 = _f32_state(p, q.S)
    return q


def seg_replace(p: Prepared, rows, new_rows, src_f32: bool = False, row_f32=None, exc=None,
                checked: bool = False) -> Prepared:
    """p with the resident rows `rows` (distinct row numbers in [0, p.N)) overwritten in place by `new_rows`
    [M, L] (src_f32 / row_f32 as seg_prepare): R by index_copy_, then one hq_seg_replace call rewrites those
    rows' Z / S and split layouts and lists the flagged rows again; byte-identical to a fresh build of the
    updated rows.  A writer, as seg_append: no scan of p may be running.  Returns a new Prepared over the same
    buffers (a p built to size is first moved into buffers of its own, once: its R may be the caller's tensor).
    IndexError for a row out of range, ValueError for a repeated row, before any launch."""
    t = torch()
    r2 = _contig((new_rows if new_rows.dim() == 2 else new_rows.view(1, -1)).to(t.float64))
    M, L = r2.shape
    if L != p.L:
        raise ValueError(f"replacement index length {L} != corpus index length {p.L}")
    sel = _row_ids(rows, p.N, r2.device, "seg_replace", checked)
    if int(sel.numel()) != M:
        raise ValueError(f"{int(sel.numel())} row numbers for {M} replacement rows")
    if not checked and M > 1 and int(t.unique(sel).numel()) != M:
        raise ValueError("seg_replace: repeated row numbers")
    rf, any32, all32 = _row_flags(src_f32, row_f32, M, r2.device, all_needs_rows=False)
    if M == 0:
        return p
    if p.base is None:  # built to size: R may be the caller's own tensor (seg_prepare keeps it), so move first
        p = seg_reserve(p, p.cap)
    p.R.index_copy_(0, sel, r2)
    _chk(_L().hq_seg_replace(ptr(r2), M, ptr(sel), L, 1 if src_f32 else 0, ptr(rf), p.N, ptr(p.Z), ptr(p.S), ptr(p.Z16),
                             ptr(p.S32), ptr(p.Zov16), ptr(p.Sov32), ptr(p.F0), stream()), exc)
    q = _carry(Prepared(p.R, p.Z, p.S, L, p.f32 or any32, all32 and p.all32), p)
    if q.f32 and not q.all32:  # mixed: float32 rows may all have left, or every float64 row may have
        q.f32, q.all32 = _f32_state(q, q.S)
    return q


def level_scores(q: Prepared, c: Prepared, level: int, exc=None):
    """Dense EXACT [Q, N] level (>= 0) or overall (level = -1) scores (reference operation order)."""
    t = torch()
    out = t.empty((q.N, c.N), dtype=t.float64, device=q.Z.device)
    _chk(_L().hq_level_scores(ptr(q.R), ptr(q.Z), ptr(q.S), q.N, ptr(c.R), ptr(c.Z), ptr(c.S), c.N, c.L, level,
                              ptr(out), stream()), exc)
    return out


_TLS = threading.local()


def _workspace(nbytes: int, dev):
    """Scan / re-rank workspace reused across the calls ONE thread makes on one stream (stream order
    makes that reuse safe: the previous call's kernels finish before the next call's first write).
    Saves an allocation between the query preparation and the first scan launch of every batch.

    Per thread, not per stream alone: the reference calls its engines from ThreadPoolExecutor workers
    (core/video_search.py:806,854), and threads sharing a stream interleave their launches (ctypes drops
    the GIL), so thread B's scan could otherwise overwrite thread A's workspace between A's scan and A's
    re-rank.  A thread's buffers return to the caching allocator when the thread ends (stream-ordered)."""
    t = torch()
    cache = getattr(_TLS, "ws", None)
    if cache is None:
        cache = _TLS.ws = {}
    key = (str(dev), stream())
    ws = cache.get(key)
    if ws is None or ws.numel() < nbytes:
        ws = cache[key] = t.empty(nbytes, dtype=t.uint8, device=dev)
    return ws[:nbytes]


@functools.lru_cache(maxsize=None)
def scan_max_list(L: int, mode: int) -> int:
    """Longest list (0 .. 64) hq_scan_topk takes at index length L (mode 0: level 0, 1: overall): its workgroup
    keeps the candidate tile, both sides' statistics, the score tile and 64 queries' lists in 160 KiB of LDS
    (scan_lds_bytes in hq_search.hip, repeated here; a longer list is refused with HQ_E_UNSUPPORTED)."""
    cols = seg_level0_len(L) if mode == 0 else seg_padded_len(L)
    nsu = 1 if mode == 0 else seg_count(L)
    rs = max(cols, 2)
    while rs % 32 != 2:
        rs += 1
    fixed = 8 * (64 * rs + 2 * 64 * nsu * 4 + 4 * 16 * 64) + 2 * 8 * 64 + 4 * 64 + 64
    return max(0, min(64, (160 * 1024 - fixed) // (16 * 64)))


def scan_topk(q: Prepared, c: Prepared, mode: int, k: int, threshold: float = 0.0, thr_mode: int = 0,
              id_base: int = 0, need_best: bool = False, exc=None):
    """Fused MFMA scan + per-query top-k on APPROXIMATE scores.  mode 0: level-0 score, 1: overall.
    thr_mode 0 none / 1 >= / 2 >.  Returns (scores [Q, k], ids [Q, k], best [Q], best_id [Q]); best and
    best_id (first arg-max of the approximate score) are None unless need_best (the level-0 scan without
    the arg-max runs the split-f16 queue scan: k_sample_topg, k_scan0g, k_pool_select)."""
    t = torch()
    Q, N = q.N, c.N
    dev = q.Z.device
    ws_bytes = int(_lib.load().hq_scan_workspace_size(Q, N, k))
    ws = _workspace(ws_bytes, dev)
    sc = t.empty((Q, k), dtype=t.float64, device=dev)
    ids = t.empty((Q, k), dtype=t.int64, device=dev)
    best = t.empty(Q, dtype=t.float64, device=dev) if need_best else None
    bid = t.empty(Q, dtype=t.int64, device=dev) if need_best else None
    # option scan_v1 (parity tests): the LDS-tiled k_scan instead of the split-f16 level-0 scan
    if (mode == 0 and not need_best and q.Z16 is not None and c.Z16 is not None
            and (q.f32 or c.f32 or _lib.get_option("scan_v1") is None)):
        _chk(_L().hq_scan0_topk_split_fl(ptr(q.Z16), ptr(q.S32), ptr(q.S), Q, ptr(c.Z16), ptr(c.S32), ptr(c.S), N,
                                         c.L, k, float(threshold), thr_mode, int(id_base), ptr(ws), ws_bytes,
                                         ptr(sc), ptr(ids), None if c.F0 is None else ptr(c.F0), stream()), exc)
        return sc, ids, best, bid
    # option scan_v1 (parity tests): the f64 overall scan instead of the split overall scan
    if mode == 1 and not need_best and q.Zov16 is None and c.Zov16 is not None and _lib.get_option("scan_v1") is None:
        packov(q, exc)  # query batches get the overall layout only when an overall scan needs it
    if (mode == 1 and not need_best and q.Zov16 is not None and c.Zov16 is not None
            and _lib.get_option("scan_v1") is None):
        ws_bytes = int(_lib.load().hq_scanov_workspace_size(Q, N, k))
        ws = _workspace(ws_bytes, dev)
        _chk(_L().hq_scanov_topk_split(ptr(q.Zov16), ptr(q.Sov32), ptr(q.S), ptr(q.Z), Q, ptr(c.Zov16), ptr(c.Sov32),
                                       ptr(c.S), ptr(c.Z), N, c.L, k, float(threshold), thr_mode, int(id_base), ptr(ws),
                                       ws_bytes, ptr(sc), ptr(ids), stream()), exc)
        return sc, ids, best, bid
    _chk(_L().hq_scan_topk(ptr(q.Z), ptr(q.S), Q, ptr(c.Z), ptr(c.S), N, c.L, mode, k, float(threshold), thr_mode,
                           int(id_base), ptr(ws), ws_bytes, ptr(sc), ptr(ids), ptr(best), ptr(bid), stream()), exc)
    return sc, ids, best, bid


def _refine_outputs(cand_id, k: int, lists: bool = True):
    """The re-rank outputs of the lists cand_id [Q, kp]: (scores [Q, k], ids [Q, k], count [Q], resolved [Q]);
    lists False: no scores and ids (None)."""
    t = torch()
    Q, dev = cand_id.shape[0], cand_id.device
    os_ = t.empty((Q, k), dtype=t.float64, device=dev) if lists else None
    oi = t.empty((Q, k), dtype=t.int64, device=dev) if lists else None
    return os_, oi, t.empty(Q, dtype=t.int32, device=dev), t.empty(Q, dtype=t.int32, device=dev)


def _refine_args(q, c, mode, cand_score, cand_id, k, threshold, thr_mode, eps, id_base, outs):
    """The leading arguments the hq_refine_* entries share: both vector sets, (mode; None: hq_refine_final_ws,
    which takes none,) the lists, their sizes and threshold, the four outputs."""
    Q, kp = cand_id.shape
    return (ptr(q.R), ptr(q.Z), ptr(q.S), Q, ptr(c.R), ptr(c.Z), ptr(c.S), c.N, c.L, *(() if mode is None else (mode,)),
            ptr(_contig(cand_score)), ptr(_contig(cand_id)), kp, k, float(threshold), thr_mode, float(eps), int(id_base),
            *(ptr(o) for o in outs))


def refine_topk(q: Prepared, c: Prepared, mode: int, cand_score, cand_id, k: int, threshold: float = 0.0,
                thr_mode: int = 0, eps: float = 1e-9, id_base: int = 0, exc=None, redo=None, count_empty: bool = False):
    """Exact re-rank of a scan list -> (scores [Q, k], ids [Q, k], count [Q], resolved [Q]).  redo (device
    int32 [1], optional): set to the number of queries needing the dense path (unresolved, or with
    count_empty, nothing passed)."""
    kp = cand_id.shape[1]
    outs = _refine_outputs(cand_id, k)
    if kp > 64:  # long lists: the lane-cooperative re-rank with its workspace
        _refine_ws(q, c, mode, cand_score, cand_id, kp, k, threshold, thr_mode, eps, id_base, *outs, count_empty, redo,
                   None, None, exc)
        return outs
    _chk(_L().hq_refine_topk(*_refine_args(q, c, mode, cand_score, cand_id, k, threshold, thr_mode, eps, id_base, outs),
                             1 if count_empty else 0, ptr(redo), stream()), exc)
    return outs


def _refine_ws(q, c, mode, cand_score, cand_id, kp, k, threshold, thr_mode, eps, id_base, os_, oi, cnt, res,
               count_empty, redo, next_redo, det, exc):
    """hq_refine_topk_ws (lists > 64: k_rank_pairs + k_rank_sort) on the stream's reusable workspace (the
    scan that produced the list has finished with it in stream order)."""
    wb = int(_lib.load().hq_refine_workspace_size(int(cand_id.shape[0]), kp, c.L))
    ws = _workspace(wb, cand_id.device)
    _chk(_L().hq_refine_topk_ws(*_refine_args(q, c, mode, cand_score, cand_id, k, threshold, thr_mode, eps, id_base,
                                              (os_, oi, cnt, res)),
                                1 if count_empty else 0, ptr(redo), ptr(next_redo), ptr(det), ptr(ws), wb, stream()),
         exc)


# refine_final_ws: write the level-0 lists (not returned).  False (the library then skips them, and in round 6 also
# their sort, by selection rounds) measured slower at M = 100 / 1000 (profiles/r06_ab_final_select.txt); the
# selection path was removed, the NULL form kept
FINAL_LEVEL0_LISTS = True


def refine_final_ws(q: Prepared, c: Prepared, cand_score, cand_id, k: int, threshold: float, thr_mode: int,
                    eps: float, id_base: int, K_out: int, redo=None, next_redo=None, exc=None):
    """The level-0 re-rank of a progressive search with its final ranking fused in (hq_refine_final_ws):
    (count, resolved, out_id [Q, K_out], out_det [Q, K_out, 1 + nseg], out_count) as refine_rescore_topk +
    progressive_final with one list and no arg-max fallback; None where the fused form does not exist (the
    caller runs the two steps)."""
    t = torch()
    Q, kp = cand_id.shape
    dev = cand_id.device
    # support probe: with Q = 0 and no counter the call only checks the form exists (nothing launched)
    rc = _L().hq_refine_final_ws(None, None, None, 0, None, None, None, c.N, c.L, None, None, kp, k, 0.0, 0, 0.0, 0,
                                 None, None, None, None, None, None, int(K_out), None, None, None, None, 0, stream())
    if rc == _lib.HQ_E_UNSUPPORTED:
        return None
    _chk(rc, exc)
    # the level-0 lists are not returned (FINAL_LEVEL0_LISTS False: not written)
    outs = _refine_outputs(cand_id, k, FINAL_LEVEL0_LISTS)
    fid = t.empty((Q, K_out), dtype=t.int64, device=dev)
    fdet = t.empty((Q, K_out, 1 + q.nseg), dtype=t.float64, device=dev)
    fcnt = t.empty(Q, dtype=t.int32, device=dev)
    ws, wb = None, 0
    if kp > 64:  # lists <= 64 take k_rank_small, which needs no workspace
        wb = int(_lib.load().hq_refine_workspace_size(Q, kp, c.L))
        ws = _workspace(wb, dev)
    rc = _L().hq_refine_final_ws(*_refine_args(q, c, None, cand_score, cand_id, k, threshold, thr_mode, eps, id_base,
                                               outs),
                                 ptr(redo), ptr(next_redo), int(K_out), ptr(fid), ptr(fdet), ptr(fcnt), ptr(ws), wb,
                                 stream())
    if rc == _lib.HQ_E_UNSUPPORTED:
        return None
    _chk(rc, exc)
    return outs[2], outs[3], fid, fdet, fcnt


def refine_rescore_topk(q: Prepared, c: Prepared, mode: int, cand_score, cand_id, k: int, threshold: float = 0.0,
                        thr_mode: int = 0, eps: float = 1e-9, id_base: int = 0, exc=None, redo=None,
                        count_empty: bool = False, next_redo=None):
    """refine_topk + the exact [overall, level_0..] re-score of its output (rescore's values for the output
    ids, zeros in empty slots) -> (scores, ids, count, resolved, det [Q, k, 1 + nseg])."""
    t = torch()
    Q, kp = cand_id.shape
    outs = _refine_outputs(cand_id, k)
    det = t.empty((Q, k, 1 + q.nseg), dtype=t.float64, device=cand_id.device)
    ce = 1 if count_empty else 0
    if kp > 64:  # long lists: the lane-cooperative re-rank with its workspace
        _refine_ws(q, c, mode, cand_score, cand_id, kp, k, threshold, thr_mode, eps, id_base, *outs, count_empty, redo,
                   next_redo, det, exc)
        return (*outs, det)
    head = _refine_args(q, c, mode, cand_score, cand_id, k, threshold, thr_mode, eps, id_base, outs)
    if next_redo is not None:  # ping-pong counters: redo arrives zeroed, the kernel clears next_redo
        _chk(_L().hq_refine_rescore_topk_pp(*head, ce, ptr(redo), ptr(next_redo), ptr(det), stream()), exc)
    else:
        _chk(_L().hq_refine_rescore_topk(*head, ce, ptr(redo), ptr(det), stream()), exc)
    return (*outs, det)


def rescore(q: Prepared, c: Prepared, ids, id_base: int = 0, exc=None):
    """EXACT [overall, level_0..] for (query, global id) pairs in ids [Q, k] -> f64 [Q, k, 1 + nseg]."""
    t = torch()
    ids = _contig(ids.to(t.int64))
    Q, k = ids.shape
    out = t.empty((Q, k, 1 + q.nseg), dtype=t.float64, device=ids.device)
    _chk(_L().hq_rescore(ptr(q.R), ptr(q.Z), ptr(q.S), Q, ptr(c.R), ptr(c.Z), ptr(c.S), c.N, c.L, ptr(ids), k,
                         int(id_base), ptr(out), stream()), exc)
    return out


THR_KEY32 = 8  # thr_mode bit of the re-rank: float32 sort keys (hq_mi355x.h HQ_THR_KEY32)


def progressive_final(s0, ids, det, best, best_id, best_det, K: int, exc=None, key32: bool = False):
    """R-way final stage of progressive search.  s0/ids [R, Q, M], det [R, Q, M, W], best/best_id
    [R, Q], best_det [R, Q, W].  Returns (out_id [Q, K], out_det [Q, K, W], count [Q]).  key32: every
    vector is float32, so scores rank by their float32-rounded values (hq_progressive_final_ex flag 1)."""
    t = torch()
    R, Q, M = ids.shape
    W = det.shape[-1]
    dev = ids.device
    oid = t.empty((Q, K), dtype=t.int64, device=dev)
    odet = t.empty((Q, K, W), dtype=t.float64, device=dev)
    cnt = t.empty(Q, dtype=t.int32, device=dev)
    _chk(_L().hq_progressive_final_ex(R, Q, M, W - 1, ptr(_contig(s0)), ptr(_contig(ids)), ptr(_contig(det)),
                                      ptr(_contig(best)), ptr(_contig(best_id)), ptr(_contig(best_det)), K, ptr(oid),
                                      ptr(odet), ptr(cnt), 1 if key32 else 0, stream()), exc)
    return oid, odet, cnt


def cosine_scores_f64(a, b, exc=None):
    """(cos + 1) / 2 of rows of a [Q, K] against rows of b [N, K] (rag/search/engine.py:622-660)."""
    t = torch()
    a2 = _contig(a.reshape(a.shape[0], -1).to(t.float32))
    b2 = _contig(b.reshape(b.shape[0], -1).to(t.float32))
    K = min(a2.shape[1], b2.shape[1])
    if a2.shape[1] != K:
        a2 = _contig(a2[:, :K])
    if b2.shape[1] != K:
        b2 = _contig(b2[:, :K])
    out = t.empty((a2.shape[0], b2.shape[0]), dtype=t.float64, device=a2.device)
    _chk(_L().hq_cosine_scores(ptr(a2), a2.shape[0], ptr(b2), b2.shape[0], K, ptr(out), stream()), exc)
    return out


def cosine_scores_dt(a, b, exc=None):
    """(cos + 1) / 2 of float32 or float64 rows (hq_cosine_scores_dt; float64 stays float64) -> f64 [Q, N].
    float32 problems large enough for the matrix cores take cosine_scores' split-f16 MFMA path."""
    t = torch()
    a2 = _contig(a.reshape(a.shape[0], -1))
    b2 = _contig(b.reshape(b.shape[0], -1))
    if a2.dtype == t.float32 and b2.dtype == t.float32:
        return cosine_scores(a2, b2, exc)
    a2, b2 = a2.to(t.float64), b2.to(t.float64)
    Kd = min(a2.shape[1], b2.shape[1])
    if a2.shape[1] != Kd:
        a2 = _contig(a2[:, :Kd])
    if b2.shape[1] != Kd:
        b2 = _contig(b2[:, :Kd])
    out = t.empty((a2.shape[0], b2.shape[0]), dtype=t.float64, device=a2.device)
    _chk(_L().hq_cosine_scores_dt(dtype_code(t.float64), ptr(a2), a2.shape[0], ptr(b2), b2.shape[0], Kd, ptr(out),
                                  stream()), exc)
    return out


def select_topk(scores, k: int, threshold: float = 0.0, thr_mode: int = 0, id_base: int = 0, exc=None):
    """Top-k (score desc, id asc) of a dense f64 [Q, N] score matrix + first arg-max."""
    t = torch()
    sc = _contig(scores.to(t.float64))
    Q, N = sc.shape
    dev = sc.device
    os_ = t.empty((Q, k), dtype=t.float64, device=dev)
    oi = t.empty((Q, k), dtype=t.int64, device=dev)
    b = t.empty(Q, dtype=t.float64, device=dev)
    bi = t.empty(Q, dtype=t.int64, device=dev)
    ws_bytes = int(_L().hq_select_workspace_size(Q, N, k))
    ws = t.empty(max(ws_bytes, 1), dtype=t.uint8, device=dev)
    _chk(_L().hq_select_topk_ws(ptr(sc), Q, N, k, float(threshold), thr_mode, int(id_base), ptr(ws), ws_bytes,
                                ptr(os_), ptr(oi), ptr(b), ptr(bi), stream()), exc)
    return os_, oi, b, bi


def pair_scores_raw(q, C, exc=None, q_f32: bool = False, c_f32: bool = False):
    """compare_indices_at_level on raw equal-length segments: q [m] vs C [N, m] -> f64 [N]; q_f32 / c_f32:
    that side holds float32 values (statistics in float32; the whole score when both are)."""
    t = torch()
    q1 = _contig(q.reshape(-1).to(t.float64))
    C2 = _contig(C.to(t.float64))
    N, m = C2.shape
    out = t.empty(N, dtype=t.float64, device=C2.device)
    _chk(_L().hq_pair_scores_raw_src(ptr(q1), ptr(C2), N, m, 1 if q_f32 else 0, 1 if c_f32 else 0, ptr(out),
                                     stream()), exc)
    return out


# ------------------------------------------------------------------- §8f row 3: pre-computed index


def precomputed_layout(n: int, max_levels: int = 6, min_square_size: int = 2, exc=None):
    """[(grid, square, count, first_output)] of core/precomputed_hilbert_index.py:121-212 (library)."""
    buf = (ctypes.c_int32 * 64)()
    k = _L().hq_precomputed_layout(int(n), int(max_levels), int(min_square_size), buf, 16)
    if k < 0:
        _chk(k, exc)
    return [(buf[4 * i], buf[4 * i + 1], buf[4 * i + 2], buf[4 * i + 3]) for i in range(min(k, 16))]


def precomputed_index(x, n: int, kind: int = 0, d: Optional[int] = None, max_levels: int = 6,
                      min_square_size: int = 2, exc=None):
    """Overlapping-square averages f32 [N, T] (core/precomputed_hilbert_index.py:65-212).
    kind 0: x = images [N, n, n] (f32/f64); kind 1: x = 1-D Hilbert-ordered parameters [N, d] (f32/f64),
    zero-padded to n*n and mapped to 2-D first (core/pipeline.py:298-319)."""
    t = torch()
    if kind == 0:
        x2 = _contig(x.view(-1, n * n) if x.dim() != 2 or x.shape[1] != n * n else x)
        dd = n * n
    else:
        x2 = x.view(1, -1) if x.dim() == 1 else x
        if x2.stride(-1) != 1:
            x2 = x2.contiguous()
        dd = int(x2.shape[1]) if d is None else int(d)
    N = int(x2.shape[0])
    lay = precomputed_layout(n, max_levels, min_square_size, exc)
    T = sum(c for (_, _, c, _) in lay)
    out = t.empty((N, T), dtype=t.float32, device=x2.device)
    stride = x2.stride(0) if N > 1 else x2.shape[1]
    _chk(_L().hq_precomputed_index(dtype_code(x2.dtype), int(kind), ptr(x2), N, stride, dd, int(n), int(max_levels),
                                   int(min_square_size), ptr(out), T, stream()), exc)
    return out


def precomputed_stats(avgs, offsets, counts, exc=None):
    """Per row and level: stats f32 [N, nlev, 3] (np.mean, np.std, np.mean(a**2)) and the normalised
    averages [N, T] ((a - mean) / std where std != 0) for the first counts[l] values of each level."""
    t = torch()
    a = _contig(avgs)
    N, T = a.shape
    nlev = len(offsets)
    off = (ctypes.c_int32 * nlev)(*offsets)
    cnt = (ctypes.c_int32 * nlev)(*counts)
    st = t.empty((N, nlev, 3), dtype=t.float32, device=a.device)
    nrm = t.zeros_like(a)
    _chk(_L().hq_precomputed_stats(ptr(a), N, T, nlev, off, cnt, ptr(st), ptr(nrm), stream()), exc)
    return st, nrm


def precomputed_similarity(qa, qn, qs, ca, cn, cs, q_offsets, c_offsets, counts, weights, levels: bool = False,
                           exc=None):
    """_calculate_precomputed_similarity for Q x N pairs -> (overall f64 [Q, N], type u8 [Q, N]
    (0 numpy float32, 1 Python float), level sims f64 [Q, N, nlev] or None)."""
    t = torch()
    Q, N = int(qa.shape[0]), int(ca.shape[0])
    nlev = len(counts)
    ov = t.empty((Q, N), dtype=t.float64, device=qa.device)
    ty = t.empty((Q, N), dtype=t.uint8, device=qa.device)
    lv = t.empty((Q, N, nlev), dtype=t.float64, device=qa.device) if levels else None
    _chk(_L().hq_precomputed_similarity(ptr(qa), ptr(qn), ptr(qs), Q, qa.shape[1], ptr(ca), ptr(cn), ptr(cs), N,
                                        ca.shape[1], nlev, (ctypes.c_int32 * nlev)(*q_offsets),
                                        (ctypes.c_int32 * nlev)(*c_offsets), (ctypes.c_int32 * nlev)(*counts),
                                        (ctypes.c_double * nlev)(*weights), ptr(ov), ptr(ty),
                                        ptr(lv) if lv is not None else None, stream()), exc)
    return ov, ty, lv


def pearson_f64(q, C, exc=None):
    """Legacy compare_indices_at_level of the pre-computed engine (:468-496) for q [m] vs C [N, m]."""
    t = torch()
    q1 = _contig(q.reshape(-1))
    C2 = _contig(C)
    N, m = C2.shape
    out = t.empty(N, dtype=t.float64, device=C2.device)
    _chk(_L().hq_pearson_f64(ptr(q1), ptr(C2), N, m, ptr(out), stream()), exc)
    return out


# --------------------------------------------------------------------- S7 on the matrix cores


class CosRows:
    """Split-f16 rows for the MFMA cosine (hq_cos_prepare): X16 [Np, 2, Kp] f16, inv [Np] f64."""

    __slots__ = ("X16", "inv", "N", "K")

    def __init__(self, X16, inv, N, K):
        self.X16, self.inv, self.N, self.K = X16, inv, int(N), int(K)


def cos_prepare(x, exc=None) -> CosRows:
    t = torch()
    x2 = x.view(1, -1) if x.dim() == 1 else x.reshape(x.shape[0], -1)
    if x2.dtype != t.float32:
        x2 = x2.to(t.float32)
    if x2.stride(-1) != 1:
        x2 = x2.contiguous()
    N, K = int(x2.shape[0]), int(x2.shape[1])
    Kp = int(_L().hq_cos_padded_k(K))
    Np = int(_L().hq_cos_padded_rows(N))
    X16 = t.empty((max(Np, 1), 2, max(Kp, 1)), dtype=t.float16, device=x2.device)
    inv = t.empty(max(Np, 1), dtype=t.float64, device=x2.device)
    if N:
        _chk(_L().hq_cos_prepare(ptr(x2), N, x2.stride(0) if N > 1 else K, K, ptr(X16), ptr(inv), stream()), exc)
    return CosRows(X16, inv, N, K)


def cosine_scores_mfma(q: CosRows, c: CosRows, exc=None, f32: bool = False):
    """(cos + 1) / 2 of every prepared query row against every prepared frame row -> f64 [Q, N]
    (f32=True: float32 [Q, N], the f64 value rounded once — the reference's own score dtype)."""
    t = torch()
    if q.K != c.K:
        raise ValueError(f"query length {q.K} != frame length {c.K}")
    out = t.empty((q.N, c.N), dtype=t.float32 if f32 else t.float64, device=q.X16.device)
    fn = _L().hq_cos_scores_mfma_f32 if f32 else _L().hq_cos_scores_mfma
    _chk(fn(ptr(q.X16), ptr(q.inv), q.N, ptr(c.X16), ptr(c.inv), c.N, q.K, ptr(out), stream()), exc)
    return out


def _query_block(q, q0: int, q1: int, operands):
    """Prepared queries [q0, q1) of CosRows / CosQRows / CosQFRows, q0 a multiple of 16: query tile t starts at
    row 16 t of the operand (1 KiB fragments, tile-major), so a block is a pointer offset into the prepared rows."""
    if q0 == 0 and q1 == q.N:
        return q
    x, v = operands(q)
    return type(q)(x[q0:], v[q0:], q1 - q0, q.K)


def _frame_topk(q, c, k, threshold, thr_mode, id_base, workspace_limit, exc, *, dense, size, fused, operands):
    """The body of cosine_topk, cosq_topk and cosqf_topk.  dense(q, c, exc): the route's [Q, N] scores; size /
    fused: its hq_*_topk_workspace_size / hq_*_topk; operands(rows): (operand fragments, per-row vector)."""
    t = torch()
    if q.K != c.K:
        raise ValueError(f"query length {q.K} != frame length {c.K}")
    k, Q, N = int(k), q.N, c.N
    if k < 1:
        raise ValueError(f"k = {k}")
    cx, cv = operands(c)
    dev = operands(q)[0].device
    os_ = t.full((Q, k), float("-inf"), dtype=t.float64, device=dev)
    oi = t.full((Q, k), -1, dtype=t.int64, device=dev)
    if Q == 0 or N == 0:
        return os_, oi
    limit = max(int(workspace_limit), 1)
    if k > 64 or k > N:
        per = max(128, limit // (8 * N) // 128 * 128)
        for q0 in range(0, Q, per):
            q1 = min(Q, q0 + per)
            s, i, _, _ = select_topk(dense(_query_block(q, q0, q1, operands), c, exc), k, threshold, thr_mode, id_base,
                                     exc)
            os_[q0:q1], oi[q0:q1] = s, i
        return os_, oi
    per = Q
    if int(size(Q, N, k)) > limit:
        per = max(128, limit // max(int(size(128, N, k)), 1) * 128)
        while per > 128 and int(size(per, N, k)) > limit:
            per -= 128
    for q0 in range(0, Q, per):
        q1 = min(Q, q0 + per)
        b = _query_block(q, q0, q1, operands)
        bx, bv = operands(b)
        wb = int(size(b.N, N, k))
        ws = _workspace(wb, dev)
        _chk(fused(ptr(bx), ptr(bv), b.N, ptr(cx), ptr(cv), N, q.K, k, float(threshold), int(thr_mode), int(id_base),
                   ptr(ws), wb, ptr(os_[q0:q1]), ptr(oi[q0:q1]), stream()), exc)
    return os_, oi


def cosine_topk(q: CosRows, c: CosRows, k: int, threshold: float = 0.0, thr_mode: int = 0, id_base: int = 0,
                workspace_limit: int = 256 << 20, exc=None):
    """The k nearest prepared frames of every prepared query -> (scores [Q, k] f64, ids [Q, k] i64), equal to
    select_topk(cosine_scores_mfma(q, c), k, threshold, thr_mode, id_base) in ids, order and score bits,
    without the [Q, N] matrix (hq_cos_topk: the selection runs in the GEMM's epilogue).  The workspace is
    about 16 Q k N / 384 bytes; above workspace_limit the queries run in blocks of a multiple of 128.
    k > 64 or k > N: the dense scores and select_topk, in query blocks under the same limit."""
    return _frame_topk(q, c, k, threshold, thr_mode, id_base, workspace_limit, exc, dense=cosine_scores_mfma,
                       size=_L().hq_cos_topk_workspace_size, fused=_L().hq_cos_topk,
                       operands=lambda r: (r.X16, r.inv))


MFMA_COS_MIN_WORK = 1 << 22


def cosine_scores(a, b, exc=None):
    """(cos + 1) / 2 of every row of a [Q, K] against every row of b [N, K] (rag/search/engine.py:622-660)
    -> f64 [Q, N].  Large problems run on the matrix cores (split-f16 MFMA, within 1e-5 of the
    reference's float32 BLAS result); small ones in the f64 kernel."""
    a2 = a.reshape(a.shape[0], -1)
    b2 = b.reshape(b.shape[0], -1)
    Q, N = int(a2.shape[0]), int(b2.shape[0])
    K = min(int(a2.shape[1]), int(b2.shape[1]))  # the reference truncates to the common length
    if Q * N * max(K, 1) >= MFMA_COS_MIN_WORK and K > 0:
        return cosine_scores_mfma(cos_prepare(a2[:, :K], exc), cos_prepare(b2[:, :K], exc), exc)
    return cosine_scores_f64(a, b, exc)


# ------------------------------------------------ comprehensive frame similarity (hq_comp.hip)


def _frames3(x):
    """Enhanced frames [N, H, W] (or one [H, W]) as a contiguous float32 / float64 device tensor."""
    t = torch()
    if x.dtype not in (t.float32, t.float64):
        x = x.to(t.float64)
    if x.dim() == 2:
        x = x.unsqueeze(0)
    if x.dim() != 3:
        raise ValueError("enhanced frames must be [N, H, W]")
    return _contig(x)


def comp_describe(frames, exc=None):
    """Per enhanced frame (h, L, width, row_mask) -> device int32 [N, 4] (hq_comp_describe): the detected original
    height, the number of non-zero index rows below it, their largest trimmed length, their bit set."""
    t = torch()
    x = _frames3(frames)
    N, H, W = (int(d) for d in x.shape)
    desc = t.empty((N, 4), dtype=t.int32, device=x.device)
    if N:
        _chk(_L().hq_comp_describe(dtype_code(x.dtype), ptr(x), N, H, W, ptr(desc), stream()), exc)
    return desc


def comp_scores(q, desc_q, c, desc_c, weights, parts: bool = False, exc=None):
    """The exact comprehensive score of every query frame [Q, H, W] against every frame [N, H, W] (one dtype,
    float32 or float64) from their comp_describe descriptors -> device f64 [Q, N] (and the components [Q, N, 3]
    with parts=True).  weights: host float64 [M + 1, M], row m = calculate_granularity_weights(m), M >= every L."""
    t = torch()
    q3, c3 = _frames3(q), _frames3(c)
    if q3.dtype != c3.dtype or q3.shape[1:] != c3.shape[1:]:
        raise ValueError(f"frames differ: {tuple(q3.shape[1:])} {q3.dtype} vs {tuple(c3.shape[1:])} {c3.dtype}")
    Q, H, W = (int(d) for d in q3.shape)
    N = int(c3.shape[0])
    wt = np.ascontiguousarray(weights, dtype=np.float64)
    ML = int(wt.shape[1]) if wt.ndim == 2 and wt.shape[0] > 1 else 0
    wd = t.as_tensor(wt.reshape(-1) if ML else np.zeros(1), device=q3.device)
    out = t.empty((Q, N), dtype=t.float64, device=q3.device)
    pt = t.empty((Q, N, 3), dtype=t.float64, device=q3.device) if parts else None
    if Q and N:
        _chk(_L().hq_comp_scores(dtype_code(q3.dtype), ptr(q3), ptr(_contig(desc_q)), Q, ptr(c3), ptr(_contig(desc_c)),
                                 N, H, W, ptr(wd), ML, ptr(out), ptr(pt) if parts else None, stream()), exc)
    return (out, pt) if parts else out


LIST_MAX = 1024


def comp_scores_listed(q, desc_q, c, desc_c, ids, weights, parts: bool = False, exc=None):
    """comp_scores through an id list (hq_comp_scores_listed, one launch): ids int64 [Q, C] -> device f64 [Q, C],
    entry (a, j) bit for bit what comp_scores writes for (query a, frame ids[a, j]); the frames are read in place.
    An id < 0 or >= N is a pad: -inf (parts 0.0).  parts=True adds the components [Q, C, 3]."""
    t = torch()
    q3, c3 = _frames3(q), _frames3(c)
    if q3.dtype != c3.dtype or q3.shape[1:] != c3.shape[1:]:
        raise ValueError(f"frames differ: {tuple(q3.shape[1:])} {q3.dtype} vs {tuple(c3.shape[1:])} {c3.dtype}")
    Q, H, W = (int(d) for d in q3.shape)
    N = int(c3.shape[0])
    il = _contig(ids.to(t.int64))
    if il.dim() != 2 or int(il.shape[0]) != Q:
        raise ValueError(f"ids {tuple(il.shape)} for {Q} queries")
    C = int(il.shape[1])
    wt = np.ascontiguousarray(weights, dtype=np.float64)
    ML = int(wt.shape[1]) if wt.ndim == 2 and wt.shape[0] > 1 else 0
    wd = t.as_tensor(wt.reshape(-1) if ML else np.zeros(1), device=q3.device)
    out = t.empty((Q, C), dtype=t.float64, device=q3.device)
    pt = t.empty((Q, C, 3), dtype=t.float64, device=q3.device) if parts else None
    if Q and C:
        _chk(_L().hq_comp_scores_listed(dtype_code(q3.dtype), ptr(q3), ptr(_contig(desc_q)), Q, ptr(c3) if N else None,
                                        ptr(_contig(desc_c)) if N else None, N, H, W, ptr(il), C, ptr(wd), ML,
                                        ptr(out), ptr(pt) if parts else None, stream()), exc)
    return (out, pt) if parts else out


def list_topk(scores, ids, k: int, threshold: float = 0.0, thr_mode: int = 0, exc=None):
    """The first k entries of every list in (score desc, list position asc) order (hq_list_topk, one launch):
    scores f64 [Q, C], ids int64 [Q, C] (id < 0: a pad; NaN scores never rank; thr_mode 0 none, 1 >=, 2 >)
    -> device (scores [Q, k] f64, ids [Q, k] i64, counts [Q] i32), -inf / -1 padded.  C <= 1024."""
    t = torch()
    sc = _contig(scores.to(t.float64))
    il = _contig(ids.to(t.int64))
    if sc.dim() != 2 or sc.shape != il.shape:
        raise ValueError(f"scores {tuple(sc.shape)} and ids {tuple(il.shape)}")
    Q, C = (int(d) for d in sc.shape)
    k = int(k)
    os_ = t.empty((Q, max(k, 0)), dtype=t.float64, device=sc.device)
    oi = t.empty((Q, max(k, 0)), dtype=t.int64, device=sc.device)
    cnt = t.empty(Q, dtype=t.int32, device=sc.device)
    _chk(_L().hq_list_topk(ptr(sc), ptr(il), Q, C, k, float(threshold), int(thr_mode), ptr(os_), ptr(oi), ptr(cnt),
                           stream()), exc)
    return os_, oi, cnt


def list_windows(heads, N: int, window: int, exc=None):
    """Every head frame widened to its window of consecutive frames (hq_list_windows, one launch;
    FrameCacheManager.cache_consecutive_frames, rag/search/frame_cache.py:66-72): heads int64 [Q, C0] (-1: no head)
    -> device (frames [Q, C0 window] i64: first appearances in head order, each window ascending, frames >= N
    dropped, -1 padded; counts [Q] i32).  window <= 64, C0 window <= 1024."""
    t = torch()
    hd = _contig(heads.to(t.int64))
    if hd.dim() != 2:
        raise ValueError(f"heads {tuple(hd.shape)} must be [Q, C0]")
    Q, C0 = (int(d) for d in hd.shape)
    window = int(window)
    out = t.empty((Q, C0 * max(window, 0)), dtype=t.int64, device=hd.device)
    cnt = t.zeros(Q, dtype=t.int32, device=hd.device)
    _chk(_L().hq_list_windows(ptr(hd), Q, C0, int(N), window, ptr(out), ptr(cnt), stream()), exc)
    return out, cnt


COMP_LAYOUT_FIELDS = ("K", "L", "ws", "stride", "ni", "nj", "off_win", "off_orig", "off_levels", "off_const",
                      "off_orig_ind", "off_win_ind")


def comp_layout(H: int, W: int, h: int, exc=None) -> dict:
    """The composite row of profile (h, L = H - h) of H x W frames (hq_comp_layout): its length K, the window
    geometry and the section offsets."""
    buf = (ctypes.c_int32 * 12)()
    k = _L().hq_comp_layout(int(H), int(W), int(h), buf)
    if k < 0:
        _chk(k, exc)
    return dict(zip(COMP_LAYOUT_FIELDS, (int(v) for v in buf)))


COMP_LDS_BYTES = 160 * 1024


def comp_prepare_fits(H: int, W: int, h: int) -> bool:
    """Whether hq_comp_prepare takes the profile: it keeps one float64 coefficient per section (H - h levels, the
    block, every window) of a tile's 16 frames in LDS, 160 KiB at the most (include/hq_mi355x.h); beyond that it
    returns HQ_E_UNSUPPORTED."""
    lay = comp_layout(H, W, h)
    return 16 * 8 * (lay["L"] + 1 + lay["ni"] * lay["nj"]) <= COMP_LDS_BYTES


def comp_prepare(frames, h: int, side: int, level_coef, exc=None) -> CosRows:
    """Float32 enhanced frames [N, H, W] of profile (h, L = H - h, every index row non-zero; the caller has
    checked the descriptors) -> their composite rows as a cosine operand (hq_comp_prepare): cosine_scores_mfma and
    cosine_topk of a side-0 (query) against a side-1 (corpus) operand return the comprehensive score.
    level_coef: host float64 [H - h], sqrt(0.5 w_l / sum w).  A [N, H, W] view whose frames are contiguous but lie
    more than H W values apart (frames cut out of a wider buffer) is read in place: its stride(0) is the kernel's ld."""
    t = torch()
    x = frames
    strided = (x.dim() == 3 and x.dtype == t.float32 and x.shape[0] > 1 and x.stride(2) == 1
               and x.stride(1) == x.shape[2] and x.stride(0) > x.shape[1] * x.shape[2])
    if not strided:
        x = _frames3(frames)
    if x.dtype != t.float32:
        raise TypeError("comp_prepare expects float32 frames")
    N, H, W = (int(d) for d in x.shape)
    ld = int(x.stride(0)) if strided else H * W
    K = comp_layout(H, W, h, exc)["K"]
    lc = np.ascontiguousarray(level_coef, dtype=np.float64).reshape(-1)
    if lc.size != H - int(h):
        raise ValueError(f"{lc.size} level coefficients for {H - int(h)} index rows")
    lcd = t.as_tensor(lc if lc.size else np.zeros(1), device=x.device)
    Kp = int(_L().hq_cos_padded_k(K))
    Np = int(_L().hq_cos_padded_rows(N))
    X16 = t.empty((max(Np, 1), 2, Kp), dtype=t.float16, device=x.device)
    inv = t.empty(max(Np, 1), dtype=t.float64, device=x.device)
    if N:
        _chk(_L().hq_comp_prepare(ptr(x), N, ld, H, W, int(h), int(side), ptr(lcd), ptr(X16), ptr(inv), stream()), exc)
    return CosRows(X16, inv, N, K)


# ------------------------------------------------ progressive hierarchical search (hq_hier.hip)

HIER_MAX_LEVELS = 8
HIER_MAX_K = 64


class HierRows:
    """Index rows of enhanced frames as hq_hier_prepare packs them: rows [N, max_levels, W] f64 (compacted, trimmed,
    zero padded), lens [N, max_levels] i32 (0: no such level), L [N] i32 on the device and levels (host int64 [N]):
    every frame's level count (a frame with more than max_levels levels keeps its first max_levels rows)."""

    __slots__ = ("rows", "lens", "L", "levels", "N", "W", "max_levels")

    def __init__(self, rows, lens, L, levels, N, W, max_levels):
        self.rows, self.lens, self.L, self.levels = rows, lens, L, levels
        self.N, self.W, self.max_levels = int(N), int(W), int(max_levels)

    @property
    def nbytes(self) -> int:
        return sum(x.numel() * x.element_size() for x in (self.rows, self.lens, self.L))


def hier_prepare(frames, desc=None, max_levels: Optional[int] = None, clamp: bool = False, exc=None) -> HierRows:
    """Enhanced frames [N, H, W] (float32 / float64) -> HierRows (hq_hier_prepare, one launch).  desc: their
    comp_describe descriptors (computed when None).  max_levels: levels kept per frame (default: the largest level
    count of the batch, at least 1).  A frame with more levels is refused with the library's HQ_E_UNSUPPORTED
    message, unless clamp=True: then its first max_levels rows are packed and `levels` keeps the true count (the
    query side of hier_filter)."""
    t = torch()
    x = _frames3(frames)
    N, H, W = (int(d) for d in x.shape)
    d_dev = comp_describe(x, exc) if desc is None else _contig(desc)
    d = d_dev.cpu().numpy().astype(np.int64).reshape(N, 4)
    levels = np.maximum(d[:, 1], 0)
    ml = int(max_levels) if max_levels is not None else max(1, min(int(levels.max(initial=0)), HIER_MAX_LEVELS))
    if clamp and N and int(levels.max(initial=0)) > ml:
        d2 = d.copy()
        for i in np.flatnonzero(levels > ml):
            m, kept = int(d2[i, 3]) & 0xFFFFFFFF, 0
            for _ in range(ml):  # the lowest max_levels bits of the row mask
                low = m & -m
                kept |= low
                m ^= low
            d2[i, 3], d2[i, 1] = kept, ml
        d_dev = t.as_tensor(d2.astype(np.int32), device=x.device)
    rows = t.empty((N, ml, W), dtype=t.float64, device=x.device)
    lens = t.empty((N, ml), dtype=t.int32, device=x.device)
    if N:
        _chk(_L().hq_hier_prepare(dtype_code(x.dtype), ptr(x), N, H * W, H, W, ptr(d_dev), ml, ptr(rows), ptr(lens),
                                  stream()), exc)
    L = t.as_tensor(levels.astype(np.int32), device=x.device)
    return HierRows(rows, lens, L, levels, N, W, ml)


def hier_filter(q: HierRows, c: HierRows, thr, ratio, kout: int = 20, want_alive: bool = False,
                workspace_bytes: int = 1 << 30, want_scores: bool = False, exc=None):
    """The progressive hierarchical cascade of every prepared query against the prepared corpus (hq_hier_filter)
    -> device (counts [Q, max_levels] i64, top_ids [Q, kout] i64 (-1 padded), top_scores [Q, kout, max_levels] f64,
    alive [Q, N] u8 or None).  thr, ratio: the level tables (max_levels values each, host).  The workspace holds
    max_levels * Qb * N float64 scores; the queries run in blocks of Qb so that it stays under workspace_bytes.
    want_scores=True (a batch that runs as one block) appends the level scores S [max_levels, Q, N] f64: a view of
    the calling thread's workspace, valid until its next workspace-using call on this stream."""
    t = torch()
    if q.W != c.W or q.max_levels != c.max_levels:
        raise ValueError(f"query rows [{q.max_levels}, {q.W}] against corpus rows [{c.max_levels}, {c.W}]")
    kout = int(kout)
    if not 0 <= kout <= HIER_MAX_K:
        raise ValueError(f"kout = {kout} (0 .. {HIER_MAX_K})")
    ml, Q, N = c.max_levels, q.N, c.N
    th = np.ascontiguousarray(thr, dtype=np.float64).reshape(-1)
    ra = np.ascontiguousarray(ratio, dtype=np.float64).reshape(-1)
    if th.size < ml or ra.size < ml:
        raise ValueError(f"{th.size} thresholds and {ra.size} ratios for {ml} levels")
    dev = c.rows.device
    counts = t.zeros((Q, ml), dtype=t.int64, device=dev)
    ids = t.full((Q, kout), -1, dtype=t.int64, device=dev)
    sc = t.zeros((Q, kout, ml), dtype=t.float64, device=dev)
    alive = t.zeros((Q, N), dtype=t.uint8, device=dev) if want_alive else None
    if Q == 0 or N == 0:
        if want_scores:
            return counts, ids, sc, alive, t.zeros((ml, Q, N), dtype=t.float64, device=dev)
        return counts, ids, sc, alive
    size = _L().hq_hier_workspace_size
    per = Q
    limit = max(int(workspace_bytes), 1)
    if int(size(Q, N, ml)) > limit:
        per = max(1, limit // max(int(size(1, N, ml)), 1))
    if want_scores and per < Q:
        raise ValueError("want_scores=True needs the batch in one workspace block")
    th_p = th.ctypes.data_as(ctypes.c_void_p)
    ra_p = ra.ctypes.data_as(ctypes.c_void_p)
    for q0 in range(0, Q, per):
        q1 = min(Q, q0 + per)
        wb = int(size(q1 - q0, N, ml))
        ws = _workspace(wb, dev)
        _chk(_L().hq_hier_filter(ptr(q.rows[q0:q1]), ptr(q.lens[q0:q1]), ptr(q.L[q0:q1]), q1 - q0, ptr(c.rows),
                                 ptr(c.lens), N, c.W, ml, th_p, ra_p, kout, ptr(ws), ptr(counts[q0:q1]),
                                 ptr(ids[q0:q1]) if kout else None, ptr(sc[q0:q1]) if kout else None,
                                 ptr(alive[q0:q1]) if want_alive else None, stream()), exc)
    if want_scores:
        return counts, ids, sc, alive, ws[:ml * Q * N * 8].view(t.float64).view(ml, Q, N)
    return counts, ids, sc, alive


# ------------------------------------------------ compressed-domain frame search (u8 frames, exact)


class CosQRows:
    """u8 rows prepared for the exact integer cosine (hq_cosq_prepare): X8 [Np, Kp] signed bytes in 1 KiB i8 MFMA
    operand fragments, stats [Np, 4] f64 (pre-scaled a, b, S, inv != 0): one byte per value resident where the
    split-f16 rows of the decoded frames hold four."""

    __slots__ = ("X8", "stats", "N", "K", "cap")

    def __init__(self, X8, stats, N, K, cap=None):
        self.X8, self.stats, self.N, self.K = X8, stats, int(N), int(K)
        # rows the buffers hold, in whole 128-row units (cosq_reserve / cosq_append / cosq_gather size them)
        self.cap = int(X8.shape[0]) // 128 * 128 if cap is None else int(cap)

    @property
    def nbytes(self) -> int:
        return self.X8.numel() * self.X8.element_size() + self.stats.numel() * self.stats.element_size()


def _frame_rows(x, rows: Optional[int], what: str, n: str):
    """x [N, r, c] (or rows [N, K]) -> (x2 [N, row length] read in place, N, K): K = rows * c values out of every
    r * c, every row by default.  what / n: the argument's name and its row-count letter in the messages."""
    if x.dim() < 2:
        raise ValueError(f"{what} must be [{n}, ...]")
    N = int(x.shape[0])
    if x.dim() == 2:
        if rows is not None:
            raise ValueError(f"rows= needs frames [{n}, r, c]")
        x2 = x if x.stride(-1) == 1 else x.contiguous()
        return x2, N, int(x2.shape[1])
    r, c = int(x.shape[1]), int(np.prod(x.shape[2:]))
    rows = r if rows is None else int(rows)
    if not 1 <= rows <= r:
        raise ValueError(f"rows = {rows} of {r}")
    return _contig(x).view(N, r * c), N, rows * c


def cosq_prepare(frames, minmax, rows: Optional[int] = None, exc=None) -> CosQRows:
    """u8 frames [N, r, c] (or rows [N, K]) with minmax f32 [N, 2] -> CosQRows of the first `rows` rows of every
    frame (all of them by default).  The frames are read in place: K = rows * c bytes out of every r * c."""
    t = torch()
    if frames.dtype != t.uint8:
        raise TypeError("cosq_prepare expects uint8 frames (quantise float32 rows with map_index_quantize / quantize_u8)")
    x2, N, K = _frame_rows(frames, rows, "frames", "N")
    mm = _contig(minmax.reshape(-1, 2).to(t.float32))
    if int(mm.shape[0]) != N:
        raise ValueError(f"{int(mm.shape[0])} (min, max) pairs for {N} frames")
    Kp = int(_L().hq_cosq_padded_k(K))
    Np = int(_L().hq_cosq_padded_rows(N))
    X8 = t.empty((max(Np, 1), max(Kp, 1)), dtype=t.int8, device=x2.device)
    stats = t.empty((max(Np, 1), 4), dtype=t.float64, device=x2.device)
    if N:
        _chk(_L().hq_cosq_prepare(ptr(x2), N, x2.stride(0) if N > 1 else int(x2.shape[1]), K, ptr(mm), ptr(X8),
                                  ptr(stats), stream()), exc)
    return CosQRows(X8, stats, N, K)


def _rows128(n: int) -> int:
    return (n + 127) // 128 * 128


def _cosq_buffers(cap: int, c: CosQRows):
    t = torch()
    X8 = t.empty((max(cap, 1), int(c.X8.shape[1])), dtype=t.int8, device=c.X8.device)
    stats = t.empty((max(cap, 1), 4), dtype=t.float64, device=c.X8.device)
    return X8, stats


def cosq_reserve(c: CosQRows, capacity: int) -> CosQRows:
    """A CosQRows of the same N rows whose buffers hold `capacity` rows, rounded up to a multiple of 128 (c itself
    when they already do): new buffers, device-to-device copies of the valid extent (the padded rows of N).  The
    rows past it are written by cosq_append."""
    cap = _rows128(int(capacity))
    if cap <= c.cap:
        return c
    X8, stats = _cosq_buffers(cap, c)
    Np = _rows128(c.N)
    X8[:Np].copy_(c.X8[:Np])
    stats[:Np].copy_(c.stats[:Np])
    return CosQRows(X8, stats, c.N, c.K, cap)


def _cosq_incoming(c: CosQRows, frames, minmax, rows, what: str):
    """The u8 frames and (min, max) pairs a writer of c takes: (x2 read in place, ld, mm, M)."""
    t = torch()
    if frames.dtype != t.uint8:
        raise TypeError(f"{what} expects uint8 frames")
    x2, M, K = _frame_rows(frames, rows, "frames", "M")
    if K != c.K:
        raise ValueError(f"{what}: frame length {K} != corpus frame length {c.K}")
    mm = _contig(minmax.reshape(-1, 2).to(t.float32))
    if int(mm.shape[0]) != M:
        raise ValueError(f"{int(mm.shape[0])} (min, max) pairs for {M} frames")
    return x2, (x2.stride(0) if M > 1 else int(x2.shape[1])), mm, M


def cosq_append(c: CosQRows, frames, minmax, rows: Optional[int] = None, exc=None) -> CosQRows:
    """c grown by the u8 `frames` [M, r, c] (or rows [M, K]) with minmax f32 [M, 2] (rows= as cosq_prepare): one
    hq_cosq_append launch prepares them behind the resident rows, which do not move, and writes the pad rows after
    them; byte-identical to cosq_prepare of all N + M frames.  Beyond the capacity the buffers grow geometrically
    (x 2, at least the need: cosq_reserve).  Returns a new CosQRows over the same buffers; c must not be searched
    afterwards (what it took for pad rows are real rows now), and searches of c still running on other streams
    must have finished before the call."""
    x2, ld, mm, M = _cosq_incoming(c, frames, minmax, rows, "cosq_append")
    if M == 0:
        return c
    N0, N1 = c.N, c.N + M
    if _rows128(N1) > c.cap:
        c = cosq_reserve(c, max(N1, 2 * c.cap))
    _chk(_L().hq_cosq_append(ptr(x2), M, ld, c.K, ptr(mm), N0, c.cap, ptr(c.X8), ptr(c.stats), stream()), exc)
    return CosQRows(c.X8, c.stats, N1, c.K, c.cap)


def cosq_replace(c: CosQRows, row_ids, frames, minmax, rows: Optional[int] = None, checked: bool = False,
                 exc=None) -> CosQRows:
    """c with the resident rows `row_ids` (distinct row numbers in [0, c.N)) overwritten in place by the u8 `frames`
    [M, r, c] (or rows [M, K]) with minmax f32 [M, 2]: one hq_cosq_replace launch rewrites those rows' bytes and
    statistics; byte-identical to cosq_prepare of the updated frames.  A writer, as cosq_append: no search of c may
    be running.  Returns c.  IndexError for a row out of range, ValueError for a repeated row, before any launch
    (checked: the caller has validated the row numbers)."""
    t = torch()
    x2, ld, mm, M = _cosq_incoming(c, frames, minmax, rows, "cosq_replace")
    sel = _row_ids(row_ids, c.N, x2.device, "cosq_replace", checked)
    if int(sel.numel()) != M:
        raise ValueError(f"{int(sel.numel())} row numbers for {M} replacement frames")
    if not checked and M > 1 and int(t.unique(sel).numel()) != M:
        raise ValueError("cosq_replace: repeated row numbers")
    if M:
        _chk(_L().hq_cosq_replace(ptr(x2), M, ld, c.K, ptr(mm), ptr(sel), c.N, ptr(c.X8), ptr(c.stats), stream()), exc)
    return c


def cosq_gather(c: CosQRows, src_rows, cap: Optional[int] = None, checked: bool = False, exc=None) -> CosQRows:
    """A new CosQRows of the rows c[src_rows] (row numbers in [0, c.N), any order, repeats allowed), in a second
    pair of buffers with room for max(cap or c.cap, M) rows (a multiple of 128): one hq_cosq_gather launch moves
    each row's 16-byte pieces and statistics, byte-identical to cosq_prepare of the selected frames.  c is only
    read.  IndexError for a row out of range, before the launch (checked: the caller has validated them)."""
    sel = _row_ids(src_rows, c.N, c.X8.device, "cosq_gather", checked)
    M = int(sel.numel())
    cap = max(_rows128(int(cap) if cap else c.cap), _rows128(M))
    X8, stats = _cosq_buffers(cap, c)
    _chk(_L().hq_cosq_gather(ptr(sel), M, c.N, c.K, ptr(c.X8), ptr(c.stats), cap, ptr(X8), ptr(stats), stream()), exc)
    return CosQRows(X8, stats, M, c.K, cap)


def cosq_scores(q: CosQRows, c: CosQRows, exc=None):
    """(cos + 1) / 2 of the dequantised rows, every prepared query against every prepared frame -> f64 [Q, N],
    within a few float64 roundings of the exact value (hq_cosq_scores: an exact int8 MFMA contraction)."""
    t = torch()
    if q.K != c.K:
        raise ValueError(f"query length {q.K} != frame length {c.K}")
    out = t.empty((q.N, c.N), dtype=t.float64, device=q.X8.device)
    _chk(_L().hq_cosq_scores(ptr(q.X8), ptr(q.stats), q.N, ptr(c.X8), ptr(c.stats), c.N, q.K, ptr(out), stream()), exc)
    return out


def cosq_topk(q: CosQRows, c: CosQRows, k: int, threshold: float = 0.0, thr_mode: int = 0, id_base: int = 0,
              workspace_limit: int = 256 << 20, exc=None):
    """The k nearest prepared u8 frames of every prepared u8 query -> (scores [Q, k] f64, ids [Q, k] i64), equal to
    select_topk(cosq_scores(q, c), k, threshold, thr_mode, id_base) in ids, order and score bits (hq_cosq_topk).
    Workspace, query blocks under workspace_limit and the dense route for k > 64 or k > N: as cosine_topk."""
    return _frame_topk(q, c, k, threshold, thr_mode, id_base, workspace_limit, exc, dense=cosq_scores,
                       size=_L().hq_cosq_topk_workspace_size, fused=_L().hq_cosq_topk,
                       operands=lambda r: (r.X8, r.stats))


# ------------------------------------------------ float32 queries against the u8 frame store (exact, asymmetric)


class CosQFRows:
    """Float32 query rows prepared for the asymmetric cosine against CosQRows frames (hq_cosqf_prepare): Q8
    [Qp, 3 Kp] the three int8 digit planes of the rows' 24-bit fixed-point values in i8 MFMA operand fragments,
    stats [Qp, 4] f64 (A_q, B_q, Sv, ok)."""

    __slots__ = ("Q8", "stats", "N", "K")

    def __init__(self, Q8, stats, N, K):
        self.Q8, self.stats, self.N, self.K = Q8, stats, int(N), int(K)

    @property
    def nbytes(self) -> int:
        return self.Q8.numel() * self.Q8.element_size() + self.stats.numel() * self.stats.element_size()


def cosqf_prepare(x, rows: Optional[int] = None, exc=None) -> CosQFRows:
    """float32 frames [Q, r, c] (or rows [Q, K]) -> CosQFRows of the first `rows` rows of every frame (all of them
    by default).  The frames are read in place: K = rows * c floats out of every r * c."""
    t = torch()
    if x.dtype != t.float32:
        raise TypeError("cosqf_prepare expects float32 queries (u8 query frames go through cosq_prepare)")
    x2, Q, K = _frame_rows(x, rows, "queries", "Q")
    Kp = int(_L().hq_cosq_padded_k(K))
    Qp = int(_L().hq_cosqf_padded_rows(Q))
    Q8 = t.empty((max(Qp, 1), 3 * max(Kp, 1)), dtype=t.int8, device=x2.device)
    stats = t.empty((max(Qp, 1), 4), dtype=t.float64, device=x2.device)
    if Q:
        _chk(_L().hq_cosqf_prepare(ptr(x2), Q, x2.stride(0) if Q > 1 else int(x2.shape[1]), K, ptr(Q8), ptr(stats),
                                   stream()), exc)
    return CosQFRows(Q8, stats, Q, K)


def cosqf_scores(q: CosQFRows, c: CosQRows, exc=None):
    """(cos + 1) / 2 of every prepared float32 query (its 24-bit fixed-point row) against every dequantised
    prepared frame -> f64 [Q, N], within a few float64 roundings of the exact value (hq_cosqf_scores: three exact
    int8 MFMA contractions per pair)."""
    t = torch()
    if q.K != c.K:
        raise ValueError(f"query length {q.K} != frame length {c.K}")
    out = t.empty((q.N, c.N), dtype=t.float64, device=q.Q8.device)
    _chk(_L().hq_cosqf_scores(ptr(q.Q8), ptr(q.stats), q.N, ptr(c.X8), ptr(c.stats), c.N, q.K, ptr(out), stream()), exc)
    return out


def cosqf_topk(q: CosQFRows, c: CosQRows, k: int, threshold: float = 0.0, thr_mode: int = 0, id_base: int = 0,
               workspace_limit: int = 256 << 20, exc=None):
    """The k nearest prepared u8 frames of every prepared float32 query -> (scores [Q, k] f64, ids [Q, k] i64),
    equal to select_topk(cosqf_scores(q, c), k, threshold, thr_mode, id_base) in ids, order and score bits
    (hq_cosqf_topk).  Workspace, query blocks under workspace_limit and the dense route for k > 64 or k > N: as
    cosq_topk."""
    return _frame_topk(q, c, k, threshold, thr_mode, id_base, workspace_limit, exc, dense=cosqf_scores,
                       size=_L().hq_cosqf_topk_workspace_size, fused=_L().hq_cosqf_topk,
                       operands=lambda r: (r.Q8 if isinstance(r, CosQFRows) else r.X8, r.stats))
