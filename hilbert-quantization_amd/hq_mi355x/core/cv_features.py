"""Image similarities of the reference's core/cv_features.py on the device: SSIM (calculate_ssim with
_calculate_ssim_manual, :386-457 and :657-704) and the template score of two equal-sized frames (template_matching,
:199-262: cv2.matchTemplate TM_CCOEFF_NORMED, a 1 x 1 map there).  Histogram correlation and ORB are not here.

Frames are uint8, 4 x 4 to 131 x 128 pixels; win_size 7 is the only window (the only one the reference calls).
No OpenCV is involved: the Gaussian taps are exp(-(i - 3)^2 / 4.5) normalised to sum 1 and the border is mirrored
without repeating the edge pixel, which is what cv2.getGaussianKernel(7, 1.5) and cv2.filter2D's default border are
documented to do (DESIGN.md lists what could not be checked against OpenCV itself)."""
from __future__ import annotations

import numpy as np

from .. import kernels as K
from .._dev import to_dev, to_np


def _check_window(win_size: int):
    if int(win_size) != 7:
        raise ValueError(f"win_size must be 7 (the reference's only window), got {win_size}")


def ssim_scores(queries_u8, frames_u8, ncc: bool = False):
    """SSIM of every query frame [Q, H, W] against every frame [N, H, W] (uint8) -> device float64 [Q, N]; ncc=True
    returns (ssim, template correlation), both [Q, N]."""
    return K.ssim_scores(K.ssim_prepare(to_dev(queries_u8)), to_dev(frames_u8), ncc=ncc)


def ssim_scores_listed(queries_u8, frames_u8, ids, ncc: bool = False):
    """The same scores for the listed frames only: ids int64 [Q, C] into frames_u8 -> device float64 [Q, C], each
    entry bit for bit the dense one; an id < 0 or >= N is a pad and scores -inf."""
    return K.ssim_scores_listed(K.ssim_prepare(to_dev(queries_u8)), to_dev(frames_u8), to_dev(ids), ncc=ncc)


def _one_u8(image, what: str):
    a = to_np(image) if hasattr(image, "device") else np.asarray(image)
    if a.ndim != 2:
        raise ValueError(f"{what} must be one 2-D grayscale frame, got shape {a.shape}")
    return a


def calculate_ssim(image1, image2, win_size: int = 7) -> float:
    """The reference's calculate_ssim(image1, image2).ssim_score for two uint8 grayscale frames of one shape.

    Only the score is returned: the SSIM map (and its mean / std fields of SSIMResult) never leaves the device.
    The reference takes float images as they are, without rounding them to uint8, so float images are refused here
    rather than scored differently; colour images and frames of different shapes (which the reference resizes with
    OpenCV) are refused too."""
    _check_window(win_size)
    a, b = _one_u8(image1, "image1"), _one_u8(image2, "image2")
    if a.dtype != np.uint8 or b.dtype != np.uint8:
        raise TypeError(f"calculate_ssim takes uint8 frames, got {a.dtype} and {b.dtype}")
    if a.shape != b.shape:
        raise ValueError(f"frames differ in shape: {a.shape} vs {b.shape}")
    return float(to_np(ssim_scores(a[None], b[None]))[0, 0])


def _template_u8(a):
    """template_matching's conversion (:225-231): a non-uint8 image is min-max scaled to 0 .. 255 and truncated."""
    if a.dtype == np.uint8:
        return a
    a = a.astype(np.float64)
    rng = a.max() - a.min()
    if not np.isfinite(rng) or rng == 0:
        raise ValueError("a constant or non-finite float image has no min-max scaling")
    return ((a - a.min()) / rng * 255).astype(np.uint8)


def template_correlation(a, b) -> float:
    """The template score of two frames of one shape: the Pearson correlation of their pixels (TM_CCOEFF_NORMED
    where the template covers the image), float64 from exact integer sums; 0.0 when either frame is constant."""
    x, y = _template_u8(_one_u8(a, "a")), _template_u8(_one_u8(b, "b"))
    if x.shape != y.shape:
        raise ValueError(f"frames differ in shape: {x.shape} vs {y.shape}")
    return float(to_np(ssim_scores(x[None], y[None], ncc=True)[1])[0, 0])
