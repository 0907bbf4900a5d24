"""The firefly pre-filter (bmfr_suppress_fireflies, include/bmfr.h) restated in
numpy, one f32 operation per line as the header documents them.  TEST
INFRASTRUCTURE ONLY: imports nothing from bmfr_amd.

    suppress(noisy, w, h, threshold=2, radius=1, floor=0, replace_nonfinite=True)
        -> (out, (clamped, replaced))
noisy: a float3 (float32) or half3 (float16) plane of a w x h region, any
shape with w * h * 3 elements; out has noisy's dtype and shape.  Pixels the
rules do not touch keep their bytes.
"""
from __future__ import annotations

import numpy as np

F32 = np.float32
KR, KG, KB = F32(0.2126), F32(0.7152), F32(0.0722)


def luminance(px: np.ndarray) -> np.ndarray:
    """Y = (0.2126f * r + 0.7152f * g) + 0.0722f * b of (..., 3) f32 pixels."""
    with np.errstate(all="ignore"):
        return (KR * px[..., 0] + KG * px[..., 1]) + KB * px[..., 2]


def neighbour_max(Y: np.ndarray, radius: int) -> np.ndarray:
    """Rule 2: the maximum finite Y over the (2r + 1)^2 window without its
    centre, clipped to the plane; -inf where no neighbour has a finite Y."""
    h, w = Y.shape
    pad = np.full((h + 2 * radius, w + 2 * radius), -np.inf, F32)
    pad[radius:radius + h, radius:radius + w] = np.where(np.isfinite(Y), Y, F32(-np.inf))
    m = np.full((h, w), -np.inf, F32)
    for dy in range(2 * radius + 1):
        for dx in range(2 * radius + 1):
            if dy != radius or dx != radius:
                m = np.maximum(m, pad[dy:dy + h, dx:dx + w])
    return m


def suppress(noisy: np.ndarray, w: int, h: int, threshold=2.0, radius=1, floor=0.0, replace_nonfinite=True):
    assert noisy.dtype in (np.float32, np.float16) and noisy.size == w * h * 3 and radius in (1, 2)
    threshold, floor = F32(threshold), F32(floor)
    src = noisy.reshape(h, w, 3)
    px = src.astype(F32)  # half widens exactly
    Y = luminance(px)
    invalid = ~np.isfinite(px).all(axis=-1)  # rule 1
    m = neighbour_max(Y, radius)             # rule 2
    with np.errstate(all="ignore"):
        limit = threshold * m                # rule 3
        limit = np.where(limit > floor, limit, floor)
        clamp = ~invalid & (m > -np.inf) & (Y > limit)  # rule 4
        s = limit / Y
        scaled = (px * s[..., None]).astype(noisy.dtype)  # a half result: round to nearest even
    out = src.copy()
    out[clamp] = scaled[clamp]
    replaced = 0
    if replace_nonfinite:
        out[invalid] = 0
        replaced = int(invalid.sum())
    return out.reshape(noisy.shape), (int(clamp.sum()), replaced)


def content(w: int, h: int, half: bool = False, frame: int = 1, seed: int = 2) -> np.ndarray:
    """A w x h noisy plane for the parity tests, (h, w, 3) float32 or float16:
    scene rand of tests/scenes_np.py (its own x50 fireflies included) with
    extremes written over it -- x50 and x1e6 pixels at corners, edges and in
    the interior, an adjacent pair, NaN / +inf / -inf channels, negative
    pixels, an exactly black 9 x 9 patch around one lit pixel, denormals and
    signed zeros, values past half's range (inf once narrowed).  Positions
    are clipped into the plane, so small planes hold them on top of each other."""
    import scenes_np
    p = np.array(scenes_np.frame("rand", w, h, frame, seed)["noisy"]).reshape(h, w, 3)
    at = lambda x, y: (min(max(y, 0), h - 1), min(max(x, 0), w - 1))  # noqa: E731
    if w >= 9 and h >= 9:
        y0, x0 = at(w - 20, h - 15)
        y0, x0 = min(y0, h - 9), min(x0, w - 9)
        p[y0:y0 + 9, x0:x0 + 9] = 0.0
        p[y0 + 4, x0 + 4] = 0.3
    spots = [(0, 0), (w - 1, 0), (0, h - 1), (w - 1, h - 1), (w // 2, 0), (0, h // 2), (w - 1, h // 2),
             (w // 2, h - 1), (w // 3, h // 3), (2 * w // 3, h // 2 + 1), (w // 5, 2 * h // 3)]
    with np.errstate(over="ignore"):  # on a 1 x 1 plane every factor lands on one pixel
        for i, (x, y) in enumerate(spots):
            p[at(x, y)] *= F32(50.0) if i % 2 == 0 else F32(1e6)
        p[at(w // 2, h // 2)] *= F32(50.0)       # the adjacent pair
        p[at(w // 2 + 1, h // 2)] *= F32(50.0)
    p[at(w // 4, h // 4)][0] = np.nan
    p[at(w // 4 + 3, h // 4)][1] = np.inf
    p[at(w // 4, h // 4 + 3)][2] = -np.inf
    p[at(w // 4 + 1, h // 4 + 1)] *= F32(50.0)  # a firefly whose neighbours include the NaN pixel
    p[at(3 * w // 4, h // 4)] = (-1.0, -2.0, -0.5)
    p[at(3 * w // 4 + 2, h // 4)] = (4.0, -0.25, 1.0)
    p[at(3 * w // 4, h // 4 + 2)] = (1e-40, 1e-41, 0.0)   # f32 denormals
    p[at(3 * w // 4 + 2, h // 4 + 2)] = (3e-7, 6e-8, 3e-7)  # half denormals
    p[at(3 * w // 4 + 4, h // 4 + 2)] = (-0.0, 0.0, -0.0)
    p[at(w // 3 + 2, 3 * h // 4)] = (1e30, 2e30, 1e29)
    p[at(w // 3 + 4, 3 * h // 4)] = (3.3e38, 3.3e38, 3.3e38)   # finite channels, Y at f32's edge
    if half:
        with np.errstate(over="ignore"):
            return p.astype(np.float16)
    return p


def differing_rings(w: int, h: int, region, radius: int) -> np.ndarray:
    """(rh, rw) mask of the pixels of region (x, y, rw, rh) of a w x h image
    whose filtered value may differ from the whole-image filter's: the
    outermost `radius` rings along the region's edges that lie inside the
    image (an edge on the image border cuts both windows alike)."""
    x0, y0, rw, rh = region
    mask = np.zeros((rh, rw), bool)
    if x0 > 0:
        mask[:, :radius] = True
    if x0 + rw < w:
        mask[:, rw - radius:] = True
    if y0 > 0:
        mask[:radius, :] = True
    if y0 + rh < h:
        mask[rh - radius:, :] = True
    return mask
