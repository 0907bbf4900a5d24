"""numpy restatement of the display-resolution TAA (bmfr_display_taa,
include/bmfr.h "Display-resolution TAA", rules 1-7): every line one np.float32
operation, as the header writes them.  The motion rule is tests/prepare_np.py's
and the surface encoding tests/resolve_np.py's, as the header says.  The GPU
tests hold the kernel to this byte for byte.  TEST INFRASTRUCTURE ONLY.

A plane is a numpy array (Hd, Wd, 3) float32 (F32X3) or (Hd, Wd, 4) float16
(F16X4, 4th component ignored when read)."""
from __future__ import annotations

import numpy as np

import prepare_np as pn
import resolve_np as rn

F32 = np.float32
INF = F32(np.inf)


def values(plane) -> np.ndarray:
    """A plane as f32 (Hd, Wd, 3); half values widen exactly."""
    plane = np.asarray(plane)
    if plane.dtype == np.float32:
        assert plane.shape[-1] == 3
        return plane
    assert plane.dtype == np.float16 and plane.shape[-1] == 4
    return plane[..., :3].astype(F32)


def vmin(a, b):
    """min that ignores a NaN operand and orders -0 below +0."""
    return np.where((a == b) & np.signbit(b), b, np.fmin(a, b)).astype(F32)


def vmax(a, b):
    """max that ignores a NaN operand and orders -0 below +0."""
    return np.where((a == b) & ~np.signbit(b), b, np.fmax(a, b)).astype(F32)


def dot(c, b) -> np.ndarray:
    """dot(c, b) = fma(c.z, b.z, fma(c.y, b.y, c.x * b.x)) for coefficients that
    are powers of two (or 0): the products are exact, so the chain is two
    rounded additions (short of overflow and underflow of a product)."""
    with np.errstate(all="ignore"):
        r = (c[..., 0] * F32(b[0]) + c[..., 1] * F32(b[1])) + c[..., 2] * F32(b[2])
    assert r.dtype == F32
    return r


def ycocg(c) -> np.ndarray:
    return np.stack([dot(c, (1, 2, 1)), dot(c, (2, 0, -2)), dot(c, (-1, 2, -1))], axis=-1)


def rgb(c) -> np.ndarray:
    return np.stack([dot(c, (.25, .25, -.25)), dot(c, (.25, 0, .25)), dot(c, (.25, -.25, -.25))], axis=-1)


def previous_position(Wd: int, Hd: int, prev_pixel=None, motion=None, motion_scale=(1.0, 1.0), at_centre=False,
                      pixel_offset=(0.5, 0.5)) -> np.ndarray:
    """Rule 2: (pfx, pfy) per display pixel, f32 (Hd, Wd, 2)."""
    assert (prev_pixel is None) != (motion is None)
    if prev_pixel is not None:
        return np.asarray(prev_pixel, F32).reshape(Hd, Wd, 2)
    return pn.prev_pixel_of(np.asarray(motion), motion_scale, at_centre, pixel_offset, (0, 0, Wd, Hd)).reshape(Hd, Wd, 2)


def bounds(s: np.ndarray):
    """Rule 4: (mnb, mxb, mnc, mxc) of the YCoCg image s; a neighbour outside
    the image does not take part (it enters as +inf / -inf)."""
    H, W, _ = s.shape
    lo = np.full((H + 2, W + 2, 3), INF, F32)
    hi = np.full((H + 2, W + 2, 3), -INF, F32)
    lo[1:-1, 1:-1] = s
    hi[1:-1, 1:-1] = s
    mnb = mnc = np.full((H, W, 3), INF, F32)
    mxb = mxc = np.full((H, W, 3), -INF, F32)
    for dy in (-1, 0, 1):
        for dx in (-1, 0, 1):
            a = lo[1 + dy:1 + dy + H, 1 + dx:1 + dx + W]
            b = hi[1 + dy:1 + dy + H, 1 + dx:1 + dx + W]
            if dx == 0 or dy == 0:
                mnc, mxc = vmin(mnc, a), vmax(mxc, b)
            mnb, mxb = vmin(mnb, a), vmax(mxb, b)
    return mnb, mxb, mnc, mxc


def display_taa(current, history, pf, blend_alpha, reset: bool = False) -> np.ndarray:
    """Rules 1-6 -> v, f32 (Hd, Wd, 3).  current, history: planes (history None:
    no history); pf: previous_position's (ignored without history)."""
    me = values(current)
    H, W, _ = me.shape
    if reset or history is None:
        return me.copy()
    hist = values(history)
    assert hist.shape == me.shape
    pf = np.asarray(pf, F32).reshape(H, W, 2)
    pfx, pfy = pf[..., 0], pf[..., 1]
    a = F32(blend_alpha)
    with np.errstate(all="ignore"):
        flx, fly = np.floor(pfx), np.floor(pfy)
        off = (flx < F32(-1)) | (fly < F32(-1)) | (flx >= F32(W)) | (fly >= F32(H))   # a NaN goes on
        mnb, mxb, mnc, mxc = bounds(ycocg(me))
        ix = np.fmin(np.fmax(flx, F32(-2)), F32(W) + F32(1)).astype(np.int64)
        iy = np.fmin(np.fmax(fly, F32(-2)), F32(H) + F32(1)).astype(np.int64)
        fx, fy = pfx - flx, pfy - fly
        omx, omy = F32(1) - fx, F32(1) - fy
        prev = np.zeros((H, W, 3), F32)
        total = np.zeros((H, W), F32)
        for j, wy, oky in ((0, omy, iy >= 0), (1, fy, iy < H - 1)):
            for i, wx, okx in ((0, omx, ix >= 0), (1, fx, ix < W - 1)):
                w = wx * wy
                tap = hist[np.clip(iy + j, 0, H - 1), np.clip(ix + i, 0, W - 1)]   # any pixel where the tap does not enter
                enter = okx & oky
                prev = np.where(enter[..., None], prev + w[..., None] * tap, prev)
                total = np.where(enter, total + w, total)
        prev = prev / total[..., None]
        py = ycocg(prev)
        lo = (mnb + mnc) / F32(2)
        hi = (mxb + mxc) / F32(2)
        cl = vmin(vmax(py, lo), hi)
        pr = rgb(cl)
        b = F32(1) - a
        v = a * me + b * pr
    assert v.dtype == F32 and prev.dtype == F32 and total.dtype == F32 and lo.dtype == F32
    return np.where(off[..., None], me, v).astype(F32)


def display_prev_pixel(fr: dict, Wd: int, Hd: int) -> np.ndarray:
    """A display-resolution prev_pixel plane (Hd, Wd, 2) for a scenes_np frame
    at display size: its positions through prev_vp (column-major) in float64,
    pfx = u Wd - jx, pfy = v Hd - (1 - jy), rounded once to f32."""
    M = np.asarray(fr["prev_vp"], np.float64).reshape(4, 4).T
    p = np.concatenate([fr["positions"].reshape(-1, 3).astype(np.float64), np.ones((Wd * Hd, 1))], axis=1)
    clip = p @ M.T
    u, v = (clip[:, 0] / clip[:, 3] + 1.0) / 2.0, (clip[:, 1] / clip[:, 3] + 1.0) / 2.0
    jx, jy = fr["jitter"]
    return np.stack([u * Wd - jx, v * Hd - (1.0 - jy)], axis=-1).astype(F32).reshape(Hd, Wd, 2)


# ---------------------------------------------------------------- content --
def as_plane(v, fmt: int, seed: int = 0) -> np.ndarray:
    """f32 values (Hd, Wd, 3) as a plane in fmt; F16X4 gets a seeded 4th component the call must ignore."""
    v = np.asarray(v, F32)
    if fmt == rn.F32X3:
        return v.copy()
    assert fmt == rn.F16X4
    out = np.empty(v.shape[:-1] + (4,), np.float16)
    out[..., :3] = rn.to_half(v)
    out[..., 3] = np.random.RandomState(seed).uniform(-4, 4, v.shape[:-1]).astype(np.float16)
    return out


def _scatter(a: np.ndarray, specials, stride: int, start: int, column=None) -> None:
    """specials into the flat view of a (or into one column of its last axis), `stride` entries apart."""
    flat = a.reshape(-1) if column is None else a.reshape(-1, a.shape[-1])[:, column]
    assert np.shares_memory(flat, a)
    for k, val in enumerate(specials):
        flat[(stride * k + start) % flat.size] = val


def nasty_content(Wd: int, Hd: int, seed: int) -> dict:
    """current, history (f32 values, (Hd, Wd, 3)), prev_pixel and motion (f32,
    (Hd, Wd, 2)) with everything the rules name: colours that are NaN, +-inf,
    negative, above 1 and beyond half's range; prev_pixel entries that are
    exact integers, sub-pixel shifts, that put ix at -2, -1, Wd - 1 and Wd (and
    iy likewise), and NaN, +-inf and +-1e30; motion vectors of a few pixels
    with the same specials.  No -0, denormal or |value| >= 1e38 colour: a
    product of the colour transforms would not be exact there."""
    rng = np.random.RandomState(seed)
    cur = rng.uniform(-0.25, 1.5, (Hd, Wd, 3)).astype(F32)
    hist = rng.uniform(-0.25, 1.5, (Hd, Wd, 3)).astype(F32)
    colours = (np.nan, np.inf, -np.inf, -3.0, 7.5, 1.0e5, -7.0e4, 65520.0, 1.0e30, 0.0)
    _scatter(cur, colours, 13, 5)
    _scatter(hist, colours[::-1], 11, 2)
    ys, xs = np.mgrid[0:Hd, 0:Wd]
    pp = np.stack([xs, ys], axis=-1).astype(F32)                         # exact integers: "was exactly here"
    shifted = rng.uniform(0, 1, (Hd, Wd)) < 0.7
    pp = np.where(shifted[..., None], pp + rng.uniform(-1.6, 1.6, (Hd, Wd, 2)).astype(F32), pp).astype(F32)
    edge_x = (-1.5, -0.5, Wd - 0.75, Wd + 0.5, -1.0, float(Wd - 1), float(Wd), -2.0)
    edge_y = (-1.5, -0.5, Hd - 0.75, Hd + 0.5, -1.0, float(Hd - 1), float(Hd), -2.0)
    wild = (np.nan, np.inf, -np.inf, 1.0e30, -1.0e30)
    _scatter(pp, edge_x + wild, 5, 1, column=0)
    _scatter(pp, wild + edge_y, 7, 3, column=1)
    mv = rng.uniform(-6, 6, (Hd, Wd, 2)).astype(F32)
    mv[rng.uniform(0, 1, (Hd, Wd)) < 0.2] = 0.0                          # static pixels
    _scatter(mv, wild, 17, 4, column=0)
    _scatter(mv, wild[::-1], 19, 6, column=1)
    return {"current": cur, "history": hist, "prev_pixel": pp, "motion": mv}


def result_plane(v, fmt: int) -> np.ndarray:
    """Rule 7: `result` in its format: the bits of v, or (half)v with 4th component (half)1."""
    v = np.asarray(v, F32)
    if fmt == rn.F32X3:
        return v.copy()
    assert fmt == rn.F16X4
    out = np.empty(v.shape[:-1] + (4,), np.float16)
    out[..., :3] = rn.to_half(v)
    out[..., 3] = np.float16(1)
    return out


def surface_pixels(v, fmt: int, bgr: bool = False, alpha: float = 1.0) -> np.ndarray:
    """Rule 7: the f32 v as dst's pixels (Hd, Wd, bytes per pixel), for resolve_np.place."""
    return rn.encode(v, fmt, bgr, alpha)
