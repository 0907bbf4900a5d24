"""numpy restatement of guided upsampling (bmfr_upsample_output, include/bmfr.h
"Guided upsampling", rules 1-6): every line one np.float32 operation, as the
header writes them.  The guides are decoded by tests/prepare_np.py and the
source value is encoded by tests/resolve_np.py, as the header says.  The GPU
tests hold the kernel to this byte for byte.  TEST INFRASTRUCTURE ONLY.

Guides are a dict with the keys of bmfr_upsample_guides: width, height, albedo,
and for guided mode normals with positions or depth (+ inv_view_proj,
pixel_offset), plane_limit_squared, normal_limit_squared; a plane's format
follows from its dtype as in prepare_np (float32 = F32X3, float16 = F16X4,
uint8 = UNORM8X4, int16 = octahedral snorm16 x 2)."""
from __future__ import annotations

import numpy as np

import prepare_np as pn

F32 = np.float32
GAMMA = F32(0.454545)
# float of the "%g" text of the library's default limits (bmfr_upsample_guides_default)
PLANE_LIMIT, NORMAL_LIMIT = F32(0.01), F32(0.1)


def tone(c) -> np.ndarray:
    """min(max(powr(max(0, c), 0.454545f), 0), 1) with the correctly rounded
    powr: (float)pow in double (NaN and c <= 0 -> 0, c >= 1 -> 1)."""
    c = np.asarray(c, F32)
    with np.errstate(all="ignore"):
        inside = (c > 0) & (c < 1)
        p = np.power(np.where(inside, c, F32(0.5)).astype(np.float64), np.float64(GAMMA)).astype(F32)
        return np.where(c > 0, np.where(c < 1, p, F32(1)), F32(0)).astype(F32)


def axis(n: int, nd: int):
    """Rule 1 along one axis: (first tap, second tap, f) per display coordinate."""
    r = F32(n) / F32(nd)
    u = (np.arange(nd).astype(F32) + F32(0.5)) * r - F32(0.5)
    assert u.dtype == F32
    x0 = np.floor(u)
    f = u - x0
    i0 = x0.astype(np.int64)
    return np.clip(i0, 0, n - 1), np.clip(i0 + 1, 0, n - 1), f


def footprint(W: int, H: int, Wd: int, Hd: int):
    """Rule 1: flat tap indices (4, Hd, Wd) and weights (4, Hd, Wd) in the order 00, 10, 01, 11."""
    xa, xb, fx = axis(W, Wd)
    ya, yb, fy = axis(H, Hd)
    gx, gy = F32(1.0) - fx, F32(1.0) - fy
    taps, weights = [], []
    for ys, wy in ((ya, gy), (yb, fy)):
        for xs, wx in ((xa, gx), (xb, fx)):
            taps.append(ys[:, None] * W + xs[None, :])
            weights.append(wx[None, :] * wy[:, None])
    w = np.stack(weights)
    assert w.dtype == F32
    return np.stack(taps), w


def display_guides(g: dict):
    """Rule 2: (A, N, P) as f32 (Hd, Wd, 3); N and P None in unguided mode."""
    Wd, Hd = g["width"], g["height"]
    A = pn.channels(g["albedo"]).reshape(Hd, Wd, 3)
    if g.get("normals") is None:
        assert g.get("positions") is None and g.get("depth") is None
        return A, None, None
    N = pn.normals_of(g["normals"]).reshape(Hd, Wd, 3)
    if g.get("positions") is not None:
        P = g["positions"].reshape(Hd, Wd, 3)
    else:
        P = pn.position_from_depth(g["depth"], g["inv_view_proj"], g.get("pixel_offset", (0.0, 0.0)), (0, 0, Wd, Hd), Wd,
                                   Hd).reshape(Hd, Wd, 3)
    return A, N.astype(F32), P.astype(F32)


def upsample(acc, W: int, H: int, g: dict, normals=None, positions=None, source: str = "hdr"):
    """Rules 1-6 -> (source values (Hd, Wd, 3) f32, fallback mask (Hd, Wd)).
    acc: filtered_accumulated, f32; normals, positions: the frame's planes,
    f32 or half (widened exactly)."""
    Wd, Hd = g["width"], g["height"]
    acc = np.asarray(acc, F32).reshape(-1, 3)
    taps, w = footprint(W, H, Wd, Hd)
    A, N, P = display_guides(g)
    guided = N is not None
    if guided:
        fn, fp = (np.asarray(p).reshape(-1, 3).astype(F32) for p in (normals, positions))
        pl = F32(g.get("plane_limit_squared", PLANE_LIMIT))
        nl = F32(g.get("normal_limit_squared", NORMAL_LIMIT))
    # -0 + t = t for every t, -0 included: a sum begins with its first term
    sw, tw = np.full((Hd, Wd), -0.0, F32), np.full((Hd, Wd), -0.0, F32)
    sc, tc = np.full((Hd, Wd, 3), -0.0, F32), np.full((Hd, Wd, 3), -0.0, F32)
    with np.errstate(all="ignore"):
        for k in range(4):
            e = acc[taps[k]]
            live = w[k] > 0
            ok = live
            if guided:
                dp = fp[taps[k]] - P
                d = (dp[..., 0] * N[..., 0] + dp[..., 1] * N[..., 1]) + dp[..., 2] * N[..., 2]
                dn = fn[taps[k]] - N
                q = (dn[..., 0] * dn[..., 0] + dn[..., 1] * dn[..., 1]) + dn[..., 2] * dn[..., 2]
                ok = live & (d * d < pl) & (q < nl)
            t = w[k][..., None] * e
            sw = np.where(ok, sw + w[k], sw)
            tw = np.where(live, tw + w[k], tw)
            sc = np.where(ok[..., None], sc + t, sc)
            tc = np.where(live[..., None], tc + t, tc)
        fell = ~(sw > 0)
        den = np.where(fell, tw, sw)
        e = np.where(fell[..., None], tc, sc) / den[..., None]
        c = A * e
    assert c.dtype == F32 and sw.dtype == F32 and sc.dtype == F32
    if not guided:
        assert not fell.any()
    return (tone(c) if source == "tonemapped" else c), fell
