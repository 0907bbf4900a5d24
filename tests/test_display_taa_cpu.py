"""The display-resolution TAA's rules (bmfr_display_taa, include/bmfr.h) on the
CPU: the numpy restatement (tests/display_taa_np.py) against a pixel-by-pixel
scalar transcription of rules 1-7 and against the CPU oracle's oracle_taa, the
properties the header states, the argument checks that need no device, and the
quality condition that makes the feature worth having.

Quality figures (scenes_np rand / far, seed 2, 12 frames, 96x64 -> 192x128:
pyoracle.OracleLoop, then upsample_np.upsample(..., "tonemapped") guided by the
display-resolution planes, then the restatement with blend_alpha 0.2 and a
float64 reprojection of the display positions; mean of the last 4 frames),
measured here with the f32 restatement:

    still camera (the jitter moves)                        rand                      far
    relative L2 from the jitter-averaged noise-free
    tone-mapped display image: upsample -> with TAA        0.1470 -> 0.0387 (0.263)  0.0495 -> 0.0109 (0.220)
    flicker (mean |change| frame to frame)                 0.0658 -> 0.0138 (0.210)  0.0092 -> 0.0016 (0.175)
    relative L2 from each frame's own jittered
    noise-free image (no bar: TAA averages it away)        0.0360 -> 0.1304          0.0068 -> 0.0447
    moving camera
    flicker: upsample -> with TAA                          0.1044 -> 0.0745 (0.714)  0.0126 -> 0.0038 (0.303)

The bars: still-camera distance and flicker <= 0.5 of the un-TAA'd figure,
moving-camera flicker < 1.0 (the feature must never add flicker).
"""
from __future__ import annotations

import functools
import math

import numpy as np
import pytest

import display_taa_np as dn
import pyoracle
import resolve_np as rn
import scenes_np
import upsample_np as un

F32 = np.float32
NOT_SCALED, SCALED = (0, 1, 2, 3), (4, 5, 6, 7, 8, 9)
SIZES = [(1, 1), (2, 1), (5, 3), (9, 7)]
ALPHA = 0.2


def same_bytes(a, b):
    return a.dtype == b.dtype and a.shape == b.shape and a.tobytes() == b.tobytes()


def same_nan_aware(a, b):
    """Equal bytes, any NaN standing for any NaN."""
    nan = np.isnan(b)
    return a.dtype == b.dtype and a.shape == b.shape and (np.isnan(a) == nan).all() and \
        same_bytes(np.where(nan, 0, a).astype(a.dtype), np.where(nan, 0, b).astype(b.dtype))


# ------------------------------------------------- the scalar transcription --
def _min(a, b):
    if a != a:
        return b
    if b != b:
        return a
    if a == b:
        return a if np.signbit(a) else b
    return a if a < b else b


def _max(a, b):
    if a != a:
        return b
    if b != b:
        return a
    if a == b:
        return b if np.signbit(a) else a
    return a if a > b else b


def _dot(c, b):
    """fma(c.z, b.z, fma(c.y, b.y, c.x * b.x)): with power-of-two coefficients the
    products are exact, so each fma is the rounded sum."""
    return F32(F32(F32(c[0] * F32(b[0])) + F32(c[1] * F32(b[1]))) + F32(c[2] * F32(b[2])))


def _ycocg(c):
    return [_dot(c, (1, 2, 1)), _dot(c, (2, 0, -2)), _dot(c, (-1, 2, -1))]


def _rgb(c):
    return [_dot(c, (.25, .25, -.25)), _dot(c, (.25, 0, .25)), _dot(c, (.25, -.25, -.25))]


def _floor(v):
    return F32(math.floor(v)) if np.isfinite(v) else F32(v)


def scalar_taa(current, history, Wd, Hd, blend_alpha, reset, prev_pixel=None, motion=None, motion_scale=(1.0, 1.0),
               at_centre=False, pixel_offset=(0.5, 0.5)):
    """Rules 1-6 of the header, one pixel and one f32 operation at a time -> v (Hd, Wd, 3)."""
    cur = dn.values(current)
    hist = None if history is None else dn.values(history)
    W, H = Wd, Hd
    a = F32(blend_alpha)
    one, half, two = F32(1), F32(0.5), F32(2)
    jx, jy = F32(pixel_offset[0]), F32(pixel_offset[1])
    out = np.empty((H, W, 3), F32)
    with np.errstate(all="ignore"):
        for Y in range(H):
            for X in range(W):
                me = [cur[Y, X, c] for c in range(3)]                                       # 1
                out[Y, X] = me
                if reset or hist is None:
                    continue
                if prev_pixel is not None:                                                  # 2
                    pfx, pfy = F32(prev_pixel[Y, X, 0]), F32(prev_pixel[Y, X, 1])
                else:
                    mx = F32(F32(motion[Y, X, 0]) * F32(motion_scale[0]))
                    my = F32(F32(motion[Y, X, 1]) * F32(motion_scale[1]))
                    if at_centre:
                        pfx = F32(F32(F32(F32(X) + half) - mx) - jx)
                        pfy = F32(F32(F32(F32(Y) + half) - my) - F32(one - jy))
                    else:
                        pfx, pfy = F32(F32(X) - mx), F32(F32(Y) - my)
                flx, fly = _floor(pfx), _floor(pfy)                                         # 3
                if flx < F32(-1) or fly < F32(-1) or flx >= F32(W) or fly >= F32(H):
                    continue
                mnb, mnc = [F32(np.inf)] * 3, [F32(np.inf)] * 3                             # 4
                mxb, mxc = [F32(-np.inf)] * 3, [F32(-np.inf)] * 3
                for dy in (-1, 0, 1):
                    for dx in (-1, 0, 1):
                        sx, sy = X + dx, Y + dy
                        if sx < 0 or sy < 0 or sx >= W or sy >= H:
                            continue
                        s = _ycocg([cur[sy, sx, c] for c in range(3)])
                        for c in range(3):
                            if dx == 0 or dy == 0:
                                mnc[c], mxc[c] = _min(mnc[c], s[c]), _max(mxc[c], s[c])
                            mnb[c], mxb[c] = _min(mnb[c], s[c]), _max(mxb[c], s[c])
                ix = int(_min(_max(flx, F32(-2)), F32(F32(W) + one)))                       # 5
                iy = int(_min(_max(fly, F32(-2)), F32(F32(H) + one)))
                fx, fy = F32(pfx - flx), F32(pfy - fly)
                omx, omy = F32(one - fx), F32(one - fy)
                prev, total = [F32(0)] * 3, F32(0)
                for j in (0, 1):
                    for i in (0, 1):
                        if not ((ix < W - 1 if i else ix >= 0) and (iy < H - 1 if j else iy >= 0)):
                            continue
                        w = F32((fx if i else omx) * (fy if j else omy))
                        for c in range(3):
                            prev[c] = F32(prev[c] + F32(w * hist[max(iy + j, 0), max(ix + i, 0), c]))   # outside only for a NaN pf
                        total = F32(total + w)
                py = _ycocg([F32(p / total) for p in prev])
                cl = []                                                                      # 6
                for c in range(3):
                    lo = F32(F32(mnb[c] + mnc[c]) / two)
                    hi = F32(F32(mxb[c] + mxc[c]) / two)
                    cl.append(_min(_max(py[c], lo), hi))
                pr = _rgb(cl)
                b = F32(one - a)
                out[Y, X] = [F32(F32(a * me[c]) + F32(b * pr[c])) for c in range(3)]
    return out


def _planes(c, cur_fmt, hist_fmt):
    return dn.as_plane(c["current"], cur_fmt, 1), dn.as_plane(c["history"], hist_fmt, 2)


MODES = {"prev_pixel": {}, "motion": dict(at_centre=False, motion_scale=(1.0, -0.5)),
         "motion_centre": dict(at_centre=True, motion_scale=(0.75, 1.0), pixel_offset=(0.3125, 0.8125))}


@pytest.mark.parametrize("mode", list(MODES))
@pytest.mark.parametrize("fmt", ["f32x3", "f16x4"])
@pytest.mark.parametrize("Wd,Hd", SIZES)
def test_restatement_equals_the_rules_pixel_by_pixel(Wd, Hd, fmt, mode):
    c = dn.nasty_content(Wd, Hd, 31 + Wd)
    f = rn.FORMATS[fmt]
    cur, hist = _planes(c, f, f)
    kw = dict(MODES[mode])
    if mode == "prev_pixel":
        kw["prev_pixel"] = c["prev_pixel"]
    else:
        kw["motion"] = c["motion"] if fmt == "f32x3" else rn.to_half(c["motion"])
    pf = dn.previous_position(Wd, Hd, **kw)
    got = dn.display_taa(cur, hist, pf, ALPHA)
    want = scalar_taa(cur, hist, Wd, Hd, ALPHA, False, **kw)
    assert same_nan_aware(got, want)
    # rule 7: result in its format, and the same through reset
    assert same_nan_aware(dn.result_plane(got, f), dn.result_plane(want, f))
    assert same_nan_aware(dn.display_taa(cur, hist, pf, ALPHA, reset=True), scalar_taa(cur, hist, Wd, Hd, ALPHA, True, **kw))


def test_content_holds_what_the_rules_name():
    """The nasty content really reaches every arm: both sides of the off-screen
    test, ix at -2, -1, Wd - 1 and Wd (iy likewise), a tap left out on each
    side, NaN / inf previous positions, and the named colours."""
    Wd, Hd = 9, 7
    c = dn.nasty_content(Wd, Hd, 31 + Wd)
    pp = c["prev_pixel"]
    with np.errstate(all="ignore"):
        fl = np.floor(pp)
        ix = np.fmin(np.fmax(fl[..., 0], F32(-2)), F32(Wd + 1))
        iy = np.fmin(np.fmax(fl[..., 1], F32(-2)), F32(Hd + 1))
    for v, n in ((ix, Wd), (iy, Hd)):
        assert {-2, -1, n - 1, n} <= set(v.reshape(-1).tolist())
    assert np.isnan(pp).any() and np.isposinf(pp).any() and np.isneginf(pp).any()
    assert (pp == F32(1e30)).any() and (pp == F32(-1e30)).any()
    whole = pp == np.floor(pp)
    assert whole.all(axis=-1).any() and (~whole).all(axis=-1).any()
    for k in ("current", "history"):
        p = c[k]
        assert np.isnan(p).any() and np.isposinf(p).any() and np.isneginf(p).any()
        assert (p < 0).any() and (p > 1).any() and (np.abs(p[np.isfinite(p)]) > 65504).any()
        assert not np.signbit(p[p == 0]).any()


# ------------------------------------------------------- against the oracle --
@pytest.mark.parametrize("frame", [0, 3])
@pytest.mark.parametrize("W,H", [(32, 32), (47, 65), (129, 53)])
def test_restatement_equals_the_oracle(W, H, frame):
    """oracle_taa (oracle/bmfr_oracle.c, the reference's kernel in C) on F32X3
    planes: seeded colours, prev_pixel planes with exact integers, sub-pixel
    shifts and far-off entries, every coordinate finite and below 2^30 in
    magnitude (beyond it the oracle's (int) cast is undefined)."""
    rng = np.random.RandomState(W * 131 + H)
    cur = rng.uniform(0, 1, (H, W, 3)).astype(F32)
    hist = rng.uniform(0, 1, (H, W, 3)).astype(F32)
    ys, xs = np.mgrid[0:H, 0:W]
    pp = (np.stack([xs, ys], axis=-1) + rng.uniform(-3, 3, (H, W, 2))).astype(F32)
    whole = rng.uniform(0, 1, (H, W)) < 0.2
    pp[whole] = np.round(pp[whole])
    far = rng.uniform(0, 1, (H, W)) < 0.05
    pp[far] = rng.uniform(-2.0 ** 29, 2.0 ** 29, (int(far.sum()), 2)).astype(F32)
    assert np.isfinite(pp).all() and (np.abs(pp) < 2.0 ** 30).all()
    cfg = pyoracle.make_cfg(W, H, NOT_SCALED, SCALED, 1, taa_blend_alpha=ALPHA)
    want = np.full((H, W, 3), np.nan, F32)
    pyoracle.load().oracle_taa(cfg, pyoracle._p(pp), pyoracle._p(cur), pyoracle._p(want), pyoracle._p(hist), frame)
    got = dn.display_taa(cur, hist, pp, F32(cfg.taa_blend_alpha), reset=frame == 0)
    assert same_bytes(got, want)
    if frame:
        assert not same_bytes(got, cur)


# --------------------------------------------------------------- properties --
@pytest.mark.parametrize("fmt", ["f32x3", "f16x4"])
def test_reset_and_no_history_pass_current_through_bit_for_bit(fmt):
    Wd, Hd = 9, 7
    c = dn.nasty_content(Wd, Hd, 5)
    f = rn.FORMATS[fmt]
    cur, hist = _planes(c, f, f)
    assert np.isnan(cur).any()
    for kw in (dict(history=hist, reset=True), dict(history=None)):
        v = dn.display_taa(cur, kw["history"], c["prev_pixel"], ALPHA, reset=kw.get("reset", False))
        assert same_bytes(v, np.ascontiguousarray(dn.values(cur)))            # a NaN's bits included
        if f == rn.F16X4:   # values that were halves round back to themselves
            assert same_bytes(dn.result_plane(v, f)[..., :3], np.ascontiguousarray(cur[..., :3]))


def test_a_nan_in_history_does_not_survive_a_finite_neighbourhood():
    Wd, Hd = 9, 7
    rng = np.random.RandomState(9)
    cur = rng.uniform(0, 1, (Hd, Wd, 3)).astype(F32)
    hist = rng.uniform(0, 1, (Hd, Wd, 3)).astype(F32)
    hist[2:5, 3:6] = np.nan
    hist[0, 0] = np.inf
    ys, xs = np.mgrid[0:Hd, 0:Wd]
    pp = np.stack([xs, ys], axis=-1).astype(F32)        # exact integers: three taps of weight 0, one of them NaN
    v = dn.display_taa(cur, hist, pp, ALPHA)
    assert np.isfinite(v).all()
    # the NaN history became lo: the clamp's lower corner, not the pixel's own colour
    assert not same_bytes(v[3, 4], cur[3, 4])
    pp = pp + F32(0.25)
    assert np.isfinite(dn.display_taa(cur, hist, pp, ALPHA)).all()


def test_blend_alpha_one_returns_current():
    Wd, Hd = 9, 7
    rng = np.random.RandomState(10)
    cur = rng.uniform(0.01, 1, (Hd, Wd, 3)).astype(F32)
    hist = rng.uniform(0, 1, (Hd, Wd, 3)).astype(F32)
    ys, xs = np.mgrid[0:Hd, 0:Wd]
    pp = (np.stack([xs, ys], axis=-1) + rng.uniform(-1, 1, (Hd, Wd, 2))).astype(F32)
    assert same_bytes(dn.display_taa(cur, hist, pp, 1.0), cur)
    assert not same_bytes(dn.display_taa(cur, hist, pp, 0.5), cur)


def test_dst_takes_the_f32_value_not_the_half_rounded_one():
    """0.4999 * 255 + 0.5 = 127.97 quantises to 127; (half)0.4999 = 0.5 quantises
    to 128.  With an F16X4 result the surface must still come from the f32 v."""
    v = np.array([[[0.4999, 0.50195, 0.2]]], F32)
    assert rn.quantise(v)[0, 0, 0] == 127 and rn.quantise(rn.to_half(v).astype(F32))[0, 0, 0] == 128
    out = dn.display_taa(v, None, None, ALPHA)
    rounded = dn.values(dn.result_plane(out, rn.F16X4))
    assert same_bytes(dn.surface_pixels(out, rn.UNORM8X4), rn.encode(v, rn.UNORM8X4))
    assert not same_bytes(dn.surface_pixels(rounded, rn.UNORM8X4), rn.encode(v, rn.UNORM8X4))


# ---------------------------------------------------- the quality condition --
W, H, WD, HD = 96, 64, 192, 128
SEED, FRAMES, LAST = 2, 12, 4


def _clean(scene, f, still):
    """The noise-free tone-mapped display image of frame f: display albedo x
    the scene's irradiance (scenes_np._render's one point light) at the
    display-resolution positions and normals, float64, then the tone map."""
    fr = scenes_np.frame(scene, WD, HD, f, SEED, still=still)
    eye = scenes_np.camera(scene, WD, HD, 0 if still else f, SEED)[0]
    pos, nrm = (fr[k].reshape(-1, 3).astype(np.float64) for k in ("positions", "normals"))
    l = eye + np.array([1.5, 2.5, 1.0]) - pos
    d2 = (l * l).sum(axis=-1)
    cosv = np.maximum((nrm * l).sum(axis=-1) / np.sqrt(d2), 0.0)
    irr = (0.25 + 3.0 * cosv / (1.0 + 0.05 * d2))[:, None] * np.array([1.0, 0.95, 0.85])
    c = fr["albedo"].reshape(-1, 3).astype(np.float64) * irr
    return np.clip(np.power(np.maximum(c, 0.0), float(un.GAMMA)), 0.0, 1.0).reshape(HD, WD, 3)


@functools.lru_cache(maxsize=None)
def sequence(scene: str, still: bool):
    """Per frame: (the tone-mapped guided upsample, the same through the TAA)."""
    cfg = pyoracle.make_cfg(W, H, NOT_SCALED, SCALED, 1)
    recs = scenes_np.run_loop(pyoracle.OracleLoop(cfg), scene, W, H, FRAMES, SEED, still=still)
    plain, taa, history = [], [], None
    for f in range(FRAMES):
        low = scenes_np.frame(scene, W, H, f, SEED, still=still)
        disp = scenes_np.frame(scene, WD, HD, f, SEED, still=still)
        g = {"width": WD, "height": HD, "albedo": disp["albedo"], "normals": disp["normals"],
             "positions": disp["positions"]}
        cur, _ = un.upsample(recs[f]["acc"].astype(F32), W, H, g, low["normals"], low["positions"], "tonemapped")
        history = dn.display_taa(cur, history, dn.display_prev_pixel(disp, WD, HD), ALPHA, reset=f == 0)
        plain.append(cur)
        taa.append(history)
    return plain, taa


def _rel_l2(a, ref) -> float:
    a = a.astype(np.float64)
    return float(np.sqrt(((a - ref) ** 2).sum() / (ref ** 2).sum()))


def _flicker(seq) -> float:
    return float(np.mean([np.abs(seq[f].astype(np.float64) - seq[f - 1]).mean() for f in range(FRAMES - LAST, FRAMES)]))


@pytest.mark.parametrize("scene", ["rand", "far"])
def test_display_taa_converges_on_the_jitter_averaged_image_and_stops_the_crawl(scene):
    plain, taa = sequence(scene, True)
    clean = [_clean(scene, f, True) for f in range(FRAMES)]
    mean = np.mean(clean, axis=0)
    last = range(FRAMES - LAST, FRAMES)
    d_plain, d_taa = (float(np.mean([_rel_l2(s[f], mean) for f in last])) for s in (plain, taa))
    o_plain, o_taa = (float(np.mean([_rel_l2(s[f], clean[f]) for f in last])) for s in (plain, taa))
    f_plain, f_taa = _flicker(plain), _flicker(taa)
    print(f"{scene} still: distance from the jitter-averaged image {d_plain:.4f} -> {d_taa:.4f} ({d_taa / d_plain:.3f}), "
          f"flicker {f_plain:.4f} -> {f_taa:.4f} ({f_taa / f_plain:.3f}), "
          f"distance from each frame's own jittered image {o_plain:.4f} -> {o_taa:.4f} (no bar)")
    assert d_taa <= 0.5 * d_plain
    assert f_taa <= 0.5 * f_plain


@pytest.mark.parametrize("scene", ["rand", "far"])
def test_display_taa_never_adds_flicker_under_a_moving_camera(scene):
    plain, taa = sequence(scene, False)
    f_plain, f_taa = _flicker(plain), _flicker(taa)
    print(f"{scene} moving: flicker {f_plain:.4f} -> {f_taa:.4f} ({f_taa / f_plain:.3f})")
    assert f_taa < 1.0 * f_plain


# ------------------------------------------------- errors without a context --
def test_arguments_are_checked_without_a_context():
    """The header's error list in its order, through _lib with plausible aligned
    addresses: every answer that needs neither a context nor a device; with all
    in order the NULL context is what is left to refuse."""
    import ctypes as C
    import bmfr_amd
    from bmfr_amd import _lib
    lib = _lib.load()
    P, Q, R = 0x1000, 0x200000, 0x400000   # plausible aligned device addresses: nothing is dereferenced
    Wd, Hd = 64, 48

    def call(null_args=False, dst=True, **edit):
        a, s = _lib.DisplayTaaArgs(), _lib.Surface()
        lib.bmfr_display_taa_default(C.byref(a), None)
        lib.bmfr_surface_default(C.byref(s))
        a.width, a.height = Wd, Hd
        a.current = _lib.Plane(P, _lib.FORMAT_F16X4, Wd * 8)
        a.history = _lib.Plane(Q, _lib.FORMAT_F32X3, Wd * 12 + 4)
        a.result = _lib.Plane(R, _lib.FORMAT_F16X4, Wd * 8 + 8)
        a.motion, a.motion_format = P, _lib.FORMAT_F16X2
        s.data, s.format, s.pitch, s.width, s.height = P, _lib.FORMAT_UNORM8X4, Wd * 4, Wd, Hd
        for k, v in edit.items():
            if k.startswith("dst_"):
                setattr(s, k[4:], v)
            elif "_" in k and k.split("_", 1)[0] in ("current", "history", "result"):
                plane, field = k.split("_", 1)
                setattr(getattr(a, plane), field, v)
            else:
                setattr(a, k, v)
        return lib.bmfr_display_taa(None, None, None if null_args else C.byref(a), C.byref(s) if dst else None)

    a = _lib.DisplayTaaArgs()
    a.width, a.reset = 5, 1
    lib.bmfr_display_taa_default(C.byref(a), None)
    assert a.width == 0 and a.reset == 0 and not a.current.data and not a.prev_pixel
    assert F32(a.blend_alpha) == F32(0.2) and list(a.motion_scale) == [1.0, 1.0]
    cfg = bmfr_amd.BmfrConfig(image_width=64, image_height=64).to_c()
    cfg.taa_blend_alpha = 0.05
    lib.bmfr_display_taa_default(C.byref(a), C.byref(cfg))
    assert F32(a.blend_alpha) == F32(0.05)

    INVALID, UNSUPPORTED = 1, 2
    assert call() == INVALID and call(dst=False) == INVALID                  # all in order: the NULL context
    # dst first, as bmfr_resolve_output checks it -- also when the arguments are wrong too
    assert call(dst_format=9) == UNSUPPORTED and call(dst_format=9, null_args=True) == UNSUPPORTED
    assert call(dst_data=None) == INVALID and call(dst_pitch=Wd * 4 - 4) == INVALID and call(dst_pitch=Wd * 4 + 2) == INVALID
    assert call(null_args=True, dst=False) == INVALID
    # an unsupported format stands out from the invalid arguments checked before it
    assert call(width=0, current_format=9) == INVALID and call(height=-1, result_format=9) == INVALID
    assert call(current_data=None, current_format=9) == INVALID and call(result_data=None, current_format=9) == INVALID
    for plane in ("current", "history", "result"):
        assert call(**{plane + "_format": _lib.FORMAT_UNORM8X4}) == UNSUPPORTED, plane
        assert call(**{plane + "_format": _lib.FORMAT_NONE}) == UNSUPPORTED, plane
    assert call(history_data=None, history_format=9, history_pitch=1) == INVALID   # a NULL plane is not looked at
    for bad in (dict(current_pitch=Wd * 8 - 8), dict(current_pitch=Wd * 8 + 4), dict(current_data=P + 4),
                dict(history_pitch=Wd * 12 - 4), dict(history_pitch=Wd * 12 + 2), dict(history_data=Q + 2),
                dict(result_pitch=Wd * 8 - 8), dict(result_pitch=Wd * 8 + 12), dict(result_data=R + 4),
                dict(current_pitch=(1 << 31) + 8), dict(history_pitch=(1 << 31) + 4),               # above 2^31
                dict(current_format=_lib.FORMAT_F32X3), dict(result_format=_lib.FORMAT_F32X3)):    # 8 B/px pitches are too small for 12
        assert call(**bad) == INVALID, bad
    # an unsupported motion format stands out from a pitch checked before it and from what comes after
    assert call(result_pitch=8, motion_format=9) == INVALID
    assert call(motion_format=9) == UNSUPPORTED and call(motion_format=_lib.FORMAT_F32X3) == UNSUPPORTED
    assert call(motion_format=9, blend_alpha=float("nan")) == UNSUPPORTED
    for bad in (dict(prev_pixel=P), dict(motion=None), dict(motion=P + 2), dict(motion=None, prev_pixel=P + 2)):
        assert call(**bad) == INVALID, bad
    # without history neither is needed or looked at: what is left is the NULL context
    for free in (dict(reset=1), dict(history_data=None)):
        for kw in (dict(motion=None), dict(prev_pixel=P), dict(motion=P + 2, motion_format=9)):
            assert call(**free, **kw) == INVALID
            assert call(**free, **kw, blend_alpha=0.5, dst=False) == INVALID
    for bad in (dict(result_data=P), dict(result_data=Q, result_format=_lib.FORMAT_F32X3, result_pitch=Wd * 12),
                dict(blend_alpha=float("nan")), dict(blend_alpha=float("inf")),
                dict(dst_width=Wd - 1), dict(dst_height=Hd - 1), dict(dst_origin_x=1), dict(dst_origin_y=-1),
                dict(dst_origin_y=1, dst_flip_y=1)):
        assert call(**bad) == INVALID, bad
