"""Guided upsampling's rules (bmfr_upsample_output, include/bmfr.h) on the CPU:
the numpy restatement (tests/upsample_np.py) against a pixel-by-pixel scalar
transcription of rules 1-6, the properties the header states, and the quality
condition on the CPU oracle that makes the feature worth having.

Quality figures (pyoracle.OracleLoop, seed 2, 8 frames, default feature lists,
half tmp_data, the library's default limits 0.01 / 0.1; relative L2 distance of
the last frame from display albedo x the scene's irradiance at the
display-resolution positions and normals), measured here with the f32
restatement:

    scene  low -> display        stretched  unguided  guided  g / s  g / u  fallback
    rand    96x64  -> 192x128    0.2557     0.0865    0.0504  0.197  0.583  0.053 %
    rand   128x80  -> 256x160    0.2338     0.0921    0.0579  0.248  0.628  0.017 %
    rand   128x80  -> 192x120    0.2293     0.0898    0.0590  0.257  0.657  0.022 %
    rand    96x64  -> 288x192    0.2829     0.0956    0.0679  0.240  0.710  0.548 %
    far     96x64  -> 192x128    0.1690     0.0255    0.0255  0.151  1      0
    far    128x80  -> 256x160    0.1504     0.0274    0.0274  0.182  1      0
    far    128x80  -> 192x120    0.1443     0.0275    0.0275  0.191  1      0
    far     96x64  -> 288x192    0.1874     0.0252    0.0252  0.135  1      0

On far (one plane) guided equals unguided byte for byte.  The bars are guided <= 0.5 stretched (both scenes), and on rand guided <= 0.85
unguided and fallback <= 2 %.
"""
from __future__ import annotations

import functools
import math

import numpy as np
import pytest

import prepare_np as pn
import pyoracle
import resolve_np as rn
import scenes_np
import upsample_np as un

F32 = np.float32
NOT_SCALED, SCALED = (0, 1, 2, 3), (4, 5, 6, 7, 8, 9)
CASES = [(5, 3, 7, 5), (2, 1, 8, 4), (1, 1, 1, 1), (9, 7, 9, 7)]
PAIRS = [(96, 64, 192, 128), (128, 80, 256, 160), (128, 80, 192, 120), (96, 64, 288, 192)]
SEED, FRAMES = 2, 8


def same_bytes(a, b):
    return a.dtype == b.dtype and a.shape == b.shape and a.tobytes() == b.tobytes()


def same_nan_aware(a, b):
    nan = np.isnan(b)
    return a.shape == b.shape and (np.isnan(a) == nan).all() and same_bytes(np.where(nan, 0, a).astype(F32),
                                                                            np.where(nan, 0, b).astype(F32))


# ------------------------------------------------------------------ content --
NORMALS = np.array([[0.0, 0.0, 1.0], [0.6, 0.0, 0.8], [0.0, -0.8, 0.6], [0.0, 0.0, 1.0]])
DEPTHS = np.array([1.0, 1.0, 1.7, 1.7])


def geometry(w: int, h: int):
    """Four surfaces over the unit square, sampled at pixel centres: normals and
    positions (h * w, 3) f32.  Surfaces 0 / 3 share a normal and differ by a
    plane step; 0 / 1 share the depth and differ by the normal."""
    ys, xs = np.mgrid[0:h, 0:w]
    u, v = (xs + 0.5) / w, (ys + 0.5) / h
    sid = (u > 0.45).astype(int) + 2 * (v > 0.55).astype(int)
    n = NORMALS[sid]
    # on the surface's plane through (0.5, 0.5, depth): n . (p - p0) = 0
    z = DEPTHS[sid] - (n[..., 0] * (u - 0.5) + n[..., 1] * (v - 0.5)) / n[..., 2]
    p = np.stack([u, v, z], axis=-1)
    return n.reshape(-1, 3).astype(F32), p.reshape(-1, 3).astype(F32)


def content(W, H, Wd, Hd, seed, guided=True, packed=False, half=False, nasty=True):
    """(acc, guides, frame normals, frame positions).  packed: UNORM8X4 albedo,
    octahedral normals and depth instead of f32 planes.  nasty: NaN, +-inf and
    -0 in acc, NaN in some guides and frame planes."""
    rng = np.random.RandomState(seed)
    acc = rng.uniform(0.0, 2.0, (W * H, 3)).astype(F32)
    fn, fp = geometry(W, H)
    N, P = geometry(Wd, Hd)
    alb = rng.uniform(0.0, 1.0, (Wd * Hd, 3)).astype(F32)
    if nasty:
        flat = acc.reshape(-1)
        for i, val in enumerate((np.nan, np.inf, -np.inf, -0.0, 1e5, 3.0e38)):
            flat[(7 * i + 3) % flat.size] = val
        if W * H > 4:
            fn[(W * H) // 3, 1] = np.nan
            fp[(W * H) // 2, 2] = np.nan
        if Wd * Hd > 4:
            N[(Wd * Hd) // 5] = np.nan
            P[(Wd * Hd) // 7, 0] = np.nan
            alb[(Wd * Hd) // 6, 2] = np.nan
    g = {"width": Wd, "height": Hd}
    if packed:
        g["albedo"] = pn.unorm8(alb, rng)
    else:
        g["albedo"] = alb.reshape(-1)
    if guided:
        if packed:   # a NaN normal has no octahedral code: the NaN guides are depths here
            g["normals"] = pn.oct_encode(np.where(np.isnan(N).any(axis=-1, keepdims=True), NORMALS[0], N)).reshape(-1)
            vp = scenes_np.view_projection("far", Wd, Hd, 0, 1)
            vp = tuple(float(F32(vp[r, c])) for c in range(4) for r in range(4))
            bad = np.isnan(P).any(axis=-1)
            g["depth"], g["inv_view_proj"] = pn.depth_and_inverse(np.nan_to_num(P) + F32(14.0), vp)
            g["depth"][bad] = np.nan
            g["pixel_offset"] = (0.25, 0.75)
        else:
            g["normals"], g["positions"] = N.reshape(-1), P.reshape(-1)
    if half:
        fn, fp = fn.astype(np.float16), fp.astype(np.float16)
    return acc, g, fn.reshape(-1), fp.reshape(-1)


# ------------------------------------------------- the scalar transcription --
def scalar_upsample(acc, W, H, g, normals, positions, source):
    """Rules 1-6 of the header, one pixel and one f32 operation at a time
    (the guides decoded by the decoders the header names)."""
    Wd, Hd = g["width"], g["height"]
    A, N, P = un.display_guides(g)
    guided = N is not None
    acc = acc.reshape(H, W, 3)
    if guided:
        fn = np.asarray(normals).reshape(H, W, 3).astype(F32)
        fp = np.asarray(positions).reshape(H, W, 3).astype(F32)
        pl = F32(g.get("plane_limit_squared", un.PLANE_LIMIT))
        nl = F32(g.get("normal_limit_squared", un.NORMAL_LIMIT))
    half, one = F32(0.5), F32(1.0)
    rx, ry = F32(W) / F32(Wd), F32(H) / F32(Hd)
    out = np.empty((Hd, Wd, 3), F32)
    fell = np.zeros((Hd, Wd), bool)

    def total(terms):
        s = terms[0]
        for t in terms[1:]:
            s = F32(s + t)
        return s

    with np.errstate(all="ignore"):
        for Y in range(Hd):
            for X in range(Wd):
                u, v = F32(F32(F32(X) + half) * rx) - half, F32(F32(F32(Y) + half) * ry) - half
                x0, y0 = F32(math.floor(u)), F32(math.floor(v))
                fx, fy = F32(u - x0), F32(v - y0)
                taps = []
                for j in (0, 1):
                    for i in (0, 1):
                        x = min(max(int(x0) + i, 0), W - 1)
                        y = min(max(int(y0) + j, 0), H - 1)
                        w = F32((fx if i else F32(one - fx)) * (fy if j else F32(one - fy)))
                        taps.append((x, y, w))
                live = [t for t in taps if t[2] > 0]
                used = live
                if guided:
                    n_, p_ = N[Y, X], P[Y, X]
                    used = []
                    for x, y, w in live:
                        dp = [F32(fp[y, x, c] - p_[c]) for c in range(3)]
                        d = F32(F32(F32(dp[0] * n_[0]) + F32(dp[1] * n_[1])) + F32(dp[2] * n_[2]))
                        dn = [F32(fn[y, x, c] - n_[c]) for c in range(3)]
                        q = F32(F32(F32(dn[0] * dn[0]) + F32(dn[1] * dn[1])) + F32(dn[2] * dn[2]))
                        if F32(d * d) < pl and q < nl:
                            used.append((x, y, w))
                    if not used:
                        used, fell[Y, X] = live, True
                sw = total([w for _, _, w in used])
                for c in range(3):
                    sc = total([F32(w * acc[y, x, c]) for x, y, w in used])
                    val = F32(A[Y, X, c] * F32(sc / sw))
                    if source == "tonemapped":
                        val = F32(0.0) if not val > 0 else (F32(1.0) if not val < 1 else
                                                            F32(math.pow(float(val), float(un.GAMMA))))
                    out[Y, X, c] = val
    return out, fell


@pytest.mark.parametrize("source", ["hdr", "tonemapped"])
@pytest.mark.parametrize("mode", ["guided", "packed", "half", "unguided"])
@pytest.mark.parametrize("W,H,Wd,Hd", CASES)
def test_restatement_equals_the_rules_pixel_by_pixel(W, H, Wd, Hd, mode, source):
    acc, g, fn, fp = content(W, H, Wd, Hd, 11 + W, guided=mode != "unguided", packed=mode == "packed",
                             half=mode == "half")
    got, fell = un.upsample(acc, W, H, g, fn, fp, source)
    want, counted = scalar_upsample(acc, W, H, g, fn, fp, source)
    assert same_nan_aware(got, want)
    assert (fell == counted).all()
    if mode == "unguided":
        assert not fell.any()


# --------------------------------------------------------------- properties --
@pytest.mark.parametrize("half", [False, True], ids=["f32", "half"])
def test_identity_at_ratio_one_is_the_hdr_resolve(half):
    """Wd = W, Hd = H, the frame's own planes and albedo as guides: u = X
    exactly, the weights are (1, 0, 0, 0), and HDR is resolve_np.hdr byte for
    byte -- also where a weight-0 neighbour is NaN or +-inf (the constructed
    image holds all of them, and -0)."""
    W, H = 37, 23
    _, w = un.footprint(W, H, W, H)
    assert (w[0] == 1).all() and (w[1:] == 0).all()
    acc = rn.constructed_image(4200 + W * H, 5)[4200:]    # the part with the specials and half's range
    assert np.isnan(acc).any() and np.isinf(acc).any() and np.signbit(acc[acc == 0]).any()
    fn, fp = geometry(W, H)
    alb = np.random.RandomState(3).uniform(-0.25, 1.5, (W * H, 3)).astype(F32)
    dt = np.float16 if half else F32
    fn, fp, alb = fn.astype(dt), fp.astype(dt), alb.astype(dt)
    g = {"width": W, "height": H, "albedo": alb.astype(F32).reshape(-1), "normals": fn.astype(F32).reshape(-1),
         "positions": fp.astype(F32).reshape(-1)}
    got, fell = un.upsample(acc, W, H, g, fn, fp)
    assert not fell.any()
    assert same_nan_aware(got.reshape(-1, 3), rn.hdr(alb, acc))
    unguided, _ = un.upsample(acc, W, H, {"width": W, "height": H, "albedo": g["albedo"]})
    assert same_nan_aware(unguided.reshape(-1, 3), rn.hdr(alb, acc))


def _two_by_one(left, right, n_right=(0.0, 0.0, 1.0), z_right=1.0):
    """A 2 x 1 frame -> 8 x 1: acc = left | right; the right pixel on its own
    surface.  The display guides are the left surface everywhere."""
    acc = np.array([left, right], F32)
    fn = np.array([[0, 0, 1], n_right], F32)
    fp = np.array([[0.25, 0.5, 1.0], [0.75, 0.5, z_right]], F32)
    N = np.tile(np.array([0, 0, 1], F32), 8)
    P = np.stack([(np.arange(8) + 0.5) / 8, np.full(8, 0.5), np.ones(8)], axis=-1).astype(F32).reshape(-1)
    g = {"width": 8, "height": 1, "albedo": np.ones(24, F32), "normals": N, "positions": P}
    return acc, g, fn.reshape(-1), fp.reshape(-1)


@pytest.mark.parametrize("kind", ["normal edge", "plane step"])
def test_a_tap_across_an_edge_contributes_nothing(kind):
    left, right = (1.0, 2.0, 3.0), (100.0, 200.0, 300.0)
    if kind == "normal edge":
        acc, g, fn, fp = _two_by_one(left, right, n_right=(0.6, 0.0, 0.8))    # |dn|^2 = 0.2 > 0.1
    else:
        acc, g, fn, fp = _two_by_one(left, right, z_right=1.2)               # d^2 = 0.04 > 0.01
    out, fell = un.upsample(acc, 2, 1, g, fn, fp)
    # display pixels 0-5 have the left pixel among their taps; 6 and 7 see the right one alone
    assert not fell[0, :6].any() and fell[0, 6:].all()
    assert same_bytes(out.reshape(8, 3)[:6], np.tile(np.array(left, F32), (6, 1)))
    free, _ = un.upsample(acc, 2, 1, {k: g[k] for k in ("width", "height", "albedo")})
    assert (free.reshape(8, 3)[2:6] != out.reshape(8, 3)[2:6]).all()          # the stretch does cross the edge


def test_a_pixel_all_of_whose_taps_fail_takes_the_unguided_value_and_is_counted():
    acc, g, fn, fp = _two_by_one((1.0, 2.0, 3.0), (5.0, 6.0, 7.0), z_right=1.2)
    fp = fp.copy()
    fp[2] = 1.2                                                             # the left pixel leaves the plane too
    out, fell = un.upsample(acc, 2, 1, g, fn, fp)
    free, none = un.upsample(acc, 2, 1, {k: g[k] for k in ("width", "height", "albedo")})
    assert fell.all() and not none.any()
    assert same_bytes(out, free)


@pytest.mark.parametrize("plane", ["normals", "positions"])
def test_nan_guides_fall_back_and_never_make_a_nan(plane):
    W, H, Wd, Hd = 9, 7, 18, 14
    acc, g, fn, fp = content(W, H, Wd, Hd, 4, nasty=False)
    g[plane] = g[plane].copy()
    g[plane].reshape(Hd, Wd, 3)[3:6, 4:9, 1] = np.nan
    out, fell = un.upsample(acc, W, H, g, fn, fp)
    free, _ = un.upsample(acc, W, H, {k: g[k] for k in ("width", "height", "albedo")})
    assert fell[3:6, 4:9].all()
    assert np.isfinite(out).all()
    assert same_bytes(out[3:6, 4:9], free[3:6, 4:9])


def test_zero_weight_taps_are_never_read_into_a_sum():
    """3 x 3 at ratio 1, every pixel NaN but the centre: the centre's three
    weight-0 taps are NaN and do not reach it."""
    acc = np.full((9, 3), np.nan, F32)
    acc[4] = (1.0, 2.0, 3.0)
    g = {"width": 3, "height": 3, "albedo": np.ones(27, F32)}
    out, _ = un.upsample(acc, 3, 3, g)
    assert same_bytes(out[1, 1], np.array([1.0, 2.0, 3.0], F32))
    assert np.isnan(out[0, 0]).all()


# ---------------------------------------------------- the quality condition --
@functools.lru_cache(maxsize=None)
def low_frames(scene: str, W: int, H: int):
    """The oracle's filtered_accumulated of the last frame, with that frame's planes."""
    cfg = pyoracle.make_cfg(W, H, NOT_SCALED, SCALED, 1)
    recs = scenes_np.run_loop(pyoracle.OracleLoop(cfg), scene, W, H, FRAMES, SEED)
    return recs[-1]["acc"].astype(F32), scenes_np.frame(scene, W, H, FRAMES - 1, SEED)


def clean_image(scene: str, Wd: int, Hd: int, fr: dict) -> np.ndarray:
    """Display albedo x the scene's irradiance (scenes_np._render's one point
    light) at the display-resolution positions and normals, float64."""
    eye = scenes_np.camera(scene, Wd, Hd, FRAMES - 1, SEED)[0]
    pos, nrm = (fr[k].reshape(-1, 3).astype(np.float64) for k in ("positions", "normals"))
    l = eye + np.array([1.5, 2.5, 1.0]) - pos
    d2 = (l * l).sum(axis=-1)
    cosv = np.maximum((nrm * l).sum(axis=-1) / np.sqrt(d2), 0.0)
    irr = (0.25 + 3.0 * cosv / (1.0 + 0.05 * d2))[:, None] * np.array([1.0, 0.95, 0.85])
    return fr["albedo"].reshape(-1, 3).astype(np.float64) * irr


def rel_l2(a, ref) -> float:
    a = a.reshape(ref.shape).astype(np.float64)
    return float(np.sqrt(((a - ref) ** 2).sum() / (ref ** 2).sum()))


@functools.lru_cache(maxsize=None)
def quality(scene: str, W: int, H: int, Wd: int, Hd: int):
    """(stretched, unguided, guided, fallback share, guided == unguided byte for byte)."""
    acc, low = low_frames(scene, W, H)
    disp = scenes_np.frame(scene, Wd, Hd, FRAMES - 1, SEED)
    clean = clean_image(scene, Wd, Hd, disp)
    plain = {"width": Wd, "height": Hd, "albedo": disp["albedo"]}
    g = dict(plain, normals=disp["normals"], positions=disp["positions"])
    guided, fell = un.upsample(acc, W, H, g, low["normals"], low["positions"])
    unguided, _ = un.upsample(acc, W, H, plain)
    stretched, _ = un.upsample(rn.hdr(low["albedo"].reshape(-1, 3), acc.reshape(-1, 3)), W, H,
                               dict(plain, albedo=np.ones(Wd * Hd * 3, F32)))
    return (rel_l2(stretched, clean), rel_l2(unguided, clean), rel_l2(guided, clean), float(fell.mean()),
            same_bytes(guided, unguided))


@pytest.mark.parametrize("W,H,Wd,Hd", PAIRS)
@pytest.mark.parametrize("scene", ["rand", "far"])
def test_guided_upsampling_beats_stretching_the_remodulated_frame(scene, W, H, Wd, Hd):
    stretched, unguided, guided, share, same = quality(scene, W, H, Wd, Hd)
    print(f"{scene} {W}x{H} -> {Wd}x{Hd}: stretched {stretched:.4f}, unguided {unguided:.4f}, guided {guided:.4f}, "
          f"guided / stretched {guided / stretched:.3f}, guided / unguided {guided / unguided:.3f}, "
          f"fallback {100 * share:.3f} %")
    assert guided <= 0.5 * stretched
    if scene == "rand":
        assert guided <= 0.85 * unguided
        assert share <= 0.02
    else:
        assert same and share == 0


# ------------------------------------------------- errors without a context --
def test_arguments_are_checked_without_a_context():
    """dst first, then source and the guides: every answer that needs neither a
    context nor a device (include/bmfr.h "Errors"); with all of them in order
    the NULL context is what is left to refuse."""
    import ctypes as C
    import bmfr_amd
    from bmfr_amd import _lib
    lib = _lib.load()
    P = 0x1000   # a plausible aligned device address: nothing is dereferenced

    def call(source=0, frame_normals=P, frame_positions=P, stats=None, null_guides=False, null_dst=False, **edit):
        g, s = _lib.UpsampleGuides(), _lib.Surface()
        lib.bmfr_upsample_guides_default(C.byref(g), None)
        lib.bmfr_surface_default(C.byref(s))
        g.width, g.height, g.albedo, g.albedo_format = 64, 64, P, _lib.FORMAT_UNORM8X4
        g.normals, g.normal_format, g.depth = P, _lib.FORMAT_OCT_SNORM16X2, P
        s.data, s.format, s.pitch, s.width, s.height = P, _lib.FORMAT_UNORM8X4, 256, 64, 64
        for k, v in edit.items():
            setattr(s if k.startswith("dst_") else g, k[4:] if k.startswith("dst_") else k, v)
        return lib.bmfr_upsample_output(None, None, source, frame_normals, frame_positions, None if null_guides else C.byref(g),
                                        None if null_dst else C.byref(s), stats)

    g = _lib.UpsampleGuides()
    g.width = 5
    lib.bmfr_upsample_guides_default(C.byref(g), C.byref(bmfr_amd.BmfrConfig(image_width=64, image_height=64).to_c()))
    assert g.width == 0 and not g.albedo
    assert F32(g.plane_limit_squared) == un.PLANE_LIMIT and F32(g.normal_limit_squared) == un.NORMAL_LIMIT
    cfg = bmfr_amd.BmfrConfig(image_width=64, image_height=64).to_c()
    cfg.position_limit_squared, cfg.normal_limit_squared = 0.0123456789, 1.0 / 3.0
    lib.bmfr_upsample_guides_default(C.byref(g), C.byref(cfg))
    assert F32(g.plane_limit_squared) == F32(float("%g" % 0.0123456789))
    assert F32(g.normal_limit_squared) == F32(float("%g" % (1.0 / 3.0)))

    assert call() == 1                                      # all in order: the NULL context
    assert call(dst_format=9) == 2 and call(dst_format=9, albedo=None) == 2 and call(null_dst=True) == 1
    for bad in (dict(source=2), dict(null_guides=True), dict(albedo=None), dict(normals=None), dict(frame_normals=None), dict(frame_positions=None),
                dict(width=0), dict(depth=None), dict(normals=None, depth=None, positions=P),
                dict(plane_limit_squared=0.0), dict(normal_limit_squared=float("nan")),
                dict(plane_limit_squared=float("inf")), dict(albedo=P + 2), dict(depth=P + 1), dict(stats=P + 2),
                dict(albedo_format=_lib.FORMAT_F16X4, albedo=P + 4)):
        assert call(**bad) == 1, bad
    for bad in (dict(albedo_format=_lib.FORMAT_OCT_SNORM16X2), dict(normal_format=_lib.FORMAT_UNORM8X4),
                dict(albedo_format=_lib.FORMAT_UNORM8X3)):
        assert call(**bad) == 2, bad
    # an unlisted format on a NULL plane is not looked at (unguided mode)
    assert call(normals=None, depth=None, normal_format=9, frame_normals=None, frame_positions=None) == 1
