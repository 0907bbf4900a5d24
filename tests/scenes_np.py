"""Deterministic numpy content for the frame loops.  TEST INFRASTRUCTURE ONLY:
imports nothing from bmfr_amd.

Every frame loop here (StagePipeline, Denoiser, pyoracle.OracleLoop,
ref_run.RefLoop) takes arbitrary planes and camera matrices, so content the
synthetic sequence (one room, eight spheres, a slow dolly) cannot produce
comes from here instead:

  pan    a fast pan (16.3 px/frame at any width, three frames right, then
         back; 3.37 px/frame up and down) over a fronto-parallel wall at
         z = 0, depth 2, with a tilted foreground quad drifting the other
         way: disocclusion on one side, occlusion on the other, taps beyond
         the image edge on either side (the reprojection's ix = -2 and
         ix = W + 1 clamps)
  far    one slightly tilted wall filling the image, every coordinate within
         10 % of 16 on every axis, sub-pixel drift; a block's x / y ranges
         are below 1 and its x^2 / y^2 ranges above, so both arms of scale()
         (bmfr.cl:200-205) are live in one frame
  rand   five room planes and six seeded quads under a seeded camera path;
         grazing floor / wall footprints straddle the position limit, so the
         tap acceptance (bmfr.cl:380-404) goes through all 16 masks
  clamp  pan, plus a screen-space patch of NaN normals, a patch of finite
         positions outside half's range once squared or cubed (x ~ 2000,
         y ~ 300), and at frame CUT_FRAME a previous camera that throws the
         quad's pixels far off the image (|pf| ~ 1e7 .. 1e8), where the float
         clamp of the reprojection decides the tap index
  clamp_nan  clamp without the out-of-range position patch: the form for f32
         tmp_data, which has no +-65504 clamp (bmfr.cl:468-473)

Out of scope for clamp, on purpose: positions stay finite (no NaN / Inf
positions), and every reprojected coordinate stays finite and below 2^30 in
magnitude.  The reference converts it with convert_int2_rtn, which is
undefined beyond the int range, so there would be nothing to be equal to.
tests/test_scenes_np.py asserts both on the CPU oracle.

Conventions (those of the synthetic sequence): pixel (x, y) of frame f looks
through NDC (2 (x + jx) / W - 1, 2 (y + 1 - jy) / H - 1), the inverse of the
reprojection of bmfr.cl:343-355; jitter is Halton(2, 3) of f + 1; matrices
are column-major view-projections.  Geometry is ray-plane / ray-quad in
float64, rounded once to f32.  Noise is an integer hash of (seed, frame,
pixel, channel) in uint32 arithmetic; nothing depends on numpy's Generator
streams or on libm (only + - * / sqrt), so the bytes are the same anywhere.

    frame(scene, W, H, f, seed, region=None, still=False, speed=1.0) -> dict
        noisy, normals, positions, albedo   flat f32, (H, W, 3) order
        prev_vp   camera matrix of frame max(f - 1, 0), 16 floats
        jitter    pixel offset of frame f, 2 floats
    region = (x0, y0, w, h): the same planes cut to a tile's region.
    still: the camera of frame 0 on every frame (the jitter still moves).
    speed: scales the pan scenes' camera path (a tiled context's halo covers
    tile_halo - 34 px of motion, the quad's parallax included).
"""
from __future__ import annotations

import functools

import numpy as np

SCENES = ("pan", "far", "rand", "clamp", "clamp_nan")
TAN_Y = 0.4663  # ~ tan(25 deg)
PAN_SPEED_PX = 16.3
PAN_X = (0, 1, 2, 3, 2, 1)        # the pan's path in units of its speed
PAN_Y = (0, 1, 2, 1, 0, 1)
CUT_FRAME = 3   # clamp: the frame whose previous camera throws the quad's pixels off the image
CUT_SCALE = 1.0e6
NAN_PATCH = (20, 30, 8, 6)        # x, y, w, h (pixels): NaN normals
RANGE_PATCH = (60, 48, 10, 8)     # finite positions beyond half's range once squared / cubed


def halton(index: int, base: int) -> float:
    f, r = 1.0, 0.0
    while index > 0:
        f /= base
        r += f * (index % base)
        index //= base
    return r


def jitter(f: int):
    return [float(np.float32(halton(f + 1, 2))), float(np.float32(halton(f + 1, 3)))]


def mix32(h):
    """The synthetic scene's 32-bit finaliser, on uint32 arrays (wrapping)."""
    h = np.asarray(h, np.uint32).copy()
    with np.errstate(over="ignore"):
        h ^= h >> np.uint32(16)
        h *= np.uint32(0x7FEB352D)
        h ^= h >> np.uint32(15)
        h *= np.uint32(0x846CA68B)
        h ^= h >> np.uint32(16)
    return h


def _u01(seed: int, k: int) -> float:
    """Seeded scalar in [0, 1)."""
    return float(mix32(np.array([(seed * 0x9E3779B1 + k * 0x85EBCA77 + 0x632BE5AB) & 0xFFFFFFFF]))[0]) / 4294967296.0


def _dot(a, b):
    """a . b over the last axis, spelled out: no BLAS, one fixed association."""
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    return a[..., 0] * b[..., 0] + a[..., 1] * b[..., 1] + a[..., 2] * b[..., 2]


def _norm(v):
    v = np.asarray(v, np.float64)
    return v / np.sqrt(_dot(v, v))


def _basis(fwd):
    fwd = _norm(fwd)
    right = _norm([-fwd[2], 0.0, fwd[0]])
    up = np.array([right[1] * fwd[2] - right[2] * fwd[1], right[2] * fwd[0] - right[0] * fwd[2],
                   right[0] * fwd[1] - right[1] * fwd[0]])
    return right, up, fwd


def _quad(c, a, b, albedo):
    """Rectangle of centre c and half-edge vectors a, b (orthogonal)."""
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    n = _norm(np.cross(a, b))
    return dict(c=np.asarray(c, np.float64), a=a, b=b, n=n, albedo=albedo)


def _plane(p, n, albedo=None):
    return dict(c=np.asarray(p, np.float64), n=_norm(n), albedo=albedo)


def camera(scene: str, W: int, H: int, f: int, seed: int, speed: float = 1.0):
    """(eye, right, up, fwd, tan_x, tan_y) of frame f, float64."""
    tan_x = TAN_Y * W / H
    if scene in ("pan", "clamp", "clamp_nan"):
        px = 2.0 * 2.0 * tan_x / W   # a pixel's footprint on the wall (depth 2)
        # there and back: 16.3 px/frame right for three frames, then left; 3.37 px/frame up and
        # down -- so that taps cross an internal tile edge in both directions and leave the image
        # on either side
        eye = np.array([speed * PAN_SPEED_PX * px * PAN_X[f % 6], speed * 3.37 * px * PAN_Y[f % 6], 2.0])
        fwd = [0.0, 0.0, -1.0]
    elif scene == "far":
        eye = np.array([16.0 + 0.002 * f, 16.0 - 0.0013 * f, 16.6])
        fwd = [0.0, 0.0, -1.0]
    elif scene == "rand":
        u = [_u01(seed, 100 + k) for k in range(12)]
        eye = np.array([-1.0 + 2.0 * u[0], 0.5 + u[1], 5.0 + u[2]])
        eye = eye + f * np.array([0.10 * (u[3] - 0.5), 0.04 * (u[4] - 0.5), -0.03 - 0.06 * u[5]])
        yaw = 0.3 * (u[6] - 0.5) + f * 0.012 * (u[7] - 0.5)
        pitch = -0.10 - 0.10 * u[8] + f * 0.004 * (u[9] - 0.5)
        fwd = [-yaw, pitch, -1.0]
    else:
        raise ValueError(scene)
    right, up, fwd = _basis(fwd)
    return eye, right, up, fwd, tan_x, TAN_Y


def view_projection(scene: str, W: int, H: int, f: int, seed: int, speed: float = 1.0):
    """Column-major VP = P V of frame f as 16 f32 values: view rows right, up,
    -fwd; GL perspective with the camera's tangents."""
    e, r, u, fw, tx, ty = camera(scene, W, H, f, seed, speed)
    n, fa = 0.05, 100.0
    V = [[r[0], r[1], r[2], -_dot(r, e)], [u[0], u[1], u[2], -_dot(u, e)],
         [-fw[0], -fw[1], -fw[2], _dot(fw, e)], [0.0, 0.0, 0.0, 1.0]]
    P = [[1.0 / tx, 0.0, 0.0, 0.0], [0.0, 1.0 / ty, 0.0, 0.0],
         [0.0, 0.0, (fa + n) / (n - fa), 2 * fa * n / (n - fa)], [0.0, 0.0, -1.0, 0.0]]
    return np.array([[sum(P[i][k] * V[k][j] for k in range(4)) for j in range(4)] for i in range(4)])


def _surfaces(scene: str, f: int, seed: int):
    """(planes, quads) of frame f."""
    if scene in ("pan", "clamp", "clamp_nan"):
        wall = _plane([0, 0, 0], [0, 0, 1])
        quad = _quad([0.9 - 0.05 * f, 0.1, 0.7], [0.45, 0.0, 0.2], [0.0, 0.5, 0.0], (0.8, 0.35, 0.2))
        return [wall], [quad]
    if scene == "far":
        return [_plane([16.0, 16.0, 14.7], [-0.10, -0.06, 1.0])], []
    planes = [_plane([0, -2, 0], [0, 1, 0]), _plane([0, 4, 0], [0, -1, 0]), _plane([0, 0, -10], [0, 0, 1]),
              _plane([-6, 0, 0], [1, 0, 0]), _plane([6, 0, 0], [-1, 0, 0])]
    quads = []
    for q in range(6):
        u = [_u01(seed, 1000 + 16 * q + k) for k in range(10)]
        c = [-4.0 + 8.0 * u[0], -1.5 + 4.0 * u[1], -7.0 + 9.0 * u[2]]
        a = np.array([0.5 + 1.2 * u[3], 0.0, 1.6 * (u[4] - 0.5)])
        b0 = np.array([0.0, 0.5 + 1.0 * u[5], 1.2 * (u[6] - 0.5)])
        b = b0 - a * (_dot(a, b0) / _dot(a, a))
        quads.append(_quad(c, a, b, (0.2 + 0.7 * u[7], 0.2 + 0.7 * u[8], 0.2 + 0.7 * u[9])))
    return planes, quads


def _render(scene: str, W: int, H: int, f: int, seed: int, cam_f: int, speed: float):
    e, r, u, fw, tx, ty = camera(scene, W, H, cam_f, seed, speed)
    jx, jy = jitter(f)
    xs = np.arange(W, dtype=np.float64)[None, :]
    ys = np.arange(H, dtype=np.float64)[:, None]
    nx = 2.0 * (xs + jx) / W - 1.0 + 0.0 * ys
    ny = 2.0 * (ys + 1.0 - jy) / H - 1.0 + 0.0 * xs
    d = fw[None, None, :] + r[None, None, :] * (nx * tx)[..., None] + u[None, None, :] * (ny * ty)[..., None]
    best = np.full((H, W), np.inf)
    pos = np.zeros((H, W, 3))
    nrm = np.zeros((H, W, 3))
    alb = np.zeros((H, W, 3))
    planes, quads = _surfaces(scene, f, seed)
    for k, s in enumerate(planes + quads):
        dn = _dot(d, s["n"])
        with np.errstate(divide="ignore", invalid="ignore"):
            t = _dot(s["c"] - e, s["n"]) / dn
        p = e[None, None, :] + d * t[..., None]
        ok = np.isfinite(t) & (t > 1e-6) & (t < best)
        if "a" in s:
            q = p - s["c"]
            ok &= (np.abs(_dot(q, s["a"])) <= _dot(s["a"], s["a"])) & (np.abs(_dot(q, s["b"])) <= _dot(s["b"], s["b"]))
        else:
            for ax in range(3):  # an axis-aligned plane's own coordinate is exact
                if abs(s["n"][ax]) == 1.0:
                    p[..., ax] = s["c"][ax]
        n = s["n"] if _dot(s["n"], fw) < 0 else -s["n"]
        if s.get("albedo") is None:
            with np.errstate(invalid="ignore"):
                chk = (np.floor(p[..., 0] * 2.0) + np.floor(p[..., 1] * 2.0) + np.floor(p[..., 2] * 2.0)) % 2.0
            a = np.where(chk[..., None] > 0.5, 0.85, 0.15) * np.array([1.0, 0.95, 0.85 + 0.03 * k])
        else:
            a = np.broadcast_to(np.array(s["albedo"]), p.shape)
        best = np.where(ok, t, best)
        pos = np.where(ok[..., None], p, pos)
        nrm = np.where(ok[..., None], n, nrm)
        alb = np.where(ok[..., None], a, alb)
    assert np.isfinite(best).all(), "every ray must hit"
    # irradiance: one point light, + - * / sqrt only
    L = e + np.array([1.5, 2.5, 1.0])
    l = L - pos
    d2 = _dot(l, l)
    cosv = np.maximum(_dot(nrm, l) / np.sqrt(d2), 0.0)
    irr = (0.25 + 3.0 * cosv / (1.0 + 0.05 * d2))[..., None] * np.array([1.0, 0.95, 0.85])
    # noise: 3 u^2 (mean 1) per channel, rare x50 fireflies
    pix = (np.arange(H, dtype=np.uint32)[:, None] * np.uint32(W) + np.arange(W, dtype=np.uint32)[None, :])
    with np.errstate(over="ignore"):
        fh = mix32(np.array([(f * 0x9E3779B1 + 0x632BE5AB) & 0xFFFFFFFF]))[0]
        base = mix32(np.array([(seed & 0xFFFFFFFF) ^ int(fh)]))[0] ^ (pix * np.uint32(0x85EBCA77))
        fire = mix32(base ^ np.uint32(0x27D4EB2F))
        noisy = np.empty((H, W, 3))
        for c in range(3):
            rr = mix32(base + np.uint32((0xC2B2AE3D * (c + 1)) & 0xFFFFFFFF))
            uu = ((rr >> np.uint32(8)).astype(np.float64) + 1.0) / 16777216.0
            noisy[..., c] = irr[..., c] * (3.0 * uu * uu)
    noisy *= np.where(fire < 429497, 50.0, 1.0)[..., None]
    return noisy, nrm, pos, alb


def _patch(W, H, rect):
    x, y, w, h = rect
    return slice(min(y, H - h), min(y, H - h) + h), slice(min(x, W - w), min(x, W - w) + w)


def patch_mask(W: int, H: int, rect) -> np.ndarray:
    m = np.zeros((H, W), bool)
    m[_patch(W, H, rect)] = True
    return m


def quad_mask(scene: str, W: int, H: int, f: int, seed: int) -> np.ndarray:
    """Pixels of frame f that show the pan scenes' foreground quad (z > 0)."""
    return _frame(scene, W, H, f, seed, False, 1.0)["positions"].reshape(H, W, 3)[..., 2] > 0


@functools.lru_cache(maxsize=256)
def _frame(scene: str, W: int, H: int, f: int, seed: int, still: bool, speed: float):
    if scene not in SCENES:
        raise ValueError(scene)
    noisy, nrm, pos, alb = _render(scene, W, H, f, seed, 0 if still else f, speed)
    if scene in ("clamp", "clamp_nan"):
        nrm[_patch(W, H, NAN_PATCH)] = np.nan
    if scene == "clamp":
        ys, xs = _patch(W, H, RANGE_PATCH)
        gy, gx = np.mgrid[ys, xs]
        pos[ys, xs, 0] = 2000.0 + 0.5 * (gx - xs.start)
        pos[ys, xs, 1] = -300.0 - 0.25 * (gy - ys.start)
    vp = view_projection(scene, W, H, 0 if still else max(f - 1, 0), seed, speed)
    if scene in ("clamp", "clamp_nan") and f == CUT_FRAME and not still:
        # agrees with the true camera on the wall (z = 0 exactly) and throws everything in front
        # of it: clip x += S z, clip y -= S z
        vp = vp.copy()
        vp[0, 2] += CUT_SCALE
        vp[1, 2] -= CUT_SCALE
    out = {k: np.ascontiguousarray(v, np.float32).reshape(-1) for k, v in
           (("noisy", noisy), ("normals", nrm), ("positions", pos), ("albedo", alb))}
    for v in out.values():
        v.setflags(write=False)
    out["prev_vp"] = tuple(float(np.float32(vp[row, col])) for col in range(4) for row in range(4))
    out["jitter"] = tuple(jitter(f))
    return out


def frame(scene: str, W: int, H: int, f: int, seed: int = 1, region=None, still: bool = False,
          speed: float = 1.0) -> dict:
    fr = _frame(scene, W, H, f, seed, bool(still), float(speed))
    out = {"prev_vp": list(fr["prev_vp"]), "jitter": list(fr["jitter"])}
    for k in ("noisy", "normals", "positions", "albedo"):
        a = fr[k]
        if region is not None:
            x0, y0, w, h = region
            assert 0 <= x0 and 0 <= y0 and x0 + w <= W and y0 + h <= H, region
            a = np.ascontiguousarray(a.reshape(H, W, 3)[y0:y0 + h, x0:x0 + w]).reshape(-1)
            a.setflags(write=False)
        out[k] = a
    return out


def run_loop(loop, scene: str, W: int, H: int, frames: int, seed: int = 1, to_device=None, sync=None,
             still: bool = False, prepare=None, source=None):
    """Drive a frame loop (upload / run_stages / swap) over a scene; returns
    the per-frame records as numpy arrays.  prepare: maps the four planes
    (numpy, f32) before upload, e.g. a round trip through half.  source: f ->
    a frame() dict, for content derived from a scene (then scene, seed and
    still are not used)."""
    from seq_util import to_np
    out = []
    for f in range(frames):
        fr = source(f) if source is not None else frame(scene, W, H, f, seed, still=still)
        planes = [fr[k] for k in ("noisy", "normals", "positions", "albedo")]
        if prepare is not None:
            planes = [prepare(p) for p in planes]
        if to_device is not None:
            planes = [to_device(p) for p in planes]
        loop.upload(*planes)
        rec = {}
        loop.run_stages(fr["prev_vp"], fr["jitter"], f, record=rec)
        if sync is not None:
            sync()
        out.append({k: to_np(v).copy() for k, v in rec.items()})
        loop.swap()
    return out
