"""The G-buffer front end (bmfr_prepare_frame, include/bmfr.h) restated in
numpy, and seeded G-buffers for its tests.  TEST INFRASTRUCTURE ONLY.

Every line of the restatement is one np.float32 operation, associated as the
header writes it: numpy's f32 +, -, *, / and sqrt are IEEE correctly rounded,
half <-> f32 conversions are exact / round to nearest even, so the kernel must
equal it byte for byte.

A G-buffer here is a dict of flat numpy planes over a region (x0, y0, w, h) of
a W x H frame, with the keys Denoiser.prepare takes; a plane's format follows
from its dtype, as there: float32 = F32X3 / F32X2, float16 = F16X4 / F16X2,
uint8 = UNORM8X4, int16 = octahedral snorm16 x 2."""
from __future__ import annotations

import numpy as np

F32 = np.float32
PLANE_KEYS = ("radiance", "albedo", "normals", "positions", "depth", "motion", "prev_positions", "prev_normals",
              "prev_object_id", "object_transforms")
OUTPUTS = ("noisy", "normals", "positions", "albedo", "prev_pixel", "prev_positions_moved", "prev_normals_moved")


# ------------------------------------------------------------ restatement --
def coords(region, dtype=np.int64):
    """Image coordinates (x, y) of the region's pixels, flat, row by row."""
    x0, y0, w, h = region
    ys, xs = np.mgrid[y0:y0 + h, x0:x0 + w]
    return xs.reshape(-1).astype(dtype), ys.reshape(-1).astype(dtype)


def channels(buf: np.ndarray) -> np.ndarray:
    """A three-channel plane as f32 (n, 3): F32X3, F16X4 (4th ignored) or UNORM8X4 (v / 255, 4th ignored)."""
    if buf.dtype == np.float32:
        return buf.reshape(-1, 3)
    if buf.dtype == np.float16:
        return buf.reshape(-1, 4)[:, :3].astype(F32)
    assert buf.dtype == np.uint8
    return buf.reshape(-1, 4)[:, :3].astype(F32) / F32(255.0)


def demodulate(radiance: np.ndarray, albedo: np.ndarray, floor):
    """A: (noisy, albedo) as f32 (n, 3)."""
    a = channels(albedo)
    with np.errstate(all="ignore"):
        d = np.where(a > F32(floor), a, F32(floor)).astype(F32)   # NaN > floor is false: the floor
        noisy = channels(radiance) / d
    return noisy, a


def position_from_depth(depth, inv_view_proj, jitter, region, W, H):
    """B: world positions (n, 3) from clip-space depth, the sample at (x + jx, y + 1 - jy)."""
    m = np.asarray(inv_view_proj, F32)
    jx, jy = F32(jitter[0]), F32(jitter[1])
    x, y = coords(region)
    depth = depth.reshape(-1)
    with np.errstate(all="ignore"):
        sx = x.astype(F32) + jx
        sy = y.astype(F32) + (F32(1.0) - jy)
        nx = (sx / F32(W)) * F32(2.0) - F32(1.0)
        ny = (sy / F32(H)) * F32(2.0) - F32(1.0)
        h = [((m[i] * nx + m[4 + i] * ny) + m[8 + i] * depth) + m[12 + i] for i in range(4)]
        out = np.stack([h[i] / h[3] for i in range(3)], axis=-1)
    assert out.dtype == F32
    return out


def oct_decode(s16: np.ndarray) -> np.ndarray:
    """C: octahedral snorm16 x 2 -> unit vectors, f32 (n, 3)."""
    e = s16.reshape(-1, 2).astype(F32) / F32(32767.0)
    e = np.where(e < F32(-1.0), F32(-1.0), e).astype(F32)
    ex, ey = e[:, 0], e[:, 1]
    ax, ay = np.abs(ex), np.abs(ey)
    z = (F32(1.0) - ax) - ay
    fx = (F32(1.0) - ay) * np.where(ex >= 0, F32(1.0), F32(-1.0))
    fy = (F32(1.0) - ax) * np.where(ey >= 0, F32(1.0), F32(-1.0))
    ox = np.where(z < 0, fx, ex).astype(F32)
    oy = np.where(z < 0, fy, ey).astype(F32)
    length = np.sqrt((ox * ox + oy * oy) + z * z)
    out = np.stack([ox / length, oy / length, z / length], axis=-1)
    assert out.dtype == F32
    return out


def oct_encode(n: np.ndarray) -> np.ndarray:
    """Unit vectors (n, 3) -> octahedral snorm16 x 2 (n, 2), computed in f64."""
    n = n.reshape(-1, 3).astype(np.float64)
    p = n[:, :2] / np.abs(n).sum(axis=1, keepdims=True)
    sign = np.where(p >= 0, 1.0, -1.0)
    folded = (1.0 - np.abs(p[:, ::-1])) * sign
    p = np.where(n[:, 2:3] < 0, folded, p)
    return np.rint(p * 32767.0).astype(np.int16)


def normals_of(buf: np.ndarray) -> np.ndarray:
    return oct_decode(buf) if buf.dtype == np.int16 else channels(buf)


def prev_pixel_of(motion, scale, at_centre, jitter, region):
    """D: motion vectors (F32X2 / F16X2) -> prev_pixel, f32 (n, 2)."""
    mv = motion.reshape(-1, 2).astype(F32)
    jx, jy = F32(jitter[0]), F32(jitter[1])
    x, y = coords(region)
    fx, fy = x.astype(F32), y.astype(F32)
    with np.errstate(all="ignore"):
        mx = mv[:, 0] * F32(scale[0])
        my = mv[:, 1] * F32(scale[1])
        if at_centre:
            pfx = ((fx + F32(0.5)) - mx) - jx
            pfy = ((fy + F32(0.5)) - my) - (F32(1.0) - jy)
        else:
            pfx = fx - mx
            pfy = fy - my
    out = np.stack([pfx, pfy], axis=-1)
    assert out.dtype == F32
    return out


def moved(plane: np.ndarray, ids, transforms, translate: bool) -> np.ndarray:
    """E: a prepared plane (f32 or f16, (n, 3)) moved by each pixel's object
    transform; pixels whose id is not in the table keep their bytes."""
    plane = plane.reshape(-1, 3)
    out = plane.copy()
    k = 0 if transforms is None else transforms.size // 12
    if k == 0:
        return out
    ids = ids.reshape(-1).view(np.uint16).astype(np.int64)
    hit = ids < k
    M = transforms.reshape(-1, 12).astype(F32)[np.where(hit, ids, 0)]
    v = plane.astype(F32)
    with np.errstate(all="ignore"):
        for i in range(3):
            r = (M[:, 4 * i] * v[:, 0] + M[:, 4 * i + 1] * v[:, 1]) + M[:, 4 * i + 2] * v[:, 2]
            if translate:
                r = r + M[:, 4 * i + 3]
            assert r.dtype == F32
            out[hit, i] = r.astype(plane.dtype)[hit]
    return out


def prepare(g: dict, jitter, region, W: int, H: int, half: bool, outputs=None) -> dict:
    """Every output of bmfr_prepare_frame whose inputs are in g (or those
    named), as flat arrays in the context's input format."""
    dt = np.float16 if half else F32
    has = lambda *names: all(g.get(n) is not None for n in names)  # noqa: E731
    out = {}
    with np.errstate(all="ignore"):
        if has("albedo"):
            out["albedo"] = channels(g["albedo"]).astype(dt)
            if has("radiance"):
                floor = g.get("albedo_floor", F32(1.0) / F32(255.0))   # bmfr_gbuffer_default's
                out["noisy"] = demodulate(g["radiance"], g["albedo"], floor)[0].astype(dt)
        if has("normals"):
            out["normals"] = normals_of(g["normals"]).astype(dt)
        if has("positions"):
            out["positions"] = g["positions"].reshape(-1, 3).astype(dt)
        elif has("depth"):
            out["positions"] = position_from_depth(g["depth"], g["inv_view_proj"], jitter, region, W, H).astype(dt)
        if has("motion"):
            out["prev_pixel"] = prev_pixel_of(g["motion"], g.get("motion_scale", (1.0, 1.0)),
                                              g.get("motion_at_pixel_centre", 0), jitter, region)
        if has("prev_positions"):
            assert g["prev_positions"].dtype == dt
            out["prev_positions_moved"] = moved(g["prev_positions"], g.get("prev_object_id"),
                                                g.get("object_transforms"), True)
        if has("prev_normals"):
            assert g["prev_normals"].dtype == dt
            out["prev_normals_moved"] = moved(g["prev_normals"], g.get("prev_object_id"), g.get("object_transforms"),
                                              False)
    if outputs is not None:
        out = {k: out[k] for k in outputs}
    return {k: np.ascontiguousarray(v).reshape(-1) for k, v in out.items()}


# -------------------------------------------------------------- generators --
def region_of(plane: np.ndarray, W: int, H: int, region) -> np.ndarray:
    """The region's pixels of a full-frame flat plane, flat."""
    x0, y0, w, h = region
    return np.ascontiguousarray(plane.reshape(H, W, -1)[y0:y0 + h, x0:x0 + w]).reshape(-1)


def depth_and_inverse(positions: np.ndarray, vp):
    """Clip-space z / w of world positions under the column-major
    view-projection vp, in f64 stored as f32, and vp's inverse (f64, stored as
    column-major f32): what a renderer's depth buffer and camera hold."""
    M = np.asarray(vp, np.float64).reshape(4, 4).T
    p = np.concatenate([positions.reshape(-1, 3).astype(np.float64), np.ones((positions.size // 3, 1))], axis=1)
    clip = p @ M.T
    depth = (clip[:, 2] / clip[:, 3]).astype(F32)
    inv = np.linalg.inv(M)
    return depth, inv.T.reshape(-1).astype(F32)


def rgba16(c: np.ndarray, rng) -> np.ndarray:
    """(n, 3) -> F16X4 with a seeded 4th component the kernel must ignore."""
    c = c.reshape(-1, 3)
    return np.concatenate([c.astype(np.float16), rng.uniform(-4, 4, (c.shape[0], 1)).astype(np.float16)],
                          axis=1).reshape(-1)


def unorm8(c: np.ndarray, rng) -> np.ndarray:
    c = c.reshape(-1, 3)
    q = np.rint(np.clip(np.nan_to_num(c.astype(np.float64)), 0, 1) * 255).astype(np.uint8)
    return np.concatenate([q, rng.randint(0, 256, (c.shape[0], 1)).astype(np.uint8)], axis=1).reshape(-1)


def engine_albedo(n: int, rng, with_nan: bool) -> np.ndarray:
    """Albedo (n, 3) f32 in [0, 1] with exact zeros, values below the default
    floor (1 / 255) and, on request, NaN."""
    a = rng.uniform(0.05, 1.0, (n, 3)).astype(F32)
    pick = rng.permutation(n)
    a[pick[:n // 16]] = 0.0
    a[pick[n // 16:n // 8], 1] = F32(1.0 / 1024.0)
    a[pick[n // 8:n // 8 + n // 32], 0] = F32(1e-30)
    if with_nan:
        a[pick[n // 4:n // 4 + n // 64], 2] = np.nan
    return a


def random_transforms(k: int, rng) -> np.ndarray:
    """k rigid 3x4 transforms (row-major), f32: a rotation about a seeded axis and a translation."""
    out = np.empty((k, 12), F32)
    for i in range(k):
        axis = rng.normal(size=3)
        axis /= np.linalg.norm(axis)
        ang = rng.uniform(-0.3, 0.3)
        K = np.array([[0, -axis[2], axis[1]], [axis[2], 0, -axis[0]], [-axis[1], axis[0], 0]])
        R = np.eye(3) + np.sin(ang) * K + (1 - np.cos(ang)) * (K @ K)
        out[i] = np.concatenate([R, rng.uniform(-1, 1, (3, 1))], axis=1).reshape(-1)
    return out


def make_gbuffer(frame: dict, vp, W: int, H: int, region, seed: int, half: bool, radiance="f32", albedo="f32",
                 normals="f32", positions="depth", motion="f32", objects: int = 5, with_nan: bool = False,
                 at_centre: int = 0, motion_scale=(1.0, 1.0)) -> dict:
    """A seeded G-buffer over `region` in the named formats, from one frame of
    the synthetic scene (`frame`: bmfr_amd.synth_frame_host's planes; vp: that
    frame's view-projection): radiance = noisy * albedo', albedo' a seeded
    plane with zeros, sub-floor values and (with_nan) NaN; the scene's normals
    and positions (or their depth); seeded motion vectors of a few pixels; and
    seeded previous planes, ids (some past the table, some 0xFFFF) and
    transforms."""
    rng = np.random.RandomState(seed)
    x0, y0, w, h = region
    n = w * h
    cut = lambda p: region_of(np.asarray(p, F32).reshape(-1), W, H, region)  # noqa: E731
    g = {}
    alb = engine_albedo(n, rng, with_nan)
    rad = (cut(frame["noisy"]).reshape(-1, 3) * np.nan_to_num(alb)).astype(F32)
    g["radiance"] = {"f32": lambda: rad.reshape(-1), "f16": lambda: rgba16(rad, rng)}[radiance]()
    g["albedo"] = {"f32": lambda: alb.reshape(-1), "f16": lambda: rgba16(alb, rng),
                   "unorm8": lambda: unorm8(alb, rng)}[albedo]()
    nrm = cut(frame["normals"])
    g["normals"] = {"f32": lambda: nrm, "f16": lambda: rgba16(nrm, rng),
                    "oct": lambda: oct_encode(nrm).reshape(-1)}[normals]()
    if positions == "given":
        g["positions"] = cut(frame["positions"])
    else:
        depth, inv = depth_and_inverse(np.asarray(frame["positions"], F32), vp)
        g["depth"], g["inv_view_proj"] = region_of(depth, W, H, region), inv
    mv = (rng.uniform(-6, 6, (n, 2)) / np.asarray(motion_scale)).astype(F32)
    g["motion"] = (mv if motion == "f32" else mv.astype(np.float16)).reshape(-1)
    g["motion_scale"], g["motion_at_pixel_centre"] = tuple(motion_scale), at_centre
    dt = np.float16 if half else F32
    g["prev_positions"] = rng.uniform(-8, 8, n * 3).astype(dt)
    g["prev_normals"] = cut(frame["normals"])[::-1].copy().astype(dt)
    if objects:
        ids = rng.randint(0, objects + 3, n).astype(np.uint16)   # some at or past the table
        ids[rng.permutation(n)[:n // 10]] = 0xFFFF
        g["prev_object_id"] = ids
        g["object_transforms"] = random_transforms(objects, rng).reshape(-1)
    return g
