"""The firefly pre-filter's rules (bmfr_suppress_fireflies, include/bmfr.h) on
the CPU: the numpy restatement (tests/firefly_np.py) against a pixel-by-pixel
transcription of the four rules, the properties the header states, and the
quality condition on the CPU oracle that makes threshold 2 the default.

Quality figures (pyoracle.OracleLoop, 128 x 80, 8 frames, seed 2, default
feature lists, half tmp_data; relative L2 distance of the TAA output over all
frames from the run whose x50 pixels are divided back out), measured here:

    scene   no filter   radius 1, threshold 2   ratio   threshold 1 (ratio)
    pan     4.76e-3     1.24e-3                 0.26    1.9 .. 3.1 over the
    rand    9.33e-3     2.62e-3                 0.28    three scenes
    far     5.08e-3     1.16e-3                 0.23
"""
from __future__ import annotations

import functools

import numpy as np
import pytest

import firefly_np as fn
import pyoracle
import scenes_np

F32 = np.float32
W, H, FRAMES, SEED = 128, 80, 8, 2
NOT_SCALED, SCALED = (0, 1, 2, 3), (4, 5, 6, 7, 8, 9)


def scalar_filter(noisy, w, h, threshold, radius, floor, replace):
    """Rules 1-4 of the header, one pixel and one f32 operation at a time."""
    k, fl = F32(threshold), F32(floor)
    src = noisy.reshape(h, w, 3)
    out = src.copy()
    clamped = replaced = 0

    def lum(px):
        r, g, b = (F32(v) for v in px)
        return F32(F32(F32(0.2126) * r + F32(0.7152) * g) + F32(0.0722) * b)

    with np.errstate(all="ignore"):
        for y in range(h):
            for x in range(w):
                p = src[y, x]
                if not np.isfinite(p.astype(F32)).all():
                    if replace:
                        out[y, x] = 0
                        replaced += 1
                    continue
                ys = [lum(src[yy, xx]) for yy in range(max(y - radius, 0), min(y + radius, h - 1) + 1)
                      for xx in range(max(x - radius, 0), min(x + radius, w - 1) + 1) if (yy, xx) != (y, x)]
                ys = [v for v in ys if np.isfinite(v)]
                if not ys:
                    continue
                limit = F32(k * max(ys))
                if not limit > fl:
                    limit = fl
                Y = lum(p)
                if Y > limit:
                    s = F32(limit / Y)
                    out[y, x] = [F32(F32(c) * s) for c in p]
                    clamped += 1
    return out.reshape(noisy.shape), (clamped, replaced)


def same_bytes(a, b):
    return a.dtype == b.dtype and a.shape == b.shape and a.tobytes() == b.tobytes()


@pytest.mark.parametrize("half", [False, True], ids=["f32", "half"])
@pytest.mark.parametrize("w,h", [(23, 17), (5, 3), (2, 1), (1, 1)])
@pytest.mark.parametrize("threshold,radius,floor,replace", [(2.0, 1, 0.0, True), (1.0, 2, 0.05, False),
                                                            (4.0, 2, 0.0, True)])
def test_restatement_equals_the_rules_pixel_by_pixel(w, h, half, threshold, radius, floor, replace):
    src = fn.content(w, h, half)
    got, stats = fn.suppress(src, w, h, threshold, radius, floor, replace)
    want, counts = scalar_filter(src, w, h, threshold, radius, floor, replace)
    assert same_bytes(got, want)
    assert stats == counts


@pytest.mark.parametrize("half", [False, True], ids=["f32", "half"])
def test_untouched_pixels_keep_their_bytes_and_stats_count_the_rest(half):
    w, h = 67, 35
    src = fn.content(w, h, half)
    out, (clamped, replaced) = fn.suppress(src, w, h)
    changed = (src.view(np.uint16 if half else np.uint32) != out.view(np.uint16 if half else np.uint32)).any(axis=-1)
    invalid = ~np.isfinite(src.astype(F32)).all(axis=-1)
    assert replaced == int(invalid.sum()) >= 3
    assert (out[invalid] == 0).all() and not np.signbit(out[invalid]).any()
    # a clamped pixel changes unless its limit is its own value scaled by exactly 1 (it is not: Y > limit)
    assert clamped >= 8 and int((changed & ~invalid).sum()) <= clamped
    assert changed.sum() < 0.05 * w * h
    # signed zeros and denormals pass through
    y, x = h // 4 + 2, 3 * w // 4 + 4
    assert np.signbit(out[y, x]).tolist() == [True, False, True]
    kept, _ = fn.suppress(src, w, h, replace_nonfinite=False)
    assert same_bytes(kept[invalid], src[invalid])


def _flat(w, h, value=1.0):
    return np.full((h, w, 3), value, F32)


def test_invalid_pixels_and_nonfinite_neighbours():
    """Rule 1: a NaN / +inf / -inf channel makes the pixel invalid whatever its
    neighbours.  Rule 2: such a pixel (its Y is not finite) is no neighbour:
    the pixel beside it is limited by its other neighbours."""
    for bad in (np.nan, np.inf, -np.inf):
        p = _flat(7, 5)
        p[2, 3, 1] = bad
        p[2, 2] = 10.0      # Y = 10 beside the invalid pixel: the limit comes from the 1s
        out, stats = fn.suppress(p, 7, 5)
        assert stats == (1, 1)
        assert (out[2, 3] == 0).all()
        np.testing.assert_allclose(out[2, 2], 2.0, rtol=1e-6)
        kept, stats = fn.suppress(p, 7, 5, replace_nonfinite=False)
        assert stats == (1, 0) and same_bytes(kept[2, 3], p[2, 3])
    # every neighbour invalid: nothing to compare with, the pixel is copied
    p = np.full((3, 3, 3), np.nan, F32)
    p[1, 1] = 1e6
    out, stats = fn.suppress(p, 3, 3, replace_nonfinite=False)
    assert stats == (0, 0) and same_bytes(out, p)
    # a 1 x 1 plane has no neighbour at all
    one = np.array([[[5.0, 6.0, 7.0]]], F32)
    out, stats = fn.suppress(one, 1, 1)
    assert stats == (0, 0) and same_bytes(out, one)


def test_floor_guards_black_regions():
    """floor = 0: a lone lit pixel among exactly black neighbours is scaled to
    0 (the header's advice); a floor at the signal's level keeps it."""
    p = np.zeros((9, 9, 3), F32)
    p[4, 4] = 0.3
    out, stats = fn.suppress(p, 9, 9)
    assert stats == (1, 0) and (out == 0).all()
    out, stats = fn.suppress(p, 9, 9, floor=0.5)
    assert stats == (0, 0) and same_bytes(out, p)


def test_adjacent_fireflies_protect_each_other():
    """A documented limit of the rule: each of two adjacent fireflies is the
    other's brightest neighbour, so neither is clamped; alone, either is."""
    p = _flat(9, 7)
    p[3, 4] = 50.0
    alone, stats = fn.suppress(p, 9, 7)
    assert stats == (1, 0)
    np.testing.assert_allclose(alone[3, 4], 2.0, rtol=1e-6)
    p[3, 5] = 50.0
    pair, stats = fn.suppress(p, 9, 7)
    assert stats == (0, 0) and same_bytes(pair, p)


@pytest.mark.parametrize("half", [False, True], ids=["f32", "half"])
@pytest.mark.parametrize("radius", [1, 2])
@pytest.mark.parametrize("region", [(0, 0, 67, 35), (30, 20, 70, 60), (61, 0, 67, 80), (0, 45, 128, 35)])
def test_region_equals_whole_image_outside_the_rings(region, radius, half):
    """The filter on a sub-rectangle equals the whole-image filter except on
    the outermost `radius` rings along the rectangle's edges inside the image."""
    src = fn.content(W, H, half)
    whole, _ = fn.suppress(src, W, H, 2.0, radius)
    x0, y0, rw, rh = region
    cut = np.ascontiguousarray(src[y0:y0 + rh, x0:x0 + rw])
    part, _ = fn.suppress(cut, rw, rh, 2.0, radius)
    rings = fn.differing_rings(W, H, region, radius)
    assert rings.any() and not rings.all()
    a, b = part[~rings], whole[y0:y0 + rh, x0:x0 + rw][~rings]
    assert same_bytes(a, b)


# ---- the quality condition ----
def fire_mask(f: int, seed: int = SEED) -> np.ndarray:
    """The pixels scenes_np._render multiplies by 50 in frame f: its `fire` hash."""
    pix = (np.arange(H, dtype=np.uint32)[:, None] * np.uint32(W) + np.arange(W, dtype=np.uint32)[None, :])
    with np.errstate(over="ignore"):
        fh = scenes_np.mix32(np.array([(f * 0x9E3779B1 + 0x632BE5AB) & 0xFFFFFFFF]))[0]
        base = scenes_np.mix32(np.array([(seed & 0xFFFFFFFF) ^ int(fh)]))[0] ^ (pix * np.uint32(0x85EBCA77))
        fire = scenes_np.mix32(base ^ np.uint32(0x27D4EB2F))
    return fire < 429497


@functools.lru_cache(maxsize=None)
def run(scene: str, mode: str) -> np.ndarray:
    """The oracle's TAA output over all frames; mode: raw (the scene as it is),
    free (its x50 pixels divided back out) or a threshold (filtered at radius 1)."""
    def source(f):
        fr = scenes_np.frame(scene, W, H, f, SEED)
        noisy = np.array(fr["noisy"]).reshape(H, W, 3)
        if mode == "free":
            noisy[fire_mask(f)] /= F32(50.0)
        elif mode != "raw":
            noisy, _ = fn.suppress(noisy, W, H, threshold=float(mode), radius=1)
        fr["noisy"] = noisy.reshape(-1)
        return fr
    cfg = pyoracle.make_cfg(W, H, NOT_SCALED, SCALED, 1)
    recs = scenes_np.run_loop(pyoracle.OracleLoop(cfg), scene, W, H, FRAMES, SEED, source=source)
    return np.concatenate([r["result"] for r in recs]).astype(np.float64)


def distance(scene: str, mode: str) -> float:
    ref = run(scene, "free")
    return float(np.sqrt(((run(scene, mode) - ref) ** 2).sum() / (ref ** 2).sum()))


def test_fire_mask_is_the_scene_s():
    """The recomputed hash names exactly the pixels that stand out: dividing
    them back leaves no pixel 20 x brighter than the frame's median."""
    share = []
    for f in range(FRAMES):
        m = fire_mask(f)
        share.append(m.mean())
        noisy = np.array(scenes_np.frame("far", W, H, f, SEED)["noisy"]).reshape(H, W, 3)
        assert m.any() or f
        lum = noisy.sum(axis=-1)
        assert not m.any() or lum[m].min() > 5 * np.median(lum)
        noisy[m] /= F32(50.0)
        assert noisy.sum(axis=-1).max() < 20 * np.median(lum)
    assert 0.5e-4 < np.mean(share) < 3e-4


@pytest.mark.parametrize("scene", ["pan", "rand", "far"])
def test_default_threshold_halves_the_damage(scene):
    raw, filtered = distance(scene, "raw"), distance(scene, "2.0")
    print(f"{scene}: no filter {raw:.3e}, radius 1 threshold 2 {filtered:.3e}, ratio {filtered / raw:.2f}")
    assert raw > 0
    assert filtered <= 0.5 * raw


@pytest.mark.parametrize("scene", ["pan", "rand", "far"])
def test_threshold_one_is_worse_than_no_filter(scene):
    raw, filtered = distance(scene, "raw"), distance(scene, "1.0")
    print(f"{scene}: no filter {raw:.3e}, radius 1 threshold 1 {filtered:.3e}, ratio {filtered / raw:.2f}")
    assert filtered > raw
