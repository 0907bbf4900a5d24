"""tests/scenes_np.py on the CPU: the generator is deterministic and agrees
with its own camera matrices, and the CPU oracle (pyoracle.OracleLoop), run
over each scene, really goes where the GPU content tests
(tests/test_gpu_content_parity.py) claim to go -- mixed tap acceptance, both
arms of scale(), the NaN guard and the +-65504 clamp of the design matrix,
the far-off reprojection.  The coverage figures are conditions on the
oracle's records, asserted here, not measurements taken on trust; the last
tests check, before anything runs on a GPU, that the clamp scene stays in
territory the reference kernels define (finite positions, reprojected
coordinates finite and below 2^30)."""
from __future__ import annotations

import hashlib

import numpy as np
import pytest

import pyoracle
import scenes_np
from ref_configs import REF_CONFIGS

FRAMES = 6
RAND_SEED = 2   # the seed the GPU tests use for every scene
POP = np.array([bin(v).count("1") for v in range(16)])
# BLOCK_OFFSETS of the reference (bmfr.cl:267-285)
OFFSETS = [(-14, -14), (4, -6), (-8, 14), (8, 0), (-10, -8), (2, 12), (12, -12), (-10, 0), (12, 14), (-8, -16),
           (6, 6), (-2, -2), (6, -14), (-16, 12), (14, -4), (-6, 4)]

# SHA-256 of frame 3 (planes, previous camera, jitter), seed RAND_SEED
DIGESTS = {
    ("pan", 128, 80): "03539cf5cb9eea3618a52f3607fb1290e2f122466046a63f83f0c5aa654a9142",
    ("far", 128, 80): "b1a434f9a965775e995943b72181b3a78c150d2b014e13ae17fdba255c6cdf4f",
    ("rand", 128, 80): "416b3d6ffe41775798b0401d1231b36ff1e3d1853084c0047fb8955090fea6bd",
    ("clamp", 100, 72): "461f9fd09caffc6d16d9119ede280d78056dc3ec6f137a4b4f000bb3f73e06c7",
    ("clamp_nan", 96, 64): "3c15eca1e5483d78877f26bd3a7a387d4dadaa9edb2c50e847421170a231b819",
}

_cache = {}


def oracle_frames(scene, name, still=False):
    key = (scene, name, still)
    if key not in _cache:
        rc = REF_CONFIGS[name]
        cfg = pyoracle.make_cfg(rc.width, rc.height, rc.not_scaled, rc.scaled, rc.half_tmp)
        _cache[key] = scenes_np.run_loop(pyoracle.OracleLoop(cfg), scene, rc.width, rc.height, FRAMES, RAND_SEED,
                                         still=still)
    return _cache[key]


def frame_digest(fr) -> str:
    h = hashlib.sha256()
    for k in ("noisy", "normals", "positions", "albedo"):
        h.update(fr[k].tobytes())
    h.update(np.asarray(fr["prev_vp"] + fr["jitter"], np.float32).tobytes())
    return h.hexdigest()


def popcount_shares(rec):
    return np.bincount(POP[rec["accept"]], minlength=5) / rec["accept"].size


def tmp_planes(rc, rec, frame):
    """tmp_data after accumulate_noisy_data as (B, MH, MW) f32 planes, and the
    image pixel (linear) each work-item of the margin grid holds
    (bmfr.cl:314-320: block offset, mirrored at the image edges)."""
    mw, mh = rc.margins
    B = rc.buffer_count
    t = rec["tmp_noisy"]
    t = t.view(np.float16).astype(np.float32) if t.dtype == np.uint16 else t
    planes = t.reshape(mh // 32, mw // 32, B, 32, 32).transpose(2, 0, 3, 1, 4).reshape(B, mh, mw)
    ox, oy = OFFSETS[frame % 16]

    def mirror(i, size):
        return np.where(i < 0, -i - 1, np.where(i >= size, 2 * size - i - 1, i))

    px = mirror(np.arange(mw) - 16 + ox, rc.width)
    py = mirror(np.arange(mh) - 16 + oy, rc.height)
    return planes, py[:, None] * rc.width + px[None, :]


@pytest.mark.parametrize("scene,W,H", list(DIGESTS))
def test_generator_is_deterministic(scene, W, H):
    a = scenes_np.frame(scene, W, H, 3, RAND_SEED)
    scenes_np._frame.cache_clear()
    b = scenes_np.frame(scene, W, H, 3, RAND_SEED)
    assert frame_digest(a) == frame_digest(b)
    assert frame_digest(a) == DIGESTS[(scene, W, H)]
    for k in ("noisy", "normals", "positions", "albedo"):
        assert a[k].dtype == np.float32 and a[k].shape == (W * H * 3,)
    # another seed / frame is another frame
    assert frame_digest(scenes_np.frame(scene, W, H, 3, RAND_SEED + 1)) != frame_digest(a)
    assert frame_digest(scenes_np.frame(scene, W, H, 4, RAND_SEED)) != frame_digest(a)


def test_region_is_a_cut_of_the_frame():
    W, H, reg = 128, 80, (24, 8, 72, 40)
    full = scenes_np.frame("rand", W, H, 2, RAND_SEED)
    cut = scenes_np.frame("rand", W, H, 2, RAND_SEED, region=reg)
    x0, y0, w, h = reg
    for k in ("noisy", "normals", "positions", "albedo"):
        want = full[k].reshape(H, W, 3)[y0:y0 + h, x0:x0 + w]
        assert cut[k].shape == (w * h * 3,) and cut[k].tobytes() == np.ascontiguousarray(want).tobytes()
    assert cut["prev_vp"] == full["prev_vp"] and cut["jitter"] == full["jitter"]


@pytest.mark.parametrize("scene", scenes_np.SCENES)
def test_inputs_stay_in_scope(scene):
    """Positions are finite in every scene; only clamp's patch has non-finite
    normals; noisy and albedo are finite and non-negative."""
    for W, H in ((128, 80), (100, 72)):
        for f in range(FRAMES):
            fr = scenes_np.frame(scene, W, H, f, RAND_SEED)
            assert np.isfinite(fr["positions"]).all()
            assert np.isfinite(fr["noisy"]).all() and (fr["noisy"] >= 0).all()
            assert np.isfinite(fr["albedo"]).all() and (fr["albedo"] > 0).all()
            bad = ~np.isfinite(fr["normals"]).reshape(H, W, 3).all(-1)
            if scene.startswith("clamp"):
                assert (bad == scenes_np.patch_mask(W, H, scenes_np.NAN_PATCH)).all()
            else:
                assert not bad.any()


@pytest.mark.parametrize("scene", ["pan", "far", "rand"])
def test_rays_and_matrix_are_mutual_inverses(scene):
    """Camera held still: every pixel reprojects to its own coordinate."""
    rc = REF_CONFIGS["s128x80_h13"]
    W, H = rc.width, rc.height
    for f, rec in enumerate(oracle_frames(scene, rc.name, still=True)[1:], 1):
        pp = rec["prev_pixel"].reshape(H, W, 2)
        assert np.abs(pp[..., 0] - np.arange(W)[None, :]).max() <= 1e-3, (scene, f)
        assert np.abs(pp[..., 1] - np.arange(H)[:, None]).max() <= 1e-3, (scene, f)


@pytest.mark.parametrize("name", ["s128x80_h13", "s128x80_f13", "s100x72_h16", "s96x64_f16", "s96x64_h7",
                                  "s80x64_h12"])
def test_rand_reaches_every_accept_mask(name):
    recs = oracle_frames("rand", name)
    masks = set()
    best = np.zeros(5)
    for rec in recs[1:]:
        masks |= set(np.unique(rec["accept"]).tolist())
        best = np.maximum(best, popcount_shares(rec))
    assert masks == set(range(16)), sorted(masks)
    assert (best >= 0.01).all(), best
    for rec in recs:
        assert np.isfinite(rec["weights"]).all() and np.isfinite(rec["result"]).all()


def test_pan_moves_fast_and_mixes_acceptance():
    rc = REF_CONFIGS["s128x80_h13"]
    W, H = rc.width, rc.height
    recs = oracle_frames("pan", rc.name)
    for f, rec in enumerate(recs[1:], 1):
        pp = rec["prev_pixel"].reshape(H, W, 2)
        assert np.median(np.abs(pp[..., 0] - np.arange(W)[None, :])) >= 10, f
        acc = rec["accept"]
        assert np.mean(acc == 0) >= 0.10, (f, np.mean(acc == 0))
        assert np.mean(acc == 15) >= 0.50, (f, np.mean(acc == 15))
        # taps beyond the leading edge: the newly revealed columns reproject past x = W going
        # right (frames 1-3), before x = -1 coming back
        assert pp[..., 0].max() >= W + 1 if f <= 3 else pp[..., 0].min() < -2
        assert np.isfinite(rec["result"]).all() and np.isfinite(rec["weights"]).all()
    assert int(recs[5]["spp"].max()) >= 5


@pytest.mark.parametrize("name", ["s128x80_h13", "s100x72_h16"])
def test_far_wall_is_near_the_bound_and_on_both_scale_arms(name):
    rc = REF_CONFIGS[name]
    recs = oracle_frames("far", name)
    for f in range(FRAMES):
        p = np.abs(scenes_np.frame("far", rc.width, rc.height, f, RAND_SEED)["positions"]).reshape(-1, 3)
        assert (p.max(0) >= 14.4).all() and p.min() >= 14.4 and p.max() <= 17.6, (p.min(0), p.max(0))
    for f, rec in enumerate(recs):
        mm = rec["mins_maxs"].reshape(-1, 2)
        rng = np.abs(mm[:, 1] - mm[:, 0])
        assert np.mean(rng > 1) >= 0.20 and np.mean(rng <= 1) >= 0.20, (f, np.mean(rng > 1))
        assert np.isfinite(rec["weights"]).all() and np.isfinite(rec["result"]).all()
        if f > 0:
            assert np.mean(rec["accept"] == 15) >= 0.90, (f, np.mean(rec["accept"] == 15))


@pytest.mark.parametrize("name", ["s128x80_h13", "s100x72_h16", "s96x64_h7", "s80x64_h12"])
def test_clamp_hits_the_guards_half_tmp(name):
    rc = REF_CONFIGS[name]
    W, H = rc.width, rc.height
    recs = oracle_frames("clamp", name)
    nan_px = np.flatnonzero(scenes_np.patch_mask(W, H, scenes_np.NAN_PATCH))
    share = []
    for f, rec in enumerate(recs):
        planes, pixel = tmp_planes(rc, rec, f)
        assert np.isfinite(planes).all(), f  # NaN -> 0 and the clamp leave nothing non-finite
        if name in ("s128x80_h13", "s100x72_h16"):
            assert int((np.abs(planes) == 65504).sum()) >= 100, (f, int((np.abs(planes) == 65504).sum()))
        elif any(c >= 7 for c in rc.scaled):  # a squared or cubed position among the features
            assert int((np.abs(planes) == 65504).sum()) > 0, f
        # rows the NaN guard zeroed: the wall's and the quad's normal.z is non-zero, the patch's is NaN
        hit = np.isin(pixel, nan_px)
        assert hit.sum() >= nan_px.size, (f, hit.sum())
        if 3 in rc.not_scaled:
            nz = rc.not_scaled.index(3)
            assert (planes[nz][hit] == 0).all() and (planes[nz][~hit] != 0).all(), f
        assert np.isfinite(rec["weights"]).all() and np.isfinite(rec["result"]).all(), f
        share.append(float(np.mean(~np.isfinite(rec["acc"]))))
        assert share[-1] <= 0.02, (f, share)
    assert share[5] <= share[1], share


@pytest.mark.parametrize("name", ["s128x80_f13", "s96x64_f16"])
def test_clamp_nan_holes_keep_f32_weights_finite(name):
    for f, rec in enumerate(oracle_frames("clamp_nan", name)):
        assert np.isfinite(rec["weights"]).all(), f
        assert np.isfinite(rec["result"]).all(), f


@pytest.mark.parametrize("scene,name", [("clamp", "s128x80_h13"), ("clamp", "s100x72_h16"), ("clamp", "s96x64_h7"),
                                        ("clamp", "s80x64_h12"), ("clamp_nan", "s128x80_f13"),
                                        ("clamp_nan", "s96x64_f16")])
def test_clamp_reprojection_stays_defined(scene, name):
    """The thrown strip (the quad's pixels at CUT_FRAME) lands within
    [1e6, 2^30) on both axes -- far enough for the float clamp of the
    reprojection to decide the tap index, inside what convert_int2_rtn
    defines -- and every reprojected coordinate of every frame is finite and
    below 2^30."""
    rc = REF_CONFIGS[name]
    W, H = rc.width, rc.height
    recs = oracle_frames(scene, name)
    for f, rec in enumerate(recs):
        pp = rec["prev_pixel"]
        assert np.isfinite(pp).all() and np.abs(pp).max() < 2.0 ** 30, (f, np.abs(pp).max())
    strip = scenes_np.quad_mask(scene, W, H, scenes_np.CUT_FRAME, RAND_SEED)
    assert strip.mean() >= 0.02
    pp = np.abs(recs[scenes_np.CUT_FRAME]["prev_pixel"].reshape(H, W, 2))
    assert pp[strip].min() >= 1e6 and pp[strip].max() < 2.0 ** 30, (pp[strip].min(), pp[strip].max())
    assert pp[~strip & (pp[..., 0] < 1e5)].size > 0  # the wall keeps its true reprojection
    assert (recs[scenes_np.CUT_FRAME]["accept"].reshape(H, W)[strip] == 0).all()
