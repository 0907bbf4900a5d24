"""Parity on content the synthetic sequence cannot produce (tests/scenes_np.py;
tests/test_scenes_np.py shows on the CPU oracle what each scene reaches):

  pan    16 px/frame there and back: accept masks 0 / 15 and the mixed ones at
         the quad's edges, taps clamped at ix = -2 and ix = W + 1
  far    a flat wall with every coordinate near 16: collinear feature
         columns, both arms of scale() in one frame
  rand   all 16 accept masks, every popcount on >= 1 % of the pixels
  clamp  NaN normals (the NaN -> 0 guard of the design matrix), positions
         beyond half's range once squared / cubed (the +-65504 clamp, half
         tmp_data only), a reprojection thrown to |pf| ~ 1e7 (the float
         clamp before the tap index); f32 tmp_data runs clamp_nan, the
         variant without the out-of-range positions

at the sizes of REF_CONFIGS entries, so the CPU oracle and both builds of the
reference kernels exist; 6 frames each.

Exact path, bit for bit: stages == oracle, stages (library powr) ==
reference strict build, on every inter-stage buffer; the fused frame (one
launch, two launches, one process_sequence call) == stages; half input
planes == the widened planes == the reference on the widened planes.
clamp compares NaN-aware (same NaN positions, everything else bit for bit);
every other scene is asserted finite and compared strictly.

fast_fit: the frame output within relative L2 1e-4 of the reference's strict
and default builds per frame, the temporal state the fit does not feed bit
for bit, and a per-tile worst case: over every 32x32 image-aligned tile (at
most four fit blocks) and frame, the relative L2 against the strict build of
(a) fast_fit and (b) the reference's own default build; max (a) <= 4 max (b).
The yardstick is the reference's build-to-build distance on the same tiles,
the factor the largest ratio of the two at frame level in the project's
records rounded up (fast_fit 3.8e-5 in config 5 against 1.2e-5).  Both
maxima go to the parity log as content_<scene>_<case>
(profiles/content_parity.json).  One case misses the per-tile bar and is a
strict expected failure of that bar alone: far at B = 16 with half tmp_data
(KNOWN_TILE_MISS below has the figures and what is known of the cause).

Tiled half inputs: 320x256 as 2x1 and 1x2 tiles, halo 40, half input planes
cut from the generator's frame, exact path and fast_fit == the untiled
half-input frames bit for bit, the halo report clean, with pan's taps
crossing the internal tile edge in both directions.  A halo of 40 covers 6 px
of motion per frame (tile_halo - 34), so pan runs at a fifth of its speed
there (3.3 px/frame on the wall, up to 5.5 on the quad).
"""
from __future__ import annotations

import pytest
import torch

import bmfr_amd
import scenes_np
from parity_harness import Suite, bmfr_cfg, check_tiled_half_inputs
from ref_configs import REF_CONFIGS
from seq_util import (ALL_KEYS, FUSED_KEYS, TILE_FACTOR, TOL, assert_finite, compare_exact, compare_nan_aware,
                      rel_l2_finite, to_np, worst_tile)

pytestmark = pytest.mark.gpu

FRAMES = 6
SEED = 2   # tests/test_scenes_np.py asserts the coverage for this seed
CANONICAL = ("s128x80_h13", "s128x80_f13", "s100x72_h16", "s96x64_f16")
GENERIC = ("s96x64_h7", "s80x64_h12")
CASES = [(s, n) for s in ("pan", "far", "rand", "clamp") for n in CANONICAL] + \
        [(s, n) for s in ("rand", "clamp") for n in GENERIC]


def content(scene: str, name: str) -> str:
    """f32 tmp_data has no +-65504 clamp: it gets clamp without the out-of-range positions."""
    return "clamp_nan" if scene == "clamp" and not REF_CONFIGS[name].half_tmp else scene


def frame(case, f):
    scene, name = case
    rc = REF_CONFIGS[name]
    return scenes_np.frame(content(scene, name), rc.width, rc.height, f, SEED)


# a case is (scene, name); a missing reference build fails
SUITE = Suite(frame, lambda case: REF_CONFIGS[case[1]], FRAMES, missing_ref=pytest.fail)


def need_ref(name, mode="strict"):
    SUITE.need_ref((None, name), mode)


def ref_frames(scene, name, mode="strict", half_in=False):
    return SUITE.ref_frames((scene, name), mode, half_in)


def oracle_frames(scene, name):
    return SUITE.oracle_frames((scene, name))


def stage_frames(scene, name, library_powr):
    return SUITE.stage_frames((scene, name), library_powr)


def device_frames(scene, name, half_in=False):
    """Per frame: (planes on the device, previous camera, jitter)."""
    return SUITE.device_frames((scene, name), half_in)


def fused_frames(scene, name, **options):
    """The production frame path, frame by frame: one launch per frame, or
    (profiled: per-kernel events) K1 and K2 as two launches."""
    return SUITE.kept_fused_frames((scene, name), **options)


def compare(scene, got, ref, keys, where):
    if scene == "clamp":
        compare_nan_aware(got, ref, keys, where)
    else:
        assert_finite(ref, keys, where + " (reference)")
        compare_exact(got, ref, keys, where)


def ids(cases):
    return ["-".join(str(v) for v in c) for c in cases]


@pytest.mark.parametrize("scene,name", CASES, ids=ids(CASES))
def test_stages_match_oracle(scene, name, gpu):
    """Default (correctly rounded) powr: every buffer equals the CPU oracle's."""
    compare(scene, stage_frames(scene, name, 0), oracle_frames(scene, name), ALL_KEYS,
            f"HIP stages vs oracle[{scene} {name}]")


@pytest.mark.parametrize("scene,name", CASES, ids=ids(CASES))
def test_stages_match_reference_strict(scene, name, gpu):
    """library_powr: the reference kernel's own powr, so every buffer is pinned."""
    compare(scene, stage_frames(scene, name, 1), ref_frames(scene, name), ALL_KEYS,
            f"HIP stages vs reference[{scene} {name}]")


@pytest.mark.parametrize("library_powr", [0, 1])
@pytest.mark.parametrize("scene,name", CASES, ids=ids(CASES))
def test_fused_frame_matches_stages(scene, name, library_powr, gpu):
    rc = REF_CONFIGS[name]
    st = stage_frames(scene, name, library_powr)
    one = fused_frames(scene, name, library_powr=library_powr)
    two = fused_frames(scene, name, profiled=True, library_powr=library_powr)
    compare(scene, one, st, tuple(FUSED_KEYS), f"one launch vs stages[{scene} {name}]")
    compare(scene, two, st, tuple(FUSED_KEYS), f"two launches vs stages[{scene} {name}]")
    frames = device_frames(scene, name)
    den = bmfr_amd.Denoiser(bmfr_cfg(rc, library_powr=library_powr))
    outs = [torch.empty(3 * rc.width * rc.height, device="cuda") for _ in range(FRAMES)]
    den.process_sequence([p for p, _, _ in frames], [(vp, jit) for _, vp, jit in frames], 0, outputs=outs)
    torch.cuda.synchronize()
    compare(scene, [{"result": to_np(o)} for o in outs], [{"result": g["result"]} for g in one], ("result",),
            f"sequence vs per-frame[{scene} {name}]")


HALF_CASES = [(s, n) for s in ("pan", "rand", "clamp") for n in ("s128x80_h13", "s100x72_h16")]


@pytest.mark.parametrize("scene,name", HALF_CASES, ids=ids(HALF_CASES))
def test_half_inputs_match_widened_and_reference(scene, name, gpu):
    """Half input planes (the paired 12-byte tap loads) through every accept
    mask and the clamped off-image tap indices."""
    half = fused_frames(scene, name, half_in=True, library_powr=1)
    # the same Denoiser on the widened planes
    wide = SUITE.fused_frames((scene, name), half_in=True, widen=True, library_powr=1)
    compare(scene, half, wide, tuple(FUSED_KEYS), f"half vs widened[{scene} {name}]")
    compare(scene, half, ref_frames(scene, name, "strict", half_in=True), tuple(FUSED_KEYS),
            f"half vs reference on widened[{scene} {name}]")
    # the half path really read half planes
    f32 = fused_frames(scene, name, library_powr=1)
    assert half[-1]["result"].tobytes() != f32[-1]["result"].tobytes()


# (case id, reference configuration, half input planes): the configurations fast_fit supports
FAST = {"h13": ("s128x80_h13", False), "f13": ("s128x80_f13", False), "h16": ("s100x72_h16", False),
        "h16_in16": ("s100x72_h16", True)}
FAST_CASES = [(s, c) for s in ("pan", "far", "rand", "clamp") for c in FAST]
# The one case that misses a bar.  Measured on an MI355X: the per-frame bars hold (worst 1.58e-5 of
# the strict build, 1.68e-5 of the default build), the per-tile bar does not: fast_fit's worst tile
# is 7.64e-5 (frame 0, the 4-pixel-wide tile at x = 96, y = 64) against 1.78e-5 for the reference's
# own default build (frame 0, tile x = 0, y = 32) -- 4.3 x, the bar is 4 x.  What is known
# (tools/content_far_probe.py, profiles/content_far_probe.txt): the excess sits in the narrow tiles
# at the right image edge, which show one or two blocks where a full tile averages four, on every
# frame; the same wall, image and block grid with the positions 8 or 15 units nearer the origin
# stay at 1-2e-5 in every tile, as do B = 13 and a width that is a multiple of 32 -- so it follows
# the magnitude of the position values (x^3 ~ 5000 in half tmp_data), not a pixel or block index:
# rounding in fast_fit's arithmetic, not its logic.  Which operation carries it was not isolated;
# the exact path's own response to one-ulp changes of the noisy input is not raised in those tiles.
# With half input planes the reference's two builds are themselves 1.03e-4 apart on a tile of this scene.
# Against the float64 least-squares fit (tests/test_gpu_fit_f64.py, case far-100x72_h16, frame 0,
# profiles/fit_f64.json; second_blend_alpha = 1 there, the same design matrix at frame 0), the four
# blocks that cover this tile, (3,2), (4,2), (3,3), (4,3) of the 5-wide block grid with 1024, 64, 192 and
# 12 in-image pixels: the reference is 7.98e-4, 8.16e-4, 1.18e-3 and 1.60e-3 from the true fit, fast_fit
# 7.90e-4, 3.37e-4, 1.19e-3 and 1.62e-3.  Both are ten to twenty times further from the truth than the
# 7.6e-5 between them, and fast_fit is not further from the true fit there than the reference is (within
# 1.3 % of it on three of the blocks, 2.4 x nearer on the fourth): on this tile it is different, not
# less accurate, and the yardstick of this xfail, the distance between the reference's two builds, says
# nothing about accuracy.
KNOWN_TILE_MISS = {
    ("far", "h16"): "fast_fit's worst 32x32 tile 7.64e-5 of the strict build (frame 0, tile 96,64) against 1.78e-5 "
                    "between the reference's builds (frame 0, tile 0,32): 4.3 x, bar 4 x; per-frame 1.58e-5 / "
                    "1.68e-5, within 1e-4.  Follows the magnitude of the positions (gone 8 units nearer the "
                    "origin, same image and blocks): inherent in fast_fit's arithmetic at B = 16 with half "
                    "tmp_data near the 16-unit bound"}


class TileBarMissed(AssertionError):
    """The per-tile bar alone: the expected failure covers nothing else."""


FAST_PARAMS = [pytest.param(*c, id="-".join(c), marks=[pytest.mark.xfail(strict=True, raises=TileBarMissed,
                                                                         reason=KNOWN_TILE_MISS[c])]
                            if c in KNOWN_TILE_MISS else []) for c in FAST_CASES]


@pytest.mark.parametrize("scene,case", FAST_PARAMS)
def test_fast_fit_within_tolerance(scene, case, gpu, parity_log):
    name, half_in = FAST[case]
    rc = REF_CONFIGS[name]
    W, H = rc.width, rc.height
    need_ref(name, "default")
    fast = fused_frames(scene, name, half_in=half_in, library_powr=1, fast_fit=1)
    strict = ref_frames(scene, name, "strict", half_in)
    default = ref_frames(scene, name, "default", half_in)
    where = f"fast_fit[{scene} {case}]"
    e_strict = [rel_l2_finite(g["result"], r["result"], where) for g, r in zip(fast, strict)]
    e_default = [rel_l2_finite(g["result"], r["result"], where) for g, r in zip(fast, default)]
    builds = [rel_l2_finite(d["result"], r["result"], where) for d, r in zip(default, strict)]
    tile_fast, tile_builds = worst_tile(fast, strict, W, H), worst_tile(default, strict, W, H)
    parity_log(f"content_{scene}_{case}", {
        "scene": content(scene, name), "config": name, "input_half": int(half_in), "frames": FRAMES,
        "fast_fit_vs_strict_per_frame": [float(f"{e:.3e}") for e in e_strict],
        "fast_fit_vs_default_per_frame": [float(f"{e:.3e}") for e in e_default],
        "default_vs_strict_per_frame": [float(f"{e:.3e}") for e in builds],
        "worst_tile_fast_fit": {"rel_l2": float(f"{tile_fast[0]:.3e}"), "frame": tile_fast[1],
                                "tile": list(tile_fast[2:])},
        "worst_tile_default_build": {"rel_l2": float(f"{tile_builds[0]:.3e}"), "frame": tile_builds[1],
                                     "tile": list(tile_builds[2:])}})
    print(f"{where}: frame worst vs strict {max(e_strict):.3e}, vs default {max(e_default):.3e}, builds "
          f"{max(builds):.3e}; tile worst fast {tile_fast}, builds {tile_builds}")
    # the fit does not feed these
    compare(scene, fast, strict, ("noisy", "spp", "prev_pixel"), where)
    if scene != "clamp":
        assert_finite(fast, ("result", "acc"), where)
    # the reference's default build is itself beyond 1e-4 of its strict build with B = 16 and half
    # tmp_data (tests/test_gpu_parity.py test_against_reference_default_build): that bar there
    bar_default = 1.5e-4 if rc.half_tmp and rc.buffer_count == 16 and max(builds) > TOL else TOL
    assert max(e_strict) <= TOL, (where, e_strict)
    assert max(e_default) <= bar_default, (where, e_default, bar_default)
    if not tile_fast[0] <= TILE_FACTOR * tile_builds[0]:
        raise TileBarMissed((where, tile_fast, tile_builds))


@pytest.mark.parametrize("fast_fit", [0, 1], ids=["exact", "fast_fit"])
@pytest.mark.parametrize("scene", ["pan", "rand"])
@pytest.mark.parametrize("gx,gy", [(2, 1), (1, 2)], ids=["2x1", "1x2"])
def test_tiled_half_inputs_match_untiled(gx, gy, scene, fast_fit, gpu):
    """Tiled contexts have non-zero plane origins and region-sized planes:
    the paired half tap loads there, against the untiled half-input frame."""
    check_tiled_half_inputs(gx, gy, scene, fast_fit=fast_fit)
