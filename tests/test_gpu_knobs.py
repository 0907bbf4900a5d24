"""Parity away from the reference's default run-time parameters: noise_amount,
blend_alpha, second_blend_alpha, taa_blend_alpha, position_limit_squared and
normal_limit_squared (ref_configs.KNOB_REF_CONFIGS; tests/test_knobs_cpu.py
shows on the CPU oracle that each of them decides the result on this content).
Every other parity test runs at the defaults, where a constant folded into a
kernel, two alphas exchanged or the %g rule of the limits dropped would not
show.

Per configuration, bit for bit on every inter-stage buffer: stages (library
powr) == the reference's strict build compiled with the same values, stages ==
the CPU oracle; on the fused frame's planes: one launch, two launches, one
process_sequence call (both schedules) == stages; half input planes == the
widened planes == the reference on them; a second context fed the first one's
prev_frame_pixel plane under a NaN matrix (the plane-reading K1s, compiled
apart) == the first.  The tiled case of tests/test_gpu_content_parity.py with
the tight set on every context, as the single call and as interior + border.
No scene here holds NaN: the reference's records are asserted finite and the
comparison is strict.

k_lit: a normal limit of 1.0000049 reaches the reference kernel as the literal
1, which rejects every tap of content whose normals are 1.0000019 apart
(knob_util); the value cast to float would accept them all.

fast_fit: the state the fit does not feed bit for bit, and the worst frame's
relative L2 of the output against the reference's strict build (a) within
max(1e-4, 4 b), b the same distance of the reference's own default build --
the project's tolerance and the factor of the content tests, against the
reference's build-to-build distance on the same frames.  Both go to the
parity log as knobs_<config>.
"""
from __future__ import annotations

import pytest
import torch

import bmfr_amd
import knob_util
from parity_harness import Suite, bmfr_cfg, check_tiled_half_inputs, fused_state
from ref_configs import KNOB_REF_CONFIGS, knob_set_of
from seq_util import ALL_KEYS, FUSED_KEYS, TILE_FACTOR, TOL, assert_finite, compare_exact, rel_l2_finite, to_np

pytestmark = pytest.mark.gpu

NAMES = list(KNOB_REF_CONFIGS)
HALF_NAMES = ["k_tight_128x80_h13", "k_loose_100x72_h16"]
PLANE_NAMES = ["k_tight_128x80_h13", "k_ends_100x72_h16"]
# canonical feature lists (fast_fit's); k_lit adds nothing there: every tap is rejected
FAST_NAMES = [n for n in NAMES if n != "k_loose_96x64_h7" and knob_set_of(n) != "lit"]


def compare(got, ref, keys, where):
    assert_finite(ref, keys, where + " (reference)")
    compare_exact(got, ref, keys, where)  # the frame counts included


# a case is a configuration name; a missing reference build fails
SUITE = Suite(knob_util.frame, KNOB_REF_CONFIGS.get, missing_ref=pytest.fail)
need_ref, ref_frames, oracle_frames, stage_frames = (SUITE.need_ref, SUITE.ref_frames, SUITE.oracle_frames,
                                                     SUITE.stage_frames)
device_frames, fused_frames = SUITE.device_frames, SUITE.kept_fused_frames


@pytest.mark.parametrize("name", NAMES)
def test_stages_match_reference_strict(name, gpu):
    """library_powr: the reference kernel's own powr, so every buffer is pinned."""
    ref = ref_frames(name)
    compare(stage_frames(name, 1), ref, ALL_KEYS, f"HIP stages vs reference[{name}]")
    if knob_set_of(name) == "lit":  # the literal 1, not float(1.0000049): every tap rejected
        assert all((r["accept"] == 0).all() and (r["spp"] == 1).all() for r in ref)


@pytest.mark.parametrize("name", NAMES)
def test_stages_match_oracle(name, gpu):
    """Default (correctly rounded) powr: every buffer equals the CPU oracle's."""
    compare(stage_frames(name, 0), oracle_frames(name), ALL_KEYS, f"HIP stages vs oracle[{name}]")


@pytest.mark.parametrize("library_powr", [0, 1])
@pytest.mark.parametrize("name", NAMES)
def test_fused_frame_matches_stages(name, library_powr, gpu, monkeypatch):
    rc = KNOB_REF_CONFIGS[name]
    n = rc.width * rc.height
    keys = tuple(FUSED_KEYS)
    st = stage_frames(name, library_powr)
    compare(fused_frames(name, library_powr=library_powr), st, keys, f"one launch vs stages[{name}]")
    compare(fused_frames(name, profiled=True, library_powr=library_powr), st, keys, f"two launches vs stages[{name}]")
    frames = device_frames(name)
    for mode in ("fused", "streams"):
        if mode == "streams":
            monkeypatch.setenv("BMFR_SEQUENCE", "streams")
        else:
            monkeypatch.delenv("BMFR_SEQUENCE", raising=False)
        den = bmfr_amd.Denoiser(bmfr_cfg(rc, library_powr=library_powr))
        outs = [torch.empty(3 * n, device="cuda") for _ in range(rc.frames)]
        den.process_sequence([p for p, _, _ in frames], [(vp, jit) for _, vp, jit in frames], 0, outputs=outs)
        torch.cuda.synchronize()
        compare([{"result": to_np(o)} for o in outs], st, ("result",), f"sequence ({mode}) vs stages[{name}]")
        compare([fused_state(den, n)], st[-1:], keys, f"state after the sequence ({mode}) vs stages[{name}]")


@pytest.mark.parametrize("name", HALF_NAMES)
def test_half_inputs_match_widened_and_reference(name, gpu):
    keys = tuple(FUSED_KEYS)
    half = fused_frames(name, half_in=True, library_powr=1)
    wide = SUITE.fused_frames(name, half_in=True, widen=True, library_powr=1)  # the same Denoiser on the widened planes
    compare(half, wide, keys, f"half vs widened[{name}]")
    compare(half, ref_frames(name, "strict", half_in=True), keys, f"half vs reference on widened[{name}]")
    # the half path really read half planes
    assert half[-1]["result"].tobytes() != fused_frames(name, library_powr=1)[-1]["result"].tobytes()


@pytest.mark.parametrize("name", PLANE_NAMES)
def test_plane_reading_k1_replays_projection(name, gpu):
    """The pattern of tests/test_gpu_motion_input.py: the *_plane kernels are
    translation units of their own and read the same Params."""
    first = fused_frames(name, library_powr=0)
    compare(first, stage_frames(name, 0), tuple(FUSED_KEYS), f"one launch vs stages[{name}]")
    got = SUITE.fused_frames(name, replay=first)  # a NaN camera, first's prev_frame_pixel plane from frame 1 on
    compare(got, first, tuple(FUSED_KEYS), f"by plane vs by matrix[{name}]")


@pytest.mark.parametrize("split", [False, True], ids=["single", "interior_border"])
@pytest.mark.parametrize("scene", ["pan", "rand"])
@pytest.mark.parametrize("gx,gy", [(2, 1), (1, 2)], ids=["2x1", "1x2"])
def test_tiled_matches_untiled_at_tight_knobs(gx, gy, scene, split, gpu):
    """Untiled frames at these values are pinned by the tests above."""
    check_tiled_half_inputs(gx, gy, scene, split=split, **KNOB_REF_CONFIGS["k_tight_128x80_h13"].knobs())


@pytest.mark.parametrize("name", FAST_NAMES)
def test_fast_fit_within_tolerance(name, gpu, parity_log):
    need_ref(name, "default")
    fast = fused_frames(name, library_powr=1, fast_fit=1)
    strict, default = ref_frames(name, "strict"), ref_frames(name, "default")
    where = f"fast_fit[{name}]"
    e_fast = [rel_l2_finite(g["result"], r["result"], where) for g, r in zip(fast, strict)]
    e_builds = [rel_l2_finite(d["result"], r["result"], where) for d, r in zip(default, strict)]
    a, b = max(e_fast), max(e_builds)
    parity_log(f"knobs_{name}", {
        "config": name, "scene": knob_util.scene_of(name)[0], "frames": len(fast),
        "knobs": {k: float(v) for k, v in KNOB_REF_CONFIGS[name].knobs().items()},
        "fast_fit_vs_strict_worst_frame": float(f"{a:.3e}"), "default_vs_strict_worst_frame": float(f"{b:.3e}"),
        "fast_fit_vs_strict_per_frame": [float(f"{e:.3e}") for e in e_fast],
        "default_vs_strict_per_frame": [float(f"{e:.3e}") for e in e_builds]})
    print(f"{where}: worst frame vs strict a = {a:.3e}, reference default vs strict b = {b:.3e}, "
          f"bar {max(TOL, TILE_FACTOR * b):.3e}")
    # the fit does not feed these
    compare(fast, strict, ("noisy", "spp", "prev_pixel"), where)
    assert_finite(fast, ("result", "acc"), where)
    assert a <= max(TOL, TILE_FACTOR * b), (where, a, b)
