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

import numpy as np
import pytest
import torch

import bmfr_amd
import knob_util
import pyoracle
import ref_run
from ref_configs import KNOB_REF_CONFIGS, knob_set_of
from seq_util import ALL_KEYS, compare_exact, to_np
from test_gpu_content_parity import (FUSED_KEYS, PLANES, TILE_FACTOR, TOL, _dev, assert_finite, cached,
                                     check_tiled_half_inputs, fused_state, need_ref, rel_l2_finite, through_half)
from test_gpu_motion_input import GARBAGE_JITTER, NAN_VP

pytestmark = pytest.mark.gpu

NAMES = list(KNOB_REF_CONFIGS)
HALF_NAMES = ["k_tight_128x80_h13", "k_loose_100x72_h16"]
PLANE_NAMES = ["k_tight_128x80_h13", "k_ends_100x72_h16"]
# canonical feature lists (fast_fit's); k_lit adds nothing there: every tap is rejected
FAST_NAMES = [n for n in NAMES if n != "k_loose_96x64_h7" and knob_set_of(n) != "lit"]


def bmfr_cfg(rc, **kw) -> bmfr_amd.BmfrConfig:
    return bmfr_amd.BmfrConfig(image_width=rc.width, image_height=rc.height, not_scaled=rc.not_scaled,
                               scaled=rc.scaled, use_half_precision_in_tmp_data=rc.half_tmp, **rc.knobs(), **kw)


def compare(got, ref, keys, where):
    assert_finite(ref, keys, where + " (reference)")
    assert len(got) == len(ref), (where, len(got), len(ref))
    compare_exact(got, ref, keys, where)


def ref_frames(name, mode="strict", half_in=False):
    need_ref(name, mode)
    return cached((name, "ref", mode, half_in), lambda: knob_util.run_loop(
        ref_run.RefLoop(KNOB_REF_CONFIGS[name], mode), name, to_device=_dev, sync=torch.cuda.synchronize,
        prepare=through_half if half_in else None))


def oracle_frames(name):
    rc = KNOB_REF_CONFIGS[name]
    cfg = pyoracle.make_cfg(rc.width, rc.height, rc.not_scaled, rc.scaled, rc.half_tmp, **rc.knobs())
    return cached((name, "oracle"), lambda: knob_util.run_loop(pyoracle.OracleLoop(cfg), name))


def stage_frames(name, library_powr):
    rc = KNOB_REF_CONFIGS[name]
    return cached((name, "stages", library_powr), lambda: knob_util.run_loop(
        bmfr_amd.StagePipeline(bmfr_cfg(rc, library_powr=library_powr)), name, to_device=_dev,
        sync=torch.cuda.synchronize))


def device_frames(name, half_in=False):
    """Per frame: (planes on the device, previous camera, jitter)."""
    def make():
        out = []
        for f in range(KNOB_REF_CONFIGS[name].frames):
            fr = knob_util.frame(name, f)
            planes = {k: _dev(fr[k].astype(np.float16) if half_in else fr[k]) for k in PLANES}
            out.append((planes, fr["prev_vp"], fr["jitter"]))
        return out
    return cached((name, "device", half_in), make)


def fused_frames(name, profiled=False, half_in=False, **kw):
    """The production frame path, frame by frame: one launch per frame, or
    (profiled: per-kernel events) K1 and K2 as two launches."""
    rc = KNOB_REF_CONFIGS[name]

    def make():
        den = bmfr_amd.Denoiser(bmfr_cfg(rc, input_half=int(half_in), **kw))
        if profiled:
            den.set_profiling(True, capacity=rc.frames, stride=1)
        out = []
        for f, (p, vp, jit) in enumerate(device_frames(name, half_in)):
            den.process_frame(p["noisy"], p["normals"], p["positions"], p["albedo"], vp, jit, f)
            out.append(fused_state(den, rc.width * rc.height))
        return out
    return cached((name, "fused", profiled, half_in, tuple(sorted(kw.items()))), make)


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
    rc = KNOB_REF_CONFIGS[name]
    keys = tuple(FUSED_KEYS)
    half = fused_frames(name, half_in=True, library_powr=1)
    den = bmfr_amd.Denoiser(bmfr_cfg(rc, library_powr=1))  # the same Denoiser on the widened planes
    wide = []
    for f, (p, vp, jit) in enumerate(device_frames(name, half_in=True)):
        w = {k: v.float() for k, v in p.items()}
        den.process_frame(w["noisy"], w["normals"], w["positions"], w["albedo"], vp, jit, f)
        wide.append(fused_state(den, rc.width * rc.height))
    compare(half, wide, keys, f"half vs widened[{name}]")
    compare(half, ref_frames(name, "strict", half_in=True), keys, f"half vs reference on widened[{name}]")
    # the half path really read half planes
    assert half[-1]["result"].tobytes() != fused_frames(name, library_powr=1)[-1]["result"].tobytes()


@pytest.mark.parametrize("name", PLANE_NAMES)
def test_plane_reading_k1_replays_projection(name, gpu):
    """The pattern of tests/test_gpu_motion_input.py: the *_plane kernels are
    translation units of their own and read the same Params."""
    rc = KNOB_REF_CONFIGS[name]
    n = rc.width * rc.height
    first = fused_frames(name, library_powr=0)
    compare(first, stage_frames(name, 0), tuple(FUSED_KEYS), f"one launch vs stages[{name}]")
    den = bmfr_amd.Denoiser(bmfr_cfg(rc))
    nan_plane = torch.full((2 * n,), float("nan"), device="cuda")  # frame 0 ignores the plane
    got = []
    for f, (p, _, _) in enumerate(device_frames(name)):
        plane = nan_plane if f == 0 else torch.from_numpy(first[f]["prev_pixel"].copy()).cuda()
        den.process_frame(p["noisy"], p["normals"], p["positions"], p["albedo"], NAN_VP, GARBAGE_JITTER, f,
                          prev_pixel=plane)
        got.append(fused_state(den, n))
    assert den.frame_status() == 0
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
