"""Every generic feature-count kernel against the reference (run on an
MI355X: pytest -m gpu).

A feature list other than the two canonical ones runs through kernels
templated on the two counts: k_fitter<NS, FS, HALF>, k_fused_block<NS, FS,
HALF> and k_fused_block<NS, FS, HALF, AuxPlanes> (bmfr_generic.h), instantiated
for NS 1..4, FS 0..9 and both tmp_data precisions -- 240 kernels.  The sweep
(ref_configs.SHAPE_REF_CONFIGS; tests/test_shapes_cpu.py asserts what it
covers) has one configuration per (NS, FS, HALF) and three odd lists at
(3, 5) in each precision; every configuration's feature counts select exactly
one instantiation of each template, so over the sweep

  test_stage_kernels_match_*          launch the 80 k_fitter
  test_fused_frame_matches_stages_*   launch the 80 k_fused_block
  test_aux_kernel_equals_named        launch the 80 k_fused_block<.., AuxPlanes>

each on a 4 x 3 block grid for 3 frames of scene "rand".

Bars, those of tests/test_gpu_parity.py: the CPU oracle == the reference's
strict build bit for bit on EXACT_KEYS and within 4e-7 max(1, |ref|max) on
tone / result (powr); the stage kernels == the reference (library_powr = 1)
and == the oracle (default powr) bit for bit on every buffer, tmp_data after
the fit included; the fused frame == the stages byte for byte; the run with
features replaced by caller-supplied planes of the same f32 values == the
named run byte for byte.  tests/test_shapes_cpu.py shows every record finite,
so bytes are compared, never NaN-aware.

Feature counts outside the instantiated range (NS 0, NS 5, FS 10) pass
bmfr_config_sizes; every entry point must refuse them as
BMFR_ERROR_UNSUPPORTED before anything is enqueued.
"""
from __future__ import annotations

import ctypes as C

import numpy as np
import pytest
import torch

import aux_np
import bmfr_amd
import shape_util
from bmfr_amd import _lib
from bmfr_amd.pipeline import _Context, hip_memcpy_d2d
from parity_harness import Suite, to_device
from ref_configs import SHAPE_REF_CONFIGS
from seq_util import ALL_KEYS, EXACT_KEYS, FUSED_KEYS, PLANES, POWR_KEYS, compare_exact
from shape_util import NAMES

pytestmark = pytest.mark.gpu

UNSUPPORTED = 2
SPLIT_NAME = "g_n3s5_h"  # the split / sequence check: an NS = 3 shape
KEYS = tuple(FUSED_KEYS)

# a case is a configuration name; a missing reference build skips
SUITE = Suite(shape_util.frame, SHAPE_REF_CONFIGS.get, missing_ref=pytest.skip)
ref_frames, stage_frames = SUITE.ref_frames, SUITE.stage_frames


@pytest.fixture(scope="module", params=NAMES)
def name(request):
    """Module scope: pytest then runs a configuration's tests together, and
    its records (each pipeline run once) are dropped when it is done."""
    yield request.param
    SUITE.clear()
    shape_util.forget(request.param)


def fused_frames(name, library_powr, aux=False, mode="frame", keep=False):
    """The Denoiser over the configuration's frames -> per-frame state.  aux:
    the list of shape_util.aux_case, with its planes.  mode: "frame", "split"
    (_interior + _border) or "sequence" (one process_sequence call; ->
    (per-frame outputs, last state)).  keep: run once per configuration."""
    run = SUITE.kept_fused_frames if keep else SUITE.fused_frames
    return run(name, aux=aux, mode=mode, library_powr=library_powr)


# ------------------------------------------------------ the sweep, per name ----
def test_oracle_matches_reference_kernels(name, gpu):
    """Pins the CPU oracle to the reference itself at this shape."""
    ref = ref_frames(name)
    orc = shape_util.oracle_frames(name)
    compare_exact(orc, ref, EXACT_KEYS, f"oracle vs reference[{name}]")
    for f, (o, r) in enumerate(zip(orc, ref)):
        for k in POWR_KEYS:
            d = np.abs(o[k].astype(np.float64) - r[k])
            assert d.max() <= 4e-7 * max(1.0, float(np.abs(r[k]).max())), (name, f, k, d.max())


def test_stage_kernels_match_reference_bitwise(name, gpu):
    """k_fitter<NS, FS, HALF>; library_powr: the reference kernel's own powr,
    so every buffer is pinned, tmp_data as the fit leaves it included."""
    compare_exact(stage_frames(name, 1), ref_frames(name), ALL_KEYS, f"HIP stages vs reference[{name}]")


def test_stage_kernels_match_oracle_bitwise(name, gpu):
    compare_exact(stage_frames(name, 0), shape_util.oracle_frames(name), ALL_KEYS, f"HIP stages vs oracle[{name}]")


@pytest.mark.parametrize("library_powr", [0, 1])
def test_fused_frame_matches_stages_bitwise(name, library_powr, gpu):
    """k_fused_block<NS, FS, HALF>."""
    fused = fused_frames(name, library_powr, keep=True)
    compare_exact(fused, stage_frames(name, library_powr), KEYS, f"fused vs stages[{name} powr {library_powr}]")


@pytest.mark.parametrize("library_powr", [0, 1])
def test_aux_kernel_equals_named(name, library_powr, gpu):
    """k_fused_block<NS, FS, HALF, AuxPlanes>: the last feature and, where
    NS >= 2, the one at position 1 come from planes holding the monomial's f32
    values; state and output equal the named run's."""
    rc = SHAPE_REF_CONFIGS[name]
    not_scaled, scaled, aux_names = shape_util.aux_case(name)
    codes = not_scaled + scaled
    assert len(codes) == len(rc.not_scaled + rc.scaled) and codes[-1] >= aux_np.AUX0
    assert len(rc.not_scaled) < 2 or len(codes) == 2 or codes[1] >= aux_np.AUX0
    for k, nm in enumerate(aux_names):  # plane k holds the code it replaced
        if nm is not None:
            assert (rc.not_scaled + rc.scaled)[codes.index(aux_np.AUX0 + k)] == aux_np.CODE_OF[nm]
    named = fused_frames(name, library_powr, keep=True)
    compare_exact(fused_frames(name, library_powr, aux=True), named, KEYS, f"aux vs named[{name} powr {library_powr}]")


# ------------------------------------------- split and sequence at NS = 3 ----
@pytest.mark.parametrize("aux", [False, True], ids=["named", "aux"])
def test_interior_border_equals_frame(aux, gpu):
    whole = fused_frames(SPLIT_NAME, 0, aux=aux)
    split = fused_frames(SPLIT_NAME, 0, aux=aux, mode="split")
    compare_exact(split, whole, KEYS, "_interior + _border vs process_frame")


@pytest.mark.parametrize("schedule", ["fused", "streams"])
@pytest.mark.parametrize("aux", [False, True], ids=["named", "aux"])
def test_sequence_equals_frames(aux, schedule, gpu, monkeypatch):
    if schedule == "streams":
        monkeypatch.setenv("BMFR_SEQUENCE", "streams")
    else:
        monkeypatch.delenv("BMFR_SEQUENCE", raising=False)
    per_frame = fused_frames(SPLIT_NAME, 0, aux=aux)
    outs, last = fused_frames(SPLIT_NAME, 0, aux=aux, mode="sequence")
    compare_exact(outs, per_frame, ("result",), "process_sequence outputs vs process_frame")
    compare_exact([last], [per_frame[-1]], KEYS, "process_sequence state vs process_frame")


# ------------------------------- feature counts outside the instantiated range ----
W, H = 80, 48
OUTSIDE = {
    "ns0": ((), (4, 5, 6)),
    "ns0_fs10": ((), tuple(range(1, 11))),
    "ns5": ((0, 1, 2, 3, 4), ()),
    "ns5_fs6": ((0, 1, 2, 3, 4), (5, 6, 7, 8, 9, 10)),
    "ns1_fs10": ((0,), tuple(range(1, 11))),
    "ns3_fs10": ((0, 1, 2), tuple(range(3, 13))),
    # lists that name planes: the aux dispatch tables
    "ns5_aux": ((0, 1, 2, 3, _lib.FEATURE_AUX0), (4,)),
    "ns2_fs10_aux": ((0, 1), tuple(range(3, 12)) + (_lib.FEATURE_AUX2,)),
}
STATE = (("noisy_accumulated", 12), ("spp", 1), ("filtered_accumulated", 12), ("result", 12), ("prev_frame_pixel", 8),
         ("tone_mapped", 12))


def _state_ptrs(den):
    return [(nm, prev, getattr(den.state(bool(prev)), nm), W * H * bpp) for prev in (0, 1) for nm, bpp in STATE]


def _snapshot(den):
    out = {}
    for nm, prev, ptr, nbytes in _state_ptrs(den):
        t = torch.empty(nbytes, dtype=torch.uint8, device="cuda")
        hip_memcpy_d2d(t.data_ptr(), ptr, nbytes)
        out[(nm, prev)] = t
    torch.cuda.synchronize()
    return {k: v.cpu().numpy().tobytes() for k, v in out.items()}


@pytest.mark.parametrize("case", list(OUTSIDE))
def test_counts_outside_the_instantiated_range_are_unsupported(case, gpu):
    """The context exists (the counts pass bmfr_config_sizes), and every frame
    entry point returns BMFR_ERROR_UNSUPPORTED with the state planes (both
    slots, filled with a pattern first), the output and the caller's buffers
    untouched."""
    not_scaled, scaled = OUTSIDE[case]
    cfg = bmfr_amd.BmfrConfig(image_width=W, image_height=H, not_scaled=not_scaled, scaled=scaled)
    assert cfg.sizes().buffer_count == len(not_scaled) + len(scaled) + 3
    den = bmfr_amd.Denoiser(cfg)
    pattern = (torch.arange(W * H * 12, device="cuda", dtype=torch.int32) % 251).to(torch.uint8)
    for _, _, ptr, nbytes in _state_ptrs(den):
        assert ptr, "the generic path's planes are all allocated"
        hip_memcpy_d2d(ptr, pattern.data_ptr(), nbytes)
    before = _snapshot(den)
    fr = shape_util.frame("g_n1s0_h", 0)
    d = {k: to_device(fr[k]) for k in PLANES}
    keep = {k: v.clone() for k, v in d.items()}
    names_aux = any(c >= _lib.FEATURE_AUX0 for c in not_scaled + scaled)
    plane = torch.ones(W * H, device="cuda")
    p = lambda t: t.data_ptr()  # noqa: E731
    fi = _lib.FrameInputs(p(d["noisy"]), p(d["normals"]), p(d["positions"]), p(d["albedo"]), None, None, None)
    ax = _lib.AuxInputs((C.c_void_p * 4)(*[p(plane)] * 4))
    vp, jit = _lib.floats(fr["prev_vp"], 16), _lib.floats(fr["jitter"], 2)
    st = torch.cuda.current_stream().cuda_stream
    out = torch.full((W * H * 3,), 7.0, device="cuda")
    outs = (C.c_void_p * 1)(p(out))
    lib, h = den.lib, den.handle
    for fn in ("bmfr_process_frame", "bmfr_process_frame_interior", "bmfr_process_frame_border"):
        if not names_aux:  # a list that names planes refuses the call without them as an invalid argument
            assert getattr(lib, fn)(h, st, C.byref(fi), vp, jit, 0) == UNSUPPORTED, fn
        assert getattr(lib, fn + "_aux")(h, st, C.byref(fi), C.byref(ax), vp, jit, 0) == UNSUPPORTED, fn
    if not names_aux:
        assert lib.bmfr_process_sequence(h, st, 1, C.byref(fi), vp, jit, 0, outs) == UNSUPPORTED
    assert lib.bmfr_process_sequence_aux(h, st, 1, C.byref(fi), C.byref(ax), vp, jit, 0, outs) == UNSUPPORTED
    torch.cuda.synchronize()
    assert lib.bmfr_output(h) is None
    assert den.frame_status() == 0
    assert _snapshot(den) == before
    assert bool((out == 7.0).all())
    for k in PLANES:
        assert torch.equal(d[k], keep[k]), k


@pytest.mark.parametrize("case", [c for c in OUTSIDE if not c.endswith("aux")])
def test_fitter_stage_outside_the_range_is_unsupported(case, gpu):
    not_scaled, scaled = OUTSIDE[case]
    ctx = _Context(bmfr_amd.BmfrConfig(image_width=W, image_height=H, not_scaled=not_scaled, scaled=scaled))
    s = ctx.sizes
    fill = lambda nbytes: torch.full((nbytes // 4 + 1,), 3.0, device="cuda")  # noqa: E731
    tmp, w, mm = fill(s.tmp_data_bytes), fill(s.weights_bytes), fill(s.mins_maxs_bytes)
    st = torch.cuda.current_stream().cuda_stream
    for frame in (0, 1):
        assert ctx.lib.bmfr_fitter(ctx.handle, st, w.data_ptr(), mm.data_ptr(), tmp.data_ptr(), frame) == UNSUPPORTED
    torch.cuda.synchronize()
    for t in (tmp, w, mm):
        assert bool((t == 3.0).all())
    ctx.close()
