"""Caller-supplied feature planes (BMFR_FEATURE_AUX0..3, bmfr_aux_inputs,
include/bmfr.h) on the GPU (run on an MI355X: pytest -m gpu).

A. A plane that holds a named monomial's f32 values (numpy f32, one rounding
   per operation: nx, px * px, (px * px) * px) must reproduce the named code
   exactly.  library_powr = 0: the Denoiser run with the planes equals
   pyoracle.OracleLoop run with the named codes (the bar of
   test_gpu_parity.test_stage_kernels_match_oracle_bitwise); library_powr = 1:
   it equals this library's own named-code Denoiser run.  Byte equality of
   result, noisy, spp, acc and prev_pixel on every frame.  The clamp scenes
   put NaNs into the state, whose payload bits IEEE leaves open and the CPU
   and the GPU choose differently (tests/test_gpu_content_parity.py compares
   them NaN-aware for the named codes too): there the comparison with the CPU
   oracle asks for the same NaN positions and the same bits everywhere else,
   and the run is also held byte for byte to the library's own named-code run.

B. Content no named code expresses -- cross terms, albedo luminance, an
   object-id step plane --: the library equals tests/aux_np.AuxOracleLoop
   (pinned to the oracle by tests/test_aux_np.py) byte for byte.

Planes are compared as bytes."""
from __future__ import annotations

import functools

import pytest

import aux_np
import pyoracle
from parity_harness import device_frames, fused_frames
from ref_configs import REF_CONFIGS, RefConfig
from seq_util import FUSED_KEYS, compare_exact, compare_nan_aware

pytestmark = pytest.mark.gpu

KEYS = tuple(FUSED_KEYS)


@functools.lru_cache(maxsize=None)
def frames_of(source, W, H, frames):
    """Per frame: the frame dict (numpy) of aux_np.frame_source.  Shared, never modified."""
    src = aux_np.frame_source(source, W, H)
    return tuple(src(f) for f in range(frames))


def denoise(W, H, not_scaled, scaled, half, source, frames, names=(), library_powr=0, mode="frame", replay=None):
    """The Denoiser over the content, frame by frame -> per-frame state
    (parity_harness.fused_frames).  names: the aux planes' contents
    (aux_np.PLANES keys).  mode: "frame", "split" (_interior + _border) or
    "sequence" (one process_sequence call).  replay: the records of a run
    whose prev_frame_pixel planes replace the camera, which is then NaN."""
    rc = RefConfig(f"aux{W}x{H}", W, H, tuple(not_scaled), tuple(scaled), half)
    content = frames_of(source, W, H, frames)
    return fused_frames(rc, device_frames(content.__getitem__, frames, W, H, aux_names=names),
                        library_powr=library_powr, mode=mode, replay=replay)


@functools.lru_cache(maxsize=None)
def oracle_named(W, H, not_scaled, scaled, half, source, frames):
    cfg = pyoracle.make_cfg(W, H, not_scaled, scaled, half)
    return aux_np.run(pyoracle.OracleLoop(cfg), source, frames)


# ---------------------------------------------------------------- part A ----
def _ref_case(name, subs, names, frames=None, source="synth"):
    rc = REF_CONFIGS[name]
    return dict(W=rc.width, H=rc.height, not_scaled=rc.not_scaled, scaled=rc.scaled, half=rc.half_tmp,
                frames=frames or rc.frames, subs=subs, names=names, source=source)


# subs: {position in not_scaled + scaled: plane index}; names[k]: the monomial plane k holds
A_CASES = {
    # height padding, all 16 block offsets, mirrored margins, half tmp_data
    "h13_nx_px2": _ref_case("s128x80_h13", {1: 0, 7: 1}, ("nx", "px2")),
    # width padding 100 -> 128, B = 16, all four planes, named out of order (AUX2 first)
    "h16_four": _ref_case("s100x72_h16", {2: 2, 4: 0, 12: 3, 8: 1}, ("px", "py2", "ny", "pz3")),
    # f32 tmp_data, one scaled feature
    "f10_py": _ref_case("s96x64_f10", {5: 0}, ("py",)),
    # NS = 2, FS = 7: the three cubes
    "h12_cubes": _ref_case("s80x64_h12", {2: 0, 3: 1, 4: 2}, ("px3", "py3", "pz3")),
    # FS = 0
    "h7_nz": _ref_case("s64x64_h7", {3: 0}, ("nz",)),
    # the same plane twice: px not scaled and scaled == the named list (0, 1, 2, 4)(4, 5, 6, 7)
    "twice_px": dict(W=96, H=64, not_scaled=(0, 1, 2, 4), scaled=(4, 5, 6, 7), half=1, frames=4,
                     subs={3: 0, 4: 0}, names=("px",), source="synth"),
    # NaN normals (NaN -> 0 in tmp_data, raw in the weighted sum), f32 tmp_data
    "clamp_nan_f16": _ref_case("s96x64_f16", {3: 0, 7: 1, 11: 2}, ("nz", "px2", "py3"), 6, "clamp_nan"),
    # NaN normals and positions beyond half's range once squared / cubed (the +-65504 clamp)
    "clamp_h16": _ref_case("s100x72_h16", {3: 0, 7: 1, 11: 2}, ("nz", "px2", "py3"), 6, "clamp"),
}


def _lists(case):
    codes, was = aux_np.substitute(case["not_scaled"] + case["scaled"], case["subs"])
    for k, code in was.items():
        assert aux_np.CODE_OF[case["names"][k]] == code, (k, case["names"][k], code)
    ns = len(case["not_scaled"])
    return codes[:ns], codes[ns:]


@pytest.mark.parametrize("library_powr", [0, 1])
@pytest.mark.parametrize("case", list(A_CASES))
def test_monomial_planes_equal_named_codes(case, library_powr, gpu):
    c = A_CASES[case]
    ns, sc = _lists(c)
    size = (c["W"], c["H"])
    got = denoise(*size, ns, sc, c["half"], c["source"], c["frames"], c["names"], library_powr)
    nans = c["source"].startswith("clamp")
    if library_powr == 0:
        want = oracle_named(*size, c["not_scaled"], c["scaled"], c["half"], c["source"], c["frames"])
        (compare_nan_aware if nans else compare_exact)(got, want, KEYS, f"aux planes vs oracle, named codes [{case}]")
    if library_powr == 1 or nans:
        named = denoise(*size, c["not_scaled"], c["scaled"], c["half"], c["source"], c["frames"], (), library_powr)
        compare_exact(got, named, KEYS, f"aux planes vs named codes, library_powr {library_powr} [{case}]")


def test_with_prev_pixel_plane(gpu):
    """Aux planes together with prev_pixel=: context B (planes, NaN camera,
    the prev_frame_pixel plane context A computed from the named list by
    matrix) reproduces A and the oracle."""
    c = _ref_case("s128x80_h13", {1: 0, 7: 1}, ("nx", "px2"), 6, "pan")
    ns, sc = _lists(c)
    size = (c["W"], c["H"])
    a = denoise(*size, c["not_scaled"], c["scaled"], c["half"], "pan", 6)
    b = denoise(*size, ns, sc, c["half"], "pan", 6, c["names"], replay=a)
    compare_exact(b, a, KEYS, "aux planes + prev_pixel vs named codes by matrix")
    compare_exact(b, oracle_named(*size, c["not_scaled"], c["scaled"], c["half"], "pan", 6), KEYS,
                  "aux planes + prev_pixel vs oracle")


def test_sequence_equals_frames(gpu):
    c = A_CASES["h16_four"]
    ns, sc = _lists(c)
    per_frame = denoise(c["W"], c["H"], ns, sc, c["half"], c["source"], c["frames"], c["names"])
    outs, last = denoise(c["W"], c["H"], ns, sc, c["half"], c["source"], c["frames"], c["names"], mode="sequence")
    compare_exact(outs, per_frame, ("result",), "process_sequence outputs vs process_frame")
    compare_exact([last], [per_frame[-1]], KEYS, "process_sequence state vs process_frame")


def test_interior_border_equals_frame(gpu):
    c = A_CASES["f10_py"]
    ns, sc = _lists(c)
    whole = denoise(c["W"], c["H"], ns, sc, c["half"], c["source"], c["frames"], c["names"])
    split = denoise(c["W"], c["H"], ns, sc, c["half"], c["source"], c["frames"], c["names"], mode="split")
    compare_exact(split, whole, KEYS, "_interior + _border vs process_frame")


# ---------------------------------------------------------------- part B ----
@pytest.mark.parametrize("source", ["synth", "rand"])
@pytest.mark.parametrize("W,H,half", aux_np.NOVEL_SIZES)
def test_novel_planes_equal_the_composed_oracle(W, H, half, source, gpu):
    """px * py and nx * ny scaled, albedo luminance not scaled, an object-id
    step plane scaled (both arms of scale(): tests/test_aux_np.py)."""
    want = aux_np.novel_frames(W, H, half, source)
    got = denoise(W, H, aux_np.NOVEL_NOT_SCALED, aux_np.NOVEL_SCALED, half, source, aux_np.NOVEL_FRAMES,
                  aux_np.NOVEL_NAMES)
    compare_exact(got, want, KEYS, f"library vs AuxOracleLoop [{W}x{H} half={half} {source}]")
