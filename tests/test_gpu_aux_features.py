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

import numpy as np
import pytest
import torch

import aux_np
import bmfr_amd
import pyoracle
from ref_configs import REF_CONFIGS

pytestmark = pytest.mark.gpu

KEYS = {"result": None, "noisy": "noisy_accumulated", "acc": "filtered_accumulated", "spp": "spp",
        "prev_pixel": "prev_frame_pixel"}
NAN_VP = [float("nan")] * 16
GARBAGE_JITTER = [float("nan"), 1e30]


def _dev(a):
    return torch.from_numpy(np.array(a, order="C")).cuda()  # a copy: generated planes may be read-only


def _state(den, n) -> dict:
    f32 = lambda m: torch.empty(m, device="cuda")  # noqa: E731
    out = {"result": den.copy_output(f32(3 * n))}
    for k, name in KEYS.items():
        if name is not None:
            out[k] = den.copy_state(name, torch.empty(n, dtype=torch.uint8, device="cuda") if k == "spp"
                                    else f32((2 if k == "prev_pixel" else 3) * n))
    torch.cuda.synchronize()
    return {k: v.cpu().numpy().copy() for k, v in out.items()}


@functools.lru_cache(maxsize=None)
def frames_of(source, W, H, frames):
    """Per frame: the frame dict (numpy) of aux_np.frame_source.  Shared, never modified."""
    src = aux_np.frame_source(source, W, H)
    return tuple(src(f) for f in range(frames))


def aux_of(names, fr, W, H):
    """The frame's aux planes on the device (None where not supplied)."""
    return [None if p is None else _dev(p)
            for p in aux_np.aux_planes(names, fr["normals"], fr["positions"], fr["albedo"], W, H)]


def denoise(W, H, not_scaled, scaled, half, source, frames, names=(), library_powr=0, mode="frame",
            prev_pixel=None):
    """The Denoiser over the content, frame by frame -> per-frame state.
    names: the aux planes' contents (aux_np.PLANES keys).  mode: "frame",
    "split" (_interior + _border) or "sequence" (one process_sequence call).
    prev_pixel: per-frame planes (numpy) that replace the camera, which is
    then NaN."""
    den = bmfr_amd.Denoiser(bmfr_amd.BmfrConfig(image_width=W, image_height=H, not_scaled=tuple(not_scaled),
                                                scaled=tuple(scaled), use_half_precision_in_tmp_data=half,
                                                library_powr=library_powr))
    n = W * H
    content = frames_of(source, W, H, frames)
    if mode == "sequence":
        fr_dev, cams, outs = [], [], []
        for fr in content:
            d = {k: _dev(fr[k]) for k in ("noisy", "normals", "positions", "albedo")}
            d["aux"] = aux_of(names, fr, W, H)
            fr_dev.append(d)
            cams.append((fr["prev_vp"], fr["jitter"]))
            outs.append(torch.empty(3 * n, device="cuda"))
        den.process_sequence(fr_dev, cams, 0, outputs=outs)
        torch.cuda.synchronize()
        assert den.frame_status() == 0
        return [{"result": o.cpu().numpy().copy()} for o in outs], _state(den, n)
    out = []
    for f, fr in enumerate(content):
        d = {k: _dev(fr[k]) for k in ("noisy", "normals", "positions", "albedo")}
        vp, jit, plane = fr["prev_vp"], fr["jitter"], None
        if prev_pixel is not None:
            vp, jit = NAN_VP, GARBAGE_JITTER
            plane = _dev(prev_pixel[f]) if f > 0 else torch.full((2 * n,), float("nan"), device="cuda")
        args = (d["noisy"], d["normals"], d["positions"], d["albedo"], vp, jit, f)
        kw = dict(prev_pixel=plane, aux=aux_of(names, fr, W, H))
        if mode == "split":
            den.process_frame_interior(*args, **kw)
            den.process_frame_border(*args, **kw)
        else:
            den.process_frame(*args, **kw)
        out.append(_state(den, n))
    assert den.frame_status() == 0
    return out


@functools.lru_cache(maxsize=None)
def oracle_named(W, H, not_scaled, scaled, half, source, frames):
    cfg = pyoracle.make_cfg(W, H, not_scaled, scaled, half)
    return aux_np.run(pyoracle.OracleLoop(cfg), source, frames)


def compare_bytes(got, want, where, keys=KEYS):
    for f, (g, w) in enumerate(zip(got, want)):
        for k in keys:
            if k not in g:
                continue
            a, b = np.frombuffer(g[k].tobytes(), np.uint8), np.frombuffer(w[k].tobytes(), np.uint8)
            assert a.size == b.size, (where, f, k, a.size, b.size)
            bad = np.flatnonzero(a != b)
            assert bad.size == 0, f"{where} frame {f} {k}: {bad.size} of {a.size} bytes differ, first at byte {bad[0]}"


def compare_nan_aware(got, want, where, keys=KEYS):
    """The same NaN positions, and the same bits everywhere else."""
    for f, (g, w) in enumerate(zip(got, want)):
        for k in keys:
            a, b = g[k].reshape(-1), w[k].reshape(-1)
            assert a.shape == b.shape and a.dtype == b.dtype, (where, f, k)
            if a.dtype != np.float32:
                assert (a == b).all(), (where, f, k)
                continue
            na, nb = np.isnan(a), np.isnan(b)
            assert (na == nb).all(), f"{where} frame {f} {k}: NaN at {int(na.sum())} vs {int(nb.sum())} places"
            bad = np.flatnonzero((a.view(np.uint32) != b.view(np.uint32)) & ~na)
            assert bad.size == 0, f"{where} frame {f} {k}: {bad.size} of {a.size} differ, first at {bad[:5]}"


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
        (compare_nan_aware if nans else compare_bytes)(got, want, f"aux planes vs oracle, named codes [{case}]")
    if library_powr == 1 or nans:
        named = denoise(*size, c["not_scaled"], c["scaled"], c["half"], c["source"], c["frames"], (), library_powr)
        compare_bytes(got, named, f"aux planes vs named codes, library_powr {library_powr} [{case}]")


def test_with_prev_pixel_plane(gpu):
    """Aux planes together with prev_pixel=: context B (planes, NaN camera,
    the prev_frame_pixel plane context A computed from the named list by
    matrix) reproduces A and the oracle."""
    c = _ref_case("s128x80_h13", {1: 0, 7: 1}, ("nx", "px2"), 6, "pan")
    ns, sc = _lists(c)
    size = (c["W"], c["H"])
    a = denoise(*size, c["not_scaled"], c["scaled"], c["half"], "pan", 6)
    b = denoise(*size, ns, sc, c["half"], "pan", 6, c["names"], prev_pixel=[r["prev_pixel"] for r in a])
    compare_bytes(b, a, "aux planes + prev_pixel vs named codes by matrix")
    compare_bytes(b, oracle_named(*size, c["not_scaled"], c["scaled"], c["half"], "pan", 6),
                  "aux planes + prev_pixel vs oracle")


def test_sequence_equals_frames(gpu):
    c = A_CASES["h16_four"]
    ns, sc = _lists(c)
    per_frame = denoise(c["W"], c["H"], ns, sc, c["half"], c["source"], c["frames"], c["names"])
    outs, last = denoise(c["W"], c["H"], ns, sc, c["half"], c["source"], c["frames"], c["names"], mode="sequence")
    compare_bytes(outs, per_frame, "process_sequence outputs vs process_frame", keys=("result",))
    compare_bytes([last], [per_frame[-1]], "process_sequence state vs process_frame")


def test_interior_border_equals_frame(gpu):
    c = A_CASES["f10_py"]
    ns, sc = _lists(c)
    whole = denoise(c["W"], c["H"], ns, sc, c["half"], c["source"], c["frames"], c["names"])
    split = denoise(c["W"], c["H"], ns, sc, c["half"], c["source"], c["frames"], c["names"], mode="split")
    compare_bytes(split, whole, "_interior + _border vs process_frame")


# ---------------------------------------------------------------- part B ----
@pytest.mark.parametrize("source", ["synth", "rand"])
@pytest.mark.parametrize("W,H,half", aux_np.NOVEL_SIZES)
def test_novel_planes_equal_the_composed_oracle(W, H, half, source, gpu):
    """px * py and nx * ny scaled, albedo luminance not scaled, an object-id
    step plane scaled (both arms of scale(): tests/test_aux_np.py)."""
    want = aux_np.novel_frames(W, H, half, source)
    got = denoise(W, H, aux_np.NOVEL_NOT_SCALED, aux_np.NOVEL_SCALED, half, source, aux_np.NOVEL_FRAMES,
                  aux_np.NOVEL_NAMES)
    compare_bytes(got, want, f"library vs AuxOracleLoop [{W}x{H} half={half} {source}]")
