"""The surface of the caller-supplied feature planes (BMFR_FEATURE_AUX0..3,
bmfr_aux_inputs, include/bmfr.h): configuration and host-side checks on
the CPU, status codes of the entry points on the GPU."""
from __future__ import annotations

import ctypes as C

import numpy as np
import pytest
import torch

import bmfr_amd
from bmfr_amd import _lib
from bmfr_amd.pipeline import aux_named, check_aux

INVALID_ARGUMENT, UNSUPPORTED = 1, 2
W, H = 96, 64
NOT_SCALED = (0, 1, 2, _lib.FEATURE_AUX1)
SCALED = (4, 5, 6, _lib.FEATURE_AUX3)


def _cfg(**kw):
    kw.setdefault("not_scaled", NOT_SCALED)
    kw.setdefault("scaled", SCALED)
    return bmfr_amd.BmfrConfig(image_width=W, image_height=H, **kw)


# ------------------------------------------------------------------- CPU ----
def test_codes_and_constants_follow_the_header():
    assert (_lib.FEATURE_AUX0, _lib.FEATURE_AUX1, _lib.FEATURE_AUX2, _lib.FEATURE_AUX3) == (13, 14, 15, 16)
    assert _lib.MAX_AUX_FEATURES == 4
    assert C.sizeof(_lib.AuxInputs) == _lib.MAX_AUX_FEATURES * C.sizeof(C.c_void_p)
    assert C.sizeof(_lib.FrameInputs) == 7 * C.sizeof(C.c_void_p)   # bmfr_frame_inputs did not grow


def test_aux_struct_matches_header():
    import os
    import subprocess
    import tempfile
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    src = '#include <stdio.h>\n#include "bmfr.h"\nint main(void){printf("%zu %d %d", sizeof(bmfr_aux_inputs), ' \
          'BMFR_MAX_AUX_FEATURES, BMFR_VERSION_MINOR);return 0;}\n'
    with tempfile.TemporaryDirectory() as d:
        c = os.path.join(d, "t.c")
        open(c, "w").write(src)
        exe = os.path.join(d, "t")
        subprocess.run(["gcc", "-I", os.path.join(root, "include"), c, "-o", exe], check=True)
        size, n, minor = map(int, subprocess.run([exe], capture_output=True, text=True, check=True).stdout.split())
    assert (size, n, minor) == (C.sizeof(_lib.AuxInputs), _lib.MAX_AUX_FEATURES, 3)


def test_config_sizes_accepts_16_rejects_17():
    lib = _lib.load()
    c = _lib.Config()
    s = _lib.Sizes()
    lib.bmfr_config_default(C.byref(c), W, H)
    for code in (13, 14, 15, 16):
        for slot in (0, 3, 4, 9):  # not-scaled and scaled, first and last
            lib.bmfr_config_default(C.byref(c), W, H)
            c.feature_buffers[slot] = code
            assert lib.bmfr_config_sizes(C.byref(c), C.byref(s)) == 0, (code, slot)
    for code in (17, -1):
        lib.bmfr_config_default(C.byref(c), W, H)
        c.feature_buffers[5] = code
        assert lib.bmfr_config_sizes(C.byref(c), C.byref(s)) == INVALID_ARGUMENT, code
    # the same plane more than once, and every feature a plane
    lib.bmfr_config_default(C.byref(c), W, H)
    for i in range(10):
        c.feature_buffers[i] = 13 + i % 4
    assert lib.bmfr_config_sizes(C.byref(c), C.byref(s)) == 0
    assert s.buffer_count == 13


def test_config_round_trips_aux_codes():
    cfg = _cfg()
    c = cfg.to_c()
    assert c.features_not_scaled == 4 and c.features_scaled == 4
    assert tuple(c.feature_buffers[:8]) == NOT_SCALED + SCALED
    assert aux_named(cfg) == (1, 3)
    assert aux_named(bmfr_amd.BmfrConfig(image_width=W, image_height=H)) == ()
    assert cfg.sizes().buffer_count == 11


def test_stage_pipeline_refuses_an_aux_list():
    with pytest.raises(ValueError, match="FEATURE_AUX"):
        bmfr_amd.StagePipeline(_cfg())


def test_check_aux_rejections():
    """On CPU tensors: every check but the last passes them, the device check
    then refuses them -- the wrong-device case."""
    named = (1, 3)
    ok = torch.zeros(H * W)
    # what the checks before the device check let through ends at the device check
    with pytest.raises(ValueError, match="cuda:0"):
        check_aux([None, ok, None, ok], named, W, H)
    with pytest.raises(ValueError, match="cuda:0"):
        check_aux([None, ok.reshape(H, W), None, ok], named, W, H)
    with pytest.raises(TypeError, match="float32"):
        check_aux([None, ok.double(), None, ok], named, W, H)
    with pytest.raises(TypeError, match="float32"):
        check_aux([None, ok.half(), None, ok], named, W, H)
    with pytest.raises(ValueError, match="elements"):
        check_aux([None, torch.zeros(H * W - 1), None, ok], named, W, H)
    with pytest.raises(ValueError, match="elements"):
        check_aux([None, torch.zeros(H * W * 3), None, ok], named, W, H)
    with pytest.raises(ValueError, match="contiguous"):
        check_aux([None, torch.zeros(H * W * 2)[::2], None, ok], named, W, H)
    with pytest.raises(ValueError, match="contiguous"):
        check_aux([None, torch.zeros(W, H).t(), None, ok], named, W, H)
    with pytest.raises(TypeError, match="torch tensor"):
        check_aux([None, np.zeros(H * W, np.float32), None, ok], named, W, H)
    # a plane the configuration names is missing
    for aux in (None, [], [None, ok], [None, None, None, ok], [ok, None, ok, None]):
        with pytest.raises(ValueError, match="missing"):
            check_aux(aux, named, W, H)
    with pytest.raises(ValueError, match="at most"):
        check_aux([ok] * 5, named, W, H)
    with pytest.raises(TypeError, match="sequence"):
        check_aux(ok, named, W, H)
    # nothing named: nothing needed, planes that are there are still checked
    assert check_aux(None, (), W, H) == (None,) * 4
    with pytest.raises(TypeError, match="float32"):
        check_aux([ok.double()], (), W, H)


# ------------------------------------------------------------------- GPU ----
def _frame(f):
    return {k: torch.from_numpy(np.ascontiguousarray(v)).cuda().reshape(-1)
            for k, v in bmfr_amd.synth_frame_host(W, H, f).items()}


def _camera(f):
    vp, _ = bmfr_amd.synth_camera(W, H, max(f - 1, 0))
    _, jit = bmfr_amd.synth_camera(W, H, f)
    return vp, jit


def _inputs(fr, prev, aux):
    """-> (bmfr_frame_inputs, bmfr_aux_inputs or None for aux = None)."""
    p = lambda t: None if t is None else t.data_ptr()  # noqa: E731
    fi = _lib.FrameInputs(p(fr["noisy"]), p(fr["normals"]), p(fr["positions"]), p(fr["albedo"]),
                          p(prev and prev["normals"]), p(prev and prev["positions"]), None)
    return fi, None if aux is None else _lib.AuxInputs((C.c_void_p * 4)(*[p(a) for a in aux]))


def _raw(den, fn, fr, prev, aux, f):
    """fn_aux with the planes; aux = None: a NULL bmfr_aux_inputs; aux = "plain": fn itself."""
    vp, jit = _camera(f)
    st = torch.cuda.current_stream().cuda_stream
    if aux == "plain":
        fi, _ = _inputs(fr, prev, None)
        return getattr(den.lib, fn)(den.handle, st, C.byref(fi), _lib.floats(vp, 16), _lib.floats(jit, 2), f)
    fi, ax = _inputs(fr, prev, aux)
    return getattr(den.lib, fn + "_aux")(den.handle, st, C.byref(fi), None if ax is None else C.byref(ax),
                                         _lib.floats(vp, 16), _lib.floats(jit, 2), f)


def _state(den):
    n = W * H
    names = (("noisy_accumulated", 3, torch.float32), ("spp", 1, torch.uint8), ("filtered_accumulated", 3, torch.float32),
             ("result", 3, torch.float32), ("prev_frame_pixel", 2, torch.float32))
    out = {nm: den.copy_state(nm, torch.empty(n * ch, dtype=dt, device="cuda")) for nm, ch, dt in names}
    torch.cuda.synchronize()
    return {k: v.cpu().numpy().tobytes() for k, v in out.items()}


def _planes(fr):
    """aux[1] = albedo's red channel, aux[3] = positions.x * positions.y."""
    a = fr["albedo"].reshape(-1, 3)
    p = fr["positions"].reshape(-1, 3)
    return [None, a[:, 0].contiguous(), None, (p[:, 0] * p[:, 1]).contiguous()]


@pytest.mark.gpu
def test_missing_plane_is_an_invalid_argument_and_leaves_state(gpu):
    den = bmfr_amd.Denoiser(_cfg())
    f0, f1 = _frame(0), _frame(1)
    # frame 0 without a named plane: refused, and the context has no frame yet
    assert _raw(den, "bmfr_process_frame", f0, None, [None, None, None, None], 0) == INVALID_ARGUMENT
    assert _raw(den, "bmfr_process_frame", f0, None, None, 0) == INVALID_ARGUMENT      # no bmfr_aux_inputs at all
    assert _raw(den, "bmfr_process_frame", f0, None, "plain", 0) == INVALID_ARGUMENT   # the call without planes
    assert _raw(den, "bmfr_process_frame", f0, None, [_planes(f0)[1], None, None, None], 0) == INVALID_ARGUMENT
    assert den.lib.bmfr_output(den.handle) is None
    assert _raw(den, "bmfr_process_frame", f0, None, _planes(f0), 0) == 0
    before = _state(den)
    for fn in ("bmfr_process_frame", "bmfr_process_frame_interior", "bmfr_process_frame_border"):
        assert _raw(den, fn, f1, f0, [None, _planes(f1)[1], None, None], 1) == INVALID_ARGUMENT, fn
        assert _raw(den, fn, f1, f0, "plain", 1) == INVALID_ARGUMENT, fn
    fi, ax = _inputs(f1, f0, [None, None, None, _planes(f1)[3]])
    vp, jit = _camera(1)
    st = torch.cuda.current_stream().cuda_stream
    assert den.lib.bmfr_process_sequence_aux(den.handle, st, 1, C.byref(fi), C.byref(ax), _lib.floats(vp, 16),
                                             _lib.floats(jit, 2), 1, None) == INVALID_ARGUMENT
    assert den.lib.bmfr_process_sequence(den.handle, st, 1, C.byref(fi), _lib.floats(vp, 16), _lib.floats(jit, 2), 1,
                                         None) == INVALID_ARGUMENT
    assert _state(den) == before
    # the frame that follows succeeds and equals a context that never saw the failed calls;
    # planes the list does not name are ignored
    junk = torch.full((7,), float("nan"), device="cuda")
    p1 = _planes(f1)
    assert _raw(den, "bmfr_process_frame", f1, f0, [junk, p1[1], junk, p1[3]], 1) == 0
    other = bmfr_amd.Denoiser(_cfg())
    other.process_frame(f0["noisy"], f0["normals"], f0["positions"], f0["albedo"], *_camera(0), 0, aux=_planes(f0))
    other.process_frame(f1["noisy"], f1["normals"], f1["positions"], f1["albedo"], *_camera(1), 1, aux=p1)
    assert _state(den) == _state(other)
    assert den.frame_status() == 0


@pytest.mark.gpu
def test_stage_calls_on_an_aux_context_are_unsupported(gpu):
    from bmfr_amd.pipeline import _Context
    ctx = _Context(_cfg())
    s = ctx.sizes
    buf = torch.zeros(max(s.tmp_data_bytes, s.image_bytes) // 4 + 16, device="cuda")
    p, st = buf.data_ptr(), torch.cuda.current_stream().cuda_stream
    vp, jit = _camera(0)
    assert ctx.lib.bmfr_accumulate_noisy_data(ctx.handle, st, p, p, p, p, p, p, p, p, p, p, p, _lib.floats(vp, 16),
                                              _lib.floats(jit, 2), 0) == UNSUPPORTED
    assert ctx.lib.bmfr_weighted_sum(ctx.handle, st, p, p, p, p, p, p, 0) == UNSUPPORTED
    # the fitter reads only tmp_data: it runs (on a zero matrix here)
    w = torch.zeros(s.weights_bytes // 4, device="cuda")
    mm = torch.zeros(s.mins_maxs_bytes // 4, device="cuda")
    assert ctx.lib.bmfr_fitter(ctx.handle, st, w.data_ptr(), mm.data_ptr(), p, 0) == 0
    torch.cuda.synchronize()
    ctx.close()


@pytest.mark.gpu
@pytest.mark.parametrize("kw", [dict(tile=(0, 0, 48, 64), tile_halo=34), dict(input_half=1)], ids=["tiled", "input_half"])
def test_aux_list_on_tiled_or_half_input_context_is_unsupported(kw, gpu):
    """As a non-canonical named list is today."""
    f0 = _frame(0)
    for lists in (dict(), dict(not_scaled=(0, 1, 2, 3), scaled=(4, 5, 6))):  # an aux list, a named non-canonical one
        den = bmfr_amd.Denoiser(_cfg(**kw, **lists))
        for fn in ("bmfr_process_frame", "bmfr_process_frame_interior"):
            assert _raw(den, fn, f0, None, _planes(f0), 0) == UNSUPPORTED, (fn, lists)
