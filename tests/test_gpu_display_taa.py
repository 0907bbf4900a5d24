"""The display-resolution TAA on the GPU (bmfr_display_taa, include/bmfr.h;
Denoiser.display_taa): the kernel against the numpy restatement
(tests/display_taa_np.py) byte for byte on the CPU test's nasty content, every
byte of `result` and `dst` it must not write still holding its sentinel; the
anchor to the reference-pinned K2 (the same TAA, run by the library itself at
trace resolution); a twelve-frame loop frame -> upsample -> display TAA against
the restatements; the untouched state and inputs; and every error."""
from __future__ import annotations

import ctypes as C
import functools
import itertools

import numpy as np
import pytest
import torch

import bmfr_amd
from bmfr_amd import _lib
import display_taa_np as dn
import resolve_np as rn
import scenes_np
import upsample_np as un
from parity_harness import assert_same_array, state_snapshot
from test_gpu_resolve import ALPHA, LAYOUTS, Surface, _cfg, _compare

pytestmark = pytest.mark.gpu

F32 = np.float32
# The smallest sizes at which the tile tails (64 x 16, four rows per thread), the one-pixel ring and the
# image border can go wrong: single pixels and rows, one tile, one pixel past a tile in x / several rows
# short of three in y (65 x 47), past two and three tiles (129, 193), a tall frame (67 x 131: one row and
# three rows past a thread's four, nine tiles down).
SIZES = [(1, 1), (2, 1), (5, 3), (32, 32), (65, 47), (129, 53), (193, 53), (67, 131)]
ONE = (65, 47)
PLANE_FORMATS = {"f32x3": rn.F32X3, "f16x4": rn.F16X4}
# previous position: prev_pixel, or motion (dtype, at the pixel centre, scale, pixel_offset)
MODES = {"prev_pixel": None, "motion_f32": (F32, False, (1.0, -0.5), (0.5, 0.5)),
         "motion_f32_centre": (F32, True, (0.75, 1.0), (0.3125, 0.8125)),
         "motion_f16": (np.float16, False, (1.5, 1.0), (0.5, 0.5)),
         "motion_f16_centre": (np.float16, True, (1.0, 1.0), (0.3125, 0.8125))}
BLEND = 0.2


@functools.lru_cache(maxsize=None)
def _den():
    """Any small context: it only names the device.  No frame is ever processed on it."""
    return bmfr_amd.Denoiser(_cfg(32, 32))


@functools.lru_cache(maxsize=None)
def _content(Wd, Hd):
    return dn.nasty_content(Wd, Hd, 31 + Wd)


def _plane(fmt, Wd, Hd, padded=0, shifted=0, fill=None) -> Surface:
    """A display plane inside a sentinel-filled buffer (test_gpu_resolve.Surface);
    padded: rows one element apart from packed; shifted: element-aligned, off a
    16-byte boundary."""
    s = Surface(fmt, Wd, Hd, rn.ALIGN[fmt] * padded, rn.ALIGN[fmt] * shifted)
    if shifted:
        assert s.tensor.data_ptr() % 16 != 0
    if fill is not None:
        s.tensor.copy_(torch.from_numpy(fill).cuda())
    return s


def _flat(a: np.ndarray, shifted=0) -> torch.Tensor:
    """A prev_pixel / motion plane on the device; shifted: one entry (two
    elements) into a larger allocation: element-aligned, off a 16-byte boundary."""
    t = torch.from_numpy(np.ascontiguousarray(a).reshape(-1)).cuda()
    if shifted:
        big = torch.empty(t.numel() + 2, dtype=t.dtype, device="cuda")
        big[2:].copy_(t)
        t = big[2:]
        assert t.data_ptr() % 16 != 0
    return t


def _run(Wd, Hd, cur="f32x3", hist="f32x3", res="f32x3", mode="prev_pixel", dst=None, bgr=False, flip=False,
         layout=(0, 0, 0), planes=(0, 0), reset=False, no_history=False, blend=BLEND, what=None):
    """One call into sentinel-filled result and dst against the restatement;
    current and history must come back as they went in."""
    den, c = _den(), _content(Wd, Hd)
    what = what or (Wd, Hd, cur, hist, res, mode, dst, bgr, flip, layout, planes, reset, no_history)
    fc, fh, fr = PLANE_FORMATS[cur], PLANE_FORMATS[hist], PLANE_FORMATS[res]
    padded, shifted = planes
    cur_np, hist_np = dn.as_plane(c["current"], fc, 1), dn.as_plane(c["history"], fh, 2)
    pc = _plane(fc, Wd, Hd, padded, shifted, cur_np)
    ph = None if no_history else _plane(fh, Wd, Hd, padded, shifted, hist_np)
    pr = _plane(fr, Wd, Hd, padded, shifted)
    kw, pos = {}, {}
    if MODES[mode] is None:
        pos["prev_pixel"] = c["prev_pixel"]
        kw["prev_pixel"] = _flat(c["prev_pixel"], shifted)
    else:
        dt, centre, scale, offset = MODES[mode]
        pos = dict(motion=c["motion"] if dt is F32 else rn.to_half(c["motion"]), motion_scale=scale, at_centre=centre,
                   pixel_offset=offset)
        kw = dict(motion=_flat(pos["motion"], shifted), motion_scale=scale, motion_at_pixel_centre=centre,
                  pixel_offset=offset)
    surface, origin = None, (0, 0)
    if dst is not None:
        f = rn.FORMATS[dst]
        pad_s, shift_s, larger = layout
        pad = {rn.UNORM8X3: 1, rn.F16X4: 8}.get(f, 4)
        surface = Surface(f, Wd + 8 * larger, Hd + 8 * larger, pad * pad_s, rn.ALIGN[f] * shift_s)
        origin = (5, 3) if larger else (0, 0)
        kw.update(dst=surface.tensor, origin=origin, flip_y=flip, bgr=bgr, alpha=ALPHA)
    before = (pc.host(), None if ph is None else ph.host())
    den.display_taa(pc.tensor, pr.tensor, history=None if ph is None else ph.tensor, blend_alpha=blend, reset=reset, **kw)
    v = dn.display_taa(cur_np, None if no_history else hist_np, dn.previous_position(Wd, Hd, **pos), blend, reset=reset)
    want = dn.result_plane(v, fr)
    pixels = np.ascontiguousarray(want).view(np.uint8).reshape(Hd, Wd, rn.BPP[fr])
    _compare(pr.host(), rn.place(pr.expected(), pr.off, pr.pitch, fr, pixels, (0, 0, Wd, Hd), Hd), fr, pr.off,
             (what, "result"), nan_in=True)
    if surface is not None:
        f = surface.fmt
        expect = rn.place(surface.expected(), surface.off, surface.pitch, f, dn.surface_pixels(v, f, bgr, ALPHA),
                          (0, 0, Wd, Hd), Hd, origin, flip)
        _compare(surface.host(), expect, f, surface.off, (what, "dst"), nan_in=True)
    assert_same_array(pc.host(), before[0], (what, "current"))
    if ph is not None:
        assert_same_array(ph.host(), before[1], (what, "history"))
    return v


@pytest.mark.parametrize("Wd,Hd", [s for s in SIZES if s != ONE])
def test_kernel_equals_restatement_at_every_size(Wd, Hd, gpu):
    v = _run(Wd, Hd, "f16x4", "f16x4", "f16x4", "motion_f16_centre", dst="unorm8x4", what=(Wd, Hd, "engine formats"))
    _run(Wd, Hd, "f32x3", "f16x4", "f32x3", "prev_pixel", dst="f32x3", flip=True, layout=(1, 1, 1), planes=(1, 1),
         what=(Wd, Hd, "f32, padded, shifted"))
    if Wd * Hd > 100:   # both arms of the off-screen test, and the specials, reach the result
        assert np.isnan(v).any() and np.isfinite(v).any()
        me = dn.values(dn.as_plane(_content(Wd, Hd)["current"], rn.F16X4, 1))
        passed = (v == me).all(axis=-1)
        assert passed.any() and not passed.all()
    assert _den().frame_status() == 0


@pytest.mark.parametrize("res", list(PLANE_FORMATS))
@pytest.mark.parametrize("hist", list(PLANE_FORMATS))
@pytest.mark.parametrize("cur", list(PLANE_FORMATS))
def test_every_plane_format_and_previous_position_source(cur, hist, res, gpu):
    Wd, Hd = ONE
    for k, mode in enumerate(MODES):
        _run(Wd, Hd, cur, hist, res, mode, dst=("unorm10x3a2", "f16x4", None)[k % 3], bgr=bool(k & 1))


@pytest.mark.parametrize("dst", list(rn.FORMATS))
def test_every_surface_format_and_switch(dst, gpu):
    Wd, Hd = ONE
    for k, (bgr, flip) in enumerate(itertools.product((False, True), (False, True))):
        _run(Wd, Hd, "f16x4", "f32x3", "f16x4", list(MODES)[k], dst=dst, bgr=bgr, flip=flip)
    for layout in LAYOUTS:
        _run(Wd, Hd, "f32x3", "f16x4", "f16x4", "prev_pixel", dst=dst, flip=bool(layout[2]), layout=layout)


@pytest.mark.parametrize("planes", [(1, 0), (0, 1), (1, 1)], ids=["padded", "shifted", "padded+shifted"])
def test_padded_pitches_and_planes_off_a_16_byte_boundary(planes, gpu):
    Wd, Hd = ONE
    for cur, hist, res in itertools.product(PLANE_FORMATS, repeat=3):
        _run(Wd, Hd, cur, hist, res, "motion_f16" if cur == res else "prev_pixel", dst=None if cur == hist else "unorm8x3",
             planes=planes)


@pytest.mark.parametrize("fmt", list(PLANE_FORMATS))
def test_reset_and_no_history_pass_current_through(fmt, gpu):
    Wd, Hd = ONE
    for kw in (dict(reset=True), dict(no_history=True), dict(reset=True, no_history=True)):
        v = _run(Wd, Hd, fmt, fmt, fmt, dst="unorm8x4", **kw)
        assert_same_array(v, np.ascontiguousarray(dn.values(dn.as_plane(_content(Wd, Hd)["current"], PLANE_FORMATS[fmt], 1))),
                          "passed through", nan_aware=True)
    # without history the previous position is neither needed nor read
    den, c = _den(), _content(Wd, Hd)
    f = PLANE_FORMATS[fmt]
    cur_np = dn.as_plane(c["current"], f, 1)
    pc, pr = _plane(f, Wd, Hd, fill=cur_np), _plane(f, Wd, Hd)
    den.display_taa(pc.tensor, pr.tensor, reset=True)
    pixels = np.ascontiguousarray(dn.result_plane(dn.values(cur_np), f)).view(np.uint8).reshape(Hd, Wd, rn.BPP[f])
    _compare(pr.host(), rn.place(pr.expected(), pr.off, pr.pitch, f, pixels, (0, 0, Wd, Hd), Hd), f, pr.off,
             "no previous position", nan_in=True)


def test_blend_alpha_extremes(gpu):
    Wd, Hd = ONE
    for blend in (1.0, 0.0, 0.05):
        _run(Wd, Hd, "f32x3", "f32x3", "f32x3", dst="unorm8x4", blend=blend)


# ------------------------------------------------- anchor: the library's own K2 --
@pytest.mark.parametrize("taa_blend_alpha", [0.2, 0.05])
@pytest.mark.parametrize("W,H", [(65, 47), (129, 53)])
def test_ratio_one_reproduces_the_library_s_own_taa(W, H, taa_blend_alpha, gpu):
    """K2 is pinned to the reference bit for bit.  At ratio 1 the unguided
    tone-mapped upsample of the frame's own albedo is K2's tone-mapped image,
    the state's prev_frame_pixel is the reprojection K2 used, and so the
    display TAA over the caller's ping-pong planes must be bmfr_output() byte
    for byte on every frame."""
    den = bmfr_amd.Denoiser(_cfg(W, H, taa_blend_alpha=taa_blend_alpha))
    planes = [torch.empty((H, W, 3), dtype=torch.float32, device="cuda") for _ in range(2)]
    current = torch.empty((H, W, 3), dtype=torch.float32, device="cuda")
    pp = torch.empty(W * H * 2, dtype=torch.float32, device="cuda")
    out = torch.empty(W * H * 3, dtype=torch.float32, device="cuda")
    for f in range(6):
        fr = scenes_np.frame("rand", W, H, f, 2)
        d = {k: torch.from_numpy(np.array(fr[k])).cuda() for k in ("noisy", "normals", "positions", "albedo")}
        den.process_frame(d["noisy"], d["normals"], d["positions"], d["albedo"], fr["prev_vp"], fr["jitter"], f)
        den.upsample(current, {"width": W, "height": H, "albedo": d["albedo"]}, source="tonemapped")
        den.copy_state("prev_frame_pixel", pp)
        result, history = planes[f & 1], planes[(f & 1) ^ 1]
        den.display_taa(current, result, history=None if f == 0 else history, prev_pixel=pp, reset=f == 0)
        den.copy_output(out)
        torch.cuda.synchronize()
        assert_same_array(result.cpu().numpy().reshape(-1), out.cpu().numpy(), (W, H, taa_blend_alpha, "frame", f))
        if f:
            assert not torch.equal(result, current)
    assert den.frame_status() == 0


# ----------------------------------------------- the loop through the library --
def test_twelve_frames_through_the_library_equal_the_restatements(gpu):
    """frame -> upsample (tone-mapped, F16X4) -> display TAA (F16X4 history
    ping-pong, UNORM8X4 dst) at 96x64 -> 192x128: result and dst on frames 0,
    1 and 11 against the same loop through upsample_np and display_taa_np on
    the library's own filtered_accumulated."""
    W, H, Wd, Hd, frames = 96, 64, 192, 128, 12
    den = bmfr_amd.Denoiser(_cfg(W, H))
    ping = [torch.zeros((Hd, Wd, 4), dtype=torch.float16, device="cuda") for _ in range(2)]
    current = torch.zeros((Hd, Wd, 4), dtype=torch.float16, device="cuda")
    dst = torch.zeros((Hd, Wd, 4), dtype=torch.uint8, device="cuda")
    acc = torch.empty(W * H * 3, dtype=torch.float32, device="cuda")
    history_np = None
    for f in range(frames):
        low, disp = scenes_np.frame("rand", W, H, f, 2), scenes_np.frame("rand", Wd, Hd, f, 2)
        d = {k: torch.from_numpy(np.array(low[k])).cuda() for k in ("noisy", "normals", "positions", "albedo")}
        g = {"width": Wd, "height": Hd, "albedo": disp["albedo"], "normals": disp["normals"],
             "positions": disp["positions"]}
        gd = {k: torch.from_numpy(np.array(v)).cuda() if isinstance(v, np.ndarray) else v for k, v in g.items()}
        pp = dn.display_prev_pixel(disp, Wd, Hd)
        den.process_frame(d["noisy"], d["normals"], d["positions"], d["albedo"], low["prev_vp"], low["jitter"], f)
        den.upsample(current, gd, d["normals"], d["positions"], source="tonemapped")
        result, history = ping[f & 1], ping[(f & 1) ^ 1]
        den.display_taa(current, result, history=None if f == 0 else history, prev_pixel=_flat(pp), reset=f == 0,
                        dst=dst, bgr=True)
        den.copy_state("filtered_accumulated", acc)
        torch.cuda.synchronize()
        vals, _ = un.upsample(acc.cpu().numpy(), W, H, g, low["normals"], low["positions"], "tonemapped")
        cur_np = rn.encode(vals, rn.F16X4).view(np.float16).reshape(Hd, Wd, 4)
        v = dn.display_taa(cur_np, history_np, pp, BLEND, reset=f == 0)
        history_np = dn.result_plane(v, rn.F16X4)
        if f in (0, 1, frames - 1):
            assert_same_array(current.cpu().numpy(), cur_np, ("current", f))
            assert_same_array(result.cpu().numpy(), history_np, ("result", f))
            assert_same_array(dst.cpu().numpy(), dn.surface_pixels(v, rn.UNORM8X4, bgr=True), ("dst", f))
    assert den.frame_status() == 0


# --------------------------------------------------------------- isolation --
def test_the_call_changes_no_state(gpu):
    """Every state plane, bmfr_output() and the frame status are what they were;
    the next frame's bytes are those of a context that never made the call."""
    W, H = 96, 64
    Wd, Hd = ONE
    frames = [scenes_np.frame("rand", W, H, f, 2) for f in range(2)]
    args = [tuple(torch.from_numpy(np.array(fr[k])).cuda() for k in ("noisy", "normals", "positions", "albedo")) +
            (fr["prev_vp"], fr["jitter"], f) for f, fr in enumerate(frames)]
    with_call, without = bmfr_amd.Denoiser(_cfg(W, H)), bmfr_amd.Denoiser(_cfg(W, H))
    c = _content(Wd, Hd)
    pc, ph = _plane(rn.F16X4, Wd, Hd, fill=dn.as_plane(c["current"], rn.F16X4, 1)), _plane(rn.F32X3, Wd, Hd, fill=c["history"])
    pr, s = _plane(rn.F16X4, Wd, Hd), Surface(rn.UNORM8X4, Wd, Hd, 0, 0)
    with_call.display_taa(pc.tensor, pr.tensor, history=ph.tensor, prev_pixel=_flat(c["prev_pixel"]), dst=s.tensor)
    assert (pr.host() != rn.SENTINEL).any()                 # legal before any frame
    assert with_call.frame_status() == 0
    for den in (with_call, without):
        den.process_frame(*args[0])
    before, ptr = state_snapshot(with_call), with_call.output_ptr()
    kept = (pc.host(), ph.host())
    pr.reset()
    with_call.display_taa(pc.tensor, pr.tensor, history=ph.tensor, prev_pixel=_flat(c["prev_pixel"]), dst=s.tensor)
    assert (pr.host() != rn.SENTINEL).any() and (s.host() != rn.SENTINEL).any()
    after = state_snapshot(with_call)
    for k in before:
        assert_same_array(after[k], before[k], k)
    assert_same_array(pc.host(), kept[0], "current")
    assert_same_array(ph.host(), kept[1], "history")
    assert with_call.output_ptr() == ptr and with_call.frame_status() == 0
    for den in (with_call, without):
        den.process_frame(*args[1])
    a, b = state_snapshot(with_call), state_snapshot(without)
    for k in a:
        assert_same_array(a[k], b[k], ("frame 1", k))
    assert with_call.frame_status() == 0


# ------------------------------------------------------------------ errors --
def test_every_error_enqueues_nothing_and_writes_nothing(gpu):
    Wd, Hd = ONE
    lib, den, c = _lib.load(), _den(), _content(Wd, Hd)
    pc = _plane(rn.F16X4, Wd, Hd, 1, fill=dn.as_plane(c["current"], rn.F16X4, 1))
    ph = _plane(rn.F32X3, Wd, Hd, 1, fill=c["history"])
    pr, s = _plane(rn.F16X4, Wd, Hd, 1), Surface(rn.UNORM8X4, Wd, Hd, 4, 0)
    motion, pp = _flat(rn.to_half(c["motion"])), _flat(c["prev_pixel"])

    def status(edit=None, null_args=False, no_dst=False, handle=den.handle, origin=(0, 0), flip_y=False, **kw):
        """The library's answer to the wrapper's checked arguments after `edit`
        (on the arguments and the surface struct); result and dst untouched."""
        kw.setdefault("motion", motion)
        a, surf = den.display_taa_args(pc.tensor, pr.tensor, history=ph.tensor, dst=s.tensor, origin=origin,
                                       flip_y=flip_y, **kw)
        if edit:
            edit(a, surf)
        st = lib.bmfr_display_taa(handle, None, None if null_args else C.byref(a), None if no_dst else C.byref(surf))
        torch.cuda.synchronize()
        assert_same_array(pr.host(), pr.expected(), "result sentinel")
        assert_same_array(s.host(), s.expected(), "dst sentinel")
        return st

    def set_(**kw):
        def edit(a, surf):
            for k, v in kw.items():
                if k.startswith("dst_"):
                    setattr(surf, k[4:], v)
                elif k.split("_", 1)[0] in ("current", "history", "result"):
                    plane, field = k.split("_", 1)
                    setattr(getattr(a, plane), field, v)
                else:
                    setattr(a, k, v)
        return edit

    cur_ptr, hist_ptr, res_ptr = pc.tensor.data_ptr(), ph.tensor.data_ptr(), pr.tensor.data_ptr()
    invalid = [
        dict(edit=set_(dst_data=None)), dict(edit=set_(dst_pitch=Wd * 4 - 4)), dict(edit=set_(dst_pitch=Wd * 4 + 6)),
        dict(edit=set_(dst_width=0)),
        dict(null_args=True), dict(null_args=True, no_dst=True),
        dict(edit=set_(width=0)), dict(edit=set_(height=-1)),
        dict(edit=set_(current_data=None)), dict(edit=set_(result_data=None)),
        dict(edit=set_(current_pitch=Wd * 8 - 8)), dict(edit=set_(history_pitch=Wd * 12 - 4)),
        dict(edit=set_(result_pitch=Wd * 8 - 8)),
        dict(edit=set_(current_pitch=pc.pitch + 4)), dict(edit=set_(history_pitch=ph.pitch + 2)),
        dict(edit=set_(result_pitch=pr.pitch + 4)),
        dict(edit=set_(current_data=cur_ptr + 4)), dict(edit=set_(history_data=hist_ptr + 2)),
        dict(edit=set_(result_data=res_ptr + 4)),
        dict(edit=set_(current_pitch=(1 << 31) + 8)), dict(edit=set_(result_pitch=(1 << 31) + 8)),   # above 2^31
        dict(edit=set_(width=Wd + 2)),                                      # the planes' pitches no longer hold a row
        dict(edit=set_(prev_pixel=pp.data_ptr())),                         # both
        dict(edit=set_(motion=None)),                                      # neither
        dict(edit=set_(motion=motion.data_ptr() + 2)),
        dict(edit=set_(motion=None, prev_pixel=pp.data_ptr() + 2)),
        dict(edit=set_(result_data=cur_ptr)),
        dict(edit=set_(result_data=hist_ptr, result_format=_lib.FORMAT_F32X3, result_pitch=ph.pitch)),
        dict(edit=set_(blend_alpha=float("nan"))), dict(edit=set_(blend_alpha=float("-inf"))),
        dict(edit=set_(dst_width=Wd - 1)), dict(edit=set_(dst_height=Hd - 1)),
        dict(origin=(1, 0)), dict(origin=(0, -1)), dict(origin=(0, 1), flip_y=True),
        dict(handle=None), dict(handle=None, no_dst=True),
    ]
    for case in invalid:
        assert status(**case) == 1, {k: v for k, v in case.items() if k != "edit"}
    unsupported = [dict(edit=set_(dst_format=_lib.FORMAT_OCT_SNORM16X2)), dict(edit=set_(dst_format=9)),
                   dict(edit=set_(current_format=_lib.FORMAT_UNORM8X4)), dict(edit=set_(history_format=_lib.FORMAT_F16X2)),
                   dict(edit=set_(result_format=_lib.FORMAT_NONE)), dict(edit=set_(result_format=_lib.FORMAT_UNORM10X3A2)),
                   dict(edit=set_(motion_format=_lib.FORMAT_F32X3)), dict(edit=set_(motion_format=_lib.FORMAT_NONE))]
    for case in unsupported:
        assert status(**case) == 2
    # dst is checked first: a bad surface with bad arguments answers for the surface
    assert status(edit=set_(dst_format=9, width=0)) == 2
    assert status(edit=set_(dst_format=9), null_args=True) == 2
    # the wrapper refuses what it can see before the call
    with pytest.raises(ValueError):
        den.display_taa(pc.tensor, pr.tensor[:-1], history=ph.tensor, motion=motion)
    with pytest.raises(TypeError):
        den.display_taa(pc.tensor, pr.tensor.float(), history=ph.tensor, motion=motion)
    with pytest.raises(ValueError):
        den.display_taa(pc.tensor.cpu(), pr.tensor, history=ph.tensor, motion=motion)
    with pytest.raises(ValueError):
        den.display_taa(pc.tensor, pr.tensor, history=ph.tensor, motion=motion[:-2])
    with pytest.raises(bmfr_amd.BmfrError) as e:
        den.display_taa(pc.tensor, pr.tensor, history=ph.tensor)           # neither prev_pixel nor motion
    assert e.value.status == 1
    assert_same_array(pr.host(), pr.expected(), "result sentinel")
    # the same arguments are fine once all is in order: with history, and without history with a
    # previous-position plane that would be refused
    den.display_taa(pc.tensor, pr.tensor, history=ph.tensor, motion=motion, dst=s.tensor)
    assert (pr.host() != rn.SENTINEL).any() and (s.host() != rn.SENTINEL).any()
    pr.reset()
    a, surf = den.display_taa_args(pc.tensor, pr.tensor, history=ph.tensor, motion=motion, reset=True)
    a.motion, a.motion_format, a.prev_pixel = motion.data_ptr() + 2, 9, pp.data_ptr() + 2
    assert lib.bmfr_display_taa(den.handle, None, C.byref(a), None) == 0
    assert (pr.host() != rn.SENTINEL).any()
    assert den.frame_status() == 0
