"""Guided upsampling on the GPU (bmfr_upsample_output, include/bmfr.h;
Denoiser.upsample): the kernel against the numpy restatement
(tests/upsample_np.py) byte for byte on a constructed image written into the
context's filtered_accumulated plane, every byte of the surface it must not
write still holding its sentinel; the counter, the cross-check against
bmfr_resolve_output at ratio 1, the untouched state, and every error."""
from __future__ import annotations

import ctypes as C
import functools
import itertools

import numpy as np
import pytest
import torch

import bmfr_amd
from bmfr_amd import _lib
from bmfr_amd.tiling import TileGrid
import prepare_np as pn
import resolve_np as rn
import upsample_np as un
from parity_harness import assert_same_array, state_snapshot
from test_gpu_resolve import ALPHA, LAYOUTS, Surface, _cfg, _compare, _first_frame, _images, _overwrite_state

pytestmark = pytest.mark.gpu

F32 = np.float32
# The smallest sizes at which the footprint, the clamps and the tile tails (64 x 4) can go wrong:
# ratios 1, 2 and 4, a non-integer ratio in both axes (71 x 50) and in one (130 x 95), one axis
# at ratio 1 (193 x 53).  The odd frame is 47 x 32: bmfr_create takes no height from 33 to 46
# (the mirrored block margin must stay inside the image), so 47 x 33 does not exist as a context.
SIZES = [(32, 32, 32, 32), (32, 32, 64, 64), (32, 32, 128, 128),
         (47, 32, 47, 32), (47, 32, 71, 50), (47, 32, 94, 64), (47, 32, 188, 128),
         (65, 47, 130, 95), (129, 53, 193, 53)]
ONE = (47, 32, 71, 50)   # the non-integer ratio, rows and columns that end inside a tile


@functools.lru_cache(maxsize=None)
def _context(W, H, half):
    """A context after frame 0 whose filtered_accumulated holds the constructed
    image -> (denoiser, the frame's device planes, filtered, normals, positions on the host)."""
    den = bmfr_amd.Denoiser(_cfg(W, H, input_half=half))
    fr = _first_frame(den, bool(half))
    result, filtered, _, _ = _images(W, H)
    _overwrite_state(den, result, filtered)
    torch.cuda.synchronize()
    return den, fr, filtered, fr["normals"].cpu().numpy(), fr["positions"].cpu().numpy()


@functools.lru_cache(maxsize=None)
def _display(Wd, Hd):
    """The synthetic scene at display resolution (host planes), its camera and jitter."""
    fr = bmfr_amd.synth_frame_host(Wd, Hd, 0)
    vp, jit = bmfr_amd.synth_camera(Wd, Hd, 0)
    return {k: np.asarray(v, F32).reshape(-1) for k, v in fr.items()}, vp, jit


def _guides(Wd, Hd, albedo="f32", normals="f32", positions="given", guided=True, seed=7):
    """Host guides in the named formats: a seeded albedo with values past half's
    range, NaN and inf (float formats); the scene's normals and positions (or
    their depth) with a few NaN pixels."""
    rng = np.random.RandomState(seed)
    n = Wd * Hd
    fr, vp, jit = _display(Wd, Hd)
    alb = rng.uniform(-0.25, 1.5, (n, 3)).astype(F32)
    alb[::97] = rng.normal(0, 300, alb[::97].shape).astype(F32)
    alb[5::211, 1] = np.nan
    alb[7::223, 2] = np.inf
    g = {"width": Wd, "height": Hd}
    g["albedo"] = {"f32": lambda: alb.reshape(-1), "f16": lambda: pn.rgba16(alb, rng),
                   "unorm8": lambda: pn.unorm8(alb, rng)}[albedo]()
    if not guided:
        return g
    nrm = fr["normals"].copy().reshape(n, 3)
    pos = fr["positions"].copy().reshape(n, 3)
    if normals == "oct":
        g["normals"] = pn.oct_encode(nrm).reshape(-1)
    else:
        nrm[11::131, 0] = np.nan
        g["normals"] = nrm.reshape(-1) if normals == "f32" else pn.rgba16(nrm, rng)
    if positions == "given":
        pos[13::137, 2] = np.nan
        g["positions"] = pos.reshape(-1)
    else:
        depth, inv = pn.depth_and_inverse(pos, vp)
        depth[13::137] = np.nan
        g["depth"], g["inv_view_proj"], g["pixel_offset"] = depth, inv, tuple(jit)
    return g


def _device(g: dict, shift: int = 0) -> dict:
    """The guides with their planes on the device; shift: each plane one pixel
    into a larger allocation (element-aligned, off a 16-byte boundary)."""
    out = {}
    for k, v in g.items():
        if isinstance(v, np.ndarray) and k != "inv_view_proj":
            t = torch.from_numpy(v).cuda()
            if shift:
                per = v.size // (g["width"] * g["height"])
                big = torch.empty(t.numel() + per, dtype=t.dtype, device="cuda")
                big[per:].copy_(t)
                t = big[per:]
                assert t.data_ptr() % 16 != 0
            out[k] = t
        else:
            out[k] = v
    return out


def _run(den, fr, filtered, fn, fp, W, H, g, fmt, source="hdr", bgr=False, flip=False, layout=(0, 0, 0), shift=0,
         what=None):
    """One call into a sentinel surface against the restatement -> the fallback count."""
    f = rn.FORMATS[fmt]
    Wd, Hd = g["width"], g["height"]
    guided = g.get("normals") is not None
    padded, shifted, larger = layout
    pad = {rn.UNORM8X3: 1, rn.F16X4: 8}.get(f, 4)
    s = Surface(f, Wd + 8 * larger, Hd + 8 * larger, pad * padded, rn.ALIGN[f] * shifted)
    origin = (5, 3) if larger else (0, 0)
    stats = torch.full((1,), 1000, dtype=torch.int32, device="cuda")
    den.upsample(s.tensor, _device(g, shift), normals=fr["normals"] if guided else None,
                 positions=fr["positions"] if guided else None, source=source, origin=origin, flip_y=flip, bgr=bgr,
                 alpha=ALPHA, stats=stats)
    vals, fell = un.upsample(filtered, W, H, g, fn, fp, source)
    want = rn.place(s.expected(), s.off, s.pitch, f, rn.encode(vals, f, bgr, ALPHA), (0, 0, Wd, Hd), Hd, origin, flip)
    _compare(s.host(), want, f, s.off, what or (fmt, source, bgr, flip, layout), nan_in=True)
    count = int(stats.item()) - 1000
    assert count == (int(fell.sum()) if guided else 0), (what, count, int(fell.sum()))
    return count, fell.size


@pytest.mark.parametrize("W,H,Wd,Hd", SIZES)
def test_kernel_equals_restatement_at_every_size(W, H, Wd, Hd, gpu):
    den, fr, filtered, fn, fp = _context(W, H, 0)
    args = (den, fr, filtered, fn, fp, W, H)
    fell, n = _run(*args, _guides(Wd, Hd), "f32x3", what="guided f32")
    assert 0 < fell < n                       # NaN guides fall back; the rest find a tap
    _run(*args, _guides(Wd, Hd, "unorm8", "oct", "depth"), "unorm8x4", source="tonemapped", what="engine formats")
    _run(*args, _guides(Wd, Hd, "f16", guided=False), "f16x4", what="unguided")
    assert den.frame_status() == 0


@pytest.mark.parametrize("source", ["hdr", "tonemapped"])
@pytest.mark.parametrize("fmt", list(rn.FORMATS))
def test_every_surface_format_source_and_switch(fmt, source, gpu):
    W, H, Wd, Hd = ONE
    den, fr, filtered, fn, fp = _context(W, H, 0)
    g = _guides(Wd, Hd, "f16", "f32", "depth")
    for bgr, flip in itertools.product((False, True), (False, True)):
        _run(den, fr, filtered, fn, fp, W, H, g, fmt, source, bgr, flip)


@pytest.mark.parametrize("positions", ["given", "depth"])
@pytest.mark.parametrize("normals", ["f32", "f16", "oct"])
@pytest.mark.parametrize("albedo", ["f32", "f16", "unorm8"])
def test_every_guide_format(albedo, normals, positions, gpu):
    W, H, Wd, Hd = ONE
    den, fr, filtered, fn, fp = _context(W, H, 0)
    _run(den, fr, filtered, fn, fp, W, H, _guides(Wd, Hd, albedo, normals, positions), "f16x4")
    _run(den, fr, filtered, fn, fp, W, H, _guides(Wd, Hd, albedo, normals, positions), "unorm10x3a2", shift=1,
         what="planes off a 16-byte boundary")


@pytest.mark.parametrize("W,H,Wd,Hd", [ONE, (47, 32, 47, 32), (65, 47, 130, 95)])
def test_input_half_contexts(W, H, Wd, Hd, gpu):
    den, fr, filtered, fn, fp = _context(W, H, 1)
    assert fn.dtype == np.float16 and fp.dtype == np.float16
    fell, n = _run(den, fr, filtered, fn, fp, W, H, _guides(Wd, Hd, "unorm8", "oct", "depth"), "f16x4")
    assert fell < n
    _run(den, fr, filtered, fn, fp, W, H, _guides(Wd, Hd), "unorm8x3", source="tonemapped")


@pytest.mark.parametrize("fmt", ["f16x4", "unorm8x3", "f32x3"])
def test_pitch_alignment_and_origin(fmt, gpu):
    W, H, Wd, Hd = ONE
    den, fr, filtered, fn, fp = _context(W, H, 0)
    g, free = _guides(Wd, Hd, "unorm8", "oct", "depth"), _guides(Wd, Hd, guided=False)
    for layout in LAYOUTS:
        _run(den, fr, filtered, fn, fp, W, H, g, fmt, flip=bool(layout[0]), layout=layout)
        _run(den, fr, filtered, fn, fp, W, H, free, fmt, bgr=True, layout=layout)


def test_stats_are_added_to_and_left_alone_when_unguided(gpu):
    W, H, Wd, Hd = ONE
    den, fr, filtered, fn, fp = _context(W, H, 0)
    g = _guides(Wd, Hd)
    _, fell = un.upsample(filtered, W, H, g, fn, fp)
    assert fell.any()
    stats = torch.full((1,), 7, dtype=torch.int32, device="cuda")
    s = Surface(rn.UNORM8X4, Wd, Hd, 0, 0)
    for k in (1, 2):
        den.upsample(s.tensor, _device(g), fr["normals"], fr["positions"], stats=stats)
        assert int(stats.item()) == 7 + k * int(fell.sum())
    before = int(stats.item())
    den.upsample(s.tensor, _device(_guides(Wd, Hd, guided=False)), stats=stats)
    assert int(stats.item()) == before
    den.upsample(s.tensor, _device(g), fr["normals"], fr["positions"])       # and no counter at all


@pytest.mark.parametrize("W,H", [(47, 32), (128, 80)])
def test_ratio_one_with_the_frame_s_own_planes_is_the_hdr_resolve(W, H, gpu):
    """The existing entry point as the reference: every tap but the first has
    weight 0, the first passes its own test, and the surface is
    bmfr_resolve_output(BMFR_RESOLVE_HDR)'s byte for byte, in every format."""
    den, fr, filtered, fn, fp = _context(W, H, 0)
    albedo = torch.from_numpy(_images(W, H)[2]).cuda().reshape(-1)
    g = {"width": W, "height": H, "albedo": albedo, "normals": fr["normals"], "positions": fr["positions"]}
    for (fmt, f), bgr, flip in itertools.product(rn.FORMATS.items(), (False, True), (False, True)):
        a, b = Surface(f, W, H, 0, 0), Surface(f, W, H, 0, 0)
        stats = torch.zeros(1, dtype=torch.int32, device="cuda")
        den.upsample(a.tensor, g, fr["normals"], fr["positions"], flip_y=flip, bgr=bgr, alpha=ALPHA, stats=stats)
        den.resolve(b.tensor, source="hdr", albedo=albedo, flip_y=flip, bgr=bgr, alpha=ALPHA)
        assert int(stats.item()) == 0
        _compare(a.host(), b.host(), f, a.off, (fmt, bgr, flip), nan_in=True)


def _frames(W, H, count):
    out = []
    for f in range(count):
        fr = bmfr_amd.synth_frame_device(W, H, f)
        vp, _ = bmfr_amd.synth_camera(W, H, max(f - 1, 0))
        _, jit = bmfr_amd.synth_camera(W, H, f)
        out.append((fr["noisy"], fr["normals"], fr["positions"], fr["albedo"], vp, jit, f))
    return out


def test_the_call_changes_no_state(gpu):
    """Every state plane, bmfr_output() and the frame status are what they were;
    the next frame's bytes are those of a context that never made the call."""
    W, H, Wd, Hd = 128, 80, 192, 120
    frames = _frames(W, H, 2)
    with_call, without = bmfr_amd.Denoiser(_cfg(W, H)), bmfr_amd.Denoiser(_cfg(W, H))
    for den in (with_call, without):
        den.process_frame(*frames[0])
    before, ptr = state_snapshot(with_call), with_call.output_ptr()
    s = Surface(rn.F16X4, Wd, Hd, 0, 0)
    stats = torch.zeros(1, dtype=torch.int32, device="cuda")
    with_call.upsample(s.tensor, _device(_guides(Wd, Hd, "unorm8", "oct", "depth")), frames[0][1], frames[0][2],
                       source="tonemapped", stats=stats)
    assert (s.host() != rn.SENTINEL).any()
    after = state_snapshot(with_call)
    for k in before:
        assert_same_array(after[k], before[k], k)
    assert with_call.output_ptr() == ptr and with_call.frame_status() == 0
    for den in (with_call, without):
        den.process_frame(*frames[1])
    a, b = state_snapshot(with_call), state_snapshot(without)
    for k in a:
        assert_same_array(a[k], b[k], ("frame 1", k))
    assert with_call.frame_status() == 0


# ------------------------------------------------------------------ errors --
def test_every_error_enqueues_nothing_and_writes_nothing(gpu):
    W, H, Wd, Hd = 128, 80, 192, 120
    lib = _lib.load()
    frames = _frames(W, H, 2)
    den = bmfr_amd.Denoiser(_cfg(W, H))
    s = Surface(rn.UNORM8X4, Wd, Hd, 4, 0)
    g = _device(_guides(Wd, Hd, "unorm8", "oct", "depth"))
    nrm, pos = frames[0][1], frames[0][2]
    stats = torch.full((2,), 5, dtype=torch.int32, device="cuda")

    def status(den=den, surface=s.tensor, guides=g, normals=nrm, positions=pos, source="hdr", origin=(0, 0),
               flip_y=False, edit=None, frame=None, stats_ptr=None, null_guides=False, code=None):
        """The library's answer to the wrapper's checked arguments after `edit`
        (on the guides and the surface struct); the surface and the counter untouched."""
        src, gs, surf = den.upsample_args(surface, guides, normals, positions, source, origin, flip_y)
        if edit:
            edit(gs, surf)
        fn_ptr, fp_ptr = frame if frame else (normals.data_ptr() if normals is not None else None,
                                              positions.data_ptr() if positions is not None else None)
        st = lib.bmfr_upsample_output(den.handle, None, src if code is None else code, fn_ptr, fp_ptr,
                                      None if null_guides else C.byref(gs), C.byref(surf),
                                      stats.data_ptr() if stats_ptr is None else stats_ptr)
        assert_same_array(s.host(), s.expected(), "sentinel")
        assert stats.tolist() == [5, 5]
        return st

    assert status() == 1                                                   # before the first frame
    den.process_frame(*frames[0])
    den.process_frame_interior(*frames[1])
    assert status() == 1                                                   # between _interior and _border
    den.process_frame_border(*frames[1])
    nrm, pos = frames[1][1], frames[1][2]

    def set_(**kw):
        def edit(gs, surf):
            for k, v in kw.items():
                setattr(surf if hasattr(surf, k) and not hasattr(gs, k) else gs, k, v)
        return edit

    invalid = [
        dict(code=2), dict(code=-1),                                        # source
        dict(null_guides=True),
        dict(edit=set_(albedo=None)),
        dict(edit=set_(normals=None)),                                      # a position source without normals
        dict(edit=set_(depth=None)),                                        # normals without a position source
        dict(frame=(None, pos.data_ptr())), dict(frame=(nrm.data_ptr(), None)),
        dict(edit=set_(plane_limit_squared=0.0)), dict(edit=set_(plane_limit_squared=-1.0)),
        dict(edit=set_(plane_limit_squared=float("nan"))), dict(edit=set_(normal_limit_squared=float("inf"))),
        dict(edit=set_(normal_limit_squared=0.0)),
        dict(edit=set_(albedo=g["albedo"].data_ptr() + 2)), dict(edit=set_(normals=g["normals"].data_ptr() + 2)),
        dict(edit=set_(depth=g["depth"].data_ptr() + 2)),
        dict(frame=(nrm.data_ptr() + 2, pos.data_ptr())), dict(frame=(nrm.data_ptr(), pos.data_ptr() + 1)),
        dict(stats_ptr=stats.data_ptr() + 2),
        dict(edit=set_(width=W - 1)), dict(edit=set_(height=H - 1)),       # below the frame
        dict(edit=set_(width=4 * W + 1)), dict(edit=set_(height=4 * H + 1)),
        dict(edit=set_(width=0)), dict(edit=set_(height=-1)),
        dict(edit=set_(width=Wd + 1)),                                      # does not fit the surface
        dict(origin=(1, 0)), dict(origin=(0, -1)), dict(origin=(0, 1), flip_y=True),
        dict(edit=set_(data=None)), dict(edit=set_(pitch=Wd * 4 - 4)), dict(edit=set_(pitch=Wd * 4 + 2)),
    ]
    for case in invalid:
        assert status(**case) == 1, {k: v for k, v in case.items() if k != "edit"}
    unsupported = [dict(edit=set_(format=_lib.FORMAT_OCT_SNORM16X2)), dict(edit=set_(format=9)),
                   dict(edit=set_(albedo_format=_lib.FORMAT_OCT_SNORM16X2)), dict(edit=set_(albedo_format=_lib.FORMAT_NONE)),
                   dict(edit=set_(normal_format=_lib.FORMAT_UNORM8X4)), dict(edit=set_(normal_format=_lib.FORMAT_UNORM8X3))]
    for case in unsupported:
        assert status(**case) == 2
    # dst is checked first: a bad surface with bad guides answers for the surface
    assert status(edit=set_(format=9, albedo=None)) == 2
    # a tiled context is refused, whatever else is right
    tiled = bmfr_amd.Denoiser(_cfg(W, H, tile=TileGrid(W, H, 2, 1, halo=34).tile(0), tile_halo=34))
    cut = bmfr_amd.synth_region_device(W, H, tiled.region, 0)
    vp, jit = bmfr_amd.synth_camera(W, H, 0)
    tiled.process_frame(cut["noisy"], cut["normals"], cut["positions"], cut["albedo"], vp, jit, 0)
    assert status(den=tiled, normals=cut["normals"], positions=cut["positions"]) == 2
    with pytest.raises(bmfr_amd.BmfrError) as e:
        tiled.upsample(s.tensor, g, cut["normals"], cut["positions"])
    assert e.value.status == 2
    assert_same_array(s.host(), s.expected(), "sentinel")
    # the same arguments are fine once all is in order
    den.upsample(s.tensor, g, nrm, pos)
    assert (s.host() != rn.SENTINEL).any()
    assert den.frame_status() == 0 and tiled.frame_status() == 0
