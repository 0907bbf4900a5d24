"""The firefly pre-filter on the GPU (bmfr_suppress_fireflies, include/bmfr.h;
Denoiser.suppress_fireflies / process_gbuffer(firefly=...); bmfr_host
--firefly): the kernel against the numpy restatement (tests/firefly_np.py)
byte for byte, its counters, its argument checks, that it touches no state,
tiles against the whole frame, and the three ways to reach it against each
other."""
from __future__ import annotations

import ctypes as C
import functools
import itertools
import subprocess

import numpy as np
import pytest
import torch

import bmfr_amd
from bmfr_amd import _build, _lib
from bmfr_amd.tiling import LoopbackTransport, TileGrid, region_slice
import firefly_np as fn
import prepare_np as pn
import scenes_np
from parity_harness import state_snapshot

pytestmark = pytest.mark.gpu

F32 = np.float32
W, H = 128, 80
# radius, threshold, floor, replace_nonfinite: every value of each, all together
RULES = list(itertools.product((1, 2), (1.0, 2.0, 4.0), (0.0, 0.05), (1, 0)))


def _cfg(**kw):
    return bmfr_amd.BmfrConfig(image_width=W, image_height=H, **kw)


def _same(got: np.ndarray, want: np.ndarray, what):
    assert got.dtype == want.dtype and got.size == want.size, (what, got.dtype, want.dtype, got.shape, want.shape)
    a, b = got.reshape(-1).view(np.uint8), want.reshape(-1).view(np.uint8)
    bad = np.flatnonzero(a != b)
    if bad.size:
        i = int(bad[0]) // got.itemsize
        raise AssertionError((what, f"{bad.size} of {a.size} bytes differ, first at element {i} (pixel {i // 3}): "
                                    f"{got.reshape(-1)[i]!r} != {want.reshape(-1)[i]!r}"))


def _plane(a: np.ndarray, offset_bytes: int = 0) -> torch.Tensor:
    """The array on the GPU, `offset_bytes` past a 16-byte boundary."""
    t = torch.from_numpy(np.ascontiguousarray(a).reshape(-1))
    k = offset_bytes // t.element_size()
    big = torch.empty(t.numel() + k, dtype=t.dtype, device="cuda")
    assert big.data_ptr() % 16 == 0
    big[k:].copy_(t)
    return big[k:]


class _Raw:
    """bmfr_debug_suppress_fireflies: the kernel on a plane of any size (the
    smallest region a context has is 32 x 32), with the Denoiser method's shape."""

    def __init__(self, w, h, half):
        self.w, self.h, self.half, self.lib = w, h, half, _lib.load()

    def suppress_fireflies(self, noisy, out, threshold, radius, floor, replace_nonfinite, stats):
        p = _lib.FireflyParams(threshold, radius, floor, int(replace_nonfinite))
        st = self.lib.bmfr_debug_suppress_fireflies(torch.cuda.current_stream().cuda_stream, noisy.data_ptr(),
                                                    out.data_ptr(), self.w, self.h, int(self.half), C.byref(p),
                                                    None if stats is None else stats.data_ptr())
        assert st == 0, st
        return out


def _filter_of(w, h, half):
    """What filters a w x h plane: a context whose region that is, or _Raw."""
    if (w, h) == (W, H):
        return bmfr_amd.Denoiser(_cfg(input_half=int(half)))
    if (w, h) == (67, 35):  # the region of a 33 x 1 tile at the image's corner, halo 34
        den = bmfr_amd.Denoiser(_cfg(input_half=int(half), tile=(0, 0, 33, 1), tile_halo=34))
        assert den.region == (0, 0, 67, 35)
        return den
    return _Raw(w, h, half)


# ----------------------------------------------------------------- parity --
# 128 x 80: whole groups in every row, several work-groups across and five down;
# 67 x 35: an odd width, so the first aligned pixel moves from row to row and every row has a head and a
# tail; 5 x 3 and 2 x 1: narrower than a group and than the window.  Off a 16-byte boundary every pixel
# takes the element-sized path.
@pytest.mark.parametrize("offset", [0, 4], ids=["aligned", "off4"])
@pytest.mark.parametrize("half", [False, True], ids=["f32", "input_half"])
@pytest.mark.parametrize("w,h", [(67, 35), (128, 80), (5, 3), (2, 1)])
def test_kernel_equals_restatement(w, h, half, offset, gpu):
    src = fn.content(w, h, half)
    assert not np.isfinite(src.astype(F32)).all()
    flt = _filter_of(w, h, half)
    noisy = _plane(src, offset)
    out = _plane(np.zeros_like(src), offset)
    assert noisy.data_ptr() % 16 == offset and out.data_ptr() % 16 == offset
    stats = torch.zeros(2, dtype=torch.int32, device="cuda")
    touched = 0
    for radius, threshold, floor, replace in RULES:
        want, counts = fn.suppress(src, w, h, threshold, radius, floor, bool(replace))
        out.fill_(-7.0)
        stats.zero_()
        flt.suppress_fireflies(noisy, out=out, threshold=threshold, radius=radius, floor=floor,
                               replace_nonfinite=bool(replace), stats=stats)
        torch.cuda.synchronize()
        what = (w, h, half, offset, radius, threshold, floor, replace)
        _same(out.cpu().numpy(), want, what)
        assert tuple(stats.cpu().tolist()) == counts, (what, stats.cpu().tolist(), counts)
        touched += sum(counts)
    _same(noisy.cpu().numpy(), src, "the input plane")
    assert touched > 0


@pytest.mark.parametrize("half", [False, True], ids=["f32", "input_half"])
def test_work_groups_with_more_than_one_tile(half, gpu):
    """A launch has about 2048 work-groups; past that each takes several tiles
    of 16 rows down its column.  40 x 32808 is one tile across and 2051 down:
    two tiles per work-group, the last work-group one (the smallest plane that
    gets there; a 4K frame runs five per work-group)."""
    w, h = 40, 2048 * 16 + 40
    rng = np.random.default_rng(5)
    src = (3.0 * rng.random((h, w, 3), dtype=F32) ** 2).astype(F32)
    src[rng.random((h, w)) < 1e-3] *= F32(50.0)
    src[rng.random((h, w)) < 1e-4] = np.nan
    src = src.astype(np.float16) if half else src
    want, counts = fn.suppress(src, w, h, 2.0, 2, 0.01, True)
    assert min(counts) > 50
    noisy, out = _plane(src), _plane(np.zeros_like(src))
    stats = torch.zeros(2, dtype=torch.int32, device="cuda")
    _Raw(w, h, half).suppress_fireflies(noisy, out, 2.0, 2, 0.01, True, stats)
    torch.cuda.synchronize()
    _same(out.cpu().numpy(), want, (w, h, half))
    assert tuple(stats.cpu().tolist()) == counts


def test_stats_accumulate_and_may_be_null(gpu):
    src = fn.content(W, H, False)
    want, counts = fn.suppress(src, W, H)
    assert counts[0] > 0 and counts[1] > 0
    den = bmfr_amd.Denoiser(_cfg())
    noisy = _plane(src)
    stats = torch.tensor([5, 7], dtype=torch.int32, device="cuda")
    den.suppress_fireflies(noisy, stats=stats)
    out = den.suppress_fireflies(noisy, stats=stats)
    assert tuple(stats.cpu().tolist()) == (5 + 2 * counts[0], 7 + 2 * counts[1])
    _same(out.cpu().numpy(), want, "with stats")
    _same(den.suppress_fireflies(noisy).cpu().numpy(), want, "stats = NULL")


# ----------------------------------------------------------------- errors --
@pytest.mark.parametrize("half", [0, 1], ids=["f32", "input_half"])
def test_invalid_arguments_write_nothing(half, gpu):
    den = bmfr_amd.Denoiser(_cfg(input_half=half))
    lib, st = den.lib, torch.cuda.current_stream().cuda_stream
    src = fn.content(W, H, bool(half))
    noisy = _plane(src)
    out = torch.full_like(noisy, -7.0)
    stats = torch.tensor([3, 4], dtype=torch.int32, device="cuda")

    def call(ctx=den.handle, a=noisy.data_ptr(), b=out.data_ptr(), stats_ptr=stats.data_ptr(), null_p=False, **kw):
        p = _lib.FireflyParams()
        lib.bmfr_firefly_default(C.byref(p))
        assert (p.threshold, p.radius, p.floor, p.replace_nonfinite) == (2.0, 1, 0.0, 1)
        for k, v in kw.items():
            setattr(p, k, v)
        return lib.bmfr_suppress_fireflies(ctx, st, a, b, None if null_p else C.byref(p), stats_ptr)

    elem = 2 if half else 4
    bad = {
        "NULL ctx": call(ctx=None), "NULL noisy": call(a=None), "NULL out": call(b=None), "NULL p": call(null_p=True),
        "in place": call(b=noisy.data_ptr()),
        "noisy off its element": call(a=noisy.data_ptr() + elem // 2),
        "out off its element": call(b=out.data_ptr() + elem // 2),
        "threshold 0": call(threshold=0.0), "threshold < 0": call(threshold=-1.0),
        "threshold NaN": call(threshold=float("nan")), "threshold inf": call(threshold=float("inf")),
        "radius 0": call(radius=0), "radius 3": call(radius=3), "radius -1": call(radius=-1),
        "floor < 0": call(floor=-0.5), "floor NaN": call(floor=float("nan")), "floor inf": call(floor=float("inf")),
    }
    torch.cuda.synchronize()
    assert all(v == 1 for v in bad.values()), bad   # BMFR_ERROR_INVALID_ARGUMENT
    assert (out == -7.0).all() and stats.cpu().tolist() == [3, 4]
    _same(noisy.cpu().numpy(), src, "the input plane")
    assert call() == 0   # the same call with nothing wrong
    torch.cuda.synchronize()
    _same(out.cpu().numpy(), fn.suppress(src, W, H)[0], "after the errors")
    # the Python host refuses planes the library would read out of bounds
    with pytest.raises(ValueError):
        den.suppress_fireflies(noisy[:-3])
    with pytest.raises(TypeError):
        den.suppress_fireflies(noisy.to(torch.float32 if half else torch.float16))
    with pytest.raises(ValueError):
        den.suppress_fireflies(noisy, out=out[:-3])


# --------------------------------------------------------- no side effects --
def test_call_between_two_frames_changes_no_state(gpu):
    """State planes and frame_status() before and after a call between frames
    0 and 1; frame 1 then equals a twin's that never called the filter."""
    A, B = bmfr_amd.Denoiser(_cfg()), bmfr_amd.Denoiser(_cfg())
    t = lambda a: torch.from_numpy(np.array(a)).cuda()  # noqa: E731
    for f in range(2):
        fr = scenes_np.frame("rand", W, H, f, 2)
        d = {k: t(fr[k]) for k in ("noisy", "normals", "positions", "albedo")}
        for den in (A, B):
            den.process_frame(d["noisy"], d["normals"], d["positions"], d["albedo"], fr["prev_vp"], fr["jitter"], f)
        if f == 0:
            before, status = state_snapshot(A), A.frame_status()
            A.suppress_fireflies(d["noisy"], radius=2, stats=torch.zeros(2, dtype=torch.int32, device="cuda"))
            torch.cuda.synchronize()
            after = state_snapshot(A)
            assert A.frame_status() == status == 0
            for name in before:
                _same(after[name], before[name], name)
    a, b = state_snapshot(A), state_snapshot(B)
    for name in a:
        _same(a[name], b[name], ("frame 1", name))
    assert A.frame_status() == 0


# ------------------------------------------------------------------ tiled --
@functools.lru_cache(maxsize=None)
def _still_frame(f: int):
    """Scene rand under a still camera (tile_halo = 34 leaves no room for
    motion) with x50 pixels on and beside the tile and region edges of both
    grids: x = 64 +- 34 and y = 32 +- 34 are where the regions end."""
    fr = scenes_np.frame("rand", W, H, f, 2, still=True)
    noisy = np.array(fr["noisy"]).reshape(H, W, 3)
    for x, y in ((63, 10), (64, 40), (97, 20), (96, 21), (30, 60), (29, 33), (5, 65), (100, 66), (31, 31),
                 (64 + f, 32), (50, 64 + f)):
        noisy[y, x] *= F32(50.0)
    fr["noisy"] = noisy.reshape(-1)
    return fr


@functools.lru_cache(maxsize=None)
def _untiled_filtered_run(radius: int, frames: int):
    """Per frame (the untiled filter's plane, the untiled output) on the GPU."""
    den = bmfr_amd.Denoiser(_cfg())
    out = []
    for f in range(frames):
        fr = _still_frame(f)
        d = {k: torch.from_numpy(np.array(fr[k])).cuda() for k in ("noisy", "normals", "positions", "albedo")}
        flt = den.suppress_fireflies(d["noisy"], radius=radius)
        den.process_frame(flt, d["normals"], d["positions"], d["albedo"], fr["prev_vp"], fr["jitter"], f)
        out.append((flt.cpu().numpy(), den.copy_output(torch.empty(W * H * 3, device="cuda")).cpu().numpy()))
    assert den.frame_status() == 0
    return out


@pytest.mark.parametrize("radius", [1, 2])
@pytest.mark.parametrize("gx,gy", [(2, 1), (1, 2)], ids=["2x1", "1x2"])
def test_tiled_filter_then_frame_equals_untiled(gx, gy, radius, gpu):
    frames, halo = 3, 34
    want = _untiled_filtered_run(radius, frames)
    grid = TileGrid(W, H, gx, gy, halo=halo)
    tiles = [bmfr_amd.Denoiser(_cfg(tile=grid.tile(r), tile_halo=halo)) for r in range(grid.ranks)]
    assert any(d.region != (0, 0, W, H) for d in tiles)
    loop = LoopbackTransport(grid)
    prev = None
    for f in range(frames):
        fr = _still_frame(f)
        full = {k: torch.from_numpy(np.array(fr[k])).cuda() for k in ("noisy", "normals", "positions", "albedo")}
        calls = []
        for d in tiles:
            cut = lambda t: region_slice(t, W, H, d.region).reshape(-1)  # noqa: E731
            flt = d.suppress_fireflies(cut(full["noisy"]), radius=radius)
            # the filtered region plane against the untiled filter's, outside the rings
            x0, y0, rw, rh = d.region
            keep = ~fn.differing_rings(W, H, d.region, radius)
            a = flt.cpu().numpy().reshape(rh, rw, 3)
            b = want[f][0].reshape(H, W, 3)[y0:y0 + rh, x0:x0 + rw]
            _same(a[keep], b[keep], (f, d.region, "filtered plane"))
            kw = {}
            if f > 0:
                kw = dict(prev_normals=cut(prev["normals"]), prev_positions=cut(prev["positions"]))
            calls.append((d, [flt, cut(full["normals"]), cut(full["positions"]), cut(full["albedo"]), fr["prev_vp"],
                              fr["jitter"], f], kw))
        if f == 0:
            for d, a, kw in calls:
                d.process_frame(*a, **kw)
        else:  # tiling.process_frame_tiled's order
            for d, a, kw in calls:
                d.process_frame_interior(*a, **kw)
            loop.exchange_all_ctx(tiles, f)
            for d, a, kw in calls:
                d.process_frame_border(*a, **kw)
        prev = full
        for r, d in enumerate(tiles):
            x0, y0, rw, rh = d.region
            tx, ty, tw, th = grid.tile(r)
            got = d.copy_output(torch.empty(rw * rh * 3, device="cuda")).cpu().numpy().reshape(rh, rw, 3)
            a = np.ascontiguousarray(got[ty - y0:ty - y0 + th, tx - x0:tx - x0 + tw])
            b = np.ascontiguousarray(want[f][1].reshape(H, W, 3)[ty:ty + th, tx:tx + tw])
            _same(a, b, (f, r, "output"))
    for d in tiles:
        assert d.halo_status() == 0 and d.frame_status() == 0


# -------------------------------------------------------- process_gbuffer --
@pytest.mark.parametrize("half", [0, 1], ids=["f32", "input_half"])
def test_process_gbuffer_with_firefly(half, gpu):
    """process_gbuffer(firefly=...) against prepare -> suppress_fireflies ->
    process_frame by hand, and firefly=None against the call without it:
    output and every state plane byte for byte, 3 frames."""
    frames, region = 3, (0, 0, W, H)
    rule = dict(threshold=2.0, radius=2, floor=0.01)
    kw = dict(radiance="f16", albedo="unorm8", normals="oct", positions="depth", motion="f16", objects=5,
              at_centre=1, motion_scale=(64.0, -40.0))
    A, B, C0, D = (bmfr_amd.Denoiser(_cfg(input_half=half)) for _ in range(4))
    dev = lambda g: {k: (torch.from_numpy(v.view(np.int16) if v.dtype == np.uint16 else v).cuda()  # noqa: E731
                         if k in pn.PLANE_KEYS else v) for k, v in g.items()}
    stats = torch.zeros(2, dtype=torch.int32, device="cuda")
    sets = [None, None]
    for f in range(frames):
        fr = bmfr_amd.synth_frame_host(W, H, f)
        vp, jit = bmfr_amd.synth_camera(W, H, f)
        prev_vp = bmfr_amd.synth_camera(W, H, max(f - 1, 0))[0]
        g = pn.make_gbuffer(fr, vp, W, H, region, 700 + f, bool(half), **kw)
        del g["prev_positions"], g["prev_normals"]   # the denoiser's own last planes
        gd = dev(g)
        A.process_gbuffer(gd, prev_vp, jit, f, firefly=dict(rule, stats=stats))
        C0.process_gbuffer(gd, prev_vp, jit, f)
        D.process_gbuffer(gd, prev_vp, jit, f, firefly=None)
        # by hand, on B
        gb = dict(gd)
        if f:
            gb["prev_positions"], gb["prev_normals"] = sets[1 - f % 2]["positions"], sets[1 - f % 2]["normals"]
        p = B.prepare(gb, jit)
        sets[f % 2] = p
        flt = B.suppress_fireflies(p["noisy"], **rule)
        B.process_frame(flt, p["normals"], p["positions"], p["albedo"], prev_vp, jit, f,
                        prev_normals=p["prev_normals_moved"] if f else None,
                        prev_positions=p["prev_positions_moved"] if f else None,
                        prev_pixel=p["prev_pixel"] if f else None)
        a, b, c, d = state_snapshot(A), state_snapshot(B), state_snapshot(C0), state_snapshot(D)
        for name in b:
            _same(a[name], b[name], (f, name, "firefly"))
            _same(d[name], c[name], (f, name, "firefly=None"))
        if f == frames - 1:
            assert not np.array_equal(a["result"], c["result"])   # the filter did something
    assert stats.cpu().tolist()[0] > 0
    for den in (A, B, C0, D):
        assert den.frame_status() == 0


# ------------------------------------------------------------------- host --
@pytest.mark.parametrize("radius", [1, 2])
def test_host_firefly_flag_matches_python_loop(tmp_path, radius, gpu):
    """bmfr_host --firefly 2 [--firefly-radius 2] against the Python
    filter-then-frame loop on the same frames, compared as
    tests/test_gpu_host.py compares the host's files with the library."""
    w, h, frames = 160, 96, 4
    exe = _build.build_host()
    args = ["--synthetic", "--width", str(w), "--height", str(h), "--frames", str(frames), "--exr", "--output",
            str(tmp_path / "ff_"), "--firefly", "2"] + (["--firefly-radius", "2"] if radius == 2 else [])
    r = subprocess.run([exe, *args], cwd=tmp_path, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout + r.stderr
    io = C.CDLL(_build.IO_LIB)
    io.bmfr_exr_read_rgb.argtypes = [C.c_char_p, C.c_int, C.c_int, C.c_void_p]
    den = bmfr_amd.Denoiser(bmfr_amd.BmfrConfig(image_width=w, image_height=h))
    plain = bmfr_amd.Denoiser(bmfr_amd.BmfrConfig(image_width=w, image_height=h))
    problems, differs = [], False
    for f in range(frames):
        fr = {k: torch.from_numpy(v.reshape(-1)).cuda() for k, v in bmfr_amd.synth_frame_host(w, h, f).items()}
        vp, _ = bmfr_amd.synth_camera(w, h, max(f - 1, 0))
        _, jit = bmfr_amd.synth_camera(w, h, f)
        flt = den.suppress_fireflies(fr["noisy"], threshold=2.0, radius=radius)
        den.process_frame(flt, fr["normals"], fr["positions"], fr["albedo"], vp, jit, f)
        plain.process_frame(fr["noisy"], fr["normals"], fr["positions"], fr["albedo"], vp, jit, f)
        want = den.copy_output(torch.empty(w * h * 3, device="cuda")).cpu().numpy().reshape(h, w, 3)
        other = plain.copy_output(torch.empty(w * h * 3, device="cuda")).cpu().numpy().reshape(h, w, 3)
        differs = differs or not np.array_equal(want, other)
        got = np.empty((h, w, 3), np.float32)
        assert io.bmfr_exr_read_rgb(str(tmp_path / f"ff_{f}.exr").encode(), w, h, got.ctypes.data) == 0
        bad = got.view(np.uint32) != want.view(np.uint32)
        if bad.any():
            problems.append(f"frame {f}: {int(bad.sum())} of {bad.size} floats differ, first at "
                            f"{np.argwhere(bad)[0].tolist()}, max |diff| {float(np.abs(got - want).max()):.3g}")
    assert not problems, "\n".join(problems)
    assert differs, "the filter changed nothing on this content: the comparison shows nothing"
