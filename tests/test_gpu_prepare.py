"""The G-buffer front end on the GPU (bmfr_prepare_frame, include/bmfr.h;
Denoiser.prepare / process_gbuffer): the kernel against the numpy restatement
(tests/prepare_np.py) byte for byte, tiles against the whole frame, and the
conventions -- jitter, row direction, half pixel, object motion -- end to end
against what the existing kernels do with the prepared planes."""
from __future__ import annotations

import functools

import numpy as np
import pytest
import torch

import bmfr_amd
from bmfr_amd.tiling import TileGrid
import prepare_np as pn
from motion_util import T, quantise, scene_frame, translated
from parity_harness import STATE, assert_same_array, state_snapshot
from seq_util import GARBAGE_JITTER, NAN_VP

pytestmark = pytest.mark.gpu

F32 = np.float32

# name -> make_gbuffer keywords.  Together: every listed format of every plane.
GBUFFERS = {
    # what an engine has: RGBA16F radiance, 8-bit albedo, octahedral normals, depth, RG16F motion in NDC units
    # against the rows at pixel centres, an object table
    "engine": dict(radiance="f16", albedo="unorm8", normals="oct", positions="depth", motion="f16", objects=5,
                   at_centre=1, motion_scale=(64.0, -40.0)),
    # the library's own vocabulary: f32 everywhere, positions given
    "reference": dict(radiance="f32", albedo="f32", normals="f32", positions="given", motion="f32", objects=3),
    # the remaining formats; NaN albedo; no object table and no id plane (the previous planes are copied)
    "mixed": dict(radiance="f32", albedo="f16", normals="f16", positions="depth", motion="f32", objects=0,
                  with_nan=True),
    "nan_f32": dict(radiance="f16", albedo="f32", normals="oct", positions="depth", motion="f16", objects=1,
                    with_nan=True),
}


def _cfg(W, H, **kw):
    return bmfr_amd.BmfrConfig(image_width=W, image_height=H, **kw)


def _tensor(a):
    if isinstance(a, np.ndarray):
        return torch.from_numpy(a.view(np.int16) if a.dtype == np.uint16 else a).cuda()
    return a


def _dev(g: dict) -> dict:
    return {k: (_tensor(v) if k in pn.PLANE_KEYS else v) for k, v in g.items()}


def _host(t: torch.Tensor) -> np.ndarray:
    return t.cpu().numpy()


@functools.lru_cache(maxsize=None)
def _synth(W, H, f):
    fr = bmfr_amd.synth_frame_host(W, H, f)
    vp, jit = bmfr_amd.synth_camera(W, H, f)
    return fr, vp, jit


# ------------------------------------------------------------------ test 1 --
# 128 x 80: whole groups only; 101 x 75 = 7575 pixels: 3 (float3) / 7 (half3) pixels past the last group
@pytest.mark.parametrize("W,H", [(128, 80), (101, 75)])
@pytest.mark.parametrize("half", [0, 1], ids=["f32", "input_half"])
@pytest.mark.parametrize("name", list(GBUFFERS))
def test_kernel_equals_restatement(name, half, W, H, gpu):
    fr, vp, jit = _synth(W, H, 3)
    region = (0, 0, W, H)
    g = pn.make_gbuffer(fr, vp, W, H, region, 1234, bool(half), **GBUFFERS[name])
    want = pn.prepare(g, jit, region, W, H, bool(half))
    assert set(want) == set(pn.OUTPUTS)
    den = bmfr_amd.Denoiser(_cfg(W, H, input_half=half))
    got = den.prepare(_dev(g), jit)
    torch.cuda.synchronize()
    assert set(got) == set(want)
    nan_in = bool(GBUFFERS[name].get("with_nan"))
    for k in pn.OUTPUTS:
        assert_same_array(_host(got[k]), want[k], (name, k), nan_aware=nan_in and k == "albedo")
    if nan_in:
        assert np.isnan(want["albedo"].astype(F32)).any() and np.isfinite(want["noisy"].astype(F32)).all()


@pytest.mark.parametrize("half", [0, 1], ids=["f32", "input_half"])
def test_planes_off_16_byte_alignment(half, gpu):
    """Planes one pixel into a larger allocation (element-aligned, not 16-byte
    aligned) take the one-pixel-per-thread path: same bytes.  A subset of the
    outputs is requested; the others' pointers stay NULL and untouched."""
    W, H = 101, 75
    n = W * H
    fr, vp, jit = _synth(W, H, 3)
    region = (0, 0, W, H)
    g = pn.make_gbuffer(fr, vp, W, H, region, 99, bool(half), **GBUFFERS["engine"])
    outputs = ("noisy", "positions", "prev_pixel", "prev_normals_moved")
    want = pn.prepare(g, jit, region, W, H, bool(half), outputs=outputs)

    def shifted(a):
        per = a.numel() // n
        big = torch.empty(a.numel() + per, dtype=a.dtype, device="cuda")
        big[per:].copy_(a)
        return big[per:]

    gd = {k: (shifted(v) if isinstance(v, torch.Tensor) and k != "object_transforms" else v) for k, v in _dev(g).items()}
    assert gd["albedo"].data_ptr() % 16 != 0
    dt = torch.float16 if half else torch.float32
    out = {k: shifted(torch.zeros(n * (2 if k == "prev_pixel" else 3), dtype=torch.float32 if k == "prev_pixel" else dt,
                                  device="cuda")) for k in outputs}
    den = bmfr_amd.Denoiser(_cfg(W, H, input_half=half))
    den.prepare(gd, jit, out=out)
    torch.cuda.synchronize()
    for k in outputs:
        assert_same_array(_host(out[k]), want[k], k)


# ------------------------------------------------------------------ test 2 --
def test_tiled_regions_match_untiled(gpu):
    """352 x 224 as 2 x 1 tiles with halo 48: each tile context's prepared
    region equals the same pixels of the untiled result.  Depth and motion at
    pixel centres are among the inputs: both depend on image coordinates."""
    W, H, halo = 352, 224, 48
    fr, vp, jit = _synth(W, H, 2)
    full = (0, 0, W, H)
    g = pn.make_gbuffer(fr, vp, W, H, full, 4321, False, **GBUFFERS["engine"])
    whole = bmfr_amd.Denoiser(_cfg(W, H)).prepare(_dev(g), jit)
    torch.cuda.synchronize()
    want = pn.prepare(g, jit, full, W, H, False)
    for k in pn.OUTPUTS:
        assert_same_array(_host(whole[k]), want[k], ("untiled", k))
    grid = TileGrid(W, H, 2, 1, halo=halo)
    per_pixel = {k: np.asarray(v).size // (W * H) for k, v in g.items() if k in pn.PLANE_KEYS and k != "object_transforms"}
    for r in range(grid.ranks):
        den = bmfr_amd.Denoiser(_cfg(W, H, tile=grid.tile(r), tile_halo=halo))
        region = den.region
        assert region != full and (region[2], region[3]) == (den.sizes.region_width, den.sizes.region_height)
        gt = {k: (pn.region_of(v, W, H, region) if k in per_pixel else v) for k, v in g.items()}
        got = den.prepare(_dev(gt), jit)
        torch.cuda.synchronize()
        for k in pn.OUTPUTS:
            assert_same_array(_host(got[k]), pn.region_of(_host(whole[k]), W, H, region), (r, k))


# ------------------------------------------------------------------ test 3 --
def _moving_world(ids_value: int):
    """test_gpu_motion_input.py::test_moving_world's runs X (static world by
    matrix) and Y (the world translated by f T at frame f, prev_pixel from X, a
    NaN matrix), with Y's previous planes moved into the current world by
    bmfr_prepare_frame: one object, identity rotation, translation T, every
    pixel's id = ids_value.  -> per frame (X's, Y's) spp / noisy_accumulated /
    prev_frame_pixel."""
    W, H, frames = 128, 80, 9
    n = W * H
    names = (STATE[0], STATE[1], STATE[4])
    X, Y = (bmfr_amd.Denoiser(_cfg(W, H)) for _ in range(2))
    table = torch.tensor([1, 0, 0, T[0], 0, 1, 0, T[1], 0, 0, 1, T[2]], dtype=torch.float32, device="cuda")
    ids = torch.full((n,), ids_value, dtype=torch.int32).to(torch.int16).cuda()
    pos_q, y_prev, out = None, None, []
    t = lambda a: torch.from_numpy(a).cuda()  # noqa: E731
    for f in range(frames):
        fr = scene_frame("synth", W, H, f)
        d = {k: t(np.array(fr[k])) for k in ("noisy", "normals", "albedo")}
        prev_q, pos_q = pos_q, quantise(fr["positions"])
        X.process_frame(d["noisy"], d["normals"], t(pos_q), d["albedo"], fr["prev_vp"], fr["jitter"], f,
                        prev_positions=t(prev_q) if f else None, prev_normals=X.prev_inputs[0] if f else None)
        x = state_snapshot(X, names)
        cur = t(translated(pos_q, f))
        moved = None
        if f:
            moved = Y.prepare({"prev_positions": y_prev[0], "prev_normals": y_prev[1], "prev_object_id": ids,
                               "object_transforms": table}, fr["jitter"])
            assert set(moved) == {"prev_positions_moved", "prev_normals_moved"}
        Y.process_frame(d["noisy"], d["normals"], cur, d["albedo"], NAN_VP, GARBAGE_JITTER, f,
                        prev_positions=moved["prev_positions_moved"] if f else None,
                        prev_normals=moved["prev_normals_moved"] if f else None,
                        prev_pixel=t(x["prev_frame_pixel"]) if f else None)
        y_prev = (cur, d["normals"])
        out.append((x, state_snapshot(Y, names)))
    assert X.frame_status() == 0 and Y.frame_status() == 0
    return out


def test_moving_world_through_prepare(gpu):
    """Every id 0: the previous planes move with the world, so the history K1
    gathers in Y equals X's byte for byte, every frame."""
    for f, (x, y) in enumerate(_moving_world(0)):
        for name in x:
            assert_same_array(y[name], x[name], ("moving world", f, name))


def test_moving_world_ids_past_the_table(gpu):
    """Every id 0xFFFF: the planes are copied, not moved, so the position test
    rejects the history as in run Z of test_moving_world: mean spp falls below X's."""
    x, y = _moving_world(0xFFFF)[-1]
    sx, sy = x["spp"].mean(), y["spp"].mean()
    print(f"mean spp after 9 frames: static world {sx:.3f}, ids past the table {sy:.3f}")
    assert sy < sx


# ------------------------------------------------------------------ test 4 --
def test_motion_vectors_against_projection(gpu):
    """A projecting context's prev_frame_pixel plane turned into motion vectors
    (mv = (x, y) - plane, f64 -> F32X2, taken at the jittered sample) and back
    through bmfr_prepare_frame: within 1e-4 px of the plane where that is
    finite and inside the image (a few f32 spacings at coordinates below 256);
    a context fed the prepared plane under a NaN matrix reaches the same spp on
    at least 99 % of the pixels of every frame (a pixel can differ where the
    round trip moves an entry across an integer).  The test prints the
    distance and the share it observed."""
    W, H, frames = 128, 80, 6
    n = W * H
    region = (0, 0, W, H)
    A, B = (bmfr_amd.Denoiser(_cfg(W, H)) for _ in range(2))
    xs, ys = pn.coords(region, np.float64)
    worst_px, worst_share = 0.0, 0.0
    for f in range(frames):
        fr = scene_frame("synth", W, H, f)
        d = {k: torch.from_numpy(np.array(fr[k])).cuda() for k in ("noisy", "normals", "positions", "albedo")}
        A.process_frame(d["noisy"], d["normals"], d["positions"], d["albedo"], fr["prev_vp"], fr["jitter"], f)
        a = state_snapshot(A, (STATE[1], STATE[4]))
        plane = a["prev_frame_pixel"].reshape(n, 2).astype(np.float64)
        with np.errstate(all="ignore"):
            mv = np.stack([xs - plane[:, 0], ys - plane[:, 1]], axis=-1).astype(F32)
        got = B.prepare({"motion": torch.from_numpy(mv.reshape(-1)).cuda()}, fr["jitter"])
        assert set(got) == {"prev_pixel"}
        pp = _host(got["prev_pixel"]).reshape(n, 2).astype(np.float64)
        inside = np.isfinite(plane).all(axis=1) & (plane[:, 0] >= 0) & (plane[:, 0] < W) & (plane[:, 1] >= 0) & \
            (plane[:, 1] < H)
        assert inside.mean() > 0.5
        worst_px = max(worst_px, np.abs(pp - plane)[inside].max())
        B.process_frame(d["noisy"], d["normals"], d["positions"], d["albedo"], NAN_VP, GARBAGE_JITTER, f,
                        prev_pixel=got["prev_pixel"] if f else None)
        share = (state_snapshot(B, (STATE[1],))["spp"] != a["spp"]).mean()
        worst_share = max(worst_share, share)
    print(f"prepared prev_pixel vs projection: max {worst_px:.2e} px inside the image; "
          f"spp differs on at most {100 * worst_share:.3f} % of pixels per frame")
    assert worst_px <= 1e-4
    assert worst_share <= 0.01
    assert A.frame_status() == 0 and B.frame_status() == 0


# ------------------------------------------------------------------ test 5 --
@pytest.mark.parametrize("half", [0, 1], ids=["f32", "input_half"])
def test_process_gbuffer_equals_process_frame(half, gpu):
    """process_gbuffer (prepare + process_frame on the denoiser's two
    alternating sets of planes) against process_frame fed the restated planes:
    output and every state plane byte for byte, 4 frames.  Frame f + 1 moves
    frame f's prepared positions / normals: a set reused too early shows."""
    W, H, frames = 128, 80, 4
    region = (0, 0, W, H)
    A = bmfr_amd.Denoiser(_cfg(W, H, input_half=half))
    B = bmfr_amd.Denoiser(_cfg(W, H, input_half=half))
    last = None
    for f in range(frames):
        fr, vp, jit = _synth(W, H, f)
        prev_vp = _synth(W, H, max(f - 1, 0))[1]
        g = pn.make_gbuffer(fr, vp, W, H, region, 500 + f, bool(half), **GBUFFERS["engine"])
        del g["prev_positions"], g["prev_normals"]   # the denoiser's own last planes
        A.process_gbuffer(_dev(g), prev_vp, jit, f)
        gr = dict(g)
        if f:
            gr["prev_positions"], gr["prev_normals"] = last["positions"], last["normals"]
        want = pn.prepare(gr, jit, region, W, H, bool(half))
        w = {k: torch.from_numpy(v).cuda() for k, v in want.items()}
        B.process_frame(w["noisy"], w["normals"], w["positions"], w["albedo"], prev_vp, jit, f,
                        prev_normals=w["prev_normals_moved"] if f else None,
                        prev_positions=w["prev_positions_moved"] if f else None,
                        prev_pixel=w["prev_pixel"] if f else None)
        last = want
        a, b = state_snapshot(A), state_snapshot(B)
        for name in b:
            assert_same_array(a[name], b[name], (f, name))
    assert A.frame_status() == 0 and B.frame_status() == 0
