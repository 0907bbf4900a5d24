"""Caller-supplied previous-frame pixel planes (bmfr_frame_inputs.prev_pixel,
include/bmfr.h): K1 reads where each pixel was in the previous frame from a
plane instead of projecting its world position through the previous camera.

The handle on exactness: K1 stores the position it used in the context's
prev_frame_pixel plane, so a second context fed that plane -- and a NaN
camera matrix and a garbage pixel offset, to show neither is read -- must
reproduce the first one byte for byte, every frame, output and state.

Planes are compared as bytes (NaNs compare)."""
from __future__ import annotations

import ctypes as C
import functools
import subprocess

import numpy as np
import pytest
import torch

import bmfr_amd
from bmfr_amd import _build, _lib
from bmfr_amd.tiling import NativeExchange, TileGrid, process_frame_tiled, region_slice
from motion_util import REACH_SIZE, bad_entries, quantise, scene_frame, shifted, translated
from parity_harness import STATE, state_snapshot
from seq_util import GARBAGE_JITTER, NAN_VP, PLANES

pytestmark = pytest.mark.gpu

FRAMES = 18          # all 16 block-grid shifts and the wrap

# name -> (BmfrConfig keywords, how context B runs its frames)
CONFIGS = {
    "half13": ({}, "frame"),                                                    # column-split K1, B = 13
    "half16": ({"scaled": bmfr_amd.SCALED_THIRD_ORDER}, "frame"),                # column-split K1, B = 16
    "f32": ({"use_half_precision_in_tmp_data": 0}, "frame"),                    # row-split K1
    "f32_fast": ({"use_half_precision_in_tmp_data": 0, "fast_fit": 1}, "frame"),  # column-split K1, f32 tmp_data
    "generic10": ({"scaled": bmfr_amd.SCALED_DEFAULT[:3]}, "frame"),            # generic-feature K1, B = 10
    "input_half": ({"input_half": 1}, "frame"),                                 # pair taps
    "input_half16": ({"input_half": 1, "scaled": bmfr_amd.SCALED_THIRD_ORDER}, "frame"),
    "fast_fit": ({"fast_fit": 1}, "frame"),                                     # against itself
    "two_launch": ({}, "two_launch"),                                           # K1 and K2 as two launches
    "sequence": ({}, "sequence"),                                               # bmfr_process_sequence
    "split": ({}, "split"),                                                     # _interior + _border
}
# scene, width, height: neither size is a multiple of 32 (mirrored margins, narrow edge blocks)
SCENES = (("synth", 128, 80), ("pan", 100, 72), ("clamp", 128, 80))


def _scene_for(scene: str, kw: dict) -> str:
    # f32 tmp_data has no +-65504 clamp: scenes_np's form of the scene for it
    return "clamp_nan" if scene == "clamp" and not kw.get("use_half_precision_in_tmp_data", 1) else scene


def _cfg(W, H, kw):
    return bmfr_amd.BmfrConfig(image_width=W, image_height=H, **kw)


def _dev(fr: dict, half: bool) -> dict:
    out = {k: torch.from_numpy(np.array(fr[k])).cuda() for k in PLANES}
    return {k: v.half() for k, v in out.items()} if half else out


def _state(den, names=STATE) -> dict:
    """The named state planes of the last frame, as bytes."""
    return {name: a.tobytes() for name, a in state_snapshot(den, names).items()}


def _frozen(kw: dict):
    return tuple(sorted(kw.items()))


@functools.lru_cache(maxsize=None)
def _reference(kw_items, scene: str, W: int, H: int, frames: int = FRAMES):
    """Context A: the frames by camera matrix.  Per frame its state planes
    (prev_frame_pixel among them: the plane context B is fed).  Computed once
    per configuration and scene, shared by the tests, never modified."""
    kw = dict(kw_items)
    den = bmfr_amd.Denoiser(_cfg(W, H, kw))
    out = []
    for f in range(frames):
        fr = scene_frame(scene, W, H, f)
        d = _dev(fr, kw.get("input_half", 0))
        den.process_frame(d["noisy"], d["normals"], d["positions"], d["albedo"], fr["prev_vp"], fr["jitter"], f)
        out.append(_state(den))
    assert den.frame_status() == 0
    return tuple(out)


def _plane(rec: dict) -> torch.Tensor:
    return torch.from_numpy(np.frombuffer(rec["prev_frame_pixel"], np.float32).copy()).cuda()


def _compare(got: dict, want: dict, what):
    for name in want:
        if name not in got:
            continue
        a, b = np.frombuffer(got[name], np.uint8), np.frombuffer(want[name], np.uint8)
        bad = np.flatnonzero(a != b)
        assert bad.size == 0, (what, name, f"{bad.size} of {a.size} bytes differ, first at byte {int(bad[0])}")


# ------------------------------------------------------------------ test 1 --
@pytest.mark.parametrize("scene,W,H", SCENES, ids=[s[0] for s in SCENES])
@pytest.mark.parametrize("config", list(CONFIGS))
def test_replay_equals_projection(config, scene, W, H, gpu):
    kw, mode = CONFIGS[config]
    scene = _scene_for(scene, kw)
    half = kw.get("input_half", 0)
    ref = _reference(_frozen(kw), scene, W, H)
    den = bmfr_amd.Denoiser(_cfg(W, H, kw))
    if mode == "two_launch":
        den.debug_frame_launches(2)
    n = W * H
    nan_plane = torch.full((n * 2,), float("nan"), device="cuda")  # frame 0 ignores the plane
    if mode == "sequence":
        # chunks [0, 7) and [7, 18); frames 3, 8, 13 carry no plane and the true camera
        for lo, hi in ((0, 7), (7, FRAMES)):
            frames, cams, outs = [], [], []
            for f in range(lo, hi):
                fr = scene_frame(scene, W, H, f)
                d = _dev(fr, half)
                by_matrix = f % 5 == 3
                d["prev_pixel"] = None if by_matrix else (nan_plane if f == 0 else _plane(ref[f]))
                frames.append(d)
                cams.append((fr["prev_vp"], fr["jitter"]) if by_matrix else (NAN_VP, GARBAGE_JITTER))
                outs.append(torch.empty(n * 3, device="cuda"))
            den.process_sequence(frames, cams, lo, outputs=outs)
            torch.cuda.synchronize()
            for f, o in zip(range(lo, hi), outs):
                _compare({"result": o.cpu().numpy().tobytes()}, {"result": ref[f]["result"]}, (config, scene, f))
            _compare(_state(den), ref[hi - 1], (config, scene, hi - 1))
        assert den.frame_status() == 0
        return
    for f in range(FRAMES):
        fr = scene_frame(scene, W, H, f)
        d = _dev(fr, half)
        args = (d["noisy"], d["normals"], d["positions"], d["albedo"], NAN_VP, GARBAGE_JITTER, f)
        plane = nan_plane if f == 0 else _plane(ref[f])
        if mode == "split":
            den.process_frame_interior(*args, prev_pixel=plane)
            den.process_frame_border(*args, prev_pixel=plane)
        else:
            den.process_frame(*args, prev_pixel=plane)
        _compare(_state(den), ref[f], (config, scene, f))
    assert den.frame_status() == 0


def test_nan_matrix_without_plane_differs(gpu):
    """The control: without the plane the NaN matrix does reach the output."""
    scene, W, H = SCENES[0]
    ref = _reference(_frozen({}), scene, W, H)
    den = bmfr_amd.Denoiser(_cfg(W, H, {}))
    for f in range(2):
        fr = scene_frame(scene, W, H, f)
        d = _dev(fr, False)
        den.process_frame(d["noisy"], d["normals"], d["positions"], d["albedo"], NAN_VP, fr["jitter"], f)
    assert _state(den)["result"] != ref[1]["result"]


# ------------------------------------------------------------------ test 2 --
def _tiled_contexts(W, H, grid, halo):
    tiles = [bmfr_amd.Denoiser(bmfr_amd.BmfrConfig(image_width=W, image_height=H, tile=grid.tile(r), tile_halo=halo))
             for r in range(grid.ranks)]
    return tiles, [NativeExchange(d, grid, r, None) for r, d in enumerate(tiles)]


def _tile_bytes(a: bytes, dtype, region, tile):
    rx, ry, rw, rh = region
    x, y, w, h = tile
    v = np.frombuffer(a, dtype).reshape(rh, rw, -1)
    return v[y - ry:y - ry + h, x - rx:x - rx + w].tobytes()


@pytest.mark.parametrize("W,H,tx,ty,halo", [(352, 224, 2, 1, 48), (256, 320, 1, 2, 40)], ids=["2x1", "1x2"])
def test_tiled_planes_match_untiled(W, H, tx, ty, halo, gpu):
    """Each rank is fed its region's slice of the untiled run's planes (and a
    NaN matrix); the halo moves by device copies.  Tile outputs and state ==
    the untiled run's, bit for bit."""
    frames = 8
    ref = _reference(_frozen({}), "synth", W, H, frames)
    grid = TileGrid(W, H, tx, ty, halo=halo)
    tiles, xs = _tiled_contexts(W, H, grid, halo)
    prev = None
    for f in range(frames):
        fr = scene_frame("synth", W, H, f)
        d = _dev(fr, False)
        process_frame_tiled(tiles, d, NAN_VP, GARBAGE_JITTER, f, exchange=lambda k: NativeExchange.run_all(xs, k),
                            prev_planes=prev, prev_pixel=_plane(ref[f]) if f > 0 else None)
        prev = d
        torch.cuda.synchronize()
        for r, t in enumerate(tiles):
            assert t.halo_status() == 0
            got = _state(t)
            for name, ch, dt in STATE:
                np_dt = np.uint8 if dt == torch.uint8 else np.uint32
                a = _tile_bytes(got[name], np_dt, t.region, grid.tile(r))
                b = _tile_bytes(ref[f][name], np_dt, (0, 0, W, H), grid.tile(r))
                assert a == b, (f, r, name)


def _halo_status(den):
    over = C.c_uint()
    st = den.lib.bmfr_halo_status(den.handle, C.byref(over))
    return st, over.value


@pytest.mark.parametrize("dx", [40.0, -40.0])
def test_reach_exceeded_through_planes(dx, gpu):
    """tests/test_gpu_reach.py's scenario (40 px of motion, 40 px halo, 2 x 2
    grid) replayed through planes: the plane of the untiled run under the
    shifted camera sends the same taps past the same tiles' valid state, so
    the same tiles report BMFR_ERROR_HALO_EXCEEDED with the same overshoot as
    tiles driven by the matrix."""
    W, H, HALO = REACH_SIZE
    grid = TileGrid(W, H, 2, 2, halo=HALO)
    full = bmfr_amd.Denoiser(bmfr_amd.BmfrConfig(image_width=W, image_height=H))
    by_matrix, xm = _tiled_contexts(W, H, grid, HALO)
    by_plane, xp = _tiled_contexts(W, H, grid, HALO)
    prev = None
    for f in range(2):
        fr = scene_frame("synth", W, H, f)
        d = _dev(fr, False)
        vp = shifted(fr["prev_vp"], dx, W) if f > 0 else fr["prev_vp"]
        full.process_frame(d["noisy"], d["normals"], d["positions"], d["albedo"], vp, fr["jitter"], f)
        plane = _plane(_state(full, STATE[4:])) if f > 0 else None
        process_frame_tiled(by_matrix, d, vp, fr["jitter"], f, exchange=lambda k: NativeExchange.run_all(xm, k),
                            prev_planes=prev)
        process_frame_tiled(by_plane, d, NAN_VP, GARBAGE_JITTER, f, exchange=lambda k: NativeExchange.run_all(xp, k),
                            prev_planes=prev, prev_pixel=plane)
        prev = d
    want = [_halo_status(t) for t in by_matrix]
    got = [_halo_status(t) for t in by_plane]
    flagged = [r for r in range(grid.ranks) if (r % 2 == 0) == (dx > 0)]
    assert [r for r, (st, _) in enumerate(want) if st == _lib.HALO_EXCEEDED] == flagged, want
    assert all(over > 0 for r, (_, over) in enumerate(want) if r in flagged), want
    assert got == want


# ------------------------------------------------------------------ test 3 --
def test_moving_world(gpu):
    """X: the static world (positions quantised to 2^-8) under the moving
    camera, by matrix.  Y: the same frames with the whole world translated by
    f T at frame f, prev_positions moved into the current frame's world,
    prev_pixel from X and a NaN matrix: every previous - current difference
    equals X's exactly (motion_util), so the history K1 gathers -- spp,
    noisy_accumulated, prev_frame_pixel -- equals X's byte for byte; only the
    fit, whose features are positions, may differ.  Z: what a caller can do
    without the plane (the moved world, X's matrices, prev_positions as
    rendered): the position test rejects the history, so its spp stays low."""
    W, H, frames = 128, 80, 9
    names = (STATE[0], STATE[1], STATE[4])
    X, Y, Z = (bmfr_amd.Denoiser(_cfg(W, H, {})) for _ in range(3))
    pos_q, moved_prev = None, None
    for f in range(frames):
        fr = scene_frame("synth", W, H, f)
        d = _dev(fr, False)
        prev_q, pos_q = pos_q, quantise(fr["positions"])
        cur = translated(pos_q, f)
        t = lambda a: torch.from_numpy(a).cuda()  # noqa: E731
        X.process_frame(d["noisy"], d["normals"], t(pos_q), d["albedo"], fr["prev_vp"], fr["jitter"], f,
                        prev_positions=t(prev_q) if f else None, prev_normals=X.prev_inputs[0] if f else None)
        x = _state(X, names)
        Y.process_frame(d["noisy"], d["normals"], t(cur), d["albedo"], NAN_VP, GARBAGE_JITTER, f,
                        prev_positions=t(translated(prev_q, f)) if f else None,
                        prev_normals=Y.prev_inputs[0] if f else None, prev_pixel=_plane(x) if f else None)
        _compare(_state(Y, names), x, ("moving world", f))
        Z.process_frame(d["noisy"], d["normals"], t(cur), d["albedo"], fr["prev_vp"], fr["jitter"], f,
                        prev_positions=t(moved_prev) if f else None, prev_normals=Z.prev_inputs[0] if f else None)
        moved_prev = cur
    spp = lambda den: np.frombuffer(_state(den, (STATE[1],))["spp"], np.uint8).mean()  # noqa: E731
    sx, sz = spp(X), spp(Z)
    print(f"mean spp after {frames} frames: static world {sx:.3f}, moved world without the plane {sz:.3f}")
    assert sz < sx


# ------------------------------------------------------------------ test 4 --
@pytest.mark.parametrize("config", ["half13", "f32", "generic10", "input_half"])
def test_out_of_image_entries(config, gpu):
    """A fixed seeded 5 % of a frame's entries overwritten with values all of
    whose taps lie outside the image (motion_util.bad_entries): those pixels
    start over (spp 1, accumulated colour = current colour), the status stays
    BMFR_OK, and every other pixel's spp / noisy_accumulated is the replay's."""
    kw, _ = CONFIGS[config]
    scene, W, H = SCENES[0]
    half = kw.get("input_half", 0)
    frames = 4
    ref = _reference(_frozen(kw), scene, W, H)
    den = bmfr_amd.Denoiser(_cfg(W, H, kw))
    n = W * H
    picked = np.random.RandomState(20240611).permutation(n)[:n // 20]
    entries = bad_entries(W, H)
    for f in range(frames):
        fr = scene_frame(scene, W, H, f)
        d = _dev(fr, half)
        plane = None
        if f > 0:
            p = np.frombuffer(ref[f]["prev_frame_pixel"], np.float32).copy().reshape(n, 2)
            if f == frames - 1:
                p[picked] = np.array([entries[i % len(entries)] for i in range(picked.size)], np.float32)
            plane = torch.from_numpy(p.reshape(-1)).cuda()
        den.process_frame(d["noisy"], d["normals"], d["positions"], d["albedo"], NAN_VP, GARBAGE_JITTER, f,
                          prev_pixel=plane)
    assert den.frame_status() == 0
    got = _state(den, STATE[:2])
    spp = np.frombuffer(got["spp"], np.uint8)
    acc = np.frombuffer(got["noisy_accumulated"], np.uint32).reshape(n, 3)
    cur = d["noisy"].float().cpu().numpy().view(np.uint32).reshape(n, 3)
    assert (spp[picked] == 1).all(), np.unique(spp[picked], return_counts=True)
    assert (acc[picked] == cur[picked]).all()
    others = np.ones(n, bool)
    others[picked] = False
    want_spp = np.frombuffer(ref[frames - 1]["spp"], np.uint8)
    want_acc = np.frombuffer(ref[frames - 1]["noisy_accumulated"], np.uint32).reshape(n, 3)
    assert (spp[others] == want_spp[others]).all()
    assert (acc[others] == want_acc[others]).all()
    assert (want_spp[picked] > 1).any(), "the overwritten pixels had history to lose"


# ------------------------------------------------------------------ test 5 --
def test_host_dump_and_replay(tmp_path, gpu):
    """bmfr_host --dump-prev-pixel writes each frame's plane as a FLOAT EXR;
    --prev-pixel reads them back and passes them from frame 1 on: identical
    outputs to the plain run."""
    W, H, F = 128, 80, 4
    exe = _build.build_host()
    io = C.CDLL(_build.IO_LIB)
    io.bmfr_exr_read_rgb.argtypes = [C.c_char_p, C.c_int, C.c_int, C.c_void_p]

    def run(*args):
        r = subprocess.run([exe, "--synthetic", "--width", str(W), "--height", str(H), "--frames", str(F), "--exr",
                            *args], cwd=tmp_path, capture_output=True, text=True, timeout=300)
        assert r.returncode == 0, r.stdout + r.stderr

    def read(path):
        out = np.empty((H, W, 3), np.float32)
        assert io.bmfr_exr_read_rgb(str(path).encode(), W, H, out.ctypes.data) == 0, path
        return out

    run("--output", str(tmp_path / "plain_"))
    run("--output", str(tmp_path / "dump_"), "--dump-prev-pixel", str(tmp_path / "pp_"))
    run("--output", str(tmp_path / "replay_"), "--prev-pixel", str(tmp_path / "pp_"))
    for f in range(F):
        want = read(tmp_path / f"plain_{f}.exr").tobytes()
        assert read(tmp_path / f"dump_{f}.exr").tobytes() == want, f
        assert read(tmp_path / f"replay_{f}.exr").tobytes() == want, f
    # the dumped plane is the library's: frame 0 maps every pixel to itself, B = 0
    pp = read(tmp_path / "pp_0.exr")
    ys, xs = np.mgrid[0:H, 0:W]
    assert (pp[..., 0] == xs).all() and (pp[..., 1] == ys).all() and (pp[..., 2] == 0).all()
