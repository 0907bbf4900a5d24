"""What the GPU parity suites share (run on an MI355X: pytest -m gpu): the
device-side helpers, the one driver of the Denoiser's frame entry points, and
the pipeline runs of a suite, each made once.  The numpy side -- the constants
and the comparators every parity claim rests on -- is tests/seq_util.py
(tests/test_seq_util_cpu.py).  TEST INFRASTRUCTURE ONLY."""
from __future__ import annotations

import numpy as np
import pytest
import torch

import aux_np
import bmfr_amd
import pyoracle
import ref_run
import scenes_np
import shape_util
from seq_util import FUSED_KEYS, GARBAGE_JITTER, NAN_VP, PLANES, through_half, to_np

# (bmfr_state plane, channels, dtype): the output and the four state planes under the library's names
STATE = (("noisy_accumulated", 3, torch.float32), ("spp", 1, torch.uint8), ("filtered_accumulated", 3, torch.float32),
         ("result", 3, torch.float32), ("prev_frame_pixel", 2, torch.float32))


def to_device(a):
    return torch.from_numpy(np.array(a, order="C")).cuda()  # a copy: the generator's planes are read-only


def bmfr_cfg(rc, lists=None, **kw) -> bmfr_amd.BmfrConfig:
    """The library's configuration of a RefConfig.  lists: (not_scaled,
    scaled) in place of the configuration's; kw: further BmfrConfig keywords."""
    not_scaled, scaled = lists or (rc.not_scaled, rc.scaled)
    return bmfr_amd.BmfrConfig(image_width=rc.width, image_height=rc.height, not_scaled=tuple(not_scaled),
                               scaled=tuple(scaled), use_half_precision_in_tmp_data=rc.half_tmp, **rc.knobs(), **kw)


# ------------------------------------------------------------ torch tensors ----
def bits(t: torch.Tensor) -> torch.Tensor:
    """Raw bits of a float tensor (NaN-safe bitwise comparison)."""
    t = t.reshape(-1)
    if t.dtype == torch.float32:
        return t.view(torch.int32)
    if t.dtype == torch.float16:
        return t.view(torch.int16)
    return t


def same_bits(a: torch.Tensor, b: torch.Tensor) -> bool:
    return a.shape == b.shape and torch.equal(bits(a), bits(b))


def assert_same(a: torch.Tensor, b: torch.Tensor, what: str) -> None:
    a, b = bits(a), bits(b)
    assert a.shape == b.shape, (what, a.shape, b.shape)
    if not torch.equal(a, b):
        bad = torch.nonzero(a != b).reshape(-1)
        raise AssertionError(f"{what}: {bad.numel()} of {a.numel()} differ, first at {bad[:5].tolist()}")


def rel_l2(a: torch.Tensor, b: torch.Tensor) -> float:
    a, b = a.double().reshape(-1), b.double().reshape(-1)
    return float(torch.linalg.norm(a - b) / torch.linalg.norm(b))


def assert_same_array(got: np.ndarray, want: np.ndarray, what, nan_aware: bool = False):
    """Byte for byte; nan_aware (inputs that hold NaN only): NaN where the
    restatement has NaN, whatever its payload, and bytes elsewhere."""
    assert got.dtype == want.dtype and got.shape == want.shape, (what, got.dtype, want.dtype, got.shape, want.shape)
    if nan_aware:
        nan = np.isnan(want)
        assert (np.isnan(got) == nan).all(), (what, "NaN positions differ")
        got, want = np.where(nan, 0, got).astype(got.dtype), np.where(nan, 0, want).astype(want.dtype)
    a, b = got.view(np.uint8), want.view(np.uint8)
    bad = np.flatnonzero(a != b)
    assert bad.size == 0, (what, f"{bad.size} of {a.size} bytes differ, first at byte {int(bad[0])}: "
                                 f"{got.reshape(-1)[bad[0] // got.itemsize]!r} != {want.reshape(-1)[bad[0] // got.itemsize]!r}")


# ------------------------------------------------------ a Denoiser's last frame ----
def fused_state(den, n, keys=FUSED_KEYS, host=True) -> dict:
    """The last frame's output and state planes by record key: numpy arrays,
    or (host=False) the tensors, still on the device and not waited for."""
    out = {}
    for k, plane in keys.items():
        t = torch.empty(n, dtype=torch.uint8, device="cuda") if k == "spp" else \
            torch.empty((2 if k == "prev_pixel" else 3) * n, device="cuda")
        out[k] = den.copy_output(t) if k == "result" else den.copy_state(plane, t)
    if not host:
        return out
    torch.cuda.synchronize()
    return {k: to_np(v).copy() for k, v in out.items()}


def state_snapshot(den, names=STATE) -> dict:
    """The named planes of the last frame by bmfr_state name, over the
    context's region (a tile's, where it is one), as numpy arrays."""
    n = den.sizes.region_width * den.sizes.region_height
    return {name: den.copy_state(name, torch.empty(n * ch, dtype=dt, device="cuda")).cpu().numpy()
            for name, ch, dt in names}


# ------------------------------------------------------------ the frame driver ----
def device_frames(frame, count, W, H, half_in=False, aux_names=()):
    """Per frame: (planes on the device -- "aux": the planes of aux_names,
    aux_np.PLANES keys --, previous camera, jitter).  frame: f -> frame dict."""
    out = []
    for f in range(count):
        fr = frame(f)
        d = {k: to_device(fr[k].astype(np.float16) if half_in else fr[k]) for k in PLANES}
        d["aux"] = [None if p is None else to_device(p)
                    for p in aux_np.aux_planes(aux_names, fr["normals"], fr["positions"], fr["albedo"], W, H)]
        out.append((d, fr["prev_vp"], fr["jitter"]))
    return out


def fused_frames(rc, frames, lists=None, launches=0, profiled=False, half_in=False, widen=False, mode="frame",
                 replay=None, **kw):
    """The Denoiser of bmfr_cfg(rc, lists, **kw) over `frames` (device_frames)
    -> per-frame output and state.  launches: debug_frame_launches; profiled:
    per-kernel events (K1 and K2 as two launches); half_in: the planes are
    half (widen: the same values as f32, into an f32 context); mode: "frame",
    "split" (_interior + _border) or "sequence" (one process_sequence call ->
    (per-frame outputs, last state)); replay: the per-frame records of another
    run, whose prev_frame_pixel plane each frame from 1 on is fed under a NaN
    camera.  frame_status is asserted OK after every frame and after the
    sequence call, so an exhausted in-kernel wait reads as
    BMFR_ERROR_SYNC_TIMEOUT and not as a wrong pixel."""
    n = rc.width * rc.height
    den = bmfr_amd.Denoiser(bmfr_cfg(rc, lists, input_half=int(half_in and not widen), **kw))
    if launches:
        den.debug_frame_launches(launches)
    if profiled:
        den.set_profiling(True, capacity=len(frames), stride=1)
    if widen:
        frames = [({k: (v.float() if k in PLANES else v) for k, v in d.items()}, vp, jit) for d, vp, jit in frames]
    if mode == "sequence":
        outs = [torch.empty(3 * n, device="cuda") for _ in frames]
        den.process_sequence([d for d, _, _ in frames], [(vp, jit) for _, vp, jit in frames], 0, outputs=outs)
        torch.cuda.synchronize()
        assert den.frame_status() == 0, (rc.name, den.frame_status())
        return [{"result": to_np(o).copy()} for o in outs], fused_state(den, n)
    out = []
    for f, (d, vp, jit) in enumerate(frames):
        plane = None
        if replay is not None:
            vp, jit = NAN_VP, GARBAGE_JITTER
            # frame 0 ignores the plane
            plane = torch.full((2 * n,), float("nan"), device="cuda") if f == 0 else to_device(replay[f]["prev_pixel"])
        args = (d["noisy"], d["normals"], d["positions"], d["albedo"], vp, jit, f)
        if mode == "split":
            den.process_frame_interior(*args, aux=d["aux"], prev_pixel=plane)
            den.process_frame_border(*args, aux=d["aux"], prev_pixel=plane)
        else:
            den.process_frame(*args, aux=d["aux"], prev_pixel=plane)
        out.append(fused_state(den, n))
        assert den.frame_status() == 0, (rc.name, f, den.frame_status())
    return out


# --------------------------------------------------- one suite's pipeline runs ----
class Suite:
    """The pipeline runs of one parity suite over its content, each made once
    and kept in the suite's own cache (clear() drops them).  A case is named
    by a key the suite chooses -- a configuration name, a (scene, name) pair.
    frame: (key, f) -> frame dict (scenes_np.frame's form); config: key ->
    RefConfig; frames: the frame count (None: the configuration's);
    missing_ref: what a missing reference build does, pytest.skip or
    pytest.fail."""

    def __init__(self, frame, config, frames=None, missing_ref=pytest.skip):
        self.frame, self.config, self.frames, self.missing_ref = frame, config, frames, missing_ref
        self.cache = {}

    def cached(self, key, make):
        if key not in self.cache:
            self.cache[key] = make()
        return self.cache[key]

    def clear(self) -> None:
        self.cache.clear()

    def need_ref(self, key, mode="strict") -> None:
        name = self.config(key).name
        if not ref_run.available(name, mode):
            self.missing_ref(f"reference build {name}_{mode} missing (oracle/build_ref.py)")

    def count(self, key) -> int:
        return self.frames or self.config(key).frames

    def run_loop(self, loop, key, **kw):
        """scenes_np.run_loop over the case's frames."""
        rc = self.config(key)
        return scenes_np.run_loop(loop, None, rc.width, rc.height, self.count(key),
                                  source=lambda f: self.frame(key, f), **kw)

    def ref_frames(self, key, mode="strict", half_in=False):
        """The reference kernels' records; half_in: on the planes rounded to half and widened."""
        self.need_ref(key, mode)
        return self.cached((key, "ref", mode, half_in), lambda: self.run_loop(
            ref_run.RefLoop(self.config(key), mode), key, to_device=to_device, sync=torch.cuda.synchronize,
            prepare=through_half if half_in else None))

    def oracle_frames(self, key):
        rc = self.config(key)
        cfg = pyoracle.make_cfg(rc.width, rc.height, rc.not_scaled, rc.scaled, rc.half_tmp, **rc.knobs())
        return self.cached((key, "oracle"), lambda: self.run_loop(pyoracle.OracleLoop(cfg), key))

    def stage_frames(self, key, library_powr=0):
        return self.cached((key, "stages", library_powr), lambda: self.run_loop(
            bmfr_amd.StagePipeline(bmfr_cfg(self.config(key), library_powr=library_powr)), key, to_device=to_device,
            sync=torch.cuda.synchronize))

    def device_frames(self, key, half_in=False, aux_names=()):
        rc = self.config(key)
        return self.cached((key, "device", half_in, tuple(aux_names)), lambda: device_frames(
            lambda f: self.frame(key, f), self.count(key), rc.width, rc.height, half_in, aux_names))

    def fused_frames(self, key, aux=False, half_in=False, **options):
        """fused_frames over the case's frames; the run is not kept.  aux: the
        list of shape_util.aux_case_of, with its planes."""
        rc = self.config(key)
        not_scaled, scaled, aux_names = shape_util.aux_case_of(rc) if aux else (rc.not_scaled, rc.scaled, ())
        return fused_frames(rc, self.device_frames(key, half_in, aux_names), (not_scaled, scaled), half_in=half_in,
                            **options)

    def kept_fused_frames(self, key, **options):
        """fused_frames, kept.  An option at its default and the option left
        out are one entry (every default is falsy)."""
        given = tuple(sorted((k, v) for k, v in options.items() if v))
        return self.cached((key, "fused") + given, lambda: self.fused_frames(key, **options))


# ------------------------------------- tiled half inputs (content and knob suites) ----
def check_tiled_half_inputs(gx, gy, scene, split=False, frames=6, seed=2, **cfg_kw):
    """The tiled case: every frame of every tile == the untiled frame bit for
    bit, the halo report clean.  split: each frame as process_frame_interior,
    halo exchange, process_frame_border instead of exchange, process_frame.
    frames, seed: the content suite's (tests/test_scenes_np.py asserts the
    coverage for this seed).  cfg_kw: BmfrConfig keywords of every context,
    the untiled one included."""
    from bmfr_amd.tiling import HipCopier, LoopbackTransport, TileGrid, state_planes
    W, H, halo = 320, 256, 40
    n = W * H
    # a halo of 40 covers 6 px of motion (include/bmfr.h: tile_halo - 34): the pan at a fifth of
    # its speed, 3.3 px/frame on the wall and up to 5.5 on the quad (1.7 x the parallax); rand
    # moves up to 5.9 px at this size
    speed = 0.2 if scene == "pan" else 1.0
    grid = TileGrid(W, H, gx, gy, halo=halo)
    kw = dict(image_width=W, image_height=H, input_half=1, **cfg_kw)
    full = bmfr_amd.Denoiser(bmfr_amd.BmfrConfig(**kw))
    tiles = [bmfr_amd.Denoiser(bmfr_amd.BmfrConfig(tile=grid.tile(r), tile_halo=halo, **kw))
             for r in range(grid.ranks)]
    loop, copier = LoopbackTransport(grid), HipCopier()
    prev = [None] * grid.ranks
    crossed = [False] * grid.ranks
    for f in range(frames):
        fr = scenes_np.frame(scene, W, H, f, seed, speed=speed)
        vp, jit = fr["prev_vp"], fr["jitter"]
        p = {k: to_device(fr[k].astype(np.float16)) for k in PLANES}
        full.process_frame(p["noisy"], p["normals"], p["positions"], p["albedo"], vp, jit, f)
        inps = []
        for d in tiles:
            cut = scenes_np.frame(scene, W, H, f, seed, region=d.region, speed=speed)
            inps.append({k: to_device(cut[k].astype(np.float16)) for k in PLANES})
        for call in ("process_frame_interior", "process_frame_border") if split else ("process_frame",):
            if f > 0 and call != "process_frame_interior":
                loop.exchange_all([state_planes(d) for d in tiles], copier)
            for r, d in enumerate(tiles):
                i = inps[r]
                getattr(d, call)(i["noisy"], i["normals"], i["positions"], i["albedo"], vp, jit, f,
                                 prev_normals=prev[r]["normals"] if prev[r] else None,
                                 prev_positions=prev[r]["positions"] if prev[r] else None)
        prev = inps
        torch.cuda.synchronize()
        want = {"result": full.copy_output(torch.empty(3 * n, device="cuda")).view(H, W, 3),
                "filtered_accumulated": full.copy_state("filtered_accumulated",
                                                        torch.empty(3 * n, device="cuda")).view(H, W, 3),
                "noisy_accumulated": full.copy_state("noisy_accumulated",
                                                     torch.empty(3 * n, device="cuda")).view(H, W, 3)}
        pp = full.copy_state("prev_frame_pixel", torch.empty(2 * n, device="cuda")).view(H, W, 2).cpu().numpy()
        assert np.isfinite(to_np(want["result"])).all()
        for r, d in enumerate(tiles):
            assert d.halo_status() == 0, (f, r)
            rx, ry, rw, rh = d.region
            x, y, w, h = grid.tile(r)
            for k, v in want.items():
                t = torch.empty(3 * rw * rh, device="cuda")
                got = (d.copy_output(t) if k == "result" else d.copy_state(k, t)).view(rh, rw, 3)
                a = got[y - ry:y - ry + h, x - rx:x - rx + w].contiguous().view(torch.int32)
                b = v[y:y + h, x:x + w].contiguous().view(torch.int32)
                assert torch.equal(a, b), (f, r, k, int((a != b).sum()))
            if f > 0:  # pixels of this tile whose reprojection lands in the image, in the other tile
                q = pp[y:y + h, x:x + w]
                inside = (q[..., 0] >= 0) & (q[..., 0] < W) & (q[..., 1] >= 0) & (q[..., 1] < H)
                own = (q[..., 0] >= x) & (q[..., 0] < x + w) & (q[..., 1] >= y) & (q[..., 1] < y + h)
                crossed[r] = crossed[r] or bool((inside & ~own).any())
    if scene == "pan":
        assert all(crossed), crossed
