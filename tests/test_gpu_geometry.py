"""The kernels at the frame sizes nothing else runs (run on an MI355X: pytest
-m gpu): 32 x 32, 47 x 47 and odd widths and heights up to 131
(ref_configs.GEOMETRY_REF_CONFIGS; tests/test_geometry_cpu.py computes what
each size reaches -- mirrored margins at full depth, a block column / row that
holds one pixel or none, 1- and 3-pixel overhangs of the TAA tiles, odd row
strides in the 6-byte and 1-byte planes -- and shows every record finite, so
bytes are compared, never NaN-aware).  Content: scene "rand", seed 7.

Over every configuration: the stage kernels == the reference's strict build
(library_powr = 1) and == the CPU oracle (default powr) on every inter-stage
buffer; Denoiser.process_frame == the stages on the output and the four state
planes; the frame as one launch, as two launches and profiled == each other
and the stages; one process_sequence call, in both schedules, == the frames.
Over the canonical lists with half tmp_data: half input planes == the same
values widened (== the reference on them); the K1 that reads a prev_pixel
plane, under a NaN camera, reproduces the context the plane came from.  Over
the two generic lists: features replaced by caller-supplied planes == the
named list; _interior + _border == the frame.  Tiled, tile_halo 34 (still
camera) and 40, with tile edges at x = 65 and y = 67: every tile == the
untiled frame.  Every run ends with frame_status OK, so an exhausted
in-kernel wait reads as BMFR_ERROR_SYNC_TIMEOUT and not as a wrong pixel.

fast_fit (not bit-exact) on the canonical configurations: the per-frame
relative L2 of `result` against the reference's strict build <= 1e-4, the
project's bar (tests/test_gpu_fast_fit.py); that figure and the distance
between the reference's own two builds on the same frames go to the parity
log as geometry_<name> (profiles/geometry_parity.json).
"""
from __future__ import annotations

import dataclasses

import numpy as np
import pytest
import torch

import aux_np
import bmfr_amd
import geometry_util as gu
import scenes_np
import shape_util
from bmfr_amd.tiling import HipCopier, LoopbackTransport, TileGrid, state_planes
from geometry_util import CANONICAL, CANONICAL_HALF, GENERIC, NAMES
from parity_harness import Suite, bmfr_cfg, fused_state, to_device
from ref_configs import GEOMETRY_REF_CONFIGS, GEOMETRY_SCENE
from seq_util import ALL_KEYS, FUSED_KEYS, PLANES, TILE_FACTOR, TOL, compare_exact, rel_l2_finite, to_np

pytestmark = pytest.mark.gpu

KEYS = tuple(FUSED_KEYS)
# a case is a configuration name; a missing reference build skips.  fused_frames: parity_harness.fused_frames
# over the configuration's frames (aux: the list of shape_util.aux_case_of with its planes); kept_frames: run once
SUITE = Suite(gu.frame, GEOMETRY_REF_CONFIGS.get, missing_ref=pytest.skip)
ref_frames, stage_frames = SUITE.ref_frames, SUITE.stage_frames
fused_frames, kept_frames = SUITE.fused_frames, SUITE.kept_fused_frames


def plain_frames(name, library_powr=0):
    return kept_frames(name, library_powr=library_powr)


# ------------------------------------------------------- every configuration ----
@pytest.mark.parametrize("name", NAMES)
def test_stage_kernels_match_reference_bitwise(name, gpu):
    """library_powr: the reference kernel's own powr, so every buffer is
    pinned, tmp_data as the fit leaves it included."""
    compare_exact(stage_frames(name, 1), ref_frames(name), ALL_KEYS, f"HIP stages vs reference[{name}]")


@pytest.mark.parametrize("name", NAMES)
def test_stage_kernels_match_oracle_bitwise(name, gpu):
    compare_exact(stage_frames(name, 0), gu.oracle_frames(name), ALL_KEYS, f"HIP stages vs oracle[{name}]")


@pytest.mark.parametrize("library_powr", [0, 1])
@pytest.mark.parametrize("name", NAMES)
def test_fused_frame_matches_stages_bitwise(name, library_powr, gpu):
    compare_exact(plain_frames(name, library_powr), stage_frames(name, library_powr), KEYS,
                  f"process_frame vs stages[{name} powr {library_powr}]")


@pytest.mark.parametrize("name", NAMES)
def test_one_launch_two_launches_and_profiled_agree(name, gpu):
    """The one-launch frame's TAA tiles wait on the completion flags of the K1
    blocks under them: at 32 x 32 one tile, mostly overhang, over a 2 x 2 block
    grid of which a row or a column is empty on some frames.  (Lists and
    precisions without a one-launch kernel run K1 and K2 apart either way.)"""
    st = stage_frames(name, 0)
    one, two = fused_frames(name, launches=1), fused_frames(name, launches=2)
    prof = fused_frames(name, profiled=True)
    compare_exact(one, two, KEYS, f"one launch vs two[{name}]")
    compare_exact(prof, two, KEYS, f"profiled vs two launches[{name}]")
    compare_exact(one, st, KEYS, f"one launch vs stages[{name}]")
    compare_exact(two, st, KEYS, f"two launches vs stages[{name}]")


@pytest.mark.parametrize("schedule", ["fused", "streams"])
@pytest.mark.parametrize("name", NAMES)
def test_sequence_equals_frames(name, schedule, gpu, monkeypatch):
    if schedule == "streams":
        monkeypatch.setenv("BMFR_SEQUENCE", "streams")
    else:
        monkeypatch.delenv("BMFR_SEQUENCE", raising=False)
    per_frame = plain_frames(name)
    outs, last = fused_frames(name, mode="sequence")
    compare_exact(outs, per_frame, ("result",), f"process_sequence outputs vs process_frame[{name}]")
    compare_exact([last], [per_frame[-1]], KEYS, f"process_sequence state vs process_frame[{name}]")


# -------------------------------------- canonical lists with half tmp_data ----
@pytest.mark.parametrize("name", CANONICAL_HALF)
def test_half_inputs_match_widened(name, gpu):
    """Half input planes: the 12-byte load of two half3 pixels at an odd pixel
    index, rows of odd stride in the 6-byte planes."""
    half = kept_frames(name, half_in=True, library_powr=1)
    wide = fused_frames(name, half_in=True, widen=True, library_powr=1)
    compare_exact(half, wide, KEYS, f"half vs widened[{name}]")
    # the half path really read half planes
    assert half[-1]["result"].tobytes() != plain_frames(name, 1)[-1]["result"].tobytes()


@pytest.mark.parametrize("name", CANONICAL_HALF)
def test_half_inputs_match_reference_on_widened(name, gpu):
    half = kept_frames(name, half_in=True, library_powr=1)
    compare_exact(half, ref_frames(name, "strict", half_in=True), KEYS, f"half vs reference on widened[{name}]")


@pytest.mark.parametrize("half_in", [False, True], ids=["f32_in", "half_in"])
@pytest.mark.parametrize("name", CANONICAL_HALF)
def test_plane_reading_k1_replays_projection(name, half_in, gpu):
    """A context fed the prev_frame_pixel plane another context computed, a
    NaN camera matrix and a garbage pixel offset reproduces it."""
    want = kept_frames(name, half_in=half_in)
    got = fused_frames(name, half_in=half_in, replay=want)
    compare_exact(got, want, KEYS, f"prev_pixel replay vs projection[{name}]")


# --------------------------------------------------------- the generic lists ----
@pytest.mark.parametrize("library_powr", [0, 1])
@pytest.mark.parametrize("name", GENERIC)
def test_aux_kernel_equals_named(name, library_powr, gpu):
    rc = GEOMETRY_REF_CONFIGS[name]
    not_scaled, scaled, aux_names = shape_util.aux_case_of(rc)
    codes = not_scaled + scaled
    assert len(codes) == len(rc.not_scaled + rc.scaled) and codes[-1] >= aux_np.AUX0
    for k, nm in enumerate(aux_names):  # plane k holds the code it replaced
        if nm is not None:
            assert (rc.not_scaled + rc.scaled)[codes.index(aux_np.AUX0 + k)] == aux_np.CODE_OF[nm]
    compare_exact(fused_frames(name, aux=True, library_powr=library_powr), plain_frames(name, library_powr), KEYS,
                  f"aux vs named[{name} powr {library_powr}]")


@pytest.mark.parametrize("aux", [False, True], ids=["named", "aux"])
@pytest.mark.parametrize("name", GENERIC)
def test_interior_border_equals_frame(name, aux, gpu):
    whole = fused_frames(name, aux=True) if aux else plain_frames(name)
    compare_exact(fused_frames(name, aux=aux, mode="split"), whole, KEYS,
                  f"_interior + _border vs process_frame[{name}]")


# ----------------------------------------------------------------------- tiled ----
@dataclasses.dataclass(frozen=True)
class ExplicitGrid(TileGrid):
    """A TileGrid whose tile rectangles are given, not an equal split."""
    rects: tuple = ()

    def tile(self, rank: int):
        return self.rects[rank]


# halo 34, the smallest: no motion allowance (include/bmfr.h: tile_halo - 34 pixels), so the scene under
# its still camera; halo 40 covers 6 px of motion, the scene as every other test here runs it (it moves
# up to 1.6 px per frame at these sizes)
HALOS = {"halo34_still": (34, True), "halo40_moving": (40, False)}
# tile edges at an odd pixel: x = 65 of 129 x 53, y = 67 of 67 x 131 (the canonical lists: a tiled
# context with any other list is BMFR_ERROR_UNSUPPORTED)
TILED = {"g129x53_h13": ((0, 0, 65, 53), (65, 0, 64, 53)), "g129x53_f13": ((0, 0, 65, 53), (65, 0, 64, 53)),
         "g67x131_h16": ((0, 0, 67, 67), (0, 67, 67, 64))}


@pytest.mark.parametrize("case", list(HALOS))
@pytest.mark.parametrize("half_in", [False, True], ids=["f32_in", "half_in"])
@pytest.mark.parametrize("name", list(TILED))
def test_tiled_matches_untiled(name, half_in, case, gpu):
    """Exact path.  Each tile reads the previous state it needs from the other
    through the loopback transport; output and state of every tile == the
    untiled frame's, the halo report clean.  Still: every previous-frame
    position stays within a pixel of its own pixel; moving: within the six
    pixels the halo covers.  Either way the blocks of a tile reach 32 pixels
    into the other and gather their history there."""
    HALO, still = HALOS[case]
    rc = GEOMETRY_REF_CONFIGS[name]
    W, H, rects = rc.width, rc.height, TILED[name]
    n = W * H
    grid = ExplicitGrid(W, H, 2 if rects[1][0] else 1, 2 if rects[1][1] else 1, halo=HALO, rects=rects)
    assert grid.ranks == len(rects) == 2 and sum(r[2] * r[3] for r in rects) == n
    kw = dict(input_half=int(half_in))
    full = bmfr_amd.Denoiser(bmfr_cfg(rc, **kw))
    tiles = [bmfr_amd.Denoiser(bmfr_cfg(rc, tile=grid.tile(r), tile_halo=HALO, **kw)) for r in range(grid.ranks)]
    for r, d in enumerate(tiles):
        assert d.region == grid.region(r)
    loop, copier = LoopbackTransport(grid), HipCopier()
    prev = [None] * grid.ranks
    cut = lambda a: a.astype(np.float16) if half_in else a  # noqa: E731
    planes = {"result": 3, "filtered_accumulated": 3, "noisy_accumulated": 3, "spp": 1}
    for f in range(rc.frames):
        fr = scenes_np.frame(GEOMETRY_SCENE, W, H, f, rc.seed, still=still)
        vp, jit = fr["prev_vp"], fr["jitter"]
        p = {k: to_device(cut(fr[k])) for k in PLANES}
        full.process_frame(p["noisy"], p["normals"], p["positions"], p["albedo"], vp, jit, f)
        inps = []
        for d in tiles:
            part = scenes_np.frame(GEOMETRY_SCENE, W, H, f, rc.seed, region=d.region, still=still)
            inps.append({k: to_device(cut(part[k])) for k in PLANES})
        if f > 0:
            loop.exchange_all([state_planes(d) for d in tiles], copier)
        for r, d in enumerate(tiles):
            i = inps[r]
            d.process_frame(i["noisy"], i["normals"], i["positions"], i["albedo"], vp, jit, f,
                            prev_normals=prev[r]["normals"] if prev[r] else None,
                            prev_positions=prev[r]["positions"] if prev[r] else None)
        prev = inps
        torch.cuda.synchronize()
        assert full.frame_status() == 0, f
        want = fused_state(full, n)
        assert np.isfinite(want["result"]).all()
        pp = want["prev_pixel"].reshape(H, W, 2)
        ys, xs = np.mgrid[0:H, 0:W]
        move = max(float(np.abs(pp[..., 0] - xs).max()), float(np.abs(pp[..., 1] - ys).max()))
        assert move < (1.0 if still else HALO - 34), (f, move)  # the premise: within what the halo covers
        for r, d in enumerate(tiles):
            assert d.halo_status() == 0 and d.frame_status() == 0, (f, r)
            rx, ry, rw, rh = d.region
            x, y, w, h = grid.tile(r)
            for k, ch in planes.items():
                t = torch.empty(ch * rw * rh, dtype=torch.uint8 if k == "spp" else torch.float32, device="cuda")
                got = to_np(d.copy_output(t) if k == "result" else d.copy_state(k, t)).reshape(rh, rw, ch)
                a = got[y - ry:y - ry + h, x - rx:x - rx + w]
                key = {"filtered_accumulated": "acc", "noisy_accumulated": "noisy"}.get(k, k)
                b = want[key].reshape(H, W, ch)[y:y + h, x:x + w]
                assert a.tobytes() == b.tobytes(), (name, f, r, k, int((a != b).sum()))
    assert int(want["spp"].max()) == rc.frames  # history was kept, so the exchanged state was read


# -------------------------------------------------------------------- fast_fit ----
@pytest.mark.parametrize("name", CANONICAL)
def test_fast_fit_within_tolerance(name, gpu, parity_log):
    rc = GEOMETRY_REF_CONFIGS[name]
    strict, default = ref_frames(name, "strict"), ref_frames(name, "default")
    fast = fused_frames(name, library_powr=1, fast_fit=1)
    where = f"fast_fit[{name}]"
    e_fast = [rel_l2_finite(g["result"], r["result"], where) for g, r in zip(fast, strict)]
    builds = [rel_l2_finite(d["result"], r["result"], where) for d, r in zip(default, strict)]
    parity_log(f"geometry_{name}", {
        "scene": GEOMETRY_SCENE, "seed": rc.seed, "config": name, "frames": rc.frames,
        "fast_fit_vs_strict_per_frame": [float(f"{e:.3e}") for e in e_fast],
        "default_vs_strict_per_frame": [float(f"{e:.3e}") for e in builds]})
    print(f"{where}: worst frame vs strict {max(e_fast):.3e} (frame {int(np.argmax(e_fast))}), the reference's "
          f"builds {max(builds):.3e}; per frame {['%.2e' % e for e in e_fast]} / {['%.2e' % e for e in builds]}")
    # the fit does not feed these
    compare_exact(fast, strict, ("noisy", "spp", "prev_pixel"), where)
    assert all(np.isfinite(g["result"]).all() and np.isfinite(g["acc"]).all() for g in fast)
    # a frame that misses is a known miss (a strict xfail with both figures, like KNOWN_TILE_MISS of
    # tests/test_gpu_content_parity.py) only within TILE_FACTOR times the builds' distance on that frame,
    # and a bug beyond; none does (worst measured 5.9e-5, g97x79_h13 frame 0, the builds 1.6e-5 apart there)
    missed = {f: (e, b, e <= TILE_FACTOR * b) for f, (e, b) in enumerate(zip(e_fast, builds)) if not e <= TOL}
    assert not missed, (where, f"frames beyond {TOL}: (fast_fit, the reference's builds, within {TILE_FACTOR} x)",
                        missed)
