"""The geometry sweep (ref_configs.GEOMETRY_REF_CONFIGS) on the CPU oracle, no
GPU: before tests/test_gpu_geometry.py runs the kernels at the smallest and
the odd frame sizes the library accepts, show that the sweep reaches what it
says and that its comparisons can be plain byte comparisons.

  * Validity: an axis n is accepted when n >= 32 and workset(n) + 30 <= 2 n --
    32, and everything from 47 up; bmfr_config_sizes accepts every size of the
    sweep and rejects 33..46 on either axis.
  * Finiteness: every recorded buffer of every frame is finite on the oracle,
    and spp reaches the frame count.
  * Coverage, computed from the block-offset table and each configuration's
    frame count: the mirrored source pixel of the extreme work-items (32 x 32
    reaches pixel 31 from below, 47 x 47 pixel 0 from above, the height 79
    pixel 32 from above); the frames on which the last block column of 65 x 47
    and the last block row of 47 x 65 hold exactly one image column / row, and
    those on which they hold none; every (W mod 64, H mod 16, H mod 12) is one
    no earlier configuration list has.
  * The edge counts: at 32 x 32 and 47 x 47 the pixel that block (0, 0) of
    frame 0 reads through its deepest mirrored work-item alone decides that
    block's result (an implementation that clamped where it should mirror
    would never read it).  The work-items at -32 and at workset + 29 belong to
    block columns that own no pixel; the pixel they alone mirror onto decides
    those blocks' recorded `weights`.
  * Three configurations are pinned to the reference's strict build through
    golden vectors (tests/golden/geometry/*.npz, tests/golden/make_golden.py
    --geometry), read as tests/test_oracle_cpu.py reads its own.
"""
from __future__ import annotations

import json
import os

import numpy as np
import pytest

import bmfr_amd
import geometry_util as gu
import knob_util
import pyoracle
import scenes_np
from aux_np import OFFSETS
from geometry_util import NAMES
from ref_configs import (FULL_REF_CONFIGS, GEOMETRY_REF_CONFIGS, GEOMETRY_SCENE, GEOMETRY_SEED, REF_CONFIGS,
                         SHAPE_SIZE)
from seq_util import ALL_KEYS, EXACT_KEYS, POWR_KEYS, digest, sample_idx

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "geometry")
SIZES = sorted({(rc.width, rc.height) for rc in GEOMETRY_REF_CONFIGS.values()})
TABLE = {"g32x32_h13": (32, 32, 1, 13, 17), "g32x32_f13": (32, 32, 0, 13, 6), "g47x47_h13": (47, 47, 1, 13, 17),
         "g47x47_h16": (47, 47, 1, 16, 6), "g65x47_h13": (65, 47, 1, 13, 17), "g47x65_f16": (47, 65, 0, 16, 10),
         "g97x79_h13": (97, 79, 1, 13, 6), "g97x79_h7": (97, 79, 1, 7, 6), "g129x53_h13": (129, 53, 1, 13, 17),
         "g129x53_f13": (129, 53, 0, 13, 6), "g67x131_h16": (67, 131, 1, 16, 6), "g67x131_h12": (67, 131, 1, 12, 6)}


def test_the_sweep_is_the_table():
    assert NAMES == list(TABLE) and len(NAMES) == 12
    for name, (w, h, half, b, frames) in TABLE.items():
        rc = GEOMETRY_REF_CONFIGS[name]
        assert (rc.width, rc.height, rc.half_tmp, rc.buffer_count, rc.frames) == (w, h, half, b, frames), name
        assert rc.seed == GEOMETRY_SEED == 7 and GEOMETRY_SCENE == "rand"
        assert rc.knobs() == REF_CONFIGS["s128x80_h13"].knobs()  # the reference's defaults
    lists = {n: (GEOMETRY_REF_CONFIGS[n].not_scaled, GEOMETRY_REF_CONFIGS[n].scaled) for n in NAMES}
    assert lists["g97x79_h7"] == ((0,), (4, 5, 6))
    assert lists["g67x131_h12"] == ((0, 3), (10, 11, 12, 7, 8, 9, 4))
    assert gu.GENERIC == ["g97x79_h7", "g67x131_h12"]
    assert gu.CANONICAL_HALF == ["g32x32_h13", "g47x47_h13", "g47x47_h16", "g65x47_h13", "g97x79_h13",
                                 "g129x53_h13", "g67x131_h16"]
    for n in gu.CANONICAL:
        assert lists[n] == ((0, 1, 2, 3), tuple(range(4, 10 if n.endswith("13") else 13))), n


# ------------------------------------------------------------------ validity ----
def test_valid_axes_are_32_and_47_up():
    assert [n for n in range(1, 200) if gu.valid_axis(n)] == [32] + list(range(47, 200))


@pytest.mark.parametrize("W,H", SIZES + [(32, 47), (47, 32), (63, 63), (79, 32)])
def test_config_accepts(W, H):
    assert gu.valid_axis(W) and gu.valid_axis(H)
    s = bmfr_amd.BmfrConfig(image_width=W, image_height=H).sizes()
    assert (s.workset_width, s.workset_height) == (gu.workset(W), gu.workset(H))
    assert s.blocks == gu.blocks(W) * gu.blocks(H)
    assert (s.region_x, s.region_y, s.region_width, s.region_height) == (0, 0, W, H)


@pytest.mark.parametrize("other", [32, 47, 131])
@pytest.mark.parametrize("n", range(33, 47))
def test_config_rejects_33_to_46_on_either_axis(n, other):
    assert not gu.valid_axis(n) and gu.valid_axis(other)
    for W, H in ((n, other), (other, n)):
        with pytest.raises(bmfr_amd.BmfrError) as e:
            bmfr_amd.BmfrConfig(image_width=W, image_height=H).sizes()
        assert e.value.status == 1, (W, H)


# ---------------------------------------------------------------- finiteness ----
def _floats(a):
    if a.dtype == np.uint16:  # half tmp_data travels as its bits
        return a.view(np.float16)
    return a if a.dtype.kind == "f" else None


@pytest.mark.parametrize("name", NAMES)
def test_every_record_is_finite(name):
    rc = GEOMETRY_REF_CONFIGS[name]
    recs = gu.oracle_frames(name)
    assert len(recs) == rc.frames
    for f, rec in enumerate(recs):
        assert set(rec) == set(ALL_KEYS), sorted(rec)
        for k, v in rec.items():
            x = _floats(v)
            assert x is None or np.isfinite(x).all(), (name, f, k, int((~np.isfinite(x)).sum()))
    assert int(recs[-1]["spp"].max()) == rc.frames
    # the content goes through the tap acceptance: no size is all-accept or all-reject
    masks = set()
    for rec in recs[1:]:
        masks |= set(np.unique(rec["accept"]).tolist())
    assert len(masks) >= 15, (name, sorted(masks))


# ------------------------------------------------------------------ coverage ----
def test_offset_table_extremes():
    """Work-items reach pixel -32 and workset + 29; the offsets are even, so
    the deepest margin a block that owns a pixel has starts at -30."""
    assert len(OFFSETS) == 16
    for axis in (0, 1):
        offs = [o[axis] for o in OFFSETS]
        assert min(offs) == -16 and max(offs) == 14 and all(o % 2 == 0 for o in offs)
        assert gu.item_range(32, min(offs))[0] == -32 and gu.item_range(47, max(offs))[1] == 64 + 29
    assert (OFFSETS[9][1], OFFSETS[13][0]) == (-16, -16)   # the two -16s: frames 9 and 13
    assert max(o[1] for o in OFFSETS[:6]) == 14 and min(o[1] for o in OFFSETS[:6]) == -14  # six frames: y = +-14


@pytest.mark.parametrize("name", NAMES)
def test_extreme_work_items_mirror_into_the_image(name):
    rc = GEOMETRY_REF_CONFIGS[name]
    for axis, n in enumerate((rc.width, rc.height)):
        below, above = gu.deepest_sources(name, axis)
        print(f"{name} axis {axis} (n = {n}): lowest work-item reads pixel {below}, highest pixel {above}")
        assert 0 <= below < n and 0 <= above < n
        if rc.frames == 17:  # all 16 offsets
            assert below == 31 and above == 2 * n - (gu.workset(n) + 29) - 1


def test_the_sizes_reach_what_they_are_there_for():
    for axis in (0, 1):
        assert gu.deepest_sources("g32x32_h13", axis)[0] == 31      # -32 -> 31, the far edge
        assert gu.deepest_sources("g47x47_h13", axis)[1] == 0       # 93 -> 0
    assert gu.deepest_sources("g47x47_h16", 1)[1] == 0              # six frames reach y = +14
    for name in ("g97x79_h13", "g97x79_h7"):
        assert gu.deepest_sources(name, 1)[1] == 32                 # 96 + 29 -> 32
    assert gu.valid_axis(47) and not gu.valid_axis(46)              # 47: the smallest valid size of its band


@pytest.mark.parametrize("name,axis", [("g65x47_h13", 0), ("g47x65_f16", 1)])
def test_last_block_holds_one_pixel_or_none(name, axis):
    """W = 65: the workset is 96, the fourth block column holds image column
    64 alone under the offset -16 and no column under any other."""
    rc = GEOMETRY_REF_CONFIGS[name]
    n = (rc.width, rc.height)[axis]
    assert n == 65 and gu.blocks(n) == 4
    held = [gu.block_pixels(n, off, gu.blocks(n) - 1) for off in gu.axis_offsets(name, axis)]
    one = [f for f, px in enumerate(held) if len(px) == 1]
    none = [f for f, px in enumerate(held) if not px]
    assert one and none and len(one) + len(none) == rc.frames, held
    assert all(held[f] == [64] for f in one)
    assert one == [f for f in range(rc.frames) if OFFSETS[f % 16][axis] == -16]
    # and on those frames the first block of the axis lies outside the image altogether
    assert all(not gu.block_pixels(n, OFFSETS[f % 16][axis], 0) for f in one)


def _triple(w, h):
    return w % 64, h % 16, h % 12


def test_tile_remainders_are_new():
    before = {_triple(rc.width, rc.height) for d in (REF_CONFIGS, FULL_REF_CONFIGS) for rc in d.values()}
    before.add(_triple(*SHAPE_SIZE))
    assert all(t[0] % 4 == 0 and t[1] % 8 == 0 for t in before)  # what the suite ran so far
    for name, rc in GEOMETRY_REF_CONFIGS.items():
        assert _triple(rc.width, rc.height) not in before, name
    got = {_triple(rc.width, rc.height) for rc in GEOMETRY_REF_CONFIGS.values()}
    # a 1-pixel overhang past one and past two 64-wide TAA tiles, and past both tile heights
    assert {t[0] for t in got} >= {1, 3, 32, 33, 47}
    assert (47, 1, 5) in got and _triple(129, 53) == (1, 5, 5) and _triple(67, 131) == (3, 3, 11)


# ----------------------------------------------------------- the edge counts ----
@pytest.mark.parametrize("which", ["corner", "x", "y"])
@pytest.mark.parametrize("name", ["g32x32_h13", "g47x47_h13"])
def test_the_deepest_mirrored_pixel_counts(name, which):
    """Frame 0 shifts the grid by (-14, -14): block (0, 0) holds the image
    pixels [0, 2) x [0, 2) and work-items down to -30, which mirror onto pixel
    29.  Within that block pixel 29 of an axis is read by the work-item at -30
    alone.  Changing `noisy` and `positions` there changes the block's result
    (frame 0's TAA passes the tone-mapped pixel through)."""
    rc = GEOMETRY_REF_CONFIGS[name]
    W, H = rc.width, rc.height
    ox, oy = OFFSETS[0]
    lo = [gu.item_range(n, off)[0] for n, off in ((W, ox), (H, oy))]
    own = [gu.block_pixels(n, off, 0) for n, off in ((W, ox), (H, oy))]
    assert lo == [-30, -30] and own == [[0, 1], [0, 1]]
    deep = [gu.mirror(p, n) for p, n in zip(lo, (W, H))]
    assert deep == [29, 29]
    for axis, n in enumerate((W, H)):  # no other work-item of block 0 reads pixel 29 of the axis
        readers = [p for p in range(lo[axis], lo[axis] + 32) if gu.mirror(p, n) == deep[axis]]
        assert readers == [lo[axis]]
    px, py = {"corner": (deep[0], deep[1]), "x": (deep[0], 1), "y": (1, deep[1])}[which]

    def run(edit):
        fr = gu.frame(name, 0)
        planes = {k: np.array(fr[k]).reshape(H, W, 3) for k in ("noisy", "normals", "positions", "albedo")}
        edit(planes)
        loop = pyoracle.OracleLoop(gu.make_cfg(name))
        loop.upload(*(planes[k].reshape(-1) for k in ("noisy", "normals", "positions", "albedo")))
        rec = {}
        loop.run_stages(fr["prev_vp"], fr["jitter"], 0, record=rec)
        return rec["result"].reshape(H, W, 3), rec["weights"].reshape(gu.blocks(H), gu.blocks(W), -1)

    def perturb(planes):
        planes["noisy"][py, px] += np.float32(2.0)
        planes["positions"][py, px] += np.float32(0.25)

    base, w0 = run(lambda planes: None)
    assert base.tobytes() == gu.oracle_frames(name)[0]["result"].tobytes()
    got, w1 = run(perturb)
    assert (w0[0, 0] != w1[0, 0]).any()
    changed = got.view(np.uint32) != base.view(np.uint32)
    assert changed[:2, :2].any(), (name, which, "block (0, 0) never read the mirrored pixel")


@pytest.mark.parametrize("name,side", [("g32x32_h13", "below"), ("g47x47_h13", "above")])
def test_the_extreme_work_item_counts_in_the_recorded_weights(name, side):
    """The work-items at -32 and at workset + 29 belong to a block column that
    lies outside the frame altogether (offset -16: [-32, 0); offset +14 at
    W = 47: [62, 94)), which owns no pixel but whose fit the stage kernels
    still run and record: the pixel it alone mirrors onto -- 31, the far
    edge, or 0 -- changes that block's `weights`, which tests/test_gpu_geometry.py
    compares in full, and no other block's."""
    rc = GEOMETRY_REF_CONFIGS[name]
    W, H = rc.width, rc.height
    off, b = (-16, 0) if side == "below" else (14, gu.blocks(W) - 1)
    F = next(f for f in range(rc.frames) if OFFSETS[f % 16][0] == off)
    assert not gu.block_pixels(W, off, b)                      # the block column owns nothing
    item = gu.item_range(W, off)[0 if side == "below" else 1]
    assert item == (-32 if side == "below" else gu.workset(W) + 29)
    src = gu.mirror(item, W)
    assert src == (31 if side == "below" else 0)
    p0 = gu.E * b - gu.E // 2 + off
    assert [p for p in range(p0, p0 + gu.E) if gu.mirror(p, W) == src] == [item]   # its only reader there
    oy = OFFSETS[F % 16][1]
    y = H // 2

    def source(f):
        fr = gu.frame(name, f)
        if f == F:
            for k, d in (("noisy", 2.0), ("positions", 0.25)):
                a = np.array(fr[k]).reshape(H, W, 3)
                a[y, src] += np.float32(d)
                fr[k] = a.reshape(-1)
        return fr

    got = scenes_np.run_loop(pyoracle.OracleLoop(gu.make_cfg(name)), GEOMETRY_SCENE, W, H, F + 1, rc.seed,
                             source=source)[F]["weights"].reshape(gu.blocks(H), gu.blocks(W), -1)
    base = gu.oracle_frames(name)[F]["weights"].reshape(gu.blocks(H), gu.blocks(W), -1)
    changed = (got.view(np.uint32) != base.view(np.uint32)).any(axis=2)

    def readers(n, o, pixel):  # the blocks of an axis one of whose work-items reads the pixel
        return [c for c in range(gu.blocks(n))
                if any(gu.mirror(p, n) == pixel for p in range(gu.E * c - gu.E // 2 + o, gu.E * c + gu.E // 2 + o))]

    cols, rows = readers(W, off, src), readers(H, oy, y)
    assert b in cols and len(cols) == 2 and rows          # the block outside the frame and its neighbour
    assert all(changed[r, b] for r in rows), (name, F, "the block outside the frame never read the mirrored pixel")
    want = np.zeros_like(changed)
    want[np.ix_(rows, cols)] = True
    assert (changed == want).all(), changed


# --------------------------------------------------------------- golden vectors ----
@pytest.mark.parametrize("name", list(gu.GOLDEN_FRAMES))
def test_oracle_matches_reference_golden_vectors(name):
    """As tests/test_oracle_cpu.py: digests on EXACT_KEYS, weights and
    mins_maxs in full, tone / result by sums and samples within its tolerance."""
    rc = GEOMETRY_REF_CONFIGS[name]
    z = np.load(os.path.join(GOLDEN, f"{name}.npz"), allow_pickle=False)
    meta = json.loads(bytes(z["meta"]).decode())
    frames = meta["frames"]
    assert frames == gu.GOLDEN_FRAMES[name] <= rc.frames and meta["mode"] == "strict" and meta["config"] == name
    assert (meta["scene"], meta["seed"]) == (GEOMETRY_SCENE, GEOMETRY_SEED)
    for f in range(frames):
        assert knob_util.frame_digest(scenes_np.frame(GEOMETRY_SCENE, rc.width, rc.height, f, rc.seed)) == \
            meta["inputs"][f], f"inputs of frame {f} changed: regenerate tests/golden/geometry (make_golden.py --geometry)"
    got = gu.oracle_frames(name)[:frames]
    for f, g in enumerate(got):
        np.testing.assert_array_equal(g["weights"], z[f"weights_{f}"], err_msg=f"frame {f} weights")
        np.testing.assert_array_equal(g["mins_maxs"], z[f"mins_maxs_{f}"], err_msg=f"frame {f} mins_maxs")
        bad = [k for k in EXACT_KEYS if digest(g[k]) != meta["digests"][f][k]]
        assert not bad, f"frame {f}: oracle differs from the reference in {bad}"
        for k in POWR_KEYS:
            ref = z[f"{k}_sample_{f}"].astype(np.float64)
            mine = g[k][sample_idx(g[k].size)].astype(np.float64)
            assert np.abs(mine - ref).max() <= 4e-7, (f, k, np.abs(mine - ref).max())
            st = meta["stats"][f][k]
            a = g[k].astype(np.float64)
            assert abs(a.sum() - st["sum"]) <= 1e-6 * a.size, (f, k)
