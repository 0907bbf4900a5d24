"""The shape sweep (ref_configs.SHAPE_REF_CONFIGS) on the CPU oracle, no GPU:
before tests/test_gpu_shapes.py runs every generic-count kernel against the
reference, show that the sweep is what it says and that its comparisons can
be plain byte comparisons.

  * Coverage: one configuration per (NS, FS, tmp_data precision), NS 1..4,
    FS 0..9 -- the counts the library instantiates k_fitter / k_fused_block
    for --, plus the three odd lists at (3, 5) in each precision; within each
    precision every code 1..12 occurs in the not-scaled group and in the
    scaled group; no list is one the specialised K1 takes; no code repeats
    outside the one list meant to.
  * Finiteness: every recorded buffer of every frame is finite on the oracle.
    CPU and GPU choose different NaN payloads (tests/test_gpu_content_parity.py),
    so a NaN anywhere would need a NaN-aware comparison; here there is none.
  * Every column counts: replacing any one feature code by another changes
    frame 0's `result` (a kernel that dropped, or read twice, one column of
    the design matrix at some count would not go unnoticed for want of effect).
"""
from __future__ import annotations

import numpy as np
import pytest

import shape_util
from ref_configs import (SHAPE_FRAMES, SHAPE_FS, SHAPE_NS, SHAPE_ODD_LISTS, SHAPE_REF_CONFIGS, SHAPE_SIZE, shape_lists,
                         shape_name, shape_of)
from seq_util import ALL_KEYS
from shape_util import NAMES

REGULAR = [shape_name(ns, fs, h) for h in (1, 0) for ns in SHAPE_NS for fs in SHAPE_FS]
ODD = [f"{shape_name(3, 5, h)}_{odd}" for h in (1, 0) for odd in SHAPE_ODD_LISTS]


def test_every_instantiated_shape_is_present_once():
    assert len(REGULAR) == 80 and len(set(REGULAR)) == 80
    assert NAMES == REGULAR + ODD and len(NAMES) == 86
    seen = set()
    for name in REGULAR:
        ns, fs, half = shape_of(name)
        assert name == shape_name(ns, fs, half)
        seen.add((ns, fs, half))
    assert seen == {(ns, fs, h) for ns in range(1, 5) for fs in range(10) for h in (0, 1)}
    for name in ODD:
        assert shape_of(name)[:2] == (3, 5)
    for name, rc in SHAPE_REF_CONFIGS.items():
        assert (rc.width, rc.height) == SHAPE_SIZE == (80, 48) and rc.frames == SHAPE_FRAMES == 3
        # both axes padded; a 4 x 3 block grid with the margins
        assert rc.workset == (96, 64) and rc.blocks == 12
        assert rc.buffer_count == len(rc.not_scaled) + len(rc.scaled) + 3
        assert f"-DR_EDGE={rc.buffer_count - 2}" in rc.ref_build_options()


def test_lists_follow_the_rule():
    for name in REGULAR:
        rc = SHAPE_REF_CONFIGS[name]
        ns, fs, _ = shape_of(name)
        assert (rc.not_scaled, rc.scaled) == shape_lists(ns, fs)
        codes = rc.not_scaled + rc.scaled
        assert codes[0] == 0, name                               # 1.f first, as in every list the reference ships
        assert all(1 <= c <= 12 for c in codes[1:]), name
        assert len(set(codes)) == len(codes), name               # no repeats
    # both precisions take the same list
    for ns in SHAPE_NS:
        for fs in SHAPE_FS:
            a, b = SHAPE_REF_CONFIGS[shape_name(ns, fs, 1)], SHAPE_REF_CONFIGS[shape_name(ns, fs, 0)]
            assert (a.not_scaled, a.scaled) == (b.not_scaled, b.scaled)


@pytest.mark.parametrize("half", [1, 0])
def test_every_code_occurs_in_both_groups(half):
    not_scaled, scaled = set(), set()
    for name in REGULAR:
        rc = SHAPE_REF_CONFIGS[name]
        if rc.half_tmp == half:
            not_scaled |= set(rc.not_scaled)
            scaled |= set(rc.scaled)
    assert not_scaled >= set(range(1, 13)), sorted(set(range(1, 13)) - not_scaled)
    assert scaled >= set(range(1, 13)), sorted(set(range(1, 13)) - scaled)


def test_no_list_is_canonical():
    assert shape_util.canonical((0, 1, 2, 3), (4, 5, 6, 7, 8, 9))
    assert shape_util.canonical((0, 1, 2, 3), tuple(range(4, 13)))
    for name, rc in SHAPE_REF_CONFIGS.items():
        assert not shape_util.canonical(rc.not_scaled, rc.scaled), name
    # the two counts of the canonical lists are in the sweep, permuted
    for half in (1, 0):
        for fs in (6, 9):
            rc = SHAPE_REF_CONFIGS[shape_name(4, fs, half)]
            assert len(rc.not_scaled) == 4 and len(rc.scaled) == fs


def test_odd_lists():
    for half in (1, 0):
        base = shape_name(3, 5, half)
        noconst, cscaled, twice = (SHAPE_REF_CONFIGS[f"{base}_{odd}"] for odd in ("noconst", "cscaled", "twice"))
        assert 0 not in noconst.not_scaled + noconst.scaled
        assert 0 in cscaled.scaled and 0 not in cscaled.not_scaled
        both = set(twice.not_scaled) & set(twice.scaled)
        assert len(both) == 1 and twice.not_scaled[0] == 0
        for rc in (noconst, cscaled):
            codes = rc.not_scaled + rc.scaled
            assert len(set(codes)) == len(codes)
        assert len(set(twice.not_scaled + twice.scaled)) == 7  # the one repeat
        for rc in (noconst, cscaled, twice):
            assert rc.half_tmp == half and all(0 <= c <= 12 for c in rc.not_scaled + rc.scaled)


def _floats(a):
    if a.dtype == np.uint16:  # half tmp_data travels as its bits
        return a.view(np.float16)
    return a if a.dtype.kind == "f" else None


@pytest.mark.parametrize("name", NAMES)
def test_every_record_is_finite(name):
    recs = shape_util.oracle_frames(name)
    assert len(recs) == SHAPE_FRAMES
    for f, rec in enumerate(recs):
        assert set(rec) == set(ALL_KEYS) , sorted(rec)
        for k, v in rec.items():
            x = _floats(v)
            assert x is None or np.isfinite(x).all(), (name, f, k, int((~np.isfinite(x)).sum()))
    # the content reaches past frame 0's special case: pixels accumulate
    assert int(recs[-1]["spp"].max()) == SHAPE_FRAMES


def test_block_min_max_order_the_zeros():
    """A scaled normal component is +0 and -0 over whole walls.  The GPU's
    fmax / fmin order the zeros (-0 < +0) whatever the operand order, and
    mins_maxs is compared bit for bit: the oracle's block minimum of a column
    of mixed zeros is -0 and its maximum +0, wherever in the block they lie."""
    import ctypes as C

    import pyoracle
    cfg = pyoracle.make_cfg(*SHAPE_SIZE, (0,), (1,), 0)
    loop = pyoracle.OracleLoop(cfg)
    assert loop.B == 5 and loop.G == 12
    rng = np.random.default_rng(1)
    tmp = rng.uniform(0.5, 1.5, (loop.G, loop.B, 1024)).astype(np.float32)
    zeros = np.zeros((loop.G, 1024), np.float32)
    zeros[0, 0] = -0.0                 # one -0 first, one last, one in the middle, alternating, halves
    zeros[1, -1] = -0.0
    zeros[2, 517] = -0.0
    zeros[3, ::2] = -0.0
    zeros[4, 1::2] = -0.0
    zeros[5, :512] = -0.0
    zeros[6, 512:] = -0.0
    zeros[7:] = -0.0
    zeros[7, 0], zeros[8, -1], zeros[9, 300], zeros[10, ::2], zeros[11, 256:] = 0.0, 0.0, 0.0, 0.0, 0.0
    tmp[:, 1] = zeros
    tmp = tmp.reshape(-1)
    loop.lib.oracle_fitter(C.byref(cfg), pyoracle._p(loop.weights), pyoracle._p(loop.mins_maxs), pyoracle._p(tmp), 0)
    bits = loop.mins_maxs.view(np.uint32).reshape(loop.G, 2)
    assert (bits[:, 0] == 0x80000000).all() and (bits[:, 1] == 0).all(), bits


@pytest.mark.parametrize("name", NAMES)
def test_every_column_counts(name):
    """One code replaced by another -- the next of 1..12 not in the list, or,
    for the one list that holds all thirteen, its neighbour's -- changes
    frame 0's result."""
    rc = SHAPE_REF_CONFIGS[name]
    codes = rc.not_scaled + rc.scaled
    base = shape_util.oracle_frames(name)[0]["result"]
    for pos, code in enumerate(codes):
        other = next((c for c in ((code + d - 1) % 12 + 1 for d in range(1, 13)) if c not in codes),
                     codes[(pos + 1) % len(codes)])
        assert other != code
        swapped = codes[:pos] + (other,) + codes[pos + 1:]
        got = shape_util.oracle_frames(name, swapped, frames=1)[0]["result"]
        share = float(np.mean(got != base))
        assert share >= 0.01, (name, pos, code, other, share)
