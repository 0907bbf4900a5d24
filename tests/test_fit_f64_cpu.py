"""tests/fit_f64_np.py on the CPU, before anything runs on a GPU: the float64
restatement's solver against an independent one, the SECOND_BLEND_ALPHA = 1
identity that lets tests/test_gpu_fit_f64.py read the fit's output from the
state plane, that no block of its cases has to be left out, where the
reference (the CPU oracle, which equals it) stands against the float64 fit,
that the GPU test's bars fail on a planted defect of 1 % in one block, and
that a case's recorded miss covers that miss and nothing more."""
from __future__ import annotations

import dataclasses

import numpy as np
import pytest

import fit_f64_np as f64
import pyoracle
import scenes_np
from ref_configs import REF_CONFIGS

_runs = {}


def oracle_run(case):
    """Per frame (the oracle's records, the float64 truth) of a case, made once and left unchanged."""
    if case not in _runs:
        rc = f64.case_config(case)
        cfg = pyoracle.make_cfg(rc.width, rc.height, rc.not_scaled, rc.scaled, rc.half_tmp, **rc.knobs())
        assert cfg.second_blend_alpha == 1.0
        recs = scenes_np.run_loop(pyoracle.OracleLoop(cfg), None, rc.width, rc.height, f64.FRAMES,
                                  source=lambda f: f64.case_frame(case, f))
        truth = []
        for f, rec in enumerate(recs):
            fr = f64.case_frame(case, f)
            truth.append(f64.truth_frame(rec["tmp_noisy"], fr["normals"], fr["positions"], rc.width, rc.height, f,
                                         rc.not_scaled, rc.scaled, float(rc.noise_amount)))
        _runs[case] = (recs, truth)
    return _runs[case]


def exact_errors(case):
    """(e_exact, count), (frames, blocks): the oracle's weighted sum against the float64 fit."""
    recs, truth = oracle_run(case)
    pairs = [f64.block_errors(rec["filtered"], t, f) for f, (rec, t) in enumerate(zip(recs, truth))]
    return np.array([e for e, _ in pairs]), np.array([c for _, c in pairs])


IDS = [f64.case_id(c) for c in f64.CASES]


def test_cases_are_the_sixteen():
    assert len(f64.CASES) == len(set(f64.CASES)) == 16


def test_hash_matches_scalar_transcription():
    """hash_random on arrays == the scalar steps of random(), bmfr.cl:161-171, in Python integers."""
    def scalar(a):
        m = 0xFFFFFFFF
        a = ((a + 0x7ed55d16) + (a << 12)) & m
        a = ((a ^ 0xc761c23c) ^ (a >> 19)) & m
        a = ((a + 0x165667b1) + (a << 5)) & m
        a = ((a + 0xd3a2646c) ^ (a << 9)) & m
        a = ((a + 0xfd7046c5) + (a << 3)) & m
        a = ((a ^ 0xb55a4f09) ^ (a >> 16)) & m
        return np.float32(a) / np.float32(4294967295.0)
    seeds = [0, 1, 1023, 1024, 13 * 1024 * 16 + 77, 0x7FFFFFFF, 0xFFFFFFFF]
    got = f64.hash_random(np.array(seeds, np.uint32))
    assert got.dtype == np.float32
    assert [float(v) for v in got] == [float(scalar(s)) for s in seeds]


@pytest.mark.parametrize("name", ["s128x80_h13", "s100x72_h16"], ids=["B13", "B16"])
def test_solver_matches_lstsq(name):
    """Every block of rand 128x80 at B = 13 and B = 16 (the third-order list at
    that size: no listed case has it, so the oracle runs it here), four
    frames: the Householder weights == numpy.linalg.lstsq (SVD) on the same
    float64 matrices, 1e-9 relative."""
    rc = dataclasses.replace(REF_CONFIGS[name], width=128, height=80)
    B = rc.buffer_count
    cfg = pyoracle.make_cfg(rc.width, rc.height, rc.not_scaled, rc.scaled, rc.half_tmp, **rc.knobs())
    recs = scenes_np.run_loop(pyoracle.OracleLoop(cfg), "rand", rc.width, rc.height, 4, f64.SEED)
    for f, rec in enumerate(recs):
        A, _, _, _ = f64.design(rec["tmp_noisy"], B, len(rc.not_scaled), f)
        assert A.shape[0] == f64.num_blocks(rc.width, rc.height)
        w = f64.householder_solve(A, B - 3)
        for g in range(A.shape[0]):
            want = np.linalg.lstsq(A[g, :, :B - 3], A[g, :, B - 3:], rcond=None)[0]
            assert np.linalg.norm(w[g] - want) <= 1e-9 * np.linalg.norm(want), (name, f, g)


@pytest.mark.parametrize("case", f64.CASES, ids=IDS)
def test_second_blend_alpha_one_identity(case):
    """acc == filtered as values on every frame: the state plane is the weighted sum."""
    recs, _ = oracle_run(case)
    for f, rec in enumerate(recs):
        assert np.isfinite(rec["filtered"]).all(), (case, f)
        assert np.array_equal(rec["acc"], rec["filtered"]), (case, f)
    # the colour columns still carry temporal history: spp grows
    assert max(int(rec["spp"].max()) for rec in recs) > 8


@pytest.mark.parametrize("case", f64.CASES, ids=IDS)
def test_no_block_excluded(case):
    """Every block that holds pixels has a non-zero truth norm; the cap on excluded blocks is zero."""
    _, truth = oracle_run(case)
    rc = f64.case_config(case)
    for f, t in enumerate(truth):
        assert np.isfinite(t).all(), (case, f)
        norm, count = f64.block_norms(t, f)
        assert count.size == f64.num_blocks(rc.width, rc.height) and count.sum() == rc.width * rc.height
        assert (norm[count > 0] > 0).all(), (case, f, np.flatnonzero((count > 0) & ~(norm > 0)))


def test_one_pixel_line_blocks_are_there():
    """65x47 and 47x65 really have block columns / rows that hold one pixel line."""
    for name, axis in (("g65x47_h13", 1), ("g47x65_f16", 0)):
        rc = f64.case_config(("rand", name, False))
        lines = set()
        for f in range(f64.FRAMES):
            g = f64.pixel_blocks(rc.width, rc.height, f)
            col = g % f64.blocks_x(rc.width) if axis else g // f64.blocks_x(rc.width)
            lines |= {int(np.ptp(np.nonzero(col == b)[axis])) + 1 for b in np.unique(col)}
        assert 1 in lines, (name, sorted(lines))


def test_where_the_reference_stands():
    """Half tmp_data puts the reference ~1e-3 from the float64 fit, f32 ~1e-6:
    the medians at least 100 x apart for the same scene and B (the unit
    roundoffs differ by 2^13), and no f32 block above 1e-4 -- a guard that the
    restatement and the oracle describe the same problem, not a kernel tolerance."""
    med = {}
    for case in f64.CASES:
        rc = f64.case_config(case)
        e, count = exact_errors(case)
        e = e[count > 0]
        assert np.isfinite(e).all(), case
        q = f64.quantiles(e)
        print(f"{f64.case_id(case)}: e_exact q50 {q['q50']:.3e} q90 {q['q90']:.3e} max {q['max']:.3e}")
        if not rc.half_tmp:
            assert q["max"] <= 1e-4, (case, q)
        if case[1] in f64.MAIN and not case[2]:
            med[(case[0], rc.buffer_count, rc.half_tmp)] = q["q50"]
    assert len(med) == 12
    for (scene, B, half), m in med.items():
        if half:
            assert m >= 100 * med[(scene, B, 0)], (scene, B, m, med[(scene, B, 0)])


def test_bars_see_a_planted_defect():
    """rand 128x80 B = 13 half, frame 3: the oracle's plane as the "fast"
    result passes the GPU test's bars; with the median block 1 % off it fails them."""
    case = ("rand", "s128x80_h13", False)
    recs, truth = oracle_run(case)
    f = 3
    rc = f64.case_config(case)
    clean = recs[f]["filtered"].reshape(rc.height, rc.width, 3)
    e_exact, count = f64.block_errors(clean, truth[f], f)
    held = np.flatnonzero(count > 0)
    g = int(held[np.argsort(e_exact[held])[(held.size - 1) // 2]])  # the median block (the lower of two)
    f64.check_bars([e_exact], [e_exact], [count], "clean")
    bad = clean.copy()
    bad[f64.pixel_blocks(rc.width, rc.height, f) == g] *= np.float32(1 + 1e-2)
    e_bad, _ = f64.block_errors(bad, truth[f], f)
    assert np.array_equal(np.delete(e_bad, g), np.delete(e_exact, g), equal_nan=True)
    with pytest.raises(f64.FitBarMissed):
        f64.check_bars([e_exact], [e_bad], [count], "planted")


def test_known_miss_covers_only_what_is_recorded():
    """A case with a recorded miss: the miss within the record is
    KnownFitBarMiss; more blocks over the bar, a larger excess, a maximum
    beyond its record, or any other bar missed, is FitBarMissed -- the bars
    that are met stay held, and the miss cannot grow unseen."""
    rng = np.random.default_rng(0)
    e = np.exp(rng.normal(np.log(2e-7), 0.3, (4, 50)))   # max / median about 2
    count = np.full(e.shape, 1024)
    known = {"blocks_over_bar": 1, "of_bar": 1.5}
    med = float(np.median(e))

    def with_blocks(*values):
        fast = e.copy()
        for i, v in enumerate(values):   # on blocks at the median of e: the bar there is 3 med
            fast[0, i] = v
        base = e.copy()
        base[0, :len(values)] = med
        return base, fast

    base, fast = with_blocks(4.2 * med)                   # 1.4 x the bar, below 3 x the maximum
    assert f64.check_bars(base, base, count, known=None)["blocks_over_bar"] == 0
    with pytest.raises(f64.KnownFitBarMiss):
        f64.check_bars(base, fast, count, known=known)
    with pytest.raises(f64.FitBarMissed):                 # the same miss without a record
        f64.check_bars(base, fast, count)
    base, fast = with_blocks(4.8 * med)                   # a larger excess than recorded
    with pytest.raises(f64.FitBarMissed):
        f64.check_bars(base, fast, count, known=known)
    base, fast = with_blocks(4.2 * med, 4.2 * med)        # more blocks than recorded
    with pytest.raises(f64.FitBarMissed):
        f64.check_bars(base, fast, count, known=known)
    base, fast = with_blocks(30 * med)                    # the maximum missed, not recorded as missed
    with pytest.raises(f64.FitBarMissed):
        f64.check_bars(base, fast, count, known={"blocks_over_bar": 1, "of_bar": 20.0})
    with pytest.raises(f64.KnownFitBarMiss):              # recorded, within the record
        f64.check_bars(base, fast, count, known={"blocks_over_bar": 1, "of_bar": 20.0, "max_ratio": 100.0})
    with pytest.raises(f64.FitBarMissed):                 # recorded, beyond it
        f64.check_bars(base, fast, count, known={"blocks_over_bar": 1, "of_bar": 20.0, "max_ratio": 2.0})
    base, fast = with_blocks(4.2 * med)                   # the recorded miss, and the quantiles 2.5 x off
    with pytest.raises(f64.FitBarMissed):
        f64.check_bars(base, np.where(fast == base, 2.5 * base, fast), count, known=known)
    assert not issubclass(f64.KnownFitBarMiss, f64.FitBarMissed)
    assert not issubclass(f64.FitBarMissed, f64.KnownFitBarMiss)
