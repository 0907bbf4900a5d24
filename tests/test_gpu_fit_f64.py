"""fast_fit against the float64 least-squares fit, block by block
(tests/fit_f64_np.py; tests/test_fit_f64_cpu.py checks the method on the CPU).

fast_fit is the one arithmetic in the library that is not bit-exact, and every
other check it has is a relative L2 norm of `result` -- after the temporal
blend, the albedo, the tone curve and TAA, over a frame or a 32x32 tile, with
the distance between the reference's two builds as the yardstick.  The block
fit has a ground truth, the least-squares solution of the block's design
matrix in float64, and the reference has a distance from it: that distance,
measured here on the same blocks, is the bar.

Each case runs two contexts for 17 frames (all 16 block-grid offsets and the
wrap), fast_fit = 0 and 1, both with second_blend_alpha = 1 and otherwise
default, and the CPU oracle on the same frames.  With that alpha the state
plane filtered_accumulated is the frame's weighted sum, value for value.  Per
frame:

  1. the exact context's filtered_accumulated == the oracle's `filtered` as
     values: anchors the identity and the oracle to the kernel
  2. the fast context's noisy_accumulated, spp and prev_frame_pixel == the
     exact context's bit for bit: the fit does not feed them
  3. over the 17 frames the fast plane differs in bits from the exact one
  4. per block, e = |plane - truth| / |truth| over the block's in-image
     pixels: e_fast[g] <= 3 max(e_exact[g], median(e_exact)), the median over
     the case's blocks of all frames
  5. over those blocks: q50 and q90 of e_fast <= 2 x e_exact's, max <= 3 x

The factors are fit_f64_np's (where they come from is written there); the
bars are relative to the reference's own accuracy, never to fast_fit's.  The
figures go to the parity log as fit_f64_<case> (profiles/fit_f64.json), with,
unasserted, the quantiles of |fast - exact| / |truth|, the per-block bar held
the other way round (the reference against fast_fit's accuracy), both paths'
blocks above 3 x the reference's median and log(e_fast / e_exact)'s mean and
spread.

Measured on an MI355X: with half tmp_data every quantile of e_fast is within
0.98-1.014 x the reference's and no block above 0.38 of its bar.  The three
cases at 128x80, B = 13 with f32 tmp_data miss the per-block bar on 4, 3 and
2 of 292 blocks (rand also the bar on the maximum, 4.03 x) and are strict
expected failures of KnownFitBarMiss, which covers that recorded miss and
nothing else: every other bar of those cases fails plainly, and so does the
miss once it grows.  KNOWN_BAR_MISS has the figures and why that is sampling
noise of two independent f32 roundings, not a defect.
"""
from __future__ import annotations

import numpy as np
import pytest

import fit_f64_np as f64
from parity_harness import Suite
from seq_util import compare_exact

pytestmark = pytest.mark.gpu

SUITE = Suite(f64.case_frame, f64.case_config, f64.FRAMES)

# case -> the recorded miss of a case whose miss is inherent in comparing two f32 roundings block by
# block: a strict expected failure of KnownFitBarMiss alone.  Assertions 1-3, the bars on q50 and q90 and
# (pan, far) the bar on the maximum are held there as everywhere and fail plainly; so does the recorded
# miss once it grows: more blocks over the per-block bar, a larger excess, a larger ratio of the maxima
# ("known": check_bars' pins, the measured figures rounded up in the last digit).
#
# Measured on an MI355X (profiles/fit_f64.json).  The three cases with f32 tmp_data at B = 13 miss the
# per-block bar on 4, 3 and 2 of their 292 blocks, and rand the bar on the maximum through one of those
# blocks.  What the log says about them:
#   - their populations are the reference's: q50 and q90 of e_fast 0.91-1.02 x e_exact's; blocks above
#     3 x the reference's median, exact / fast: 12 / 11, 15 / 11, 12 / 15 (blocks_above_3_median): the
#     fast path's tail is not the heavier one;
#   - log(e_fast / e_exact) over the blocks has mean -0.07..+0.01 and standard deviation 0.47-0.60
#     (log_ratio): no bias, and a spread under which log 3 = 1.1 is two standard deviations.  With half
#     tmp_data both paths share the matrix's quantisation error and no block is above 0.38 of its bar;
#     with f32 tmp_data nothing is shared (|fast - exact| / |truth| has e's own median), a block's two
#     errors are independent draws, and the bar asks one to be within 3 x of the other;
#   - the reference does not meet that either: held the other way round, e_exact <= 3 max(e_fast,
#     median(e_fast)), it misses on 4, 1 and 2 blocks of the same cases, full 1024-pixel blocks among
#     them, and on 2 and 2 blocks of pan and far at 96x64 B = 16, where fast_fit misses on none
#     (mirror_blocks_over_bar).
# All nine blocks over the bar are partial blocks (64 to 832 in-image pixels; 207 of the 292 are
# partial), five of them in the bottom block row, and B = 16 at 96x64 and 47x65 has none.  Neither is a
# class: this test's body on the swapped configurations (f32 tmp_data at 96x64 B = 13 and at 128x80
# B = 16; not committed as cases: the issue fixes those) gave forward misses 2 / 0 / 0 at 96x64 B = 13
# and 2 / 0 / 1 at 128x80 B = 16 (pan / far / rand), three of those five on full 1024-pixel blocks,
# against mirror misses 2 / 0 / 0 and 3 / 1 / 0: 14 forward and 17 mirror misses over the twelve f32
# runs' 2934 blocks.  The largest excess over the bar is rand's 2.44 x forward and 1.75 x mirrored.  So: the
# sampling noise of a per-block comparison of two f32 roundings, on about 0.5 % of the blocks either way;
# nothing to resolve was found in fast_fit's arithmetic, and the bars stay where the method put them.
_F13 = ("{n} of 292 blocks above 3 max(e_exact, median): worst {w}; q50 / q90 / max of e_fast {r} x e_exact's.  "
        "Two independent f32 roundings per block: no bias (mean log ratio {b}), fast_fit's tail no heavier than "
        "the reference's, and the reference held to the same bar against fast_fit misses on {m} blocks")
KNOWN_BAR_MISS = {
    ("pan", "s128x80_f13", False): {"known": {"blocks_over_bar": 4, "of_bar": 1.350}, "reason": _F13.format(
        n=4, w="e_fast 9.28e-7 against e_exact 1.31e-7, median 2.29e-7 (frame 0, block 3, 64 pixels): 1.35 x the bar",
        r="1.02 / 0.92 / 1.17", b="-0.02", m=4)},
    ("far", "s128x80_f13", False): {"known": {"blocks_over_bar": 3, "of_bar": 1.276}, "reason": _F13.format(
        n=3, w="e_fast 8.79e-7 against e_exact 2.30e-7, median 2.00e-7 (frame 0, block 17, 448 pixels): 1.28 x the bar",
        r="1.02 / 0.94 / 1.05", b="+0.01", m=1)},
    ("rand", "s128x80_f13", False): {"known": {"blocks_over_bar": 2, "of_bar": 2.440, "max_ratio": 4.029},
                                     "reason": _F13.format(
        n=2, w="e_fast 5.84e-6 against e_exact 7.98e-7 (frame 14, block 16, 128 pixels): 2.44 x the bar, and the "
               "case's maximum, 4.03 x e_exact's 1.45e-6 against the bar of 3 x",
        r="0.91 / 1.02 / 4.03", b="-0.07", m=2)}}
# case -> (frame, blocks) whose own figures go to the log as well: the four blocks under the 32x32 tile
# at (96, 64) of frame 0, the one tests/test_gpu_content_parity.py's KNOWN_TILE_MISS is about
LOGGED_BLOCKS = {("far", "s100x72_h16", False): (0, (13, 14, 18, 19))}

PARAMS = [pytest.param(c, id=f64.case_id(c), marks=[pytest.mark.xfail(strict=True, raises=f64.KnownFitBarMiss,
                                                                      reason=KNOWN_BAR_MISS[c]["reason"])]
                       if c in KNOWN_BAR_MISS else []) for c in f64.CASES]


def sig(q: dict) -> dict:
    return {k: float(f"{v:.3e}") for k, v in q.items()}


@pytest.mark.parametrize("case", PARAMS)
def test_fast_fit_against_float64_fit(case, gpu, parity_log):
    rc = f64.case_config(case)
    W, H, half_in = rc.width, rc.height, case[2]
    where = f"fit_f64[{f64.case_id(case)}]"
    oracle = SUITE.oracle_frames(case)
    exact = SUITE.fused_frames(case, half_in=half_in)
    fast = SUITE.fused_frames(case, half_in=half_in, fast_fit=1)
    SUITE.clear()
    assert len(oracle) == len(exact) == len(fast) == f64.FRAMES
    # 1: the identity, and the oracle, against the kernel
    for f in range(f64.FRAMES):
        assert np.isfinite(oracle[f]["filtered"]).all(), (where, f)
        assert np.array_equal(exact[f]["acc"], oracle[f]["filtered"]), f"{where} frame {f}: exact path != oracle"
    # 2: what the fit does not feed
    compare_exact(fast, exact, ("noisy", "spp", "prev_pixel"), where)
    # 3: not vacuous
    assert any(a["acc"].tobytes() != b["acc"].tobytes() for a, b in zip(fast, exact)), f"{where}: fast_fit == exact"
    # 4, 5: accuracy against the float64 fit
    e_exact, e_fast, d, count = [], [], [], []
    for f in range(f64.FRAMES):
        fr = f64.case_frame(case, f)
        truth = f64.truth_frame(oracle[f]["tmp_noisy"], fr["normals"], fr["positions"], W, H, f, rc.not_scaled,
                                rc.scaled, float(rc.noise_amount))
        ee, n = f64.block_errors(exact[f]["acc"], truth, f)
        ef, _ = f64.block_errors(fast[f]["acc"], truth, f)
        diff, _ = f64.block_norms(fast[f]["acc"].astype(np.float64).reshape(H, W, 3) -
                                  exact[f]["acc"].astype(np.float64).reshape(H, W, 3), f)
        norm, _ = f64.block_norms(truth, f)
        assert (norm[n > 0] > 0).all(), (where, f)
        e_exact.append(ee), e_fast.append(ef), count.append(n)
        d.append(np.where(n > 0, diff / np.where(n > 0, norm, 1.0), np.nan))
    held = np.array(count) > 0

    def unasserted():
        """What the log keeps beside the bars: the per-block bar held the other way round (the reference
        against fast_fit's accuracy), each path's blocks above 3 x the reference's median, and the mean
        and spread of log(e_fast / e_exact) over the blocks."""
        ee, ef = np.array(e_exact)[held], np.array(e_fast)[held]
        mirror = ee / (f64.BLOCK_FACTOR * np.maximum(ef, np.median(ef)))
        lr = np.log(ef / ee)
        return {"mirror_blocks_over_bar": int((mirror > 1.0).sum()),
                "mirror_worst_of_bar": float(f"{mirror.max():.3f}"),
                "blocks_above_3_median": {"exact": int((ee > 3 * np.median(ee)).sum()),
                                          "fast": int((ef > 3 * np.median(ee)).sum())},
                "log_ratio": {"mean": float(f"{lr.mean():.3f}"), "std": float(f"{lr.std():.3f}")}}

    def record(stats):
        extra = {}
        if case in LOGGED_BLOCKS:
            f, blocks = LOGGED_BLOCKS[case]
            extra["blocks_of_interest"] = {"frame": f, "blocks": {
                str(g): {"pixels": int(count[f][g]), "e_exact": float(f"{e_exact[f][g]:.3e}"),
                         "e_fast": float(f"{e_fast[f][g]:.3e}")} for g in blocks}}
        parity_log(f"fit_f64_{f64.case_id(case).replace('-', '_')}", {
            **extra,
            "scene": case[0], "config": case[1], "input_half": int(half_in), "frames": f64.FRAMES,
            "blocks": stats["blocks"], "e_exact": sig(stats["exact"]), "e_fast": sig(stats["fast"]),
            "ratio": {k: float(f"{v:.3f}") for k, v in stats["ratio"].items()},
            "worst_block": stats["worst_block"], "worst_block_vs_bar": stats["worst_block_vs_bar"],
            "blocks_over_bar": stats["blocks_over_bar"], "over_bar": stats["over_bar"], **unasserted(),
            "fast_minus_exact_over_truth": sig(f64.quantiles(np.array(d)[held])), "missed": stats["missed"]})
        print(f"{where}: e_exact {sig(stats['exact'])} e_fast {sig(stats['fast'])} ratio {stats['ratio']} "
              f"worst {stats['worst_block']} vs bar {stats['worst_block_vs_bar']}")

    f64.check_bars(e_exact, e_fast, count, where, record=record, known=KNOWN_BAR_MISS.get(case, {}).get("known"))
