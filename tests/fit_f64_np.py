"""The block fit in float64: what fit_block and oracle_weighted_sum of
oracle/bmfr_oracle.c compute, with every rounding removed and every discrete
decision kept as the reference takes it.  TEST INFRASTRUCTURE ONLY: numpy,
vectorised over blocks, nothing from bmfr_amd.

The problem statement is the frame's design matrix as accumulate_noisy_data
left it (the oracle record tmp_noisy, [block][column][1024 rows], B columns,
the last three the colour channels) -- its half or f32 quantisation included:

  scaling   columns >= n_not_scaled: min and max over the 1024 rows (exact in
            any precision); (v - min) / (max - min) when the reference divides,
            fabsf(max - min) > 1.0f in f32, else v - min; not rounded back
  noise     columns 1 .. B-4, row r: noise_amount * 2 * (hash_random(r +
            fb 1024 + frame B 1024) - 0.5f); hash and - 0.5f in uint32 / f32 as
            add_random forms them, product and sum in float64
  solve     Householder QR without pivoting, the reference's column order,
            back substitution: (B-3) x 3 weights per block
  sum       the pixel's block from the 16-entry offset table, the features
            from the frame's f32 normals and positions (monomials in f32, as
            feature() forms them), scaled with the block's min / max in
            float64, the dot product in float64, clamped at 0

block_errors measures a plane against that truth block by block; check_bars
holds a not-bit-exact path to the reference's own distance from the truth
(tests/test_gpu_fit_f64.py; tests/test_fit_f64_cpu.py checks the solver
against numpy.linalg.lstsq and the bars against a planted defect).

With second_blend_alpha = 1 the blend weight of accumulate_filtered_data is
max(1 / spp, 1) = 1, so the state plane filtered_accumulated is the frame's
weighted sum, value for value, at every frame: no debug entry point is needed
to see the fit's output.
"""
from __future__ import annotations

import dataclasses

import numpy as np

from ref_configs import GEOMETRY_REF_CONFIGS, REF_CONFIGS

EDGE, PIXELS = 32, 1024
# BLOCK_OFFSETS of the reference (bmfr.cl:267-285)
OFFSETS = ((-14, -14), (4, -6), (-8, 14), (8, 0), (-10, -8), (2, 12), (12, -12), (-10, 0), (12, 14), (-8, -16),
           (6, 6), (-2, -2), (6, -14), (-16, 12), (14, -4), (-6, 4))
FRAMES = 17   # all 16 block-grid offsets and the wrap
SEED = 2      # tests/test_scenes_np.py asserts what the scenes reach for this seed

# (scene, configuration, half input planes): canonical lists only, the generic kernels have no fast form
MAIN = ("s128x80_h13", "s128x80_f13", "s100x72_h16", "s96x64_f16")
CASES = [(s, n, False) for s in ("pan", "far", "rand") for n in MAIN] + \
        [("far", "s100x72_h16", True), ("rand", "s100x72_h16", True),   # BASELINE config 5's kernel
         ("rand", "g65x47_h13", False), ("rand", "g47x65_f16", False)]  # block columns / rows of one pixel line


def case_id(case) -> str:
    scene, name, half_in = case
    return f"{scene}-{name[1:]}" + ("_in16" if half_in else "")


def case_config(case):
    """The case's RefConfig: its size, lists and tmp_data precision, SECOND_BLEND_ALPHA 1, 17 frames."""
    name = case[1]
    rc = REF_CONFIGS[name] if name in REF_CONFIGS else GEOMETRY_REF_CONFIGS[name]
    return dataclasses.replace(rc, name=f"fit64_{name}", second_blend_alpha="1.0f", frames=FRAMES)


def case_frame(case, f):
    """scenes_np.frame of the case; half input planes: the planes rounded to
    half and widened, what the half path reads and the oracle is given."""
    import scenes_np
    scene, _, half_in = case
    rc = case_config(case)
    fr = scenes_np.frame(scene, rc.width, rc.height, f, SEED)
    if half_in:
        for k in ("noisy", "normals", "positions", "albedo"):
            fr[k] = fr[k].astype(np.float16).astype(np.float32)
    return fr


# ------------------------------------------------------------------ pieces ----
def hash_random(a) -> np.ndarray:
    """random(), bmfr.cl:161-171: uint32 hash, then (float)a / (float)UINT_MAX in f32."""
    a = np.asarray(a, np.uint32).copy()
    u = np.uint32
    with np.errstate(over="ignore"):
        a = (a + u(0x7ed55d16)) + (a << u(12))
        a = (a ^ u(0xc761c23c)) ^ (a >> u(19))
        a = (a + u(0x165667b1)) + (a << u(5))
        a = (a + u(0xd3a2646c)) ^ (a << u(9))
        a = (a + u(0xfd7046c5)) + (a << u(3))
        a = (a ^ u(0xb55a4f09)) ^ (a >> u(16))
    return a.astype(np.float32) / np.float32(4294967295.0)


def blocks_x(W: int) -> int:
    return (W + EDGE - 1) // EDGE + 1


def num_blocks(W: int, H: int) -> int:
    return blocks_x(W) * ((H + EDGE - 1) // EDGE + 1)


def pixel_blocks(W: int, H: int, frame: int) -> np.ndarray:
    """(H, W): the block whose weights a pixel's weighted sum reads (bmfr.cl:703-758)."""
    ox, oy = OFFSETS[frame % 16]
    gx = (np.arange(W) + EDGE // 2 - ox) // EDGE
    gy = (np.arange(H) + EDGE // 2 - oy) // EDGE
    return gy[:, None] * blocks_x(W) + gx[None, :]


def widen(tmp: np.ndarray) -> np.ndarray:
    """A tmp_data record as f32 values (half buffers travel as their bits)."""
    return tmp.view(np.float16).astype(np.float32) if tmp.dtype == np.uint16 else np.asarray(tmp, np.float32)


def design(tmp_noisy, B: int, n_not_scaled: int, frame: int, noise_amount: float = 1e-2):
    """-> (A, mins, maxs, divide): the matrices the fit solves, (G, 1024, B)
    float64, and per block and scaled column the min, the max (f32) and
    whether the reference divides by max - min."""
    t = widen(tmp_noisy).reshape(-1, B, PIXELS)
    A = t.astype(np.float64).transpose(0, 2, 1).copy()
    mins, maxs = t[:, n_not_scaled:B - 3].min(axis=2), t[:, n_not_scaled:B - 3].max(axis=2)
    divide = np.abs(maxs - mins) > np.float32(1.0)  # scale(), bmfr.cl:200-205, in f32
    lo, hi = mins.astype(np.float64), maxs.astype(np.float64)
    den = np.where(divide, hi - lo, 1.0)
    A[:, :, n_not_scaled:B - 3] = (A[:, :, n_not_scaled:B - 3] - lo[:, None, :]) / den[:, None, :]
    r = np.arange(PIXELS, dtype=np.int64)
    for fb in range(1, B - 3):  # add_random(), bmfr.cl:173-182: column 0 and the colours get none
        seed = (r + fb * PIXELS + frame * B * PIXELS).astype(np.uint32)
        h = hash_random(seed) - np.float32(0.5)
        A[:, :, fb] += noise_amount * 2.0 * h.astype(np.float64)[None, :]
    return A, mins, maxs, divide


def householder_solve(A: np.ndarray, n: int) -> np.ndarray:
    """Least squares of every block at once: (G, m, n + 3) -> (G, n, 3).
    Householder QR on the first n columns in their order, no pivoting, the
    reflections applied to the three right-hand sides, back substitution."""
    A = A.copy()
    for k in range(n):
        x = A[:, k:, k]
        u = x.copy()
        u[:, 0] += np.copysign(np.sqrt((x * x).sum(axis=1)), x[:, 0])  # the sign that does not cancel
        ulen2 = (u * u).sum(axis=1)
        T = A[:, k:, k:]
        dots = np.einsum("gi,gij->gj", u, T)
        T -= (2.0 * dots / ulen2[:, None])[:, None, :] * u[:, :, None]
    R, Y = A[:, :n, :n], A[:, :n, n:]
    w = np.zeros((A.shape[0], n, 3))
    for i in range(n - 1, -1, -1):
        w[:, i] = (Y[:, i] - np.einsum("gj,gjc->gc", R[:, i, i + 1:], w[:, i + 1:])) / R[:, i, i, None]
    return w


def features(codes, normals, positions) -> np.ndarray:
    """(H W, len(codes)) f32: feature(), with the monomials multiplied out in f32."""
    n, p = np.asarray(normals, np.float32).reshape(-1, 3), np.asarray(positions, np.float32).reshape(-1, 3)
    out = np.empty((n.shape[0], len(codes)), np.float32)
    for j, c in enumerate(codes):
        if c == 0:
            out[:, j] = 1.0
        elif c <= 3:
            out[:, j] = n[:, c - 1]
        else:
            v = p[:, (c - 4) % 3]
            out[:, j] = v if c <= 6 else v * v if c <= 9 else v * v * v
    return out


def truth_frame(tmp_noisy, normals, positions, W, H, frame, not_scaled, scaled, noise_amount=1e-2):
    """The frame's weighted-sum output of the float64 fit, (H, W, 3) float64."""
    ns, B = len(not_scaled), len(not_scaled) + len(scaled) + 3
    A, mins, maxs, divide = design(tmp_noisy, B, ns, frame, noise_amount)
    assert A.shape[0] == num_blocks(W, H), (A.shape, W, H)
    weights = householder_solve(A, B - 3)
    g = pixel_blocks(W, H, frame).reshape(-1)
    v = features(tuple(not_scaled) + tuple(scaled), normals, positions).astype(np.float64)
    lo, hi = mins.astype(np.float64)[g], maxs.astype(np.float64)[g]
    v[:, ns:] = (v[:, ns:] - lo) / np.where(divide[g], hi - lo, 1.0)
    out = np.einsum("pf,pfc->pc", v, weights[g])
    return np.maximum(out, 0.0).reshape(H, W, 3)


# ------------------------------------------------------------------ errors ----
def block_norms(plane, frame: int):
    """Per block: the L2 norm of `plane` ((H, W, 3)) over the block's in-image pixels x 3, and their count."""
    plane = np.asarray(plane, np.float64)
    H, W = plane.shape[:2]
    g = pixel_blocks(W, H, frame).reshape(-1)
    G = num_blocks(W, H)
    sq = np.bincount(g, weights=(plane.reshape(-1, 3) ** 2).sum(axis=1), minlength=G)
    return np.sqrt(sq), np.bincount(g, minlength=G)


def block_errors(got, truth, frame: int):
    """Per block e[g] = |got - truth|_2 / |truth|_2 over the block's in-image
    pixels x 3 channels (NaN for a block without pixels), and the pixel count."""
    truth = np.asarray(truth, np.float64)
    got = np.asarray(got, np.float64).reshape(truth.shape)
    num, count = block_norms(got - truth, frame)
    den, _ = block_norms(truth, frame)
    with np.errstate(divide="ignore", invalid="ignore"):
        return np.where(count > 0, num / den, np.nan), count


def quantiles(e) -> dict:
    e = np.asarray(e, np.float64)
    return {"q50": float(np.median(e)), "q90": float(np.quantile(e, 0.9)), "max": float(e.max())}


# -------------------------------------------------------------------- bars ----
# What fast_fit changes in the fit, each against the reference's correctly rounded form:
#   - the pivot's square root and reciprocal and the back substitution's divisions at hardware
#     precision, 1 ulp instead of 1/2 ulp;
#   - the scaling of a column as one fused x s + o with s = rcp(max - min) (1 ulp) and o = RN(-min s),
#     in the fit and in the weighted sum alike, instead of a subtraction and a correctly rounded
#     division: one rounding per element instead of two, on a factor 1 ulp off.  The constant column
#     is in the basis, so an offset common to a column changes no fitted value;
#   - the step-0 noise as one f32 fused multiply-add on the amount rounded to f32 instead of a sum in
#     double rounded once: within an ulp of the element;
#   - the trailing update fused (fewer roundings than the reference's three), and with f32 tmp_data
#     the squares of the column norms fused into their sums (one rounding fewer each);
#   - the wave-wide sums as butterflies: another association, the same length.
# No operation's error bound is more than twice the reference's, so 2 x on the stable quantiles; an
# extreme over a few hundred samples, or one block against its own lucky draw, gets 3 x for that
# sampling noise.
QUANTILE_FACTOR = 2.0
MAX_FACTOR = 3.0
BLOCK_FACTOR = 3.0


class FitBarMissed(AssertionError):
    """An accuracy bar against the float64 fit is missed: a failure."""


class KnownFitBarMiss(AssertionError):
    """Only the bars a case is recorded to miss are missed, and no further than
    recorded: the one thing an expected failure of that case covers."""


def check_bars(e_exact, e_fast, count, where="", record=None, known=None) -> dict:
    """e_exact, e_fast, count: (frames, blocks).  Over the blocks that hold
    pixels, all frames together: per block e_fast <= 3 max(e_exact,
    median(e_exact)); q50 and q90 of e_fast <= 2 x e_exact's; max <= 3 x.
    Returns the figures (record: called with them first, met or missed).

    A missed bar raises FitBarMissed.  known: the recorded miss of a case,
    {"blocks_over_bar": n, "of_bar": x} for the per-block bar and, where the
    maximum is missed too, "max_ratio": r.  Then the bars not named there are
    held as ever, a named bar missed further than recorded (more blocks over
    it, a larger excess, a larger ratio) raises FitBarMissed as well, and only
    a miss within the record raises KnownFitBarMiss."""
    e_exact, e_fast, count = (np.asarray(a).reshape(len(e_exact), -1) for a in (e_exact, e_fast, count))
    ok = count > 0
    assert ok.any() and np.isfinite(e_exact[ok]).all() and np.isfinite(e_fast[ok]).all(), where
    ex, fa = e_exact[ok], e_fast[ok]
    qe, qf = quantiles(ex), quantiles(fa)
    ratio = {k: qf[k] / qe[k] for k in qe}
    excess = np.where(ok, e_fast / (BLOCK_FACTOR * np.maximum(e_exact, qe["q50"])), 0.0)

    def block(f, g, **more):
        return {"frame": int(f), "block": int(g), "pixels": int(count[f, g]), "e_fast": float(f"{e_fast[f, g]:.3e}"),
                "e_exact": float(f"{e_exact[f, g]:.3e}"), **more}

    f, g = np.unravel_index(int(np.argmax(np.where(ok, e_fast, -1.0))), ok.shape)
    over = [block(bf, bg, of_bar=float(f"{excess[bf, bg]:.3f}")) for bf, bg in np.argwhere(excess > 1.0)]
    bf, bg = np.unravel_index(int(np.argmax(excess)), ok.shape)
    stats = {"exact": qe, "fast": qf, "ratio": ratio, "blocks": int(ok.sum()), "worst_block": block(f, g),
             "worst_block_vs_bar": block(bf, bg, of_bar=float(f"{excess[bf, bg]:.3f}")),
             "blocks_over_bar": len(over), "over_bar": over}
    missed = {}
    if over:
        missed["block"] = (f"{len(over)} blocks above {BLOCK_FACTOR} max(e_exact, median), "
                           f"worst {excess.max():.3f} x the bar")
    for k in ("q50", "q90"):
        if not qf[k] <= QUANTILE_FACTOR * qe[k]:
            missed[k] = f"{k} {qf[k]:.3e} > {QUANTILE_FACTOR} x {qe[k]:.3e}"
    if not qf["max"] <= MAX_FACTOR * qe["max"]:
        missed["max"] = f"max {qf['max']:.3e} > {MAX_FACTOR} x {qe['max']:.3e}"
    stats["missed"] = list(missed.values())
    if record is not None:
        record(stats)
    if not missed:
        return stats
    if known is None:
        raise FitBarMissed((where, stats["missed"], stats))
    allowed = {"block"} | ({"max"} if "max_ratio" in known else set())
    beyond = [m for k, m in missed.items() if k not in allowed]
    if "block" in missed and (len(over) > known["blocks_over_bar"] or excess.max() > known["of_bar"]):
        beyond.append(f"per-block bar missed further than recorded ({known['blocks_over_bar']} blocks, "
                      f"{known['of_bar']} x the bar): {missed['block']}")
    if "max" in missed and "max" in allowed and ratio["max"] > known["max_ratio"]:
        beyond.append(f"maximum missed further than recorded ({known['max_ratio']} x): {ratio['max']:.3f} x")
    if beyond:
        raise FitBarMissed((where, beyond, stats))
    raise KnownFitBarMiss((where, stats["missed"], stats))
