"""The knob configurations (ref_configs.KNOB_REF_CONFIGS) on the CPU oracle, no
GPU: before tests/test_gpu_knobs.py compares kernels at other values of
noise_amount, the three blend alphas and the two limits, show that on this
content every one of those values decides the result.  The figures are
conditions on the oracle's records, asserted here:

  * every frame's weights and result are finite;
  * each non-default knob of a set, reset alone to the reference's default,
    changes `result` on >= 1 % of its elements in some frame; a limit also
    changes `accept`, blend_alpha changes `noisy`, second_blend_alpha changes
    `acc` and leaves `noisy` and `spp` alone;
  * tight, loose and ends reach spp 14 at frame 13 (second_blend_alpha's
    default 0.1 caps 1 / spp from spp 11 on), k_cut keeps spp at 1;
  * k_lit (knob_util): the normal limit 1.0000049 as the kernel sees it, the
    literal 1, rejects every tap; the same value cast to float accepts them.

Two configurations are pinned to the reference's strict build through golden
vectors (tests/golden/knobs/*.npz, tests/golden/make_golden.py --knobs), read
as tests/test_oracle_cpu.py reads its own."""
from __future__ import annotations

import dataclasses
import json
import os

import numpy as np
import pytest

import knob_util
import pyoracle
from ref_configs import KNOB_REF_CONFIGS, KNOB_SETS, RefConfig, knob_set_of
from seq_util import EXACT_KEYS, POWR_KEYS, digest, sample_idx

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "knobs")
GOLDEN_NAMES = ("k_tight_128x80_h13", "k_loose_100x72_h16")
KNOBS = ("noise_amount", "blend_alpha", "second_blend_alpha", "taa_blend_alpha", "position_limit_squared",
         "normal_limit_squared")
DEFAULTS = {f.name: f.default for f in dataclasses.fields(RefConfig) if f.name in KNOBS}
LIMITS = ("position_limit_squared", "normal_limit_squared")
# k_lit's limit is told from the default by nothing on its content (either rejects every tap): what it
# is told from is the same value without the %g rule, test_lit_limit_is_decided_by_the_g_text
RESET_CASES = [(n, k) for n in KNOB_REF_CONFIGS if knob_set_of(n) != "lit" for k in KNOB_SETS[knob_set_of(n)]]

_cache = {}


def make_cfg(rc):
    return pyoracle.make_cfg(rc.width, rc.height, rc.not_scaled, rc.scaled, rc.half_tmp, **rc.knobs())


def oracle_frames(name, reset=None, cfg_edit=None):
    """The oracle's records over the configuration's frames; reset: a knob put
    back to the reference's default; cfg_edit: applied to the oracle_cfg."""
    key = (name, reset, cfg_edit is not None)
    if key not in _cache:
        rc = KNOB_REF_CONFIGS[name]
        if reset is not None:
            rc = dataclasses.replace(rc, **{reset: DEFAULTS[reset]})
        cfg = make_cfg(rc)
        if cfg_edit is not None:
            cfg_edit(cfg)
        _cache[key] = knob_util.run_loop(pyoracle.OracleLoop(cfg), name)
    return _cache[key]


def share(a, b, key):
    """Largest per-frame share of elements of `key` that differ."""
    return max(float(np.mean(x[key] != y[key])) for x, y in zip(a, b))


def test_knob_values_are_the_literals():
    """"0.05f" is float32(0.05), "1e-3" the double 1e-3; every set differs
    from the defaults where it says it does."""
    k = KNOB_REF_CONFIGS["k_loose_100x72_h16"].knobs()
    assert k["blend_alpha"] == float(np.float32(0.05)) and k["taa_blend_alpha"] == 0.5
    assert k["noise_amount"] == 1e-1 and k["position_limit_squared"] == 0.123456789
    d = RefConfig("d", 128, 80).knobs()
    assert d == dict(noise_amount=1e-2, blend_alpha=float(np.float32(0.2)), second_blend_alpha=float(np.float32(0.1)),
                     taa_blend_alpha=float(np.float32(0.2)), position_limit_squared=0.01, normal_limit_squared=0.1)
    for name, rc in KNOB_REF_CONFIGS.items():
        changed = {key for key in KNOBS if rc.knobs()[key] != d[key]}
        assert changed == set(KNOB_SETS[knob_set_of(name)]), name
    opts = KNOB_REF_CONFIGS["k_ends_128x80_h13"].ref_build_options()
    assert "-DPOSITION_LIMIT_SQUARED=1" in opts and "-DNOISE_AMOUNT=0.5" in opts and "-DBLEND_ALPHA=0.0f" in opts
    assert "-DPOSITION_LIMIT_SQUARED=0.123457" in KNOB_REF_CONFIGS["k_loose_96x64_h7"].ref_build_options()


@pytest.mark.parametrize("name", list(KNOB_REF_CONFIGS))
def test_everything_stays_finite(name):
    recs = oracle_frames(name)
    assert len(recs) == KNOB_REF_CONFIGS[name].frames
    for f, rec in enumerate(recs):
        assert np.isfinite(rec["weights"]).all() and np.isfinite(rec["result"]).all(), f


@pytest.mark.parametrize("name,knob", RESET_CASES, ids=[f"{n}-{k}" for n, k in RESET_CASES])
def test_each_knob_matters_on_its_own(name, knob):
    a, b = oracle_frames(name), oracle_frames(name, reset=knob)
    s = share(a, b, "result")
    print(f"{name} {knob} -> default: result differs on {s:.2%}, accept on {share(a, b, 'accept'):.3%}")
    assert s >= 0.01, (name, knob, s)
    if knob in LIMITS:
        assert share(a, b, "accept") > 0, (name, knob)
    if knob == "blend_alpha":
        assert share(a, b, "noisy") > 0, name
    if knob == "second_blend_alpha":
        assert share(a, b, "acc") > 0, name
        assert share(a, b, "noisy") == 0 and share(a, b, "spp") == 0, name


@pytest.mark.parametrize("name", list(KNOB_REF_CONFIGS))
def test_spp_range(name):
    recs = oracle_frames(name)
    ks = knob_set_of(name)
    if ks in ("tight", "loose", "ends"):
        assert len(recs) == 14 and int(recs[13]["spp"].max()) == 14
    elif ks == "cut":
        assert len(recs) == 14 and all((rec["spp"] == 1).all() for rec in recs)


def test_lit_limit_is_decided_by_the_g_text():
    name = "k_lit_128x80_h13"
    rc = KNOB_REF_CONFIGS[name]
    assert "%g" % rc.normal_limit_squared == "1" and float(np.float32(rc.normal_limit_squared)) > 1.0
    # the content: consecutive frames' normals are LIT_DISTANCE_SQ apart on every pixel, in the
    # kernel's own f32 arithmetic (bmfr.cl:393-396), and nothing else moves the acceptance
    assert float(knob_util.LIT_DISTANCE_SQ) == float(np.float32(1 + 2.0 ** -19))
    assert 1.0 < knob_util.LIT_DISTANCE_SQ < np.float32(rc.normal_limit_squared)
    for f in range(1, rc.frames):
        p, c = (knob_util.frame(name, g)["normals"].reshape(-1, 3) for g in (f - 1, f))
        d = p - c
        assert d.dtype == np.float32
        assert (np.abs(d[:, 0]) == knob_util.LIT_DELTA).all() and (d[:, 1:] == 0).all(), f
        assert ((d[:, 0] * d[:, 0] + d[:, 1] * d[:, 1]) + d[:, 2] * d[:, 2] == knob_util.LIT_DISTANCE_SQ).all(), f
    n = rc.width * rc.height
    cfg = make_cfg(rc)
    assert cfg.normal_limit_sq == 1.0
    for f, rec in enumerate(oracle_frames(name)):
        assert int(rec["spp"].max()) == 1 and not (rec["accept"] == 15).any(), f
        assert (rec["accept"] == 0).all(), f

    def cast(cfg):
        cfg.normal_limit_sq = float(np.float32(rc.normal_limit_squared))
    for f, rec in enumerate(oracle_frames(name, cfg_edit=cast)):
        assert int(rec["spp"].max()) == f + 1, f
        if f > 0:
            assert np.count_nonzero(rec["accept"] == 15) >= 0.9 * n, (f, np.mean(rec["accept"] == 15))


@pytest.mark.parametrize("name", GOLDEN_NAMES)
def test_oracle_matches_reference_golden_vectors(name):
    """As tests/test_oracle_cpu.py: digests on EXACT_KEYS, weights and
    mins_maxs in full, tone / result by sums and samples within its tolerance."""
    rc = KNOB_REF_CONFIGS[name]
    z = np.load(os.path.join(GOLDEN, f"{name}.npz"), allow_pickle=False)
    meta = json.loads(bytes(z["meta"]).decode())
    frames = meta["frames"]
    assert frames == rc.frames and meta["mode"] == "strict"
    assert (meta["scene"], meta["seed"]) == (knob_util.scene_of(name)[0], knob_util.SEED)
    assert meta["knobs"] == {k: getattr(rc, k) if k not in LIMITS else "%g" % getattr(rc, k) for k in KNOBS}
    for f in range(frames):
        assert knob_util.frame_digest(knob_util.frame(name, f)) == meta["inputs"][f], \
            f"inputs of frame {f} changed: regenerate tests/golden/knobs with make_golden.py --knobs"
    got = oracle_frames(name)
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
