#!/usr/bin/env python3
"""Generate the golden vectors under tests/golden/ from the reference's own
kernels.  TEST INFRASTRUCTURE; runs on an MI355X (the reference .cl compiled
by oracle/build_ref.py in strict mode, driven by oracle/ref_run.py).

Inputs are the deterministic synthetic frames of libbmfr's host generator;
their SHA-256 is stored so a changed generator is detected instead of
silently compared.  Per frame the fixture keeps
  * SHA-256 of every bit-exact buffer (seq_util.EXACT_KEYS),
  * weights and mins_maxs in full,
  * tone / result (powr-dependent) as float64 sums and an 8192-element
    strided sample (compared with a tolerance on the CPU side).

Other content and other configurations: make(name, out_dir, configs, scene,
seed) takes the configuration dictionary and a scene of tests/scenes_np.py; the
fixture then records the scene, the seed and the six knob texts of the
configuration.  --knobs makes the fixtures of tests/test_knobs_cpu.py
(ref_configs.KNOB_REF_CONFIGS on scene rand) under tests/golden/knobs/,
--geometry those of tests/test_geometry_cpu.py (GEOMETRY_REF_CONFIGS, the first
geometry_util.GOLDEN_FRAMES frames of each) under tests/golden/geometry/.

Usage (GPU box): python tests/golden/make_golden.py [--out DIR] [config ...]
                 python tests/golden/make_golden.py --knobs [--out DIR] [config ...]
                 python tests/golden/make_golden.py --geometry [--out DIR] [config ...]
"""
from __future__ import annotations

import dataclasses
import json
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
for p in (ROOT, os.path.join(ROOT, "oracle"), os.path.join(ROOT, "tests")):
    sys.path.insert(0, p)

import numpy as np  # noqa: E402
import torch  # noqa: E402

import ref_run  # noqa: E402
import geometry_util  # noqa: E402
import knob_util  # noqa: E402
import scenes_np  # noqa: E402
from ref_configs import (GEOMETRY_REF_CONFIGS, GEOMETRY_SCENE, GEOMETRY_SEED, KNOB_REF_CONFIGS, REF_CONFIGS,  # noqa: E402
                         fmt_g)
from seq_util import EXACT_KEYS, POWR_KEYS, digest, frame_inputs, input_digest, run_loop, sample_idx  # noqa: E402


KNOB_GOLDEN = ("k_tight_128x80_h13", "k_loose_100x72_h16")  # tests/test_knobs_cpu.py GOLDEN_NAMES


def knob_texts(rc) -> dict:
    """The six run-time parameters as the reference's -D string carries them."""
    return {"noise_amount": rc.noise_amount, "blend_alpha": rc.blend_alpha,
            "second_blend_alpha": rc.second_blend_alpha, "taa_blend_alpha": rc.taa_blend_alpha,
            "position_limit_squared": fmt_g(rc.position_limit_squared),
            "normal_limit_squared": fmt_g(rc.normal_limit_squared)}


def make(name: str, out_dir: str = HERE, configs=REF_CONFIGS, scene: str | None = None,
         seed: int | None = None) -> str:
    """scene None: the synthetic sequence (seed: the configuration's)."""
    rc = configs[name]
    dev = lambda a: torch.from_numpy(np.array(a, order="C")).cuda()  # noqa: E731  (a copy: scenes' planes are read-only)
    if scene is None:
        frames = run_loop(ref_run.RefLoop(rc, "strict"), rc, rc.frames, to_device=dev, sync=torch.cuda.synchronize)
        meta = {"seed": rc.seed, "inputs": [input_digest(frame_inputs(rc, f)) for f in range(rc.frames)]}
    else:
        frames = scenes_np.run_loop(ref_run.RefLoop(rc, "strict"), scene, rc.width, rc.height, rc.frames, seed,
                                    to_device=dev, sync=torch.cuda.synchronize)
        meta = {"scene": scene, "seed": seed, "knobs": knob_texts(rc),
                "inputs": [knob_util.frame_digest(scenes_np.frame(scene, rc.width, rc.height, f, seed))
                           for f in range(rc.frames)]}
    meta.update({"config": name, "frames": rc.frames, "mode": "strict",
                 "digests": [{k: digest(fr[k]) for k in EXACT_KEYS} for fr in frames],
                 "stats": []})
    arrays = {}
    for f, fr in enumerate(frames):
        arrays[f"weights_{f}"] = fr["weights"]
        arrays[f"mins_maxs_{f}"] = fr["mins_maxs"]
        st = {}
        for k in POWR_KEYS:
            a = fr[k].astype(np.float64)
            st[k] = {"sum": float(a.sum()), "sumsq": float((a * a).sum())}
            arrays[f"{k}_sample_{f}"] = fr[k][sample_idx(fr[k].size)]
        meta["stats"].append(st)
    os.makedirs(out_dir, exist_ok=True)
    path = os.path.join(out_dir, f"{name}.npz")
    np.savez_compressed(path, meta=np.frombuffer(json.dumps(meta).encode(), np.uint8), **arrays)
    return path


if __name__ == "__main__":
    import argparse
    ap = argparse.ArgumentParser()
    ap.add_argument("configs", nargs="*")
    ap.add_argument("--out", help="output directory (default: tests/golden, with --knobs tests/golden/knobs)")
    ap.add_argument("--knobs", action="store_true", help="the knob fixtures: KNOB_REF_CONFIGS on scene rand")
    ap.add_argument("--geometry", action="store_true", help="the geometry fixtures: GEOMETRY_REF_CONFIGS on scene rand")
    a = ap.parse_args()
    if a.geometry:
        for n in a.configs or list(geometry_util.GOLDEN_FRAMES):
            cut = {n: dataclasses.replace(GEOMETRY_REF_CONFIGS[n], frames=geometry_util.GOLDEN_FRAMES[n])}
            print(make(n, a.out or os.path.join(HERE, "geometry"), cut, GEOMETRY_SCENE, GEOMETRY_SEED), flush=True)
    elif a.knobs:
        for n in a.configs or KNOB_GOLDEN:
            assert knob_util.scene_of(n) == ("rand", False), n
            print(make(n, a.out or os.path.join(HERE, "knobs"), KNOB_REF_CONFIGS, "rand", knob_util.SEED), flush=True)
    else:
        for n in a.configs or list(REF_CONFIGS):
            print(make(n, a.out or HERE), flush=True)
