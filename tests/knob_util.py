"""Content of the knob configurations (ref_configs.KNOB_REF_CONFIGS), shared
by tests/test_knobs_cpu.py, tests/test_gpu_knobs.py and the golden generator.
TEST INFRASTRUCTURE ONLY: imports nothing from bmfr_amd.

Every configuration but k_lit runs scene rand of tests/scenes_np.py, seed 2.

k_lit runs the far wall under a still camera with, on odd frames,
LIT_DELTA = 1 + 2^-20 added to every normal's x component.  The wall has one
normal, so between consecutive frames the normal difference is (+-LIT_DELTA,
0, 0) exactly on every pixel and its squared length the f32 value 1.0000019
(LIT_DISTANCE_SQ); the reprojection does not read normals.  A normal limit of
1.0000049 reaches the reference kernel as the literal 1 (%g), which rejects
every tap; the value itself, cast to float, would accept them.
"""
from __future__ import annotations

import numpy as np

import scenes_np
from ref_configs import KNOB_REF_CONFIGS, knob_set_of
from seq_util import PLANES

SEED = 2
LIT_DELTA = np.float32(1 + 2.0 ** -20)
LIT_DISTANCE_SQ = np.float32(LIT_DELTA * LIT_DELTA)  # 1.0000019


def scene_of(name: str):
    """(scenes_np scene, still camera)"""
    return ("far", True) if knob_set_of(name) == "lit" else ("rand", False)


def frame(name: str, f: int) -> dict:
    """scenes_np.frame of the configuration's content."""
    rc = KNOB_REF_CONFIGS[name]
    scene, still = scene_of(name)
    fr = scenes_np.frame(scene, rc.width, rc.height, f, SEED, still=still)
    if knob_set_of(name) == "lit" and f % 2:
        n = np.array(fr["normals"]).reshape(-1, 3)
        n[:, 0] += LIT_DELTA
        n.setflags(write=False)
        fr["normals"] = n.reshape(-1)
    return fr


def run_loop(loop, name: str, **kw):
    """scenes_np.run_loop over the configuration's frames."""
    rc = KNOB_REF_CONFIGS[name]
    return scenes_np.run_loop(loop, scene_of(name)[0], rc.width, rc.height, rc.frames, SEED,
                              source=lambda f: frame(name, f), **kw)


def frame_digest(fr: dict) -> str:
    """SHA-256 of a frame's planes, previous camera and jitter."""
    import hashlib
    h = hashlib.sha256()
    for k in PLANES:
        h.update(fr[k].tobytes())
    h.update(np.asarray(list(fr["prev_vp"]) + list(fr["jitter"]), np.float32).tobytes())
    return h.hexdigest()
