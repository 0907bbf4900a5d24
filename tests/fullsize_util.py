"""Shared by tests/test_gpu_reference_fullsize.py, tests/test_gpu_pair_taps.py
and tests/golden/make_fullsize_digests.py: the full-size cases
(ref_configs.FULL_REF_CONFIGS), their inputs as the library's GPU renderer
makes them, and the digests of the reference's outputs.  TEST INFRASTRUCTURE
ONLY; needs a GPU."""
from __future__ import annotations

import hashlib
import os

import torch

import bmfr_amd
from parity_harness import bits, bmfr_cfg
from seq_util import PLANES

DIGESTS = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "fullsize_digests.json")
# (test id, reference build, half input planes)
CASES = [("f1920x1080_h13", "f1920x1080_h13", 0), ("f3840x2160_h13", "f3840x2160_h13", 0),
         ("f3840x2160_f13", "f3840x2160_f13", 0), ("f3840x2160_h16", "f3840x2160_h16", 0),
         ("f3840x2160_h16_in16", "f3840x2160_h16", 1), ("f7680x4320_h13", "f7680x4320_h13", 0),
         ("f1280x720_h13", "f1280x720_h13", 0), ("f1920x1080_h13_60f", "f1920x1080_h13", 0),
         ("f3840x2160_h13_60f", "f3840x2160_h13", 0)]


def sha(t: torch.Tensor) -> str:
    return hashlib.sha256(bits(t).cpu().numpy().tobytes()).hexdigest()


def frame_planes(rc, f: int, half: int):
    """The synthetic frame f (GPU renderer); with half, rounded to half3 --
    what the half-input path reads -- and the reference gets those values widened."""
    fr = bmfr_amd.synth_frame_device(rc.width, rc.height, f, seed=rc.seed)
    if half:
        h = {k: fr[k].half() for k in PLANES}
        return h, {k: v.float() for k, v in h.items()}
    return fr, fr


def cameras(rc, f: int):
    vp, _ = bmfr_amd.synth_camera(rc.width, rc.height, max(f - 1, 0))
    _, jit = bmfr_amd.synth_camera(rc.width, rc.height, f)
    return vp, jit


def hip_cfg(rc, half_in: int, library_powr: int = 1) -> bmfr_amd.BmfrConfig:
    return bmfr_cfg(rc, library_powr=library_powr, input_half=half_in)
