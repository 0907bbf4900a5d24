"""bench.py's plain run (`--gpus 1 --steps K --warmup W`, no --full): K timed
frames, the result line's fields, nothing of what --full measures, and
--dump-outputs: the file holds the TAA output of the last timed frame, bit
for bit what a Denoiser with the bench's configuration computes here from
the same frames."""
from __future__ import annotations

import json
import os
import subprocess
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
W, H, STEPS, WARMUP = 160, 96, 3, 2  # 5 x 3 blocks: a one-launch frame, an edge block row


def test_plain_run_times_k_frames_and_dumps_last_output(gpu, tmp_path):
    import torch

    import bmfr_amd
    dump = tmp_path / "out"
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--steps", str(STEPS),
                        "--warmup", str(WARMUP), "--width", str(W), "--height", str(H), "--spin-up", "0",
                        "--dump-outputs", str(dump)], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr[-2000:]
    lines = [ln for ln in r.stdout.splitlines() if ln.startswith("{")]
    assert len(lines) == 1, r.stdout[-2000:]
    line = json.loads(lines[0])
    assert line["unit"] == "ms/frame" and line["higher_is_better"] is False and line["dtype"] == "f32+f16 tmp_data"
    assert line["steps"] == STEPS and line["warmup"] == WARMUP and line["config"]["frames_timed"] == STEPS
    assert line["ms_per_step"] == line["value"] > 0
    # what --full adds is not in a plain line
    assert not [k for k in line if k.startswith("ms_per_frame_")], sorted(line)
    assert "cpu_baseline" not in line and "psnr_db" not in line
    assert os.listdir(dump) == ["output.npy"]
    got = np.load(dump / "output.npy")
    assert got.dtype == np.float32 and got.shape == (W * H, 3)

    # the bench's configuration and frames 0 .. WARMUP + STEPS - 1, here
    den = bmfr_amd.Denoiser(bmfr_amd.BmfrConfig(image_width=W, image_height=H, use_half_precision_in_tmp_data=1,
                                                fast_fit=1))
    for f in range(WARMUP + STEPS):
        fr = bmfr_amd.synth_frame_device(W, H, f)
        vp, _ = bmfr_amd.synth_camera(W, H, max(f - 1, 0))
        _, jit = bmfr_amd.synth_camera(W, H, f)
        den.process_frame(fr["noisy"], fr["normals"], fr["positions"], fr["albedo"], vp, jit, f)
    want = den.copy_output(torch.empty(W * H * 3, device="cuda")).cpu().numpy().reshape(-1, 3)
    assert np.isfinite(want).all() and want.max() > 0
    assert got.tobytes() == want.tobytes(), f"max |diff| {np.abs(got - want).max()}"
