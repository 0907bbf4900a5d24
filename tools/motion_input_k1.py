#!/usr/bin/env python3
"""K1 event time with and without a caller-supplied previous-frame pixel plane
(bmfr_frame_inputs.prev_pixel), on the GPU.

  python tools/motion_input_k1.py [W H] [--frames N] [--fast-fit] [--third-order] [--half-tmp 0|1]

A first context runs the synthetic sequence by camera matrix and keeps the
plane it stored for every frame (bmfr_state_view.prev_frame_pixel).  Then two
contexts run the sequence frame by frame: M projects with the matrix again, P
is fed the recorded plane and a NaN matrix, so both do the same work
downstream of the reprojection and P's results equal M's (checked on the last
frame).  Their frames are interleaved, and which of the two goes first
alternates from frame to frame: the second one finds the frame's input planes
warm in the caches.  K1 / K2 means over frames 5.. from libbmfr's profiling
events (bmfr_set_profiling: K1 and K2 as two launches)."""
import argparse
import os
import sys

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
import torch  # noqa: E402

import bmfr_amd  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("size", nargs="*", type=int, default=[3840, 2160])
ap.add_argument("--frames", type=int, default=45)
ap.add_argument("--fast-fit", action="store_true")
ap.add_argument("--third-order", action="store_true")
ap.add_argument("--half-tmp", type=int, default=1)
a = ap.parse_args()
W, H = a.size
cfg = bmfr_amd.BmfrConfig(image_width=W, image_height=H, fast_fit=int(a.fast_fit),
                          use_half_precision_in_tmp_data=a.half_tmp,
                          scaled=bmfr_amd.SCALED_THIRD_ORDER if a.third_order else bmfr_amd.SCALED_DEFAULT)
n = W * H
nan_vp = [float("nan")] * 16


def inputs(f):
    fr = bmfr_amd.synth_frame_device(W, H, f)
    vp, _ = bmfr_amd.synth_camera(W, H, max(f - 1, 0))
    _, jit = bmfr_amd.synth_camera(W, H, f)
    return (fr["noisy"], fr["normals"], fr["positions"], fr["albedo"]), vp, jit


rec = bmfr_amd.Denoiser(cfg)
planes = []
for f in range(a.frames):
    args, vp, jit = inputs(f)
    rec.process_frame(*args, vp, jit, f)
    planes.append(rec.copy_state("prev_frame_pixel", torch.empty(2 * n, device="cuda")))
torch.cuda.synchronize()
rec.close()
A, B = bmfr_amd.Denoiser(cfg), bmfr_amd.Denoiser(cfg)
for d in (A, B):
    d.set_profiling(True, a.frames)
for f in range(a.frames):
    args, vp, jit = inputs(f)
    runs = [lambda: A.process_frame(*args, vp, jit, f),
            lambda: B.process_frame(*args, nan_vp, jit, f, prev_pixel=planes[f] if f > 0 else None)]
    for run in (runs if f % 2 == 0 else runs[::-1]):
        run()
    torch.cuda.synchronize()
same = torch.equal(A.copy_output(torch.empty(3 * n, device="cuda")).view(torch.int32),
                   B.copy_output(torch.empty(3 * n, device="cuda")).view(torch.int32))
for name, d in (("matrix", A), ("plane", B)):
    rows = [r for r in d.profile() if r[0] >= 5]
    k1 = sorted(r[1] for r in rows)
    k2 = sorted(r[2] for r in rows)
    print(f"{W}x{H} B={cfg.buffer_count} half_tmp={a.half_tmp} fast_fit={int(a.fast_fit)} {name:6s}: "
          f"K1 mean {sum(k1) / len(k1):.4f} median {k1[len(k1) // 2]:.4f} min {k1[0]:.4f} ms, "
          f"K2 mean {sum(k2) / len(k2):.4f} ms ({len(rows)} frames)")
print("outputs equal:", same)
sys.exit(0 if same else 1)
