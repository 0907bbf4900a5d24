#!/usr/bin/env python3
"""Cost of the output back end (bmfr_resolve_output) against a device copy of
the same bytes, on the GPU.

  python tools/resolve_bench.py [W H] [--rounds N] [--launches N] [--sets N] [--out FILE]

Four configurations (default 3840 x 2160):
  output_unorm8x4   OUTPUT -> UNORM8X4        12 B/px read,  4 B/px written
  output_f16x4      OUTPUT -> F16X4           12 B/px read,  8 B/px written
  hdr_f16x4         HDR -> F16X4, f32 albedo  24 B/px read,  8 B/px written
  hdr_f16x4_half    HDR -> F16X4, half3 albedo (input_half)  18 B/px read, 8 B/px written
The yardstick is hipMemcpyAsync device-to-device of half the bytes the
configuration reads plus writes, so that it moves (reads + writes) the same
number; the byte count comes from the shapes.  The state plane a call reads is
the context's own, so buffer sets are rotated by rotating CONTEXTS (--sets,
default 6, each with its own albedo plane and surface): between two uses of a
line the data touched is far beyond the 256 MiB Infinity Cache.  After a
warm-up, rounds alternate: `launches` resolve calls between two device events,
then `launches` copies between two device events (default 10 x 24 timed
launches each).  Run one process at a time, under a time limit."""
import argparse
import ctypes as C
import os
import sys

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
import torch  # noqa: E402

import bmfr_amd  # noqa: E402
from bmfr_amd.pipeline import hip_memcpy_d2d  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("size", nargs="*", type=int, default=[3840, 2160])
ap.add_argument("--rounds", type=int, default=10)
ap.add_argument("--launches", type=int, default=24)
ap.add_argument("--sets", type=int, default=6)
ap.add_argument("--out", default="")
a = ap.parse_args()
W, H = a.size
n = W * H
dev = torch.device("cuda", 0)

# name -> (source, surface dtype, channels, input_half, bytes per pixel read, written)
CONFIGS = {
    "output_unorm8x4": ("output", torch.uint8, 4, 0, 12, 4),
    "output_f16x4": ("output", torch.float16, 4, 0, 12, 8),
    "hdr_f16x4": ("hdr", torch.float16, 4, 0, 24, 8),
    "hdr_f16x4_half": ("hdr", torch.float16, 4, 1, 18, 8),
}


def bench(name):
    source, dt, ch, half, read, written = CONFIGS[name]
    vp, jit = bmfr_amd.synth_camera(W, H, 0)
    calls, keep = [], []
    for _ in range(a.sets):
        den = bmfr_amd.Denoiser(bmfr_amd.BmfrConfig(image_width=W, image_height=H, input_half=half))
        fr = bmfr_amd.synth_frame_device(W, H, 0)
        if half:
            fr = {k: v.to(torch.float16) for k, v in fr.items()}
        den.process_frame(fr["noisy"], fr["normals"], fr["positions"], fr["albedo"], vp, jit, 0)
        dst = torch.empty((H, W, ch), dtype=dt, device=dev)
        albedo = fr["albedo"] if source == "hdr" else None
        # the checked ctypes arguments once per set: the timed loop is the library call alone
        calls.append((den, den.resolve_args(dst, source=source, albedo=albedo)))
        keep.append((dst, albedo))
    torch.cuda.synchronize()
    total = (read + written) * n
    copy_bytes = total // 2
    src = [torch.empty(copy_bytes, dtype=torch.uint8, device=dev).random_() for _ in range(a.sets)]
    dst = torch.empty(copy_bytes, dtype=torch.uint8, device=dev)
    stream = torch.cuda.current_stream().cuda_stream

    def run_resolve(i):
        den, (s, alb, surf) = calls[i % a.sets]
        st = den.lib.bmfr_resolve_output(den.handle, stream, s, alb, C.byref(surf))
        assert st == 0, st

    def run_copy(i):
        hip_memcpy_d2d(dst.data_ptr(), src[i % a.sets].data_ptr(), copy_bytes)

    def timed(fn):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for i in range(a.launches):
            fn(i)
        e1.record()
        e1.synchronize()
        return e0.elapsed_time(e1) / a.launches   # ms per launch

    for fn in (run_resolve, run_copy):   # warm-up
        timed(fn)
    tr, tc = [], []
    for _ in range(a.rounds):
        tr.append(timed(run_resolve))
        tc.append(timed(run_copy))
    med = lambda v: sorted(v)[len(v) // 2]  # noqa: E731
    mr, mc = med(tr), med(tc)
    lines = [
        f"{name}: {W}x{H}, {read} B/px read + {written} B/px written = {total / 1e6:.1f} MB per call, "
        f"{a.sets} contexts rotated, {a.rounds} rounds x {a.launches} launches, alternating",
        f"  resolve  median {mr:.4f} ms (min {min(tr):.4f}, max {max(tr):.4f})  {total / mr / 1e9:.3f} TB/s",
        f"  copy     median {mc:.4f} ms (min {min(tc):.4f}, max {max(tc):.4f})  {total / mc / 1e9:.3f} TB/s "
        f"(hipMemcpyAsync D2D of {copy_bytes / 1e6:.1f} MB: the same bytes read + written)",
        f"  ratio resolve / copy = {mr / mc:.3f}",
    ]
    for den, _ in calls:
        assert den.frame_status() == 0
        den.close()
    return lines


lines = []
for name in CONFIGS:
    lines += bench(name)
lines.append(f"bmfr_host readback per frame at {W}x{H}: {12 * n / 1e6:.1f} MB (12 B/px) by default, "
             f"{3 * n / 1e6:.1f} MB (3 B/px) with --device-quantize, by construction; wall time not measured")
text = "\n".join(lines)
print(text)
if a.out:
    with open(a.out, "w") as f:
        f.write(text + "\n")
