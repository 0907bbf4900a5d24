#!/usr/bin/env python3
"""Cost of the firefly pre-filter (bmfr_suppress_fireflies) against a device
copy of the same bytes, on the GPU.

  python tools/firefly_bench.py [W H] [--rounds N] [--launches N] [--sets N] [--out FILE]

Four cases: float3 and half3 planes (input_half), radius 1 and 2, threshold 2.
The yardstick is hipMemcpyAsync device-to-device of one plane: it reads and
writes what the filter must, 24 B/px for float3 and 12 B/px for half3 (the
ring a work-group re-reads is meant to hit in L2 and is not counted).  Input
planes hold noise with x50 pixels at a 1.5e-4 share and are rotated (--sets,
default 12) so that the data touched between two uses of a line is beyond the
256 MiB Infinity Cache.  After a warm-up, rounds alternate: `launches` filter
calls between two device events, then `launches` copies between two device
events (default 10 x 25 = 250 timed launches each); the filter is timed with the
two counters (stats) and without (stats = NULL: no atomics).  Run one process at a
time, under a time limit."""
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
ap.add_argument("--launches", type=int, default=25)
ap.add_argument("--sets", type=int, default=12)
ap.add_argument("--out", default="")
a = ap.parse_args()
W, H = a.size
n = W * H
dev = torch.device("cuda", 0)


def bench(half: int, radius: int):
    dt = torch.float16 if half else torch.float32
    den = bmfr_amd.Denoiser(bmfr_amd.BmfrConfig(image_width=W, image_height=H, input_half=half))
    sets = []
    for _ in range(a.sets):
        p = torch.rand(n, 3, device=dev).square_().mul_(3.0)
        p[torch.rand(n, device=dev) < 1.5e-4] *= 50.0
        sets.append(p.to(dt).reshape(-1))
    out = torch.empty_like(sets[0])
    dst = torch.empty_like(sets[0])
    plane_bytes = sets[0].numel() * sets[0].element_size()
    total = 2 * plane_bytes
    stats = torch.zeros(2, dtype=torch.int32, device=dev)
    _, params = den.firefly_args(sets[0], out, threshold=2.0, radius=radius, stats=stats)
    stream = torch.cuda.current_stream().cuda_stream

    def run_filter(i, stats_ptr=stats.data_ptr()):
        st = den.lib.bmfr_suppress_fireflies(den.handle, stream, sets[i % a.sets].data_ptr(), out.data_ptr(),
                                             C.byref(params), stats_ptr)
        assert st == 0, st

    def run_filter_no_stats(i):
        run_filter(i, None)

    def run_copy(i):
        hip_memcpy_d2d(dst.data_ptr(), sets[i % a.sets].data_ptr(), plane_bytes)

    def timed(fn):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for i in range(a.launches):
            fn(i)
        e1.record()
        e1.synchronize()
        return e0.elapsed_time(e1) / a.launches   # ms per launch

    for fn in (run_filter, run_filter_no_stats, run_copy):   # warm-up
        timed(fn)
    stats.zero_()
    run_filter(0)
    torch.cuda.synchronize()
    clamped = stats.cpu().tolist()[0]
    tf, tn, tc = [], [], []
    for _ in range(a.rounds):
        tf.append(timed(run_filter))
        tn.append(timed(run_filter_no_stats))
        tc.append(timed(run_copy))
    med = lambda v: sorted(v)[len(v) // 2]  # noqa: E731
    mf, mn, mc = med(tf), med(tn), med(tc)
    name = f"{'half3' if half else 'float3'} radius {radius}"
    lines = [
        f"{name}: {W}x{H}, {total // n} B/px read + written = {total / 1e6:.1f} MB per call, {a.sets} input planes "
        f"rotated, {a.rounds} rounds x {a.launches} launches, alternating; {100.0 * clamped / n:.2f} % of pixels clamped",
        f"  filter   median {mf:.4f} ms (min {min(tf):.4f}, max {max(tf):.4f})  {total / mf / 1e9:.3f} TB/s (with stats)",
        f"  filter   median {mn:.4f} ms (min {min(tn):.4f}, max {max(tn):.4f})  {total / mn / 1e9:.3f} TB/s (stats = NULL)",
        f"  copy     median {mc:.4f} ms (min {min(tc):.4f}, max {max(tc):.4f})  {total / mc / 1e9:.3f} TB/s "
        f"(hipMemcpyAsync D2D of {plane_bytes / 1e6:.1f} MB)",
        f"  ratio filter / copy = {mf / mc:.3f} with stats, {mn / mc:.3f} without",
    ]
    den.close()
    return lines


lines = []
for half in (0, 1):
    for radius in (1, 2):
        lines += bench(half, radius)
text = "\n".join(lines)
print(text)
if a.out:
    with open(a.out, "w") as f:
        f.write(text + "\n")
