#!/usr/bin/env python3
"""Cost of the display-resolution TAA (bmfr_display_taa) against a device copy
of the same compulsory bytes, on the GPU.

  python tools/display_taa_bench.py [Wd Hd] [--rounds N] [--launches N] [--sets N] [--out FILE]

Four configurations (default 3840 x 2160); compulsory bytes per display pixel --
`current`, the previous position and `history` read once, `result` and `dst`
written once:
  engine         F16X4 planes, F16X2 motion, UNORM8X4 dst      8 + 4 + 8 + 8 + 4 = 32
  engine_no_dst  the same without dst                          8 + 4 + 8 + 8     = 28
  f32            F32X3 planes, prev_pixel, F32X3 dst           12 + 8 + 12 + 12 + 12 = 56
  engine_reset   engine formats with reset = 1                 8 + 8 + 4         = 20
The yardstick is hipMemcpyAsync device-to-device of half those bytes, so that
it moves (reads + writes) the same number; the byte count comes from the
shapes.  The kernel reads each pixel of `current` for up to nine display pixels
and each history pixel for about four: what it fetches beyond the compulsory
bytes is served by the caches or shows in the ratio.  Plane sets are rotated
(--sets, default 6, each with its own planes, motion and surface): between two
uses of a line the data touched is beyond the 256 MiB Infinity Cache.  The
motion is a seeded field of a few pixels, so the history taps scatter as a
camera move scatters them.  After a warm-up, rounds alternate: `launches` calls
between two device events, then `launches` copies between two device events
(default 10 x 24 timed launches each).  Run one process at a time, under a
time limit.  The committed figures are `--out profiles/display_taa_bench.txt`
with the defaults."""
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
Wd, Hd = a.size
nd = Wd * Hd
dev = torch.device("cuda", 0)

# name -> (plane dtype, channels, previous position, dst (dtype, channels) or None, reset, compulsory B/px)
CONFIGS = {
    "engine": (torch.float16, 4, "motion_f16", (torch.uint8, 4), False, 8 + 4 + 8 + 8 + 4),
    "engine_no_dst": (torch.float16, 4, "motion_f16", None, False, 8 + 4 + 8 + 8),
    "f32": (torch.float32, 3, "prev_pixel", (torch.float32, 3), False, 12 + 8 + 12 + 12 + 12),
    "engine_reset": (torch.float16, 4, "motion_f16", (torch.uint8, 4), True, 8 + 8 + 4),
}


def colour(dt, ch, seed):
    g = torch.Generator(device=dev).manual_seed(seed)
    return torch.rand((Hd, Wd, ch), generator=g, device=dev, dtype=torch.float32).to(dt)


def bench(name, den):
    dt, ch, where, surface, reset, bpp = CONFIGS[name]
    calls, keep = [], []
    for k in range(a.sets):
        cur, hist, res = colour(dt, ch, 3 * k), colour(dt, ch, 3 * k + 1), torch.empty((Hd, Wd, ch), dtype=dt, device=dev)
        g = torch.Generator(device=dev).manual_seed(1000 + k)
        mv = (torch.rand(nd * 2, generator=g, device=dev) - 0.5) * 6.0          # +- 3 pixels
        kw = {}
        if where == "prev_pixel":
            ys, xs = torch.meshgrid(torch.arange(Hd, device=dev), torch.arange(Wd, device=dev), indexing="ij")
            kw["prev_pixel"] = (torch.stack([xs, ys], dim=-1).reshape(-1).float() - mv).contiguous()
        else:
            kw["motion"] = mv.to(torch.float16)
        dst = None if surface is None else torch.empty((Hd, Wd, surface[1]), dtype=surface[0], device=dev)
        # the checked ctypes arguments once per set: the timed loop is the library call alone
        calls.append(den.display_taa_args(cur, res, history=hist, dst=dst, reset=reset, **kw))
        keep.append((cur, hist, res, kw, dst))
    torch.cuda.synchronize()
    total = bpp * nd
    copy_bytes = total // 2
    src = [torch.empty(copy_bytes, dtype=torch.uint8, device=dev).random_() for _ in range(a.sets)]
    out = torch.empty(copy_bytes, dtype=torch.uint8, device=dev)
    stream = torch.cuda.current_stream().cuda_stream

    def run_taa(i):
        args, surf = calls[i % a.sets]
        st = den.lib.bmfr_display_taa(den.handle, stream, C.byref(args), C.byref(surf) if surf is not None else None)
        assert st == 0, st

    def run_copy(i):
        hip_memcpy_d2d(out.data_ptr(), src[i % a.sets].data_ptr(), copy_bytes)

    def timed(fn):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for i in range(a.launches):
            fn(i)
        e1.record()
        e1.synchronize()
        return e0.elapsed_time(e1) / a.launches   # ms per launch

    for fn in (run_taa, run_copy):   # warm-up
        timed(fn)
    tt, tc = [], []
    for _ in range(a.rounds):
        tt.append(timed(run_taa))
        tc.append(timed(run_copy))
    med = lambda v: sorted(v)[len(v) // 2]  # noqa: E731
    mt, mc = med(tt), med(tc)
    return [
        f"{name}: {Wd}x{Hd}, {bpp} B per display pixel = {total / 1e6:.1f} MB compulsory per call, {a.sets} plane sets "
        f"rotated, {a.rounds} rounds x {a.launches} launches, alternating",
        f"  display_taa median {mt:.4f} ms (min {min(tt):.4f}, max {max(tt):.4f})  {total / mt / 1e9:.3f} TB/s compulsory",
        f"  copy        median {mc:.4f} ms (min {min(tc):.4f}, max {max(tc):.4f})  {total / mc / 1e9:.3f} TB/s "
        f"(hipMemcpyAsync D2D of {copy_bytes / 1e6:.1f} MB: the same bytes read + written)",
        f"  ratio display_taa / copy = {mt / mc:.3f}",
    ]


den = bmfr_amd.Denoiser(bmfr_amd.BmfrConfig(image_width=32, image_height=32))   # the context only names the device
lines = []
for name in CONFIGS:
    lines += bench(name, den)
assert den.frame_status() == 0
den.close()
text = "\n".join(lines)
print(text)
if a.out:
    with open(a.out, "w") as f:
        f.write(text + "\n")
