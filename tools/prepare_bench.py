#!/usr/bin/env python3
"""Cost of the G-buffer front end (bmfr_prepare_frame) against a device copy of
the same bytes, on the GPU.

  python tools/prepare_bench.py [W H] [--config engine|reference|both] [--rounds N] [--launches N] [--out FILE]

Two configurations (every output requested in both):
  engine     radiance F16X4, albedo UNORM8X4, octahedral normals, depth, F16X2
             motion, ids and one transform table, half3 planes (input_half)
  reference  F32X3 everywhere, positions given, F32X2 motion, ids and a table,
             float3 planes
The yardstick is hipMemcpyAsync device-to-device of half the bytes the
configuration reads plus writes, so that it moves (reads + writes) the same
number; the byte count comes from the shapes (bytes_per_pixel below).  Input
sets are rotated (--sets, default 3) so that the data touched between two uses
of a line is far beyond the 256 MiB Infinity Cache.  After a warm-up, rounds
alternate: `launches` prepare calls between two device events, then `launches`
copies between two device events (default 10 x 25 = 250 timed launches each).
Run one process at a time, under a time limit."""
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
ap.add_argument("--config", default="both", choices=["engine", "reference", "both"])
ap.add_argument("--rounds", type=int, default=10)
ap.add_argument("--launches", type=int, default=25)
ap.add_argument("--sets", type=int, default=3)
ap.add_argument("--objects", type=int, default=64)
ap.add_argument("--out", default="")
a = ap.parse_args()
W, H = a.size
n = W * H
dev = torch.device("cuda", 0)

# plane -> (dtype, elements per pixel) per configuration; outputs follow from the context's input format
CONFIGS = {
    "engine": dict(half=1, planes={"radiance": (torch.float16, 4), "albedo": (torch.uint8, 4),
                                   "normals": (torch.int16, 2), "depth": (torch.float32, 1),
                                   "motion": (torch.float16, 2), "prev_positions": (torch.float16, 3),
                                   "prev_normals": (torch.float16, 3), "prev_object_id": (torch.int16, 1)}),
    "reference": dict(half=0, planes={"radiance": (torch.float32, 3), "albedo": (torch.float32, 3),
                                      "normals": (torch.float32, 3), "positions": (torch.float32, 3),
                                      "motion": (torch.float32, 2), "prev_positions": (torch.float32, 3),
                                      "prev_normals": (torch.float32, 3), "prev_object_id": (torch.int16, 1)}),
}


def bytes_per_pixel(c):
    size = lambda dt: torch.empty(0, dtype=dt).element_size()  # noqa: E731
    read = sum(size(dt) * per for dt, per in c["planes"].values())
    plane = 3 * (2 if c["half"] else 4)
    written = 6 * plane + 8   # noisy, normals, positions, albedo, two moved planes; prev_pixel
    return read, written


def plane(dt, count):
    if dt == torch.uint8:
        return torch.randint(0, 256, (count,), dtype=torch.uint8, device=dev)
    if dt == torch.int16:
        return torch.randint(-32767, 32768, (count,), dtype=torch.int32, device=dev).to(torch.int16)
    return torch.rand(count, dtype=torch.float32, device=dev).add_(0.25).to(dt)


def bench(name):
    c = CONFIGS[name]
    den = bmfr_amd.Denoiser(bmfr_amd.BmfrConfig(image_width=W, image_height=H, input_half=c["half"]))
    vp, jit = bmfr_amd.synth_camera(W, H, 1)
    sets = []
    for _ in range(a.sets):
        g = {k: plane(dt, n * per) for k, (dt, per) in c["planes"].items()}
        g["prev_object_id"] = torch.randint(0, a.objects + 2, (n,), dtype=torch.int32, device=dev).to(torch.int16)
        g["object_transforms"] = torch.rand(a.objects * 12, device=dev)
        g["inv_view_proj"] = vp  # any well-conditioned matrix: the arithmetic does not depend on the values
        sets.append(g)
    out = den.prepare(sets[0], jit)
    assert len(out) == 7, sorted(out)
    read, written = bytes_per_pixel(c)
    total = (read + written) * n
    copy_bytes = total // 2
    src = [torch.empty(copy_bytes, dtype=torch.uint8, device=dev).random_() for _ in range(a.sets)]
    dst = torch.empty(copy_bytes, dtype=torch.uint8, device=dev)

    # the checked ctypes arguments once per set: the timed loop is the library call alone
    calls = [den.prepare_args(g, out)[:2] for g in sets]
    off = (C.c_float * 2)(*jit)
    stream = torch.cuda.current_stream().cuda_stream

    def run_prepare(i):
        gb, pr = calls[i % a.sets]
        st = den.lib.bmfr_prepare_frame(den.handle, stream, C.byref(gb), C.byref(pr), off)
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

    for fn in (run_prepare, run_copy):   # warm-up
        timed(fn)
    tp, tc = [], []
    for _ in range(a.rounds):
        tp.append(timed(run_prepare))
        tc.append(timed(run_copy))
    med = lambda v: sorted(v)[len(v) // 2]  # noqa: E731
    mp, mc = med(tp), med(tc)
    lines = [
        f"{name}: {W}x{H}, {read} B/px read + {written} B/px written = {total / 1e6:.1f} MB per call, "
        f"{a.sets} input sets rotated, {a.rounds} rounds x {a.launches} launches, alternating",
        f"  prepare  median {mp:.4f} ms (min {min(tp):.4f}, max {max(tp):.4f})  {total / mp / 1e9:.3f} TB/s",
        f"  copy     median {mc:.4f} ms (min {min(tc):.4f}, max {max(tc):.4f})  {total / mc / 1e9:.3f} TB/s "
        f"(hipMemcpyAsync D2D of {copy_bytes / 1e6:.1f} MB: the same bytes read + written)",
        f"  ratio prepare / copy = {mp / mc:.3f} (bar: 1.25)",
    ]
    den.close()
    return lines


lines = []
for name in (["engine", "reference"] if a.config == "both" else [a.config]):
    lines += bench(name)
text = "\n".join(lines)
print(text)
if a.out:
    with open(a.out, "w") as f:
        f.write(text + "\n")
