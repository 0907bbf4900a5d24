#!/usr/bin/env python3
"""Cost of guided upsampling (bmfr_upsample_output) against a device copy of
the same compulsory bytes, on the GPU.

  python tools/upsample_bench.py [W H Wd Hd] [--rounds N] [--launches N] [--sets N] [--out FILE]

Four configurations (default 1920 x 1080 -> 3840 x 2160); bytes per DISPLAY
pixel of guides read and surface written, per FRAME pixel of low-resolution
planes (filtered_accumulated, and in guided mode the frame's normals and
positions) read once:
  engine_f16x4     UNORM8X4 albedo, octahedral normals, depth -> F16X4, HDR          12 + 8, 36
  engine_unorm8x4  the same guides -> UNORM8X4, tone-mapped                          12 + 4, 36
  f32_guided       F32X3 albedo, normals, positions -> F32X3, HDR                    36 + 12, 36
  unguided         UNORM8X4 albedo -> F16X4, HDR                                      4 + 8, 12
The yardstick is hipMemcpyAsync device-to-device of half those bytes, so that
it moves (reads + writes) the same number; the byte count comes from the
shapes.  The kernel reads each tap pixel for up to 4 s^2 display pixels: what
it fetches beyond the compulsory bytes is served by the caches or shows in the
ratio.  Buffer sets are rotated by rotating CONTEXTS (--sets, default 4, each
with its own guides and surface): between two uses of a line the data touched
is beyond the 256 MiB Infinity Cache.  After a warm-up, rounds alternate:
`launches` calls between two device events, then `launches` copies between two
device events (default 10 x 24 timed launches each).  Run one process at a
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
ap.add_argument("size", nargs="*", type=int, default=[1920, 1080, 3840, 2160])
ap.add_argument("--rounds", type=int, default=10)
ap.add_argument("--launches", type=int, default=24)
ap.add_argument("--sets", type=int, default=4)
ap.add_argument("--out", default="")
a = ap.parse_args()
W, H, Wd, Hd = a.size
n, nd = W * H, Wd * Hd
dev = torch.device("cuda", 0)

# name -> (guide formats, guided, surface dtype, channels, source, guide B/px, surface B/px, low-resolution B/px)
CONFIGS = {
    "engine_f16x4": ("engine", True, torch.float16, 4, "hdr", 12, 8, 36),
    "engine_unorm8x4": ("engine", True, torch.uint8, 4, "tonemapped", 12, 4, 36),
    "f32_guided": ("f32", True, torch.float32, 3, "hdr", 36, 12, 36),
    "unguided": ("engine", False, torch.float16, 4, "hdr", 4, 8, 12),
}


def oct_encode(nrm):
    """Unit vectors (n, 3) -> octahedral snorm16 x 2, on the device."""
    v = nrm.double()
    p = v[:, :2] / v.abs().sum(dim=1, keepdim=True)
    folded = (1.0 - p.flip(1).abs()) * torch.where(p >= 0, 1.0, -1.0)
    p = torch.where(v[:, 2:3] < 0, folded, p)
    return torch.round(p * 32767.0).to(torch.int16).reshape(-1)


def display_guides(formats, guided):
    """The synthetic scene at display resolution as a renderer's G-buffer."""
    fr = bmfr_amd.synth_frame_device(Wd, Hd, 0)
    vp, jit = bmfr_amd.synth_camera(Wd, Hd, 0)
    alb, nrm, pos = (fr[k].reshape(nd, 3) for k in ("albedo", "normals", "positions"))
    g = {"width": Wd, "height": Hd}
    if formats == "f32":
        g["albedo"] = alb.reshape(-1)
        if guided:
            g["normals"], g["positions"] = nrm.reshape(-1), pos.reshape(-1)
        return g
    q = torch.round(alb.clamp(0, 1) * 255).to(torch.uint8)
    g["albedo"] = torch.cat([q, torch.full((nd, 1), 255, dtype=torch.uint8, device=dev)], dim=1).reshape(-1)
    if guided:
        g["normals"] = oct_encode(nrm)
        M = torch.tensor(vp, dtype=torch.float64, device=dev).reshape(4, 4).T   # column-major -> rows
        clip = torch.cat([pos.double(), torch.ones((nd, 1), dtype=torch.float64, device=dev)], dim=1) @ M.T
        g["depth"] = (clip[:, 2] / clip[:, 3]).float()
        g["inv_view_proj"] = torch.linalg.inv(M).T.reshape(-1).float().tolist()
        g["pixel_offset"] = jit
    return g


def bench(name):
    formats, guided, dt, ch, source, gbytes, sbytes, lbytes = CONFIGS[name]
    vp, jit = bmfr_amd.synth_camera(W, H, 0)
    calls, keep = [], []
    fell = None
    for k in range(a.sets):
        den = bmfr_amd.Denoiser(bmfr_amd.BmfrConfig(image_width=W, image_height=H))
        fr = bmfr_amd.synth_frame_device(W, H, 0)
        den.process_frame(fr["noisy"], fr["normals"], fr["positions"], fr["albedo"], vp, jit, 0)
        dst = torch.empty((Hd, Wd, ch), dtype=dt, device=dev)
        g = display_guides(formats, guided)
        nrm, pos = (fr["normals"], fr["positions"]) if guided else (None, None)
        if k == 0 and guided:   # the share of fallback pixels, once, outside the timed loop
            stats = torch.zeros(1, dtype=torch.int32, device=dev)
            den.upsample(dst, g, nrm, pos, source=source, stats=stats)
            fell = int(stats.item())
        # the checked ctypes arguments once per set: the timed loop is the library call alone
        calls.append((den, den.upsample_args(dst, g, nrm, pos, source=source), nrm, pos))
        keep.append((dst, g, fr))
    torch.cuda.synchronize()
    total = (gbytes + sbytes) * nd + lbytes * n
    copy_bytes = total // 2
    src = [torch.empty(copy_bytes, dtype=torch.uint8, device=dev).random_() for _ in range(a.sets)]
    dst = torch.empty(copy_bytes, dtype=torch.uint8, device=dev)
    stream = torch.cuda.current_stream().cuda_stream

    def run_upsample(i):
        den, (s, gs, surf), nrm, pos = calls[i % a.sets]
        st = den.lib.bmfr_upsample_output(den.handle, stream, s, nrm.data_ptr() if guided else None,
                                          pos.data_ptr() if guided else None, C.byref(gs), C.byref(surf), None)
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

    for fn in (run_upsample, run_copy):   # warm-up
        timed(fn)
    tu, tc = [], []
    for _ in range(a.rounds):
        tu.append(timed(run_upsample))
        tc.append(timed(run_copy))
    med = lambda v: sorted(v)[len(v) // 2]  # noqa: E731
    mu, mc = med(tu), med(tc)
    lines = [
        f"{name}: {W}x{H} -> {Wd}x{Hd}, {gbytes} + {sbytes} B per display pixel, {lbytes} B per frame pixel = "
        f"{total / 1e6:.1f} MB compulsory per call, {a.sets} contexts rotated, {a.rounds} rounds x {a.launches} "
        f"launches, alternating" + (f", {100.0 * fell / nd:.3f} % fallback pixels" if fell is not None else ""),
        f"  upsample median {mu:.4f} ms (min {min(tu):.4f}, max {max(tu):.4f})  {total / mu / 1e9:.3f} TB/s compulsory",
        f"  copy     median {mc:.4f} ms (min {min(tc):.4f}, max {max(tc):.4f})  {total / mc / 1e9:.3f} TB/s "
        f"(hipMemcpyAsync D2D of {copy_bytes / 1e6:.1f} MB: the same bytes read + written)",
        f"  ratio upsample / copy = {mu / mc:.3f}",
    ]
    for den, *_ in calls:
        assert den.frame_status() == 0
        den.close()
    return lines


lines = []
for name in CONFIGS:
    lines += bench(name)
text = "\n".join(lines)
print(text)
if a.out:
    with open(a.out, "w") as f:
        f.write(text + "\n")
