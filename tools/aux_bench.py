#!/usr/bin/env python3
"""Cost of caller-supplied feature planes (BMFR_FEATURE_AUX0..3) in the
generic-feature K1, on the GPU.

  python tools/aux_bench.py [W H] [--cases a,b,c] [--rounds N] [--frames N] [--warmup N] [--out FILE]

Three feature lists of counts 4 + 6, half tmp_data (none canonical, so all run
the generic-feature path: K1, then the TAA kernel):
  a  named codes only: (1, nx, ny, nz)(px, py, pz, px^2, py^2, pz^3)
  b  the same list with pz^3 delivered as an aux plane
  c  the same list with nz, pz, py^2 and pz^3 delivered as aux planes
The planes hold the monomials' own f32 values, so all three compute the same
frames.  Content: the synthetic sequence, rendered on the device once, frames
0 .. warmup + frames - 1.  A round runs the sequence from frame 0 for each
case in turn (alternating, so drift hits all cases alike) and times frames
warmup .. between two device events: ms per frame of bmfr_process_frame.  The
figure per case is the median over the rounds; min and max give the
run-to-run spread a difference has to exceed.

An A/B library (BMFR_LIB=NAME, e.g. tools/ab.py build-rev NAME=REV of a
revision that predates the aux codes, with BMFR_ALLOW_FOREIGN_BUILD=1) can run
case a only: --cases a.  Run one process at a time, under a time limit."""
import argparse
import os
import sys

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
import torch  # noqa: E402

import bmfr_amd  # noqa: E402
from bmfr_amd import _lib  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("size", nargs="*", type=int, default=[3840, 2160])
ap.add_argument("--cases", default="a,b,c")
ap.add_argument("--rounds", type=int, default=5)
ap.add_argument("--frames", type=int, default=40, help="timed frames per round")
ap.add_argument("--warmup", type=int, default=4, help="untimed frames at the start of each round")
ap.add_argument("--out", default="")
a = ap.parse_args()
W, H = a.size
n = W * H

A0 = getattr(_lib, "FEATURE_AUX0", 13)
NAMED = ((0, 1, 2, 3), (4, 5, 6, 7, 8, 12))
# case -> (not_scaled, scaled, what each aux plane holds: (input plane, component, power))
CASES = {
    "a": (NAMED[0], NAMED[1], ()),
    "b": (NAMED[0], (4, 5, 6, 7, 8, A0), (("positions", 2, 3),)),
    "c": ((0, 1, 2, A0), (4, 5, A0 + 1, 7, A0 + 2, A0 + 3),
          (("normals", 2, 1), ("positions", 2, 1), ("positions", 1, 2), ("positions", 2, 3))),
}
cases = a.cases.split(",")
total = a.warmup + a.frames


def monomial(fr, plane, comp, power):
    v = fr[plane].reshape(n, 3)[:, comp]
    out = v
    for _ in range(power - 1):
        out = out * v   # (v * v) * v: one rounding per operation, as the named code
    return out.contiguous()


frames, cams = [], []
for f in range(total):
    frames.append(bmfr_amd.synth_frame_device(W, H, f))
    vp, _ = bmfr_amd.synth_camera(W, H, max(f - 1, 0))
    _, jit = bmfr_amd.synth_camera(W, H, f)
    cams.append((vp, jit))
need = {spec for c in cases for spec in CASES[c][2]}
planes = [{spec: monomial(fr, *spec) for spec in need} for fr in frames]
torch.cuda.synchronize()

dens = {c: bmfr_amd.Denoiser(bmfr_amd.BmfrConfig(image_width=W, image_height=H, not_scaled=CASES[c][0],
                                                 scaled=CASES[c][1])) for c in cases}


def run(c):
    """One pass over the sequence -> ms per frame of frames warmup .. ."""
    den, specs = dens[c], CASES[c][2]
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    for f in range(total):
        if f == a.warmup:
            e0.record()
        fr, (vp, jit) = frames[f], cams[f]
        kw = {"aux": [planes[f][s] for s in specs]} if specs else {}
        den.process_frame(fr["noisy"], fr["normals"], fr["positions"], fr["albedo"], vp, jit, f, **kw)
    e1.record()
    e1.synchronize()
    assert den.frame_status() == 0
    return e0.elapsed_time(e1) / a.frames


for c in cases:   # warm-up pass: code objects, allocations
    run(c)
times = {c: [] for c in cases}
for _ in range(a.rounds):
    for c in cases:
        times[c].append(run(c))
med = lambda v: sorted(v)[len(v) // 2]  # noqa: E731
lib = os.environ.get("BMFR_LIB") or "working tree"
lines = [f"aux_bench: {W}x{H}, half tmp_data, counts 4 + 6, library: {lib} (build id {bmfr_amd.build_id()[:16]}), "
         f"{a.rounds} rounds alternating, {a.frames} timed frames per round after {a.warmup} warm-up frames, "
         f"ms per frame (K1 + TAA) by device events"]
for c in cases:
    v = times[c]
    lines.append(f"  ({c}) {len(CASES[c][2])} aux planes  median {med(v):.4f} ms  min {min(v):.4f}  max {max(v):.4f}  "
                 f"spread {(max(v) - min(v)) / med(v) * 100:.2f} %")
if "a" in cases:
    for c in cases:
        if c != "a":
            lines.append(f"  ({c}) / (a) = {med(times[c]) / med(times['a']):.4f}")
text = "\n".join(lines)
print(text)
if a.out:
    with open(a.out, "a") as f:
        f.write(text + "\n")
