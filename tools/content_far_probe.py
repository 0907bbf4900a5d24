#!/usr/bin/env python3
"""Where fast_fit departs from the exact path on a flat wall far from the origin.

tests/test_gpu_content_parity.py holds fast_fit's worst 32x32 tile to 4 x the
reference's own build-to-build worst tile; the `far` scene (tests/scenes_np.py:
one flat wall, every coordinate near 16) misses that at B = 16 with half
tmp_data, in the 4-pixel-wide tiles at the right edge of the 100x72 frame.
This probe prints the per-tile relative L2 of fast_fit against the exact path
(which equals the reference's strict build bit for bit, so no reference build
is needed and any size can be run) for

  * widths that are / are not a multiple of 32 (a narrow edge tile shows a
    single block; a full tile averages up to four),
  * the same wall moved 8 and 15 units towards the origin (positions and the
    camera matrix shifted together: the same image, smaller coordinates),
  * B = 13 (no cubes),

and, as a measure of the blocks' conditioning that does not involve fast_fit,
the exact path against itself with every noisy input value moved one f32 ulp
up (a relative change of at most 1.2e-7).

Run on a GPU from the repository root: python tools/content_far_probe.py
(output of one run: profiles/content_far_probe.txt).
"""
from __future__ import annotations

import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "oracle"), os.path.join(ROOT, "tests")):
    sys.path.insert(0, p)

import numpy as np  # noqa: E402
import torch  # noqa: E402

import bmfr_amd  # noqa: E402
import scenes_np  # noqa: E402

PLANES = ("noisy", "normals", "positions", "albedo")


def run(W, H, scaled, fast_fit, shift, frames=4, ulp=False):
    den = bmfr_amd.Denoiser(bmfr_amd.BmfrConfig(image_width=W, image_height=H, scaled=scaled, fast_fit=fast_fit,
                                                library_powr=1))
    out = []
    for f in range(frames):
        fr = scenes_np.frame("far", W, H, f, 2)
        pos = (fr["positions"].reshape(-1, 3) - np.float32(shift)).astype(np.float32).reshape(-1)
        m = list(fr["prev_vp"])  # M' = M T(+shift): the shifted positions reproject as the original ones did
        for r in range(4):
            m[12 + r] = float(np.float32(m[12 + r] + shift * (m[r] + m[4 + r] + m[8 + r])))
        t = {k: torch.from_numpy(np.array(pos if k == "positions" else fr[k])).cuda() for k in PLANES}
        if ulp:
            t["noisy"] = torch.nextafter(t["noisy"], torch.full_like(t["noisy"], float("inf")))
        den.process_frame(t["noisy"], t["normals"], t["positions"], t["albedo"], m, fr["jitter"], f)
        out.append(den.copy_output(torch.empty(3 * W * H, device="cuda")).cpu().numpy().reshape(H, W, 3))
    return out


def tiles(label, got, want, W, H):
    for f in (0, 3):
        d, b = got[f].astype(np.float64) - want[f], want[f].astype(np.float64)
        print(f"{label} frame {f} frame rel-L2 {np.linalg.norm(d) / np.linalg.norm(b):.2e}", flush=True)
        for ty in range(0, H, 32):
            print("   ", " ".join("%.1e" % (np.linalg.norm(d[ty:ty + 32, tx:tx + 32]) /
                                            np.linalg.norm(b[ty:ty + 32, tx:tx + 32])) for tx in range(0, W, 32)))


def main():
    third = bmfr_amd.SCALED_THIRD_ORDER
    for W, H, scaled, shift, label in [(100, 72, third, 0.0, "B16 100x72"), (128, 96, third, 0.0, "B16 128x96"),
                                       (200, 136, third, 0.0, "B16 200x136"),
                                       (100, 72, third, 8.0, "B16 100x72 coords-8"),
                                       (100, 72, third, 15.0, "B16 100x72 coords-15"),
                                       (100, 72, bmfr_amd.SCALED_DEFAULT, 0.0, "B13 100x72")]:
        fast, exact = run(W, H, scaled, 1, shift), run(W, H, scaled, 0, shift)
        tiles(label + ": fast_fit vs exact,", fast, exact, W, H)
        tiles(label + ": exact, noisy + 1 ulp vs exact,", run(W, H, scaled, 0, shift, ulp=True), exact, W, H)


if __name__ == "__main__":
    main()
