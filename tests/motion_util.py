"""Shared content for the prev_pixel (caller-supplied previous-frame pixel
plane) tests.  TEST INFRASTRUCTURE ONLY.

scene_frame: one frame of the library's synthetic scene ("synth") or of a
tests/scenes_np.py scene, as numpy planes + camera.

The moving-world construction (test 3 of test_gpu_motion_input.py): the
synthetic scene's positions quantised to multiples of 2^-8 (run X), and the
same world translated by f T at frame f (runs Y, Z).  |position| < 2^10 and
f T is a multiple of 2^-3 below 2^3, so every translated coordinate is a
multiple of 2^-8 below 2^11: 19 significant bits, exact in f32.  Subtracting
f T gives back the quantised plane bit for bit, and every previous - current
difference of the moved world equals the static world's."""
from __future__ import annotations

import numpy as np

import scenes_np

T = (0.25, -0.5, 0.125)   # the world's translation per frame
QUANTUM = 2.0 ** -8
# width, height and halo of the reach scenario: 40 px of motion against a 40 px halo on a 2 x 2 grid
# (tests/test_gpu_reach.py by matrix, tests/test_gpu_motion_input.py through planes)
REACH_SIZE = (320, 256, 40)


def shifted(vp, dx: float, width: int):
    """The column-major VP with clip x += (2 dx / width) w: every reprojection
    lands dx pixels further right (bmfr.cl:343-355)."""
    k = 2.0 * dx / width
    m = list(vp)
    for c in range(4):  # row 0 += k * row 3
        m[4 * c] += k * m[4 * c + 3]
    return m


def scene_frame(scene: str, W: int, H: int, f: int) -> dict:
    """noisy / normals / positions / albedo (flat f32, read-only), prev_vp
    (16 floats, the camera of frame max(f - 1, 0)) and jitter of frame f."""
    if scene != "synth":
        return scenes_np.frame(scene, W, H, f)
    import bmfr_amd
    fr = {k: v.reshape(-1) for k, v in bmfr_amd.synth_frame_host(W, H, f).items()}
    vp, _ = bmfr_amd.synth_camera(W, H, max(f - 1, 0))
    _, jit = bmfr_amd.synth_camera(W, H, f)
    fr["prev_vp"], fr["jitter"] = vp, jit
    return fr


def quantise(positions: np.ndarray) -> np.ndarray:
    """Positions rounded to multiples of 2^-8 (f32)."""
    q = np.rint(positions.astype(np.float64) / QUANTUM) * QUANTUM + 0.0  # (+ 0.0: no -0, which a round trip loses)
    out = q.astype(np.float32)
    assert (out.astype(np.float64) == q).all() and np.abs(q).max() < 1024.0
    return out


def translated(positions_q: np.ndarray, k: int) -> np.ndarray:
    """positions_q + k T in f32, with the exactness the tests rely on
    asserted: subtracting k T gives back positions_q bit for bit."""
    t = np.tile(np.asarray(T, np.float32) * np.float32(k), positions_q.size // 3)
    moved = positions_q + t
    assert moved.dtype == np.float32
    assert (moved.astype(np.float64) == positions_q.astype(np.float64) + t.astype(np.float64)).all()
    assert (moved - t).tobytes() == positions_q.tobytes()
    return moved


def bad_entries(W: int, H: int) -> list:
    """prev_pixel entries every tap of which lies outside a W x H image: huge
    finite values, infinities, NaN, and one pixel past each image edge (taps
    floor(p) and floor(p) + 1: -2 and W are the nearest positions with none
    in [0, W))."""
    inf, nan = float("inf"), float("nan")
    return [(1e9, 3.0), (-1e9, 3.0), (3.0, 1e9), (3.0, -1e9), (1e9, -1e9),
            (inf, 3.0), (-inf, 3.0), (3.0, inf), (3.0, -inf), (-inf, inf),
            (nan, 3.0), (3.0, nan), (nan, nan),
            (-2.0, 3.5), (float(W), 3.5), (3.5, -2.0), (3.5, float(H)), (-1.001, 3.5), (3.5, -1.001)]
