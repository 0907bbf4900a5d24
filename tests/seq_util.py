"""Shared helpers for the sequence tests: drive any frame loop (CPU oracle,
reference kernels, libbmfr stages) over the synthetic sequence and compare
the recorded buffers -- "records": the list of per-frame dicts of numpy
buffers one pipeline run returns.  Numpy only (the two functions that render
the synthetic sequence load the library); the device side of the GPU suites
is tests/parity_harness.py.  tests/test_seq_util_cpu.py pins the comparators."""
from __future__ import annotations

import hashlib

import numpy as np

from ref_configs import RefConfig

# Buffers whose values are pinned bit for bit.  tone / result go through
# powr(), which the GPU library does not round correctly, so the CPU oracle
# is held to a tolerance there (GPU vs GPU stays bit-exact).
EXACT_KEYS = ("tmp_noisy", "tmp_fit", "weights", "mins_maxs", "filtered", "acc", "spp", "accept",
              "prev_pixel", "noisy")
POWR_KEYS = ("tone", "result")
ALL_KEYS = EXACT_KEYS + POWR_KEYS
PLANES = ("noisy", "normals", "positions", "albedo")
# record key -> bmfr_state plane.  (The fused kernel keeps the accept bits in registers -- bmfr_state
# reports no accept plane -- so they are compared through what they decide: spp and both accumulations.)
FUSED_KEYS = {"result": "result", "noisy": "noisy_accumulated", "acc": "filtered_accumulated", "spp": "spp",
              "prev_pixel": "prev_frame_pixel"}
# what a frame that replays a prev_pixel plane gets as its camera: a NaN matrix and a garbage pixel
# offset, to show neither is read
NAN_VP = [float("nan")] * 16
GARBAGE_JITTER = [float("nan"), 1e30]
TOL = 1e-4  # north_star: "within 1e-4 relative L2 of the OpenCL reference" (tests/test_gpu_fast_fit.py)
# fast_fit against the reference's own build-to-build distance: the largest ratio of the two at frame
# level in the project's records rounded up (tests/test_gpu_content_parity.py)
TILE_FACTOR = 4.0


def frame_inputs(rc: RefConfig, frame: int):
    import bmfr_amd
    return bmfr_amd.synth_frame_host(rc.width, rc.height, frame, seed=rc.seed)


def camera(rc: RefConfig, frame: int):
    """(camera_matrices[max(frame-1,0)], pixel_offsets[frame]), bmfr.cpp:440-444."""
    import bmfr_amd
    vp, _ = bmfr_amd.synth_camera(rc.width, rc.height, max(frame - 1, 0))
    _, jit = bmfr_amd.synth_camera(rc.width, rc.height, frame)
    return vp, jit


def input_digest(fr) -> str:
    h = hashlib.sha256()
    for k in PLANES:
        h.update(np.ascontiguousarray(fr[k], np.float32).tobytes())
    return h.hexdigest()


def to_np(x) -> np.ndarray:
    if hasattr(x, "detach"):
        x = x.detach().cpu()
        if str(x.dtype) == "torch.float16":
            return x.view(__import__("torch").int16).numpy().view(np.uint16)
        return x.numpy()
    return np.asarray(x)


def digest(a) -> str:
    return hashlib.sha256(np.ascontiguousarray(to_np(a)).tobytes()).hexdigest()


def sample_idx(n: int, k: int = 8192) -> np.ndarray:
    return np.unique(np.linspace(0, n - 1, min(n, k)).astype(np.int64))


def run_loop(loop, rc: RefConfig, frames: int, to_device=None, sync=None):
    """Run `frames` frames; returns a list of per-frame dicts of numpy arrays."""
    out = []
    for f in range(frames):
        fr = frame_inputs(rc, f)
        if to_device is not None:
            fr = {k: to_device(v) for k, v in fr.items()}
        loop.upload(fr["noisy"], fr["normals"], fr["positions"], fr["albedo"])
        vp, jit = camera(rc, f)
        rec = {}
        loop.run_stages(vp, jit, f, record=rec)
        if sync is not None:
            sync()
        out.append({k: to_np(v).copy() for k, v in rec.items()})
        loop.swap()
    return out


def rel_l2(a, b) -> float:
    a = np.asarray(a, np.float64)
    b = np.asarray(b, np.float64)
    d = np.linalg.norm(a - b)
    n = np.linalg.norm(b)
    return float(d / n) if n > 0 else float(d)


def through_half(a: np.ndarray) -> np.ndarray:
    return a.astype(np.float16).astype(np.float32)


def _frame_pairs(got, ref, where):
    """(frame, got's record, ref's record); a run that stopped early is not equal to its reference."""
    assert len(got) == len(ref), f"{where}: {len(got)} frames against {len(ref)}"
    return enumerate(zip(got, ref))


def _flat_pair(g, r, k, where, f):
    a, b = g[k], r[k]
    assert a.shape == b.shape and a.dtype == b.dtype, (where, f, k, a.shape, b.shape, a.dtype, b.dtype)
    return np.ascontiguousarray(a).reshape(-1), np.ascontiguousarray(b).reshape(-1)


def _bits(a: np.ndarray) -> np.ndarray:
    return a.view({1: np.uint8, 2: np.uint16, 4: np.uint32, 8: np.uint64}[a.itemsize])


def _floats(a: np.ndarray):
    if a.dtype == np.uint16:  # half buffers travel as their bits (to_np)
        return a.view(np.float16)
    return a if a.dtype.kind == "f" else None


def compare_exact(got, ref, keys=EXACT_KEYS, where=""):
    """Assert bitwise equality of every key (as raw bytes) on every frame;
    report the first mismatching frame with a useful summary.  A key that a
    record lacks is an error: a caller that compares fewer keys names them."""
    for f, (g, r) in _frame_pairs(got, ref, where):
        for k in keys:
            a, b = _flat_pair(g, r, k, where, f)
            bad = np.flatnonzero(_bits(a) != _bits(b))
            if bad.size:
                msg = f"{where} frame {f} {k}: {bad.size} of {a.size} differ, first at {bad[:5]}: " \
                      f"{a[bad[:5]]} vs {b[bad[:5]]}"
                if a.dtype == np.float32:
                    with np.errstate(all="ignore"):
                        msg += f", rel_l2 {rel_l2(a, b):.3e}"
                raise AssertionError(msg)


def compare_nan_aware(got, ref, keys, where=""):
    """Equal when the NaN positions are the same set and every other element,
    infinities included, has the same bits."""
    for f, (g, r) in _frame_pairs(got, ref, where):
        for k in keys:
            a, b = _flat_pair(g, r, k, where, f)
            fa, fb = _floats(a), _floats(b)
            if fa is None:
                bad = np.flatnonzero(a != b)
            else:
                na, nb = np.isnan(fa), np.isnan(fb)
                assert (na == nb).all(), f"{where} frame {f} {k}: NaN at {int(na.sum())} vs {int(nb.sum())} places, " \
                                         f"first difference at {np.flatnonzero(na != nb)[:5]}"
                bad = np.flatnonzero((_bits(a) != _bits(b)) & ~na)
            assert bad.size == 0, f"{where} frame {f} {k}: {bad.size} of {a.size} differ, first at {bad[:5]}: " \
                                  f"{a[bad[:5]]} vs {b[bad[:5]]}"


def assert_finite(frames, keys, where=""):
    for f, g in enumerate(frames):
        for k in keys:
            v = _floats(g[k])
            assert v is None or np.isfinite(v).all(), (where, f, k)


def rel_l2_finite(a, b, where):
    """Relative L2 over the elements finite in the reference b; the
    non-finite positions must coincide.  None where the reference's norm is 0."""
    fa, fb = np.isfinite(a), np.isfinite(b)
    assert (fa == fb).all(), (where, int((~fa).sum()), int((~fb).sum()))
    a, b = a[fb].astype(np.float64), b[fb].astype(np.float64)
    n = np.linalg.norm(b)
    return float(np.linalg.norm(a - b) / n) if n > 0 else None


def worst_tile(frames, ref, W, H):
    """(worst relative L2, frame, tile x, tile y) over the 32x32 image-aligned
    tiles of `result`; tiles whose reference norm is zero are skipped."""
    worst = (0.0, -1, -1, -1)
    for f, (g, r) in _frame_pairs(frames, ref, "worst_tile"):
        a, b = g["result"].reshape(H, W, 3), r["result"].reshape(H, W, 3)
        for ty in range(0, H, 32):
            for tx in range(0, W, 32):
                e = rel_l2_finite(a[ty:ty + 32, tx:tx + 32], b[ty:ty + 32, tx:tx + 32], (f, tx, ty))
                if e is not None and e > worst[0]:
                    worst = (e, f, tx, ty)
    return worst
