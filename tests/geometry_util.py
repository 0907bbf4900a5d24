"""Shared by the geometry sweep's tests (ref_configs.GEOMETRY_REF_CONFIGS;
tests/test_geometry_cpu.py, tests/test_gpu_geometry.py) and the golden
generator: the sweep's content, the CPU oracle over it, and the block-grid
arithmetic the coverage claims are computed from.  TEST INFRASTRUCTURE ONLY:
imports nothing from bmfr_amd."""
from __future__ import annotations

import pyoracle
import scenes_np
import shape_util
from aux_np import OFFSETS
from ref_configs import GEOMETRY_REF_CONFIGS, GEOMETRY_SCENE

NAMES = list(GEOMETRY_REF_CONFIGS)
CANONICAL = [n for n, rc in GEOMETRY_REF_CONFIGS.items() if shape_util.canonical(rc.not_scaled, rc.scaled)]
CANONICAL_HALF = [n for n in CANONICAL if GEOMETRY_REF_CONFIGS[n].half_tmp]
GENERIC = [n for n in NAMES if n not in CANONICAL]
# pinned to the reference's strict build without a GPU (tests/golden/geometry/*.npz), and the
# frames each fixture keeps: 17 frames of g65x47 would pass the size of a committed file
GOLDEN_FRAMES = {"g32x32_h13": 17, "g47x47_h16": 6, "g65x47_h13": 6}
E = 32  # BLOCK_EDGE_LENGTH


def frame(name: str, f: int) -> dict:
    """Frame f of the configuration's content (scenes_np.frame: shared, read-only)."""
    rc = GEOMETRY_REF_CONFIGS[name]
    return scenes_np.frame(GEOMETRY_SCENE, rc.width, rc.height, f, rc.seed)


def run_loop(loop, name: str, frames=None, **kw):
    rc = GEOMETRY_REF_CONFIGS[name]
    return scenes_np.run_loop(loop, GEOMETRY_SCENE, rc.width, rc.height, frames or rc.frames, rc.seed, **kw)


def make_cfg(name: str):
    rc = GEOMETRY_REF_CONFIGS[name]
    return pyoracle.make_cfg(rc.width, rc.height, rc.not_scaled, rc.scaled, rc.half_tmp, **rc.knobs())


_oracle = {}


def oracle_frames(name: str):
    """The CPU oracle's records over the configuration's frames, computed once
    and never modified."""
    if name not in _oracle:
        _oracle[name] = run_loop(pyoracle.OracleLoop(make_cfg(name)), name)
    return _oracle[name]


# ---- the block grid on one axis (bmfr.cl:207-216, 267-285, 310-317) ----
def mirror(p: int, n: int) -> int:
    return -p - 1 if p < 0 else (2 * n - p - 1 if p >= n else p)


def workset(n: int) -> int:
    return E * ((n + E - 1) // E)


def valid_axis(n: int) -> bool:
    """include/bmfr.h: every margin work-item less than one image size out of range."""
    return n >= E and workset(n) + 30 <= 2 * n


def item_range(n: int, off: int):
    """(first, last) pixel of the margin grid's work-items on an axis of n
    pixels under the block offset `off`: gid - 16 + off, gid < workset + 32."""
    return -E // 2 + off, workset(n) + E // 2 + off - 1


def block_pixels(n: int, off: int, b: int):
    """The image pixels inside block b of the axis: those it owns."""
    p0 = E * b - E // 2 + off
    return [p for p in range(p0, p0 + E) if 0 <= p < n]


def blocks(n: int) -> int:
    return workset(n) // E + 1


def axis_offsets(name: str, axis: int):
    """The block offsets the configuration's frames take on the axis (0: x, 1: y)."""
    return [OFFSETS[f % 16][axis] for f in range(GEOMETRY_REF_CONFIGS[name].frames)]


def deepest_sources(name: str, axis: int):
    """The mirrored source pixel of the lowest and of the highest work-item
    the configuration's frames reach on the axis -> (from below, from above)."""
    rc = GEOMETRY_REF_CONFIGS[name]
    n = (rc.width, rc.height)[axis]
    lo = min(item_range(n, off)[0] for off in axis_offsets(name, axis))
    hi = max(item_range(n, off)[1] for off in axis_offsets(name, axis))
    assert -n <= lo and hi <= 2 * n - 1, (name, axis, lo, hi)
    return mirror(lo, n), mirror(hi, n)
