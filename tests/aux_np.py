"""Caller-supplied feature planes (BMFR_FEATURE_AUX0..3, include/bmfr.h) on
the CPU.  TEST INFRASTRUCTURE ONLY.

AuxOracleLoop composes the unchanged CPU oracle (pyoracle) into the frame
loop of a feature list that names aux planes: the oracle's own stages run
wherever no feature is evaluated, and the two places that evaluate features
are done here, in numpy f32 with one rounding per operation --

  1. oracle_accumulate_noisy_data with placeholder named codes of the same
     counts (everything but the aux columns of tmp_data is then right),
  2. the aux columns of tmp_data overwritten with the plane's value at each
     work-item's mirrored pixel: NaN -> 0 and, half tmp_data, the +-65504
     clamp and rounding to half (bmfr.cl:448-473),
  3. oracle_fitter (reads only tmp_data),
  4. the weighted sum (bmfr.cl:703-758): features in list order, the raw
     plane value for an aux feature, scale() with the block's min / max for
     the scaled group, clamp at 0,
  5. oracle_accumulate_filtered_data and oracle_taa.

The planes of a frame are functions of that frame's input planes (PLANES
below), so the loop takes the same upload / run_stages / swap drivers as
every other loop (seq_util.run_loop, scenes_np.run_loop) and a GPU test can
form the same planes from the same inputs.  tests/test_aux_np.py pins the
helper to pyoracle.OracleLoop on monomial planes, byte for byte."""
from __future__ import annotations

import ctypes as C

import numpy as np

import pyoracle
from pyoracle import _p

AUX0 = 13
PLACEHOLDER = 0   # "1.f": the named code that stands in for an aux code in step 1
# BLOCK_OFFSETS of the reference (bmfr.cl:267-285)
OFFSETS = [(-14, -14), (4, -6), (-8, 14), (8, 0), (-10, -8), (2, 12), (12, -12), (-10, 0), (12, 14), (-8, -16),
           (6, 6), (-2, -2), (6, -14), (-16, 12), (14, -4), (-6, 4)]

f32 = np.float32


# ---- planes: (normals, positions, albedo) as (N, 3) f32, W, H -> (N,) f32, one rounding per operation ----
def _col(a, i):
    return np.ascontiguousarray(a[:, i])


def luminance(n, p, a, W, H):
    return (f32(0.2126) * a[:, 0] + f32(0.7152) * a[:, 1]) + f32(0.0722) * a[:, 2]


def object_id(n, p, a, W, H):
    """A step plane: four screen-space "objects" with ids 0, 3, 5, 8.  A block
    inside one of them has max - min = 0 (scale()'s |d| <= 1 arm), a block
    across an edge at least 2 (the other arm)."""
    y, x = np.divmod(np.arange(W * H), W)
    return (f32(3.0) * (x >= W // 2) + f32(5.0) * (y >= (2 * H) // 3)).astype(f32)


PLANES = {
    "one": lambda n, p, a, W, H: np.ones(n.shape[0], f32),
    "nx": lambda n, p, a, W, H: _col(n, 0),
    "ny": lambda n, p, a, W, H: _col(n, 1),
    "nz": lambda n, p, a, W, H: _col(n, 2),
    "px": lambda n, p, a, W, H: _col(p, 0),
    "py": lambda n, p, a, W, H: _col(p, 1),
    "pz": lambda n, p, a, W, H: _col(p, 2),
    "px2": lambda n, p, a, W, H: p[:, 0] * p[:, 0],
    "py2": lambda n, p, a, W, H: p[:, 1] * p[:, 1],
    "pz2": lambda n, p, a, W, H: p[:, 2] * p[:, 2],
    "px3": lambda n, p, a, W, H: (p[:, 0] * p[:, 0]) * p[:, 0],
    "py3": lambda n, p, a, W, H: (p[:, 1] * p[:, 1]) * p[:, 1],
    "pz3": lambda n, p, a, W, H: (p[:, 2] * p[:, 2]) * p[:, 2],
    # what no named code expresses
    "pxpy": lambda n, p, a, W, H: p[:, 0] * p[:, 1],
    "nxny": lambda n, p, a, W, H: n[:, 0] * n[:, 1],
    "lum": luminance,
    "objid": object_id,
}
# the named code a monomial plane stands for
CODE_OF = {"one": 0, "nx": 1, "ny": 2, "nz": 3, "px": 4, "py": 5, "pz": 6, "px2": 7, "py2": 8, "pz2": 9, "px3": 10, "py3": 11,
           "pz3": 12}


def aux_planes(names, normals, positions, albedo, W, H):
    """The four planes (None where names[k] is None) of one frame, from its
    flat f32 input planes."""
    n, p, a = (np.asarray(v, f32).reshape(-1, 3) for v in (normals, positions, albedo))
    with np.errstate(all="ignore"):
        out = [None if nm is None else np.ascontiguousarray(PLANES[nm](n, p, a, W, H), f32) for nm in names]
    return out + [None] * (4 - len(out))


def named_feature(code, n, p):
    """feature() of the oracle / feature_value() of the library, on (N, 3) f32."""
    if code == 0:
        return np.ones(n.shape[0], f32)
    if code <= 3:
        return n[:, code - 1]
    if code <= 6:
        return p[:, code - 4]
    if code <= 9:
        return p[:, code - 7] * p[:, code - 7]
    return (p[:, code - 10] * p[:, code - 10]) * p[:, code - 10]


def scale(v, mn, mx):
    """scale(), bmfr.cl:200-205."""
    d = mx - mn
    return np.where(np.abs(d) > f32(1.0), (v - mn) / d, v - mn)


class AuxOracleLoop(pyoracle.OracleLoop):
    """The frame loop of the feature list (not_scaled, scaled), whose codes
    13..16 name the planes `names` = up to four keys of PLANES."""

    def __init__(self, width, height, not_scaled, scaled, half_tmp, names, **knobs):
        self.codes = tuple(not_scaled) + tuple(scaled)
        self.names = tuple(names) + (None,) * (4 - len(names))
        assert all(self.names[c - AUX0] is not None for c in self.codes if c >= AUX0), "a named plane has no content"
        stand_in = lambda cs: tuple(PLACEHOLDER if c >= AUX0 else c for c in cs)  # noqa: E731
        super().__init__(pyoracle.make_cfg(width, height, stand_in(not_scaled), stand_in(scaled), half_tmp, **knobs))
        self.NS, self.FS = len(not_scaled), len(scaled)
        self.mw, self.mh = 32 * ((width + 31) // 32) + 32, 32 * ((height + 31) // 32) + 32

    def planes(self):
        W, H = self.cfg.width, self.cfg.height
        return aux_planes(self.names, self.cur(self.normals), self.cur(self.positions), self.albedo, W, H)

    def item_pixels(self, frame):
        """(GY, GX, 32, 32): the (mirrored) image pixel of every work-item of
        the margin grid, in tmp_data's block order (bmfr.cl:310-320)."""
        W, H = self.cfg.width, self.cfg.height
        ox, oy = OFFSETS[frame % 16]

        def mirror(i, size):
            return np.where(i < 0, -i - 1, np.where(i >= size, 2 * size - i - 1, i))

        px = mirror(np.arange(self.mw) - 16 + ox, W)
        py = mirror(np.arange(self.mh) - 16 + oy, H)
        lin = py[:, None] * W + px[None, :]
        return lin.reshape(self.mh // 32, 32, self.mw // 32, 32).transpose(0, 2, 1, 3)

    def overwrite_aux_columns(self, planes, frame):
        pix = self.item_pixels(frame)
        t = self.tmp.reshape(self.mh // 32, self.mw // 32, self.B, 32, 32)
        for f, code in enumerate(self.codes):
            if code < AUX0:
                continue
            v = planes[code - AUX0][pix]
            v = np.where(np.isnan(v), f32(0.0), v)
            if self.cfg.half_tmp:
                v = np.maximum(np.minimum(v, f32(65504.0)), f32(-65504.0))
                t[:, :, f] = v.astype(np.float16).view(np.uint16)
            else:
                t[:, :, f] = v

    def weighted_sum(self, planes, frame):
        W, H, B = self.cfg.width, self.cfg.height, self.B
        n = self.cur(self.normals).reshape(-1, 3)
        p = self.cur(self.positions).reshape(-1, 3)
        y, x = np.divmod(np.arange(W * H), W)
        ox, oy = OFFSETS[frame % 16]
        g = (x + 16 - ox) // 32 + ((y + 16 - oy) // 32) * (self.mw // 32)
        w = self.weights.reshape(self.G, B - 3, 3)
        mm = self.mins_maxs.reshape(self.G, self.FS, 2) if self.FS else None
        col = np.zeros((W * H, 3), f32)
        with np.errstate(all="ignore"):
            for f, code in enumerate(self.codes):
                v = planes[code - AUX0] if code >= AUX0 else named_feature(code, n, p)
                if f >= self.NS:
                    v = scale(v, mm[g, f - self.NS, 0], mm[g, f - self.NS, 1])
                v = v.astype(f32)
                col = col + w[g, f] * v[:, None]
            col = np.where(col < f32(0.0), f32(0.0), col)
        assert col.dtype == f32
        self.filtered[:] = col.reshape(-1)

    def run_stages(self, prev_vp, jitter, frame: int, record=None) -> None:
        lib, c = self.lib, C.byref(self.cfg)
        vp = np.asarray(prev_vp, np.float32)
        jt = np.asarray(jitter, np.float32)
        planes = self.planes()
        lib.oracle_accumulate_noisy_data(
            c, _p(self.prev_pixels), _p(self.accept), _p(self.cur(self.normals)), _p(self.prev(self.normals)),
            _p(self.cur(self.positions)), _p(self.prev(self.positions)), _p(self.cur(self.noisy)),
            _p(self.prev(self.noisy)), _p(self.prev(self.spp)), _p(self.cur(self.spp)), _p(self.tmp),
            _p(vp), _p(jt), frame)
        self.overwrite_aux_columns(planes, frame)
        if record is not None:
            record["tmp_noisy"] = self.tmp.copy()
        lib.oracle_fitter(c, _p(self.weights), _p(self.mins_maxs), _p(self.tmp), frame)
        self.weighted_sum(planes, frame)
        lib.oracle_accumulate_filtered_data(
            c, _p(self.filtered), _p(self.prev_pixels), _p(self.accept), _p(self.albedo), _p(self.tone),
            _p(self.cur(self.spp)), _p(self.prev(self.out)), _p(self.cur(self.out)), frame)
        lib.oracle_taa(c, _p(self.prev_pixels), _p(self.tone), _p(self.cur(self.result)),
                       _p(self.prev(self.result)), frame)
        if record is not None:
            record.update(
                tmp_fit=self.tmp.copy(), weights=self.weights.copy(), mins_maxs=self.mins_maxs.copy(),
                filtered=self.filtered.copy(), acc=self.cur(self.out).copy(), tone=self.tone.copy(),
                result=self.cur(self.result).copy(), spp=self.cur(self.spp).copy(),
                accept=self.accept.copy(), prev_pixel=self.prev_pixels.copy(),
                noisy=self.cur(self.noisy).copy())


def substitute(codes, subs):
    """A feature list with its entries at positions `subs` = {position: k}
    replaced by code AUX0 + k -> (list, {k: the replaced code})."""
    out = list(codes)
    was = {}
    for pos, k in subs.items():
        was[k] = out[pos]
        out[pos] = AUX0 + k
    return tuple(out), was


# The feature list of the content tests: luminance not scaled; the cross terms
# and the object id scaled.  NS = 4, FS = 6 (B = 13, non-canonical).
NOVEL_NOT_SCALED = (0, 1, 2, AUX0 + 0)
NOVEL_SCALED = (4, 5, 6, AUX0 + 1, AUX0 + 2, AUX0 + 3)
NOVEL_NAMES = ("lum", "pxpy", "nxny", "objid")
# (width, height, half tmp_data)
NOVEL_SIZES = ((100, 72, 1), (96, 64, 0))
NOVEL_FRAMES = 6


# ---- content: the synthetic sequence, or a scene of scenes_np, as frame dicts ----
def frame_source(source: str, W: int, H: int):
    """f -> dict(noisy, normals, positions, albedo flat f32, prev_vp, jitter).
    source: "synth" (the synthetic sequence) or a scenes_np scene (seed 2)."""
    if source == "synth":
        import seq_util
        from ref_configs import RefConfig
        rc = RefConfig(f"aux{W}x{H}", W, H)

        def synth(f):
            fr = {k: np.ascontiguousarray(v, f32).reshape(-1) for k, v in seq_util.frame_inputs(rc, f).items()}
            fr["prev_vp"], fr["jitter"] = seq_util.camera(rc, f)
            return fr
        return synth
    import scenes_np
    return lambda f: scenes_np.frame(source, W, H, f, 2)


def run(loop, source: str, frames: int):
    import scenes_np
    W, H = loop.cfg.width, loop.cfg.height
    return scenes_np.run_loop(loop, source, W, H, frames, source=frame_source(source, W, H))


_novel = {}


def novel_frames(W: int, H: int, half_tmp: int, source: str, names=NOVEL_NAMES):
    """The records of AuxOracleLoop over the content tests' list; computed
    once per case, shared by the tests, never modified."""
    key = (W, H, half_tmp, source, tuple(names))
    if key not in _novel:
        _novel[key] = run(AuxOracleLoop(W, H, NOVEL_NOT_SCALED, NOVEL_SCALED, half_tmp, names), source, NOVEL_FRAMES)
    return _novel[key]
