"""Test configurations shared by the oracle, the reference build and the tests.

TEST INFRASTRUCTURE ONLY.  A configuration is the reference's `#define`
surface (bmfr.cpp:32-118) for one image size / feature set / tmp precision.
`ref_build_options()` reproduces the JIT `-D` string of bmfr.cpp:205-232.
"""
from __future__ import annotations

import dataclasses

# Feature codes (same numbering as include/bmfr.h and oracle/bmfr_oracle.h)
# and the OpenCL expression text the reference pastes into FEATURE_BUFFERS.
FEATURE_TEXT = {
    0: "1.f",
    1: "normal.x", 2: "normal.y", 3: "normal.z",
    4: "world_position.x", 5: "world_position.y", 6: "world_position.z",
    7: "world_position.x*world_position.x",
    8: "world_position.y*world_position.y",
    9: "world_position.z*world_position.z",
    10: "world_position.x*world_position.x*world_position.x",
    11: "world_position.y*world_position.y*world_position.y",
    12: "world_position.z*world_position.z*world_position.z",
}

NOT_SCALED_DEFAULT = (0, 1, 2, 3)                 # bmfr.cpp:65-69
SCALED_DEFAULT = (4, 5, 6, 7, 8, 9)               # bmfr.cpp:71-77
SCALED_THIRD_ORDER = SCALED_DEFAULT + (10, 11, 12)  # BASELINE config 5


def fmt_g(x: float) -> str:
    """`std::ostream << double` with default flags: %g, 6 significant digits
    (bmfr.cpp:226-227 stream the dataset limits this way)."""
    return "%g" % x


@dataclasses.dataclass(frozen=True)
class RefConfig:
    name: str
    width: int
    height: int
    not_scaled: tuple = NOT_SCALED_DEFAULT
    scaled: tuple = SCALED_DEFAULT
    half_tmp: int = 1
    frames: int = 4
    noise_amount: str = "1e-2"          # NOISE_AMOUNT text, bmfr.cpp:58
    blend_alpha: str = "0.2f"           # bmfr.cpp:60
    second_blend_alpha: str = "0.1f"    # bmfr.cpp:61
    taa_blend_alpha: str = "0.2f"       # bmfr.cpp:62
    position_limit_squared: float = 0.01
    normal_limit_squared: float = 0.1
    seed: int = 0x424D4652

    @property
    def buffer_count(self) -> int:
        return len(self.not_scaled) + len(self.scaled) + 3

    @property
    def workset(self):
        return (32 * ((self.width + 31) // 32), 32 * ((self.height + 31) // 32))

    @property
    def margins(self):
        ww, wh = self.workset
        return ww + 32, wh + 32

    @property
    def blocks(self) -> int:
        mw, mh = self.margins
        return (mw // 32) * (mh // 32)

    def knobs(self) -> dict:
        """The six run-time parameters as the values the reference kernel sees
        in its literals, under the keyword names of BmfrConfig and
        pyoracle.make_cfg: the alphas are float literals ("0.05f" ->
        float32(0.05)), NOISE_AMOUNT a double literal; the two limits stay
        doubles, both sides apply the %g rule themselves."""
        import numpy as np
        f32 = lambda t: float(np.float32(float(t.rstrip("fF"))))  # noqa: E731
        return dict(noise_amount=float(self.noise_amount), blend_alpha=f32(self.blend_alpha),
                    second_blend_alpha=f32(self.second_blend_alpha), taa_blend_alpha=f32(self.taa_blend_alpha),
                    position_limit_squared=self.position_limit_squared,
                    normal_limit_squared=self.normal_limit_squared)

    def feature_text(self) -> str:
        return ",".join(FEATURE_TEXT[c] for c in self.not_scaled + self.scaled)

    def ref_build_options(self) -> list:
        ww, wh = self.workset
        mw, mh = self.margins
        b = self.buffer_count
        d = {
            "BUFFER_COUNT": b,
            "FEATURES_NOT_SCALED": len(self.not_scaled),
            "FEATURES_SCALED": len(self.scaled),
            "IMAGE_WIDTH": self.width,
            "IMAGE_HEIGHT": self.height,
            "WORKSET_WIDTH": ww,
            "WORKSET_HEIGHT": wh,
            "FEATURE_BUFFERS": self.feature_text(),
            "LOCAL_WIDTH": 8,
            "LOCAL_HEIGHT": 8,
            "WORKSET_WITH_MARGINS_WIDTH": mw,
            "WORKSET_WITH_MARGINS_HEIGHT": mh,
            "BLOCK_EDGE_LENGTH": 32,
            "BLOCK_PIXELS": 1024,
            "R_EDGE": b - 2,
            "NOISE_AMOUNT": self.noise_amount,
            "BLEND_ALPHA": self.blend_alpha,
            "SECOND_BLEND_ALPHA": self.second_blend_alpha,
            "TAA_BLEND_ALPHA": self.taa_blend_alpha,
            "POSITION_LIMIT_SQUARED": fmt_g(self.position_limit_squared),
            "NORMAL_LIMIT_SQUARED": fmt_g(self.normal_limit_squared),
            "COMPRESSED_R": 1,
            "CACHE_TMP_DATA": 1,
            "ADD_REQD_WG_SIZE": 1,
            "LOCAL_SIZE": 256,
            "USE_HALF_PRECISION_IN_TMP_DATA": self.half_tmp,
        }
        return [f"-D{k}={v}" for k, v in d.items()]


# Golden-vector configurations: small enough for the
# pure-CPU oracle to run in seconds, covering height padding (80 -> 96),
# width padding (100 -> 128), all 16 block offsets over 16 frames, both tmp
# precisions, the 3rd-order feature set (B = 16) and non-default feature
# lists (B = 7, 10, 12; no scaled features).
REF_CONFIGS = {
    c.name: c
    for c in (
        RefConfig("s128x80_h13", 128, 80, frames=17),
        RefConfig("s128x80_f13", 128, 80, half_tmp=0, frames=6),
        RefConfig("s100x72_h16", 100, 72, scaled=SCALED_THIRD_ORDER, frames=6),
        RefConfig("s96x64_f16", 96, 64, scaled=SCALED_THIRD_ORDER, half_tmp=0, frames=4),
        RefConfig("s48x48_h13", 48, 48, frames=4),
        RefConfig("s1280x720_h13", 1280, 720, frames=2),
        # other feature lists (bmfr.cpp:65-77): generic-count kernels
        RefConfig("s96x64_h7", 96, 64, not_scaled=(0,), scaled=(4, 5, 6), frames=4),
        RefConfig("s96x64_f10", 96, 64, scaled=(4, 5, 6), half_tmp=0, frames=4),
        RefConfig("s80x64_h12", 80, 64, not_scaled=(0, 3), scaled=(10, 11, 12, 7, 8, 9, 4), frames=4),
        RefConfig("s64x64_h7", 64, 64, scaled=(), frames=3),
    )
}

# BASELINE.json's configurations at their own sizes (GPU tests only: the CPU
# oracle is too slow there, so no golden .npz; tests/golden/fullsize_digests.json
# keeps SHA-256 digests of the reference's outputs).  frames: how many frames
# tests/test_gpu_reference_fullsize.py compares.
FULL_REF_CONFIGS = {
    c.name: c
    for c in (
        RefConfig("f1920x1080_h13", 1920, 1080, frames=17),              # config 2
        # 4K: 17 frames, so every one of the 16 block-grid offsets (bmfr.cl:267-285) is hit
        RefConfig("f3840x2160_h13", 3840, 2160, frames=17),              # config 3 (reference default build)
        RefConfig("f3840x2160_f13", 3840, 2160, half_tmp=0, frames=17),  # config 3, fp32 tmp_data
        RefConfig("f3840x2160_h16", 3840, 2160, scaled=SCALED_THIRD_ORDER, frames=17),  # config 5 (3rd order)
        RefConfig("f7680x4320_h13", 7680, 4320, frames=3),               # config 4's frame, untiled
        # B = 16 with f32 tmp_data: the MFMA experiment's tolerance reference (tools/mfma_experiment.py)
        RefConfig("f3840x2160_f16", 3840, 2160, scaled=SCALED_THIRD_ORDER, half_tmp=0, frames=4),
        RefConfig("f1280x720_h13", 1280, 720, frames=60),                # a whole 60-frame sequence
    )
}

# The run-time parameter surface away from the reference's defaults
# (tests/test_knobs_cpu.py, tests/test_gpu_knobs.py).  A set names only what it
# changes.  tight / loose / ends move all six; the limits of loose and ends are
# not their own %g text (0.123456789 -> "0.123457", 1.0000049 -> "1").  cut:
# BLEND_ALPHA 1 keeps spp at 1.  lit: a normal limit whose %g text is "1", on
# content whose squared normal distance is 1.0000019 (tests/knob_util.py).
KNOB_SETS = {
    "tight": dict(noise_amount="1e-3", blend_alpha="0.5f", second_blend_alpha="0.25f", taa_blend_alpha="0.05f",
                  position_limit_squared=0.0025, normal_limit_squared=3.0),
    "loose": dict(noise_amount="1e-1", blend_alpha="0.05f", second_blend_alpha="0.02f", taa_blend_alpha="0.5f",
                  position_limit_squared=0.123456789, normal_limit_squared=1.5),
    "ends": dict(noise_amount="0.5", blend_alpha="0.0f", second_blend_alpha="0.0f", taa_blend_alpha="1.0f",
                 position_limit_squared=1.0000049, normal_limit_squared=0.5),
    "cut": dict(blend_alpha="1.0f"),
    "lit": dict(normal_limit_squared=1.0000049),
}
KNOB_FRAMES = 14  # SECOND_BLEND_ALPHA 0.1 caps 1 / spp from spp 11 on


def _knob_config(knob_set: str, base: str, frames: int = KNOB_FRAMES) -> RefConfig:
    """Size, feature list and tmp precision of REF_CONFIGS["s" + base]."""
    return dataclasses.replace(REF_CONFIGS["s" + base], name=f"k_{knob_set}_{base}", frames=frames,
                               **KNOB_SETS[knob_set])


KNOB_REF_CONFIGS = {
    c.name: c
    for c in (
        _knob_config("tight", "128x80_h13"),
        _knob_config("tight", "128x80_f13"),
        _knob_config("loose", "100x72_h16"),
        _knob_config("loose", "96x64_h7"),   # generic-count K1
        _knob_config("ends", "128x80_h13"),
        _knob_config("ends", "100x72_h16"),
        _knob_config("cut", "128x80_h13"),
        _knob_config("lit", "128x80_h13", frames=8),
    )
}


def knob_set_of(name: str) -> str:
    return name.split("_")[1]


# The shape sweep (tests/test_shapes_cpu.py, tests/test_gpu_shapes.py): one
# configuration per (FEATURES_NOT_SCALED, FEATURES_SCALED, tmp_data precision)
# the library instantiates a generic-count kernel for -- NS 1..4, FS 0..9, both
# precisions, 80 in all --, named g_n<NS>s<FS>_<h|f>.  80x48: both axes padded
# (96x64 workset, 4x3 block grid with the margins).  3 frames: reprojection, two
# block offsets, the noise seed's frame term.  Content: scene "rand" of
# tests/scenes_np.py with seed SHAPE_SEED.
#
# Lists: position 0 is code 0 (1.f), as in every list the reference ships; the
# other NS + FS - 1 positions are codes 1..12 without repetition, by a rotation:
# position i holds 1 + (start + 5 i) mod 12, start = (7 FS + 4 NS + extra) mod
# 12, extra = SHAPE_ROTATION.get((NS, FS), 0).  A step of 5 never gives 1, 2, 3
# in a row, so no list is a canonical one.  Both precisions take the same list.
SHAPE_SIZE = (80, 48)
SHAPE_FRAMES = 3
SHAPE_SCENE = "rand"
SHAPE_SEED = 7
SHAPE_NS = (1, 2, 3, 4)
SHAPE_FS = tuple(range(10))
# (NS, FS) -> another rotation, for a list on which the CPU oracle's records
# are not all finite (tests/test_shapes_cpu.py); none needed so far
SHAPE_ROTATION = {}


def shape_lists(ns: int, fs: int):
    """(not_scaled, scaled) of the sweep's shape (ns, fs)."""
    start = (7 * fs + 4 * ns + SHAPE_ROTATION.get((ns, fs), 0)) % 12
    rest = tuple(1 + (start + 5 * i) % 12 for i in range(ns + fs - 1))
    return (0,) + rest[:ns - 1], rest[ns - 1:]


def shape_name(ns: int, fs: int, half_tmp: int) -> str:
    return f"g_n{ns}s{fs}_{'h' if half_tmp else 'f'}"


def shape_of(name: str):
    """(NS, FS, half_tmp) of a sweep name, the odd lists included."""
    rc = SHAPE_REF_CONFIGS[name]
    return len(rc.not_scaled), len(rc.scaled), rc.half_tmp


# Lists the rule does not give, at (3, 5) in both precisions: no constant at
# all; the constant in the scaled group (a constant column's max - min is 0:
# the |max - min| <= 1 arm of scale(), bmfr.cl:200-205, leaves a zero column);
# one code (position.x) in both groups.  Position 0 of the first two is a
# position: the first column is the one the fit adds no noise to (bmfr.cl:623-626),
# and a normal component vanishes on whole blocks of an axis-aligned wall, which
# makes the first Householder step 0 / 0 in the reference itself.
SHAPE_ODD_LISTS = {
    "noconst": ((6, 2, 10), (4, 8, 12, 1, 5)),
    "cscaled": ((5, 1, 3), (7, 0, 9, 11, 2)),
    "twice": ((0, 4, 2), (4, 6, 8, 10, 12)),
}


def _shape_config(name, lists, half_tmp) -> RefConfig:
    return RefConfig(name, *SHAPE_SIZE, not_scaled=lists[0], scaled=lists[1], half_tmp=half_tmp,
                     frames=SHAPE_FRAMES, seed=SHAPE_SEED)


SHAPE_REF_CONFIGS = {
    c.name: c
    for c in [_shape_config(shape_name(ns, fs, h), shape_lists(ns, fs), h)
              for h in (1, 0) for ns in SHAPE_NS for fs in SHAPE_FS] +
             [_shape_config(f"{shape_name(3, 5, h)}_{odd}", lists, h)
              for h in (1, 0) for odd, lists in SHAPE_ODD_LISTS.items()]
}


# The geometry sweep (tests/test_geometry_cpu.py, tests/test_gpu_geometry.py):
# frame sizes at the accepted end of the library's rule -- an axis n is valid
# when n >= 32 and workset(n) + 30 <= 2 n, so 32 and everything from 47 up --
# with odd widths and heights.  Named g<W>x<H>_<h|f><B>.  Content: scene "rand"
# with seed GEOMETRY_SEED.  17 frames go through all 16 block offsets (both
# -16s included), 6 frames still reach +-14 in y.  What each size is there for
# is computed from the block-offset table in tests/test_geometry_cpu.py.
GEOMETRY_SCENE = "rand"
GEOMETRY_SEED = 7
GEOMETRY_GENERIC_LISTS = {7: ((0,), (4, 5, 6)), 12: ((0, 3), (10, 11, 12, 7, 8, 9, 4))}


def _geometry_config(w, h, half_tmp, buffers, frames) -> RefConfig:
    lists = {13: (NOT_SCALED_DEFAULT, SCALED_DEFAULT), 16: (NOT_SCALED_DEFAULT, SCALED_THIRD_ORDER),
             **GEOMETRY_GENERIC_LISTS}[buffers]
    return RefConfig(f"g{w}x{h}_{'h' if half_tmp else 'f'}{buffers}", w, h, not_scaled=lists[0], scaled=lists[1],
                     half_tmp=half_tmp, frames=frames, seed=GEOMETRY_SEED)


GEOMETRY_REF_CONFIGS = {
    c.name: c
    for c in (
        _geometry_config(32, 32, 1, 13, 17),    # smallest frame; -32 -> 31; 2 x 2 blocks; one TAA tile
        _geometry_config(32, 32, 0, 13, 6),     # the same on the row-split K1
        _geometry_config(47, 47, 1, 13, 17),    # 93 -> 0; odd stride
        _geometry_config(47, 47, 1, 16, 6),     # B = 16 at the limit
        _geometry_config(65, 47, 1, 13, 17),    # one-pixel block column; 1 px past a TAA tile in x
        # one-pixel block row; 1 px past the 16-high TAA tile, 5 past the 12-high.  10 frames: the y offset -16, on which
        # the last block row holds image row 64 alone, is frame 9's
        _geometry_config(47, 65, 0, 16, 10),
        _geometry_config(97, 79, 1, 13, 6),     # height 79: work-item 96 + 29 mirrors onto pixel 32
        _geometry_config(97, 79, 1, 7, 6),      # generic-count K1 at an odd size
        _geometry_config(129, 53, 1, 13, 17),   # 1 px past two TAA tiles; H mod 16 = 5, mod 12 = 5
        _geometry_config(129, 53, 0, 13, 6),
        _geometry_config(67, 131, 1, 16, 6),    # tall; H mod 16 = 3, mod 12 = 11
        _geometry_config(67, 131, 1, 12, 6),    # generic K1, tall
    )
}


# Build modes of the reference: "strict" fixes the arithmetic OpenCL leaves to
# the implementation (no contraction, correctly rounded / and sqrt) and is the
# one the oracle is pinned to bit-for-bit; "default" is what bmfr.cpp's
# options alone give (contraction on, 2.5-ulp divide) and is compared with a
# tolerance.
REF_MODES = {
    "strict": ["-ffp-contract=off", "-cl-fp32-correctly-rounded-divide-sqrt"],
    "default": [],
}
