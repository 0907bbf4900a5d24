"""The stand-alone K2's tile order (run on an MI355X: pytest -m gpu).

k_fused_taa walks its 64 x 12 tiles against K1's order (last tile row first,
each XCD's band bottom-up): tile index G - 1 - xcd_swizzle(g, G).  That order
is reached only when a frame runs as two launches, which frames this small do
not by default, so every run here forces it (debug_frame_launches(2)).  The
sizes cover the tile counts G at which the XCD renumbering takes another path:
G < 8 (XCDs without a tile), G a multiple of 8, and remainders 1, 3 and 7.

  size      tile grid   G
  32 x 32    1 x 3       3
  64 x 84    1 x 7       7
  65 x 47    2 x 4       8
  192 x 32   3 x 3       9    (a height of 33..46 is not a valid frame: include/bmfr.h)
  131 x 97   3 x 9      27

Frames 0-3 of scene "rand": frame 0 has no history, the others gather the
reprojection taps and the TAA history.  Bars: the two-launch run's output and
every state plane == the forced one-launch run's byte for byte (exact fit and
fast_fit), and, exact fit, == the CPU oracle's.  A tile the reversed order
left out would show: the output buffer a frame writes starts out holding an
earlier frame's pixels, never this frame's.  Half input planes (the pair-tap
loads) at 131 x 97: two launches == one launch == the same values widened.
Every run ends with frame_status OK.
"""
from __future__ import annotations

import pytest

import scenes_np
from parity_harness import Suite
from ref_configs import RefConfig
from seq_util import FUSED_KEYS, compare_exact

pytestmark = pytest.mark.gpu

KEYS = tuple(FUSED_KEYS)
SCENE, SEED, FRAMES = "rand", 7, 4
TILE_W, TILE_H = 64, 12  # kTaaW, kTaaH (bmfr_kernels.hip)
# (width, height) -> the tile count the size is there for
SIZES = {(32, 32): 3, (64, 84): 7, (65, 47): 8, (192, 32): 9, (131, 97): 27}
CONFIGS = {f"k2_{w}x{h}": RefConfig(f"k2_{w}x{h}", w, h, frames=FRAMES, seed=SEED) for w, h in SIZES}
NAMES = list(CONFIGS)
HALF_NAME = "k2_131x97"


def frame(name: str, f: int) -> dict:
    rc = CONFIGS[name]
    return scenes_np.frame(SCENE, rc.width, rc.height, f, rc.seed)


SUITE = Suite(frame, CONFIGS.get, missing_ref=pytest.fail)  # no reference build is asked for


def tiles(w: int, h: int) -> int:
    return ((w + TILE_W - 1) // TILE_W) * ((h + TILE_H - 1) // TILE_H)


def test_sizes_cover_the_tile_counts():
    assert {tiles(w, h) for w, h in SIZES} == set(SIZES.values()) and all(tiles(w, h) == g for (w, h), g in SIZES.items())
    counts = sorted(SIZES.values())
    assert any(g < 8 for g in counts) and any(g % 8 == 0 for g in counts)
    assert {1, 3, 7} <= {g % 8 for g in counts}


@pytest.mark.parametrize("name", NAMES)
def test_two_launches_match_one_launch_and_oracle(name, gpu):
    """Exact fit."""
    two = SUITE.fused_frames(name, launches=2)
    one = SUITE.fused_frames(name, launches=1)
    assert len(two) == FRAMES
    compare_exact(two, one, KEYS, f"two launches vs one[{name}]")
    compare_exact(two, SUITE.oracle_frames(name), KEYS, f"two launches vs oracle[{name}]")
    SUITE.clear()


@pytest.mark.parametrize("name", NAMES)
def test_two_launches_match_one_launch_fast_fit(name, gpu):
    two = SUITE.fused_frames(name, launches=2, fast_fit=1)
    one = SUITE.fused_frames(name, launches=1, fast_fit=1)
    compare_exact(two, one, KEYS, f"fast_fit: two launches vs one[{name}]")
    SUITE.clear()


@pytest.mark.parametrize("fast_fit", [0, 1], ids=["exact", "fast_fit"])
def test_two_launches_half_inputs(fast_fit, gpu):
    """Half input planes: K1's previous position / normal taps are the 12-byte
    pair loads, albedo in K2 a 4- and a 2-byte load."""
    two = SUITE.fused_frames(HALF_NAME, half_in=True, launches=2, fast_fit=fast_fit)
    one = SUITE.fused_frames(HALF_NAME, half_in=True, launches=1, fast_fit=fast_fit)
    wide = SUITE.fused_frames(HALF_NAME, half_in=True, widen=True, launches=2, fast_fit=fast_fit)
    compare_exact(two, one, KEYS, f"half inputs: two launches vs one[{HALF_NAME}]")
    compare_exact(two, wide, KEYS, f"half inputs vs widened[{HALF_NAME}]")
    # the half path really read half planes
    plain = SUITE.fused_frames(HALF_NAME, launches=2, fast_fit=fast_fit)
    assert two[-1]["result"].tobytes() != plain[-1]["result"].tobytes()
    SUITE.clear()
