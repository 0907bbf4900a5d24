"""What the record comparators of tests/seq_util.py mean, on hand-made
records: every parity claim in DESIGN.md rests on compare_exact (bytes) and
compare_nan_aware (the same NaN positions, bytes everywhere else), and the
fast_fit bars on rel_l2_finite and worst_tile.  No GPU, no library."""
from __future__ import annotations

import numpy as np
import pytest

from seq_util import compare_exact, compare_nan_aware, rel_l2_finite, worst_tile

KEYS = ("result", "spp", "tmp_noisy")
BOTH = pytest.mark.parametrize("compare", [compare_exact, compare_nan_aware])
F32_NAN, F32_NAN_PAYLOAD, F32_NAN_NEGATIVE = 0x7fc00000, 0x7fc00001, 0xffc00000
F16_NAN, F16_NAN_PAYLOAD = 0x7e00, 0x7e01


def records():
    """Two frames: an f32 buffer, the uint8 spp plane and a half buffer as its
    bits (seq_util.to_np), frame 1 with an infinity of each sign."""
    out = []
    for f in range(2):
        result = np.array([0.25, -1.5, 3.0, 0.0, 7.0, 1e-3], np.float32) + np.float32(f)
        tmp = np.array([1.0, -2.5, 0.0, 1e-3], np.float16) + np.float16(f)
        if f == 1:
            result[4], result[5], tmp[3] = np.inf, -np.inf, np.inf
        out.append({"result": result, "spp": np.array([1, 2, 3, 255], np.uint8), "tmp_noisy": tmp.view(np.uint16)})
    return out


def set_bits(rec, key, index, pattern):
    """The element's bits replaced, whatever the buffer's dtype."""
    a = rec[key]
    a.view({2: np.uint16, 4: np.uint32}[a.itemsize])[index] = pattern


def fails(compare, got, ref, *named):
    with pytest.raises(AssertionError) as e:
        compare(got, ref, KEYS, "case")
    for text in named:
        assert text in str(e.value), str(e.value)


@BOTH
def test_identical_records_pass(compare):
    compare(records(), records(), KEYS, "case")  # equal infinities included


@BOTH
def test_one_low_mantissa_bit_fails_and_is_located(compare):
    got = records()
    got[1]["result"].view(np.uint32)[2] ^= 1
    fails(compare, got, records(), "case", "frame 1 result")
    fails(compare, records(), got, "frame 1 result")


@BOTH
def test_signed_zero_fails(compare):
    got = records()
    assert got[0]["result"][3] == 0.0
    got[0]["result"][3] = -0.0
    fails(compare, got, records(), "frame 0 result")
    got = records()
    set_bits(got[0], "tmp_noisy", 2, 0x8000)  # half -0
    fails(compare, got, records(), "frame 0 tmp_noisy")


@pytest.mark.parametrize("key,a,b", [("result", F32_NAN, F32_NAN_PAYLOAD), ("result", F32_NAN, F32_NAN_NEGATIVE),
                                     ("tmp_noisy", F16_NAN, F16_NAN_PAYLOAD)], ids=["f32", "f32_sign", "half"])
def test_nan_payload_is_open_to_nan_aware_only(key, a, b):
    got, ref = records(), records()
    set_bits(got[1], key, 1, a)
    set_bits(ref[1], key, 1, b)
    compare_nan_aware(got, ref, KEYS, "case")
    fails(compare_exact, got, ref, f"frame 1 {key}")
    set_bits(ref[1], key, 1, a)  # the same payload: equal bytes
    compare_exact(got, ref, KEYS, "case")


@pytest.mark.parametrize("key,nan", [("result", F32_NAN), ("tmp_noisy", F16_NAN)], ids=["f32", "half"])
def test_nan_at_another_index_fails(key, nan):
    got, ref = records(), records()
    set_bits(got[0], key, 0, nan)
    set_bits(ref[0], key, 1, nan)
    fails(compare_nan_aware, got, ref, f"frame 0 {key}", "NaN")
    fails(compare_exact, got, ref, f"frame 0 {key}")
    fails(compare_nan_aware, got, records(), f"frame 0 {key}")  # NaN against a number


def test_half_buffer_differs_beside_a_nan():
    """The NaN mask covers the NaN alone: a differing half beside it is found."""
    got, ref = records(), records()
    set_bits(got[1], "tmp_noisy", 0, F16_NAN)
    set_bits(ref[1], "tmp_noisy", 0, F16_NAN_PAYLOAD)
    compare_nan_aware(got, ref, KEYS, "case")
    got[1]["tmp_noisy"][1] ^= 1
    fails(compare_nan_aware, got, ref, "frame 1 tmp_noisy")


@BOTH
def test_infinities_of_opposite_sign_fail(compare):
    got = records()
    assert np.isposinf(got[1]["result"][4])
    got[1]["result"][4] = -np.inf
    fails(compare, got, records(), "frame 1 result")
    got = records()
    set_bits(got[1], "tmp_noisy", 3, 0xfc00)  # half -inf
    fails(compare, got, records(), "frame 1 tmp_noisy")


@BOTH
def test_spp_difference_fails(compare):
    got = records()
    got[1]["spp"][0] = 2
    fails(compare, got, records(), "frame 1 spp")


@BOTH
def test_shape_or_dtype_mismatch_fails(compare):
    got = records()
    got[0]["result"] = got[0]["result"].reshape(2, 3)
    fails(compare, got, records())
    got = records()
    got[0]["result"] = got[0]["result"][:5]
    fails(compare, got, records())
    for key, other in (("result", np.uint32), ("tmp_noisy", np.float16), ("spp", np.int8)):  # the same bytes
        got = records()
        got[1][key] = got[1][key].view(other)
        fails(compare, got, records())


@BOTH
def test_frame_count_mismatch_fails(compare):
    fails(compare, records()[:1], records(), "1", "2")
    fails(compare, [], records())
    fails(compare, records(), records()[:1])


@BOTH
def test_a_missing_key_is_not_skipped(compare):
    got = records()
    del got[1]["spp"]
    with pytest.raises(KeyError):
        compare(got, records(), KEYS, "case")
    compare(got, records(), ("result",), "case")  # a caller that compares one key says so


def test_rel_l2_finite():
    b = np.array([3.0, np.inf, 4.0, np.nan], np.float32)
    a = np.array([3.0, np.inf, 4.5, np.nan], np.float32)
    assert rel_l2_finite(a, b, "case") == pytest.approx(0.1)  # over the finite elements: 0.5 / 5
    assert rel_l2_finite(b, b, "case") == 0.0
    for bad in (np.array([3.0, 1.0, 4.0, np.nan], np.float32), np.array([np.inf, np.inf, 4.0, np.nan], np.float32),
                np.array([3.0, np.inf, 4.0, 0.0], np.float32)):
        with pytest.raises(AssertionError):
            rel_l2_finite(bad, b, "case")  # the non-finite positions differ
        with pytest.raises(AssertionError):
            rel_l2_finite(b, bad, "case")
    assert rel_l2_finite(np.ones(4, np.float32), np.zeros(4, np.float32), "case") is None  # no reference norm
    assert rel_l2_finite(np.array([np.nan], np.float32), np.array([np.nan], np.float32), "case") is None


def test_worst_tile_finds_an_error_in_a_narrow_edge_tile():
    """36 x 33: 32 x 32 tiles at x = 0, 32 and y = 0, 32; the tile at x = 32 is
    four pixels wide (the shape of the project's one known per-tile miss), the
    row at y = 32 one pixel high.  A small error there outweighs a larger
    absolute one spread over a full tile."""
    W, H = 36, 33
    rng = np.random.default_rng(1)
    ref = [{"result": (1.0 + rng.random(H * W * 3)).astype(np.float32)} for _ in range(2)]
    got = [{"result": r["result"].copy()} for r in ref]
    assert worst_tile(got, ref, W, H) == (0.0, -1, -1, -1)
    full = got[0]["result"].reshape(H, W, 3)
    full[:32, :32] += np.float32(1.5e-3)  # the whole first tile of frame 0: |error| 0.083, relative 1e-3
    edge = got[1]["result"].reshape(H, W, 3)
    edge[5, 34, 1] += np.float32(0.05)  # one value of the 4-wide tile at (32, 0) of frame 1: relative 1.7e-3
    e, f, tx, ty = worst_tile(got, ref, W, H)
    assert (f, tx, ty) == (1, 32, 0)
    a, b = edge[:32, 32:], ref[1]["result"].reshape(H, W, 3)[:32, 32:]
    assert e == pytest.approx(np.linalg.norm((a - b).astype(np.float64)) / np.linalg.norm(b.astype(np.float64)))
    assert e > rel_l2_finite(full[:32, :32], ref[0]["result"].reshape(H, W, 3)[:32, :32], "full tile") > 0
    # the one-pixel-high row of tiles is walked too
    got[0]["result"].reshape(H, W, 3)[32, 35, 0] += np.float32(1.0)
    assert worst_tile(got, ref, W, H)[1:] == (0, 32, 32)
    with pytest.raises(AssertionError):
        worst_tile(got[:1], ref, W, H)
