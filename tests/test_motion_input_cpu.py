"""bmfr_frame_inputs.prev_pixel (include/bmfr.h), the parts that need no GPU:
the struct layout, the exactness of the moving-world construction the GPU test
relies on (tests/motion_util.py), and the Python wrapper's checks of a plane
before it reaches the library."""
from __future__ import annotations

import ctypes as C

import numpy as np
import pytest
import torch

import bmfr_amd
from bmfr_amd import _lib
from bmfr_amd.pipeline import check_prev_pixel
from motion_util import T, quantise, translated


def test_frame_inputs_layout():
    names = [n for n, _ in _lib.FrameInputs._fields_]
    assert names == ["noisy", "normals", "positions", "albedo", "prev_normals", "prev_positions", "prev_pixel"]
    assert C.sizeof(_lib.FrameInputs) == 7 * C.sizeof(C.c_void_p)
    assert _lib.FrameInputs.prev_pixel.offset == 6 * C.sizeof(C.c_void_p)
    # code that fills the first six members leaves the plane NULL: today's behaviour
    assert _lib.FrameInputs(1, 2, 3, 4, 5, 6).prev_pixel is None


def test_moving_world_is_exact():
    """Quantised to 2^-8 and translated by f T, every coordinate stays exact in
    f32 -- translated() asserts it --, so previous - current differences in the
    moved world equal the static world's bit for bit, as f32 subtractions."""
    W, H = 128, 80
    q = [quantise(bmfr_amd.synth_frame_host(W, H, f)["positions"].reshape(-1)) for f in (0, 1, 8)]
    for a in q:
        assert (a * 256.0 == np.rint(a * 256.0)).all()
    for k, (prev, cur) in ((1, (q[0], q[1])), (8, (q[1], q[2]))):
        moved_prev, moved_cur = translated(prev, k), translated(cur, k)
        assert (moved_prev - moved_cur).tobytes() == (prev - cur).tobytes()
        # and the translation is large against the position limit (0.1 world units): without the
        # plane and the moved prev_positions, the position test rejects every tap
        assert sum(t * t for t in T) > 0.01
    with pytest.raises(AssertionError):
        translated(np.array([1.0 + 2.0 ** -23, 0.0, 0.0], np.float32), 4096 * 8)  # would round


def test_wrapper_rejects_wrong_planes():
    W, H = 100, 72
    check_prev_pixel(None, W, H)
    good_shape = torch.zeros(H, W, 2)
    with pytest.raises(ValueError, match="cuda"):       # right shape and dtype, wrong device
        check_prev_pixel(good_shape, W, H)
    with pytest.raises(ValueError, match="cuda"):
        check_prev_pixel(torch.zeros(H * W * 2), W, H)
    for bad in (torch.zeros(H, W, 3), torch.zeros(W, H, 2), torch.zeros(H * W), torch.zeros(H * W * 2 + 2),
                torch.zeros(H, W)):
        with pytest.raises(ValueError, match="shape"):
            check_prev_pixel(bad, W, H)
    for dt in (torch.float16, torch.float64, torch.int32):
        with pytest.raises(TypeError, match="float32"):
            check_prev_pixel(torch.zeros(H, W, 2, dtype=dt), W, H)
    with pytest.raises(ValueError, match="contiguous"):
        check_prev_pixel(torch.zeros(H, W, 4)[..., :2], W, H)
    with pytest.raises(TypeError):
        check_prev_pixel(np.zeros((H, W, 2), np.float32), W, H)


def test_denoiser_checks_before_calling_the_library():
    """Denoiser.process_frame and friends run the check first: a context that
    never reaches the library (no handle, no GPU) still rejects the plane."""
    class NoLibrary:
        def __getattr__(self, name):
            raise AssertionError(f"the library was called ({name})")

    den = bmfr_amd.Denoiser.__new__(bmfr_amd.Denoiser)
    den.lib, den.handle, den.device, den.prev_inputs = NoLibrary(), None, 0, None
    den.sizes = bmfr_amd.BmfrConfig(image_width=100, image_height=72).sizes()
    wrong = torch.zeros(72, 100, 3)
    for method in ("process_frame", "process_frame_interior", "process_frame_border"):
        with pytest.raises(ValueError, match="shape"):
            getattr(den, method)(None, None, None, None, [0.0] * 16, [0.0] * 2, 1, prev_pixel=wrong)
    with pytest.raises(ValueError, match="shape"):
        den.process_sequence([{"noisy": None, "normals": None, "positions": None, "albedo": None,
                               "prev_pixel": wrong}], [([0.0] * 16, [0.0] * 2)], 0)
    # a tiled context takes its region's plane, not the frame's
    den.sizes = bmfr_amd.BmfrConfig(image_width=320, image_height=256, tile=(0, 0, 160, 128), tile_halo=40).sizes()
    assert (den.sizes.region_width, den.sizes.region_height) == (200, 168)
    with pytest.raises(ValueError, match="shape"):
        den.process_frame(None, None, None, None, [0.0] * 16, [0.0] * 2, 1, prev_pixel=torch.zeros(256, 320, 2))
