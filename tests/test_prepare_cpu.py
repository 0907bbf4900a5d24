"""The G-buffer front end (bmfr_prepare_frame, include/bmfr.h), the parts that
need no GPU: the struct layouts, the argument checks, and properties of the
numpy restatement (tests/prepare_np.py) the GPU tests hold the kernel to."""
from __future__ import annotations

import ctypes as C
import os
import subprocess

import numpy as np

import bmfr_amd
from bmfr_amd import _lib
import prepare_np as pn

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
F32 = np.float32


def test_struct_sizes_match_header(tmp_path):
    """The ctypes mirrors of bmfr_gbuffer / bmfr_prepared have the header's sizes and field offsets."""
    src = ('#include <stdio.h>\n#include <stddef.h>\n#include "bmfr.h"\nint main(void){printf("%zu %zu %zu %zu %zu %d", '
           'sizeof(bmfr_gbuffer), sizeof(bmfr_prepared), offsetof(bmfr_gbuffer, inv_view_proj), '
           'offsetof(bmfr_gbuffer, n_objects), offsetof(bmfr_prepared, prev_normals_moved), '
           '(int)BMFR_FORMAT_F16X2);return 0;}\n')
    c = tmp_path / "t.c"
    c.write_text(src)
    exe = str(tmp_path / "t")
    subprocess.run(["gcc", "-I", os.path.join(ROOT, "include"), str(c), "-o", exe], check=True)
    got = list(map(int, subprocess.run([exe], capture_output=True, text=True, check=True).stdout.split()))
    assert got == [C.sizeof(_lib.GBuffer), C.sizeof(_lib.Prepared), _lib.GBuffer.inv_view_proj.offset,
                   _lib.GBuffer.n_objects.offset, _lib.Prepared.prev_normals_moved.offset, _lib.FORMAT_F16X2]


def test_gbuffer_default():
    lib = _lib.load()
    g = _lib.GBuffer()
    C.memset(C.byref(g), 0xFF, C.sizeof(g))
    lib.bmfr_gbuffer_default(C.byref(g))
    assert F32(g.albedo_floor) == F32(1.0) / F32(255.0)
    assert tuple(g.motion_scale) == (1.0, 1.0)
    g.albedo_floor, g.motion_scale[0], g.motion_scale[1] = 0.0, 0.0, 0.0
    assert bytes(g) == bytes(C.sizeof(g))


def _call(g, out, ctx=None, jitter=True):
    lib = _lib.load()
    off = (C.c_float * 2)(0.5, 0.5)
    return lib.bmfr_prepare_frame(ctx, None, C.byref(g) if g is not None else None,
                                  C.byref(out) if out is not None else None, off if jitter else None)


def _gbuffer(**kw):
    g = _lib.GBuffer()
    _lib.load().bmfr_gbuffer_default(C.byref(g))
    for k, v in kw.items():
        setattr(g, k, v)
    return g


def test_argument_checks_need_no_device():
    """g and out are validated before the context is looked at: a missing
    input is status 1, an unlisted format status 2, and a call that passes
    both still fails with 1 on the NULL context (nothing is launched).  The
    plane pointers are never dereferenced by the checks."""
    P = 0x1000  # stands for a device plane
    full = dict(radiance=P, radiance_format=_lib.FORMAT_F16X4, albedo=P, albedo_format=_lib.FORMAT_UNORM8X4,
                normals=P, normal_format=_lib.FORMAT_OCT_SNORM16X2, depth=P, motion=P,
                motion_format=_lib.FORMAT_F16X2, prev_positions=P, prev_normals=P, prev_object_id=P,
                object_transforms=P, n_objects=3)
    everything = _lib.Prepared(P, P, P, P, P, P, P)
    assert _call(None, everything) == 1
    assert _call(_gbuffer(**full), None) == 1
    assert _call(_gbuffer(**full), everything, jitter=False) == 1
    assert _call(_gbuffer(**full), everything) == 1            # valid, but NULL ctx
    assert _call(_gbuffer(), _lib.Prepared()) == 1             # requests nothing, NULL ctx
    # each output without one of its inputs
    needs = {"noisy": ("radiance", "albedo"), "albedo": ("albedo",), "normals": ("normals",), "positions": ("depth",),
             "prev_pixel": ("motion",), "prev_positions_moved": ("prev_positions", "prev_object_id"),
             "prev_normals_moved": ("prev_normals", "prev_object_id")}
    for name, inputs in needs.items():
        for missing in inputs:
            kw = dict(full)
            kw[missing] = None
            # an unlisted format elsewhere does not mask the missing input: it is reported first
            kw["motion_format" if missing != "motion" else "normal_format"] = 99
            out = _lib.Prepared()
            setattr(out, name, P)
            assert _call(_gbuffer(**kw), out) == 1, (name, missing)
    # positions: either source will do
    kw = dict(full, positions=P, depth=None)
    assert _call(_gbuffer(**kw), _lib.Prepared(positions=P)) == 1   # passes the checks: NULL ctx
    for n in (-1, 65536):
        assert _call(_gbuffer(**dict(full, n_objects=n)), everything) == 1
    assert _call(_gbuffer(**dict(full, object_transforms=None)), everything) == 1
    # ids may be missing when there is no table
    assert _call(_gbuffer(**dict(full, prev_object_id=None, object_transforms=None, n_objects=0)), everything) == 1
    # formats not listed for a plane
    unlisted = {"radiance_format": (_lib.FORMAT_NONE, _lib.FORMAT_UNORM8X4, _lib.FORMAT_OCT_SNORM16X2,
                                    _lib.FORMAT_F32X2, 7, -1),
                "albedo_format": (_lib.FORMAT_NONE, _lib.FORMAT_OCT_SNORM16X2, _lib.FORMAT_F16X2),
                "normal_format": (_lib.FORMAT_NONE, _lib.FORMAT_UNORM8X4, _lib.FORMAT_F32X2),
                "motion_format": (_lib.FORMAT_NONE, _lib.FORMAT_F32X3, _lib.FORMAT_F16X4, 99)}
    for field, formats in unlisted.items():
        for fmt in formats:
            assert _call(_gbuffer(**dict(full, **{field: fmt})), everything) == 2, (field, fmt)
    # a NULL plane's format is not looked at
    assert _call(_gbuffer(**dict(full, motion=None, motion_format=99)), _lib.Prepared(normals=P)) == 1


def test_wrapper_checks_planes_before_the_call():
    """Denoiser.prepare_args refuses a plane the kernel would read out of
    bounds -- wrong dtype, wrong size, not on the GPU -- before any call that
    needs a device (a denoiser without a context stands in)."""
    import pytest
    import torch
    W, H = 100, 72
    den = bmfr_amd.Denoiser.__new__(bmfr_amd.Denoiser)
    den.lib, den.handle, den.device = _lib.load(), None, 0
    den.cfg = bmfr_amd.BmfrConfig(image_width=W, image_height=H)
    den.sizes = den.cfg.sizes()
    n = W * H
    with pytest.raises(TypeError, match="albedo"):
        den.prepare_args({"albedo": torch.zeros(n * 3, dtype=torch.float64)})
    with pytest.raises(TypeError, match="normals"):
        den.prepare_args({"normals": torch.zeros(n * 4, dtype=torch.uint8)})      # UNORM8X4 is for albedo only
    with pytest.raises(ValueError, match="elements"):
        den.prepare_args({"radiance": torch.zeros(n * 3, dtype=torch.float16)})   # RGBA16F has 4 per pixel
    with pytest.raises(ValueError, match="elements"):
        den.prepare_args({"depth": torch.zeros(n + 1)})
    with pytest.raises(ValueError, match="cuda"):
        den.prepare_args({"motion": torch.zeros(n * 2)})
    with pytest.raises(TypeError, match="prev_positions"):
        den.prepare_args({"prev_positions": torch.zeros(n * 3, dtype=torch.float16)})   # an f32 context's planes
    with pytest.raises(ValueError, match="object_transforms"):
        den.prepare_args({"object_transforms": torch.zeros(13)})
    with pytest.raises(TypeError):
        den.prepare_args({"albedo": np.zeros(n * 3, np.float32)})


def test_octahedral_round_trip():
    rng = np.random.RandomState(7)
    n = rng.normal(size=(20000, 3))
    n /= np.linalg.norm(n, axis=1, keepdims=True)
    axes = np.array([[1, 0, 0], [-1, 0, 0], [0, 1, 0], [0, -1, 0], [0, 0, 1], [0, 0, -1], [0.6, 0, -0.8]], float)
    n = np.concatenate([n, axes])
    enc = pn.oct_encode(n)
    dec = pn.oct_decode(enc)
    assert dec.dtype == F32
    assert np.abs(np.linalg.norm(dec.astype(np.float64), axis=1) - 1).max() < 1e-6
    assert np.abs(dec.astype(np.float64) - n).max() < 2 / 32767
    # every code decodes to a unit vector, -32768 like -32767
    codes = np.array([[-32768, 0], [-32768, -32768], [32767, 32767], [0, 0], [-32767, 5]], np.int16)
    d = pn.oct_decode(codes)
    assert np.abs(np.linalg.norm(d.astype(np.float64), axis=1) - 1).max() < 1e-6
    assert d[0].tobytes() == pn.oct_decode(np.array([[-32767, 0]], np.int16))[0].tobytes()


def test_motion_conventions():
    region = (3, 5, 40, 24)
    rng = np.random.RandomState(3)
    mv = rng.uniform(-9, 9, 40 * 24 * 2).astype(F32)
    x, y = pn.coords(region)
    # zero motion at the jittered sample: the pixel itself, exactly, whatever the jitter
    p = pn.prev_pixel_of(np.zeros_like(mv), (1, 1), 0, (0.3, 0.7), region)
    assert (p[:, 0] == x).all() and (p[:, 1] == y).all()
    # jitter (0.5, 0.5): the two conventions agree bit for bit
    a = pn.prev_pixel_of(mv, (1, 1), 0, (0.5, 0.5), region)
    b = pn.prev_pixel_of(mv, (1, 1), 1, (0.5, 0.5), region)
    assert np.abs(a.astype(np.float64) - b).max() <= 2.0 ** -18   # one rounding of x + 0.5 - m, |.| < 64
    exact = pn.prev_pixel_of(np.rint(mv * 4) / 4, (1, 1), 1, (0.5, 0.5), region)   # quarter-pixel vectors: no rounding
    assert exact.tobytes() == pn.prev_pixel_of(np.rint(mv * 4) / 4, (1, 1), 0, (0.5, 0.5), region).tobytes()
    # NDC vectors against the row direction scale by (W / 2, -H / 2)
    W, H = 128, 80
    ndc = (mv.reshape(-1, 2) / np.array([W / 2, -H / 2])).astype(F32).reshape(-1)
    c = pn.prev_pixel_of(ndc, (W / 2, -H / 2), 0, (0.5, 0.5), region)
    assert np.abs(c.astype(np.float64) - a).max() < 1e-4
    # half vectors widen exactly
    h = mv.astype(np.float16)
    assert pn.prev_pixel_of(h, (1, 1), 0, (0.1, 0.2), region).tobytes() == \
        pn.prev_pixel_of(h.astype(F32), (1, 1), 0, (0.1, 0.2), region).tobytes()


def test_demodulation_guard():
    alb = np.array([0.0, 1.0 / 1024, np.nan, 0.5, 1.0 / 255, 1.0], F32)
    rad = np.array([1.0, 2.0, 3.0, 4.0, 5.0, 6.0], F32)
    floor = F32(1.0) / F32(255.0)
    noisy, a = pn.demodulate(rad, alb, floor)
    assert a.tobytes() == alb.reshape(-1, 3).tobytes()   # the albedo output is not floored
    want = rad / np.array([floor, floor, floor, 0.5, floor, 1.0], F32)
    assert noisy.reshape(-1).tobytes() == want.tobytes() and np.isfinite(noisy).all()


def test_moved_planes():
    rng = np.random.RandomState(5)
    n = 64
    plane = rng.uniform(-4, 4, n * 3).astype(F32)
    ids = np.arange(n).astype(np.uint16) % 4
    ids[::7] = 0xFFFF
    tr = pn.random_transforms(3, rng).reshape(-1)
    got = pn.moved(plane, ids, tr, True).reshape(-1, 3)
    keep = ids >= 3
    assert got[keep].tobytes() == plane.reshape(-1, 3)[keep].tobytes()
    M = tr.reshape(3, 3, 4).astype(np.float64)
    for i in np.flatnonzero(~keep)[:10]:
        want = M[ids[i], :, :3] @ plane.reshape(-1, 3)[i] + M[ids[i], :, 3]
        assert np.abs(got[i] - want).max() < 1e-5
    assert pn.moved(plane, None, None, True).tobytes() == plane.tobytes()   # no table: a copy


def test_depth_convention_pin():
    """The restated depth -> position, pushed back through the library's
    reprojection (bmfr.cl:343-355, in f64) with the same frame's matrix and
    jitter, lands on the pixel itself: (x, y) within 0.01 px.  A wrong jitter
    sign, row direction or half-pixel would miss by >= 0.3 px with this jitter;
    f32 round-off at this size is orders of magnitude below the bound."""
    W, H, f = 128, 80, 2
    jitter = (0.3, 0.7)
    fr = bmfr_amd.synth_frame_host(W, H, f)
    vp, _ = bmfr_amd.synth_camera(W, H, f)
    depth, inv = pn.depth_and_inverse(fr["positions"], vp)
    region = (0, 0, W, H)
    pos = pn.position_from_depth(depth, inv, jitter, region, W, H).astype(np.float64)
    m = np.asarray(vp, np.float64)
    p4 = np.concatenate([pos, np.ones((W * H, 1))], axis=1)
    u = (p4 @ m[[0, 4, 8, 12]]) / (p4 @ m[[3, 7, 11, 15]])     # .s048c / .s37bf
    v = (p4 @ m[[1, 5, 9, 13]]) / (p4 @ m[[3, 7, 11, 15]])     # .s159d / .s37bf
    px = (u + 1) / 2 * W - jitter[0]
    py = (v + 1) / 2 * H - (1 - jitter[1])
    x, y = pn.coords(region)
    err = max(np.abs(px - x).max(), np.abs(py - y).max())
    print(f"depth -> position -> reprojection: max error {err:.2e} px")
    assert err < 0.01
    # and the scene's own depth at its own jitter gives back the scene's positions
    _, own = bmfr_amd.synth_camera(W, H, f)
    back = pn.position_from_depth(depth, inv, own, region, W, H)
    assert np.abs(back - fr["positions"].reshape(-1, 3)).max() < 0.05


def test_generated_gbuffers_cover_the_edge_cases():
    W, H = 128, 80
    fr = bmfr_amd.synth_frame_host(W, H, 1)
    vp, jit = bmfr_amd.synth_camera(W, H, 1)
    g = pn.make_gbuffer(fr, vp, W, H, (0, 0, W, H), 11, False, with_nan=True)
    a = g["albedo"]
    assert (a == 0).any() and np.isnan(a).any() and ((a > 0) & (a < 1 / 255)).any()
    ids = g["prev_object_id"]
    assert (ids == 0xFFFF).any() and (ids < 5).any() and ((ids >= 5) & (ids < 0xFFFF)).any()
    again = pn.make_gbuffer(fr, vp, W, H, (0, 0, W, H), 11, False, with_nan=True)
    for k in g:
        assert np.asarray(g[k]).tobytes() == np.asarray(again[k]).tobytes()
    out = pn.prepare(g, jit, (0, 0, W, H), W, H, False)
    assert set(out) == set(pn.OUTPUTS)
    assert np.isfinite(out["noisy"]).all()   # zero / tiny / NaN albedo all take the floor
    # every format's generator round-trips through the restatement's decoder
    rng = np.random.RandomState(1)
    c = rng.uniform(0, 1, (50, 3)).astype(F32)
    assert pn.channels(pn.rgba16(c, rng)).tobytes() == c.astype(np.float16).astype(F32).tobytes()
    assert np.abs(pn.channels(pn.unorm8(c, rng)) - c).max() <= 0.5 / 255 + 1e-7
