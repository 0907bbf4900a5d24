"""The output back end (bmfr_resolve_output, include/bmfr.h), the parts that
need no GPU: the struct layout, the argument checks, and properties of the
numpy restatement (tests/resolve_np.py) the GPU tests hold the kernel to."""
from __future__ import annotations

import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import bmfr_amd
from bmfr_amd import _lib
import resolve_np as rn

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
F32 = np.float32
P = 0x10000   # stands for a device surface, aligned to anything


def test_struct_matches_header(tmp_path):
    """The ctypes mirror of bmfr_surface has the header's size and field offsets; the new format codes."""
    fields = [n for n, _ in _lib.Surface._fields_]
    src = ('#include <stdio.h>\n#include <stddef.h>\n#include "bmfr.h"\nint main(void){printf("%zu ", sizeof(bmfr_surface));\n'
           + "".join(f'printf("%zu ", offsetof(bmfr_surface, {n}));\n' for n in fields)
           + 'printf("%d %d %d %d %d %d", (int)BMFR_FORMAT_F16X2, (int)BMFR_FORMAT_UNORM8X3, (int)BMFR_FORMAT_UNORM10X3A2, '
             '(int)BMFR_RESOLVE_OUTPUT, (int)BMFR_RESOLVE_HDR, (int)BMFR_FORMAT_UNORM8X4);return 0;}\n')
    c = tmp_path / "t.c"
    c.write_text(src)
    exe = str(tmp_path / "t")
    subprocess.run(["gcc", "-I", os.path.join(ROOT, "include"), str(c), "-o", exe], check=True)
    got = list(map(int, subprocess.run([exe], capture_output=True, text=True, check=True).stdout.split()))
    assert got == [C.sizeof(_lib.Surface)] + [getattr(_lib.Surface, n).offset for n in fields] + \
        [_lib.FORMAT_F16X2, _lib.FORMAT_UNORM8X3, _lib.FORMAT_UNORM10X3A2, _lib.RESOLVE_OUTPUT, _lib.RESOLVE_HDR,
         _lib.FORMAT_UNORM8X4]
    # existing values keep their numbers; the restatement uses the same codes
    assert (_lib.FORMAT_F16X2, _lib.FORMAT_UNORM8X3, _lib.FORMAT_UNORM10X3A2) == (6, 7, 8)
    assert rn.FORMATS == {"f32x3": _lib.FORMAT_F32X3, "f16x4": _lib.FORMAT_F16X4, "unorm8x4": _lib.FORMAT_UNORM8X4,
                          "unorm8x3": _lib.FORMAT_UNORM8X3, "unorm10x3a2": _lib.FORMAT_UNORM10X3A2}


def test_surface_default():
    lib = _lib.load()
    s = _lib.Surface()
    C.memset(C.byref(s), 0xFF, C.sizeof(s))
    lib.bmfr_surface_default(C.byref(s))
    assert s.alpha == 1.0
    s.alpha = 0.0
    assert bytes(s) == bytes(C.sizeof(s))
    lib.bmfr_surface_default(None)   # a NULL surface is not a crash


def _surface(**kw):
    s = _lib.Surface()
    _lib.load().bmfr_surface_default(C.byref(s))
    base = dict(data=P, format=_lib.FORMAT_UNORM8X4, pitch=64 * 4, width=64, height=48)
    base.update(kw)
    for k, v in base.items():
        setattr(s, k, v)
    return s


def _call(s, source=_lib.RESOLVE_OUTPUT, albedo=None):
    return _lib.load().bmfr_resolve_output(None, None, source, albedo, C.byref(s) if s is not None else None)


def test_argument_checks_need_no_device():
    """dst, source and albedo are validated before the context is looked at: a
    bad surface is status 1, a format outside the five status 2, and a call
    that passes both still fails with 1 on the NULL context.  The pointers are
    never dereferenced by the checks."""
    bpp = {_lib.FORMAT_F32X3: 12, _lib.FORMAT_F16X4: 8, _lib.FORMAT_UNORM8X4: 4, _lib.FORMAT_UNORM8X3: 3,
           _lib.FORMAT_UNORM10X3A2: 4}
    align = {_lib.FORMAT_F32X3: 4, _lib.FORMAT_F16X4: 8, _lib.FORMAT_UNORM8X4: 4, _lib.FORMAT_UNORM8X3: 1,
             _lib.FORMAT_UNORM10X3A2: 4}
    assert _call(None) == 1
    assert _call(_surface(data=None)) == 1
    for fmt, b in bpp.items():
        ok = dict(format=fmt, pitch=64 * b)
        assert _call(_surface(**ok)) == 1                                   # passes the checks: NULL ctx
        assert _call(_surface(**ok), _lib.RESOLVE_HDR, P) == 1              # idem
        assert _call(_surface(**dict(ok, pitch=64 * b + 8 * align[fmt]))) == 1   # a padded pitch passes too
        assert _call(_surface(**dict(ok, pitch=64 * b - align[fmt]))) == 1  # pitch < width * bytes per pixel
        assert _call(_surface(**dict(ok, width=0))) == 1
        assert _call(_surface(**dict(ok, height=0))) == 1
        assert _call(_surface(**dict(ok, width=-3))) == 1
        assert _call(_surface(**dict(ok, height=-1))) == 1
        if align[fmt] > 1:
            for off in range(1, align[fmt]):
                assert _call(_surface(**dict(ok, data=P + off))) == 1, (fmt, off)           # data off its alignment
                assert _call(_surface(**dict(ok, pitch=64 * b + off))) == 1, (fmt, off)     # pitch off its alignment
        for source in (-1, 2, 99):
            assert _call(_surface(**ok), source, P) == 1
        assert _call(_surface(**ok), _lib.RESOLVE_HDR, None) == 1           # HDR needs the albedo
    # UNORM8X3 takes any address and any pitch that holds a row
    assert _call(_surface(format=_lib.FORMAT_UNORM8X3, data=P + 1, pitch=64 * 3 + 1)) == 1
    # formats outside the five: unsupported, reported whatever else is wrong after the surface itself
    for fmt in (_lib.FORMAT_NONE, _lib.FORMAT_OCT_SNORM16X2, _lib.FORMAT_F32X2, _lib.FORMAT_F16X2, 9, -1, 99):
        assert _call(_surface(format=fmt)) == 2, fmt
    # which of two answers a call gets is told apart by the surface that passes: make the
    # distinction visible with one that can only fail on the context
    assert _call(_surface()) == 1 and _call(_surface(format=9)) == 2


def test_prepare_frame_refuses_the_surface_formats():
    """The two new codes are output formats: bmfr_prepare_frame keeps answering unsupported for them."""
    lib = _lib.load()
    off = (C.c_float * 2)(0.5, 0.5)
    for fmt in (_lib.FORMAT_UNORM8X3, _lib.FORMAT_UNORM10X3A2):
        for field, plane in (("radiance_format", "radiance"), ("albedo_format", "albedo"), ("normal_format", "normals"),
                             ("motion_format", "motion")):
            g = _lib.GBuffer()
            lib.bmfr_gbuffer_default(C.byref(g))
            setattr(g, plane, P)
            setattr(g, field, fmt)
            out = _lib.Prepared()
            assert lib.bmfr_prepare_frame(None, None, C.byref(g), C.byref(out), off) == 2, (fmt, field)


def test_wrapper_checks_the_surface_before_the_call():
    """Denoiser.resolve_args refuses a surface the kernel would write out of
    bounds -- wrong dtype, shape, device, inner strides -- and an albedo of the
    wrong size, before any call that needs a device."""
    import torch
    W, H = 100, 72
    den = bmfr_amd.Denoiser.__new__(bmfr_amd.Denoiser)
    den.lib, den.handle, den.device = _lib.load(), None, 0
    den.cfg = bmfr_amd.BmfrConfig(image_width=W, image_height=H)
    den.sizes = den.cfg.sizes()
    with pytest.raises(TypeError, match="dst"):
        den.resolve_args(np.zeros((H, W, 4), np.uint8))
    with pytest.raises(TypeError, match="dst"):
        den.resolve_args(torch.zeros((H, W, 4), dtype=torch.float32))     # RGBA32F is not a surface format
    with pytest.raises(TypeError, match="dst"):
        den.resolve_args(torch.zeros((H, W, 3), dtype=torch.float16))     # nor RGB16F
    with pytest.raises(TypeError, match="dst"):
        den.resolve_args(torch.zeros((H, W), dtype=torch.uint8))
    with pytest.raises(TypeError, match="dst"):
        den.resolve_args(torch.zeros((H * W * 4,), dtype=torch.uint8))
    with pytest.raises(ValueError, match="cuda"):
        den.resolve_args(torch.zeros((H, W, 4), dtype=torch.uint8))       # a host tensor
    with pytest.raises(ValueError, match="cuda"):
        den.resolve_args(torch.zeros((H, W), dtype=torch.int32))
    whole = torch.zeros((H, W, 4), dtype=torch.uint8)
    for bad in (whole[:, :, :3],                                          # a channel slice: pixels not packed
                whole.transpose(0, 1),                                    # columns for rows
                whole[:, :1].expand(H, W, 4),                             # rows that overlap
                torch.zeros((H, 2 * W), dtype=torch.int32)[:, ::2]):      # every other word
        with pytest.raises(ValueError, match="packed"):
            den.resolve_args(bad)
    with pytest.raises(ValueError, match="source"):
        den.resolve_args(whole, source="linear")
    with pytest.raises(ValueError, match="albedo"):
        den.resolve_args(whole, source="hdr")
    with pytest.raises(ValueError, match="elements"):
        den.resolve_args(whole, source="hdr", albedo=torch.zeros(W * H * 3 - 3))
    with pytest.raises(TypeError, match="albedo"):
        den.resolve_args(whole, source="hdr", albedo=torch.zeros(W * H * 3, dtype=torch.float16))   # an f32 context


# ---------------------------------------------------- the restatement itself --
def _rounds_onto_an_integer(c, scale):
    """Where the f32 sum fl(fl(c * scale) + 0.5f) is an integer k + 1 although
    the exact c * scale + 0.5 is below it: the roundings carried the value up
    onto the integer.  The one place where one rounding per operation and exact
    arithmetic part ways."""
    c32 = rn.clamp01(c)
    s32 = (c32 * F32(scale) + F32(0.5)).astype(np.float64)
    return (s32 == np.floor(s32)) & (c32.astype(np.float64) * scale + 0.5 < s32)


def test_quantisation_against_float64():
    """q = floorf(c * 255.0f + 0.5f) against floor(c * 255 + 0.5) in float64 on
    the dense set (all k / 255 and (k + 0.5) / 255 with two f32 neighbours on
    each side, 1e5 seeded uniforms in [-0.5, 1.5], +-0, +-inf, NaN, denormals).

    The two agree on every value EXCEPT where the f32 roundings carry the sum
    up onto an integer k + 1 exactly (the exact product lies below k + 0.5 by
    less than half an ulp): there the f32 rule -- which is bmfr_png_write_rgb's, and what the PNG files pin --
    gives k + 1 and float64 gives k.  On this set those are 128 values, each the
    f32 nearest to (k + 0.5) / 255 for some k >= 128; measured over every f32
    within 20000 ulps of every midpoint (1.0e7 values) the same 128 and no
    other.  So "equal to float64" does not hold as an identity; what holds, and
    is asserted, is equality off those ties and k + 1 on them."""
    d = rn.dense_set()
    assert d.size > 102000 and np.isnan(d).any() and np.isinf(d).any()
    q, q64 = rn.quantise(d), rn.quantise_f64(d)
    assert q.max() == 255 and q.min() == 0
    tie = _rounds_onto_an_integer(d, 255.0)
    print(f"8-bit: {np.count_nonzero(q != q64)} of {d.size} values differ from float64, {np.count_nonzero(tie)} ties")
    assert (q[~tie] == q64[~tie]).all()
    assert (q[tie] == q64[tie] + 1).all()
    assert 0 < np.count_nonzero(tie) <= 256
    # NaN, negatives and -0 quantise to 0, +inf and everything from 1 up to 255
    sp = np.array([np.nan, -np.nan, -0.0, 0.0, -1e-30, -np.inf, np.inf, 1.0, 1.5, 3e38], F32)
    assert rn.quantise(sp).tolist() == [0, 0, 0, 0, 0, 0, 255, 255, 255, 255]
    assert rn.quantise(sp, 1023.0).tolist()[6:] == [1023] * 4
    # exact levels map to themselves and the level spacing is respected
    k = np.arange(256)
    assert (rn.quantise((k / 255.0).astype(F32)) == k).all()
    k = np.arange(1024)
    assert (rn.quantise((k / 1023.0).astype(F32), 1023.0) == k).all()


def test_contraction_cannot_show_in_the_unorm_formats():
    """The header says "never contracted".  For the quantisation that rule has
    no observable consequence: a fused fma(c, 255, 0.5f) gives the same integer
    as the two-rounding form on every value of the dense set, and the same for
    1023 -- and over every f32 within 20000 ulps of every (k + 0.5) / 255 and
    (k + 0.5) / 1023 (5.1e7 values, measured once) there is no difference
    either.  Reason: the two can only part where the sum is within half an ulp
    of an integer k + 1; there the product lies within half an ulp of k + 0.5,
    whose ulp is never larger than the sum's, so both round onto k + 1.  A
    value on which they differ, which the GPU comparison could then catch, does
    not exist for either scale; the GPU tests pin the bytes, and this test pins
    that the two forms are indistinguishable (what a contracted build would
    have to match anyway)."""
    d = rn.dense_set()
    for scale in (255.0, 1023.0, 3.0):
        assert (rn.quantise(d, scale) == rn.quantise_fused(d, scale)).all(), scale
        mids = ((np.arange(int(scale) + 1) + 0.5) / scale).astype(F32)
        near = (mids.view(np.uint32).astype(np.int64)[:, None] + np.arange(-64, 65)[None, :]).astype(np.uint32).view(F32)
        assert (rn.quantise(near, scale) == rn.quantise_fused(near, scale)).all(), scale


def test_ten_bit_packing_round_trips():
    rng = np.random.RandomState(9)
    r, g, b = (rng.randint(0, 1024, 5000).astype(np.uint32) for _ in range(3))
    a = rng.randint(0, 4, 5000).astype(np.uint32)
    w = rn.pack10(r, g, b, a)
    assert w.dtype == np.dtype("<u4")
    for got, want in zip(rn.unpack10(w), (r, g, b, a)):
        assert (got == want).all()
    # through the encoder: bytes are the little-endian word, bgr swaps bits 0-9 with 20-29
    v = rng.uniform(-0.2, 1.2, (300, 3)).astype(F32)
    for bgr in (False, True):
        e = rn.encode(v, rn.UNORM10X3A2, bgr, 0.6)
        word = e[:, 0].astype(np.uint32) | e[:, 1].astype(np.uint32) << 8 | e[:, 2].astype(np.uint32) << 16 | \
            e[:, 3].astype(np.uint32) << 24
        c0, c1, c2, al = rn.unpack10(word)
        q = rn.quantise(v, 1023.0)
        assert (c0 == q[:, 2 if bgr else 0]).all() and (c1 == q[:, 1]).all() and (c2 == q[:, 0 if bgr else 2]).all()
        assert (al == 2).all()   # floor(0.6 * 3 + 0.5)


def test_encodings():
    v = np.array([[0.0, 0.5, 1.0], [np.nan, 70000.0, -70000.0], [65519.996, 65520.0, 1e-8]], F32)
    h = rn.encode(v, rn.F16X4, False, 0.7).view(np.float16).reshape(3, 4)
    assert h[0].tolist()[:3] == [0.0, 0.5, 1.0] and h[0, 3] == np.float16(0.7)
    assert np.isnan(h[1, 0]) and h[1, 1] == np.inf and h[1, 2] == -np.inf
    assert h[2, 0] == np.float16(65504) and h[2, 1] == np.inf and h[2, 2] == 0   # the tie at 65520 goes to even: inf
    assert rn.encode(v, rn.F32X3).tobytes() == v.tobytes()
    assert rn.encode(v, rn.F32X3, True).tobytes() == v[:, ::-1].tobytes()
    e = rn.encode(v, rn.UNORM8X4, True, 0.7)
    assert e[0].tolist() == [255, 128, 0, 179] and e[1].tolist() == [0, 255, 0, 179]
    assert rn.encode(v, rn.UNORM8X3, True).tolist() == e[:, :3].tolist()
    # a half3 albedo widens exactly; the product is one f32 multiply
    a = np.array([0.1, 0.2, 0.3], np.float16)
    f = np.array([3.0, 5.0, 7.0], F32)
    assert rn.hdr(a, f).tobytes() == (a.astype(F32) * f).tobytes()


def test_place_touches_only_the_tile():
    W, H = 12, 7
    tile = (4, 2, 5, 3)
    px = np.arange(3 * 5 * 3, dtype=np.uint8).reshape(3, 5, 3)
    for flip in (False, True):
        buf = np.full(16 + (H + 8) * ((W + 8) * 3 + 1), rn.SENTINEL, np.uint8)
        pitch = (W + 8) * 3 + 1
        rn.place(buf, 16, pitch, rn.UNORM8X3, px, tile, H, (5, 3), flip)
        rows = buf[16:16 + (H + 8) * pitch].reshape(H + 8, pitch)
        y0 = 3 + (H - 2 - 3 if flip else 2)
        block = rows[y0:y0 + 3, (5 + 4) * 3:(5 + 4 + 5) * 3].reshape(3, 5, 3)
        assert (block == (px[::-1] if flip else px)).all()
        rows[y0:y0 + 3, (5 + 4) * 3:(5 + 4 + 5) * 3] = rn.SENTINEL
        assert (buf == rn.SENTINEL).all()
