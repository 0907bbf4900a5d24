"""The output back end on the GPU (bmfr_resolve_output, include/bmfr.h;
Denoiser.resolve, tiling.resolve_tiled): the kernel against the numpy
restatement (tests/resolve_np.py) byte for byte on a constructed image written
into the context's state planes, every byte of the surface it must not write
still holding its sentinel, tiles against the untiled frame, and the real
output against copy_output."""
from __future__ import annotations

import ctypes as C
import functools
import itertools

import numpy as np
import pytest
import torch

import bmfr_amd
from bmfr_amd import _lib
from bmfr_amd.pipeline import hip_memcpy_d2d
from bmfr_amd.tiling import TileGrid, region_slice, resolve_tiled
import resolve_np as rn
from parity_harness import assert_same_array

pytestmark = pytest.mark.gpu

F32 = np.float32
ALPHA = 0.7   # quantises to 179 / 2 and is inexact in half: a swapped or dropped alpha shows
DTYPES = {rn.F32X3: (torch.float32, 3), rn.F16X4: (torch.float16, 4), rn.UNORM8X4: (torch.uint8, 4),
          rn.UNORM8X3: (torch.uint8, 3), rn.UNORM10X3A2: (torch.int32, None)}


def _cfg(W, H, **kw):
    return bmfr_amd.BmfrConfig(image_width=W, image_height=H, **kw)


def _first_frame(den, half: bool = False):
    """Frame 0 of the synthetic scene on the context's region."""
    W, H = den.cfg.image_width, den.cfg.image_height
    fr = bmfr_amd.synth_region_device(W, H, den.region, 0)
    if half:
        fr = {k: v.to(torch.float16) for k, v in fr.items()}
    vp, jit = bmfr_amd.synth_camera(W, H, 0)
    den.process_frame(fr["noisy"], fr["normals"], fr["positions"], fr["albedo"], vp, jit, 0)
    return fr


def _overwrite_state(den, result: np.ndarray, filtered: np.ndarray) -> None:
    """The constructed images (region pixels x 3, f32) into the context's
    result and filtered_accumulated planes, through the bmfr_state pointers."""
    sv = den.state()
    torch.cuda.synchronize()
    for ptr, img in ((sv.result, result), (sv.filtered_accumulated, filtered)):
        t = torch.from_numpy(np.ascontiguousarray(img, F32)).cuda()
        assert t.numel() * 4 == den.sizes.region_bytes
        hip_memcpy_d2d(ptr, t.data_ptr(), den.sizes.region_bytes)
        torch.cuda.synchronize()


@functools.lru_cache(maxsize=None)
def _images(W, H):
    """Full-frame constructed planes: result, filtered_accumulated, albedo (f32), albedo (half)."""
    n = W * H
    result, filtered = rn.constructed_image(n, 101), rn.constructed_image(n, 202)[::-1].copy()
    rng = np.random.RandomState(303)
    albedo = rng.uniform(-0.25, 1.5, (n, 3)).astype(F32)
    albedo[::97] = rng.normal(0, 300, (albedo[::97].shape)).astype(F32)   # products past half's range
    albedo[5::211, 1] = np.nan
    albedo[7::223, 2] = np.inf
    return result, filtered, albedo, albedo.astype(np.float16)


@functools.lru_cache(maxsize=None)
def _untiled(W, H, half):
    """A context after frame 0 whose state planes hold the constructed images."""
    den = bmfr_amd.Denoiser(_cfg(W, H, input_half=half))
    _first_frame(den, bool(half))
    result, filtered, alb32, alb16 = _images(W, H)
    _overwrite_state(den, result, filtered)
    albedo = torch.from_numpy(alb16 if half else alb32).cuda().reshape(-1)
    return den, albedo


def _values(W, H, source):
    """The restated source values of the full frame, (H, W, 3) f32."""
    result, filtered, alb32, alb16 = _images(W, H)
    v = {"output": result, "hdr": rn.hdr(alb32, filtered), "hdr_half": rn.hdr(alb16, filtered)}[source]
    return v.reshape(H, W, 3)


class Surface:
    """A surface inside a larger sentinel-filled byte buffer: guard bytes before
    and after, data `data_off` bytes past a 16-byte boundary, rows `pitch` apart."""

    def __init__(self, fmt, width, height, pad, data_off):
        self.fmt, self.width, self.height = fmt, width, height
        self.pitch = width * rn.BPP[fmt] + pad
        self.off = 2 * self.pitch // 16 * 16 + 16 + data_off   # at least a guard row in front
        self.size = self.off + (height + 2) * self.pitch + 16
        self.buf = torch.full((self.size,), rn.SENTINEL, dtype=torch.uint8, device="cuda")
        assert self.buf.data_ptr() % 16 == 0
        dt, ch = DTYPES[fmt]
        flat = self.buf[self.off:self.off + (self.size - self.off) // 8 * 8].view(dt)
        es = flat.element_size()
        assert self.pitch % es == 0
        shape, strides = ((height, width, ch), (self.pitch // es, ch, 1)) if ch else ((height, width), (self.pitch // es, 1))
        self.tensor = torch.as_strided(flat, shape, strides)
        assert self.tensor.data_ptr() == self.buf.data_ptr() + self.off

    def expected(self) -> np.ndarray:
        return np.full(self.size, rn.SENTINEL, np.uint8)

    def host(self) -> np.ndarray:
        torch.cuda.synchronize()
        return self.buf.cpu().numpy()

    def reset(self) -> None:
        self.buf.fill_(rn.SENTINEL)


def _compare(got: np.ndarray, want: np.ndarray, fmt, off, what, nan_in: bool):
    """Whole buffers byte for byte -- written pixels, pitch padding, guard rows
    and columns alike; float formats on inputs that hold NaN: NaN-aware on the
    buffer viewed as elements from the surface's first byte."""
    dt = rn.FLOAT_DTYPE.get(fmt)
    if dt is None or not nan_in:
        return assert_same_array(got, want, what)
    es = np.dtype(dt).itemsize
    a = off % es
    b = a + (got.size - a) // es * es
    assert_same_array(got[:a], want[:a], (what, "front"))
    assert_same_array(got[b:], want[b:], (what, "back"))
    assert_same_array(got[a:b].view(dt), want[a:b].view(dt), what, nan_aware=True)


LAYOUTS = list(itertools.product((0, 1), (0, 1), (0, 1)))   # padded pitch, data off a 16-byte boundary, larger surface


# ------------------------------------------------------------ untiled cases --
# 128 x 80: whole groups only; 101 x 75: row tails 1..3, rows that start off a group from the second on
@pytest.mark.parametrize("W,H", [(128, 80), (101, 75)])
@pytest.mark.parametrize("source", ["output", "hdr", "hdr_half"])
@pytest.mark.parametrize("fmt", list(rn.FORMATS))
def test_kernel_equals_restatement(fmt, source, W, H, gpu):
    f = rn.FORMATS[fmt]
    den, albedo = _untiled(W, H, int(source == "hdr_half"))
    v = _values(W, H, source)
    pad = {rn.UNORM8X3: 1, rn.F16X4: 8}.get(f, 4)
    for bgr in (False, True):
        pixels = rn.encode(v, f, bgr, ALPHA)
        for flip, (padded, shifted, larger) in itertools.product((False, True), LAYOUTS):
            s = Surface(f, W + 8 * larger, H + 8 * larger, pad * padded, rn.ALIGN[f] * shifted)
            origin = (5, 3) if larger else (0, 0)
            den.resolve(s.tensor, source="output" if source == "output" else "hdr", albedo=albedo, origin=origin,
                        flip_y=flip, bgr=bgr, alpha=ALPHA)
            want = rn.place(s.expected(), s.off, s.pitch, f, pixels, (0, 0, W, H), H, origin, flip)
            # F32X3 of the output plane carries the bits through, a NaN's payload included
            _compare(s.host(), want, f, s.off, (fmt, source, bgr, flip, padded, shifted, larger),
                     nan_in=not (f == rn.F32X3 and source == "output"))
    assert den.frame_status() == 0


def test_unaligned_albedo_takes_the_pixel_path(gpu):
    """An albedo plane one pixel into a larger allocation (element-aligned, not
    16-byte aligned): every pixel goes through the one-per-thread path, same bytes."""
    W, H = 101, 75
    den, albedo = _untiled(W, H, 0)
    big = torch.empty(albedo.numel() + 3, dtype=albedo.dtype, device="cuda")
    big[3:].copy_(albedo)
    assert big[3:].data_ptr() % 16 != 0
    v = _values(W, H, "hdr")
    for fmt, f in rn.FORMATS.items():
        s = Surface(f, W, H, 0, 0)
        den.resolve(s.tensor, source="hdr", albedo=big[3:], alpha=ALPHA)
        want = rn.place(s.expected(), s.off, s.pitch, f, rn.encode(v, f, False, ALPHA), (0, 0, W, H), H)
        _compare(s.host(), want, f, s.off, fmt, nan_in=True)


def test_a_format_holds_the_same_bytes_whichever_entry_point_wrote_it(gpu):
    """include/bmfr.h's promise, which csrc/bmfr_pixel_io.h keeps by being the
    only encoder: one frame through bmfr_resolve_output (HDR), through
    bmfr_upsample_output at ratio 1 (unguided, HDR, the frame's own albedo as
    the display albedo: the first tap has weight 1, the rest 0) and through
    bmfr_display_taa (reset, fed the tight F32X3 HDR resolve) leaves the same
    surface byte for byte in every format.  65 x 47: resolve's groups, heads
    and tails, and a partial 64-wide tile in the other two; bgr, flip_y, an
    origin inside a larger surface with a padded pitch; alpha 0.5, so that the
    alpha lane of the 8-, 10- and 16-bit formats is neither empty nor full.  The
    resolve's surface is itself held to the restatement."""
    W, H, alpha, origin = 65, 47, 0.5, (5, 3)
    den, albedo = _untiled(W, H, 0)
    current = Surface(rn.F32X3, W, H, 0, 0)
    den.resolve(current.tensor, source="hdr", albedo=albedo)
    result = torch.empty((H, W, 3), dtype=torch.float32, device="cuda")
    guides = {"width": W, "height": H, "albedo": albedo}
    kw = dict(origin=origin, flip_y=True, bgr=True, alpha=alpha)
    for fmt, f in rn.FORMATS.items():
        pad = {rn.UNORM8X3: 1, rn.F16X4: 8}.get(f, 4)
        resolved, upsampled, displayed = (Surface(f, W + 8, H + 8, pad, 0) for _ in range(3))
        den.resolve(resolved.tensor, source="hdr", albedo=albedo, **kw)
        den.upsample(upsampled.tensor, guides, source="hdr", **kw)
        den.display_taa(current.tensor, result, reset=True, dst=displayed.tensor, **kw)
        want = rn.place(resolved.expected(), resolved.off, resolved.pitch, f,
                        rn.encode(_values(W, H, "hdr"), f, True, alpha), (0, 0, W, H), H, origin, True)
        _compare(resolved.host(), want, f, resolved.off, (fmt, "resolve"), nan_in=True)
        want = resolved.host()
        _compare(upsampled.host(), want, f, resolved.off, (fmt, "upsample"), nan_in=True)
        _compare(displayed.host(), want, f, resolved.off, (fmt, "display_taa"), nan_in=True)
    assert den.frame_status() == 0


# -------------------------------------------------------------- tiled cases --
@functools.lru_cache(maxsize=None)
def _untiled_surfaces(W, H):
    """The untiled context's resolve of the constructed image per (format,
    source, flip_y), tight surfaces, as host bytes (H, W * bpp) -- themselves
    held to the restatement."""
    den, albedo = _untiled(W, H, 0)
    out = {}
    for (fmt, f), source, flip in itertools.product(rn.FORMATS.items(), ("output", "hdr"), (False, True)):
        s = Surface(f, W, H, 0, 0)
        den.resolve(s.tensor, source=source, albedo=albedo, flip_y=flip, bgr=True, alpha=ALPHA)
        got = s.host()
        want = rn.place(s.expected(), s.off, s.pitch, f, rn.encode(_values(W, H, source), f, True, ALPHA),
                        (0, 0, W, H), H, (0, 0), flip)
        _compare(got, want, f, s.off, ("untiled", fmt, source, flip), nan_in=True)
        out[fmt, source, flip] = got[s.off:s.off + H * s.pitch].reshape(H, s.pitch)
    return out


@pytest.mark.parametrize("halo", [34, 35, 36, 37])
@pytest.mark.parametrize("nx,ny", [(2, 1), (1, 2)])
def test_tiles_match_untiled(nx, ny, halo, gpu):
    """352 x 224 as 2 x 1 and 1 x 2 tiles: with halos 34..37 the second tile's
    first source pixel sits at every offset mod 4 inside its region.  Each tile
    into the whole-frame surface (resolve_tiled) and into a tile-sized surface
    with a negative origin: both equal the untiled context's resolve of the same
    image, cut accordingly; a tile leaves the rest of the whole-frame surface,
    its own halo's pixels included, at the sentinel."""
    W, H = 352, 224
    full = _untiled_surfaces(W, H)
    result, filtered, alb32, _ = _images(W, H)
    grid = TileGrid(W, H, nx, ny, halo=halo)
    dens = []
    for r in range(grid.ranks):
        den = bmfr_amd.Denoiser(_cfg(W, H, tile=grid.tile(r), tile_halo=halo))
        _first_frame(den)
        cut = lambda a: region_slice(torch.from_numpy(a), W, H, den.region).numpy().reshape(-1, 3)  # noqa: E731
        _overwrite_state(den, cut(result), cut(filtered))
        dens.append(den)
    offsets = {(d.cfg.tile[0] - d.region[0] + (d.cfg.tile[1] - d.region[1]) * d.region[2]) % 4 for d in dens}
    albedo = torch.from_numpy(alb32).cuda()
    for (fmt, f), source, flip in itertools.product(rn.FORMATS.items(), ("output", "hdr"), (False, True)):
        bpp = rn.BPP[f]
        want = full[fmt, source, flip]
        kw = dict(source=source, flip_y=flip, bgr=True, alpha=ALPHA)
        s = Surface(f, W, H, 0, 0)
        # one tile alone: its rectangle equals the untiled surface's, everything else is untouched
        for den in dens:
            s.reset()
            tx, ty, tw, th = den.cfg.tile
            y0 = H - ty - th if flip else ty
            resolve_tiled([den], s.tensor, albedo=albedo if source == "hdr" else None, **kw)
            got = s.host()
            alone = s.expected()[s.off:s.off + H * s.pitch].reshape(H, s.pitch)
            alone[y0:y0 + th, tx * bpp:(tx + tw) * bpp] = want[y0:y0 + th, tx * bpp:(tx + tw) * bpp]
            whole = s.expected()
            whole[s.off:s.off + H * s.pitch] = alone.reshape(-1)
            _compare(got, whole, f, s.off, ("tile alone", fmt, source, flip, den.cfg.tile), nan_in=True)
            # the tile-sized surface: origin = -tile (flipped: the frame's last row maps to H - 1 rows below it)
            t = Surface(f, tw, th, 0, 0)
            oy = -(H - ty - th) if flip else -ty
            den.resolve(t.tensor, albedo=region_slice(albedo, W, H, den.region).reshape(-1) if source == "hdr" else None,
                        origin=(-tx, oy), **kw)
            small = t.expected()
            small[t.off:t.off + th * t.pitch] = want[y0:y0 + th, tx * bpp:(tx + tw) * bpp].reshape(-1)
            _compare(t.host(), small, f, t.off, ("tile-sized", fmt, source, flip, den.cfg.tile), nan_in=True)
        # every tile into one surface: the untiled surface
        s.reset()
        resolve_tiled(dens, s.tensor, albedo=albedo if source == "hdr" else None, **kw)
        whole = s.expected()
        whole[s.off:s.off + H * s.pitch] = want.reshape(-1)
        _compare(s.host(), whole, f, s.off, ("composed", fmt, source, flip), nan_in=True)
    if nx == 2:
        assert halo % 4 in offsets   # the halo shifts the second tile's first source pixel
    for den in dens:
        assert den.frame_status() == 0


# -------------------------------------------------------------- end to end --
def test_output_f32x3_equals_copy_output(gpu):
    """128 x 80, 3 real frames: OUTPUT -> F32X3 with pitch W * 12 is copy_output, byte for byte."""
    W, H = 128, 80
    den = bmfr_amd.Denoiser(_cfg(W, H))
    for f in range(3):
        fr = bmfr_amd.synth_frame_device(W, H, f)
        vp, _ = bmfr_amd.synth_camera(W, H, max(f - 1, 0))
        _, jit = bmfr_amd.synth_camera(W, H, f)
        den.process_frame(fr["noisy"], fr["normals"], fr["positions"], fr["albedo"], vp, jit, f)
        dst = torch.full((H, W, 3), -1.0, dtype=torch.float32, device="cuda")
        assert dst.stride(0) * 4 == W * 12
        den.resolve(dst)
        want = den.copy_output(torch.empty(W * H * 3, device="cuda"))
        torch.cuda.synchronize()
        assert_same_array(dst.cpu().numpy().reshape(-1), want.cpu().numpy(), ("frame", f))
    assert den.frame_status() == 0


# ------------------------------------------------------------------ errors --
def test_errors_with_a_context_write_nothing(gpu):
    W, H = 128, 80
    lib = _lib.load()
    den = bmfr_amd.Denoiser(_cfg(W, H))
    s = Surface(rn.UNORM8X4, W, H, 4, 0)
    small = Surface(rn.UNORM8X4, W - 1, H, 0, 0)
    albedo = torch.zeros(W * H * 3, device="cuda")

    def refused(fn, surfaces=(s,)):
        with pytest.raises(bmfr_amd.BmfrError) as e:
            fn()
        assert e.value.status == 1
        for q in surfaces:
            assert_same_array(q.host(), q.expected(), "sentinel")

    refused(lambda: den.resolve(s.tensor))                                 # before the first frame
    frames = []
    for f in range(2):
        fr = bmfr_amd.synth_frame_device(W, H, f)
        vp, _ = bmfr_amd.synth_camera(W, H, max(f - 1, 0))
        _, jit = bmfr_amd.synth_camera(W, H, f)
        frames.append((fr["noisy"], fr["normals"], fr["positions"], fr["albedo"], vp, jit, f))
    den.process_frame(*frames[0])
    den.process_frame_interior(*frames[1])
    refused(lambda: den.resolve(s.tensor))                                 # between _interior and _border
    den.process_frame_border(*frames[1])
    refused(lambda: den.resolve(small.tensor), (small,))                   # the frame does not fit the surface
    refused(lambda: den.resolve(s.tensor, origin=(1, 0)))                  # pushed out to the right
    refused(lambda: den.resolve(s.tensor, origin=(0, -1)))                 # and out at the top
    refused(lambda: den.resolve(s.tensor, origin=(0, 1), flip_y=True))
    with pytest.raises(ValueError, match="albedo"):                        # the wrapper refuses first
        den.resolve(s.tensor, source="hdr")
    src, _, surf = den.resolve_args(s.tensor, source="hdr", albedo=albedo)
    st = lib.bmfr_resolve_output(den.handle, None, src, None, C.byref(surf))   # and the library: NULL albedo for HDR
    assert st == 1
    assert_same_array(s.host(), s.expected(), "sentinel")
    den.resolve(s.tensor)                                                  # the same surface is fine once all is in order
    assert (s.host() != rn.SENTINEL).any()
    assert den.frame_status() == 0
