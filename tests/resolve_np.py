"""numpy restatement of the output back end (bmfr_resolve_output, include/bmfr.h
"Output back end"): every line one np.float32 operation, as the header writes
them.  The GPU tests hold the kernel to this byte for byte."""
from __future__ import annotations

import numpy as np

F32 = np.float32
SENTINEL = 0xA5

# bmfr_format (include/bmfr.h)
F32X3, F16X4, UNORM8X4, UNORM8X3, UNORM10X3A2 = 1, 2, 3, 7, 8
FORMATS = {"f32x3": F32X3, "f16x4": F16X4, "unorm8x4": UNORM8X4, "unorm8x3": UNORM8X3, "unorm10x3a2": UNORM10X3A2}
BPP = {F32X3: 12, F16X4: 8, UNORM8X4: 4, UNORM8X3: 3, UNORM10X3A2: 4}
ALIGN = {F32X3: 4, F16X4: 8, UNORM8X4: 4, UNORM8X3: 1, UNORM10X3A2: 4}
FLOAT_DTYPE = {F32X3: np.float32, F16X4: np.float16}   # formats whose bytes can hold a NaN


def clamp01(v) -> np.ndarray:
    """c = v > 0 ? (v < 1 ? v : 1) : 0  (NaN -> 0)."""
    v = np.asarray(v, F32)
    with np.errstate(invalid="ignore"):
        return np.where(v > 0, np.where(v < 1, v, F32(1)), F32(0)).astype(F32)


def quantise(v, scale: float = 255.0) -> np.ndarray:
    """q = (uint)floorf(c * scale + 0.5f): the product rounded to f32, then the sum."""
    p = clamp01(v) * F32(scale)
    assert p.dtype == F32
    return np.floor(p + F32(0.5)).astype(np.uint32)


def quantise_f64(v, scale: float = 255.0) -> np.ndarray:
    """floor(c * scale + 0.5) in float64 (exact for every f32 c in [0, 1])."""
    return np.floor(clamp01(v).astype(np.float64) * scale + 0.5).astype(np.uint32)


def quantise_fused(v, scale: float = 255.0) -> np.ndarray:
    """What a contracted fma(c, scale, 0.5f) would give: the exact product and
    sum (float64 holds them for every f32 c in [0, 1]) rounded to f32 once."""
    return np.floor((clamp01(v).astype(np.float64) * scale + 0.5).astype(F32)).astype(np.uint32)


def to_half(v) -> np.ndarray:
    """(half)v: round to nearest even, overflow to +-inf, NaN stays NaN."""
    with np.errstate(over="ignore", invalid="ignore"):
        return np.asarray(v, F32).astype(np.float16)


def pack10(r, g, b, a) -> np.ndarray:
    r, g, b, a = (np.asarray(c, np.uint32) for c in (r, g, b, a))
    return (r | (g << np.uint32(10)) | (b << np.uint32(20)) | (a << np.uint32(30))).astype("<u4")


def unpack10(w):
    w = np.asarray(w, np.uint32)
    return w & 1023, (w >> 10) & 1023, (w >> 20) & 1023, w >> 30


def hdr(albedo, filtered) -> np.ndarray:
    """v = a * f; a half3 albedo widens exactly."""
    with np.errstate(all="ignore"):
        v = np.asarray(albedo).astype(F32) * np.asarray(filtered, F32)
    assert v.dtype == F32
    return v


def encode(v, fmt: int, bgr: bool = False, alpha: float = 1.0) -> np.ndarray:
    """(..., 3) f32 source values -> (..., bytes per pixel) uint8, little-endian."""
    v = np.asarray(v, F32)
    if bgr:
        v = v[..., ::-1]
    lead = v.shape[:-1]
    if fmt == F32X3:
        out = np.ascontiguousarray(v).view(np.uint8)
    elif fmt == F16X4:
        h = np.empty(lead + (4,), np.float16)
        h[..., :3] = to_half(v)
        h[..., 3] = to_half(F32(alpha))
        out = h.view(np.uint8)
    elif fmt in (UNORM8X4, UNORM8X3):
        q = quantise(v).astype(np.uint8)
        if fmt == UNORM8X4:
            q = np.concatenate([q, np.broadcast_to(quantise(F32(alpha)).astype(np.uint8), lead + (1,))], axis=-1)
        out = np.ascontiguousarray(q)
    elif fmt == UNORM10X3A2:
        q = quantise(v, 1023.0)
        w = pack10(q[..., 0], q[..., 1], q[..., 2], quantise(F32(alpha), 3.0))
        out = np.ascontiguousarray(w)[..., None].view(np.uint8)
    else:
        raise ValueError(fmt)
    return out.reshape(lead + (BPP[fmt],))


def place(buf: np.ndarray, data_off: int, pitch: int, fmt: int, pixels: np.ndarray, tile, H: int, origin=(0, 0),
          flip_y: bool = False) -> np.ndarray:
    """Write the encoded pixels (th, tw, bpp) of the tile (tx, ty, tw, th) of an
    H-row frame into the flat uint8 buffer, whose surface pixel (0, 0) is at
    byte data_off: frame pixel (x, y) -> surface pixel (origin_x + x,
    origin_y + (flip_y ? H - 1 - y : y)).  Nothing else is touched."""
    tx, ty, tw, th = tile
    bpp = BPP[fmt]
    assert pixels.shape == (th, tw, bpp) and buf.dtype == np.uint8 and buf.ndim == 1
    for r in range(th):
        y = ty + r
        row = origin[1] + (H - 1 - y if flip_y else y)
        start = data_off + row * pitch + (origin[0] + tx) * bpp
        buf[start:start + tw * bpp] = pixels[r].reshape(-1)
    return buf


def _with_neighbours(x: np.ndarray) -> np.ndarray:
    out = [x]
    lo = hi = x
    for _ in range(2):
        lo, hi = np.nextafter(lo, F32(-np.inf)), np.nextafter(hi, F32(np.inf))
        out += [lo, hi]
    return np.concatenate(out).astype(F32)


def structured(levels: int) -> np.ndarray:
    """All k / levels and (k + 0.5) / levels with their two f32 neighbours on each side."""
    k = np.arange(levels + 1, dtype=np.float64)
    x = np.concatenate([k / levels, (k + 0.5) / levels]).astype(F32)
    return _with_neighbours(x)


def specials() -> np.ndarray:
    tiny = np.array([1, 2, 0x7FFFFF, 0x800000, 0x80000001, 0x807FFFFF], np.uint32).view(F32)   # denormals, FLT_MIN
    return np.concatenate([np.array([0.0, -0.0, np.inf, -np.inf, np.nan, -np.nan], F32), tiny])


def dense_set(seed: int = 0x5E7, uniform: int = 100000) -> np.ndarray:
    """The inputs the quantisation is examined on: the 8-bit levels and their
    midpoints with f32 neighbours, `uniform` seeded values in [-0.5, 1.5],
    +-0, +-inf, NaN and denormals."""
    rng = np.random.RandomState(seed)
    return np.concatenate([structured(255), specials(), rng.uniform(-0.5, 1.5, uniform).astype(F32)])


def constructed_image(pixels: int, seed: int) -> np.ndarray:
    """(pixels, 3) f32 for a state plane: the 8- and 10-bit levels and midpoints
    with neighbours, the specials, values above half's range and at its
    rounding boundaries, a seeded normal field, then the uniform part of the
    dense set -- repeated to fill the plane (truncated when the plane is small:
    the structured parts come first)."""
    rng = np.random.RandomState(seed)
    big = np.array([65504.0, 65519.996, 65520.0, 65536.0, 1e5, -1e5, 7e4, 3.4e38, -65520.0, 6.1e-5, 5.96e-8, 2.98e-8,
                    2.9802326e-08, 1.0009766, 1.00048828125, 2049.0, 2051.0], F32)
    base = np.concatenate([structured(255), structured(1023), specials(), big,
                           rng.normal(0.4, 0.6, 2000).astype(F32), rng.uniform(-0.5, 1.5, 100000).astype(F32)])
    return np.resize(base, pixels * 3).reshape(pixels, 3).astype(F32)
