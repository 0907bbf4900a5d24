"""EXR / PNG I/O of the host (host/image_io.cpp), checked
against an independent numpy + zlib implementation of the same published
formats (tests/exr_write_py.py): OpenEXR 2 scanline and tiled files (HALF / FLOAT
channels, NONE / RLE / ZIPS / ZIP / PXR24 / B44 / B44A compression, PIZ
through the independent encoder tests/exr_piz_py.py and DWAA / DWAB through
tests/exr_dwa_py.py; one-level and mip-mapped tiles) and
8-bit RGB PNG.  EXR parity is unpinned: no OpenEXR library and no reference
.exr file exist here, so the reader is only as right as these encoders'
reading of the published format."""
from __future__ import annotations

import ctypes as C
import os
import struct
import zlib

import numpy as np
import pytest

from bmfr_amd import _build
import exr_dwa_py
import exr_piz_py
from exr_write_py import (B44_DECODED, B44_SHIFTS, DWA_DECODED, DWA_OPTS, RAW_CHUNKS, _b44_ordered, _dwa_image, _img,
                          f24_values, write_exr_py)

LIB = None


def lib():
    global LIB
    if LIB is None:
        _build.build_host()
        LIB = C.CDLL(_build.IO_LIB)
        LIB.bmfr_exr_info.argtypes = [C.c_char_p, C.POINTER(C.c_int), C.POINTER(C.c_int), C.POINTER(C.c_int)]
        LIB.bmfr_exr_read_rgb.argtypes = [C.c_char_p, C.c_int, C.c_int, C.c_void_p]
        LIB.bmfr_exr_write_rgb.argtypes = [C.c_char_p, C.c_int, C.c_int, C.c_void_p, C.c_size_t, C.c_int]
        LIB.bmfr_png_write_rgb.argtypes = [C.c_char_p, C.c_int, C.c_int, C.c_void_p, C.c_size_t]
        LIB.bmfr_io_error.restype = C.c_char_p
    return LIB


def read_exr_py(path):
    """Independent decoder for the FLOAT/NONE/ZIP files the host writes."""
    b = open(path, "rb").read()
    assert struct.unpack_from("<I", b, 0)[0] == 20000630
    p, attrs = 8, {}
    while b[p]:
        e = b.index(b"\0", p)
        name = b[p:e].decode()
        e2 = b.index(b"\0", e + 1)
        size = struct.unpack_from("<i", b, e2 + 1)[0]
        attrs[name] = b[e2 + 5:e2 + 5 + size]
        p = e2 + 5 + size
    p += 1
    x0, y0, x1, y1 = struct.unpack("<iiii", attrs["dataWindow"])
    W, H = x1 - x0 + 1, y1 - y0 + 1
    comp = attrs["compression"][0]
    lpc = 16 if comp == 3 else 1
    n_chunks = (H + lpc - 1) // lpc
    offs = struct.unpack_from(f"<{n_chunks}Q", b, p)
    out = np.zeros((H, W, 3), np.float32)
    for o in offs:
        y, size = struct.unpack_from("<ii", b, o)
        data = b[o + 8:o + 8 + size]
        lines = min(lpc, H - y)
        raw_size = lines * W * 12
        if size < raw_size:
            t = np.frombuffer(zlib.decompress(data), np.uint8).astype(np.int64)
            t = (t[0] + np.concatenate([[0], np.cumsum(t[1:] - 128)])) & 255  # undo the delta predictor
            half = (len(t) + 1) // 2
            r = np.empty(len(t), np.uint8)
            r[0::2] = t[:half]
            r[1::2] = t[half:]
            data = r.tobytes()
        a = np.frombuffer(data, np.float32).reshape(lines, 3, W)  # B, G, R
        out[y:y + lines] = a[:, ::-1, :].transpose(0, 2, 1)
    return out


def read_png_py(path):
    b = open(path, "rb").read()
    assert b[:8] == b"\x89PNG\r\n\x1a\n"
    p, idat, W = 8, b"", 0
    while p < len(b):
        n = struct.unpack(">I", b[p:p + 4])[0]
        typ, data = b[p + 4:p + 8], b[p + 8:p + 8 + n]
        assert zlib.crc32(typ + data) == struct.unpack(">I", b[p + 8 + n:p + 12 + n])[0]
        if typ == b"IHDR":
            W, H, depth, ctype = struct.unpack(">IIBB", data[:10])
            assert (depth, ctype) == (8, 2)
        elif typ == b"IDAT":
            idat += data
        p += 12 + n
    rows = np.frombuffer(zlib.decompress(idat), np.uint8).reshape(H, 1 + 3 * W)
    assert (rows[:, 0] == 0).all()
    return rows[:, 1:].reshape(H, W, 3)


# ------------------------------------------------------------------ tests --
@pytest.mark.parametrize("comp", [0, 3])
def test_exr_write_read_roundtrip(tmp_path, comp):
    img = _img()
    H, W, _ = img.shape
    path = str(tmp_path / f"rt{comp}.exr").encode()
    assert lib().bmfr_exr_write_rgb(path, W, H, img.ctypes.data, W * 3, comp) == 0, lib().bmfr_io_error()
    w, h, c = C.c_int(), C.c_int(), C.c_int()
    assert lib().bmfr_exr_info(path, C.byref(w), C.byref(h), C.byref(c)) == 0
    assert (w.value, h.value, c.value) == (W, H, 3)
    back = np.empty_like(img)
    assert lib().bmfr_exr_read_rgb(path, W, H, back.ctypes.data) == 0, lib().bmfr_io_error()
    assert back.tobytes() == img.tobytes()
    # an independent decoder reads the same values
    assert read_exr_py(path.decode()).tobytes() == img.tobytes()


@pytest.mark.parametrize("comp", [0, 1, 2, 3, 4])
@pytest.mark.parametrize("half", [False, True])
def test_exr_reader_against_reference_encoder(tmp_path, comp, half):
    img = _img(41, 29, seed=comp + 7 * half)
    chans = {"R": img[..., 0], "G": img[..., 1], "B": img[..., 2], "A": np.ones(img.shape[:2], np.float32)}
    path = str(tmp_path / f"ref{comp}{int(half)}.exr")
    write_exr_py(path, chans, comp, half)
    H, W, _ = img.shape
    out = np.empty_like(img)
    assert lib().bmfr_exr_read_rgb(path.encode(), W, H, out.ctypes.data) == 0, lib().bmfr_io_error()
    want = img.astype(np.float16).astype(np.float32) if half else img
    np.testing.assert_array_equal(out, want)


def test_exr_errors(tmp_path):
    p = tmp_path / "bad.exr"
    p.write_bytes(b"not an exr file at all")
    out = np.empty(3, np.float32)
    assert lib().bmfr_exr_read_rgb(str(p).encode(), 1, 1, out.ctypes.data) != 0
    assert b"OpenEXR" in lib().bmfr_io_error()
    img = _img(8, 8)
    path = str(tmp_path / "wrongsize.exr").encode()
    assert lib().bmfr_exr_write_rgb(path, 8, 8, img.ctypes.data, 24, 0) == 0
    big = np.empty((9, 8, 3), np.float32)
    assert lib().bmfr_exr_read_rgb(path, 8, 9, big.ctypes.data) != 0


def test_png_quantisation(tmp_path):
    img = _img(23, 31)
    img[3, 3] = [np.nan, 0.5, 1.5]
    H, W, _ = img.shape
    path = str(tmp_path / "o.png").encode()
    assert lib().bmfr_png_write_rgb(path, W, H, img.ctypes.data, W * 3) == 0, lib().bmfr_io_error()
    got = read_png_py(path.decode())
    want = np.floor(np.clip(np.nan_to_num(img, nan=0.0), 0, 1) * 255 + 0.5).astype(np.uint8)
    np.testing.assert_array_equal(got, want)


@pytest.mark.parametrize("shape", [(1, 1), (33, 70), (7, 300), (64, 5), (40, 300)])
@pytest.mark.parametrize("half", [False, True])
def test_exr_piz_shapes(tmp_path, shape, half):
    """PIZ: partial last chunks, one-pixel and very wide / narrow images (odd
    wavelet rows / columns at every level), smooth data (14-bit wavelet,
    long runs) and noise (16-bit wavelet: many distinct words)."""
    H, W = shape
    rng = np.random.default_rng(H * 1000 + W)
    yy, xx = np.mgrid[0:H, 0:W].astype(np.float32)
    smooth = (np.sin(xx / 9.0) + yy / 50.0).astype(np.float32)
    img = np.stack([smooth, rng.normal(0, 10, (H, W)).astype(np.float32), np.zeros((H, W), np.float32)], -1)
    img[:, :, 2][::3] = 0.5  # runs
    chans = {"R": img[..., 0], "G": img[..., 1], "B": img[..., 2]}
    path = str(tmp_path / "piz.exr")
    exr_piz_py.MAX_VALUES.clear()
    write_exr_py(path, chans, 4, half)
    if shape == (40, 300) and not half:  # both wavelet forms: the first chunk 16-bit, the 8-line tail 14-bit
        assert max(exr_piz_py.MAX_VALUES) >= 1 << 14 and min(exr_piz_py.MAX_VALUES) < 1 << 14
    out = np.empty_like(img)
    assert lib().bmfr_exr_read_rgb(path.encode(), W, H, out.ctypes.data) == 0, lib().bmfr_io_error()
    want = img.astype(np.float16).astype(np.float32) if half else img
    np.testing.assert_array_equal(out, want)


@pytest.mark.parametrize("half", [False, True])
@pytest.mark.parametrize("shape", [(41, 29), (16, 16), (1, 70), (33, 1)])
def test_exr_pxr24(tmp_path, shape, half):
    """PXR24 (OpenImageIO reads it, bmfr.cpp:145-163): lossless for HALF,
    FLOAT samples rounded to 24 bits (f24_values); partial 16-line chunks."""
    H, W = shape
    img = np.random.default_rng(H + W).normal(0, 3, (H, W, 3)).astype(np.float32)
    img[0, 0] = [np.inf, -0.0, np.float32(1.0 + 2 ** -16)]  # the dropped byte's top bit: rounds up
    img[-1, -1] = [np.nan, 65504.0, np.float32(3.4028235e38)]  # NaN; no rounding into infinity
    chans = {"R": img[..., 0], "G": img[..., 1], "B": img[..., 2]}
    path = str(tmp_path / "pxr24.exr")
    RAW_CHUNKS.clear()
    write_exr_py(path, chans, 5, half)
    out = np.empty_like(img)
    assert lib().bmfr_exr_read_rgb(path.encode(), W, H, out.ctypes.data) == 0, lib().bmfr_io_error()
    want = img.astype(np.float16).astype(np.float32) if half else f24_values(img)
    for _, y0, n, x0, w in RAW_CHUNKS if not half else []:  # FLOAT chunks stored uncompressed: exact
        want[y0:y0 + n, x0:x0 + w] = img[y0:y0 + n, x0:x0 + w]
    np.testing.assert_array_equal(out, want)


@pytest.mark.parametrize("comp", [0, 1, 3, 4, 5])
@pytest.mark.parametrize("tile,mipmap", [((16, 16), False), ((32, 8), False), ((64, 64), False),
                                         ((16, 16), True)])
def test_exr_tiled(tmp_path, comp, tile, mipmap):
    """Tiled single-part files (renderer output): partial edge tiles, a tile
    larger than the image, and a mip map whose full-resolution level is read."""
    img = _img(37, 53, seed=comp)
    chans = {"R": img[..., 0], "G": img[..., 1], "B": img[..., 2], "A": np.ones(img.shape[:2], np.float32)}
    path = str(tmp_path / "tiled.exr")
    RAW_CHUNKS.clear()
    write_exr_py(path, chans, comp, False, tile=tile, mipmap=mipmap)
    H, W, _ = img.shape
    w, h, c = C.c_int(), C.c_int(), C.c_int()
    assert lib().bmfr_exr_info(path.encode(), C.byref(w), C.byref(h), C.byref(c)) == 0
    assert (w.value, h.value, c.value) == (W, H, 4)
    out = np.empty_like(img)
    assert lib().bmfr_exr_read_rgb(path.encode(), W, H, out.ctypes.data) == 0, lib().bmfr_io_error()
    want = f24_values(img) if comp == 5 else img.copy()
    for lv, y0, n, x0, w in RAW_CHUNKS:  # level-0 tiles stored uncompressed are exact
        if lv == 0:
            want[y0:y0 + n, x0:x0 + w] = img[y0:y0 + n, x0:x0 + w]
    np.testing.assert_array_equal(out, want)


def test_exr_tiled_rejects_bad_tiles(tmp_path):
    """A tiled file without a tile description, or a tile of another level
    where level (0, 0) is expected, is rejected with a message."""
    img = _img(8, 8)
    chans = {"R": img[..., 0], "G": img[..., 1], "B": img[..., 2]}
    path = tmp_path / "t.exr"
    write_exr_py(str(path), chans, 0, False, tile=(4, 4))
    data = path.read_bytes()
    i = data.index(b"tiles\0tiledesc\0")
    no_desc = data[:i] + b"tileX\0" + data[i + 6:]  # attribute renamed: no tile description
    out = np.empty_like(img)
    (tmp_path / "nodesc.exr").write_bytes(no_desc)
    assert lib().bmfr_exr_read_rgb(str(tmp_path / "nodesc.exr").encode(), 8, 8, out.ctypes.data) != 0
    assert b"tile" in lib().bmfr_io_error()
    # the first tile's level x -> 1
    p = 8
    while data[p]:  # attributes: name, type, size, value
        e2 = data.index(b"\0", data.index(b"\0", p) + 1)
        p = e2 + 5 + struct.unpack_from("<i", data, e2 + 1)[0]
    first = struct.unpack_from("<Q", data, p + 1)[0]  # the offset table follows the terminating null
    b = bytearray(data)
    struct.pack_into("<i", b, first + 8, 1)
    (tmp_path / "level.exr").write_bytes(bytes(b))
    assert lib().bmfr_exr_read_rgb(str(tmp_path / "level.exr").encode(), 8, 8, out.ctypes.data) != 0
    assert b"bad tile" in lib().bmfr_io_error()


def _b44_want(shape, chunks_of, names):
    """The decoded image of B44_DECODED's chunks, as float32, (H, W) per channel."""
    H, W = shape
    out = {}
    for n in names:
        a = np.zeros((H, W), np.uint16)
        for (y0, x0), d in B44_DECODED[n].items():
            a[y0:y0 + d.shape[0], x0:x0 + d.shape[1]] = d
        out[n] = a.view(np.float16).astype(np.float32)
    return out


@pytest.mark.parametrize("comp", [6, 7])
@pytest.mark.parametrize("shape,tile", [((41, 29), None), ((32, 32), None), ((3, 70), None), ((70, 2), None),
                                        ((37, 53), (16, 8))])
def test_exr_b44(tmp_path, comp, shape, tile):
    """B44 / B44A (OpenImageIO reads them, bmfr.cpp:145-163): HALF channels in
    4x4 blocks -- lossless where a block's samples differ little (shift 0),
    rounded to 2^shift steps below the block maximum elsewhere (the closed
    form t_max - (d << shift) of the published scheme, independent of the
    decoder's running sums), flat blocks in 3 bytes (B44A), partial edge
    blocks; a FLOAT channel in the same chunk is stored raw."""
    H, W = shape
    rng = np.random.default_rng(H * W + comp)
    yy, xx = np.mgrid[0:H, 0:W].astype(np.float32)
    img = np.stack([1.0 + xx / 512.0,                                  # smooth: shift 0, lossless
                    rng.normal(0, 3, (H, W)).astype(np.float32),      # noise: lossy blocks
                    np.where(yy < H // 8 * 4, 0.5, -2.0).astype(np.float32)], -1)  # flat blocks
    img[0, 0, 1] = np.inf
    img[-1, -1, 1] = -0.0
    chans = {"R": img[..., 0], "G": img[..., 1], "B": img[..., 2], "A": rng.normal(0, 1, (H, W)).astype(np.float32)}
    types = {"A": False}
    path = str(tmp_path / "b44.exr")
    B44_DECODED.clear()
    B44_SHIFTS.clear()
    RAW_CHUNKS.clear()
    write_exr_py(path, chans, comp, True, tile=tile, types=types)
    out = np.empty_like(img)
    assert lib().bmfr_exr_read_rgb(path.encode(), W, H, out.ctypes.data) == 0, lib().bmfr_io_error()
    want = _b44_want((H, W), B44_DECODED, "RGB")
    for _, y0, n, x0, w in RAW_CHUNKS:  # chunks B44 would not shrink are stored as they are
        for c, ch in enumerate("RGB"):
            want[ch][y0:y0 + n, x0:x0 + w] = img[y0:y0 + n, x0:x0 + w, c].astype(np.float16)
    np.testing.assert_array_equal(out[..., 0], want["R"])
    np.testing.assert_array_equal(out[..., 1], want["G"])
    np.testing.assert_array_equal(out[..., 2], want["B"])
    # lossless where the scheme is: smooth and flat channels
    np.testing.assert_array_equal(out[..., 0], img[..., 0].astype(np.float16).astype(np.float32))
    np.testing.assert_array_equal(out[..., 2], img[..., 2].astype(np.float16).astype(np.float32))
    # the noisy channel: lossy, each sample within half a step (2^shift of the
    # ordered code) of its own -- measured in the ordered code, where the
    # scheme rounds
    g = img[..., 1].astype(np.float16)
    fin = np.isfinite(g)
    code = lambda a: _b44_ordered(a.view(np.uint16))  # noqa: E731
    err = np.abs(code(out[..., 1].astype(np.float16))[fin] - code(g)[fin])
    assert err.max() <= 1 << (max(B44_SHIFTS) - 1)
    assert err.max() > 0 or RAW_CHUNKS
    assert (-1 in B44_SHIFTS) == (comp == 7)  # 3-byte flat blocks: B44A only


def test_exr_b44_rejects_plinear(tmp_path):
    img = _img(8, 8)
    chans = {"R": img[..., 0], "G": img[..., 1], "B": img[..., 2]}
    path = tmp_path / "lin.exr"
    write_exr_py(str(path), chans, 6, True)
    b = bytearray(path.read_bytes())
    i = b.index(b"R\0", b.index(b"chlist"))
    b[i + 2 + 4] = 1  # R's pLinear flag
    path.write_bytes(bytes(b))
    out = np.empty_like(img)
    assert lib().bmfr_exr_read_rgb(str(path).encode(), 8, 8, out.ctypes.data) != 0
    assert b"pLinear" in lib().bmfr_io_error()


def _dwa_want(shape, names, raw_img, types):
    """The decoded R, G, B of DWA_DECODED's chunks (HALF channels: half bit
    patterns; FLOAT: the samples), raw chunks as stored, as float32."""
    H, W = shape
    out = {}
    for n in names:
        half = types.get(n, True)
        a = np.zeros((H, W), np.uint16 if half else np.float32)
        for (y0, x0), d in DWA_DECODED[n].items():
            a[y0:y0 + d.shape[0], x0:x0 + d.shape[1]] = d
        out[n] = a.view(np.float16).astype(np.float32) if half else a
    for _, y0, ln, x0, w in RAW_CHUNKS:  # chunks DWA would not shrink are stored as they are
        for n in names:
            v = raw_img[n][y0:y0 + ln, x0:x0 + w]
            out[n][y0:y0 + ln, x0:x0 + w] = v.astype(np.float16).astype(np.float32) if types.get(n, True) else v
    return out


@pytest.mark.parametrize("comp", [8, 9])
@pytest.mark.parametrize("shape,tile", [((41, 29), None), ((300, 21), None), ((3, 9), None), ((67, 53), (32, 16))])
@pytest.mark.parametrize("version,ac_mode", [(2, 0), (2, 1), (1, 0)])
def test_exr_dwa(tmp_path, comp, shape, tile, version, ac_mode):
    """DWAA / DWAB (OpenImageIO reads them, bmfr.cpp:145-163): an R, G, B set
    of HALF channels through the lossy DCT with the colour transform, an
    alpha (RLE) and a FLOAT depth channel (UNKNOWN) in the same chunks,
    static-Huffman and deflated AC terms, version-2 rules and version 1's
    fixed set, partial 8x8 blocks and partial chunks (DWAB: 256 lines), tiles.
    Bit for bit against the decode exr_dwa_py.py predicts from the
    coefficients it wrote; and close to the input (the codec is lossy)."""
    H, W = shape
    r, g, b = _dwa_image(H, W, H * W + comp)
    chans = {"R": r, "G": g, "B": b, "A": np.full((H, W), 0.5, np.float32), "Z": (r * 100).astype(np.float32)}
    types = {"Z": False}
    path = str(tmp_path / "dwa.exr")
    DWA_DECODED.clear()
    RAW_CHUNKS.clear()
    DWA_OPTS.update(version=version, ac_mode=ac_mode, drop=0.02)
    try:
        write_exr_py(path, chans, comp, True, tile=tile, types=types)
    finally:
        DWA_OPTS.update(version=2, ac_mode=0, drop=0.02)
    out = np.empty((H, W, 3), np.float32)
    assert lib().bmfr_exr_read_rgb(path.encode(), W, H, out.ctypes.data) == 0, lib().bmfr_io_error()
    want = _dwa_want((H, W), "RGB", chans, types)
    for c, n in enumerate("RGB"):
        np.testing.assert_array_equal(out[..., c], want[n], err_msg=n)
    # lossy, but close: relative error on the finite samples
    for c, src in enumerate((r, g, b)):
        fin = np.isfinite(src)
        err = np.abs(out[..., c][fin] - src[fin]) / np.maximum(np.abs(src[fin]), 0.05)
        assert np.median(err) < 0.05, (c, np.median(err))
    assert len(RAW_CHUNKS) < len(DWA_DECODED["R"]) or H * W < 64  # DWA-coded chunks (tiny images: stored)


def test_exr_dwa_partial_colour_set(tmp_path):
    """R and G without a HALF B (here FLOAT: an UNKNOWN channel) form no
    colour set: each is its own lossy decoder, no colour transform."""
    H, W = 20, 19
    r, g, b = _dwa_image(H, W, 5)
    chans = {"R": r, "G": g, "B": b}
    types = {"B": False}
    path = str(tmp_path / "dwa_rg.exr")
    DWA_DECODED.clear()
    RAW_CHUNKS.clear()
    write_exr_py(path, chans, 8, True, types=types)
    out = np.empty((H, W, 3), np.float32)
    assert lib().bmfr_exr_read_rgb(path.encode(), W, H, out.ctypes.data) == 0, lib().bmfr_io_error()
    want = _dwa_want((H, W), "RGB", chans, types)
    for c, n in enumerate("RGB"):
        np.testing.assert_array_equal(out[..., c], want[n], err_msg=n)
    np.testing.assert_array_equal(out[..., 2], b)  # UNKNOWN: lossless


def test_exr_dwa_float_lossy_channels(tmp_path):
    """FLOAT R, G, B under OpenEXR's version-2 default rules, which mark them
    LOSSY_DCT too: decoded as halves (colour transform included) and widened
    exactly to float."""
    H, W = 24, 37
    r, g, b = _dwa_image(H, W, 11)
    chans = {"R": r, "G": g, "B": b}
    types = {"R": False, "G": False, "B": False}
    path = str(tmp_path / "dwa_f.exr")
    DWA_DECODED.clear()
    RAW_CHUNKS.clear()
    DWA_OPTS.update(rules=exr_dwa_py.DEFAULT_RULES_FLOAT)
    try:
        write_exr_py(path, chans, 9, True, types=types)
    finally:
        DWA_OPTS.pop("rules")
    assert not RAW_CHUNKS
    out = np.empty((H, W, 3), np.float32)
    assert lib().bmfr_exr_read_rgb(path.encode(), W, H, out.ctypes.data) == 0, lib().bmfr_io_error()
    want = _dwa_want((H, W), "RGB", chans, types)
    for c, n in enumerate("RGB"):
        np.testing.assert_array_equal(out[..., c], want[n], err_msg=n)
        assert (want[n] == want[n].astype(np.float16).astype(np.float32)).all()  # halves, widened


def test_exr_dwa_rejects_plinear_lossy_channel(tmp_path):
    """A LOSSY_DCT channel with the pLinear flag is refused as unsupported
    (not reported as corrupt data)."""
    H, W = 32, 64
    r, g, b = _dwa_image(H, W, 13)
    path = tmp_path / "dwa_lin.exr"
    DWA_DECODED.clear()
    RAW_CHUNKS.clear()
    write_exr_py(str(path), {"R": r, "G": g, "B": b}, 8, True)
    assert not RAW_CHUNKS
    bb = bytearray(path.read_bytes())
    i = bb.index(b"G\0", bb.index(b"chlist"))
    bb[i + 2 + 4] = 1  # G's pLinear flag
    path.write_bytes(bytes(bb))
    out = np.empty((H, W, 3), np.float32)
    assert lib().bmfr_exr_read_rgb(str(path).encode(), W, H, out.ctypes.data) != 0
    err = lib().bmfr_io_error()
    assert b"unsupported" in err and b"pLinear" in err and b"corrupt" not in err, err


def test_exr_dwa_rejects_corrupt_chunks(tmp_path):
    """Bad sizes, an unknown version or AC mode, and a truncated AC stream
    are errors, not crashes (the ASan corpus in test_sanitizers.py covers
    random damage)."""
    H, W = 32, 64
    r, g, b = _dwa_image(H, W, 9)
    path = tmp_path / "dwa.exr"
    DWA_DECODED.clear()
    RAW_CHUNKS.clear()
    write_exr_py(str(path), {"R": r, "G": g, "B": b}, 8, True)
    data = path.read_bytes()
    p = 8
    while data[p]:  # attributes: name, type, size, value
        e2 = data.index(b"\0", data.index(b"\0", p) + 1)
        p = e2 + 5 + struct.unpack_from("<i", data, e2 + 1)[0]
    first = struct.unpack_from("<Q", data, p + 1)[0] + 8  # the first chunk's DWA sizes (after y, size)
    assert struct.unpack_from("<Q", data, first)[0] == 2
    out = np.empty((H, W, 3), np.float32)
    for field, value in ((0, 7), (10, 5), (8, 10 ** 6), (9, 3)):  # version, AC mode, AC count, DC count
        bb = bytearray(data)
        struct.pack_into("<Q", bb, first + 8 * field, value)
        (tmp_path / "bad.exr").write_bytes(bytes(bb))
        assert lib().bmfr_exr_read_rgb(str(tmp_path / "bad.exr").encode(), W, H, out.ctypes.data) != 0, field
        assert b"corrupt chunk" in lib().bmfr_io_error()
