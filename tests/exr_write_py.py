"""An independent numpy + zlib OpenEXR 2 writer, the reference encoder of
tests/test_image_io.py and the source of the malformed-file corpus of
tests/test_sanitizers.py: scanline and tiled files (HALF / FLOAT channels,
NONE / RLE / ZIPS / ZIP / PXR24 / B44 / B44A compression, PIZ through
tests/exr_piz_py.py and DWAA / DWAB through tests/exr_dwa_py.py; one-level and
mip-mapped tiles), and the test images both write.  TEST INFRASTRUCTURE ONLY.

The module-level tables (RAW_CHUNKS, B44_DECODED, B44_SHIFTS, DWA_DECODED)
record what the last files written hold as a decoder sees it; DWA_OPTS is the
form of the DWA chunks.  A test clears / sets them around its own writes."""
from __future__ import annotations

import struct
import zlib

import numpy as np

import exr_dwa_py
from exr_piz_py import piz_compress


def _attr(name, typ, data):
    return name.encode() + b"\0" + typ.encode() + b"\0" + struct.pack("<i", len(data)) + data


def _predict(raw: bytes) -> bytes:
    a = np.frombuffer(raw, np.uint8)
    t = np.concatenate([a[0::2], a[1::2]]).astype(np.int32)
    d = t.copy()
    d[1:] = (t[1:] - t[:-1] + 128 + 256) & 255
    return d.astype(np.uint8).tobytes()


def _rle(data: bytes) -> bytes:
    out, i, n = bytearray(), 0, len(data)
    while i < n:
        j = i
        while j < n and j - i < 127 and data[j] == data[i]:
            j += 1
        if j - i >= 3:
            out += struct.pack("b", j - i - 1) + data[i:i + 1]
            i = j
        else:
            k = i
            while k < n and k - i < 127 and not (k + 2 < n and data[k] == data[k + 1] == data[k + 2]):
                k += 1
            out += struct.pack("b", -(k - i)) + data[i:k]
            i = k
    return bytes(out)


def f24(a: np.ndarray) -> np.ndarray:
    """PXR24's float -> 24-bit conversion (published OpenEXR scheme): the top
    24 bits of the float, rounded half up in the mantissa, not rounding into
    infinity; NaN stays NaN."""
    i = np.ascontiguousarray(a, np.float32).view(np.uint32).astype(np.int64)
    s, e, m = i & 0x80000000, i & 0x7f800000, i & 0x007fffff
    r = ((e | m) + (m & 0x80)) >> 8
    r = np.where(r >= 0x7f8000, (e | m) >> 8, r)
    m8 = m >> 8
    special = np.where(m != 0, (e >> 8) | m8 | (m8 == 0), e >> 8)
    return (np.where(e == 0x7f800000, special, r) | (s >> 8)).astype(np.int64)


def f24_values(a: np.ndarray) -> np.ndarray:
    """What a PXR24 FLOAT sample decodes to: the 24 bits, low byte zero."""
    return (f24(a) << 8).astype(np.uint32).view(np.float32).reshape(np.shape(a))


def _pxr24(img, names, y0, lines, x0, w, half):
    """One PXR24 chunk: per line and channel, sample differences split into
    byte planes (most significant first), deflated."""
    out = bytearray()
    for y in range(y0, y0 + lines):
        for n in names:
            row = np.ascontiguousarray(img[n][y, x0:x0 + w])
            if half:
                v = row.astype(np.float16).view(np.uint16).astype(np.int64)
                nb = 2
            else:
                v = f24(row)
                nb = 3
            d = np.diff(np.concatenate([[0], v])) & 0xffffffff
            for k in range(nb):
                out += ((d >> (8 * (nb - 1 - k))) & 255).astype(np.uint8).tobytes()
    return zlib.compress(bytes(out))


def _b44_shift_round(x, shift):
    """B44's x / 2^shift rounded to nearest, ties to even (published OpenEXR scheme)."""
    x = x << 1
    a = (1 << shift) - 1
    b = (x >> (shift + 1)) & 1
    return (x + a + b) >> (shift + 1)


def _b44_ordered(h16: np.ndarray) -> np.ndarray:
    """Half bit patterns -> B44's ordered 16-bit codes (inf / NaN -> 0x8000)."""
    h = h16.astype(np.int64)
    t = np.where(h & 0x8000, (~h) & 0xffff, h | 0x8000)
    return np.where((h & 0x7c00) == 0x7c00, 0x8000, t)


def _b44_block(s: np.ndarray, flat: bool):
    """One 4x4 block (16 half bit patterns, row-major) -> (bytes, decoded bit
    patterns).  The decoded block in closed form: t_max - (d_i << shift)."""
    t = _b44_ordered(s)
    tmax = int(t.max())
    bias = 0x20
    shift = -1
    while True:
        shift += 1
        d = np.array([_b44_shift_round(tmax - int(v), shift) for v in t])
        r = [d[0] - d[4], d[4] - d[8], d[8] - d[12],
             d[0] - d[1], d[4] - d[5], d[8] - d[9], d[12] - d[13],
             d[1] - d[2], d[5] - d[6], d[9] - d[10], d[13] - d[14],
             d[2] - d[3], d[6] - d[7], d[10] - d[11], d[14] - d[15]]
        r = [int(v) + bias for v in r]
        if min(r) >= 0 and max(r) <= 0x3f:
            break
    if flat and min(r) == bias and max(r) == bias:
        t0 = int(t[0])
        dec = np.full(16, t0, np.int64)
        out = bytes([t0 >> 8, t0 & 255, 0xfc])
    else:
        t0 = (tmax - (int(d[0]) << shift)) & 0xffff
        dec = (tmax - (d.astype(np.int64) << shift)) & 0xffff
        b = [t0 >> 8, t0 & 255, (shift << 2) | (r[0] >> 4), (r[0] << 4) | (r[1] >> 2), (r[1] << 6) | r[2],
             (r[3] << 2) | (r[4] >> 4), (r[4] << 4) | (r[5] >> 2), (r[5] << 6) | r[6],
             (r[7] << 2) | (r[8] >> 4), (r[8] << 4) | (r[9] >> 2), (r[9] << 6) | r[10],
             (r[11] << 2) | (r[12] >> 4), (r[12] << 4) | (r[13] >> 2), (r[13] << 6) | r[14]]
        out = bytes(v & 255 for v in b)
    dec = np.where(dec & 0x8000, dec & 0x7fff, (~dec) & 0xffff)  # ordered code -> half bits
    return out, dec.astype(np.uint16), shift


B44_DECODED = {}  # channel -> {(y0, x0): half bit patterns of the chunk as B44 decodes it}
B44_SHIFTS = []   # shift of every block written (-1: a B44A flat block)


def _b44(img, names, y0, lines, x0, w, half, flat, types):
    """One B44 / B44A chunk: channel after channel over the chunk; HALF
    channels as 4x4 blocks (edge blocks padded by repeating the last row /
    column), other channels raw."""
    out = bytearray()
    for n in names:
        a = np.ascontiguousarray(img[n][y0:y0 + lines, x0:x0 + w])
        if not types.get(n, half):
            out += a.astype(np.float32).tobytes()
            continue
        h = a.astype(np.float16).view(np.uint16)
        ph, pw = (lines + 3) // 4 * 4, (w + 3) // 4 * 4
        hp = np.pad(h, ((0, ph - lines), (0, pw - w)), mode="edge")
        dec = np.zeros((ph, pw), np.uint16)
        for by in range(0, ph, 4):
            for bx in range(0, pw, 4):
                blk, d, sh = _b44_block(hp[by:by + 4, bx:bx + 4].reshape(16), flat)
                B44_SHIFTS.append(-1 if len(blk) == 3 else sh)  # -1: a 3-byte flat block
                out += blk
                dec[by:by + 4, bx:bx + 4] = d.reshape(4, 4)
        B44_DECODED.setdefault(n, {})[(y0, x0)] = dec[:lines, :w]
    return bytes(out)


RAW_CHUNKS = []  # (level, y0, lines, x0, w) of the chunks write_exr_py stored uncompressed
DWA_DECODED = {}  # channel -> {(y0, x0): the chunk's samples as a DWA decoder produces them}
DWA_OPTS = {"version": 2, "ac_mode": 0, "drop": 0.02}  # DWA chunks' form (exr_dwa_py.dwa_compress)


def _chunk_data(img, names, dt, compression, y0, lines, x0, w, half, level=0, types=None):
    types = types or {}
    raw = b"".join(np.ascontiguousarray(img[n][y, x0:x0 + w]).astype(
        (np.float16 if types[n] else np.float32) if n in types else dt).tobytes()
                   for y in range(y0, y0 + lines) for n in names)
    if compression == 1:
        data = _rle(_predict(raw))
    elif compression in (2, 3):
        data = zlib.compress(_predict(raw))
    elif compression == 4:
        data = piz_compress(raw, w, lines, [1 if half else 2] * len(names))
    elif compression == 5:
        data = _pxr24(img, names, y0, lines, x0, w, half)
    elif compression in (6, 7):
        data = _b44(img, names, y0, lines, x0, w, half, compression == 7, types)
    elif compression in (8, 9):
        ptypes = {n: (1 if types.get(n, half) else 2) for n in names}
        data, dec = exr_dwa_py.dwa_compress({n: img[n][y0:y0 + lines, x0:x0 + w] for n in names}, ptypes, lines, w,
                                            **DWA_OPTS)
        for n in names:
            DWA_DECODED.setdefault(n, {})[(y0, x0)] = dec[n]
    else:
        data = raw
    if compression and len(data) >= len(raw):  # OpenEXR stores such a chunk as it is
        RAW_CHUNKS.append((level, y0, lines, x0, w))
        return raw
    return data


def write_exr_py(path, img: dict, compression: int, half: bool, tile=None, mipmap=False, types=None):
    """img: channel name -> (H, W) float array.  Channels are stored sorted by
    name.  compression 0 NONE, 1 RLE, 2 ZIPS, 3 ZIP, 4 PIZ, 5 PXR24, 6 B44,
    7 B44A, 8 DWAA, 9 DWAB.  types: channel name -> True (HALF) / False
    (FLOAT) where it differs from `half` (B44 / DWA chunks only).
    tile = (tw, th): a tiled file (ONE_LEVEL, or MIPMAP_LEVELS round-down
    with mipmap=True: the lower levels follow level 0, box-filtered)."""
    names = sorted(img)
    H, W = img[names[0]].shape
    ptype, dt = (1, np.float16) if half else (2, np.float32)
    types = types or {}
    chl = b"".join(n.encode() + b"\0" + struct.pack("<iIii", (1 if types[n] else 2) if n in types else ptype, 0, 1, 1)
                   for n in names) + b"\0"
    box = struct.pack("<iiii", 0, 0, W - 1, H - 1)
    version = 2 | (0x200 if tile else 0)
    hdr = (struct.pack("<II", 20000630, version) + _attr("channels", "chlist", chl) +
           _attr("compression", "compression", bytes([compression])) + _attr("dataWindow", "box2i", box) +
           _attr("displayWindow", "box2i", box) + _attr("lineOrder", "lineOrder", b"\0") +
           _attr("pixelAspectRatio", "float", struct.pack("<f", 1)) +
           _attr("screenWindowCenter", "v2f", struct.pack("<ff", 0, 0)) +
           _attr("screenWindowWidth", "float", struct.pack("<f", 1)))
    if tile:
        hdr += _attr("tiles", "tiledesc", struct.pack("<IIB", tile[0], tile[1], 1 if mipmap else 0))
    hdr += b"\0"
    chunks = []
    if tile:
        tw, th = tile
        levels = [img]
        while mipmap and max(levels[-1][names[0]].shape) > 1:
            h2, w2 = (max(1, d // 2) for d in levels[-1][names[0]].shape)
            levels.append({n: levels[-1][n][:2 * h2:2, :2 * w2:2][:h2, :w2] for n in names})
        for lv, im in enumerate(levels):
            lh, lw = im[names[0]].shape
            for ty in range((lh + th - 1) // th):
                for tx in range((lw + tw - 1) // tw):
                    x0, y0 = tx * tw, ty * th
                    w, lines = min(tw, lw - x0), min(th, lh - y0)
                    data = _chunk_data(im, names, dt, compression, y0, lines, x0, w, half, lv, types)
                    chunks.append(struct.pack("<iiiii", tx, ty, lv, lv, len(data)) + data)
    else:
        lpc = {0: 1, 1: 1, 2: 1, 3: 16, 4: 32, 5: 16, 6: 32, 7: 32, 8: 32, 9: 256}[compression]
        for y0 in range(0, H, lpc):
            data = _chunk_data(img, names, dt, compression, y0, min(H, y0 + lpc) - y0, 0, W, half, types=types)
            chunks.append(struct.pack("<ii", y0, len(data)) + data)
    off = len(hdr) + 8 * len(chunks)
    table = b""
    for c in chunks:
        table += struct.pack("<Q", off)
        off += len(c)
    with open(path, "wb") as f:
        f.write(hdr + table + b"".join(chunks))


def _img(H=37, W=53, seed=1):
    rng = np.random.default_rng(seed)
    img = rng.normal(0, 3, (H, W, 3)).astype(np.float32)
    img[0, 0] = [np.inf, -0.0, 65504.0]
    img[1, :5, 0] = 0.25  # runs for RLE
    img[2, :] = 1.0
    return img


def _dwa_image(H, W, seed):
    rng = np.random.default_rng(seed)
    yy, xx = np.mgrid[0:H, 0:W].astype(np.float32)
    r = 0.5 + 0.4 * np.sin(xx / 7.0) * np.cos(yy / 5.0)                       # smooth, below 1
    g = np.abs(0.3 + 0.1 * np.sin(yy / 3.0) + rng.normal(0, 0.03, (H, W))).astype(np.float32)  # noise
    b = (1.0 + 30.0 * (xx + yy) / (W + H)).astype(np.float32)                 # above 1: the log branch
    b[::5, ::3] *= -1.0                                                      # negative samples
    g[0, 0] = np.inf                                                          # non-finite -> 0 on the codec's scale
    return r.astype(np.float32), g, b
