"""Radiance .hdr (RGBE) files for sky maps: a reader and a writer in plain numpy.

read_hdr(path) -> float32 (H, W, 3), linear radiance, top row first: what scene.Sky.map takes.
write_hdr(path, image, rle=True) writes one, run-length encoded per channel (the "new" scheme) or flat.

The format: a text header ("#?RADIANCE", "FORMAT=32-bit_rle_rgbe", a blank line), the resolution line "-Y H +X W",
then H scanlines of W pixels of four bytes (r, g, b, e): channel value = byte * 2^(e - 136), e = 0 meaning black.  A
run-length encoded scanline starts with the bytes 2, 2, W >> 8, W & 255 (8 <= W < 32768) and holds the four channels one
after the other, each as runs: a count byte n > 128 followed by one byte repeated n - 128 times, or n <= 128 followed by
n literal bytes.  The writer rounds a mantissa to nearest, so a written value is within 1/256 of its pixel's largest
channel of the original -- the format's own quantisation.  Only the standard "-Y H +X W" orientation is read; the older
pixel-run encoding is not.
"""
from __future__ import annotations

from pathlib import Path

import numpy as np


def rgbe_encode(image: np.ndarray) -> np.ndarray:
    """float (H, W, 3) -> uint8 (H, W, 4).  Negative and NaN channels count as 0; values above RGBE's largest,
    255 * 2^119, are held at it."""
    img = np.nan_to_num(np.asarray(image, np.float64), nan=0.0, posinf=float(np.finfo(np.float32).max), neginf=0.0)
    img = np.minimum(np.maximum(img, 0.0), 255.0 * 2.0 ** 119)  # RGBE's largest value: (255, e = 255)
    v = img.max(axis=2)
    _, e = np.frexp(v)  # v = m * 2^e, m in [0.5, 1)
    q = np.floor(img * np.exp2(8.0 - e)[..., None] + 0.5)
    up = (q > 255.0).any(axis=2)  # the largest mantissa rounded up to 256: one exponent more
    e = e + up
    q = np.where(up[..., None], np.floor(img * np.exp2(8.0 - e)[..., None] + 0.5), q)
    out = np.zeros(img.shape[:2] + (4,), np.uint8)
    ok = (v >= 1e-32) & (e + 128 >= 1)
    out[..., :3] = np.where(ok[..., None], q, 0.0).astype(np.uint8)
    out[..., 3] = np.where(ok, e + 128, 0).astype(np.uint8)
    return out


def rgbe_decode(rgbe: np.ndarray) -> np.ndarray:
    """uint8 (..., 4) -> float32 (..., 3)."""
    e = rgbe[..., 3].astype(np.int32)
    f = np.where(e == 0, 0.0, np.exp2((e - 136).astype(np.float64)))
    return (rgbe[..., :3].astype(np.float64) * f[..., None]).astype(np.float32)


def _rle_channel(row: np.ndarray) -> bytes:
    """One channel of a scanline as runs (runs of at least 3 equal bytes are packed, the rest literal)."""
    out = bytearray()
    n = len(row)
    # starts and lengths of the maximal runs of equal bytes
    edge = np.flatnonzero(np.diff(row)) + 1
    starts = np.concatenate(([0], edge))
    lens = np.diff(np.concatenate((starts, [n])))
    lit_from = 0

    def flush(upto: int) -> None:
        nonlocal lit_from
        while lit_from < upto:
            k = min(128, upto - lit_from)
            out.append(k)
            out.extend(row[lit_from:lit_from + k].tobytes())
            lit_from += k

    for s, ln in zip(starts.tolist(), lens.tolist()):
        if ln < 3:
            continue
        flush(s)
        b = int(row[s])
        left = ln
        while left > 0:
            k = min(127, left)
            out.append(128 + k)
            out.append(b)
            left -= k
        lit_from = s + ln
    flush(n)
    return bytes(out)


def write_hdr(path, image: np.ndarray, rle: bool = True) -> None:
    """Write float (H, W, 3) linear radiance as a Radiance .hdr file; rle=False, or a width outside [8, 32767],
    writes flat scanlines."""
    image = np.asarray(image)
    if image.ndim != 3 or image.shape[2] != 3 or image.shape[0] == 0 or image.shape[1] == 0:
        raise ValueError(f"an image has shape (H, W, 3), not {image.shape}")
    H, W = image.shape[:2]
    px = rgbe_encode(image)
    body = bytearray()
    if rle and 8 <= W < 32768:
        for y in range(H):
            body.extend(bytes((2, 2, W >> 8, W & 255)))
            for c in range(4):
                body.extend(_rle_channel(px[y, :, c]))
    else:
        body.extend(px.tobytes())
    head = f"#?RADIANCE\nFORMAT=32-bit_rle_rgbe\n\n-Y {H} +X {W}\n".encode("ascii")
    Path(path).write_bytes(head + bytes(body))


def read_hdr(path) -> np.ndarray:
    """Read a Radiance .hdr file (flat or run-length encoded scanlines) -> float32 (H, W, 3), top row first."""
    data = Path(path).read_bytes()
    if not (data.startswith(b"#?RADIANCE") or data.startswith(b"#?RGBE")):
        raise ValueError("not a Radiance .hdr file (no #?RADIANCE signature)")
    end = data.find(b"\n\n")
    if end < 0:
        raise ValueError("no end of header")
    header = data[:end].decode("ascii", "replace").split("\n")
    fmt = [ln.split("=", 1)[1].strip() for ln in header if ln.startswith("FORMAT=")]
    if fmt and fmt[0] != "32-bit_rle_rgbe":
        raise ValueError(f"format {fmt[0]} is not 32-bit_rle_rgbe")
    pos = end + 2
    nl = data.find(b"\n", pos)
    if nl < 0:
        raise ValueError("no resolution line")
    res = data[pos:nl].decode("ascii", "replace").split()
    if len(res) != 4 or res[0] != "-Y" or res[2] != "+X":
        raise ValueError(f"resolution line {' '.join(res)!r}: only '-Y H +X W' is read")
    H, W = int(res[1]), int(res[3])
    if H <= 0 or W <= 0:
        raise ValueError("empty image")
    buf = np.frombuffer(data, np.uint8, offset=nl + 1)
    px = np.empty((H, W, 4), np.uint8)
    p = 0
    for y in range(H):
        if p + 4 > len(buf):
            raise ValueError("file ends inside the pixels")
        rle = 8 <= W < 32768 and buf[p] == 2 and buf[p + 1] == 2 and (int(buf[p + 2]) << 8 | int(buf[p + 3])) == W
        if not rle:
            if p + 4 * W > len(buf):
                raise ValueError("file ends inside the pixels")
            px[y] = buf[p:p + 4 * W].reshape(W, 4)
            p += 4 * W
            continue
        p += 4
        for c in range(4):
            x = 0
            while x < W:
                if p >= len(buf):
                    raise ValueError("file ends inside a scanline")
                n = int(buf[p])
                p += 1
                if n > 128:
                    n -= 128
                    if x + n > W or p >= len(buf):
                        raise ValueError("a run leaves its scanline")
                    px[y, x:x + n, c] = buf[p]
                    p += 1
                else:
                    if n == 0 or x + n > W or p + n > len(buf):
                        raise ValueError("a run leaves its scanline")
                    px[y, x:x + n, c] = buf[p:p + n]
                    p += n
                x += n
    return rgbe_decode(px)
