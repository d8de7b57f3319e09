"""Dependency-free PNG container (zlib only): the writer of the image output (diner_amd.imageio) and the
reader the tests use.  Kept apart from imageio.py so that fixture generators and data tools can write PNGs WITHOUT the HIP extension
(imageio imports diner_amd.ops, which loads libdiner_hip.so)."""
import struct
import zlib

import numpy as np


def write_png(path, arr, level=1):
    """(H,W,3) or (H,W) uint8 array / tensor -> 8-bit PNG (filter type 0 rows, one IDAT)."""
    a = arr.detach().cpu().numpy() if hasattr(arr, "detach") else np.asarray(arr)
    assert a.dtype == np.uint8 and a.ndim in (2, 3)
    H, W = a.shape[:2]
    ch = 1 if a.ndim == 2 else a.shape[2]
    color = {1: 0, 3: 2, 4: 6}[ch]
    raw = np.concatenate([np.zeros((H, 1), np.uint8), a.reshape(H, W * ch)], axis=1).tobytes()

    def chunk(tag, data):
        return struct.pack(">I", len(data)) + tag + data + struct.pack(">I", zlib.crc32(tag + data) & 0xffffffff)

    with open(path, "wb") as f:
        f.write(b"\x89PNG\r\n\x1a\n" + chunk(b"IHDR", struct.pack(">IIBBBBB", W, H, 8, color, 0, 0, 0)) +
                chunk(b"IDAT", zlib.compress(raw, level)) + chunk(b"IEND", b""))


def read_png(path):
    """8-bit gray / RGB / RGBA, non-interlaced PNG (filter types 0-4, as PIL / torchvision write them) -> uint8 array (H,W) or (H,W,C).
    Reads what write_png writes and the folders diner_amd.evaluate scores."""
    data = open(path, "rb").read()
    assert data[:8] == b"\x89PNG\r\n\x1a\n"
    pos, idat, hdr = 8, b"", None
    while pos < len(data):
        n, tag = struct.unpack(">I", data[pos:pos + 4])[0], data[pos + 4:pos + 8]
        body = data[pos + 8:pos + 8 + n]
        assert zlib.crc32(tag + body) & 0xffffffff == struct.unpack(">I", data[pos + 8 + n:pos + 12 + n])[0]
        if tag == b"IHDR":
            hdr = struct.unpack(">IIBBBBB", body)
        elif tag == b"IDAT":
            idat += body
        pos += 12 + n
    W, H, depth, color, _, _, interlace = hdr
    assert depth == 8 and interlace == 0
    ch = {0: 1, 2: 3, 6: 4}[color]
    rows = np.frombuffer(zlib.decompress(idat), np.uint8).reshape(H, 1 + W * ch)
    if (rows[:, 0] == 0).all():                                    # what write_png writes: no reconstruction needed
        out = rows[:, 1:].reshape(H, W, ch)
    else:
        out = _unfilter(rows, H, W, ch).reshape(H, W, ch)
    return out[..., 0] if ch == 1 else out


def _unfilter(rows, H, W, ch):
    """Reconstruct the filtered scanlines of an 8-bit image (PNG spec 9.2; PIL writes adaptive filters): rows (H, 1 + W ch)."""
    n = W * ch
    out = np.zeros((H, n), np.uint8)
    prev = np.zeros(n, np.int16)
    for i in range(H):
        ft, x = int(rows[i, 0]), rows[i, 1:].astype(np.int16)
        if ft == 0:
            cur = x
        elif ft == 2:                                              # Up
            cur = (x + prev) & 0xff
        elif ft in (1, 3, 4):                                      # Sub / Average / Paeth depend on the reconstructed left byte
            cur = np.empty(n, np.int16)
            for c in range(ch):                                    # one pass per channel: stride ch along the row
                xs, up = x[c::ch], prev[c::ch]
                if ft == 1:
                    cur[c::ch] = np.cumsum(xs, dtype=np.int64) & 0xff
                    continue
                res = np.empty(len(xs), np.int16)
                left = ul = 0
                for j in range(len(xs)):
                    b = int(up[j])
                    if ft == 3:
                        v = (int(xs[j]) + ((left + b) >> 1)) & 0xff
                    else:
                        p = left + b - ul
                        pa, pb, pc = abs(p - left), abs(p - b), abs(p - ul)
                        pr = left if pa <= pb and pa <= pc else (b if pb <= pc else ul)
                        v = (int(xs[j]) + pr) & 0xff
                    res[j] = v
                    left, ul = v, b
                cur[c::ch] = res
        else:
            raise ValueError(f"PNG row {i}: unknown filter type {ft}")
        out[i] = cur.astype(np.uint8)
        prev = cur
    return out
