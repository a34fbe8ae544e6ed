"""A dependency-free PNG writer and reader for what the evaluation overlays need: 8-bit grey and 8-bit RGB, non-interlaced,
with the standard library's zlib and struct.  Why: the reference saves its visualised detections with cv2.imwrite
(utils/eval.py:104-108) and OpenCV is not a dependency.  Written to the PNG specification (ISO/IEC 15948): signature, IHDR, one
or more IDAT chunks that together hold one zlib stream, IEND, a CRC-32 over each chunk's type and data.  The writer emits
filter type 0 (None) on every scanline; the reader undoes all five filter types, so that files from other writers load, and
checks every CRC.  Anything else -- 16-bit samples, palettes, alpha, interlacing -- raises PngUnsupported."""
import struct
import zlib

import numpy as np

SIGNATURE = b"\x89PNG\r\n\x1a\n"
_CHANNELS = {0: 1, 2: 3}  # colour type -> samples per pixel


class PngUnsupported(NotImplementedError):
    pass


def _chunk(kind, data):
    return struct.pack(">I", len(data)) + kind + data + struct.pack(">I", zlib.crc32(kind + data) & 0xFFFFFFFF)


def encode_png(array, level=6):
    """uint8 [H,W] (grey) or [H,W,3] (RGB) -> the bytes of a PNG file"""
    a = np.asarray(array)
    if a.dtype != np.uint8 or a.ndim not in (2, 3) or (a.ndim == 3 and a.shape[2] != 3) or a.shape[0] < 1 or a.shape[1] < 1:
        raise ValueError("encode_png: need a uint8 array [H,W] or [H,W,3] with H, W >= 1, got %s %s" % (a.dtype, a.shape))
    H, W = a.shape[:2]
    rows = np.zeros((H, 1 + W * (3 if a.ndim == 3 else 1)), np.uint8)  # a filter byte 0 in front of every scanline
    rows[:, 1:] = a.reshape(H, -1)
    ihdr = struct.pack(">IIBBBBB", W, H, 8, 2 if a.ndim == 3 else 0, 0, 0, 0)
    return SIGNATURE + _chunk(b"IHDR", ihdr) + _chunk(b"IDAT", zlib.compress(rows.tobytes(), level)) + _chunk(b"IEND", b"")


def write_png(path, array, level=6):
    with open(path, "wb") as f:
        f.write(encode_png(array, level))


def _unfilter(raw, H, stride, bpp):
    out = np.zeros((H, stride), np.uint8)
    prev = np.zeros((stride,), np.int64)
    for y in range(H):
        kind = raw[y * (stride + 1)]
        line = np.frombuffer(raw, np.uint8, stride, y * (stride + 1) + 1).astype(np.int64)
        if kind == 0:
            cur = line
        elif kind == 2:
            cur = (line + prev) & 255
        elif kind in (1, 3, 4):  # these look at the pixel on the left: byte by byte
            cur = np.zeros((stride,), np.int64)
            for i in range(stride):
                a = cur[i - bpp] if i >= bpp else 0
                b = prev[i]
                if kind == 1:
                    pred = a
                elif kind == 3:
                    pred = (a + b) // 2
                else:
                    c = prev[i - bpp] if i >= bpp else 0
                    p = a + b - c
                    pa, pb, pc = abs(p - a), abs(p - b), abs(p - c)
                    pred = a if (pa <= pb and pa <= pc) else (b if pb <= pc else c)
                cur[i] = (line[i] + pred) & 255
        else:
            raise PngUnsupported("png: unknown filter type %d" % kind)
        out[y] = cur
        prev = cur
    return out


def decode_png(data):
    """the bytes of a PNG file -> uint8 [H,W] (grey) or [H,W,3] (RGB)"""
    if data[:8] != SIGNATURE:
        raise ValueError("png: not a PNG file")
    at, ihdr, idat, ended = 8, None, [], False
    while at + 12 <= len(data) and not ended:
        n, kind = struct.unpack(">I4s", data[at:at + 8])
        body = data[at + 8:at + 8 + n]
        if len(body) != n or at + 12 + n > len(data):
            raise ValueError("png: truncated chunk %r" % kind)
        if struct.unpack(">I", data[at + 8 + n:at + 12 + n])[0] != zlib.crc32(kind + body) & 0xFFFFFFFF:
            raise ValueError("png: bad CRC in chunk %r" % kind)
        at += 12 + n
        if kind == b"IHDR":
            ihdr = struct.unpack(">IIBBBBB", body)
        elif kind == b"IDAT":
            idat.append(body)
        elif kind == b"IEND":
            ended = True
        elif not kind[0] & 0x20:  # an upper-case first letter: a critical chunk this reader does not know (PLTE among them)
            raise PngUnsupported("png: critical chunk %r" % kind)
    if ihdr is None or not idat or not ended:
        raise ValueError("png: IHDR, IDAT or IEND missing")
    W, H, depth, ctype, comp, filt, interlace = ihdr
    if depth != 8 or ctype not in _CHANNELS or comp != 0 or filt != 0 or interlace != 0:
        raise PngUnsupported("png: only 8-bit grey / RGB without interlacing, got depth %d colour type %d interlace %d" %
                             (depth, ctype, interlace))
    ch = _CHANNELS[ctype]
    raw = zlib.decompress(b"".join(idat))
    if len(raw) != H * (W * ch + 1):
        raise ValueError("png: %d bytes of image data, expected %d" % (len(raw), H * (W * ch + 1)))
    px = _unfilter(raw, H, W * ch, ch)
    return px.reshape(H, W) if ch == 1 else px.reshape(H, W, 3)


def read_png(path):
    with open(path, "rb") as f:
        return decode_png(f.read())
