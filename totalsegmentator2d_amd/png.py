"""A PNG writer for the visuals of :mod:`visual`: 8-bit greyscale and 8-bit RGB, non-interlaced, every scanline with filter type 0, one
IDAT chunk.  stdlib ``zlib`` and ``struct`` only (what ``sitk.WriteImage(vis, '*.png')`` is in the reference's ``Result.save``)."""
from __future__ import annotations

import struct
import zlib

import numpy as np

SIGNATURE = b'\x89PNG\r\n\x1a\n'


def _chunk(kind: bytes, data: bytes) -> bytes:
    return struct.pack('>I', len(data)) + kind + data + struct.pack('>I', zlib.crc32(kind + data) & 0xFFFFFFFF)


def encode(pixels: np.ndarray, level: int = 6) -> bytes:
    """uint8 ``[h, w]`` (greyscale) or ``[h, w, 3]`` (RGB) -> the bytes of a PNG file."""
    a = np.asarray(pixels)
    if a.dtype != np.uint8 or not (a.ndim == 2 or (a.ndim == 3 and a.shape[2] == 3)) or a.shape[0] < 1 or a.shape[1] < 1:
        raise ValueError(f"png: expected uint8 [h, w] or [h, w, 3] with h, w >= 1, found {a.dtype} {a.shape}")
    h, w = a.shape[:2]
    rows = np.zeros((h, 1 + w * (3 if a.ndim == 3 else 1)), np.uint8)      # column 0: the filter type of the scanline, 0 = None
    rows[:, 1:] = a.reshape(h, -1)
    ihdr = struct.pack('>IIBBBBB', w, h, 8, 2 if a.ndim == 3 else 0, 0, 0, 0)
    return SIGNATURE + _chunk(b'IHDR', ihdr) + _chunk(b'IDAT', zlib.compress(rows.tobytes(), level)) + _chunk(b'IEND', b'')


def write(img, path: str) -> None:
    """Write an :class:`nrrd.Image` (or an array) of a visual to ``path``."""
    data = encode(getattr(img, 'array', img))
    with open(path, 'wb') as f:
        f.write(data)
