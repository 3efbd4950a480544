"""Baseline-JPEG views without PIL (include/poem_hip.h "baseline JPEG"): :class:`EncodedImage`, the handle a record's
``image_<i>.jpg`` member stays when the dataset is built with ``image_decode="device"``, and the ctypes mirror of
``poem_jpeg_desc_t``.  The decode itself happens in ``transform.warp_views``: Huffman decoding on host threads into the pinned
staging buffer, reconstruction on the GPU into the blob ``poem_warp_affine`` reads.  A stream the library refuses (progressive,
CMYK, out-of-range data, damaged, ...) is decoded by PIL instead -- the device route returns PIL's bytes or is not taken."""
import ctypes
import io

import numpy as np


class JpegDesc(ctypes.Structure):
    """include/poem_hip.h poem_jpeg_desc_t"""
    _fields_ = [("status", ctypes.c_int32), ("height", ctypes.c_int32), ("width", ctypes.c_int32), ("ncomp", ctypes.c_int32),
                ("hs", ctypes.c_int32), ("vs", ctypes.c_int32), ("blocks_w", ctypes.c_int32 * 3), ("blocks_h", ctypes.c_int32 * 3),
                ("coef_offset", ctypes.c_int64), ("coef_bytes", ctypes.c_int64), ("block_base", ctypes.c_int64),
                ("quad_base", ctypes.c_int64), ("quant", (ctypes.c_uint16 * 64) * 3)]


DESC_BYTES = ctypes.sizeof(JpegDesc)
assert DESC_BYTES == 464


class JpegScan(ctypes.Structure):
    """include/poem_hip.h poem_jpeg_scan_t (the device entropy route)"""
    _fields_ = [("byte_offset", ctypes.c_int64), ("byte_count", ctypes.c_int64), ("sub_base", ctypes.c_int64),
                ("sub_count", ctypes.c_int32), ("restart", ctypes.c_int32), ("table_base", ctypes.c_int32),
                ("table_count", ctypes.c_int32), ("dc_sel", ctypes.c_uint8 * 3), ("ac_sel", ctypes.c_uint8 * 3),
                ("reserved", ctypes.c_uint8 * 2)]


SCAN_BYTES = ctypes.sizeof(JpegScan)
HUFF_BYTES = 1424                                            # sizeof(poem_jpeg_huff_t)
assert SCAN_BYTES == 48


def jpeg_size(data):
    """(height, width) from the frame header of a JPEG stream (any SOFn), without decoding; ValueError if there is none."""
    n, pos = len(data), 2
    if data[:2] != b"\xff\xd8":
        raise ValueError("not a JPEG stream")
    while pos + 4 <= n:
        if data[pos] != 0xFF:
            raise ValueError("bad JPEG marker")
        m = data[pos + 1]
        if m == 0xFF:
            pos += 1
            continue
        if m in (0x01, 0xD8) or 0xD0 <= m <= 0xD7:
            pos += 2
            continue
        if 0xC0 <= m <= 0xCF and m not in (0xC4, 0xC8, 0xCC):
            if pos + 9 > n:
                break
            return int.from_bytes(data[pos + 5:pos + 7], "big"), int.from_bytes(data[pos + 7:pos + 9], "big")
        if m in (0xD9, 0xDA):
            break
        pos += 2 + int.from_bytes(data[pos + 2:pos + 4], "big")
    raise ValueError("JPEG stream without a frame header")


class EncodedImage:
    """An undecoded JPEG view: holds the bytes, knows its ``shape == (H, W, 3)`` from the header, and turns into PIL's pixels
    wherever an array is asked for (``np.asarray(handle)``, ``np.array(handle, copy=True)``) -- so host code that touches pixels
    (the occlusion patch, a user's own code) sees exactly what ``decode_rgb8`` gives today."""
    __slots__ = ("data", "shape", "entropy")
    dtype = np.dtype(np.uint8)
    ndim = 3

    def __init__(self, data, entropy=None):
        self.data = bytes(data)
        self.entropy = entropy                                   # "device": warp_views Huffman-decodes this view on the GPU
        h, w = jpeg_size(self.data)
        self.shape = (h, w, 3)

    @property
    def size(self):
        return self.shape[0] * self.shape[1] * 3

    @property
    def coef_bound(self):
        """Bytes that hold this image's int16 DCT coefficients whatever its sampling: three components on a grid padded to whole
        16x16 MCUs (what ``poem_jpeg_entropy_decode`` asks for is at most this)."""
        return 3 * 128 * (2 * -(-self.shape[0] // 16)) * (2 * -(-self.shape[1] // 16))

    def decode(self):
        from PIL import Image
        with Image.open(io.BytesIO(self.data)) as im:
            return np.asarray(im.convert("RGB"), dtype=np.uint8)

    def __array__(self, dtype=None, copy=None):
        out = self.decode()
        if dtype is not None and np.dtype(dtype) != out.dtype:
            return out.astype(dtype)
        return out.copy() if copy else out                       # (PIL's buffer is read-only: a requested copy must be writable)

    def __repr__(self):
        return f"EncodedImage({self.shape[0]}x{self.shape[1]}, {len(self.data)} bytes)"
