"""The picture hash arithmetic shared by the host and the device (p265_amd/csrc/pichash_math.h) through
p265r_plane_hash_host, against hashlib and bitstream.plane_hash (hashlib, p265fe_plane_hash, numpy).  No GPU."""
import ctypes
import hashlib
import os
import re

import numpy as np
import pytest

from p265_amd import _lib, bitstream, recon

HEADER = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "p265r.h")
TYPES = (_lib.HASH_MD5, _lib.HASH_CRC, _lib.HASH_CHECKSUM)
# (width, height); (8, 4) and (24, 12) are there for the residue 32 of the byte count mod 64 at one byte per sample
SHAPES = [(4, 4), (8, 8), (12, 4), (36, 20), (68, 36), (260, 260), (520, 264), (8, 4), (24, 12)]
SEGS = (0, 1, 3, 16, 64, 1000)
DTYPES = ((np.uint8, 255), (np.uint16, 4095))


def _plane(dtype, mx, w, h, padded, seed):
    rng = np.random.default_rng(seed)
    full = rng.integers(0, mx + 1, (h, w + 24), dtype=dtype)
    return full[:, :w] if padded else np.ascontiguousarray(full[:, :w])


def test_shape_list_covers_every_residue_and_both_mask_halves():
    """The byte count mod 64 decides where MD5's padding falls: a plane is a multiple of 16 samples, so 0 / 16 /
    32 / 48 exist at one byte per sample and 0 / 32 at two.  x >= 256 and y >= 256 reach the mask's high terms."""
    assert {w * h % 64 for w, h in SHAPES} == {0, 16, 32, 48}
    assert {2 * w * h % 64 for w, h in SHAPES} == {0, 32}
    assert any(w > 256 for w, _ in SHAPES) and any(h > 256 for _, h in SHAPES)
    assert all(w % 4 == 0 and h % 4 == 0 for w, h in SHAPES)


@pytest.mark.parametrize("dtype,mx", DTYPES, ids=["u8", "u16"])
@pytest.mark.parametrize("w,h", SHAPES)
def test_host_function_equals_the_existing_hashes(dtype, mx, w, h):
    for padded in (False, True):
        p = _plane(dtype, mx, w, h, padded, 100 * w + h + padded)
        assert (p.strides[0] > w * p.itemsize) == padded
        tight = np.ascontiguousarray(p)
        for t in TYPES:
            want = bitstream.plane_hash(tight, t)
            if t == _lib.HASH_MD5:
                assert want == hashlib.md5(tight.astype("<u%d" % p.itemsize).tobytes()).digest()
            for seg in SEGS:
                assert recon.plane_hash_host(p, t, seg) == want, (w, h, t, seg, padded)


@pytest.mark.parametrize("dtype,mx", DTYPES, ids=["u8", "u16"])
def test_zero_planes_and_one_maximal_sample_at_either_end(dtype, mx):
    """An all-zero plane (the CRC is its initial-value term alone), and one maximal sample at the first and at
    the last position: the CRC's largest and smallest position exponent."""
    for w, h in ((8, 8), (36, 20), (520, 264)):
        for where in (None, (0, 0), (h - 1, w - 1)):
            p = np.zeros((h, w), dtype)
            if where is not None:
                p[where] = np.iinfo(dtype).max
            for t in TYPES:
                want = bitstream.plane_hash(p, t)
                for seg in (0, 1, 16, 1000):
                    assert recon.plane_hash_host(p, t, seg) == want, (w, h, where, t, seg)


def test_rejections():
    lib = _lib.load()
    buf = np.zeros((16, 32), np.uint8)
    out = (ctypes.c_uint8 * 16)()

    def call(plane=buf.ctypes.data, w=16, h=16, stride=32, bps=1, t=0, seg=0, o=out):
        return lib.p265r_plane_hash_host(plane, w, h, stride, bps, t, seg, o)

    assert call() == _lib.OK
    assert call(bps=2, stride=32) == _lib.OK
    assert call(plane=None) == _lib.EINVAL
    assert call(o=None) == _lib.EINVAL
    for w, h in ((0, 16), (16, 0), (-4, 16), (16, -4), (14, 16), (16, 6), (18, 16)):
        assert call(w=w, h=h) == _lib.EINVAL, (w, h)
    for bps in (0, 3, 4):
        assert call(bps=bps) == _lib.EINVAL
    assert call(stride=15) == _lib.EINVAL
    assert call(bps=2, stride=31) == _lib.EINVAL
    for t in (-1, 3, 16):
        assert call(t=t) == _lib.EINVAL
    with pytest.raises(_lib.P265RError):
        recon.plane_hash_host(buf, 3)


def test_constants_header_and_exports():
    assert (_lib.HASH_MD5, _lib.HASH_CRC, _lib.HASH_CHECKSUM) == (bitstream.HASH_MD5, bitstream.HASH_CRC, bitstream.HASH_CHECKSUM)
    txt = open(HEADER).read()
    fe = open(os.path.join(os.path.dirname(HEADER), "p265fe.h")).read()
    for name, val in (("MD5", 0), ("CRC", 1), ("CHECKSUM", 2)):
        assert int(re.search(r"#define\s+P265R_HASH_%s\s+(\d+)" % name, txt).group(1)) == val
        assert int(re.search(r"#define\s+P265FE_HASH_%s\s+(\d+)" % name, fe).group(1)) == val
    lib = _lib.load()
    for fn in ("p265r_batch_hash_async", "p265r_batch_hash_read", "p265r_plane_hash_host"):
        assert re.search(r"\b%s\s*\(" % fn, txt), fn
        assert hasattr(lib, fn) and fn in _lib.SIGNATURES, fn
    assert lib.p265r_abi_version() == 2
    # the ABI calls refuse NULL before they touch a device
    assert lib.p265r_batch_hash_async(None, None, 0) == _lib.EINVAL
    assert lib.p265r_batch_hash_read(None, None, None, 0) == _lib.EINVAL


def test_unknown_hash_on_raises_before_anything_starts():
    from p265_amd import decoder
    import threading
    before = threading.active_count()
    with pytest.raises(ValueError):
        decoder.decode_bytes(b"", hash_on="gpu")
    with pytest.raises(ValueError):
        next(decoder.decode_chunks(iter([b""]), hash_on=None))
    with pytest.raises(ValueError):
        decoder.decode_file(os.path.join(os.path.dirname(__file__), "golden", "sanity.bin"), hash_on="Device")
    assert threading.active_count() <= before                     # no parser or submitter thread was started
    from p265_amd import dec
    assert dec.parse_cmd(["-b", "x"]).hash_on == "host" and dec.parse_cmd(["-b", "x", "--hash-on", "device"]).hash_on == "device"
    with pytest.raises(SystemExit):
        dec.parse_cmd(["-b", "x", "--hash-on", "gpu"])
