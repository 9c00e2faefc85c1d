"""Unequal luma / chroma bit depths (p265r_params.split_bit_depth), the parts that need no GPU: the opt-in flag at
p265r_create, the params record, the parity of the two oracles on the GPU tests' pictures, the wide digest, and the
stream generator whose streams the GPU tests decode end to end."""
import ctypes

import numpy as np
import pytest

import split_cases as S
from oracle import recon_oracle as O
from p265_amd import _lib, bitstream, digest
from p265_amd import records as R


def _params_c(y, c, flag):
    p = _lib.Params()
    p.version, p.pic_width, p.pic_height, p.chroma_format_idc = 2, 64, 64, 1
    p.ctb_log2_size, p.min_tb_log2_size, p.max_tb_log2_size = 6, 2, 5
    p.bit_depth_luma, p.bit_depth_chroma, p.split_bit_depth = y, c, flag
    return p


def _create(y, c, flag):
    lib = _lib.load()
    p, h = _params_c(y, c, flag), ctypes.c_void_p()
    rc = lib.p265r_create(0, ctypes.byref(p), ctypes.byref(h))
    if rc == _lib.OK:
        lib.p265r_destroy(h)
    else:
        assert not h.value
    return rc


@pytest.mark.parametrize("y,c", [(10, 8), (8, 9), (12, 10), (8, 12)])
def test_unequal_depths_need_the_flag(y, c):
    """Without the flag unequal depths stay P265R_EUNSUPPORTED; with it p265r_create goes on to the device (P265R_OK
    where one exists, P265R_ENODEV where none does)."""
    assert _create(y, c, 0) == _lib.EUNSUPPORTED
    assert _create(y, c, 1) in (_lib.OK, _lib.ENODEV)


def test_flag_bounds():
    assert _create(13, 8, 1) == _lib.EUNSUPPORTED
    assert _create(8, 13, 1) == _lib.EUNSUPPORTED
    assert _create(7, 10, 1) == _lib.EUNSUPPORTED
    assert _create(10, 7, 1) == _lib.EUNSUPPORTED
    assert _create(10, 8, 2) == _lib.EINVAL
    assert _create(10, 10, 2) == _lib.EINVAL
    # the flag with equal depths is legal and changes nothing
    assert _create(10, 10, 1) == _create(10, 10, 0) != _lib.EUNSUPPORTED
    # monochrome ignores the flag with the chroma depth
    p, h = _params_c(10, 8, 2), ctypes.c_void_p()
    p.chroma_format_idc = 0
    rc = _lib.load().p265r_create(0, ctypes.byref(p), ctypes.byref(h))
    assert rc in (_lib.OK, _lib.ENODEV)
    if rc == _lib.OK:
        _lib.load().p265r_destroy(h)


def test_params_record():
    assert R.PARAMS_DTYPE.itemsize == 32 == ctypes.sizeof(_lib.Params)
    assert R.PARAMS_DTYPE.fields["split_bit_depth"][1] == _lib.Params.split_bit_depth.offset == 21
    assert R.PARAMS_DTYPE.fields["reserved"][0].shape == (10,)
    assert int(R.make_params()["split_bit_depth"]) == 0
    p = R.make_params(bit_depth_luma=8, bit_depth_chroma=10, split_bit_depth=1)
    assert int(p["split_bit_depth"]) == 1 and p.tobytes()[21] == 1 and not any(p.tobytes()[22:])
    assert R.params_dict(p)["split_bit_depth"] == 1
    assert R.make_params(**R.params_dict(p)).tobytes() == p.tobytes()          # (tiles.py, halo.py, pic_params)
    assert R.pic_params(p, R.Picture(None, None, None, size=(64, 64)))["split_bit_depth"] == 1
    assert [np.dtype(d) for d in R.plane_dtypes(p)] == [np.uint8, np.uint16, np.uint16]
    assert R.split_depths(p) and not R.split_depths(R.make_params(bit_depth_luma=10, bit_depth_chroma=10))
    from p265_amd import recon
    pc = recon._params_c(p)
    assert (pc.bit_depth_luma, pc.bit_depth_chroma, pc.split_bit_depth) == (8, 10, 1)
    assert bytes(pc) == p.tobytes()
    assert bitstream._params_np(pc).tobytes() == p.tobytes()


def test_validate_mirrors_the_bounds():
    params, pics, _ = S.case("narrow", 0)
    R.validate(params, pics[0])
    kw = R.params_dict(params)
    for bad in (dict(split_bit_depth=0), dict(split_bit_depth=2), dict(bit_depth_chroma=13), dict(bit_depth_luma=7)):
        with pytest.raises(R.RecordError):
            R.validate(R.make_params(**dict(kw, **bad)), pics[0])
    R.validate(R.make_params(**dict(kw, bit_depth_chroma=8, split_bit_depth=1)), pics[0])     # equal depths + flag
    for fn, arg in ((R.require_420, params), (R.require_equal_depths, params)):
        with pytest.raises(ValueError, match="unequal bit depths"):
            fn(arg, "test")


def test_tile_halo_and_multirank_paths_refuse_by_name():
    from p265_amd import dist, halo, tiles
    params, pics, _ = S.case("narrow", 1)
    for call in (lambda: tiles.tile_grid(params, pics[0]), lambda: tiles.split(params, pics[0]),
                 lambda: tiles.stitch(params, [], []), lambda: halo.TileGrid(params, [0, 5], [0, 3]),
                 lambda: dist.broadcast_params(params)):
        with pytest.raises(ValueError, match="unequal bit depths"):
            call()


@pytest.mark.parametrize("name,k", [(n, k) for n in ("tiles", "uniform") for k in range(len(S.PAIRS))] +
                         [(n, k) for n in ("narrow", "ragged", "sao_only", "no_sao_dbk", "no_sao") for k in (0, 1)])
def test_oracle_parity(name, k):
    """c_oracle.decode equals O.decode_picture on the GPU cases' pictures; the planes are typed per component."""
    params, pics, refs = S.case(name, k)
    y, c = S.PAIRS[k]
    want = [np.uint8 if y == 8 else np.uint16] + [np.uint8 if c == 8 else np.uint16] * 2
    for pic, (rec, out) in zip(pics, refs):
        rec_py, out_py = O.decode_picture(R.params_dict(R.pic_params(params, pic)), pic.as_oracle_dict())
        for ci in range(3):
            assert rec[ci].dtype == out[ci].dtype == want[ci]
            np.testing.assert_array_equal(rec[ci], rec_py[ci])
            np.testing.assert_array_equal(out[ci], out_py[ci])


@pytest.mark.parametrize("k", range(len(S.PAIRS)))
def test_uniform_case_reaches_both_clip_limits(k):
    """Y and at least one of Cb / Cr reach 0 and their own maximum in the oracle's reconstruction, so a wrong clip
    limit or a wrong row-kernel instance cannot pass the GPU comparison."""
    _, _, refs = S.case("uniform", k)
    y, c = S.PAIRS[k]
    lo = [min(int(rec[ci].min()) for rec, _ in refs) for ci in range(3)]
    hi = [max(int(rec[ci].max()) for rec, _ in refs) for ci in range(3)]
    assert lo[0] == 0 and hi[0] == (1 << y) - 1
    assert any(lo[ci] == 0 and hi[ci] == (1 << c) - 1 for ci in (1, 2))


def test_plane_digest_wide():
    rng = np.random.default_rng(5)
    p8 = rng.integers(0, 256, (6, 12)).astype(np.uint8)
    words = (p8[:, 0::2].astype(np.uint64) | (p8[:, 1::2].astype(np.uint64) << np.uint64(16))).ravel()
    m1, m2, mask = 0xbf58476d1ce4e5b9, 0x94d049bb133111eb, (1 << 64) - 1
    want = 0
    for pos, w in enumerate(words):
        z = int(w) | (pos << 32)
        z = ((z ^ (z >> 30)) * m1) & mask
        z = ((z ^ (z >> 27)) * m2) & mask
        want = (want + (z ^ (z >> 31))) & mask
    assert digest.plane_digest(p8, wide=True) == want == digest.plane_digest(p8.astype(np.uint16))
    assert digest.plane_digest(p8) != want and digest.plane_digest(p8) == digest.plane_digest(p8, wide=False)
    p16 = rng.integers(0, 1024, (6, 12)).astype(np.uint16)
    assert digest.plane_digest(p16, wide=True) == digest.plane_digest(p16)
    got = digest.picture_digest([p16, p8, p8], wide=True)
    assert got.dtype == np.uint64 and [int(v) for v in got] == [digest.plane_digest(p16), want, want]


@pytest.mark.parametrize("depths,kind", [((8, 10), "md5"), ((12, 10), "crc"), ((10, 8), "checksum"), ((8, 12), "md5")])
def test_stream_generator(depths, kind):
    """A generated stream parses to params that carry both depths and the flag; its SEI holds the hash of the C
    oracle's planes, each in its own sample width; SAO is coded only where the two depths share sao_offset_abs' cMax."""
    from streamgen_split import StreamGenSplit
    g = StreamGenSplit(40 + depths[0], depths=depths, width=136, height=72, ctb_log2=5, max_tb_log2=5, max_th_depth=2,
                       frames=2, hash_sei=kind, pcm=(3, 4, False), qp_delta_depth=1, cb_qp_offset=-1, cr_qp_offset=2)
    data, pics, refs = g.stream()
    dec = bitstream.decode_stream(data, validate=True)
    assert len(dec) == len(pics) == len(refs) == 2
    code = {"md5": bitstream.HASH_MD5, "crc": bitstream.HASH_CRC, "checksum": bitstream.HASH_CHECKSUM}[kind]
    for d, (prm, pic, poc), (rec, out) in zip(dec, pics, refs):
        assert (int(d.params["bit_depth_luma"]), int(d.params["bit_depth_chroma"])) == depths
        assert int(d.params["split_bit_depth"]) == 1 and d.params.tobytes() == prm.tobytes()
        assert int(d.params["sample_adaptive_offset"]) == int(min(depths[0], 10) == min(depths[1], 10))
        assert (d.picture.tbs["c_idx"] > 0).any() and (d.picture.tbs["flags"] & R.TB_PCM).any()
        assert [p.dtype.itemsize for p in out] == [1 if b == 8 else 2 for b in (depths[0], depths[1], depths[1])]
        assert d.hash_type == code and d.hash == [bitstream.plane_hash(p, code) for p in out]
        assert [len(h) for h in d.hash] == [{"md5": 16, "crc": 2, "checksum": 4}[kind]] * 3
    # an equal-depth SPS keeps the flag clear
    import streamgen
    eq = bitstream.decode_stream(streamgen.StreamGen(3, bit_depth=10).stream()[0])
    assert int(eq[0].params["split_bit_depth"]) == 0
