"""Encode -> parse round trips of monochrome (chroma_format_idc 0) streams (CPU only).

tests/streamgen_mono.py writes ChromaArrayType 0 syntax from random decisions and builds the records with
frontend.PictureBuilder; libp265fe.so must parse each stream back into exactly those records (CTUs, TBs,
coefficients, nofilter map), with the parameters the back-end takes (chroma_format_idc 0, one bit depth, no chroma
QP offsets), the conformance window in luma samples, the POC order and the one-component picture hash."""
import numpy as np
import pytest

import streamgen
from streamgen_mono import StreamGenMono, luma_hash
from p265_amd import bitstream

CASES = {
    "ctb16": dict(),
    "ctb32": dict(ctb_log2=5, min_cb_log2=3, max_tb_log2=5, max_th_depth=2, width=136, height=72),
    "ctb64_ragged": dict(width=200, height=72, ctb_log2=6, max_tb_log2=5, max_th_depth=2),
    "tiles_wpp": dict(tiles=(2, 2), wpp=True),
    "tiles": dict(tiles=(2, 2), lf_across_tiles=0),
    "wpp": dict(wpp=True),
    "slices_dependent": dict(slices=[(0, False), (13, False), (30, True)], deblocking="override"),
    "tiles_slices": dict(tiles=(3, 2), slices=[(0, False), (16, False), (20, True)]),
    # a quantization group below the CU that opens it: with cbfChroma = 0 a CU whose luma cbfs are all zero
    # codes no cu_qp_delta_abs, and the next CU of the group does
    "qp_delta_d1": dict(qp_delta_depth=1, cbf_prob=0.45),
    "qp_delta_d2_ctb32": dict(qp_delta_depth=2, ctb_log2=5, width=192, height=128, cbf_prob=0.5),
    "pcm_lf_off": dict(pcm=(3, 4, True)),
    "pcm_bypass": dict(pcm=(3, 3, False), bypass=True),
    "bypass_tskip_sdh": dict(bypass=True, tskip=True, sign_hiding=True, tskip_prob=0.6),
    "plain": dict(sign_hiding=False, tskip=False, sao=False, strong=False, deblocking="off"),
    "scaling_sps": dict(scaling_lists="sps"),
    "chroma_qp_offsets_ignored": dict(slice_chroma_offsets=(3, -5), cb_qp_offset=-4, cr_qp_offset=6, qp_delta_depth=1),
    "bd8_chroma12": dict(sps_bit_depth_chroma=12, pcm=(3, 4, False)),
    "bd10_chroma8": dict(bit_depth=10, sps_bit_depth_chroma=8, qp_delta_depth=1, init_qp=14, slice_qp_delta=-20,
                         pcm=(3, 4, True)),
    "bd12_chroma9_tiles": dict(bit_depth=12, sps_bit_depth_chroma=9, tiles=(2, 2), qp_delta_depth=1, init_qp=4,
                               slice_qp_delta=-25, pcm=(3, 4, True)),
    "five_frames_reordered": dict(frames=5, poc_order=[0, 4, 2, 1, 3], max_reorder=2),
}


def roundtrip(seed, threads=2, **cfg):
    g = StreamGenMono(seed, **cfg)
    data, pics = g.stream()
    dec = bitstream.decode_stream(data, threads=threads, validate=True)
    assert len(dec) == len(pics)
    for d, (prm, p, poc) in zip(dec, pics):
        assert int(d.params["chroma_format_idc"]) == 0
        assert int(d.params["bit_depth_chroma"]) == int(d.params["bit_depth_luma"]) == g.bd
        assert int(d.params["pps_cb_qp_offset"]) == int(d.params["pps_cr_qp_offset"]) == 0
        assert d.params.tobytes() == prm.tobytes()
        assert d.poc == poc
        assert (p.tbs["c_idx"] == 0).all() and len(p.tbs) > 0
        assert np.array_equal(d.picture.ctus, p.ctus)
        assert not d.picture.ctus["sao_type"][:, 1:].any()
        assert np.array_equal(d.picture.tbs, p.tbs)
        assert np.array_equal(d.picture.coef, p.coef)
        if g.scaling_factors is None:
            assert d.scaling is None
        else:
            assert np.array_equal(d.scaling, g.scaling_factors)
        if p.nofilter is None:
            assert d.picture.nofilter is None
        else:
            assert np.array_equal(d.picture.nofilter, p.nofilter)
    return g, data, dec


@pytest.mark.parametrize("name", sorted(CASES))
@pytest.mark.parametrize("seed", [0, 1])
def test_roundtrip(name, seed):
    g, _, dec = roundtrip(2000 + 17 * seed + len(name), **CASES[name])
    pic = dec[0].picture
    if CASES[name].get("pcm"):
        assert (pic.tbs["flags"] & 8).any()
    if CASES[name].get("qp_delta_depth") is not None:
        assert len(set(int(q) for q in pic.tbs["qp"])) > 2


def test_luma_sao_parameters_are_parsed():
    """sao() with one component: band and edge offsets of luma reach the records (a slice draws slice_sao_luma_flag
    with probability 0.85, so a few seeds are enough to see both types)."""
    seen = set()
    for seed in range(6):
        _, _, dec = roundtrip(300 + seed, slices=[(0, False), (24, False)])
        seen |= set(int(t) for t in dec[0].picture.ctus["sao_type"][:, 0])
    assert seen == {0, 1, 2}


def test_odd_conformance_window():
    """SubWidthC = SubHeightC = 1: the window offsets are luma samples, odd ones included."""
    g, _, dec = roundtrip(9, conf_window=(1, 3, 2, 5), width=136, height=104)
    assert dec[0].crop == (1, 3, 2, 5)


def test_output_order_of_reordered_frames():
    g, _, dec = roundtrip(5, frames=5, poc_order=[0, 4, 2, 1, 3], max_reorder=2)
    assert [d.poc for d in dec] == [0, 4, 2, 1, 3]
    assert [d.output_rank for d in dec] == [0, 4, 2, 1, 3]
    assert [d.nal_unit_type for d in dec] == [19, 1, 1, 1, 1]


@pytest.mark.parametrize("bd", [8, 10])
@pytest.mark.parametrize("kind", ["md5", "crc", "checksum"])
def test_one_component_hash_sei(kind, bd):
    """The SEI of a monochrome picture carries one component; placeholder bytes and a real plane's hash."""
    g = StreamGenMono(11, hash_sei=kind, bit_depth=bd)
    data, pics = g.stream()
    dec = bitstream.decode_stream(data)
    assert dec[0].hash_type == g.last_hash[0] and dec[0].hash == g.last_hash[1] and len(dec[0].hash) == 1
    rng = np.random.default_rng(bd)
    plane = rng.integers(0, 1 << bd, (96, 128)).astype(np.uint8 if bd == 8 else np.uint16)
    g = StreamGenMono(12, hash_sei=kind, bit_depth=bd)
    data, pics = g.stream(lambda params, pic: [plane, None, None])
    dec = bitstream.decode_stream(data)
    code = {"md5": bitstream.HASH_MD5, "crc": bitstream.HASH_CRC, "checksum": bitstream.HASH_CHECKSUM}[kind]
    assert dec[0].hash == luma_hash([plane], kind) == [bitstream.plane_hash(plane, code)]
    assert dec[0].hash == streamgen.picture_hash([plane], kind)


def test_chunked_feeding_equals_one_shot():
    g = StreamGenMono(21, frames=4, tiles=(2, 2), slices=[(0, False), (10, False), (20, True)], hash_sei="md5",
                      poc_order=[0, 3, 1, 2], max_reorder=2, pcm=(3, 4, True))
    data, pics = g.stream()
    whole = bitstream.decode_stream(data, threads=2)
    for size in (1, 7, 256, 4096):
        parser = bitstream.StreamParser(threads=2)
        got = []
        for i in range(0, len(data), size):
            got += parser.feed(data[i:i + size])
        got += parser.feed(b"", flush=True)
        assert len(got) == len(whole) == 4
        for a, b in zip(got, whole):
            assert a.params.tobytes() == b.params.tobytes() and a.poc == b.poc
            assert a.output_rank == -1                  # (a streaming parser leaves the order to the OutputQueue)
            assert a.hash == b.hash and a.crop == b.crop
            assert np.array_equal(a.picture.ctus, b.picture.ctus) and np.array_equal(a.picture.tbs, b.picture.tbs)
            assert np.array_equal(a.picture.coef, b.picture.coef)


@pytest.mark.parametrize("idc", [2, 3])
def test_other_chroma_formats_stay_unsupported(idc):
    data, _ = StreamGenMono(3, chroma_format_idc=idc).stream()
    with pytest.raises(bitstream.UnsupportedStream, match="chroma_format_idc"):
        bitstream.decode_stream(data)


def test_separate_colour_planes_stay_unsupported():
    data, _ = StreamGenMono(3, chroma_format_idc=3, separate_colour_plane=1).stream()
    with pytest.raises(bitstream.UnsupportedStream, match="separate_colour_plane"):
        bitstream.decode_stream(data)


def test_420_streams_parse_as_before():
    """The 4:2:0 generator's stream still yields chroma records and three hash components."""
    g = streamgen.StreamGen(4, hash_sei="crc")
    data, pics = g.stream()
    dec = bitstream.decode_stream(data)
    assert int(dec[0].params["chroma_format_idc"]) == 1 and (dec[0].picture.tbs["c_idx"] > 0).any()
    assert len(dec[0].hash) == 3 and np.array_equal(dec[0].picture.tbs, pics[0][1].tbs)
