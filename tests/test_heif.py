"""p265_amd/heif.py without a device: box round trips through tests/heifgen.py, items back to Annex-B byte for byte,
the D4 composition table, clap mapping, every named refusal, seeded mutations, and the VUI colour description the
front-end carries in p265fe_picture_info.reserved."""
import os
import struct
import time

import numpy as np
import pytest

import heifgen as HG
from p265_amd import bitstream, heif
from streamgen import StreamGen

GOLDEN = os.path.join(os.path.dirname(__file__), "golden")


def stream(n=1, w=64, h=48, seed=3, **kw):
    g = StreamGen(seed, width=w, height=h, frames=n, idr_period=1, hash_sei="md5", **kw)
    return g.stream()[0]


@pytest.fixture(scope="module")
def four():
    return stream(4, 64, 64)


VARIANTS = [dict(), dict(infe_version=3, iloc_version=2, pitm_version=1, iref_version=1, ipma_version=1, ipma_wide=True),
            dict(iloc_version=0, mdat="64"), dict(mdat="end", ipma_wide=True)]


@pytest.mark.parametrize("bk", VARIANTS)
@pytest.mark.parametrize("big", [False, True])
def test_probe_gives_back_what_was_written(four, bk, big):
    idat = bk.get("iloc_version", 1) > 0
    data = HG.grid_file(four, 2, 2, (120, 100), (64, 64), transforms=[HG.irot(1), HG.imir(0)],
                        colr=HG.colr_nclx(1, 13, 1, False), grid_big=big, grid_method=1 if idat else 0,
                        extents=3, build_kw=bk)
    info = heif.probe(data)
    assert info["primary"] == 1 and "heic" in info["brands"]
    g = info["items"][1]
    assert (g["type"], g["rows"], g["cols"], g["tiles"], g["tile_size"]) == ("grid", 2, 2, [2, 3, 4, 5], (64, 64))
    assert g["coded_size"] == (120, 100) and g["size"] == (100, 120) and g["window"] == (0, 0, 120, 100)
    assert g["orientation"] == heif.COMPOSE[1][4] == 5 and g["colour"] == ("bt709", False)
    assert g["bit_depth"] == 8 and g["chroma_format"] == 1 and g["aux_kind"] is None
    for t in (2, 3, 4, 5):
        assert info["items"][t]["type"] == "hvc1" and info["items"][t]["size"] == (64, 64)
    # the ONE stream of the grid is the generator's stream
    c = heif.Container(data)
    assert heif.item_stream(c, heif._resolve(c, c.items[1])) == four


@pytest.mark.parametrize("ls", [1, 2, 4])
def test_items_back_to_annexb_for_every_nal_length_size(ls):
    s = stream(1, 16, 16, seed=5, cbf_prob=0.05, chroma_cbf_prob=0.0, split_prob=0.0, sao=False)
    assert max(len(n) for n in HG.split_nals(s)) < 256          # (1-byte lengths can hold it)
    for kw in (dict(), dict(extents=4), dict(method=1, extents=2)):
        data = HG.single_file(s, (16, 16), length_size=ls, **kw)
        c = heif.Container(data)
        info = heif._resolve(c, c.items[1])
        assert info.hvcc["length_size"] == ls
        assert heif.item_stream(c, info) == s


def _apply(a, o):
    a = np.rot90(a, o & 3)
    return a[:, ::-1] if o >> 2 else a


def test_d4_table_equals_numpy():
    A = np.arange(15).reshape(3, 5)
    for o1 in range(8):
        for o2 in range(8):
            assert np.array_equal(_apply(_apply(A, o1), o2), _apply(A, heif.COMPOSE[o1][o2])), (o1, o2)
    # imir axis 1 (top-bottom) is o = 6
    assert np.array_equal(_apply(A, 6), A[::-1])


@pytest.mark.parametrize("o", range(8))
def test_clap_after_an_orientation_maps_back(o):
    A = np.arange(12 * 20).reshape(12, 20)
    R = _apply(A, o)
    x, y, w, h = 2, 4, 6, 4
    bx, by, bw, bh = heif.map_rect_back((x, y, w, h), 20, 12, o)
    assert np.array_equal(_apply(A[by:by + bh, bx:bx + bw], o), R[y:y + h, x:x + w])


def test_transform_sequence_reduces_to_window_and_orientation(four):
    # irot 1, then a clap in the turned image (100 wide x 120 high), then imir
    data = HG.grid_file(four, 2, 2, (120, 100), (64, 64), transforms=[HG.irot(1), HG.clap_rect(10, 20, 40, 60, 100, 120),
                                                                      HG.imir(0)])
    g = heif.probe(data)["items"][1]
    A = np.arange(100 * 120).reshape(100, 120)
    want = _apply(_apply(A, 1)[20:80, 10:50], 4)
    x, y, w, h = g["window"]
    assert np.array_equal(_apply(A[y:y + h, x:x + w], g["orientation"]), want)
    assert g["size"] == (40, 60)


def _refused(data, word, cls=heif.UnsupportedHeif):
    with pytest.raises(cls) as e:
        heif.probe(data)
    assert word in str(e.value), str(e.value)


def test_every_named_refusal(four):
    one = stream(1, 64, 48)
    ok = HG.single_file(one, (64, 48))
    assert heif.probe(ok)["items"][1]["size"] == (64, 48)
    _refused(HG.single_file(one, (64, 48), brands=(b"msf1", b"hevc")), "image sequence")
    _refused(HG.single_file(one, (64, 48), brands=(b"avif", b"avis")), "brand")
    for typ in ("iovl", "iden", "av01", "jpeg"):
        _refused(HG.build([HG.Item(1, typ, b"\0" * 8, [(HG.ispe(8, 8), False)])], 1), "'%s'" % typ)
    _refused(HG.single_file(one, (64, 48), transforms=[HG.box(b"zzzz", b"\1\2")]), "essential property 'zzzz'")
    assert heif.probe(HG.single_file(one, (64, 48), colr=HG.box(b"zzzz", b"\1")))["items"][1]["size"] == (64, 48)
    _refused(HG.single_file(one, (64, 48), transforms=[HG.clap(31, 20)]), "not on whole samples")
    _refused(HG.single_file(one, (64, 48), transforms=[HG.clap_rect(3, 2, 10, 10, 64, 48)]), "odd left / top")
    _refused(HG.single_file(one, (64, 48), colr=HG.colr_nclx(1, 1, 0, True)), "matrix_coeffs 0")
    _refused(HG.single_file(one, (64, 48), colr=HG.colr_nclx(1, 1, 14, True)), "matrix_coeffs 14")
    _refused(HG.single_file(one, (64, 48), chroma_format=3), "4:4:4")
    _refused(HG.single_file(one, (64, 48), chroma_format=2), "4:2:2")
    # tiles with differing hvcC / ispe
    items = HG.grid_items(four, 2, 2, (120, 100), (64, 64), 1)
    items[2].props[1] = (HG.ispe(64, 32), False)
    _refused(HG.build(items, 1), "differing ispe")
    items = HG.grid_items(four, 2, 2, (120, 100), (64, 64), 1)
    items[3].props[0] = (HG.hvcc(HG.access_units(four)[0], 2), True)
    _refused(HG.build(items, 1), "differing hvcC")
    # malformed, not unsupported: a grid that refers to itself, a missing tile, an output outside the last tile
    items = HG.grid_items(four, 2, 2, (120, 100), (64, 64), 1)
    items[0].refs["dimg"][1] = 1
    _refused(HG.build(items, 1), "refers to itself", heif.HeifError)
    items = HG.grid_items(four, 2, 2, (120, 100), (64, 64), 1)
    items[0].refs["dimg"][1] = 77
    _refused(HG.build(items, 1), "does not exist", heif.HeifError)
    _refused(HG.grid_file(four, 2, 2, (64, 100), (64, 64)), "last tile", heif.HeifError)
    # ICC profiles are kept, never applied; unspecified matrix -> the default
    assert heif.probe(HG.single_file(one, (64, 48), colr=HG.colr_icc(b"abc")))["items"][1]["icc"] is True
    assert heif.probe(HG.single_file(one, (64, 48), colr=HG.colr_nclx(2, 2, 2, False)))["items"][1]["colour"] == ("bt601", True)
    assert heif.probe(HG.single_file(one, (64, 48), colr=HG.colr_nclx(9, 16, 9, False)))["items"][1]["colour"] == ("bt2020", False)


def _box_boundaries(data):
    out, budget = set(), heif._Budget()

    def walk(a, b, depth):
        for typ, s, e in heif._boxes(memoryview(data), a, b, budget, depth, "x"):
            out.update((s - 8, s, e))
            if typ in (b"meta",):
                walk(s + 4, e, depth + 1)
            elif typ in (b"iprp", b"ipco"):
                walk(s, e, depth + 1)
    walk(0, len(data), 0)
    return sorted(out)


def test_three_thousand_mutations_parse_or_raise_heiferror(four):
    """Byte flips, truncations at every box boundary +- 1, size fields set to 0 / 1 / 2^32 - 1 / 2^63, a self-referencing
    dimg: each either parses or raises HeifError, within a time bound per file; nothing else escapes."""
    base = HG.grid_file(four, 2, 2, (120, 100), (64, 64), transforms=[HG.irot(1)], colr=HG.colr_nclx(1, 13, 1, False),
                        alpha_stream=four, grid_method=1, extents=2)
    meta_end = base.index(b"mdat") - 4
    bounds = _box_boundaries(base)
    rng = np.random.default_rng(2024)
    cases = []
    for b in bounds:
        for d in (-1, 0, 1):
            if 0 <= b + d <= len(base):
                cases.append(base[:b + d])
    for b in bounds:
        if b + 8 <= meta_end:
            for v in (0, 1, 0xFFFFFFFF):
                cases.append(base[:b] + struct.pack(">I", v) + base[b + 4:])
            cases.append(base[:b] + struct.pack(">I", 1) + base[b + 4:b + 8] + struct.pack(">Q", 1 << 63) + base[b + 16:])
    items = HG.grid_items(four, 2, 2, (120, 100), (64, 64), 1)
    items[0].refs["dimg"] = [1, 1, 1, 1]
    cases.append(HG.build(items, 1))
    while len(cases) < 3000:
        m = bytearray(base)
        for _ in range(int(rng.integers(1, 4))):
            m[int(rng.integers(0, meta_end))] ^= 1 << int(rng.integers(0, 8))
        cases.append(bytes(m))
    parsed = 0
    for k, data in enumerate(cases):
        t0 = time.perf_counter()
        try:
            heif.probe(data)
            parsed += 1
        except heif.HeifError:
            pass
        assert time.perf_counter() - t0 < 1.0, k
    assert len(cases) >= 3000 and 0 < parsed < len(cases)


def test_reserved_carries_the_vui_colour_description():
    """A generated stream's VUI says video_signal_type present, limited range, matrix_coeffs 1; sanity.bin has none."""
    d = bitstream.decode_stream(stream(1, 64, 48))[0]
    assert d.colour == (1, False)
    assert bitstream.colour_of(0x8000 | 0x100 | 9) == (9, True) and bitstream.colour_of(0) is None
    s = bitstream.decode_stream(open(os.path.join(GOLDEN, "sanity.bin"), "rb").read())[0]
    assert s.colour is None


def test_a_chain_of_grids_is_cut_at_its_first_link():
    """1200 chained 1 x 1 grid items (each the only tile of the one before): a grid of derived images is refused at the
    first link -- no recursion, whatever the chain's length -- and probing every item stays quick."""
    one = stream(1, 64, 48)
    ps, aus = HG.access_units(one)
    n = 1200
    items = [HG.Item(k, "grid", HG.grid_payload(1, 1, 64, 48), [(HG.ispe(64, 48), False)], refs={"dimg": [k + 1]})
             for k in range(1, n + 1)]
    items.append(HG.Item(n + 1, "hvc1", HG.length_prefixed(aus[0]), [(HG.hvcc(ps), True), (HG.ispe(64, 48), False)]))
    data = HG.build(items, 1)
    t0 = time.perf_counter()
    _refused(data, "grid of derived images")
    info = heif.probe(HG.build(items, n))                  # the last link is a plain grid over an hvc1 tile
    assert time.perf_counter() - t0 < 5.0
    assert info["items"][n]["tiles"] == [n + 1] and "derived" in info["items"][1]["error"]


def test_extents_cannot_add_up_to_more_than_the_file():
    """65535 extents of length 0 (each the whole file): refused as malformed, nothing of that size is ever joined."""
    one = stream(1, 64, 48)
    data = bytearray(HG.single_file(one, (64, 48), extents=1))
    c = heif.Container(bytes(data))
    c.items[1].extents = [(0, 0, 0)] * 65535
    with pytest.raises(heif.HeifError, match="add up to more than the file"):
        c.item_bytes(c.items[1])
    # through the file: an iloc written with that many zero-length extents
    it = HG.Item(1, "hvc1", b"", [(HG.hvcc(HG.access_units(one)[0]), True), (HG.ispe(64, 48), False)])
    it.zero_extents = 4000
    blob = HG.build([it], 1)
    with pytest.raises(heif.HeifError):
        c = heif.Container(blob)
        heif.item_stream(c, heif._resolve(c, c.items[1]))
