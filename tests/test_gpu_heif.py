"""HEIF end to end on the GPU: files written by tests/heifgen.py from tests/streamgen.py tiles (which carry an MD5 SEI of
the C oracle's decode) through heif.decode / decode_many and the command line; every frame equals tests/grid_ref.py
applied to the C oracle's planes of the tiles, bit for bit, and the tiles' MD5 SEI verifies."""
import os
import subprocess
import sys

import numpy as np
import pytest

import grid_ref as GR
import heifgen as HG
import streamgen
from oracle import c_oracle
from p265_amd import records as R
from streamgen import StreamGen
from streamgen_mono import StreamGenMono

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def mods():
    from p265_amd import heif, recon
    if recon.device_count() < 1:
        pytest.fail("no HIP device visible: GPU tests must run on the MI355X box")
    return heif, recon


def _oracle(prm, pic, scaling=None):
    return c_oracle.decode(prm, [pic], with_recon=False, scaling=scaling)[0][1]


def _luma(prm, pic, scaling=None):
    kw = R.params_dict(prm)
    kw["chroma_format_idc"] = 1
    return c_oracle.decode(R.make_params(**kw), [pic], with_recon=False, scaling=scaling)[0][1][:1]


def tiles_stream(n, w, h, seed, vui=None, **kw):
    """(Annex-B stream of n independent pictures with MD5 SEI, the oracle's planes per picture)."""
    g = StreamGen(seed, width=w, height=h, frames=n, idr_period=1, hash_sei="md5", **kw)
    if vui is not None:
        data, pics = with_vui(g, *vui)
    else:
        data, pics = g.stream(planes_fn=_oracle)
    return data, [_oracle(prm, pic) for prm, pic, _ in pics]


def with_vui(g, matrix, full_range):
    """g.stream() with the SPS VUI's video_full_range_flag and matrix_coeffs replaced: the writer's calls after
    video_format (the only 3-bit value 5) are full_range (1 bit), colour_description_present (1 bit) and three bytes."""
    base = streamgen.BitWriter

    class Patched(base):
        def __init__(self):
            super().__init__()
            self.k, self.in_ue = -1, False

        def ue(self, v):
            self.in_ue = True
            try:
                super().ue(v)
            finally:
                self.in_ue = False

        def u(self, v, n):
            if self.in_ue:
                return super().u(v, n)
            if (v, n) == (5, 3) and self.k < 0:
                self.k = 0
            elif self.k >= 0:
                self.k += 1
                if self.k == 1:
                    v = int(full_range)
                elif self.k == 5:
                    v = matrix
            return super().u(v, n)

    sps = g.sps
    def patched_sps():
        streamgen.BitWriter = Patched
        try:
            return sps()
        finally:
            streamgen.BitWriter = base
    g.sps = patched_sps
    return g.stream(planes_fn=_oracle)


def check(img, tiles, rows, cols, out, bd, recon, fmt, sample, crop=(0, 0, 0, 0), upsample="nearest", index=0):
    want = GR.frame(tiles, rows, cols, out, bd, fmt, sample, img.colour[0], img.colour[1], upsample, crop, img.orientation)
    got = img.frames.to_host()[index]
    assert len(got) == len(want)
    for g, w in zip(got, want):
        assert g.shape == w.shape and g.dtype == w.dtype
        np.testing.assert_array_equal(g, w)


def test_single_item(mods):
    heif, recon = mods
    data, tiles = tiles_stream(1, 64, 48, 31)
    img = heif.decode(HG.single_file(data, (64, 48), extents=2), export=recon.ExportSpec.named("rgb24", upsample="bilinear"))
    assert (img.width, img.height, img.bit_depth, img.orientation, img.colour) == (64, 48, 8, 0, ("bt709", False))
    assert img.frames.plane(0, 0).__cuda_array_interface__["shape"] == (48, 64, 3)
    check(img, tiles, 1, 1, (64, 48), 8, recon, "rgb_packed", "u8", upsample="bilinear")
    img.frames.free()


def test_grid_turned_then_mirrored_hash_on_device(mods):
    heif, recon = mods
    data, tiles = tiles_stream(4, 64, 64, 32)
    f = HG.grid_file(data, 2, 2, (120, 100), (64, 64), transforms=[HG.irot(1), HG.imir(0)], grid_method=1, grid_big=True,
                     build_kw=dict(infe_version=3, iloc_version=2, ipma_wide=True))
    img = heif.decode(f, export=recon.ExportSpec.named("rgb24", upsample="bilinear"), hash_on="device")
    assert (img.width, img.height, img.orientation) == (100, 120, 5)
    check(img, tiles, 2, 2, (120, 100), 8, recon, "rgb_packed", "u8", upsample="bilinear")
    plain = heif.decode(f, export=recon.ExportSpec.named("nv12"), apply_orientation=False)
    assert (plain.width, plain.height, plain.orientation) == (120, 100, 0)
    check(plain, tiles, 2, 2, (120, 100), 8, recon, "semiplanar", "native")
    # a tampered MD5 SEI (the last tile's last NAL unit ends the file) is noticed
    bad = bytearray(f)
    bad[-5] ^= 0x10
    with pytest.raises(heif.HeifError, match="hash"):
        heif.decode(bytes(bad), export=recon.ExportSpec.named("nv12"))
    img.frames.free()
    plain.frames.free()


def test_ten_bit_grid_as_p010(mods):
    heif, recon = mods
    data, tiles = tiles_stream(2, 64, 32, 33, bit_depth=10)
    f = HG.grid_file(data, 1, 2, (126, 30), (64, 32), bit_depth=10, transforms=[HG.irot(3)])
    img = heif.decode(f, export=recon.ExportSpec.named("p010"))
    assert (img.width, img.height, img.bit_depth, img.orientation) == (30, 126, 10, 3)
    check(img, tiles, 1, 2, (126, 30), 10, recon, "semiplanar", "msb16")
    img.frames.free()


def test_monochrome_alpha_auxiliary_grid(mods):
    heif, recon = mods
    data, tiles = tiles_stream(4, 64, 64, 34)
    g = StreamGenMono(35, width=64, height=64, frames=4, idr_period=1, hash_sei="md5")
    adata, apics = g.stream(planes_fn=_luma)
    atiles = [list(_luma(prm, pic)) for prm, pic, _ in apics]
    f = HG.grid_file(data, 2, 2, (128, 120), (64, 64), transforms=[HG.imir(1)], alpha_stream=adata,
                     alpha_kw=dict(chroma_format=0))
    info = heif.probe(f)
    assert info["items"][100]["aux_kind"] == "alpha" and info["items"][100]["aux_of"] == 1
    assert info["items"][100]["chroma_format"] == 0
    img = heif.decode(f, export=recon.ExportSpec.named("rgb24"))
    assert img.orientation == 6 and img.alpha is not None
    check(img, tiles, 2, 2, (128, 120), 8, recon, "rgb_packed", "u8")
    want = GR.frame(atiles, 2, 2, (128, 120), 8, "planar", orientation=6)
    got = img.alpha.to_host()[0]
    assert len(got) == 1
    np.testing.assert_array_equal(got[0], want[0])
    assert heif.decode(f, aux=()).alpha is None
    img.frames.free()
    img.alpha.free()


def test_colr_nclx_wins_over_the_vui(mods):
    """colr nclx 709 limited on a stream whose VUI says 601 full; the same stream without colr takes the VUI; an
    explicit spec wins with colour="spec"."""
    heif, recon = mods
    data, tiles = tiles_stream(1, 64, 48, 36, vui=(6, True))
    spec = recon.ExportSpec.named("rgb24", matrix="bt2020", full_range=False)
    a = heif.decode(HG.single_file(data, (64, 48), colr=HG.colr_nclx(1, 13, 1, False)), export=spec)
    b = heif.decode(HG.single_file(data, (64, 48)), export=spec)
    c = heif.decode(HG.single_file(data, (64, 48)), export=spec, colour="spec")
    assert (a.colour, b.colour, c.colour) == (("bt709", False), ("bt601", True), ("bt2020", False))
    for img in (a, b, c):
        check(img, tiles, 1, 1, (64, 48), 8, recon, "rgb_packed", "u8")
        img.frames.free()
    assert not np.array_equal(GR.frame(tiles, 1, 1, (64, 48), 8, "rgb_packed", "u8", "bt709", False)[0],
                              GR.frame(tiles, 1, 1, (64, 48), 8, "rgb_packed", "u8", "bt601", True)[0])


def test_decode_many_equals_three_single_decodes(mods):
    heif, recon = mods
    files, all_tiles = [], []
    for k in range(3):
        data, tiles = tiles_stream(2, 64, 48, 40, init_qp=22 + 4 * k)
        files.append(HG.grid_file(data, 2, 1, (60, 90), (64, 48), transforms=[HG.irot(2)]))
        all_tiles.append(tiles)
    spec = recon.ExportSpec.named("rgb-planar-f16")
    many = heif.decode_many(files, export=spec)
    assert len(many) == 3 and many[0].frames is many[2].frames and len(many[0].frames) == 3
    dense = many[0].frames.batch_array(0).__cuda_array_interface__
    assert dense["shape"] == (3, 3, 90, 60) and dense["typestr"] == "<f2"
    for k in range(3):
        assert many[k].index == k
        check(many[k], all_tiles[k], 2, 1, (60, 90), 8, recon, "rgb_planar", "f16", index=k)
        one = heif.decode(files[k], export=spec)
        for p, q in zip(one.frames.to_host()[0], many[0].frames.to_host()[k]):
            np.testing.assert_array_equal(p, q)
        one.frames.free()
    many[0].frames.free()


def test_command_line_writes_the_same_bytes(mods, tmp_path):
    heif, recon = mods
    data, tiles = tiles_stream(4, 64, 64, 41)
    path = tmp_path / "x.heic"
    path.write_bytes(HG.grid_file(data, 2, 2, (120, 100), (64, 64), transforms=[HG.irot(1)]))
    out = tmp_path / "x.rgb"
    env = dict(os.environ, PYTHONPATH=ROOT)
    r = subprocess.run([sys.executable, "-m", "p265_amd.dec", "--heif", str(path), "-o", str(out), "--format", "rgb24"],
                       check=True, env=env, cwd=ROOT, timeout=120, capture_output=True, text=True)
    assert "'width': 100" in r.stdout and "'height': 120" in r.stdout
    want = GR.frame(tiles, 2, 2, (120, 100), 8, "rgb_packed", "u8", "bt709", False, orientation=1)[0]
    assert out.read_bytes() == want.tobytes()
    r = subprocess.run([sys.executable, "-m", "p265_amd.dec", "--heif", str(path), "--probe"], check=True, env=env, cwd=ROOT,
                       timeout=120, capture_output=True, text=True)
    assert "'primary': 1" in r.stdout and "'grid'" in r.stdout
