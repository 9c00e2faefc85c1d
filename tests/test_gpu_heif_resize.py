"""Scaled HEIF output on the GPU: images of differing grid shape, item size, clap window and orientation decoded by ONE
``decode_many(..., ExportSpec(size=...))`` into slots of one size, each equal to tests/grid_resize_ref.py applied to the
C oracle's planes of its tiles; the alpha auxiliary image through the same call; the command line with two inputs."""
import os
import subprocess
import sys

import numpy as np
import pytest

import grid_ref as GR
import grid_resize_ref as GRR
import heifgen as HG
from streamgen import StreamGen
from streamgen_mono import StreamGenMono
from test_gpu_heif import _luma, tiles_stream

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SCALE = (float(np.float32(1 / (255 * 0.229))), float(np.float32(1 / (255 * 0.224))), float(np.float32(1 / (255 * 0.225))))
BIAS = (float(np.float32(-0.485 / 0.229)), float(np.float32(-0.456 / 0.224)), float(np.float32(-0.406 / 0.225)))


@pytest.fixture(scope="module")
def mods():
    from p265_amd import heif, recon
    if recon.device_count() < 1:
        pytest.fail("no HIP device visible: GPU tests must run on the MI355X box")
    return heif, recon


@pytest.fixture(scope="module")
def three():
    """(file, tiles, rows, cols, item size, crop, orientation, oriented size) of three images over one SPS and tile
    size 64 x 64: a 2 x 2 grid with clap + irot, a single hvc1 item with imir, a 2 x 3 grid."""
    out = []
    data, tiles = tiles_stream(4, 64, 64, 50, init_qp=22)
    f = HG.grid_file(data, 2, 2, (120, 100), (64, 64), transforms=[HG.clap_rect(4, 2, 100, 80, 120, 100), HG.irot(1)])
    out.append((f, tiles, 2, 2, (120, 100), (4, 16, 2, 18), 1, (80, 100)))
    data, tiles = tiles_stream(1, 64, 64, 50, init_qp=26)
    out.append((HG.single_file(data, (60, 50), transforms=[HG.imir(0)]), tiles, 1, 1, (60, 50), (0, 0, 0, 0), 4, (60, 50)))
    data, tiles = tiles_stream(6, 64, 64, 50, init_qp=30)
    out.append((HG.grid_file(data, 2, 3, (180, 120), (64, 64)), tiles, 2, 3, (180, 120), (0, 0, 0, 0), 0, (180, 120)))
    return out


def want_slot(case, spec, colour, bd=8):
    _, tiles, rows, cols, out, crop, o, _ = case
    return GRR.frame(tiles, rows, cols, out, bd, spec.format, tuple(spec.size), spec.sample, colour[0], colour[1], crop, o,
                     spec.resize, spec.scale, spec.bias)


def test_three_shapes_one_call_one_dense_array(mods, three):
    heif, recon = mods
    spec = recon.ExportSpec.named("rgb-planar-f16", size=(40, 24), resize="area", scale=SCALE, bias=BIAS)
    many = heif.decode_many([c[0] for c in three], export=spec)
    assert len(many) == 3 and many[0].frames is many[2].frames and len(many[0].frames) == 3
    dense = many[0].frames.batch_array(0).__cuda_array_interface__
    assert dense["shape"] == (3, 3, 24, 40) and dense["typestr"] == "<f2"
    host = many[0].frames.to_host()
    for k, (img, case) in enumerate(zip(many, three)):
        assert (img.index, img.width, img.height, img.orientation, img.source_size) == (k, 40, 24, case[6], case[7])
        want = want_slot(case, spec, img.colour)
        assert len(host[k]) == len(want) == 3
        for g, w in zip(host[k], want):
            assert g.shape == w.shape == (24, 40) and g.dtype == w.dtype
            np.testing.assert_array_equal(g.view(np.uint16), w.view(np.uint16))
    # one image alone through the same path gives its slot of the shared call
    one = heif.decode(three[0][0], export=spec, aux=())
    for p, q in zip(one.frames.to_host()[0], host[0]):
        np.testing.assert_array_equal(p.view(np.uint16), q.view(np.uint16))
    one.frames.free()
    many[0].frames.free()


def test_alpha_auxiliary_is_resized_with_its_image(mods):
    heif, recon = mods
    data, tiles = tiles_stream(4, 64, 64, 51)
    g = StreamGenMono(52, width=64, height=64, frames=4, idr_period=1, hash_sei="md5")
    adata, apics = g.stream(planes_fn=_luma)
    atiles = [list(_luma(prm, pic)) for prm, pic, _ in apics]
    f = HG.grid_file(data, 2, 2, (128, 120), (64, 64), transforms=[HG.imir(1)], alpha_stream=adata,
                     alpha_kw=dict(chroma_format=0))
    spec = recon.ExportSpec.named("rgb24", size=(41, 31), resize="bilinear")
    img = heif.decode(f, export=spec)
    assert (img.width, img.height, img.orientation, img.source_size) == (41, 31, 6, (128, 120)) and img.alpha is not None
    want = GRR.frame(tiles, 2, 2, (128, 120), 8, "rgb_packed", (41, 31), "u8", img.colour[0], img.colour[1], orientation=6,
                     filt="bilinear")
    np.testing.assert_array_equal(img.frames.to_host()[0][0], want[0])
    got = img.alpha.to_host()[0]
    assert len(got) == 1 and got[0].shape == (31, 41)
    np.testing.assert_array_equal(got[0], GRR.frame(atiles, 2, 2, (128, 120), 8, "planar", (41, 31), orientation=6,
                                                    filt="bilinear")[0])
    img.frames.free()
    img.alpha.free()
    # an alpha image coded 4:2:0: even sizes only, refused by name otherwise
    adata, atiles = tiles_stream(4, 64, 64, 53)
    f = HG.grid_file(data, 2, 2, (128, 120), (64, 64), transforms=[HG.irot(3)], alpha_stream=adata)
    img = heif.decode(f, export=recon.ExportSpec.named("rgb24", size=(40, 30), resize="area"))
    got = img.alpha.to_host()[0]
    np.testing.assert_array_equal(got[0], GRR.frame(atiles, 2, 2, (128, 120), 8, "planar", (40, 30), orientation=3,
                                                    filt="area")[0])
    img.frames.free()
    img.alpha.free()
    with pytest.raises(heif.UnsupportedHeif, match="alpha auxiliary image coded 4:2:0"):
        heif.decode(f, export=spec)
    assert heif.decode(f, export=spec, aux=()).alpha is None


def test_command_line_with_resize_and_two_inputs(mods, three, tmp_path):
    heif, recon = mods
    paths = []
    for k in (0, 2):
        p = tmp_path / ("%d.heic" % k)
        p.write_bytes(three[k][0])
        paths.append(str(p))
    out = tmp_path / "x.rgb"
    env = dict(os.environ, PYTHONPATH=ROOT)
    r = subprocess.run([sys.executable, "-m", "p265_amd.dec", "--heif"] + paths + ["-o", str(out), "--format", "rgb24", "--resize",
                        "40x24", "--resize-filter", "area"], check=True, env=env, cwd=ROOT, timeout=120, capture_output=True,
                       text=True)
    assert r.stdout.count("'width': 40") == 2 and r.stdout.count("'height': 24") == 2
    spec = recon.ExportSpec.named("rgb24", size=(40, 24), resize="area")
    want = b"".join(want_slot(three[k], spec, ("bt709", False))[0].tobytes() for k in (0, 2))
    assert out.read_bytes() == want
    # several files without --resize: refused on the command line
    r = subprocess.run([sys.executable, "-m", "p265_amd.dec", "--heif"] + paths + ["--format", "rgb24"], env=env, cwd=ROOT,
                       timeout=120, capture_output=True, text=True)
    assert r.returncode != 0 and "--resize" in r.stderr


def test_without_a_size_nothing_changed(mods, three):
    """The unscaled path: the grid export's frame, as tests/test_gpu_heif.py checks it; differently shaped images are
    still refused there."""
    heif, recon = mods
    f, tiles, rows, cols, out, crop, o, size = three[0]
    img = heif.decode(f, export=recon.ExportSpec.named("rgb24", upsample="bilinear"))
    assert (img.width, img.height, img.orientation, img.source_size) == (size[0], size[1], o, size)
    want = GR.frame(tiles, rows, cols, out, 8, "rgb_packed", "u8", img.colour[0], img.colour[1], "bilinear", crop, o)
    got = img.frames.to_host()[0]
    assert got[0].shape == want[0].shape == (size[1], size[0], 3)
    np.testing.assert_array_equal(got[0], want[0])
    img.frames.free()
    with pytest.raises(heif.UnsupportedHeif, match="not equally shaped"):
        heif.decode_many([three[0][0], three[2][0]], export=recon.ExportSpec.named("rgb24"))
