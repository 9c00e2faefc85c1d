"""Device-side picture hash (p265r_batch_hash_async / _read, decoder hash_on="device") on the MI355X.  The
expectation is always the host hash (bitstream.plane_hash) of the planes download() returns for the same batch."""
import os

import numpy as np
import pytest

import planted_lf
from p265_amd import _lib, bitstream, synth
from p265_amd import records as R

pytestmark = pytest.mark.gpu

GOLDEN = os.path.join(os.path.dirname(__file__), "golden")
TYPES = (_lib.HASH_MD5, _lib.HASH_CRC, _lib.HASH_CHECKSUM)
# (8, 8), (16, 8), (24, 8), (32, 8): the smallest pictures, chroma planes of 16 / 32 / 48 / 64 samples; (72, 40):
# chroma rows of 36 samples (a tail behind two 16-byte loads at 8 bits); (528, 520): x and y >= 256 in luma and chroma
RAGGED = [(8, 8), (16, 8), (24, 8), (32, 8), (72, 40), (136, 72), (528, 520)]


@pytest.fixture(scope="module")
def recon_mod():
    from p265_amd import recon
    if recon.device_count() < 1:
        pytest.fail("no HIP device visible: GPU tests must run on the MI355X box")
    return recon


def want_hashes(planes, hash_type):
    return [[bitstream.plane_hash(p, hash_type) for p in pic] for pic in planes]


def check_batch(ctx, b, types=TYPES):
    """Every type on the device against the host hash of the batch's downloaded planes; -> the planes."""
    planes = ctx.download(b)
    for t in types:
        got = ctx.picture_hash(b, t)
        want = want_hashes(planes, t)
        for i, (g, w) in enumerate(zip(got, want)):
            assert g == w, (t, i, planes[i][0].shape, [x.hex() for x in g], [x.hex() for x in w])
    return planes


def test_ragged_sizes_cover_every_residue():
    chroma = [(w // 2) * (h // 2) for w, h in RAGGED]
    assert {n % 64 for n in chroma} == {0, 16, 32, 48} and {2 * n % 64 for n in chroma} == {0, 32}
    assert any(w // 2 > 256 and h // 2 > 256 for w, h in RAGGED)
    assert any(w < max(x for x, _ in RAGGED) for w, _ in RAGGED)       # stride != row bytes for some picture


@pytest.mark.parametrize("bd", [8, 10, 12])
def test_ragged_batch_every_type(recon_mod, bd):
    big = R.make_params(pic_width=528, pic_height=520, ctb_log2_size=5, bit_depth_luma=bd, bit_depth_chroma=bd)
    pics = []
    for k, (w, h) in enumerate(RAGGED):
        pp = R.pic_params(big, R.Picture(ctus=None, tbs=None, coef=None, size=(w, h)))
        pic = synth.make_picture(pp, 7300 + 5 * k + bd, perf=bool(k % 2), deblocking=True, sao=True)
        pic.size = (w, h)
        pics.append(pic)
    with recon_mod.ReconContext(big) as ctx:
        b = ctx.upload(pics)
        ctx.run(b)
        planes = check_batch(ctx, b)
        b.free()
    assert [p[0].shape for p in planes] == [(h, w) for w, h in RAGGED]
    assert any(p[0].shape[1] < 528 for p in planes)


def test_130_small_pictures_in_one_batch(recon_mod):
    """More planes than one wave of MD5 chains; the accumulators of many pictures."""
    params = R.make_params(pic_width=16, pic_height=16, ctb_log2_size=4)
    pics = [synth.make_picture(params, 7500 + k, deblocking=True) for k in range(130)]
    with recon_mod.ReconContext(params) as ctx:
        b = ctx.upload(pics)
        ctx.run(b)
        planes = check_batch(ctx, b)
        raw = None
        for t in TYPES:
            ctx.hash_async(b, t)
            raw = ctx.hash_read(b)
            assert raw.shape == (130, 3, 16) and raw.dtype == np.uint8
            assert not raw[:, :, _lib.HASH_BYTES[t]:].any()
        b.free()
    assert len({p[0].tobytes() for p in planes}) > 100                   # (the pictures differ)


@pytest.mark.parametrize("bd", [8, 10])
def test_planted_pcm_planes(recon_mod, bd):
    """PCM pictures with the in-loop filters off: the decoded planes ARE the planted ones -- all zero, all max,
    one maximal sample at the first / at the last position of each plane."""
    w = h = 64
    mx = (1 << bd) - 1
    dt = np.uint16 if bd > 8 else np.uint8
    shapes = [(h, w), (h // 2, w // 2), (h // 2, w // 2)]
    sets = [[np.zeros(s, dt) for s in shapes], [np.full(s, mx, dt) for s in shapes],
            [np.zeros(s, dt) for s in shapes], [np.zeros(s, dt) for s in shapes]]
    for p in sets[2]:
        p[0, 0] = mx
    for p in sets[3]:
        p[-1, -1] = mx
    pics = []
    for planes in sets:
        spec = planted_lf.Spec(bd, 4, 16, w, h)
        spec.dbk[:] = False
        pics.append(planted_lf.build(spec, planes, "a", sao=False))
    params = planted_lf.params_of(bd, 4, "a", False, w, h)
    with recon_mod.ReconContext(params) as ctx:
        b = ctx.upload(pics)
        ctx.run(b)
        got = check_batch(ctx, b)
        b.free()
    for g, planes in zip(got, sets):
        for a, p in zip(g, planes):
            np.testing.assert_array_equal(a, p)


def test_sanity_frames(recon_mod):
    dec = bitstream.decode_stream(open(os.path.join(GOLDEN, "sanity.bin"), "rb").read())
    assert len(dec) == 3
    for d in dec:
        with recon_mod.ReconContext(d.params, scaling=d.scaling) as ctx:
            b = ctx.upload([d.picture])
            ctx.run(b)
            check_batch(ctx, b)
            b.free()


def test_call_order(recon_mod):
    params = R.make_params(pic_width=72, pic_height=40, ctb_log2_size=4)
    pics = [synth.make_picture(params, 7600 + k, deblocking=True) for k in range(3)]
    spec = recon_mod.ExportSpec(format="semiplanar", crop=(2, 2, 0, 2))
    with recon_mod.ReconContext(params) as ctx:
        b = ctx.upload(pics)
        with pytest.raises(_lib.P265RError) as e:
            ctx.hash_async(b, _lib.HASH_MD5)                    # never run
        assert e.value.code == _lib.ESTATE
        ctx.run(b)
        with pytest.raises(_lib.P265RError) as e:
            ctx.hash_read(b)                                    # nothing enqueued yet
        assert e.value.code == _lib.ESTATE
        with pytest.raises(_lib.P265RError) as e:
            ctx.hash_async(b, 3)
        assert e.value.code == _lib.EINVAL
        out = np.zeros(48 * 3, np.uint8)
        import ctypes
        ptr = out.ctypes.data_as(ctypes.POINTER(ctypes.c_uint8))
        ctx.hash_async(b, _lib.HASH_CHECKSUM)
        assert ctx.lib.p265r_batch_hash_read(ctx.handle, b.handle, ptr, 48 * 3 - 1) == _lib.EINVAL
        assert ctx.lib.p265r_batch_hash_read(ctx.handle, b.handle, None, 48 * 3) == _lib.EINVAL
        # a later call overwrites the buffer
        ctx.hash_async(b, _lib.HASH_MD5)
        ctx.hash_async(b, _lib.HASH_CRC)
        raw = ctx.hash_read(b)
        planes = ctx.download(b)
        want = want_hashes(planes, _lib.HASH_CRC)
        for i in range(3):
            for c in range(3):
                assert raw[i, c, :2].tobytes() == want[i][c] and not raw[i, c, 2:].any()
        # behind an export on the same lane: the exported frames are those of an export made without it
        alone = ctx.export(b, spec)
        ref = [[p.copy() for p in fr] for fr in alone.to_host()]
        alone.free()
        fr = ctx.export(b, spec)
        ctx.hash_async(b, _lib.HASH_MD5)
        got = fr.to_host()
        assert ctx.hash_read(b)[:, :, :16].tobytes() == b"".join(x for pic in want_hashes(planes, _lib.HASH_MD5) for x in pic)
        for g, r in zip(got, ref):
            for a, p in zip(g, r):
                np.testing.assert_array_equal(a, p)
        fr.free()
        b.free()


# ---- decoder --------------------------------------------------------------------------------------------------
def _boom(*a, **kw):
    raise AssertionError("not to be called with hash_on='device'")


def _device_decode_equals_host(recon_mod, monkeypatch, data, spec, n, **kw):
    from p265_amd import decoder
    host = decoder.decode_bytes(data, export=spec, **kw)
    want = [f.device.tobytes() for f in host]
    assert len(host) == n and all(f.hash_ok is True for f in host)
    for f in host:
        f.device.release()
    with monkeypatch.context() as m:
        m.setattr(recon_mod.ReconContext, "download", _boom)      # no plane comes back
        m.setattr(bitstream, "plane_hash", _boom)                 # nothing is hashed on the host
        dev = decoder.decode_bytes(data, export=spec, hash_on="device", **kw)
        assert len(dev) == n
        for f, w in zip(dev, want):
            assert f.hash_ok is True and f.planes is None and f.device is not None
            assert f.device.tobytes() == w
            f.device.release()


@pytest.mark.parametrize("name,fmt,n", [("synth_1080p_4pic.bin", "nv12", 4), ("synth_main10.bin", "p010", 3)])
def test_decoder_export_md5_streams(recon_mod, monkeypatch, name, fmt, n):
    data = open(os.path.join(GOLDEN, name), "rb").read()
    _device_decode_equals_host(recon_mod, monkeypatch, data, recon_mod.ExportSpec.named(fmt), n)


@pytest.mark.parametrize("kind", ["crc", "checksum"])
def test_decoder_export_crc_and_checksum_streams(recon_mod, monkeypatch, kind):
    import streamgen
    from oracle import c_oracle
    g = streamgen.StreamGen(81, hash_sei=kind, width=136, height=104, frames=3)
    data, _ = g.stream(planes_fn=lambda prm, pic, scaling=None: c_oracle.decode(prm, [pic], with_recon=False,
                                                                                 scaling=scaling)[0][1])
    assert {d.hash_type for d in bitstream.decode_stream(data)} == {{"crc": 1, "checksum": 2}[kind]}
    _device_decode_equals_host(recon_mod, monkeypatch, data, recon_mod.ExportSpec.named("nv12"), 3, batch=2)


def test_decoder_without_export_returns_planes_and_hashes_on_the_device(recon_mod, monkeypatch):
    from p265_amd import decoder
    data = open(os.path.join(GOLDEN, "synth_main10.bin"), "rb").read()
    host = decoder.decode_bytes(data)
    with monkeypatch.context() as m:
        m.setattr(bitstream, "plane_hash", _boom)
        dev = decoder.decode_bytes(data, hash_on="device")
    assert len(dev) == len(host) == 3
    for f, h in zip(dev, host):
        assert f.hash_ok is True and h.hash_ok is True and f.device is None
        for a, p in zip(f.planes, h.planes):
            np.testing.assert_array_equal(a, p)


def test_decoder_flipped_sei_bit_raises_for_that_picture(recon_mod):
    from p265_amd import decoder
    data = bytearray(open(os.path.join(GOLDEN, "synth_main10.bin"), "rb").read())
    dec = bitstream.decode_stream(bytes(data))
    digest = dec[1].hash[1]                                     # picture 1's Cb digest
    at = bytes(data).find(digest)
    assert at > 0 and bytes(data).find(digest, at + 1) < 0
    j = next(j for j in range(1, 15) if all(digest[j + d] > 3 for d in (-1, 0, 1)) and digest[j] ^ 0x10 > 3)
    data[at + j] ^= 0x10
    flipped = bitstream.decode_stream(bytes(data))
    assert [d.hash == e.hash for d, e in zip(dec, flipped)] == [True, False, True]
    with pytest.raises(decoder.HashMismatch, match=r"picture 1 "):
        decoder.decode_bytes(bytes(data), hash_on="device", export=recon_mod.ExportSpec.named("p010"))
    # without verification the decode completes and reports it
    frames = decoder.decode_bytes(bytes(data), hash_on="device", verify_hash=False)
    assert [f.hash_ok for f in frames] == [True, False, True]
