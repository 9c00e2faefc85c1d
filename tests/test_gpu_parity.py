"""HIP path (through the C ABI) vs the CPU oracle, bit-exact.

Runs on a real MI355X only (``-m gpu``).  Every case compares the pre-SAO
reconstruction AND the SAO output planes of libp265r.so with oracle/recon_oracle.py
on the same records: sanity.bin's three frames (front-end records pinned by the
reference's 95 golden traces), config 2, seeded synthetic pictures covering every
mode / size / QP, picture-edge CTUs, CTB 16/32/64, multiple slices and tiles,
transform skip, transquant bypass and PCM, and a full 1080p frame.
"""
import os

import numpy as np
import pytest

from oracle import recon_oracle as O
from p265_amd import frontend, synth
from p265_amd import records as R

pytestmark = pytest.mark.gpu

GOLDEN = os.path.join(os.path.dirname(__file__), "golden")


@pytest.fixture(scope="module")
def recon_mod():
    from p265_amd import recon
    if recon.device_count() < 1:
        pytest.fail("no HIP device visible: GPU tests must run on the MI355X box")
    return recon


def _check(recon_mod, params, pics, label=""):
    with recon_mod.ReconContext(params) as ctx:
        outs, recs = ctx.decode(pics, with_recon=True)
    pd = R.params_dict(params)
    for i, pic in enumerate(pics):
        rec_ref, out_ref = O.decode_picture(pd, pic.as_oracle_dict())
        for c in range(3):
            np.testing.assert_array_equal(recs[i][c], rec_ref[c], err_msg="%s pic %d recon c%d" % (label, i, c))
            np.testing.assert_array_equal(outs[i][c], out_ref[c], err_msg="%s pic %d sao c%d" % (label, i, c))
    return outs


# row pipeline variants: the two shipped builds (W = 8 and W = 12 waves per workgroup, both 80 VGPRs);
# P265R_QUAD job merging (bit 0 luma 4x4 quads, bit 1 chroma 4x4 quads, bit 2 Cb+Cr 8x8 pairs on the
# general path instead of the fast one); fair CU sharing off (P265R_FAIR=0) with job prep on the
# batch stream (P265R_FORK_PREP=0); the row queue with the luma chain not leading (P265R_LUMA_LEAD=0)
# and leading by more rows than a picture has (40); small batches run their luma and chroma chains on
# two workgroups per picture unless P265R_SPLIT=0 (the large-batch layout, which the bench runs), and
# smaller ones each chain on P265R_XG workgroups of 4 waves with progress and lines in global memory
# (default 4, "rows_auto"; 2 and 8; 0: the one-workgroup-per-chain W = 16 layout); P265R_TR_CHECK=1 poisons
# the top-right part of a CTU's row-above copy until the top-right wait, so a job the prep kernel placed
# before that wait but which reads the top-right CTU fails parity deterministically (not by timing).
ROW_VARIANTS = {"rows": {"P265R_ROW_WAVES": "8"}, "rows_auto": {},
                "rows_nosplit": {"P265R_SPLIT": "0"},
                "rows_w16": {"P265R_XG": "0"}, "rows_xg2": {"P265R_XG": "2", "P265R_TR_CHECK": "1"},
                "rows_xg8": {"P265R_XG": "8", "P265R_TR_CHECK": "1"}, "rows_xgchk": {"P265R_TR_CHECK": "1"},
                "rows_nofair": {"P265R_ROW_WAVES": "12", "P265R_FAIR": "0", "P265R_FORK_PREP": "0", "P265R_SPLIT": "0"},
                "rows_lead0": {"P265R_ROW_WAVES": "8", "P265R_LUMA_LEAD": "0", "P265R_SPLIT": "0"},
                "rows12": {"P265R_ROW_WAVES": "12"},
                "rows_lead40": {"P265R_ROW_WAVES": "12", "P265R_LUMA_LEAD": "40", "P265R_SPLIT": "0"},
                "rows_quad1": {"P265R_ROW_WAVES": "12", "P265R_QUAD": "1"},
                "rows_noquad": {"P265R_ROW_WAVES": "8", "P265R_QUAD": "4"},
                "rows_lf": {"P265R_ROW_WAVES": "8", "P265R_SAO_ROWS": "0"},
                "rows_saostrip": {"P265R_ROW_WAVES": "8", "P265R_SAO_ROWS": "2"}}


@pytest.fixture(params=["rows", "rows_auto", "rows_nosplit", "rows_w16", "rows_xg2", "rows_xg8", "rows_xgchk", "steps", "rows_nofair", "rows_lead0", "rows12", "rows_lead40", "rows_quad1",
                        "rows_noquad", "rows_lf", "rows_saostrip"])
def schedule(request, monkeypatch):
    """Both intra schedules (CU-local row pipeline, W = 8 and 12, with and without the luma / chroma
    4x4 quad jobs and the Cb+Cr 8x8 fast path; per-diagonal launches); SAO-only batches by the
    streaming SAO kernel or the loop-filter kernel."""
    if request.param == "steps":
        monkeypatch.setenv("P265R_SCHEDULE", "steps")
    else:
        monkeypatch.setenv("P265R_SCHEDULE", "rows")
        for k, v in ROW_VARIANTS[request.param].items():
            monkeypatch.setenv(k, v)
    return request.param


def test_sanity_bin_frames(recon_mod, schedule):
    params, pics = frontend.pictures_from_frontend_npz(os.path.join(GOLDEN, "sanity_frontend.npz"))
    _check(recon_mod, params, pics, "sanity")


def test_sanity_bin_yuv_pinned(recon_mod):
    """C1 pin: the HIP output of sanity.bin hashes to the committed SHA-256 of the 3-frame I420
    YUV (tests/golden/pin_sanity_yuv.py) -- conformant (deblocking + SAO), SURVEY §0.7's recon +
    SAO, and the reconstruction -- independently of the oracle computed in this run."""
    import hashlib
    import json
    pins = json.load(open(os.path.join(GOLDEN, "sanity_frontend.json")))["decoded_yuv_sha256"]
    params, pics = frontend.pictures_from_frontend_npz(os.path.join(GOLDEN, "sanity_frontend.npz"))
    _, nodbk = frontend.pictures_from_frontend_npz(os.path.join(GOLDEN, "sanity_frontend.npz"), deblocking=False)
    with recon_mod.ReconContext(params) as ctx:
        outs, recs = ctx.decode(pics, with_recon=True)
        outs_nodbk = ctx.decode(nodbk)
    def sha(frames):
        return hashlib.sha256(b"".join(np.ascontiguousarray(p).tobytes() for f in frames for p in f)).hexdigest()
    assert sha(outs) == pins["conformant"]
    assert sha(outs_nodbk) == pins["recon_sao"]
    assert sha(recs) == pins["recon"]
    with recon_mod.ReconContext(params) as ctx:
        dp = recon_mod.decode_pictures(ctx, pics[:1])[0]
    assert dp.get_reconstructed_sample(17, 9, 1) == recs[0][1][4, 8]
    assert dp.get_output_sample(351, 287, 0) == outs[0][0][287, 351]


def test_config2_single_ctu(recon_mod):
    params, pic = synth.c2_picture()
    _check(recon_mod, params, [pic], "c2")


@pytest.mark.parametrize("ctb_log2,w,h", [(6, 352, 288), (5, 200, 136), (4, 72, 40), (6, 136, 72)])
def test_synthetic_uniform_modes(recon_mod, schedule, ctb_log2, w, h):
    params = R.make_params(pic_width=w, pic_height=h, ctb_log2_size=ctb_log2)
    pics = [synth.make_picture(params, 1000 + 10 * ctb_log2 + s, perf=False) for s in range(3)]
    _check(recon_mod, params, pics, "uniform")


def test_slices_tiles_and_loop_filter_flags(recon_mod, schedule):
    params = R.make_params(pic_width=264, pic_height=200, ctb_log2_size=5, loop_filter_across_tiles=0)
    pics = [synth.make_picture(params, 77 + s, perf=False, tiles=(3, 2), n_slices=4, lf_across_slices=None)
            for s in range(3)]
    _check(recon_mod, params, pics, "tiles")
    params = R.make_params(pic_width=264, pic_height=200, ctb_log2_size=6, loop_filter_across_tiles=1)
    pics = [synth.make_picture(params, 91 + s, perf=False, tiles=(2, 2), n_slices=3, lf_across_slices=False)
            for s in range(2)]
    _check(recon_mod, params, pics, "tiles-lf")


def test_transform_skip_and_bypass(recon_mod):
    params = R.make_params(pic_width=192, pic_height=128)
    pics = [synth.make_picture(params, 5 + s, perf=False, tskip_rate=0.5, bypass_rate=0.2) for s in range(2)]
    _check(recon_mod, params, pics, "tskip/bypass")


def test_no_sao_and_no_strong_smoothing(recon_mod):
    params = R.make_params(pic_width=256, pic_height=128, sample_adaptive_offset=0, strong_intra_smoothing=0)
    pics = [synth.make_picture(params, 300 + s, perf=False) for s in range(2)]
    _check(recon_mod, params, pics, "nosao")


def test_pcm_blocks(recon_mod):
    params = R.make_params(pic_width=64, pic_height=64)
    rng = np.random.default_rng(9)
    b = frontend.PictureBuilder(params, pcm_loop_filter_disabled=True)
    samples = [rng.integers(0, 256, (32, 32)).astype(np.int16)] + [rng.integers(0, 256, (16, 16)).astype(np.int16)] * 2
    b.add_cu(0, 0, 5, 0, [0] * 4, 0, 0, 0, 0, [], pcm=True, pcm_samples=samples)
    for i, (x, y) in enumerate([(32, 0), (0, 32), (32, 32)]):
        co = [synth._coef_block(rng, 5, 0.2), synth._coef_block(rng, 4, 0.2), None]
        tu = dict(x=x, y=y, log2=5, blk=0, cbf=[1, 1, 0], tskip=[0, 0, 0], coef=co)
        b.add_cu(x, y, 5, 0, [(7 * i + 3) % 35] * 4, 1, 30, 29, 29, [tu])
    b.add_ctu(0, sao_type=(2, 1, 1), sao_abs=[[3, 1, 2, 4]] * 3, sao_sign=[[0, 1, 0, 1]] * 3,
              sao_band=(5, 10, 20), sao_eo=(1, 0, 0))
    _check(recon_mod, params, [b.finish()], "pcm")


def test_1080p_frame(recon_mod, schedule):
    params = R.make_params(pic_width=1920, pic_height=1080)
    pics = [synth.make_picture(params, 265 + 3, perf=True)]
    _check(recon_mod, params, pics, "1080p")


def test_batch_independence(recon_mod):
    """A picture decodes to the same planes alone and inside a mixed batch."""
    params = R.make_params(pic_width=320, pic_height=192)
    pics = [synth.make_picture(params, 40 + s, perf=bool(s % 2)) for s in range(6)]
    with recon_mod.ReconContext(params) as ctx:
        together = ctx.decode(pics)
        alone = [ctx.decode([p])[0] for p in pics]
    for i in range(len(pics)):
        for c in range(3):
            np.testing.assert_array_equal(together[i][c], alone[i][c])


def test_resident_batch_rerun_is_stable(recon_mod):
    """upload once, run twice: identical output (inputs are not consumed by a run)."""
    params = R.make_params(pic_width=256, pic_height=192)
    pics = [synth.make_picture(params, 60 + s) for s in range(2)]
    with recon_mod.ReconContext(params) as ctx:
        b = ctx.upload(pics)
        ctx.run(b)
        first = ctx.download(b)
        ctx.run(b)
        second = ctx.download(b)
        b.free()
    for i in range(2):
        for c in range(3):
            np.testing.assert_array_equal(first[i][c], second[i][c])


@pytest.mark.parametrize("sync_first", [True, False])
def test_pipelined_batches(recon_mod, sync_first):
    """p265r_set_pipeline: three resident batches on two streams, each run several times back to
    back with the runs interleaved across streams; every output equals the oracle, whether the
    host waits for all streams first (ctx.sync) or downloads each batch right after its last run
    (the download orders itself behind the batch's own stream)."""
    params = R.make_params(pic_width=320, pic_height=192)
    sets = [[synth.make_picture(params, 700 + 10 * k + s, perf=bool(s % 2)) for s in range(3)] for k in range(3)]
    pd = R.params_dict(params)
    with recon_mod.ReconContext(params) as ctx:
        ctx.set_pipeline(2)
        bs = [ctx.upload(p) for p in sets]
        outs = [None] * len(bs)
        for rep in range(3):
            for k, b in enumerate(bs):
                ctx.run(b)
                if rep == 2 and not sync_first:
                    outs[k] = ctx.download(b)
        if sync_first:
            ctx.sync()
            outs = [ctx.download(b) for b in bs]
        for b in bs:
            b.free()
    for k, pics in enumerate(sets):
        for i, p in enumerate(pics):
            ref = O.decode_picture(pd, p.as_oracle_dict())[1]
            for c in range(3):
                np.testing.assert_array_equal(outs[k][i][c], ref[c], err_msg="set %d pic %d c%d" % (k, i, c))


def test_pipelined_small_batches_eight_lanes(recon_mod):
    """p265r_set_pipeline(8): eight small batches (every phase on its lane stream), runs
    interleaved over the lanes twice, then downloaded in reverse order: every output equals
    the oracle."""
    params = R.make_params(pic_width=192, pic_height=128)
    sets = [[synth.make_picture(params, 900 + 10 * k + s, perf=bool((k + s) % 2)) for s in range(2)] for k in range(8)]
    pd = R.params_dict(params)
    with recon_mod.ReconContext(params) as ctx:
        ctx.set_pipeline(8)
        bs = [ctx.upload(p) for p in sets]
        for _ in range(2):
            for b in bs:
                ctx.run(b)
        outs = [ctx.download(b) for b in reversed(bs)][::-1]
        for b in bs:
            b.free()
    for k, pics in enumerate(sets):
        for i, p in enumerate(pics):
            ref = O.decode_picture(pd, p.as_oracle_dict())[1]
            for c in range(3):
                np.testing.assert_array_equal(outs[k][i][c], ref[c], err_msg="set %d pic %d c%d" % (k, i, c))


def test_pipelined_chip_filling_batches(recon_mod):
    """Batches of at least one picture per CU in a pipelined context (forked prep streams; after the
    first run the W = 8 row kernel beside the other lanes' phases; the phase-ordered variant of round
    4 is an A/B build, P265R_PHASE_ORDER): three such batches of 64x64 pictures, each run twice,
    interleaved; the first, a middle and the last picture of every batch equal the oracle."""
    params = R.make_params(pic_width=64, pic_height=64)
    distinct = [synth.make_picture(params, 950 + s, perf=bool(s % 2)) for s in range(4)]
    pd = R.params_dict(params)
    ref = [O.decode_picture(pd, p.as_oracle_dict())[1] for p in distinct]
    with recon_mod.ReconContext(params) as ctx:
        n = int(ctx.describe()["num_cus"])               # one picture per CU: the large-batch path
        sets = [[distinct[(k + i) % 4] for i in range(n)] for k in range(3)]
        ctx.set_pipeline(3)
        bs = [ctx.upload(p) for p in sets]
        for _ in range(2):
            for b in bs:
                ctx.run(b)
        ctx.sync()
        for k, b in enumerate(bs):
            ctx.status(b)
            idx = [0, n // 2, n - 1]
            outs = ctx.download(b, only=idx)
            for i in idx:
                for c in range(3):
                    np.testing.assert_array_equal(outs[i][c], ref[(k + i) % 4][c], err_msg="batch %d pic %d c%d" % (k, i, c))
            b.free()


PHASE_BUILDS = {"default": None, "phase_order": "libp265r_phaseorder.so", "early_residual": "libp265r_earlyres.so"}


@pytest.mark.parametrize("build", sorted(PHASE_BUILDS))
def test_pipelined_chip_filling_and_small_batches_mixed(recon_mod, build):
    """One pipelined context runs a chip-filling batch (forked prep stream) interleaved with a small
    batch (all phases on its lane): every run of either must wait for its OWN previous intra phase
    before overwriting its residual pool and job lists.  Every run is checked: a device digest is
    enqueued after each one (p265r_batch_digest_async, its own slot), so a run corrupted by the next
    run's residual phase is caught even though the next run rewrites the planes.  The A/B phase
    schedules -- P265R_PHASE_ORDER=1 (residual + prep wait for the last intra launch of ANY lane, which a
    small batch's runs do not order) and P265R_EARLY_RESIDUAL=1 (re-runs start their residual phase when
    the batch's previous intra phase ends) -- run the same body in a child process on their builds."""
    import json
    import subprocess
    import sys
    if PHASE_BUILDS[build] is not None:
        root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
        lib = os.path.join(root, "p265_amd", PHASE_BUILDS[build])
        assert os.path.exists(lib), "build the check variants first (make)"
        env = {k: v for k, v in os.environ.items() if not k.startswith("P265R_")}
        env.update(P265R_LIB=lib, P265R_EXPECT_BUILD=build)
        p = subprocess.run([sys.executable, "-u", "-m", "pytest", "-x", "-q", "-p", "no:cacheprovider",
                            os.path.abspath(__file__) + "::test_pipelined_chip_filling_and_small_batches_mixed[default]"],
                           env=env, cwd=root, capture_output=True, text=True, timeout=240)
        assert p.returncode == 0 and "1 passed" in p.stdout, (p.stdout + p.stderr)[-3000:]
        return
    from p265_amd import _lib, digest
    params = R.make_params(pic_width=64, pic_height=64)
    distinct = [synth.make_picture(params, 970 + s, perf=bool(s % 2)) for s in range(4)]
    pd = R.params_dict(params)
    want = [digest.picture_digest(O.decode_picture(pd, p.as_oracle_dict())[1]) for p in distinct]
    rounds = 4
    with recon_mod.ReconContext(params) as ctx:
        d = ctx.describe()
        expect = os.environ.get("P265R_EXPECT_BUILD")
        assert (d["phase_order"], d["early_residual"]) == {None: (0, 0), "phase_order": (1, 0),
                                                           "early_residual": (0, 1)}[expect], d
        n = int(d["num_cus"])
        big = [distinct[i % 4] for i in range(n)]
        small = [distinct[(i + 1) % 4] for i in range(4)]
        ctx.set_pipeline(3)
        bb, bs = ctx.upload(big), ctx.upload(small)
        assert 2 * rounds <= _lib.DIGEST_SLOTS
        for r in range(rounds):
            ctx.run(bb)
            ctx.digest_async(bb, r)
            for k in range(2):
                ctx.run(bs)
                ctx.digest_async(bs, 2 * r + k)
        for pics, b, slots in ((big, bb, rounds), (small, bs, 2 * rounds)):
            got = ctx.digest_slots(b, slots)
            for s_ in range(slots):
                for i in range(len(pics)):
                    assert np.array_equal(got[s_, i], want[distinct.index(pics[i])]), \
                        "run %d, picture %d of a %d-picture batch" % (s_, i, len(pics))
            b.free()


def test_batch_digest_equals_host_digest(recon_mod):
    """p265r_batch_digest (device) equals p265_amd/digest.py (host) on the oracle's planes, for the
    output planes and the reconstruction, on a ragged batch with deblocking (so the two differ) and
    odd picture sizes."""
    from p265_amd import digest
    big = R.make_params(pic_width=264, pic_height=200, ctb_log2_size=5)
    sizes = [(264, 200), (128, 72), (40, 200), (264, 8)]
    pics = []
    for k, (w, h) in enumerate(sizes):
        pp = R.pic_params(big, R.Picture(ctus=None, tbs=None, coef=None, size=(w, h)))
        pic = synth.make_picture(pp, 990 + k, perf=bool(k % 2), deblocking=True)
        pic.size = (w, h)
        pics.append(pic)
    with recon_mod.ReconContext(big) as ctx:
        b = ctx.upload(pics)
        ctx.run(b)
        got, got_rec = ctx.digest(b), ctx.digest(b, recon=True)
        b.free()
    for i, pic in enumerate(pics):
        rec_ref, out_ref = O.decode_picture(R.params_dict(R.pic_params(big, pic)), pic.as_oracle_dict())
        assert np.array_equal(got[i], digest.picture_digest(out_ref)), "out %d" % i
        assert np.array_equal(got_rec[i], digest.picture_digest(rec_ref)), "recon %d" % i
        assert not np.array_equal(got[i], got_rec[i])


@pytest.mark.parametrize("ctb_log2,deblocking", [(6, False), (5, False), (4, False), (6, "random"), (5, True)])
def test_ragged_batch(recon_mod, schedule, ctb_log2, deblocking):
    """Pictures of different sizes in ONE batch (p265r_picture.pic_width / pic_height, up to the
    context's size): every one equals the oracle decode at its own size -- CTB 64 / 32 (16-sample
    strip SAO), CTB 16 (4-sample strip SAO), with deblocking (loop-filter kernel), tiles, slices."""
    big = R.make_params(pic_width=264, pic_height=200, ctb_log2_size=ctb_log2, loop_filter_across_tiles=0)
    sizes = [(264, 200), (128, 72), (200, 136), (264, 64), (8 << ctb_log2 >> 3, 200), (96, 200)]
    pics = []
    for k, (w, h) in enumerate(sizes):
        pp = R.pic_params(big, R.Picture(ctus=None, tbs=None, coef=None, size=(w, h)))
        pic = synth.make_picture(pp, 500 + 7 * k + ctb_log2, perf=bool(k % 2), tiles=(2, 1) if k == 2 else (1, 1),
                                 n_slices=2 if k == 3 else 1, deblocking=deblocking, bypass_rate=0.03 if k == 5 else 0.0)
        pic.size = (w, h)
        pics.append(pic)
    with recon_mod.ReconContext(big) as ctx:
        outs, recs = ctx.decode(pics, with_recon=True)
    for i, (pic, (w, h)) in enumerate(zip(pics, sizes)):
        pp = R.pic_params(big, pic)
        assert outs[i][0].shape == (h, w)
        rec_ref, out_ref = O.decode_picture(R.params_dict(pp), pic.as_oracle_dict())
        for c in range(3):
            np.testing.assert_array_equal(recs[i][c], rec_ref[c], err_msg="pic %d %dx%d recon c%d" % (i, w, h, c))
            np.testing.assert_array_equal(outs[i][c], out_ref[c], err_msg="pic %d %dx%d out c%d" % (i, w, h, c))


def test_c5_tiles_of_a_real_stream_in_one_batch(recon_mod):
    """C5 from bytes: the 2 x 2 uneven tiles (1920 x 1088 top, 1920 x 1072 bottom) of the two 4K
    pictures of synth_4k_tiles.bin as ONE ragged batch; the stitched pictures reproduce the
    stream's MD5 picture-hash SEI."""
    import hashlib
    from p265_amd import bitstream, tiles
    pics = bitstream.decode_stream(open(os.path.join(GOLDEN, "synth_4k_tiles.bin"), "rb").read())
    parts = [tiles.split(p.params, p.picture) for p in pics]
    units = [u for ps in parts for u in ps]
    assert sorted({(int(tp["pic_width"]), int(tp["pic_height"])) for tp, _, _ in units}) == [(1920, 1072), (1920, 1088)]
    with recon_mod.ReconContext(tiles.ragged_params(units)) as ctx:
        outs = ctx.decode([tpic for _, tpic, _ in units])
    k = 0
    for p, ps in zip(pics, parts):
        full = tiles.stitch(p.params, ps, outs[k:k + len(ps)])
        k += len(ps)
        assert [hashlib.md5(np.ascontiguousarray(full[c]).tobytes()).digest() for c in range(3)] == p.hash


def test_batch_status_and_selective_download(recon_mod):
    """p265r_batch_status after re-runs of a resident batch (the bench's output check) and a
    download of a subset of its pictures (the others are not transferred)."""
    params = R.make_params(pic_width=320, pic_height=192)
    pics = [synth.make_picture(params, 810 + s, perf=True) for s in range(4)]
    pd = R.params_dict(params)
    with recon_mod.ReconContext(params) as ctx:
        ctx.set_pipeline(2)
        bs = [ctx.upload(pics), ctx.upload(pics)]
        for _ in range(3):
            for b in bs:
                ctx.run(b)
        for b in bs:
            ctx.status(b)
            outs = ctx.download(b, only=[0, 3])
            assert outs[1] is None and outs[2] is None
            for i in (0, 3):
                ref = O.decode_picture(pd, pics[i].as_oracle_dict())[1]
                for c in range(3):
                    np.testing.assert_array_equal(outs[i][c], ref[c])
            b.free()


def test_invalid_records_rejected(recon_mod):
    params = R.make_params(pic_width=64, pic_height=64)
    pic = synth.make_picture(params, 3)
    bad = R.Picture(ctus=pic.ctus.copy(), tbs=pic.tbs.copy(), coef=pic.coef)
    bad.tbs["x"][0] = 200
    with recon_mod.ReconContext(params) as ctx:
        with pytest.raises(Exception):
            ctx.decode([bad])


@pytest.mark.parametrize("bd", [8, 10, 12])
def test_out_of_range_qp_rejected(recon_mod, bd):
    """p265r_tb.qp is qP incl. QpBdOffset, 0 .. 51 + 6 * (BitDepth - 8): the largest legal value uploads and
    decodes (every TB of a valid picture set to it, PCM ones too); one more, or 255, on one luma, chroma, PCM or
    uncoded record is EINVAL at upload -- on the dense and on the sparse path, before any kernel is launched (a qp of
    64 and above would set edge bits of the one-byte deblocking map entry, and shift Dequant's scale out of
    range)."""
    from oracle import c_oracle
    from p265_amd import _lib
    params = R.make_params(pic_width=64, pic_height=64, bit_depth_luma=bd, bit_depth_chroma=bd)
    pic = synth.make_picture(params, 3, deblocking=True, pcm_rate=0.2)
    top = 51 + 6 * (bd - 8)
    flags = pic.tbs["flags"]
    luma = int(np.nonzero((pic.tbs["c_idx"] == 0) & (flags & R.TB_CBF != 0) & (flags & R.TB_PCM == 0))[0][0])
    chroma = int(np.nonzero((pic.tbs["c_idx"] > 0) & (flags & R.TB_CBF != 0) & (flags & R.TB_PCM == 0))[0][0])
    pcm = int(np.nonzero((pic.tbs["c_idx"] == 0) & (flags & R.TB_PCM != 0))[0][0])
    uncoded = int(np.nonzero((pic.tbs["c_idx"] == 0) & (flags & (R.TB_CBF | R.TB_PCM) == 0))[0][0])
    ok = R.Picture(ctus=pic.ctus, tbs=pic.tbs.copy(), coef=pic.coef, nofilter=pic.nofilter)
    ok.tbs["qp"] = top
    R.validate(params, ok)
    ref = c_oracle.decode(params, [ok])[0]
    with recon_mod.ReconContext(params) as ctx:
        for sparse in (False, True):
            outs = ctx.decode([ok], sparse=sparse)
            for c in range(3):
                np.testing.assert_array_equal(outs[0][c], ref[1][c], err_msg="qp %d c%d sparse=%r" % (top, c, sparse))
        runs = ctx.describe()
        for k in (luma, chroma, pcm, uncoded):
            for qp in (top + 1, 255):
                bad = R.Picture(ctus=pic.ctus, tbs=pic.tbs.copy(), coef=pic.coef, nofilter=pic.nofilter)
                bad.tbs["qp"][k] = qp
                with pytest.raises(R.RecordError):
                    R.validate(params, bad)
                for sparse in (False, True):
                    with pytest.raises(_lib.P265RError) as ei:
                        ctx.upload([bad], sparse=sparse)
                    assert ei.value.code == _lib.EINVAL, (k, qp, sparse)
        assert ctx.describe() == runs              # refused at upload: nothing was launched


def test_invalid_chroma_size_and_tb_count_rejected(recon_mod):
    """A 32x32 chroma TB (impossible in 4:2:0) and a CTU listing more TBs (or chroma TBs)
    than it has 4x4 units are EINVAL at upload, before anything reaches the GPU."""
    from p265_amd import _lib
    params = R.make_params(pic_width=64, pic_height=64)
    pic = synth.make_picture(params, 3)
    bad = R.Picture(ctus=pic.ctus.copy(), tbs=pic.tbs.copy(), coef=pic.coef)
    k = int(np.nonzero(bad.tbs["c_idx"] > 0)[0][0])
    bad.tbs["log2_size"][k] = 5
    bad.tbs["x"][k] = bad.tbs["y"][k] = 0
    bad.tbs["flags"][k] = 0
    reps = (3 * 16 * 16 // 2 + 1) // len(pic.tbs) + 1
    bad2 = R.Picture(ctus=pic.ctus.copy(), tbs=np.concatenate([pic.tbs] * reps), coef=pic.coef)
    bad2.ctus["tb_count"][0] = 3 * 16 * 16 // 2 + 1
    from test_records import chroma_overfull
    for b in (bad, bad2, chroma_overfull(pic)):
        with pytest.raises(R.RecordError):
            R.validate(params, b)
        with recon_mod.ReconContext(params) as ctx:
            with pytest.raises(_lib.P265RError) as ei:
                ctx.decode([b])
            assert ei.value.code == _lib.EINVAL


def test_unreferenced_tb_records_are_checked(recon_mod):
    """Every TB of the array is packed, also one no CTU lists: its coefficient range and size are checked at
    upload (ERANGE / EINVAL) instead of being read past the caller's coefficient array."""
    from p265_amd import _lib
    params = R.make_params(pic_width=64, pic_height=64)
    pic = synth.make_picture(params, 3)
    extra = np.zeros(1, R.TB_DTYPE)
    extra["flags"] = R.TB_CBF
    extra["log2_size"] = 5
    for field, value, code in (("coef_off", len(pic.coef), _lib.ERANGE), ("log2_size", 7, _lib.EINVAL)):
        e = extra.copy()
        e[field] = value
        bad = R.Picture(ctus=pic.ctus, tbs=np.concatenate([pic.tbs, e]), coef=pic.coef)
        with recon_mod.ReconContext(params) as ctx:
            with pytest.raises(_lib.P265RError) as ei:
                ctx.upload([bad])
            assert ei.value.code == code


def test_chroma_sao_type_mismatch_rejected(recon_mod):
    """Cb and Cr share SaoTypeIdx and SaoEoClass (7.4.9.3.2): records that differ are EINVAL."""
    from p265_amd import _lib
    params = R.make_params(pic_width=64, pic_height=64)
    pic = synth.make_picture(params, 3)
    for typ, cls in (((0, 2, 1), (0, 0, 0)), ((0, 2, 2), (0, 1, 3))):
        bad = R.Picture(ctus=pic.ctus.copy(), tbs=pic.tbs, coef=pic.coef)
        bad.ctus["sao_type"][0] = typ
        bad.ctus["sao_class"][0] = cls
        with recon_mod.ReconContext(params) as ctx:
            with pytest.raises(_lib.P265RError) as ei:
                ctx.decode([bad])
            assert ei.value.code == _lib.EINVAL


def test_oversized_batch_returns_erange(recon_mod):
    """A batch whose coded coefficients exceed the signed 32-bit residual offsets the row
    kernel uses (2^31 int16) is refused with ERANGE at upload (no device allocation):
    22 pictures of 8192x8192, every TB coded, all sharing one 1024-sample coefficient block."""
    from p265_amd import _lib
    params = R.make_params(pic_width=8192, pic_height=8192)
    wc = hc = 8192 // 64
    per_ctu = []
    for c_idx, lg, step in ((0, 5, 32), (1, 4, 16), (2, 4, 16)):
        for y in range(0, 64 >> (c_idx > 0), step):
            for x in range(0, 64 >> (c_idx > 0), step):
                per_ctu.append((x, y, lg, c_idx))
    n = len(per_ctu)
    tbs = np.zeros(wc * hc * n, R.TB_DTYPE)
    ctus = np.zeros(wc * hc, R.CTU_DTYPE)
    base = np.array(per_ctu, np.int64)
    for rs in range(wc * hc):
        cx, cy = (rs % wc) * 64, (rs // wc) * 64
        sl = slice(rs * n, (rs + 1) * n)
        sub = (base[:, 3] > 0).astype(np.int64)
        tbs["x"][sl] = (cx >> sub) + base[:, 0]
        tbs["y"][sl] = (cy >> sub) + base[:, 1]
        tbs["log2_size"][sl] = base[:, 2]
        tbs["c_idx"][sl] = base[:, 3]
        ctus["tb_begin"][rs] = rs * n
        ctus["tb_count"][rs] = n
    tbs["flags"] = R.TB_CBF
    tbs["qp"] = 30
    pic = R.Picture(ctus=ctus, tbs=tbs, coef=np.zeros(1024, np.int16))
    assert pic.n_coded_coef * 22 > 2 ** 31
    with recon_mod.ReconContext(params) as ctx:
        with pytest.raises(_lib.P265RError) as ei:
            ctx.upload([pic] * 22)
        assert ei.value.code == _lib.ERANGE


def test_many_small_pictures_per_workgroup(recon_mod, schedule):
    """More pictures than resident workgroups: the row queue of one workgroup crosses
    picture boundaries (several pictures in flight per workgroup, line-buffer slots reused)."""
    params = R.make_params(pic_width=64, pic_height=128, ctb_log2_size=5)
    uniq = [synth.make_picture(params, 500 + s, perf=False) for s in range(5)]
    pics = [uniq[i % 5] for i in range(1200)]
    with recon_mod.ReconContext(params) as ctx:
        outs = ctx.decode(pics)
    pd = R.params_dict(params)
    refs = [O.decode_picture(pd, u.as_oracle_dict())[1] for u in uniq]
    for i in range(len(pics)):
        for c in range(3):
            np.testing.assert_array_equal(outs[i][c], refs[i % 5][c], err_msg="pic %d c%d" % (i, c))


def _component_major(pic):
    """Same picture with each CTU's TBs reordered to [all Y, all Cb, all Cr]: the decode
    order inside every component is unchanged, so the output must be identical; the Cb
    and Cr TBs of a TU are no longer adjacent (unpaired chroma jobs)."""
    tbs = pic.tbs.copy()
    for ctu in pic.ctus:
        b, n = int(ctu["tb_begin"]), int(ctu["tb_count"])
        seg = pic.tbs[b:b + n]
        order = np.argsort(seg["c_idx"], kind="stable")
        tbs[b:b + n] = seg[order]
    return R.Picture(ctus=pic.ctus, tbs=tbs, coef=pic.coef, nofilter=pic.nofilter, meta=dict(pic.meta))


@pytest.fixture(params=["auto", "xgchk", "xg8chk", "w16"])
def xg_variant(request, monkeypatch):
    """The latency layouts small batches run: cross-group chains (default xg 4), their checking instance
    (P265R_TR_CHECK=1: top-right part of the row-above copy poisoned until its wait, the left half of every
    bottom line served by the half-CTU publish alone, prep's `br` checked against the TB extents), xg 8
    checked, and the one-workgroup-per-chain W = 16 split."""
    env = {"auto": {}, "xgchk": {"P265R_TR_CHECK": "1"}, "xg8chk": {"P265R_XG": "8", "P265R_TR_CHECK": "1"},
           "w16": {"P265R_XG": "0"}}[request.param]
    for k, v in env.items():
        monkeypatch.setenv(k, v)
    return request.param


def test_component_major_tb_order(recon_mod, xg_variant):
    params = R.make_params(pic_width=200, pic_height=136, ctb_log2_size=5)
    pics = [_component_major(synth.make_picture(params, 4040 + s, perf=False)) for s in range(2)]
    _check(recon_mod, params, pics, "component-major")
    params, sp = frontend.pictures_from_frontend_npz(os.path.join(GOLDEN, "sanity_frontend.npz"))
    _check(recon_mod, params, [_component_major(sp[0])], "sanity-component-major")


# ---------------------------------------------------------------------------------
# in-loop filters: deblocking (8.7.2) + SAO fused in loopfilter_kernel
# ---------------------------------------------------------------------------------

def _check_c(recon_mod, params, pics, label=""):
    """Like _check, against the C oracle twin (equal to the Python one: tests/test_deblock.py)."""
    from oracle import c_oracle
    with recon_mod.ReconContext(params) as ctx:
        outs, recs = ctx.decode(pics, with_recon=True)
    ref = c_oracle.decode(params, pics, threads=8)
    for i in range(len(pics)):
        for c in range(3):
            np.testing.assert_array_equal(recs[i][c], ref[i][0][c], err_msg="%s pic %d recon c%d" % (label, i, c))
            np.testing.assert_array_equal(outs[i][c], ref[i][1][c], err_msg="%s pic %d out c%d" % (label, i, c))


@pytest.mark.parametrize("ctb_log2,w,h,tiles,slices,lf_tiles,sao", [
    (6, 352, 288, (1, 1), 1, 1, True), (5, 264, 200, (3, 2), 4, 0, True), (5, 264, 200, (3, 2), 4, 1, False),
    (4, 72, 40, (1, 1), 3, 1, True), (6, 136, 72, (2, 1), 2, 1, True), (4, 200, 136, (2, 2), 5, 0, False)])
def test_deblocking_synthetic(recon_mod, ctb_log2, w, h, tiles, slices, lf_tiles, sao):
    params = R.make_params(pic_width=w, pic_height=h, ctb_log2_size=ctb_log2, loop_filter_across_tiles=lf_tiles,
                           sample_adaptive_offset=int(sao), pps_cb_qp_offset=(w % 7) - 3, pps_cr_qp_offset=3 - (h % 7))
    pics = [synth.make_picture(params, 1300 + 7 * s + ctb_log2, perf=False, tiles=tiles, n_slices=slices,
                               lf_across_slices=None, deblocking="random", bypass_rate=0.04, pcm_rate=0.03, sao=sao)
            for s in range(3)]
    _check(recon_mod, params, pics, "dbk")


def test_deblocking_1080p(recon_mod):
    params = R.make_params(pic_width=1920, pic_height=1080)
    pics = [synth.make_picture(params, 265 + 4 + s, perf=True, deblocking=True) for s in range(2)]
    _check_c(recon_mod, params, pics, "dbk-1080p")


def test_deblocking_4k_tiles(recon_mod):
    params = R.make_params(pic_width=3840, pic_height=2160, loop_filter_across_tiles=1)
    pics = [synth.make_picture(params, 4000, perf=True, tiles=(2, 2), deblocking="random")]
    _check_c(recon_mod, params, pics, "dbk-4k")


@pytest.mark.parametrize("kernel", ["1", "2"])
def test_sao_only_window_kernel(recon_mod, kernel, monkeypatch):
    """SAO-only batches (no deblocking): slices, tiles, bypass, PCM, ragged right / bottom edges
    (widths not a multiple of 16), CTB 16/32/64, through the per-CTB kernel (P265R_SAO_ROWS=1) and
    the strip kernel (2)."""
    monkeypatch.setenv("P265R_SAO_ROWS", kernel)
    for ctb_log2, w, h in ((6, 200, 136), (5, 264, 200), (4, 72, 40), (6, 136, 72), (5, 328, 104), (6, 1000, 232)):
        params = R.make_params(pic_width=w, pic_height=h, ctb_log2_size=ctb_log2, loop_filter_across_tiles=0)
        pics = [synth.make_picture(params, 1700 + s, perf=False, tiles=(2, 1), n_slices=3, lf_across_slices=None,
                                   bypass_rate=0.05, pcm_rate=0.03 * s) for s in range(2)]
        _check_c(recon_mod, params, pics, "sao-only")


@pytest.mark.parametrize("bd,w,h,ctb_log2", [(8, 2000, 72, 6), (8, 2000, 72, 5), (10, 1000, 72, 5), (10, 1000, 136, 6)])
def test_sao_strip_second_strips(recon_mod, bd, w, h, ctb_log2):
    """SAO-only batches whose planes reach into a second strip of the streaming strip kernels: at 8 bits
    chroma width 1000 (sao_strip16.h, 992-sample strips: one 8-sample column past the strip, a partial
    16-sample lane), at 10 bits luma width 1000 and chroma width 500 (sao16.h, 496-sample strips: 4 samples
    past the strip, a partial 8-sample lane).  Tiles without filtering across them and slices put different
    3x3 permissions on either side of the strip boundary.  SAO must change samples of every component in
    the second strip, or the comparison there would say nothing."""
    params = R.make_params(pic_width=w, pic_height=h, ctb_log2_size=ctb_log2, loop_filter_across_tiles=0,
                           bit_depth_luma=bd, bit_depth_chroma=bd)
    pic = synth.make_picture(params, 7000 + bd + ctb_log2, perf=False, tiles=(3, 2), n_slices=4, lf_across_slices=None,
                             deblocking=False, pcm_rate=0.03, bypass_rate=0.03)
    with recon_mod.ReconContext(params) as ctx:
        outs, recs = ctx.decode([pic], with_recon=True)
    rec_ref, out_ref = O.decode_picture(R.params_dict(params), pic.as_oracle_dict())
    strip = 992 if bd == 8 else 496
    for c in range(3):
        changed = int(np.count_nonzero(np.asarray(rec_ref[c])[:, strip:] != np.asarray(out_ref[c])[:, strip:]))
        assert changed > 0, "oracle: SAO changes no sample at x >= %d of component %d" % (strip, c)
        np.testing.assert_array_equal(recs[0][c], rec_ref[c], err_msg="strip2 recon c%d" % c)
        np.testing.assert_array_equal(outs[0][c], out_ref[c], err_msg="strip2 sao c%d" % c)


# ---------------------------------------------------------------------------------
# C5 with loop_filter_across_tiles_enabled_flag = 1: tile reconstruction + halo + filtering
# ---------------------------------------------------------------------------------

def _tile_halo_decode(recon_mod, params, pic):
    """Every tile on its own through the library (reconstruction pass, then the in-loop
    filters on its extended tile with the neighbours' halos): stitched tile outputs."""
    from p265_amd import halo, tiles
    grid = halo.TileGrid.from_picture(params, pic)
    datas = []
    for t, (tp, tpic, _) in enumerate(tiles.split(params, pic, recon_only=True)):
        with recon_mod.ReconContext(tp) as ctx:
            out = ctx.decode([tpic])[0]                  # no in-loop filters in this pass: out = recon
        d = halo.TileData(grid, pic, t)
        d.recon = out
        datas.append(d)
    outs = {}
    for t in range(grid.n_tiles):
        ep, epic, origin, inner = halo.ext_picture(params, grid, datas[t], [datas[n].halo_for(t) for n in grid.neighbours(t)])
        with recon_mod.ReconContext(ep) as ctx:
            outs[t] = halo.crop_inner(ctx.decode([epic])[0], origin, inner)
    return grid, outs


@pytest.mark.parametrize("w,h,ctb_log2,tiles_xy,perf", [(264, 200, 5, (2, 2), False), (200, 136, 4, (3, 2), False),
                                                        (3840, 2160, 6, (2, 2), True)])
def test_tile_halo_equals_whole_picture(recon_mod, w, h, ctb_log2, tiles_xy, perf):
    from oracle import c_oracle
    params = R.make_params(pic_width=w, pic_height=h, ctb_log2_size=ctb_log2, loop_filter_across_tiles=1,
                           pps_cb_qp_offset=1, pps_cr_qp_offset=-2)
    pic = synth.make_picture(params, 2024 + w, perf=perf, tiles=tiles_xy, n_slices=1 if perf else 3,
                             lf_across_slices=None, deblocking="random", bypass_rate=0.03)
    grid, outs = _tile_halo_decode(recon_mod, params, pic)
    ref = c_oracle.decode(params, [pic], threads=8)[0][1]
    for t, planes in outs.items():
        x0, x1, y0, y1 = grid.luma_rect(grid.rect(t))
        for c in range(3):
            s = 0 if c == 0 else 1
            np.testing.assert_array_equal(planes[c], ref[c][y0 >> s:y1 >> s, x0 >> s:x1 >> s], err_msg="tile %d c%d" % (t, c))


def test_download_into_frame_pool(recon_mod):
    """ctx.download(into=frames) refills a caller's frame pool (bench.py's PCIe leg): same planes as a
    fresh download, the pool's arrays themselves are written, and a mismatched pool is refused."""
    params = R.make_params(pic_width=200, pic_height=136, ctb_log2_size=5)
    a = [synth.make_picture(params, 7100 + s, perf=bool(s)) for s in range(2)]
    b = [synth.make_picture(params, 7200 + s, perf=bool(s)) for s in range(2)]
    with recon_mod.ReconContext(params) as ctx:
        ba, bb = ctx.upload(a), ctx.upload(b)
        ctx.run(ba)
        ctx.run(bb)
        pool = ctx.download(ba)
        want_b = ctx.download(bb)
        got = ctx.download(bb, into=pool)
        assert all(got[i][k] is pool[i][k] for i in range(2) for k in range(3))
        for i in range(2):
            for k in range(3):
                np.testing.assert_array_equal(pool[i][k], want_b[i][k])
        bad = [[p.copy() for p in f] for f in pool]
        bad[1][2] = bad[1][2][:, :-1].copy()
        with pytest.raises(ValueError):
            ctx.download(ba, into=bad)
        with pytest.raises(ValueError):
            ctx.download(ba, into=pool[:1])
        ba.free(); bb.free()
