"""Monochrome (4:0:0, chroma_format_idc 0) on the GPU through the C ABI, bit-exact against the oracles' luma.

A monochrome picture is the luma of a 4:2:0 one (tests/mono.py to_mono: the chroma TB records dropped, the CTU
ranges renumbered, chroma SAO cleared; tests/test_mono_records.py shows with both oracles that luma does not depend on
them), so the expected reconstruction and decoded plane are plane 0 of what the C oracle computes for the 4:2:0
picture.  Every test asserts the row layout p265r_describe reports: ``luma`` (the third layout of intra_rows_kernel:
luma rows only, one workgroup per picture slot) with the W of the build, or ``steps`` (the per-diagonal kernel).
"""
import dataclasses

import numpy as np
import pytest

import mono as M
import planted as P
import planted_lf as L
import planted_sao as S
import planted_struct as PS
import streamgen
from oracle import c_oracle
from p265_amd import _lib, digest, synth
from p265_amd import records as R
from test_gpu_parity import ROW_VARIANTS

pytestmark = pytest.mark.gpu

# schedule -> (environment, expected layout, expected W at 8 bits, at 9..12 bits; None: no row kernel)
SCHEDULES = {
    "steps": ({"P265R_SCHEDULE": "steps"}, "steps", 0, 0),
    "rows": (dict(ROW_VARIANTS["rows"], P265R_SCHEDULE="rows"), "luma", 8, 8),            # W = 8
    "rows12": (dict(ROW_VARIANTS["rows12"], P265R_SCHEDULE="rows"), "luma", 12, 12),
    "nosplit": (dict(ROW_VARIANTS["rows_nosplit"], P265R_SCHEDULE="rows"), "luma", 12, 12),  # P265R_SPLIT=0, by run
    "by_run": ({"P265R_SCHEDULE": "rows"}, "luma", 16, 12),      # a small batch: W = 16 at 8 bits
}
TILES_KW = dict(perf=False, tiles=(2, 2), n_slices=3, lf_across_slices=None, deblocking="random", bypass_rate=0.05,
                pcm_rate=0.03, tskip_rate=0.3)
CASES = {"uniform": (dict(perf=False, deblocking=True), {}), "tiles": (TILES_KW, {}),
         "sao_only": (dict(perf=True, deblocking=False, tskip_rate=0.2, pcm_rate=0.02), {}),
         "no_filter": (dict(perf=False, deblocking=False), dict(sample_adaptive_offset=0))}


@pytest.fixture(scope="module")
def recon_mod():
    from p265_amd import recon
    if recon.device_count() < 1:
        pytest.fail("no HIP device visible: GPU tests must run on the MI355X box")
    return recon


def _set_env(monkeypatch, schedule):
    for k in ("P265R_SCHEDULE", "P265R_ROW_WAVES", "P265R_SPLIT", "P265R_SAO_ROWS"):
        monkeypatch.delenv(k, raising=False)
    for k, v in SCHEDULES[schedule][0].items():
        monkeypatch.setenv(k, v)


def _luma_ref(params, pics, scaling=None):
    """[(reconstruction Y, decoded Y)] of 4:2:0 pictures by the C oracle (every picture at its own size)."""
    return [(rec[0], out[0]) for rec, out in c_oracle.decode(params, pics, threads=8, scaling=scaling)]


def _assert_layout(d, schedule, bd, label):
    env, layout, w8, w16 = SCHEDULES[schedule]
    assert d["chroma_format_idc"] == 0, label
    assert d["last_launch_layout"] == layout, (label, d["last_launch_layout"])
    assert d["last_launch_row_waves"] == (w8 if bd == 8 else w16), (label, d["last_launch_row_waves"])
    assert not d["last_launch_split"] and not d["last_launch_xg"], label


def _compare(outs, recs, want, label, metas=None):
    assert len(outs) == len(want)
    for i, (rec_y, out_y) in enumerate(want):
        tag = "%s pic %d %r" % (label, i, metas[i] if metas else "")
        assert len(outs[i]) == 1 and (recs is None or len(recs[i]) == 1), tag
        if recs is not None:
            np.testing.assert_array_equal(recs[i][0], rec_y, err_msg=tag + " recon")
        np.testing.assert_array_equal(outs[i][0], out_y, err_msg=tag + " out")
        assert outs[i][0].dtype == np.asarray(out_y).dtype


def _decode(recon_mod, params, mono_pics, want, label, sparse=False):
    """One batch of monochrome pictures in a context of ``params``'s monochrome twin -> describe()."""
    with recon_mod.ReconContext(M.mono_params(params)) as ctx:
        outs, recs = ctx.decode(mono_pics, with_recon=True, sparse=sparse)
        d = ctx.describe()
    _compare(outs, recs, want, label, [p.meta for p in mono_pics])
    return d


# ---- seeded parity -----------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("case", sorted(CASES))
@pytest.mark.parametrize("bd", [8, 10, 12])
@pytest.mark.parametrize("lg", [4, 5, 6])
@pytest.mark.parametrize("w,h", [(136, 72), (200, 136)])
def test_seeded_parity(recon_mod, monkeypatch, w, h, lg, bd, case):
    """136 x 72 and 200 x 136 (no multiple of any CTB size), CTB 16 / 32 / 64, BitDepth 8 / 10 / 12; deblocking on,
    tiles + slices + PCM + bypass + transform skip, SAO only, no in-loop filter.  A batch of 1 (the small-batch
    layout) and of 3 pictures under the per-diagonal kernel, W = 8, W = 12, P265R_SPLIT=0 and the build chosen by
    run; the filters change luma where they are on."""
    kw, pkw = CASES[case]
    params = R.make_params(pic_width=w, pic_height=h, ctb_log2_size=lg, bit_depth_luma=bd, bit_depth_chroma=bd,
                           loop_filter_across_tiles=0, pps_cb_qp_offset=-1, pps_cr_qp_offset=2, **pkw)
    full = [synth.make_picture(params, 6100 + 7 * lg + bd + s, **kw) for s in range(3)]
    want = _luma_ref(params, full)
    pics = [M.to_mono(p) for p in full]
    if case != "no_filter":
        assert sum(int((np.asarray(o) != np.asarray(r)).sum()) for r, o in want) > 200
    for schedule in SCHEDULES:
        _set_env(monkeypatch, schedule)
        for n in (1, 3):
            label = "%dx%d ctb%d bd%d %s %s n=%d" % (w, h, 1 << lg, bd, case, schedule, n)
            d = _decode(recon_mod, params, pics[:n], want[:n], label)
            _assert_layout(d, schedule, bd, label)


@pytest.mark.parametrize("schedule", ["rows", "rows12", "by_run"])
@pytest.mark.parametrize("bd,lg", [(8, 4), (8, 5), (10, 4)])
def test_many_pictures_per_workgroup(recon_mod, monkeypatch, bd, lg, schedule):
    """2 num_cus + 3 pictures of 64 x 64: more pictures than workgroups fit at once, so a workgroup decodes several
    pictures in turn and reuses its picture slots (W = 8 rows span three 4-row pictures at CTB 16)."""
    params = R.make_params(pic_width=64, pic_height=64, ctb_log2_size=lg, bit_depth_luma=bd, bit_depth_chroma=bd)
    distinct = [synth.make_picture(params, 6400 + s, perf=bool(s % 2), deblocking=bool(s % 3 == 0), tskip_rate=0.1)
                for s in range(12)]
    ref = _luma_ref(params, distinct)
    mono = [M.to_mono(p) for p in distinct]
    _set_env(monkeypatch, schedule)
    with recon_mod.ReconContext(M.mono_params(params)) as ctx:
        n = 2 * int(ctx.describe()["num_cus"]) + 3
        order = [(5 * i + i // 12) % 12 for i in range(n)]
        outs, recs = ctx.decode([mono[k] for k in order], with_recon=True)
        d = ctx.describe()
    assert d["last_launch_layout"] == "luma" and d["last_launch_row_waves"] == (12 if schedule == "by_run" else SCHEDULES[schedule][2])
    _compare(outs, recs, [ref[k] for k in order], "many bd%d ctb%d %s" % (bd, 1 << lg, schedule))


# ---- planted sets through to_mono --------------------------------------------------------------------------------------

@pytest.mark.parametrize("schedule", ["by_run", "rows", "steps"])
@pytest.mark.parametrize("bd", [8, 10, 12])
def test_planted_set(recon_mod, monkeypatch, bd, schedule):
    """tests/planted.py: every luma mode x size x placement x neighbour style (and the chain pictures), the full-size
    pictures as one batch, the narrower ones as a ragged one."""
    pics = [pic for _, pic in P.planted_set(bd)] + [pic for _, pic, _ in P.chain_set(bd)]
    params = P.set_params(bd)
    key = ("planted", bd)
    if key not in _REFS:
        _REFS[key] = _luma_ref(params, pics)
    want = _REFS[key]
    full = [i for i, p in enumerate(pics) if tuple(p.size) == (P.MAX_W, P.MAX_H)]
    rest = [i for i, p in enumerate(pics) if tuple(p.size) != (P.MAX_W, P.MAX_H)]
    _set_env(monkeypatch, schedule)
    for idx in (full, rest):
        d = _decode(recon_mod, params, [M.to_mono(pics[i]) for i in idx], [want[i] for i in idx],
                    "planted bd%d %s" % (bd, schedule))
        assert d["last_launch_layout"] == SCHEDULES[schedule][1]
        if schedule == "by_run" and idx is full:
            assert d["last_launch_row_waves"] == 12          # far more pictures than CUs: W = 12 alone


_REFS = {}


@pytest.mark.parametrize("schedule", ["by_run", "rows"])
@pytest.mark.parametrize("lg", [4, 5, 6])
def test_planted_struct_set(recon_mod, monkeypatch, lg, schedule):
    """tests/planted_struct.py (every TB tiling, job-list edge and CTU wait; its ``counts`` and ``quads`` families
    among them) without the chroma records: the luma list's 64-entry window and chunk edges now fall on other TBs.
    From the records: the thinned set still reaches luma lists of 61 / 64 / 67 / 127 / 130 / 256 TBs at CTB 64 and
    61 / 64 at CTB 32 (a CTB 32 has at most 64 luma TBs, a CTB 16 at most 16: those lose nothing to the thinning,
    they never had the longer lists)."""
    pics = PS.struct_set(8, lg)
    mono = [M.to_mono(p) for p in pics]
    lengths = set(int(v) for m in mono for v in M.luma_list_lengths(m))
    reach = {6: (61, 64, 67, 127, 130, 256), 5: (61, 64), 4: (16,)}[lg]
    assert all(v in lengths for v in reach), (lg, sorted(lengths))
    fams = set(p.meta["family"] for p in pics)
    assert "quads" in fams and (lg == 4 or "counts" in fams)
    _set_env(monkeypatch, schedule)
    for edges in (False, True):
        idx = [i for i, p in enumerate(pics) if PS.is_ragged(p) == edges]
        params = PS.set_params(8, lg, edges=edges)
        key = ("struct", lg, edges)
        if key not in _REFS:
            _REFS[key] = _luma_ref(params, [pics[i] for i in idx])
        d = _decode(recon_mod, params, [mono[i] for i in idx], _REFS[key], "struct ctb%d %s edges=%r" % (1 << lg, schedule, edges))
        assert d["last_launch_layout"] == "luma"


@pytest.mark.parametrize("sao", [False, True])
@pytest.mark.parametrize("bd", [8, 10, 12])
@pytest.mark.parametrize("lg", [4, 5, 6])
def test_planted_lf_set(recon_mod, monkeypatch, lg, bd, sao):
    """tests/planted_lf.py (every deblocking decision, offset and rule) at each CTB size and depth, SAO off and on:
    loopfilter_kernel<L, true> / loopfilter16_kernel<L, true> with no chroma window to load, edge to filter or unit
    to write.  The variant (chroma QP offsets, loop_filter_across_tiles) rotates over the matrix."""
    variant = "abc"[(lg + bd // 2 + int(sao)) % 3]
    pics = L.lf_set(bd, lg, variant, sao)
    params = L.params_of(bd, lg, variant, sao)
    want = _luma_ref(params, pics)
    assert sum(int((np.asarray(o) != np.asarray(r)).sum()) for r, o in want) > 1000
    _set_env(monkeypatch, "by_run")
    d = _decode(recon_mod, params, [M.to_mono(dataclasses.replace(p, size=None)) for p in pics], want,
                "lf bd%d ctb%d %s sao=%r" % (bd, 1 << lg, variant, sao))
    assert d["last_launch_layout"] == "luma"


SAO_RUNS = [  # (bd, lg, dbk, P265R_SAO_ROWS, kernel)
    (8, 4, False, None, "sao_rows_kernel"), (8, 5, False, "2", "sao_rows_kernel"),
    (8, 5, False, None, "sao_strip16_kernel<5>"), (8, 6, False, None, "sao_strip16_kernel<6>"),
    (10, 5, False, None, "sao16_strip_kernel"), (12, 6, False, None, "sao16_strip_kernel"),
    (8, 4, False, "0", "loopfilter_kernel<4, false>"), (8, 6, False, "0", "loopfilter_kernel<6, false>"),
    (8, 5, True, None, "loopfilter_kernel<5, true>"), (10, 4, True, None, "loopfilter16_kernel<4, true>")]


@pytest.mark.parametrize("bd,lg,dbk,sao_rows,kernel", SAO_RUNS)
def test_planted_sao_set(recon_mod, monkeypatch, bd, lg, dbk, sao_rows, kernel):
    """tests/planted_sao.py (every class, band, clip and CTB-border rule; its ``strips`` pictures cross the strip
    edges of every strip kernel) on each kernel that filters SAO.  Without the chroma strips a picture's strip units
    are numbered anew (sao.h strip_pos)."""
    pics = S.sao_set(bd, lg, 1, dbk)
    key = ("sao", bd, lg, dbk)
    if key not in _REFS:
        _REFS[key] = [(rec[0], out[0]) for rec, out in S.c_decode(bd, lg, 1, pics)]
    want = _REFS[key]
    assert sum(int((np.asarray(o) != np.asarray(r)).sum()) for r, o in want) > 1000
    _set_env(monkeypatch, "by_run")
    if sao_rows is not None:
        monkeypatch.setenv("P265R_SAO_ROWS", sao_rows)
    for (w, h), idx in S.by_size(pics).items():
        d = _decode(recon_mod, S.params_of(bd, lg, 1, w, h), [M.to_mono(dataclasses.replace(pics[i], size=None)) for i in idx],
                    [want[i] for i in idx], "sao bd%d ctb%d %s %dx%d" % (bd, 1 << lg, kernel, w, h))
        assert d["sao_rows"] == (1 if sao_rows is None else int(sao_rows))


# ---- batch variants ----------------------------------------------------------------------------------------------------

def _ragged(bd, lg, deblocking):
    ctb = 1 << lg
    big = R.make_params(pic_width=3 * ctb, pic_height=3 * ctb, ctb_log2_size=lg, bit_depth_luma=bd, bit_depth_chroma=bd)
    sizes = [(3 * ctb, 3 * ctb), (2 * ctb + 8, ctb + 8), (8, 3 * ctb), (3 * ctb, 8), (ctb, ctb), (2 * ctb - 8, 3 * ctb - 8)]
    pics = []
    for k, (w, h) in enumerate(sizes):
        pp = R.pic_params(big, R.Picture(ctus=None, tbs=None, coef=None, size=(w, h)))
        pic = synth.make_picture(pp, 6600 + k + bd, perf=bool(k % 2), deblocking=deblocking)
        pic.size = (w, h)
        pics.append(pic)
    return big, pics


@pytest.mark.parametrize("schedule", ["by_run", "rows", "steps"])
@pytest.mark.parametrize("bd,lg,deblocking", [(8, 5, True), (8, 4, False), (10, 6, True), (12, 5, False)])
def test_ragged_batch(recon_mod, monkeypatch, bd, lg, deblocking, schedule):
    """Six picture sizes in one 3 x 3 CTB context: pic_geo keeps cw = ch = 0 for every picture of the batch."""
    big, pics = _ragged(bd, lg, deblocking)
    want = _luma_ref(big, pics)
    _set_env(monkeypatch, schedule)
    d = _decode(recon_mod, big, [M.to_mono(p) for p in pics], want, "ragged bd%d ctb%d %s" % (bd, 1 << lg, schedule))
    _assert_layout(d, schedule, bd, "ragged")


@pytest.mark.parametrize("bd", [8, 10])
def test_sparse_upload(recon_mod, monkeypatch, bd):
    params = R.make_params(pic_width=200, pic_height=136, ctb_log2_size=5, bit_depth_luma=bd, bit_depth_chroma=bd,
                           loop_filter_across_tiles=0)
    full = [synth.make_picture(params, 6700 + s, **TILES_KW) for s in range(3)]
    _set_env(monkeypatch, "by_run")
    d = _decode(recon_mod, params, [M.to_mono(p) for p in full], _luma_ref(params, full), "sparse bd%d" % bd, sparse=True)
    assert d["last_launch_layout"] == "luma"


@pytest.mark.parametrize("bd", [8, 10])
def test_recon_input_takes_luma_only(recon_mod, monkeypatch, bd):
    """P265R_PIC_RECON_INPUT: the luma reconstruction alone goes up (recon[1..2] stay null); only the filters run."""
    params = R.make_params(pic_width=136, pic_height=72, ctb_log2_size=4, bit_depth_luma=bd, bit_depth_chroma=bd)
    full = [synth.make_picture(params, 6800 + s, perf=False, deblocking=True) for s in range(2)]
    want = _luma_ref(params, full)
    pics = []
    for p, (rec_y, _) in zip(full, want):
        m = M.to_mono(p)
        m.recon_input = [np.ascontiguousarray(rec_y)]
        pics.append(m)
    _set_env(monkeypatch, "by_run")
    with recon_mod.ReconContext(M.mono_params(params)) as ctx:
        outs = ctx.decode(pics)
        d = ctx.describe()
    _compare(outs, None, want, "recon input bd%d" % bd)
    assert d["last_launch_layout"] == "none"                # no intra phase ran


def test_resident_batches_over_two_lanes_with_digests(recon_mod, monkeypatch):
    """Three resident batches over two lanes, each run twice, a device digest after every run: equal to digest.py on
    Y; the entries of planes 1 and 2 are zero.  W = 12 while a lane runs alone, W = 8 beside another lane's run."""
    params = R.make_params(pic_width=200, pic_height=136, ctb_log2_size=5)
    full = [synth.make_picture(params, 6900 + s, perf=bool(s % 2), deblocking=bool(s % 3 == 0)) for s in range(9)]
    want = _luma_ref(params, full)
    mono = [M.to_mono(p) for p in full]
    _set_env(monkeypatch, "nosplit")
    with recon_mod.ReconContext(M.mono_params(params)) as ctx:
        ctx.set_pipeline(2)
        batches = [ctx.upload(mono[3 * k:3 * k + 3]) for k in range(3)]
        for rep in range(2):
            for b in batches:
                ctx.run(b)
                ctx.digest_async(b, rep)
                ctx.digest_async(b, 2 + rep, recon=True)
        d = ctx.describe()
        for k, b in enumerate(batches):
            slots = ctx.digest_slots(b, 4)
            for i in range(3):
                rec_y, out_y = want[3 * k + i]
                for rep in range(2):
                    assert int(slots[rep, i, 0]) == digest.plane_digest(out_y), (k, i, rep)
                    assert int(slots[2 + rep, i, 0]) == digest.plane_digest(rec_y), (k, i, rep)
            assert not slots[:, :, 1:].any()
            got = ctx.digest(b)
            assert not got[:, 1:].any() and [int(v) for v in got[:, 0]] == [digest.plane_digest(want[3 * k + i][1]) for i in range(3)]
            assert ctx.job_count(b)[1] == 0 and ctx.job_count(b)[0] > 0
        outs = [o for b in batches for o in ctx.download(b)]
        for b in batches:
            b.free()
    assert d["last_launch_layout"] == "luma" and d["row_launches"]["w12"] >= 1 and d["row_launches"]["w8"] >= 1, d["row_launches"]
    _compare(outs, None, want, "two lanes")


# ---- picture hash ------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("bd", [8, 10])
@pytest.mark.parametrize("w,h", [(72, 40), (528, 520)])
def test_device_picture_hash(recon_mod, monkeypatch, w, h, bd):
    """MD5, CRC and checksum of Y on the device equal p265r_plane_hash_host and streamgen.picture_hash of the oracle's
    Y (528 x 520: the size tests/test_gpu_picture_hash.py uses to cross hash segments); bytes 16..47 of every picture
    are zero."""
    params = R.make_params(pic_width=w, pic_height=h, ctb_log2_size=5, bit_depth_luma=bd, bit_depth_chroma=bd)
    full = [synth.make_picture(params, 7000 + w + s, perf=True, deblocking=bool(s)) for s in range(2)]
    want = _luma_ref(params, full)
    _set_env(monkeypatch, "by_run")
    with recon_mod.ReconContext(M.mono_params(params)) as ctx:
        b = ctx.upload([M.to_mono(p) for p in full])
        ctx.run(b)
        for kind, code in (("md5", _lib.HASH_MD5), ("crc", _lib.HASH_CRC), ("checksum", _lib.HASH_CHECKSUM)):
            got = ctx.picture_hash(b, code)
            raw = ctx.hash_read(b)
            assert not raw[:, 1:, :].any(), kind
            for i, (_, out_y) in enumerate(want):
                y = np.asarray(out_y, np.uint8 if bd == 8 else np.uint16)
                assert len(got[i]) == 1
                assert got[i][0] == streamgen.picture_hash([y], kind)[0], (kind, i)
                assert got[i][0] == recon_mod.plane_hash_host(y, code, seg_words=1024), (kind, i)
        b.free()


# ---- refusals ----------------------------------------------------------------------------------------------------------

def test_chroma_records_are_refused_before_any_launch(recon_mod):
    params = R.make_params(pic_width=136, pic_height=72, ctb_log2_size=5)
    full = synth.make_picture(params, 7100, perf=False, deblocking=True)
    ok = M.to_mono(full)
    with recon_mod.ReconContext(M.mono_params(params)) as ctx:
        for bad in (full, dataclasses.replace(ok, ctus=_with(ok.ctus, "sao_type", (3, 1), 2, also=(3, 2)))):
            with pytest.raises(_lib.P265RError) as ei:
                ctx.upload([bad])
            assert ei.value.code == _lib.EINVAL
            with pytest.raises(_lib.P265RError) as ei:
                ctx.upload([ok, bad], sparse=True)
            assert ei.value.code == _lib.EINVAL
        d = ctx.describe()
        assert d["last_launch_layout"] == "none" and not any(d["row_launches"].values())
        outs = ctx.decode([ok])                                  # the context is still good
    np.testing.assert_array_equal(outs[0][0], _luma_ref(params, [full])[0][1])
    for idc in (2, 3):
        kw = R.params_dict(params)
        kw["chroma_format_idc"] = idc
        with pytest.raises(_lib.P265RError) as ei:
            recon_mod.ReconContext(R.make_params(**kw))
        assert ei.value.code == _lib.EINVAL


def _with(ctus, field, at, value, also=None):
    c = ctus.copy()
    c[field][at] = value
    if also is not None:
        c[field][also] = value
    return c
