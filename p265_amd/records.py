"""Record format of the reconstruction batch (numpy mirror of include/p265r.h).

The reference decoder keeps everything the hot path needs inside its syntax-tree
objects (decoder/cu.py, decoder/tu.py, decoder/sao.py) and reads it back per sample
through tree walks (tu.py:667-701, ctu.py:33-71).  The MI355X back-end instead
receives flat, fixed-size records per picture:

  CTU_DTYPE  one per CTU (raster order): TB range, slice/tile ids, SAO parameters
  TB_DTYPE   one per transform block in decode order: position, size, component,
             intra mode, flags, qP, offset of its dense int16 coefficients
  coef       int16 TransCoeffLevel, N*N raster [y][x] per coded TB

``Picture`` bundles them; ``Params`` is the 32-byte sequence-parameter POD.
"""
from dataclasses import dataclass, field
from typing import Optional

import numpy as np

ABI_VERSION = 2                 # include/p265r.h P265R_ABI_VERSION (2: per-picture size)

TB_CBF, TB_TSKIP, TB_BYPASS, TB_PCM = 0x01, 0x02, 0x04, 0x08
PIC_RECON_INPUT = 0x01
CTU_LF_ACROSS_SLICES, CTU_DEBLOCK = 0x01, 0x02

PARAMS_DTYPE = np.dtype([
    ("version", "<u4"), ("pic_width", "<u2"), ("pic_height", "<u2"),
    ("chroma_format_idc", "u1"), ("bit_depth_luma", "u1"), ("bit_depth_chroma", "u1"),
    ("ctb_log2_size", "u1"), ("min_tb_log2_size", "u1"), ("max_tb_log2_size", "u1"),
    ("strong_intra_smoothing", "u1"), ("constrained_intra_pred", "u1"),
    ("sample_adaptive_offset", "u1"), ("loop_filter_across_tiles", "u1"),
    ("scaling_list_enabled", "u1"), ("pps_cb_qp_offset", "i1"), ("pps_cr_qp_offset", "i1"),
    ("split_bit_depth", "u1"), ("reserved", "u1", 10)])
assert PARAMS_DTYPE.itemsize == 32

CTU_DTYPE = np.dtype([
    ("tb_begin", "<u4"), ("tb_count", "<u2"), ("tile_id", "<u2"), ("slice_addr", "<u4"),
    ("flags", "u1"), ("sao_type", "u1", 3), ("sao_class", "u1", 3), ("deblock_offsets", "u1"),
    ("sao_offset", "i1", (3, 4))])
assert CTU_DTYPE.itemsize == 32

TB_DTYPE = np.dtype([
    ("x", "<u2"), ("y", "<u2"), ("log2_size", "u1"), ("c_idx", "u1"), ("pred_mode", "u1"),
    ("flags", "u1"), ("qp", "u1"), ("reserved", "u1", 3), ("coef_off", "<u4")])
assert TB_DTYPE.itemsize == 16

PARAM_KEYS = [n for n in PARAMS_DTYPE.names if n not in ("version", "reserved")]


def make_params(**kw) -> np.ndarray:
    """Build a params record; unspecified fields default to the sanity.bin-like SPS/PPS."""
    d = dict(pic_width=352, pic_height=288, chroma_format_idc=1, bit_depth_luma=8,
             bit_depth_chroma=8, ctb_log2_size=6, min_tb_log2_size=2, max_tb_log2_size=5,
             strong_intra_smoothing=1, constrained_intra_pred=0, sample_adaptive_offset=1,
             loop_filter_across_tiles=1, scaling_list_enabled=0, pps_cb_qp_offset=0, pps_cr_qp_offset=0,
             split_bit_depth=0)
    for k, v in kw.items():
        if k not in d:
            raise KeyError("unknown params field %r" % k)
        d[k] = v
    p = np.zeros((), PARAMS_DTYPE)
    p["version"] = ABI_VERSION
    for k, v in d.items():
        p[k] = v
    return p


def is_mono(params) -> bool:
    """chroma_format_idc 0 (4:0:0, ChromaArrayType 0): a picture is its luma plane alone."""
    return int(params["chroma_format_idc"]) == 0


def n_planes(params) -> int:
    """Planes of a decoded picture: 3 (Y, Cb, Cr), or 1 (Y) for monochrome params."""
    return 1 if is_mono(params) else 3


def require_420(params, what):
    """The tile, halo and multi-rank paths handle three planes of one sample type: monochrome params and params
    with unequal bit depths are refused by name."""
    if is_mono(params):
        raise ValueError("%s: monochrome (chroma_format_idc 0) pictures are not supported here; decode them as "
                         "whole pictures (recon.ReconContext, decoder.decode_*)" % what)
    require_equal_depths(params, what)


def split_depths(params) -> bool:
    """BitDepthY != BitDepthC (4:2:0 params; a monochrome picture has no chroma depth)."""
    return not is_mono(params) and int(params["bit_depth_luma"]) != int(params["bit_depth_chroma"])


def require_equal_depths(params, what):
    """The tile, halo and multi-rank paths, the device-side output and the device-side picture hash take one bit
    depth per picture: params with BitDepthY != BitDepthC are refused by name."""
    if split_depths(params):
        raise ValueError("%s: unequal bit depths (BitDepthY %d, BitDepthC %d) are not supported here; decode such "
                         "pictures whole (recon.ReconContext, decoder.decode_*) with host hashing and host output"
                         % (what, int(params["bit_depth_luma"]), int(params["bit_depth_chroma"])))


def check_depths(params):
    """The bit-depth rules of p265r_create: each depth 8..12; unequal depths only with split_bit_depth = 1 (a value
    above 1 is invalid).  Monochrome params: the luma depth alone."""
    y, c, f = int(params["bit_depth_luma"]), int(params["bit_depth_chroma"]), int(params["split_bit_depth"])
    if not 8 <= y <= 12:
        raise RecordError("bit_depth_luma %d outside 8..12" % y)
    if is_mono(params):
        return
    if f > 1:
        raise RecordError("split_bit_depth is 0 or 1, got %d" % f)
    if f == 0 and y != c:
        raise RecordError("bit depths %d / %d differ without split_bit_depth" % (y, c))
    if not 8 <= c <= 12:
        raise RecordError("bit_depth_chroma %d outside 8..12" % c)


def plane_dtypes(params):
    """numpy sample type of the Y, Cb, Cr planes: uint8 at BitDepth 8, uint16 (little-endian) above
    (include/p265r.h p265r_picture.out / recon).  Monochrome params: the Y plane alone."""
    dy = np.uint8 if int(params["bit_depth_luma"]) <= 8 else np.uint16
    if is_mono(params):
        return [dy]
    dc = np.uint8 if int(params["bit_depth_chroma"]) <= 8 else np.uint16
    return [dy, dc, dc]


def plane_shapes(params):
    """[y][x] shapes of the planes plane_dtypes() lists (4:2:0 chroma: half size each way)."""
    w, h = int(params["pic_width"]), int(params["pic_height"])
    if is_mono(params):
        return [(h, w)]
    return [(h, w), (h // 2, w // 2), (h // 2, w // 2)]


def qp_bd_offset(params, c_idx=0) -> int:
    """QpBdOffsetY / QpBdOffsetC = 6 * (BitDepth - 8) (7.4.3.2.1)."""
    return 6 * (int(params["bit_depth_luma" if c_idx == 0 else "bit_depth_chroma"]) - 8)


def deblock_offsets(beta_offset_div2, tc_offset_div2) -> int:
    """P265R_DEBLOCK_OFFSETS: two 4-bit two's-complement fields (each -6..6)."""
    for v in (beta_offset_div2, tc_offset_div2):
        if not -6 <= v <= 6:
            raise ValueError("deblocking offset_div2 out of range: %d" % v)
    return (beta_offset_div2 & 15) | ((tc_offset_div2 & 15) << 4)


def unpack_deblock_offsets(v):
    """(slice_beta_offset_div2, slice_tc_offset_div2) of a CTU record's deblock_offsets byte."""
    b, t = int(v) & 15, (int(v) >> 4) & 15
    return (b - 16 if b >= 8 else b), (t - 16 if t >= 8 else t)


def params_dict(p) -> dict:
    return {k: int(p[k]) for k in PARAM_KEYS}


def pic_params(params, pic):
    """The parameter set one picture of a batch decodes with: the context's ``params``, with the
    picture's own size when it has one (Picture.size, a ragged batch)."""
    if pic is None or pic.size is None:
        return params
    w, h = (int(v) for v in pic.size)
    if w == int(params["pic_width"]) and h == int(params["pic_height"]):
        return params
    if w > int(params["pic_width"]) or h > int(params["pic_height"]) or w <= 0 or h <= 0 or w % 8 or h % 8:
        raise RecordError("picture size %dx%d does not fit the context's %dx%d (multiples of 8)"
                          % (w, h, int(params["pic_width"]), int(params["pic_height"])))
    kw = params_dict(params)
    kw.update(pic_width=w, pic_height=h)
    return make_params(**kw)


def ctb_grid(p):
    ctb = 1 << int(p["ctb_log2_size"])
    w, h = int(p["pic_width"]), int(p["pic_height"])
    return (w + ctb - 1) // ctb, (h + ctb - 1) // ctb


@dataclass
class Picture:
    """Records of one picture (the C struct p265r_picture without the output planes)."""
    ctus: np.ndarray                      # CTU_DTYPE, raster order
    tbs: np.ndarray                       # TB_DTYPE
    coef: np.ndarray                      # int16
    nofilter: Optional[np.ndarray] = None  # uint8 per 8x8 luma block or None
    meta: dict = field(default_factory=dict)
    # P265R_PIC_RECON_INPUT: the reconstruction [Y, Cb, Cr] (uint8) is given; only the
    # in-loop filters run on it (TB records then serve the deblocking map only)
    recon_input: Optional[list] = None
    # this picture's luma (width, height) when it is smaller than the batch context's params
    # (p265r_picture.pic_width / pic_height): the uneven tiles of one picture in one batch
    size: Optional[tuple] = None

    def as_oracle_dict(self):
        return {"ctus": self.ctus, "tbs": self.tbs, "coef": self.coef, "nofilter": self.nofilter}

    @property
    def n_coded_coef(self):
        m = (self.tbs["flags"] & (TB_CBF | TB_PCM)) != 0
        return int(np.sum(1 << (2 * self.tbs["log2_size"][m].astype(np.int64))))


class RecordError(ValueError):
    pass


@dataclass
class SparsePicture:
    """A picture whose transformed TBs carry their coefficients as entries (include/p265r.h
    p265r_sparse_coef, p265r_batch_upload_sparse): ``nz`` uint32 entries pos | (uint16)level << 16,
    ``tbs`` with coef_off = first entry and the entry count in reserved[0..1] for sparse TBs (CBF
    without PCM / bypass), coef_off into ``coef`` (the PCM / bypass samples alone) for the others."""
    ctus: np.ndarray
    tbs: np.ndarray
    nz: np.ndarray                         # uint32
    coef: np.ndarray                       # int16: raw (PCM / bypass) samples only
    nofilter: Optional[np.ndarray] = None
    size: Optional[tuple] = None
    recon_input: Optional[list] = None
    meta: dict = field(default_factory=dict)
    # the dense coef_off of every TB of the picture sparsify() was given, so that densify() restores that
    # layout exactly (a picture built tile by tile keeps its coefficients in tile-scan order); None: TB order
    dense_off: Optional[np.ndarray] = None


def _tb_kinds(tbs):
    """(sparse, raw) masks of a TB array: coded through a transform (or transform skip) / coded PCM or
    bypass (dense by nature)."""
    f = tbs["flags"]
    dense_kind = (f & (TB_PCM | TB_BYPASS)) != 0
    return ((f & TB_CBF) != 0) & ~dense_kind, ((f & (TB_CBF | TB_PCM)) != 0) & dense_kind


def _ranges(starts, lengths):
    """Concatenated aranges start[i] .. start[i] + length[i], and the index i of every element."""
    lengths = lengths.astype(np.int64)
    owner = np.repeat(np.arange(len(lengths)), lengths)
    first = np.cumsum(lengths) - lengths
    within = np.arange(int(lengths.sum()), dtype=np.int64) - np.repeat(first, lengths)
    return np.repeat(starts.astype(np.int64), lengths) + within, owner, within


def sparsify(pic: Picture) -> SparsePicture:
    """The sparse form of a dense picture (what the C p265r_sparsify computes): the non-zero levels of
    every transformed TB in raster order, the PCM / bypass samples compacted in TB order."""
    tbs = pic.tbs.copy()
    tbs["reserved"] = 0
    dense_off = pic.tbs["coef_off"].copy()
    coef = np.ascontiguousarray(pic.coef, np.int16)
    sparse, raw = _tb_kinds(tbs)
    nn = 1 << (2 * tbs["log2_size"].astype(np.int64))
    if ((tbs["coef_off"].astype(np.int64) + nn)[sparse | raw] > len(coef)).any():
        raise RecordError("coefficient range outside coef array")
    si = np.flatnonzero(sparse)
    idx, owner, pos = _ranges(tbs["coef_off"][si], nn[si])
    val = coef[idx]
    keep = val != 0
    nz = (pos[keep].astype(np.uint32) | (val[keep].view(np.uint16).astype(np.uint32) << 16)).astype(np.uint32)
    count = np.bincount(owner[keep], minlength=len(si)).astype(np.int64)
    tbs["coef_off"][si] = np.cumsum(count) - count
    tbs["reserved"][si, 0] = count & 0xff
    tbs["reserved"][si, 1] = count >> 8
    ri = np.flatnonzero(raw)
    ridx, _, _ = _ranges(tbs["coef_off"][ri], nn[ri])
    tbs["coef_off"][ri] = np.cumsum(nn[ri]) - nn[ri]
    return SparsePicture(ctus=pic.ctus, tbs=tbs, nz=nz, coef=coef[ridx], nofilter=pic.nofilter, size=pic.size,
                         recon_input=pic.recon_input, meta=dict(pic.meta), dense_off=dense_off)


def densify(sp: SparsePicture) -> Picture:
    """The dense picture of a sparse one: every coded TB's N*N values at the offsets sparsify() found
    them (``dense_off``: densify(sparsify(pic)) == pic), else packed in TB order."""
    tbs = sp.tbs.copy()
    sparse, raw = _tb_kinds(tbs)
    nn = 1 << (2 * tbs["log2_size"].astype(np.int64))
    coded = sparse | raw
    off = np.zeros(len(tbs), np.int64)
    off[coded] = np.cumsum(nn[coded]) - nn[coded]
    n_coef = int(nn[coded].sum())
    if sp.dense_off is not None:
        off = sp.dense_off.astype(np.int64)
        n_coef = int((off + nn)[coded].max()) if coded.any() else 0
    coef = np.zeros(n_coef, np.int16)
    si = np.flatnonzero(sparse)
    count = tbs["reserved"][si, 0].astype(np.int64) | (tbs["reserved"][si, 1].astype(np.int64) << 8)
    eidx, owner, _ = _ranges(tbs["coef_off"][si], count)
    if len(eidx) and int(eidx.max()) >= len(sp.nz):
        raise RecordError("entry range outside the entry array")
    ent = np.ascontiguousarray(sp.nz, np.uint32)[eidx]
    pos = (ent & 0xffff).astype(np.int64)
    if (pos >= nn[si][owner]).any():
        raise RecordError("entry position outside its TB")
    coef[off[si][owner] + pos] = (ent >> 16).astype(np.uint16).view(np.int16)
    ri = np.flatnonzero(raw)
    ridx, rowner, rpos = _ranges(tbs["coef_off"][ri], nn[ri])
    if len(ridx) and int(ridx.max()) >= len(sp.coef):
        raise RecordError("raw sample range outside coef array")
    coef[off[ri][rowner] + rpos] = np.ascontiguousarray(sp.coef, np.int16)[ridx]
    tbs["coef_off"] = np.where(coded | (sp.dense_off is not None), off, tbs["coef_off"])
    tbs["reserved"] = 0
    return Picture(ctus=sp.ctus, tbs=tbs, coef=coef, nofilter=sp.nofilter, meta=dict(sp.meta),
                   recon_input=sp.recon_input, size=sp.size)


def check_shapes(params, pic: Picture):
    """The checks the C ABI cannot do itself (array dtypes and lengths behind the raw
    pointers); everything inside the records is validated again by p265r_batch_upload."""
    params = pic_params(params, pic)
    wc, hc = ctb_grid(params)
    if pic.ctus.dtype != CTU_DTYPE or pic.tbs.dtype != TB_DTYPE or pic.coef.dtype != np.int16:
        raise RecordError("record dtypes do not match the ABI")
    if len(pic.ctus) != wc * hc:
        raise RecordError("expected %d CTUs, got %d" % (wc * hc, len(pic.ctus)))
    w, h = int(params["pic_width"]), int(params["pic_height"])
    if pic.nofilter is not None and len(pic.nofilter) != ((w + 7) // 8) * ((h + 7) // 8):
        raise RecordError("nofilter map has the wrong size")


def validate(params, pic: Picture):
    """Host-side checks mirroring the C++ ones (p265_amd/csrc/upload_host.cpp: validate_picture).

    The kernels assume every record lies inside its CTU and picture; these checks are
    what keeps a malformed record from faulting the GPU.
    """
    params = pic_params(params, pic)
    check_depths(params)
    wc, hc = ctb_grid(params)
    if pic.ctus.dtype != CTU_DTYPE or pic.tbs.dtype != TB_DTYPE or pic.coef.dtype != np.int16:
        raise RecordError("record dtypes do not match the ABI")
    if len(pic.ctus) != wc * hc:
        raise RecordError("expected %d CTUs, got %d" % (wc * hc, len(pic.ctus)))
    ctb_log2 = int(params["ctb_log2_size"])
    w, h = int(params["pic_width"]), int(params["pic_height"])
    tbs = pic.tbs
    begin = pic.ctus["tb_begin"].astype(np.int64)
    end = begin + pic.ctus["tb_count"]
    if (end > len(tbs)).any():
        raise RecordError("CTU TB range outside the TB array")
    lg = tbs["log2_size"].astype(np.int64)
    c = tbs["c_idx"].astype(np.int64)
    if ((lg < 2) | (lg > 5)).any() or (c > 2).any() or (tbs["pred_mode"] > 34).any():
        raise RecordError("TB size / component / mode out of range")
    if ((c > 0) & (lg > 4)).any():
        raise RecordError("4:2:0 chroma TB larger than 16x16")
    if (pic.ctus["tb_count"].astype(np.int64) > 3 * (1 << (2 * (ctb_log2 - 2))) // 2).any():
        raise RecordError("CTU lists more TBs than it has 4x4 units")
    cs = np.concatenate([[0], np.cumsum(tbs["c_idx"] == 0)])
    if ((cs[end] - cs[begin]) > (1 << (2 * (ctb_log2 - 2)))).any():
        raise RecordError("CTU lists more luma TBs than it has 4x4 units")
    cc = np.concatenate([[0], np.cumsum(tbs["c_idx"] != 0)])
    if ((cc[end] - cc[begin]) > 2 * (1 << (2 * (ctb_log2 - 3)))).any():
        raise RecordError("CTU lists more chroma TBs than it has 4x4 chroma units")
    qp_max = np.where(c > 0, 51 + qp_bd_offset(params, 1), 51 + qp_bd_offset(params, 0))
    if (tbs["qp"] > qp_max).any():
        raise RecordError("TB qp above 51 + QpBdOffset of its component")
    sub = (c > 0).astype(np.int64)
    xl, yl = tbs["x"].astype(np.int64) << sub, tbs["y"].astype(np.int64) << sub
    nl = (1 << lg) << sub
    if ((xl >= w) | (yl >= h)).any():
        raise RecordError("TB outside picture")
    counts = pic.ctus["tb_count"].astype(np.int64)
    owner = np.repeat(np.arange(len(pic.ctus)), counts)
    # idx[k] = TB index of the k-th (CTU, TB) pair: tb_begin of its CTU + rank inside the CTU
    first = np.cumsum(counts) - counts
    idx = np.repeat(begin, counts) + (np.arange(int(counts.sum())) - np.repeat(first, counts))
    if len(idx):
        cx, cy = (owner % wc) << ctb_log2, (owner // wc) << ctb_log2
        ctb = 1 << ctb_log2
        bad = ((xl[idx] < cx) | (yl[idx] < cy) | (xl[idx] + nl[idx] > cx + ctb) | (yl[idx] + nl[idx] > cy + ctb))
        if bad.any():
            raise RecordError("TB not inside its CTU")
    coded = (tbs["flags"] & (TB_CBF | TB_PCM)) != 0
    if (tbs["coef_off"][coded].astype(np.int64) + (1 << (2 * lg[coded])) > len(pic.coef)).any():
        raise RecordError("coefficient range outside coef array")
    if (pic.ctus["sao_type"] > 2).any():
        raise RecordError("bad SaoTypeIdx")
    if is_mono(params):
        if (c > 0).any():
            raise RecordError("chroma TB in a monochrome picture")
        if (pic.ctus["sao_type"][:, 1:] != 0).any():
            raise RecordError("chroma SaoTypeIdx in a monochrome picture")
    st, sc = pic.ctus["sao_type"], pic.ctus["sao_class"]
    if ((st[:, 1] != st[:, 2]) | ((st[:, 1] == 2) & (sc[:, 1] != sc[:, 2]))).any():
        raise RecordError("Cb and Cr must share SaoTypeIdx and SaoEoClass (7.4.9.3.2)")
    nib = np.stack([pic.ctus["deblock_offsets"] & 15, pic.ctus["deblock_offsets"] >> 4])
    if ((nib == 7) | (nib == 8) | (nib == 9)).any():
        raise RecordError("deblocking offset_div2 outside -6..6")
    if pic.nofilter is not None and len(pic.nofilter) != ((w + 7) // 8) * ((h + 7) // 8):
        raise RecordError("nofilter map has the wrong size")
