"""Monochrome (4:0:0) twins of 4:2:0 record sets.

``to_mono(pic)`` drops the chroma TB records of a 4:2:0 ``records.Picture``, renumbers the CTU ranges and clears
the chroma SAO parameters; ``mono_params(params)`` is the parameter set that goes with it (chroma_format_idc 0,
one bit depth, no chroma QP offsets).  Luma reconstruction, luma deblocking and luma SAO read no chroma sample
and no chroma record (tests/test_mono_records.py checks that with both oracles), so the expected planes of a
monochrome picture are plane 0 of what the oracles compute for the 4:2:0 picture it came from: every seeded or
planted set of the repository is a monochrome set too.
"""
import numpy as np

from p265_amd import records as R


def mono_params(params):
    kw = R.params_dict(params)
    kw.update(chroma_format_idc=0, bit_depth_chroma=kw["bit_depth_luma"], pps_cb_qp_offset=0, pps_cr_qp_offset=0)
    return R.make_params(**kw)


def to_mono(pic):
    """The picture without its chroma records.  Every CTU keeps its luma TBs in their order; the TB array is
    rebuilt CTU by CTU (raster), so records no CTU lists are dropped too.  The coefficient array stays whole
    (the chroma blocks in it are no longer referenced)."""
    ctus = pic.ctus.copy()
    begin = ctus["tb_begin"].astype(np.int64)
    count = ctus["tb_count"].astype(np.int64)
    first = np.cumsum(count) - count
    idx = np.repeat(begin, count) + (np.arange(int(count.sum())) - np.repeat(first, count))
    owner = np.repeat(np.arange(len(ctus)), count)
    keep = pic.tbs["c_idx"][idx] == 0
    tbs = np.ascontiguousarray(pic.tbs[idx[keep]])
    n_luma = np.bincount(owner[keep], minlength=len(ctus)).astype(np.int64)
    ctus["tb_count"] = n_luma
    ctus["tb_begin"] = np.cumsum(n_luma) - n_luma
    ctus["sao_type"][:, 1:] = 0
    ctus["sao_class"][:, 1:] = 0
    ctus["sao_offset"][:, 1:, :] = 0
    rin = None if pic.recon_input is None else [pic.recon_input[0]]
    return R.Picture(ctus=ctus, tbs=tbs, coef=pic.coef, nofilter=pic.nofilter, meta=dict(pic.meta, mono=True),
                     recon_input=rin, size=pic.size)


def luma_list_lengths(pic):
    """Luma TB records per CTU (the length of the CTU's luma list before job prep merges 4x4 quads)."""
    return pic.ctus["tb_count"].astype(np.int64)


def grey(params, shape):
    """A chroma plane of 1 << (BitDepth - 1): what a 4:2:0 consumer is handed for a monochrome picture."""
    bd = int(params["bit_depth_luma"])
    return np.full(shape, 1 << (bd - 1), np.uint8 if bd <= 8 else np.uint16)
