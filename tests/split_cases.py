"""The seeded pictures of the unequal-bit-depth tests (tests/test_split_depth.py on the CPU,
tests/test_gpu_split_depth.py on the GPU) and their references: the C oracle's planes, computed once per case."""
import functools

from oracle import c_oracle
from p265_amd import records as R
from p265_amd import synth

# (BitDepthY, BitDepthC) for k = 0..6
PAIRS = [(8, 10), (10, 8), (8, 12), (12, 8), (10, 12), (12, 10), (9, 11)]


def split_params(y, c, **kw):
    return R.make_params(bit_depth_luma=y, bit_depth_chroma=c, split_bit_depth=int(y != c), **kw)


def tiles_case(k):
    """200 x 136, CTB 32, 2 x 2 tiles, 3 slices, random deblocking, bypass, PCM, transform skip."""
    y, c = PAIRS[k]
    params = split_params(y, c, pic_width=200, pic_height=136, ctb_log2_size=5, loop_filter_across_tiles=0,
                          pps_cb_qp_offset=-1, pps_cr_qp_offset=2)
    pics = [synth.make_picture(params, 7300 + 10 * k + s, perf=False, tiles=(2, 2), n_slices=3, lf_across_slices=None,
                               deblocking="random", bypass_rate=0.05, pcm_rate=0.03, tskip_rate=0.3) for s in range(2)]
    return params, pics


def uniform_case(k):
    """136 x 72, CTB 64, no PCM, deblocking on: uniformly random modes and QPs (the planes reach 0 and the maximum)."""
    y, c = PAIRS[k]
    params = split_params(y, c, pic_width=136, pic_height=72, ctb_log2_size=6, pps_cb_qp_offset=2, pps_cr_qp_offset=-2)
    pics = [synth.make_picture(params, 7500 + 10 * k + s, perf=False, deblocking=True) for s in range(3)]
    return params, pics


def narrow_case(k):
    """72 x 40, CTB 16: chroma rows of 36 samples -- two full 16-byte groups of the narrowing kernel plus 4 bytes."""
    y, c = PAIRS[k]
    params = split_params(y, c, pic_width=72, pic_height=40, ctb_log2_size=4)
    pics = [synth.make_picture(params, 7700 + 10 * k + s, perf=False, deblocking="random", pcm_rate=0.02) for s in range(2)]
    return params, pics


def ragged_case(k):
    """264 x 200, 128 x 72 and 40 x 200 pictures in one 264 x 200 context (CTB 32)."""
    y, c = PAIRS[k]
    big = split_params(y, c, pic_width=264, pic_height=200, ctb_log2_size=5)
    pics = []
    for j, (w, h) in enumerate([(264, 200), (128, 72), (40, 200)]):
        pp = R.pic_params(big, R.Picture(ctus=None, tbs=None, coef=None, size=(w, h)))
        pic = synth.make_picture(pp, 7800 + 10 * k + j, perf=bool(j % 2), deblocking=bool(j % 2))
        pic.size = (w, h)
        pics.append(pic)
    return big, pics


def sao_only_case(k):
    """136 x 72, CTB 32, SAO without deblocking (the streaming SAO kernel of the 16-bit path)."""
    y, c = PAIRS[k]
    params = split_params(y, c, pic_width=136, pic_height=72, ctb_log2_size=5)
    pics = [synth.make_picture(params, 7900 + 10 * k + s, perf=False, deblocking=False, tskip_rate=0.2, pcm_rate=0.02)
            for s in range(2)]
    return params, pics


def no_sao_case(k, deblocking):
    y, c = PAIRS[k]
    params = split_params(y, c, pic_width=128, pic_height=64, sample_adaptive_offset=0)
    pics = [synth.make_picture(params, 8000 + 10 * k + s, perf=False, deblocking=deblocking) for s in range(2)]
    return params, pics


CASES = {"tiles": tiles_case, "uniform": uniform_case, "narrow": narrow_case, "ragged": ragged_case,
         "sao_only": sao_only_case, "no_sao_dbk": lambda k: no_sao_case(k, True), "no_sao": lambda k: no_sao_case(k, False)}


@functools.lru_cache(maxsize=None)
def case(name, k):
    """(params, pictures, [(recon planes, out planes)] of the C oracle) -- shared, read-only."""
    params, pics = CASES[name](k)
    refs = c_oracle.decode(params, pics, threads=4)
    for rec, out in refs:
        for p in list(rec) + list(out):
            p.flags.writeable = False
    return params, pics, refs
