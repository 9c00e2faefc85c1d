"""Planted SAO pictures: PCM pictures (the technique of tests/planted_lf.py) whose samples, SAO parameters and
CTU attributes are chosen so that every rule of 8.7.3 sits at its threshold (plain Python, no GPU).

The reconstruction of a picture of PCM CUs is the planted planes.  Every CU has QpY 0 and every slice zero
deblocking offsets, so beta = tC = 0 and deblocking, where it is on, runs and changes nothing: the SAO input is
the planted planes with deblocking off (the SAO-only kernels) and on (the fused window kernels).  sao_set()
asserts that equality for every picture of a deblocking-on set.

sao_set(bit_depth, ctb_log2, lf_tiles, dbk=False) is the fixed set of one context; every picture's meta["kind"]
says what it plants:

``edge``     128 x 128, four pictures: every CTU edge offset in every component, the classes rotating over the CTUs
             and the pictures, the largest offsets the front-end emits.  Samples are PALETTE[rank]: the rank
             (0, 1, 2) of sample (x, y) is SEQ[(x + 2 y + phase) % 13], a sequence in which every one of the nine
             pairs (sgn(v - a), sgn(v - b)) occurs along each of the four directions (steps 1, 2, 3 and 1 in
             x + 2 y); 13 is prime to 16, so every pair meets every x residue.  The palette changes per vertical
             stripe: (0, 1, 2) and (max - 2, max - 1, max) differ by 1 and clip, (0, A, max) and (0, max - A, max)
             differ by the full range and land on 0 and max exactly (A: the largest offset).
``band``     128 x 128: every CTU band offset; sao_band_position runs over 0..31 (luma; Cb + 11, Cr + 22), every
             CTB holds both end values of all 32 bands, the offsets have mixed signs at the largest magnitude,
             negative on band 0 and positive on band 31.  ``mix``: band, edge and off CTUs side by side.
``wide``     raw sao_offset records: -128, 127, 1, -1, 0 in every slot, both types.
``borders``  3 x 3 CTBs of samples that are strict extrema along all four directions (any allowed filtering
             changes them), under enumerated slice and tile layouts (BORDER_LAYOUTS).
``nofilter`` 136 x 128 of the same samples in 8 x 8 CUs, some with cu_transquant_bypass, some PCM under
             pcm_loop_filter_disabled, at both parities of the 8-block columns and rows.
``strips``   the smallest pictures that cross a strip boundary of the context's strip kernel (strip_size), with a
             partial last lane, tile and slice boundaries around the boundary CTBs, all three types.
"""
import dataclasses

import numpy as np

import planted_lf as L
from oracle import c_oracle
from oracle import recon_oracle as O
from p265_amd import records as R

DEPTHS = (8, 10, 12)
CTB_LOG2 = (4, 5, 6)
SEQ = np.array([1, 2, 2, 2, 2, 1, 0, 0, 0, 1, 0, 2, 0])
DIRS = [(dx, dy) for dy in (-1, 0, 1) for dx in (-1, 0, 1) if dx or dy]


def max_abs(bd):
    """The largest sao_offset_abs (7.4.9.3.2)."""
    return (1 << (min(bd, 10) - 5)) - 1


def max_offset(bd):
    """The largest SaoOffsetVal magnitude the front-end emits: 7, 31, 31 << 2."""
    return max_abs(bd) << (bd - min(bd, 10))


def params_of(bd, ctb_log2, lf_tiles, w=128, h=128, sao=True):
    return R.make_params(pic_width=w, pic_height=h, ctb_log2_size=ctb_log2, sample_adaptive_offset=int(sao),
                         bit_depth_luma=bd, bit_depth_chroma=bd, loop_filter_across_tiles=int(lf_tiles))


def strip_size(bd, ctb_log2):
    """(width, height, strip) of the context's ``strips`` pictures: sao_rows_kernel 248-sample strips (8 bits,
    CTB 16), sao_strip16_kernel 992 (8 bits, CTB 32 / 64), sao16_strip_kernel 496 (above 8 bits); two CTB rows
    and a partial one."""
    h = (2 << ctb_log2) + 8
    if bd > 8:
        return 1000, h, 496
    return (520, h, 248) if ctb_log2 == 4 else (2008, h, 992)


# ---------------------------------------------------------------------------------
# samples
# ---------------------------------------------------------------------------------

def palettes(bd):
    mx, a = (1 << bd) - 1, max_offset(bd)
    return np.array([(0, 1, 2), (mx - 2, mx - 1, mx), (0, a, mx), (0, mx - a, mx)], np.int64)


def rank_planes(bd, w, h, phase):
    """PALETTE[stripe][SEQ[(x + 2 y + phase) % 13]]; four palette stripes across a plane (at least 16 wide)."""
    out = []
    for c in range(3):
        pw, ph = w >> (c > 0), h >> (c > 0)
        ys, xs = np.mgrid[0:ph, 0:pw]
        stripe = max(16, pw // 4)
        out.append(palettes(bd)[(xs // stripe + phase + c) % 4, SEQ[(xs + 2 * ys + phase + 5 * c) % 13]])
    return out


def band_values(bd):
    """Both end values of all 32 bands."""
    sh = bd - 5
    return np.array([v for k in range(32) for v in (k << sh, ((k + 1) << sh) - 1)], np.int64)


def fill_band(planes, bd, spec, rs):
    """CTB rs of every component: the 64 band end values, over and over, from a phase of the CTB's own."""
    rx, ry = rs % spec.wc, rs // spec.wc
    vals = band_values(bd)
    for c in range(3):
        cs = spec.ctb >> (c > 0)
        blk = planes[c][ry * cs:(ry + 1) * cs, rx * cs:(rx + 1) * cs]
        n = np.arange(blk.size).reshape(blk.shape)
        blk[:] = vals[(n + 7 * rs + 3 * c) % 64]


def extrema_planes(bd, w, h):
    """mid + 2 (x % 2) + 4 (y % 2): the two neighbours along every one of the four directions are equal and
    differ from the sample, so edgeIdx is 1 or 4 for every class and a non-zero offset changes the sample."""
    mid = 1 << (bd - 1)
    out = []
    for c in range(3):
        ys, xs = np.mgrid[0:h >> (c > 0), 0:w >> (c > 0)]
        out.append(mid + 2 * (xs % 2) + 4 * (ys % 2))
    return out


# ---------------------------------------------------------------------------------
# CTU attributes
# ---------------------------------------------------------------------------------

def new_spec(bd, ctb_log2, cu, w, h):
    s = L.Spec(bd, ctb_log2, cu, w, h)
    s.qp[:] = 0
    s.dbk[:] = False
    s.sao = [None] * (s.wc * s.hc)
    s.raw = {}                                       # (rs, c) -> raw sao_offset, written past add_ctu
    return s


def set_sao(spec, rs, types, classes, offsets):
    """CTU rs: per component SaoTypeIdx, class or band position, and four signed offsets in sao_offset_abs
    units (edge offset takes the inferred signs whatever is given)."""
    spec.sao[rs] = dict(sao_type=tuple(types), sao_abs=[[abs(int(v)) for v in o] for o in offsets],
                        sao_sign=[[int(v < 0) for v in o] for o in offsets], sao_band=tuple(classes), sao_eo=tuple(classes))


def set_layout(spec, col_starts=(0,), row_starts=(0,), cuts=(), flags=(1,)):
    """Tiles from the CTB columns / rows they start at; slices are runs in tile-scan order cut at the positions
    ``cuts`` (and at every tile), slice k with slice_loop_filter_across_slices flags[k % len(flags)]."""
    n = spec.wc * spec.hc
    for rs in range(n):
        tc = sum(rs % spec.wc >= c for c in col_starts) - 1
        tr = sum(rs // spec.wc >= r for r in row_starts) - 1
        spec.tile[rs] = tr * len(col_starts) + tc
    sid, prev = 0, None
    for ts, rs in enumerate(np.lexsort((np.arange(n), spec.tile))):
        sid += ts > 0 and (ts in cuts or spec.tile[rs] != prev)
        prev = spec.tile[rs]
        spec.slice[rs], spec.lf_across[rs] = sid, bool(flags[sid % len(flags)])


def _build(spec, planes, lf_tiles, meta):
    planes = [np.ascontiguousarray(p, np.int64) for p in planes]
    pic = L.build(spec, planes, None, meta=meta, params=params_of(spec.bd, spec.ctb_log2, lf_tiles, spec.w, spec.h))
    for (rs, c), o in spec.raw.items():
        pic.ctus["sao_offset"][rs, c] = o
    pic.size = (spec.w, spec.h)
    return pic


def _band_signs(pos, rs):
    """Mixed signs: negative on band 0, positive on band 31, else alternating from the CTU's parity."""
    out = []
    for k in range(4):
        b = (pos + k) & 31
        out.append(-1 if b == 0 else 1 if b == 31 else (-1 if (k + rs) % 2 else 1))
    return out


# ---------------------------------------------------------------------------------
# the kinds
# ---------------------------------------------------------------------------------

def edge_picture(bd, ctb_log2, j):
    s = new_spec(bd, ctb_log2, 16, 128, 128)
    a = [max_abs(bd)] * 4
    for rs in range(s.wc * s.hc):
        k = rs + rs // s.wc + j
        set_sao(s, rs, (2, 2, 2), (k % 4, (k + 2) % 4, (k + 2) % 4), [a, a, a])
    return _build(s, rank_planes(bd, 128, 128, j), 1, dict(kind="edge", j=j))


def n_band_pictures(ctb_log2):
    return max(1, 32 >> (2 * (7 - ctb_log2)))


def band_picture(bd, ctb_log2, j):
    s = new_spec(bd, ctb_log2, 16, 128, 128)
    n, a = s.wc * s.hc, max_abs(bd)
    planes = rank_planes(bd, 128, 128, j)
    for rs in range(n):
        pos = [(n * j + rs + 11 * c) % 32 for c in range(3)]
        set_sao(s, rs, (1, 1, 1), pos, [[a * v for v in _band_signs(p, rs)] for p in pos])
        fill_band(planes, bd, s, rs)
    return _build(s, planes, 1, dict(kind="band", j=j))


def mix_picture(bd, ctb_log2):
    """Band, edge and off CTUs side by side (luma and chroma one step apart), band positions at the wrap."""
    s = new_spec(bd, ctb_log2, 16, 128, 128)
    a = max_abs(bd)
    planes = rank_planes(bd, 128, 128, 2)
    for rs in range(s.wc * s.hc):
        k = rs % s.wc + rs // s.wc
        ty, tc = (1, 2, 0)[k % 3], (2, 0, 1)[k % 3]
        pos = [29 + (rs + c) % 3 for c in range(3)]              # bands 31 and 0 in every window
        cls = [pos[c] if t == 1 else (rs + c) % 4 for c, t in enumerate((ty, tc, tc))]
        cls[2] = cls[2] if tc == 1 else cls[1]
        set_sao(s, rs, (ty, tc, tc), cls, [[a * v for v in _band_signs(cls[c], rs)] for c in range(3)])
        if ty == 1 or tc == 1:
            keep = [p.copy() for p in planes]
            fill_band(planes, bd, s, rs)
            for c, t in enumerate((ty, tc, tc)):
                if t != 1:
                    planes[c] = keep[c]
                    continue
                # two samples of the CTB for the exact landings: A - A = 0 in band 0, (max - A) + A = max in band 31
                cs = s.ctb >> (c > 0)
                planes[c][(rs // s.wc) * cs, (rs % s.wc) * cs:(rs % s.wc) * cs + 2] = (max_offset(bd), (1 << bd) - 1 - max_offset(bd))
    return _build(s, planes, 1, dict(kind="mix"))


WIDE = (-128, 127, 1, -1, 0)


def wide_picture(bd, ctb_log2, j):
    """Raw records: slot i of CTU rs, component c holds WIDE[(rs + c + j + i) % 5]: every value in every slot,
    edge-offset signs of every kind."""
    s = new_spec(bd, ctb_log2, 16, 128, 128)
    planes = rank_planes(bd, 128, 128, j + 1)
    for rs in range(s.wc * s.hc):
        k = rs % s.wc + rs // s.wc + j
        ty, tc = (2, 1) if k % 2 else (1, 2)
        pos = [(28 + rs + 3 * c) % 32 for c in range(3)]
        cls = [pos[0] if ty == 1 else (rs // 2) % 4] + ([pos[1], pos[2]] if tc == 1 else [(rs // 2 + 1) % 4] * 2)
        set_sao(s, rs, (ty, tc, tc), cls, [[1] * 4] * 3)
        keep = [p.copy() for p in planes]
        fill_band(planes, bd, s, rs)
        for c, t in enumerate((ty, tc, tc)):
            s.raw[(rs, c)] = [WIDE[(rs + c + j + i) % 5] for i in range(4)]
            if t != 1:
                planes[c] = keep[c]
    return _build(s, planes, 1, dict(kind="wide", j=j))


def _border_layouts():
    """Slice and tile layouts of a 3 x 3 CTB picture, enumerated: one cut at every CTU and two cuts at every pair
    of consecutive CTUs, with the flags (0, 1, 0) and (1, 0, 1); every way to split the columns and / or the rows
    into tiles, a slice per tile and a slice per CTU, with the flags both ways."""
    out = []
    for f in ((0, 1), (1, 0)):
        out += [dict(cuts=(c,), flags=f) for c in range(1, 9)]
        out += [dict(cuts=(c, c + 1), flags=f) for c in range(1, 8)]
    splits = [(0,), (0, 1), (0, 2), (0, 1, 2)]
    for cols in splits:
        for rows in splits:
            if len(cols) == 1 and len(rows) == 1 or len(cols) + len(rows) > 4:
                continue
            for f in ((0, 1), (1, 0)):
                out.append(dict(col_starts=cols, row_starts=rows, flags=f))
            if len(cols) + len(rows) == 3 or (cols, rows) == ((0, 2), (0, 1)):
                for f in ((0, 1), (1, 0), (1, 1, 0), (0, 0, 1)):
                    out.append(dict(col_starts=cols, row_starts=rows, cuts=tuple(range(1, 9)), flags=f))
    return out


BORDER_LAYOUTS = _border_layouts()
# (layout, class rotation): CTU rs has luma class (rs + rotation) % 4, chroma two further.  Every layout once, and
# again the two that forbid a diagonal between two allowed orthogonals (one cut at the last CTU; two tile columns,
# a slice per CTU), so that the diagonal classes of every component meet them
BORDER_PICTURES = [(li, li % 4) for li in range(len(BORDER_LAYOUTS))] + [(8, 3), (56, 1), (8, 1), (56, 3)]


def borders_picture(bd, ctb_log2, lf_tiles, li, rot):
    n = 3 << ctb_log2
    s = new_spec(bd, ctb_log2, 16, n, n)
    set_layout(s, **BORDER_LAYOUTS[li])
    a = [max_abs(bd)] * 4
    for rs in range(9):
        set_sao(s, rs, (2, 2, 2), ((rs + rot) % 4, (rs + rot + 2) % 4, (rs + rot + 2) % 4), [a, a, a])
    return _build(s, extrema_planes(bd, n, n), lf_tiles, dict(kind="borders", layout=li, rot=rot))


def nofilter_picture(bd, ctb_log2, j):
    s = new_spec(bd, ctb_log2, 8, 136, 128)
    ys, xs = np.mgrid[0:16, 0:17]
    hsh = (3 * xs + 5 * ys + j) % 7
    s.nf, s.nf_pcm = hsh == 0, hsh == 3
    a = [max_abs(bd)] * 4
    for rs in range(s.wc * s.hc):
        t = 1 if rs % 5 == 4 else 2
        set_sao(s, rs, (t, t, t), [15] * 3 if t == 1 else ((rs + j) % 4, (rs + j + 1) % 4, (rs + j + 1) % 4), [a, a, a])
    return _build(s, extrema_planes(bd, 136, 128), 1, dict(kind="nofilter", j=j))


def strips_picture(bd, ctb_log2, lf_tiles, j):
    """Tiles start at the CTB holding the last column before a luma or chroma strip boundary (its left neighbour
    is in another tile), slices are runs of three CTUs with alternating flags (its right neighbour is, sooner or later,
    in another slice); the classes rotate over the CTUs, every fifth CTU is band offset, every seventh off."""
    w, h, strip = strip_size(bd, ctb_log2)
    s = new_spec(bd, ctb_log2, 8, w, h)
    cols = {0} | {(b - 1) >> ctb_log2 for b in range(strip, w, strip)} | {(2 * b - 2) >> ctb_log2 for b in range(strip, w // 2, strip)}
    n = s.wc * s.hc
    set_layout(s, col_starts=tuple(sorted(cols)), cuts=tuple(range(3, n, 3)), flags=(j % 2, 1 - j % 2))
    a = max_abs(bd)
    planes = rank_planes(bd, w, h, j)
    for rs in range(n):
        k = rs % s.wc + rs // s.wc + j
        t = [1 if (k + c) % 5 == 2 else 0 if (k + c) % 7 == 5 else 2 for c in (0, 1)]
        ty, tc = t
        pos = [(30 + rs + 5 * c) % 32 for c in range(3)]
        cls = [pos[0] if ty == 1 else k % 4] + ([pos[1], pos[2]] if tc == 1 else [(k + 1) % 4] * 2)
        if rs % s.wc == s.wc - 1 and rs // s.wc < 2:  # the picture's last column changes under the vertical class and band offset only
            ty = tc = 2 - rs // s.wc
            cls = pos if ty == 1 else [1, 1, 1]
        set_sao(s, rs, (ty, tc, tc), cls, [[a * v for v in _band_signs(cls[c], rs)] for c in range(3)])
        if ty == 1 or tc == 1:
            keep = [p.copy() for p in planes]
            fill_band(planes, bd, s, rs)
            for c, tt in enumerate((ty, tc, tc)):
                if tt != 1:
                    planes[c] = keep[c]
    return _build(s, planes, lf_tiles, dict(kind="strips", j=j, strip=strip))


N_EDGE, N_WIDE, N_NOFILTER, N_STRIPS = 4, 2, 2, 2
_SETS, _SHARED = {}, {}


def _shared(key, fn, *args):
    """Pictures without tiles do not depend on loop_filter_across_tiles: built once for both sets."""
    if key not in _SHARED:
        _SHARED[key] = fn(*args)
    return _SHARED[key]


def with_deblocking(pic):
    """The same picture with deblocking on in every slice (zero offsets; QpY is 0 everywhere)."""
    ctus = pic.ctus.copy()
    ctus["flags"] |= R.CTU_DEBLOCK
    twin = dataclasses.replace(pic, ctus=ctus, meta=dict(pic.meta, dbk=True))
    twin.spec, twin.planes = pic.spec, pic.planes
    return twin


def by_size(pics):
    """{(w, h): [index]} of a set: one batch per picture size."""
    groups = {}
    for i, p in enumerate(pics):
        groups.setdefault(tuple(p.size), []).append(i)
    return groups


def c_decode(bd, ctb_log2, lf_tiles, pics, sao=True):
    """[(recon, out)] of the C oracle, every picture at its own size."""
    res = [None] * len(pics)
    for (w, h), idx in by_size(pics).items():
        prm = params_of(bd, ctb_log2, lf_tiles, w, h, sao)
        for i, r in zip(idx, c_oracle.decode(prm, [dataclasses.replace(pics[i], size=None) for i in idx], threads=8)):
            res[i] = r
    return res


def sao_set(bit_depth, ctb_log2, lf_tiles, dbk=False):
    """[Picture] of the fixed set of one context (built once per process).  ``dbk``: with deblocking on, which
    must change nothing (asserted here with the C oracle, SAO off)."""
    key = (bit_depth, ctb_log2, int(lf_tiles), bool(dbk))
    if key in _SETS:
        return _SETS[key]
    if dbk:
        pics = [with_deblocking(p) for p in sao_set(bit_depth, ctb_log2, lf_tiles)]
        for pic, (rec, out) in zip(pics, c_decode(bit_depth, ctb_log2, lf_tiles, pics, sao=False)):
            for c in range(3):
                assert np.array_equal(rec[c], pic.planes[c]) and np.array_equal(out[c], pic.planes[c]), pic.meta
        _SETS[key] = pics
        return pics
    bd, k = bit_depth, (bit_depth, ctb_log2)
    pics = [_shared(k + ("edge", j), edge_picture, bd, ctb_log2, j) for j in range(N_EDGE)]
    pics += [_shared(k + ("band", j), band_picture, bd, ctb_log2, j) for j in range(n_band_pictures(ctb_log2))]
    pics.append(_shared(k + ("mix",), mix_picture, bd, ctb_log2))
    pics += [_shared(k + ("wide", j), wide_picture, bd, ctb_log2, j) for j in range(N_WIDE)]
    pics += [borders_picture(bd, ctb_log2, lf_tiles, li, rot) for li, rot in BORDER_PICTURES]
    pics += [_shared(k + ("nofilter", j), nofilter_picture, bd, ctb_log2, j) for j in range(N_NOFILTER)]
    pics += [strips_picture(bd, ctb_log2, lf_tiles, j) for j in range(N_STRIPS)]
    _SETS[key] = pics
    return pics


def py_sao(bd, ctb_log2, lf_tiles, pic, planes=None):
    """The Python oracle's SAO of the planted planes (the reconstruction; deblocking changes nothing)."""
    prm = R.params_dict(params_of(bd, ctb_log2, lf_tiles, *pic.size))
    return O.sao_picture(prm, pic.as_oracle_dict(), pic.planes if planes is None else planes)


_CHANGED = {}


def changed_floor(bd, ctb_log2, lf_tiles, pics=None):
    """Per component: in how many samples of the set (or of ``pics`` out of it) the Python oracle's SAO output
    differs from its input.  A decode changes as many; a comparison of untouched planes cannot pass for one."""
    n = [0, 0, 0]
    for pic in sao_set(bd, ctb_log2, lf_tiles) if pics is None else pics:
        key = (bd, ctb_log2, lf_tiles, repr(sorted(pic.meta.items())))
        if key not in _CHANGED:
            out = py_sao(bd, ctb_log2, lf_tiles, pic)
            _CHANGED[key] = [int((out[c] != pic.planes[c]).sum()) for c in range(3)]
        n = [a + b for a, b in zip(n, _CHANGED[key])]
    return n
