"""Scaled device-side output, the parts that need no device: the position rule (p265r_resize_position against the
restatement tests/resize_ref.py), the area weights and the division, the derived accuracy bound of the bilinear
filter, the float path (two separately rounded fp32 operations, F16 rounding), every refusal p265r_resize_layout
can see, and the Python surface (ExportSpec, plane_view, batch_array, the command line)."""
import ctypes
from fractions import Fraction

import numpy as np
import pytest

import export_ref as X
import resize_ref as RR
from p265_amd import _lib, dec, recon
from p265_amd import records as R

NS = (2, 8, 24, 40, 1920, 8192)
FILTER_ID = {"nearest": _lib.RS_NEAREST, "bilinear": _lib.RS_BILINEAR, "area": _lib.RS_AREA}

# fl32(fl32(v * scale) + bias) differs from the fused fl32(v * scale + bias) here (found by search on the CPU over the
# ImageNet-style normalisation scale = 1 / ((2^B - 1) std), bias = -mean / std, mean 0.485, std 0.229)
PINNED_F32 = (100, np.float32(0.017124753), np.float32(-2.117904))           # B = 8
# ... and at B = 12 these values also differ after the F16 rounding
PINNED_F16 = ((1986, 2642), np.float32(0.0010663766), np.float32(-2.117904))


def ms_of(n):
    return sorted({m for m in (1, 2, 3, 7, n - 1, n, n + 1, 2 * n, 16384) if 1 <= m <= 16384})


def c_positions(filt, n, m, hs, chroma, vertical):
    fn = _lib.load().p265r_resize_position
    i0, i1, f = ctypes.c_int32(), ctypes.c_int32(), ctypes.c_int32()
    r0, r1, rf = ctypes.byref(i0), ctypes.byref(i1), ctypes.byref(f)
    out = np.empty((len(hs), 3), np.int64)
    for k, h in enumerate(hs):
        assert fn(filt, n, m, int(h), chroma, vertical, r0, r1, rf) == _lib.OK
        out[k] = (i0.value, i1.value, f.value)
    return out


@pytest.mark.parametrize("n", NS)
def test_position_rule_equals_the_restatement_for_every_h(n):
    for m in ms_of(n):
        for chroma_grid in (False, True):
            if chroma_grid and m % 2:
                continue
            count = m // 2 if chroma_grid else m
            for vertical in (0, 1):
                hs = RR.grid_h(count, chroma_grid, bool(vertical))
                for chroma in (0, 1):
                    got = c_positions(_lib.RS_NEAREST, n, m, hs, chroma, vertical)
                    want = RR.nearest_index(n, m, hs, bool(chroma))
                    assert np.array_equal(got[:, 0], want) and np.array_equal(got[:, 1], want) and not got[:, 2].any()
                    got = c_positions(_lib.RS_BILINEAR, n, m, hs, chroma, vertical)
                    i0, i1, f = RR.bilinear_taps(n, m, hs, bool(chroma), bool(vertical))
                    assert np.array_equal(got[:, 0], i0) and np.array_equal(got[:, 1], i1) and np.array_equal(got[:, 2], f), \
                        (n, m, chroma_grid, vertical, chroma)
                    n_p = n // 2 if chroma else n
                    assert got[:, :2].min() >= 0 and got[:, :2].max() <= n_p - 1


def test_identity_and_clamps():
    for n in NS:
        hs = RR.grid_h(n, False, False)
        # nearest at m = n: the identity on luma, C[x >> 1] on chroma
        assert np.array_equal(RR.nearest_index(n, n, hs, False), np.arange(n))
        assert np.array_equal(RR.nearest_index(n, n, hs, True), np.arange(n) >> 1)
        assert np.array_equal(c_positions(_lib.RS_NEAREST, n, n, hs, 0, 0)[:, 0], np.arange(n))
        # bilinear at m = n: the sample itself, f = 0
        got = c_positions(_lib.RS_BILINEAR, n, n, hs, 0, 1)
        assert np.array_equal(got[:, 0], np.arange(n)) and not got[:, 2].any()
        # both clamps fire on upscale: the first output left of sample 0, the last right of sample n - 1
        m = 2 * n
        got = c_positions(_lib.RS_BILINEAR, n, m, RR.grid_h(m, False, False), 0, 0)
        assert tuple(got[0]) == (0, min(1, n - 1), 0)                  # pos = U - 32768 < 0, clamped to 0
        assert tuple(got[-1]) == (n - 1, n - 1, 0)                     # pos above (n - 1) << 16, clamped
        u = RR.u_of(RR.grid_h(m, False, False), n, m)
        assert u[0] - 32768 < 0 and u[-1] - 32768 > (n - 1) << 16


def host_plane(win, nw, nh, chroma_plane, chroma_grid, filt, mw, mh, norm=None):
    """p265r_resize_plane_host of a window (2-D array of the plane's own samples)."""
    src = np.ascontiguousarray(win, np.uint16)
    ow, oh = (mw // 2, mh // 2) if chroma_grid else (mw, mh)
    dst = np.empty((oh, ow), np.int32)
    if norm is None:
        rc = _lib.load().p265r_resize_plane_host(src.ctypes.data, src.shape[1], nw, nh, int(chroma_plane), int(chroma_grid),
                                                 FILTER_ID[filt], mw, mh, dst.ctypes.data, None, None, None)
        assert rc == _lib.OK, rc
        return dst
    nb = (ctypes.c_float * 2)(*norm)
    f32, f16 = np.empty((oh, ow), np.float32), np.empty((oh, ow), np.uint16)
    rc = _lib.load().p265r_resize_plane_host(src.ctypes.data, src.shape[1], nw, nh, int(chroma_plane), int(chroma_grid),
                                             FILTER_ID[filt], mw, mh, dst.ctypes.data, ctypes.addressof(nb), f32.ctypes.data,
                                             f16.ctypes.data)
    assert rc == _lib.OK, rc
    return dst, f32, f16.view(np.float16)


@pytest.mark.parametrize("filt", RR.FILTERS)
def test_host_reference_equals_the_restatement(filt):
    rng = np.random.default_rng(5)
    for (nw, nh), (mw, mh) in (((72, 40), (34, 18)), ((72, 40), (72, 40)), ((72, 40), (36, 20)), ((66, 26), (2, 2)),
                               ((72, 40), (100, 56)), ((24, 10), (32, 6)), ((130, 8), (16, 8)), ((2, 2), (2, 2))):
        if filt == "area" and (mw > nw or mh > nh):
            continue
        top = (255, 1023, 4095)[(nw + mw) % 3]
        for cp, cg in ((False, False), (True, False), (True, True)):
            ph, pw = (nh // 2, nw // 2) if cp else (nh, nw)
            win = rng.integers(0, top + 1, (ph, pw))
            got = host_plane(win, nw, nh, cp, cg, filt, mw, mh)
            assert np.array_equal(got, RR.resize_plane(win, nw, nh, cp, cg, filt, mw, mh)), (nw, nh, mw, mh, cp, cg)


def test_area_weights_constants_and_a_hand_worked_shrink():
    for n in NS:
        for m in ms_of(n):
            if m > n:
                continue
            for cp, cg in ((False, False), (True, False), (True, True)):
                if (cp and n % 2) or (cg and m % 2):
                    continue
                N, M = RR.box(n, m, cp, cg)
                outs, smp = (m // 2 if cg else m), (n // 2 if cp else n)
                if outs * smp > 40_000_000:
                    continue
                w = RR.area_weights(N, M, outs, smp)
                assert np.all(w.sum(axis=1) == N) and np.all(w.sum(axis=0) == M)       # every sample is used exactly once
    # a constant plane stays constant, at 0 and at the largest sample
    for top in (0, 255, 4095):
        for (nw, nh), (mw, mh) in (((72, 40), (34, 18)), ((72, 40), (31, 17)), ((8192, 2), (1, 1)), ((2, 8192), (2, 2))):
            for cp, cg in ((False, False), (True, False), (True, True)):
                if cg and (mw % 2 or mh % 2):
                    continue
                win = np.full((nh // 2, nw // 2) if cp else (nh, nw), top)
                assert (host_plane(win, nw, nh, cp, cg, "area", mw, mh) == top).all()
                assert (RR.resize_plane(win, nw, nh, cp, cg, "area", mw, mh) == top).all()
    # 2 : 1 is (a + b + c + d + 2) >> 2
    win = np.array([[1, 2, 10, 20], [3, 5, 30, 41], [255, 255, 0, 1], [255, 254, 1, 1]])
    want = np.array([[(1 + 2 + 3 + 5 + 2) >> 2, (10 + 20 + 30 + 41 + 2) >> 2], [(255 * 3 + 254 + 2) >> 2, (0 + 1 + 1 + 1 + 2) >> 2]])
    assert np.array_equal(host_plane(win, 4, 4, False, False, "area", 2, 2), want)
    assert np.array_equal(RR.resize_plane(win, 4, 4, False, False, "area", 2, 2), want)
    # 3 -> 2, hand-worked: output 0 = (2 a + b) / 3, output 1 = (b + 2 c) / 3, rounded; rows likewise
    win = np.array([[9, 0, 3]] * 3)
    assert np.array_equal(host_plane(win, 3, 3, False, False, "area", 2, 2), [[6, 2]] * 2)


def test_reciprocal_division_equals_floor_division():
    """Through the host reference: one output that covers the whole window is (sum + (d >> 1)) // d with d = nw nh.
    Windows whose sums sit at, just below and just above multiples of d, ends of the divisor range included
    (make resize-check runs the numerator exhaustively for small divisors and around every quotient for large ones)."""
    rng = np.random.default_rng(11)
    for nw, nh in ((1, 1), (1, 2), (3, 1), (3, 5), (7, 9), (17, 31), (64, 64), (1920, 2), (8192, 3), (5, 8192), (8191, 7)):
        d = nw * nh
        for top in (255, 4095):
            for _ in range(12):
                win = rng.integers(0, top + 1, (nh, nw))
                # steer the sum onto a rounding boundary: sum + d // 2 = q d + e, e in (-1, 0, 1)
                s = int(win.sum())
                for e in (-1, 0, 1):
                    q = (s + d // 2) // d
                    delta = q * d + e - d // 2 - s
                    w2 = win.copy().reshape(-1)
                    for k in range(w2.size):
                        if delta == 0:
                            break
                        step = int(np.clip(delta, -int(w2[k]), top - int(w2[k])))
                        w2[k] += step
                        delta -= step
                    w2 = w2.reshape(nh, nw)
                    got = host_plane(w2, nw, nh, False, False, "area", 1, 1)
                    assert int(got[0, 0]) == (int(w2.sum()) + d // 2) // d, (nw, nh, top, e)


def _window_with_sum(total, nw, nh, top):
    """A window of nw x nh samples in 0 .. top whose sum is ``total`` (filled greedily)."""
    full, rest = divmod(total, top) if top else (0, 0)
    w = np.zeros(nw * nh, np.int64)
    w[:full] = top
    if rest:
        w[full] = rest
    assert int(w.sum()) == total
    return w.reshape(nh, nw)


def test_reciprocal_division_exhaustive_for_small_divisors():
    """d = 1, 2, 3, 4, 6: EVERY reachable numerator 0 .. 4095 d through the host reference (one output over the whole
    window) equals the floor division."""
    for nw, nh in ((1, 1), (2, 1), (1, 3), (2, 2), (3, 2)):
        d = nw * nh
        for total in range(4095 * d + 1):
            got = host_plane(_window_with_sum(total, nw, nh, 4095), nw, nh, False, False, "area", 1, 1)
            if int(got[0, 0]) != (total + d // 2) // d:
                raise AssertionError((nw, nh, total, int(got[0, 0])))


def test_reciprocal_division_proof_conditions_and_range_ends():
    """The proof of resize_math.h restated in Python integers: rcp = ceil(2^64 / d) fits 64 bits for d > 1, 2^12 d^2 <=
    2^64 on the whole range d <= 2^26, and with them mulhi(x, rcp) = x // d for every x < 2^12 d -- checked at every
    quotient boundary for divisors at both ends of the range.  Then the C code at the upper end: 8192 x 8192 and 8191 x
    8192 windows (d = 2^26 and just below) with sums at the largest numerator and on rounding boundaries."""
    for d in (2, 3, 5, 255, 4096, (1 << 26) - 1, 1 << 26, 8191 * 8192, 8191 * 8191, 1920 * 1080):
        rcp = -((-1 << 64) // d)                                  # ceil(2^64 / d)
        assert rcp == ((1 << 64) - 1) // d + 1 and rcp < 1 << 64 and (1 << 12) * d * d <= 1 << 64
        for q in list(range(0, 40)) + list(range(4056, 4097)):
            for e in (-1, 0, 1):
                x = q * d + e
                if 0 <= x < (1 << 12) * d:
                    assert (x * rcp) >> 64 == x // d, (d, x)
    for nw, nh in ((8192, 8192), (8191, 8192)):
        d = nw * nh
        for total in (4095 * d, 4095 * d - d // 2 - 1, 4095 * d - d // 2, 2048 * d + d - d // 2 - 1, 2048 * d + d - d // 2,
                      d - d // 2 - 1, d - d // 2, 0):
            got = host_plane(_window_with_sum(total, nw, nh, 4095).astype(np.uint16), nw, nh, False, False, "area", 1, 1)
            assert int(got[0, 0]) == (total + d // 2) // d, (nw, nh, total)


@pytest.mark.parametrize("n", (8, 24, 40, 1920, 8192))
def test_bilinear_accuracy_bound_is_derived(n):
    """A ramp s[x] = x: the integer result against the float64 centre-aligned position (i + 0.5) n / m - 0.5, clamped to
    the plane: within 0.5 (the final rounding) + 1 / 256 (the 8-bit fraction) + m 2^-16 (the floor in step, accumulated
    over at most m outputs)."""
    ramp = np.arange(n)
    for m in ms_of(n):
        exact = np.clip((np.arange(m) + 0.5) * n / m - 0.5, 0, n - 1)
        bound = 0.5 + 1 / 256 + m * 2.0 ** -16
        for axis in (0, 1):
            win = np.tile(ramp, (2, 1)) if axis == 0 else np.tile(ramp[:, None], (1, 2))
            nw, nh, mw, mh = (n, 2, m, 2) if axis == 0 else (2, n, 2, m)
            got = host_plane(win, nw, nh, False, False, "bilinear", mw, mh)
            line = got[0, :] if axis == 0 else got[:, 0]
            err = np.abs(line - exact).max()
            assert err <= bound, (n, m, axis, err, bound)
            ref = RR.resize_plane(win, nw, nh, False, False, "bilinear", mw, mh)
            assert np.array_equal(got, ref)


def _exact_f32(fr):
    """A Fraction rounded once to float32 (nearest, ties to even)."""
    f = np.float32(float(fr))
    cands = [f, np.nextafter(f, np.float32(np.inf)), np.nextafter(f, np.float32(-np.inf))]
    return min(cands, key=lambda x: (abs(Fraction(float(x)) - fr), int(np.float32(x).view(np.uint32)) & 1))


def test_float_path_is_two_rounded_operations():
    # ImageNet-style normalisation at 8 and 12 bits over every value: numpy float32 multiply, then add
    for B, (mean, std) in ((8, (0.485, 0.229)), (12, (0.406, 0.225))):
        scale, bias = np.float32(1 / ((2 ** B - 1) * std)), np.float32(-mean / std)
        v = np.arange(2 ** B).reshape(2 ** (B - 4), 16)
        got, f32, f16 = host_plane(v, 16, 2 ** (B - 4), False, False, "nearest", 16, 2 ** (B - 4), norm=(scale, bias))
        assert np.array_equal(got, v)
        want = v.astype(np.float32) * scale + bias
        assert want.dtype == np.float32 and np.array_equal(f32, want)
        assert np.array_equal(f16.view(np.uint16), want.astype(np.float16).view(np.uint16))
        assert np.array_equal(f32, RR.float_out(v, scale, bias, np.float32))
    # the pinned triples: unfused differs from the single rounding of the exact v * scale + bias, and the host gives
    # the unfused one
    v, scale, bias = PINNED_F32
    unfused = np.float32(np.float32(v) * scale) + bias
    fused = _exact_f32(Fraction(v) * Fraction(float(scale)) + Fraction(float(bias)))
    assert unfused != fused
    _, f32, _ = host_plane(np.full((2, 2), v), 2, 2, False, False, "nearest", 2, 2, norm=(scale, bias))
    assert (f32 == unfused).all() and (f32 != fused).all()
    vs, scale, bias = PINNED_F16
    for v in vs:
        unfused = np.float32(np.float32(v) * scale) + bias
        fused = _exact_f32(Fraction(v) * Fraction(float(scale)) + Fraction(float(bias)))
        assert np.float16(unfused) != np.float16(fused)
        _, _, f16 = host_plane(np.full((2, 2), v), 2, 2, False, False, "nearest", 2, 2, norm=(scale, bias))
        assert (f16 == np.float16(unfused)).all()
    # the default scale reproduces the plain export's float value
    for B in (8, 10, 12):
        v = np.arange(2 ** B).reshape(-1, 16)
        k = np.float32(1 / (2 ** B - 1))
        _, f32, f16 = host_plane(v, 16, v.shape[0], False, False, "nearest", 16, v.shape[0], norm=(k, 0.0))
        assert np.array_equal(f32, v.astype(np.float32) * k)
        assert np.array_equal(f16.view(np.uint16), (v.astype(np.float32) * k).astype(np.float16).view(np.uint16))
    # F16 rounding over a dense sweep: ties, subnormals, overflow
    v = np.arange(4096).reshape(-1, 16)
    for scale, bias in ((2.0 ** -11, 0.0), (2.0 ** -24, 0.0), (2.0 ** -25, 2.0 ** -26), (16.0, 0.5), (1.0, 2.0 ** -12), (17.0, 0.0)):
        _, f32, f16 = host_plane(v, 16, v.shape[0], False, False, "nearest", 16, v.shape[0], norm=(scale, bias))
        with np.errstate(over="ignore"):
            want = (v.astype(np.float32) * np.float32(scale) + np.float32(bias)).astype(np.float16)
        assert np.array_equal(f16.view(np.uint16), want.view(np.uint16)), (scale, bias)


def _layout_rc(bd=8, mono=False, align=1, size=(34, 18), filt=_lib.RS_BILINEAR, flags=0, scale=(1, 1, 1), bias=(0, 0, 0), **fields):
    pc = recon._params_c(R.make_params(pic_width=72, pic_height=40, bit_depth_luma=bd, bit_depth_chroma=bd,
                                       chroma_format_idc=0 if mono else 1))
    d = _lib.ExportDesc()
    for k, v in fields.items():
        setattr(d, k, v)
    rs = _lib.ResizeDesc()
    rs.out_width, rs.out_height, rs.filter, rs.flags = size[0], size[1], filt, flags
    for c in range(3):
        rs.scale[c], rs.bias[c] = scale[c], bias[c]
    return _lib.load().p265r_resize_layout(ctypes.byref(pc), ctypes.byref(d), ctypes.byref(rs), align), d


def test_every_refusal_of_the_layout_call():
    rgb = dict(format=_lib.FMT_RGB_PLANAR, sample=_lib.SMP_F32)
    assert _layout_rc()[0] == _lib.OK and _layout_rc(**rgb)[0] == _lib.OK
    assert _layout_rc(filt=3)[0] == _lib.EINVAL
    assert _layout_rc(flags=2)[0] == _lib.EINVAL and _layout_rc(flags=3, **rgb)[0] == _lib.EINVAL
    for size in ((0, 18), (34, 0), (16386, 18), (34, 16386)):
        assert _layout_rc(size=size)[0] == _lib.EINVAL, size
    assert _layout_rc(size=(16384, 16384))[0] == _lib.OK
    # an odd size where the format has half-size chroma
    for fmt in (_lib.FMT_PLANAR, _lib.FMT_SEMIPLANAR):
        assert _layout_rc(format=fmt, size=(33, 18))[0] == _lib.EINVAL and _layout_rc(format=fmt, size=(34, 17))[0] == _lib.EINVAL
    for fmt in (_lib.FMT_RGB_PLANAR, _lib.FMT_RGB_PACKED):
        assert _layout_rc(format=fmt, size=(31, 17))[0] == _lib.OK
    assert _layout_rc(mono=True, format=_lib.FMT_PLANAR, size=(31, 17))[0] == _lib.OK
    assert _layout_rc(mono=True, format=_lib.FMT_SEMIPLANAR, size=(31, 18))[0] == _lib.EINVAL
    assert _layout_rc(mono=True, format=_lib.FMT_SEMIPLANAR, size=(32, 18))[0] == _lib.OK
    # NORM needs a float sample and finite values
    assert _layout_rc(flags=_lib.RS_NORM, **rgb)[0] == _lib.OK
    assert _layout_rc(flags=_lib.RS_NORM, format=_lib.FMT_RGB_PACKED, sample=_lib.SMP_F16)[0] == _lib.OK
    for smp in (_lib.SMP_NATIVE, _lib.SMP_U8):
        assert _layout_rc(flags=_lib.RS_NORM, format=_lib.FMT_RGB_PLANAR, sample=smp)[0] == _lib.EINVAL
    assert _layout_rc(flags=_lib.RS_NORM)[0] == _lib.EINVAL                                  # planar, native
    for bad in (float("inf"), float("-inf"), float("nan")):
        assert _layout_rc(flags=_lib.RS_NORM, scale=(1, bad, 1), **rgb)[0] == _lib.EINVAL
        assert _layout_rc(flags=_lib.RS_NORM, bias=(0, 0, bad), **rgb)[0] == _lib.EINVAL
        assert _layout_rc(scale=(1, bad, 1), **rgb)[0] == _lib.OK                            # not used without the flag
    # the export descriptor's own rules still hold; upsample is ignored
    assert _layout_rc(format=4)[0] == _lib.EINVAL and _layout_rc(sample=_lib.SMP_F16)[0] == _lib.EINVAL
    assert _layout_rc(sample=_lib.SMP_MSB16)[0] == _lib.EINVAL and _layout_rc(bd=10, sample=_lib.SMP_MSB16)[0] == _lib.OK
    assert _layout_rc(crop_left=1)[0] == _lib.EINVAL and _layout_rc(matrix=3, **rgb)[0] == _lib.EINVAL
    assert _layout_rc(upsample=9, **rgb)[0] == _lib.OK
    assert _layout_rc(align=3, bd=10)[0] == _lib.EINVAL and _layout_rc(align=(1 << 20) + 1)[0] == _lib.EINVAL
    lib = _lib.load()
    pc, d, rs = recon._params_c(R.make_params()), _lib.ExportDesc(), _lib.ResizeDesc()
    assert lib.p265r_resize_layout(None, ctypes.byref(d), ctypes.byref(rs), 1) == _lib.EINVAL
    assert lib.p265r_resize_layout(ctypes.byref(pc), None, ctypes.byref(rs), 1) == _lib.EINVAL
    assert lib.p265r_resize_layout(ctypes.byref(pc), ctypes.byref(d), None, 1) == _lib.EINVAL


def _planes(fmt, es, w, h, mono=False):
    if mono and fmt == "planar":
        return [(w * es, h)]
    return {"planar": [(w * es, h), (w // 2 * es, h // 2), (w // 2 * es, h // 2)], "semiplanar": [(w * es, h), (w * es, h // 2)],
            "rgb_planar": [(w * es, h)] * 3, "rgb_packed": [(3 * w * es, h)]}[fmt]


@pytest.mark.parametrize("bd", [8, 10])
def test_layout_does_not_depend_on_the_picture(bd):
    for mono in (False, True):
        params = R.make_params(pic_width=72, pic_height=40, bit_depth_luma=bd, bit_depth_chroma=bd, chroma_format_idc=0 if mono else 1)
        for fmt, sample in (("planar", "native"), ("semiplanar", "native"), ("rgb_planar", "f16"), ("rgb_packed", "u8"),
                            ("rgb_planar", "f32"), ("rgb_packed", "native")):
            es = np.dtype(X.sample_dtype(sample, bd)).itemsize
            for align in (1, 256):
                spec = recon.ExportSpec(format=fmt, sample=sample, crop=(2, 4, 2, 6), pitch_align=align, size=(34, 18), resize="area")
                lay = recon.export_layout(params, spec)
                up = lambda v: (v + align - 1) // align * align
                off, planes = 0, _planes(fmt, es, 34, 18, mono)
                assert lay.n_planes == len(planes) and lay.size == (34, 18)
                for k, (row, rows) in enumerate(planes):
                    assert lay.plane_off[k] == off and lay.pitch[k] == up(row), (fmt, sample, align, k)
                    off = up(off + up(row) * rows)
                assert lay.frame_bytes == off
                lay2 = recon.export_layout(params, spec, (24, 16))
                assert (lay2.plane_off, lay2.pitch, lay2.frame_bytes) == (lay.plane_off, lay.pitch, lay.frame_bytes)
                # plane_view: the output shape, whatever the picture's size
                for size in ((72, 40), (24, 16)):
                    shape0, strides0 = lay.plane_view(0, size)
                    assert shape0 == ((18, 34, 3) if fmt == "rgb_packed" else (18, 34))
                    assert strides0[0] == lay.pitch[0]
                    if fmt == "semiplanar":
                        assert lay.plane_view(1, size) == ((9, 17, 2), (lay.pitch[1], 2 * es, es))
                    if fmt == "planar" and not mono:
                        assert lay.plane_view(2, size) == ((9, 17), (lay.pitch[2], es))


def test_export_spec_fields_and_descriptors():
    s = recon.ExportSpec()
    assert (s.size, s.resize, s.scale, s.bias) == (None, "bilinear", None, None)           # appended, today's behaviour
    assert recon.ExportSpec("planar", "native", "bt709", False, "nearest", (0, 0, 0, 0), 1) == s
    with pytest.raises(ValueError):
        s.resize_desc()
    r = recon.ExportSpec(size=(224, 200)).resize_desc()
    assert (r.out_width, r.out_height, r.filter, r.flags) == (224, 200, _lib.RS_BILINEAR, 0)
    r = recon.ExportSpec.named("rgb-planar-f16", size=(224, 224), resize="area", scale=(2, 3, 4), bias=(-1, -2, -3)).resize_desc()
    assert r.filter == _lib.RS_AREA and r.flags == _lib.RS_NORM and list(r.scale) == [2, 3, 4] and list(r.bias) == [-1, -2, -3]
    r = recon.ExportSpec(size=(8, 8), resize=_lib.RS_NEAREST, bias=(1, 1, 1)).resize_desc()
    assert r.filter == _lib.RS_NEAREST and r.flags == _lib.RS_NORM and list(r.scale) == [1, 1, 1]
    with pytest.raises(ValueError):
        recon.ExportSpec(size=(8, 8), resize="cubic").resize_desc()
    with pytest.raises(ValueError):
        recon.ExportSpec(size=(8, 8), scale=(1, 2)).resize_desc()
    params = R.make_params(pic_width=72, pic_height=40)
    with pytest.raises(_lib.P265RError):
        recon.export_layout(params, recon.ExportSpec(size=(33, 18)))                        # planar, odd
    with pytest.raises(_lib.P265RError):
        recon.export_layout(params, recon.ExportSpec(size=(34, 18), scale=(1, 1, 1)))       # NORM on integers
    # without a size nothing changes: the plain layout call
    lay = recon.export_layout(params, recon.ExportSpec(format="rgb_packed", sample="u8"))
    assert lay.size is None and lay.resize is None and lay.plane_view(0, (72, 40))[0] == (40, 72, 3)


def _frames(params, spec, sizes, ptr=0x10000):
    lay = recon.export_layout(params, spec)
    return recon.DeviceFrames(ptr, lay.frame_bytes * len(sizes), lay, sizes)


def test_batch_array_shapes_strides_and_errors():
    params = R.make_params(pic_width=72, pic_height=40, bit_depth_luma=10, bit_depth_chroma=10)
    ragged = [(72, 40), (24, 16), (40, 40)]
    fr = _frames(params, recon.ExportSpec(format="rgb_planar", sample="f16", size=(34, 18), pitch_align=256), ragged)
    a = fr.batch_array().__cuda_array_interface__
    lay = fr.layout
    assert a["shape"] == (3, 3, 18, 34) and a["typestr"] == "<f2" and a["data"] == (0x10000, False)
    assert a["strides"] == (lay.frame_bytes, lay.plane_off[1] - lay.plane_off[0], 256, 2) and lay.frame_bytes == 3 * 18 * 256
    fr = _frames(params, recon.ExportSpec(format="rgb_packed", sample="u8", size=(31, 17)), ragged)
    a = fr.batch_array().__cuda_array_interface__
    assert a["shape"] == (3, 17, 31, 3) and a["strides"] == (17 * 93, 93, 3, 1) and a["typestr"] == "|u1"
    fr = _frames(params, recon.ExportSpec(format="semiplanar", sample="msb16", size=(34, 18)), ragged)
    assert fr.batch_array(0).__cuda_array_interface__["shape"] == (3, 18, 34)
    a = fr.batch_array(1).__cuda_array_interface__
    assert a["shape"] == (3, 9, 17, 2) and a["strides"] == (fr.layout.frame_bytes, 68, 4, 2)
    assert a["data"][0] == 0x10000 + fr.layout.plane_off[1]
    fr = _frames(params, recon.ExportSpec(format="planar", size=(34, 18)), ragged)
    assert fr.batch_array(2).__cuda_array_interface__["shape"] == (3, 9, 17)
    with pytest.raises(IndexError):
        fr.batch_array(3)
    # a plain export of one size is one array too; a ragged one is not
    fr = _frames(params, recon.ExportSpec(format="rgb_planar", sample="f32"), [(72, 40)] * 2)
    assert fr.batch_array().__cuda_array_interface__["shape"] == (2, 3, 40, 72)
    with pytest.raises(ValueError):
        _frames(params, recon.ExportSpec(format="rgb_planar", sample="f32"), ragged).batch_array()
    # R, G, B planes that are not evenly spaced
    fr = _frames(params, recon.ExportSpec(format="rgb_planar", sample="f32", size=(34, 18)), ragged)
    fr.layout.plane_off[2] += 4
    with pytest.raises(ValueError):
        fr.batch_array()
    with pytest.raises(IndexError):
        _frames(params, recon.ExportSpec(format="rgb_planar", sample="f32", size=(34, 18)), ragged).batch_array(1)


def test_command_line_options(capsys):
    a = dec.parse_cmd(["-b", "x.bin", "--format", "rgb-planar-f16", "--resize", "224x200", "--resize-filter", "area"])
    s = dec.export_spec(a)
    assert s.size == (224, 200) and s.resize == "area" and s.format == "rgb_planar" and s.sample == "f16"
    s = dec.export_spec(dec.parse_cmd(["-b", "x.bin", "--format", "nv12", "--resize", "960X540"]))
    assert s.size == (960, 540) and s.resize == "bilinear"
    assert dec.export_spec(dec.parse_cmd(["-b", "x.bin", "--format", "nv12"])).size is None
    assert dec.export_spec(dec.parse_cmd(["-b", "x.bin"])) is None
    for argv in (["--resize", "224x224"], ["--resize-filter", "area"], ["--format", "i420", "--resize", "8x8"],
                 ["--format", "nv12", "--resize-filter", "area"], ["--format", "nv12", "--resize", "224"],
                 ["--format", "nv12", "--resize", "axb"]):
        with pytest.raises(SystemExit):
            dec.parse_cmd(["-b", "x.bin"] + argv)
        assert "--resize" in capsys.readouterr().err
