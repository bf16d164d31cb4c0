"""The depthwise yardstick (tests/_dw.py) checked on the CPU: the float64 statements against F.pad + F.conv2d(groups = C) + autograd, the
float32 models within the derived bounds of float64, the exact fma against rationals, the one-hot expectation, the dispatch statement, and
mutants of the model that must each break the check meant to catch them.  What tests/test_dw_abi_gpu.py holds the kernels to is therefore
a model that is itself pinned.

Mutant factors (deterministic; worst error / bound of the mutant over the cases below, the smallest over the mutant's cases; each test
asserts a tenth of it):
    taps transposed 2.86e7        dgrad without the rotation 4.29e7        pad off by one at dilation 2 6.69e16
    stride-2 column parity swapped 9.14e20        last odd column dropped 4.19e6        statistics of the unrounded values 67.4
(the inputs span 45 binades, so a misplaced tap puts a large value where the bound expects a small one: hence the size of the factors)
The rounding mutants (8 in the bound, truncation, the accumulate term re-scaled with the new scale) are judged by bits.
"""
from fractions import Fraction

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from tests import _dw as D
from tests import _planes as P

CASES = D.F32_CASES + D.HALF_CASES


def _ids(c):
    return 'x'.join(map(str, c))


def _worst(got, ref, bound, strict=True):
    err = np.abs(np.asarray(got, dtype=np.float64) - ref)
    live = bound > 0
    assert not strict or (err[~live] == 0).all()          # a mutant is judged on the elements that have a bound
    return float((err[live] / bound[live]).max()) if live.any() else 0.0


def _inputs(case, seed=0):
    B, H, W, C, s, dl = case
    d = D.Desc(*case)
    x, _ = D.wide(seed + 1, (B, H, W, C))
    dy, _ = D.wide(seed + 2, (B, d.OH, d.OW, C), mag=2.0 ** -8)
    w, wa = D.filt(seed + 3, C)
    return d, x, dy, w, wa


@pytest.mark.parametrize('case', CASES, ids=_ids)
def test_fp64_statements_against_torch(case):
    d, x, dy, w, _ = _inputs(case)
    x64 = torch.from_numpy(x.astype(np.float64)).permute(0, 3, 1, 2).clone().requires_grad_(True)
    w64 = torch.from_numpy(w.astype(np.float64)).view(d.C, 1, 3, 3).clone().requires_grad_(True)
    y = F.conv2d(F.pad(x64, (d.dil,) * 4), w64, stride=d.stride, dilation=d.dil, groups=d.C)
    assert tuple(y.shape[2:]) == (d.OH, d.OW)
    dx, dw = torch.autograd.grad(y, (x64, w64), torch.from_numpy(dy.astype(np.float64)).permute(0, 3, 1, 2))
    for name, mine, ref in (('y', D.fwd64(x, w, d.stride, d.dil), y.detach().permute(0, 2, 3, 1).numpy()),
                            ('dx', D.dgrad64(dy, w, d.H, d.W, d.stride, d.dil), dx.permute(0, 2, 3, 1).numpy()),
                            ('dw', D.wgrad64(x, dy, d.stride, d.dil), dw.view(d.C, 9).numpy())):
        mag = {'y': D.conv64(D.fwd_terms(x, d.stride, d.dil), w, True), 'dx': D.conv64(D.dgrad_terms(dy, d.H, d.W, d.stride, d.dil), w, True),
               'dw': D.wgrad64(x, dy, d.stride, d.dil, True)}[name]
        assert (np.abs(mine - ref) <= 64 * 2.0 ** -53 * mag).all(), name           # two float64 sums of the same terms in different orders
    old, _ = D.wide(9, x.shape)
    keep = np.random.RandomState(3).rand(*x.shape) > 0.4
    full = D.dgrad64(dy, w, d.H, d.W, d.stride, d.dil, old, old, keep)
    assert np.array_equal(full, D.dgrad64(dy, w, d.H, d.W, d.stride, d.dil) + old.astype(np.float64) + np.where(keep, old.astype(np.float64), 0.0))


def test_fma32_is_exact():
    r = np.random.RandomState(0)
    n = 3000
    a = (r.standard_normal(n) * 2.0 ** r.randint(-20, 20, n)).astype(np.float32)
    b = (r.standard_normal(n) * 2.0 ** r.randint(-10, 10, n)).astype(np.float16).astype(np.float32)
    c = (-a * b * (1 + r.standard_normal(n) * 2.0 ** r.randint(-30, 2, n))).astype(np.float32)          # cancellation at every distance
    c[::7] = (r.standard_normal(n) * 2.0 ** r.randint(-40, 40, n)).astype(np.float32)[::7]
    got = D.fma32(a, b, c)
    for i in range(n):
        exact = Fraction(float(a[i])) * Fraction(float(b[i])) + Fraction(float(c[i]))
        lo = np.float32(float(exact))                        # Python rounds a Fraction to float64 correctly; float32 candidates around it
        cands = [np.nextafter(lo, np.float32(-np.inf)), lo, np.nextafter(lo, np.float32(np.inf))]
        best = min(cands, key=lambda v: (abs(Fraction(float(v)) - exact), int(np.float32(v).view(np.uint32)) & 1))
        assert got[i] == best, (i, a[i], b[i], c[i], got[i], best)


@pytest.mark.parametrize('case', CASES, ids=_ids)
def test_models_lie_within_the_bounds(case):
    d, x, dy, w, wa = _inputs(case)
    worst = {}
    e = D.expect_fwd(x, w, d)
    worst['fwd'] = _worst(e.out, e.ref, e.bound)
    old, _ = D.wide(9, x.shape)
    for name, o in (('dgrad', None), ('dgrad+', old)):
        e = D.expect_dgrad(dy, w, d, o)
        worst[name] = _worst(e.out, e.ref, e.bound)
    smallest = [np.abs(e.out[e.out != 0]).min()]
    for mult in (1.0, 128.0):
        xh, dyh = D.wide_half(1, x.shape, mult=mult), D.wide_half(2, dy.shape, 2.0 ** -8, mult)
        oldh = D.wide_half(9, x.shape, 2.0 ** -6)
        for path in ('strip', 'tile') if (d.stride, d.dil) == (1, 1) else ('tileg',):
            e = D.expect_fwd_h(xh, w, wa, d, path)
            assert float(np.abs(e.ref).max()) <= float(P.float_of(e.bits))
            for bits in (xh.bits, dyh.bits, oldh.bits, e.bits):
                assert 2.0 ** -40 <= float(P.float_of(bits)) <= 2.0 ** 20          # the window in which the reference meets no fp32 subnormal
            worst['fwd_h %s x%g' % (path, mult)] = _worst(e.out.astype(np.float64) / float(e.s), e.ref, e.bound)
            for name, kw in (('', {}), ('+h', dict(old=oldh)), ('+f', dict(old=old, half_out=False)), ('f', dict(half_out=False))):
                e = D.expect_dgrad_h(dyh, w, wa, d, path, **kw)
                got = e.out.astype(np.float64) / (float(e.s) if e.s is not None else 1.0)
                worst['dgrad_h%s %s x%g' % (name, path, mult)] = _worst(got, e.ref, e.bound)
                if e.s is None:
                    smallest.append(np.abs(e.out[e.out != 0]).min())
    assert min(smallest) >= 2.0 ** -126, 'an fp32 subnormal in the reference itself'
    top = max(worst, key=worst.get)
    print('%s: worst model / bound %.3f (%s)' % (_ids(case), worst[top], top))
    assert worst[top] <= 1.0, worst


@pytest.mark.parametrize('val', [1.0, 1.5])
def test_one_hot_expectation(val):
    """Tap value 1.0: the fp32 model returns the shifted input bit for bit; on halves the model equals the single rounding of the exactly
    known value, ties included (1.5 x an odd half)."""
    case = (1, 9, 17, 8, 1, 1)
    d, x, _, _, _ = _inputs(case)
    xh = D.wide_half(1, x.shape)
    ties = 0
    for tap in range(9):
        w, wa = D.one_hot(d.C, tap, val)
        shifted = D.fwd_terms(x, 1, 1)[tap][0]
        if val == 1.0:
            assert np.array_equal(D.canon32(D.expect_fwd(x, w, d).out).view(np.uint32), D.canon32(shifted).view(np.uint32))
        for path in ('strip', 'tile'):
            e = D.expect_fwd_h(xh, w, wa, d, path)
            exact = D.fwd_terms(xh.h, 1, 1)[tap][0].astype(np.float64) * val * (float(e.s) / float(xh.s))
            assert np.array_equal(P.canon(e.out.view(np.uint16)), P.canon(exact.astype(np.float16).view(np.uint16)))
            m = np.abs(exact) * 2.0 ** 24                    # in units of the subnormal spacing: integers and halves
            ulp = np.maximum(2.0 ** np.floor(np.log2(np.maximum(m, 1.0))) * 2.0 ** -10, 1.0)
            ties += int((np.mod(m / ulp, 1.0) == 0.5).sum())
    print('one-hot %.1f: %d exact ties among the expected halves' % (val, ties))
    assert ties > 50


def test_dispatch_statement():
    """The path property each GPU case exists for."""
    path = {c: D.half_path(D.Desc(*c)) for c in D.HALF_CASES + [D.HALF_BIG]}
    assert [path[c] for c in D.HALF_CASES] == ['tile', 'tile', 'tile', 'strip', 'tile', 'tileg', 'tileg', 'tileg', 'tileg', 'tileg']
    assert [D.half_path(D.Desc(*c), 0) for c in D.HALF_CASES] == ['strip'] * 4 + [None] * 6
    assert [D.f32_path(D.Desc(*c)) for c in D.F32_CASES] == ['strip'] * 5 + ['general'] * 7
    assert D.make_tiles(D.Desc(*D.HALF_CASES[0])).n_tiles == 1 and D.make_tiles(D.Desc(*D.HALF_CASES[1])).n_tiles == 4
    t = D.make_tiles(D.Desc(*D.HALF_CASES[2]))
    assert t.chunks == 2 and 136 - D.CHUNK == 8
    t = D.make_tiles(D.Desc(*D.HALF_BIG))
    assert (t.n_tiles, t.groups) == (1056, 1024)
    big = D.Desc(*D.F32_SPB2)
    g = D.make_slab(big.B * big.H * big.W, big.C)
    st = D.make_strips(big, g)
    assert (g.cols, g.RL, g.nslab) == (256, 1, 428) and (st.n_strips, st.strips_per_block, st.blocks) == (1026, 2, 513)
    assert D.depths(big, 'strip', 2) == (513, 2 * 2 * st.seg, 0)
    assert D.make_strips(D.Desc(2, 66, 130, 1024), D.make_slab(2 * 66 * 130, 1024)).strips_per_block == 2          # the 67 MB shape it stands for
    ws = D.Desc(*D.WS_CASE)
    assert D.depths(ws, 'strip', 2)[0] == 4 and D.make_slab(ws.B * ws.H * ws.W, ws.C).nslab == 2
    g = D.make_slab(2 * 9 * 70, 20)
    s = D.make_strips(D.Desc(2, 9, 70, 20), g)
    assert g.CV == 5 and s.nseg > 1 and s.nseg * s.seg > 70                                        # ragged segments, odd vector count
    assert D.make_slab(24, 1028).cols == 256 and 1028 // 4 - 256 == 1                              # one live column in the second pass
    assert not D.half_ok(D.Desc(2, 7, 9, 16, 2, 1)) and not D.half_ok(D.Desc(1, 8, 16, 8, 1, 1, 12, 8)) and not D.half_ok(D.Desc(1, 9, 1, 8), 0)
    assert D.half_ok(D.Desc(1, 9, 1, 8)) and D.half_ok(D.Desc(1, 5, 6, 12)) and not D.bn_ok(D.Desc(1, 5, 6, 12))


# ---- mutants ---------------------------------------------------------------------------------------------------------------------------------------
def _mutant_factor(name, cases, make):
    """make(d, x, dy, w) -> (mutant output, ref, bound); the smallest worst-ratio over the cases."""
    f = []
    for c in cases:
        d, x, dy, w, _ = _inputs(c)
        f.append(_worst(*make(d, x, dy, w), strict=False))
    print('mutant %-34s smallest factor over the bound %.3g' % (name, min(f)))
    return min(f)


S1 = [(2, 5, 7, 8, 1, 1), (1, 9, 17, 8, 1, 1)]


def test_mutant_taps_transposed():
    def make(d, x, dy, w):
        e = D.expect_fwd(x, w, d)
        return D.chain32(D.fwd_terms(x, d.stride, d.dil), w.transpose(0, 2, 1)), e.ref, e.bound
    assert _mutant_factor('taps transposed', S1 + [(1, 9, 10, 24, 1, 2)], make) > 2.86e6


def test_mutant_dgrad_without_rotation():
    def make(d, x, dy, w):
        e = D.expect_dgrad(dy, w, d)
        return D.chain32(D.dgrad_terms(dy, d.H, d.W, d.stride, d.dil), w[:, ::-1, ::-1]), e.ref, e.bound
    assert _mutant_factor('dgrad without the rotation', S1 + [(2, 8, 10, 16, 2, 1)], make) > 4.29e6


def test_mutant_pad_off_by_one_at_dilation_2():
    def make(d, x, dy, w):
        e = D.expect_fwd(x, w, d)
        return D.chain32(D.fwd_terms(x, d.stride, d.dil, pad=d.dil - 1), w), e.ref, e.bound
    assert _mutant_factor('pad off by one at dilation 2', [(1, 9, 10, 24, 1, 2), (1, 8, 16, 8, 1, 2)], make) > 6.69e15


def test_mutant_stride2_parity_swapped():
    def make(d, x, dy, w):
        e = D.expect_dgrad(dy, w, d)
        return D.chain32(D.dgrad_terms(dy, d.H, d.W, d.stride, d.dil, wshift=1), w), e.ref, e.bound
    assert _mutant_factor('stride-2 column parity swapped', [(2, 8, 10, 16, 2, 1), (1, 8, 32, 8, 2, 1)], make) > 9.14e19


def test_mutant_last_odd_column_dropped():
    def make(d, x, dy, w):
        e = D.expect_fwd(x, w, d)
        y = e.out.copy()
        y[:, :, -1] = 0
        return y, e.ref, e.bound
    assert _mutant_factor('last odd column dropped', [(1, 9, 17, 8, 1, 1), (2, 19, 37, 136, 1, 1)], make) > 4.19e5


def test_mutant_statistics_of_the_unrounded_values():
    f = []
    for c in [(1, 9, 17, 8, 1, 1), (2, 19, 37, 136, 1, 1), (1, 5, 6, 12, 1, 1)]:
        d, x, _, w, wa = _inputs(c)
        xh = D.wide_half(1, x.shape)
        path = D.half_path(d)
        e = D.expect_fwd_h(xh, w, wa, d, path)
        stored = e.out.astype(np.float64) / float(e.s)
        b1, b2 = D.stats_bound(stored, d, path)
        s1, s2, _ = D.stats64(stored)
        u1, u2, _ = D.stats64(e.ref)
        f.append(max(_worst(u1, s1, b1), _worst(u2, s2, b2)))
    print('mutant %-34s smallest factor over the bound %.3g' % ('statistics of the unrounded values', min(f)))
    assert min(f) > 6.74


def test_rounding_mutants_break_the_bit_comparison():
    d, x, dy, w, wa = _inputs((1, 9, 17, 8, 1, 1))
    xh, dyh = D.wide_half(1, x.shape), D.wide_half(2, dy.shape, 2.0 ** -8)
    for path in ('strip', 'tile'):
        e = D.expect_fwd_h(xh, w, wa, d, path)
        # 8 instead of 9: other bits of the bound (and, here, another scale)
        assert D.expect_fwd_h(xh, w, wa, d, path, nine=8.0).bits != e.bits
        # truncation: other halves on random data, and on every tie of the 1.5 tap that rounds away from zero
        t = D.expect_fwd_h(xh, w, wa, d, path, cvt=D.rz16)
        assert (P.canon(t.out.view(np.uint16)) != P.canon(e.out.view(np.uint16))).mean() > 0.2
        w15, wa15 = D.one_hot(d.C, 4, 1.5)
        a, b = D.expect_fwd_h(xh, w15, wa15, d, path), D.expect_fwd_h(xh, w15, wa15, d, path, cvt=D.rz16)
        assert (P.canon(a.out.view(np.uint16)) != P.canon(b.out.view(np.uint16))).sum() > 20
        # the accumulate term re-scaled with the new scale instead of its own: off by the ratio of the scales
        for mag in (2.0 ** -16, 2.0 ** -10):
            oldh = D.wide_half(9, x.shape, mag)
            good, bad = D.expect_dgrad_h(dyh, w, wa, d, path, old=oldh), D.expect_dgrad_h(dyh, w, wa, d, path, old=oldh, rescale_bug=True)
            assert good.s != oldh.s
            assert (P.canon(good.out.view(np.uint16)) != P.canon(bad.out.view(np.uint16))).mean() > 0.2
