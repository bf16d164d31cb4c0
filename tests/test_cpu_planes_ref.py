"""The fp16-plane yardstick (tests/_planes.py) checked on the CPU against float64: the model meets the bounds it derives, both branches of
each bound carry a real share of the data, the planted edges are where they are meant to be, the address map and the filter layouts agree
with plain loops.  What tests/test_planes_abi_gpu.py holds the kernels to bit for bit is therefore a model that is itself pinned."""
import numpy as np
import pytest

from tests import _planes as P

MULTS = (1.0, 2.0, 32.0, 4096.0)          # range scalars: the maximum and 2^1, 2^5, 2^12 x it


def _inputs():
    for seed, (m, c) in enumerate([(37, 72), (1031, 32), (64, 96)]):
        for mult in MULTS:
            x, bits = P.plant(P.wide(seed, m, c), mult)
            yield 'wide%d x%g' % (seed, mult), x, bits


@pytest.mark.parametrize('name,x,bits', list(_inputs()), ids=lambda v: v if isinstance(v, str) else '')
def test_model_meets_its_bounds(name, x, bits):
    s = P.scale_for(bits)
    amax = float(np.abs(x).max())
    assert P.float_of(bits) >= amax and 2.0 ** 14 <= float(P.float_of(bits)) * float(s) < 2.0 ** 15
    x64 = x.astype(np.float64)
    h0, h1 = P.split(x, s)
    assert np.array_equal((x * s).astype(np.float64), x64 * float(s)), 'the scaling is not exact'
    assert P.join_is_exact(h0, h1)
    for npl, bound in ((2, P.bound2(x, s)), (1, P.bound1(x, s))):
        back = P.join(h0, h1 if npl == 2 else None, s)
        err = np.abs(back.astype(np.float64) - x64)
        worst = float((err / bound).max())
        print('%s  %d plane(s): worst err / bound %.3f, floor share %.2f' % (name, npl, worst, P.floor_share(x, s, npl)))
        assert (err <= bound).all(), (name, npl, worst)
        assert worst > 0.99, 'the bound is not attained: the planted ties are missing'
        assert np.array_equal(P.round_trip_bound(x, s, npl), bound)          # no fp32 subnormals here
        # both branches of the bound are exercised
        assert 0.2 <= P.floor_share(x, s, npl) <= 0.8, (name, npl, P.floor_share(x, s, npl))
    # zeros keep their sign, the maximum is there with both signs
    assert (h0[x == 0].view(np.uint16) == np.where(np.signbit(x[x == 0]), 0x8000, 0).astype(np.uint16)).all() and (h1[x == 0] == 0).all()
    assert (x == amax).any() and (x == -amax).any()


def test_planted_edges_hit_what_they_name():
    """Ties to even with both neighbours, subnormal pieces, the window edge: read off the pieces of the planted values."""
    s = P.scale_for(P.bits_of(1.0))                    # 2^14
    v = np.array(P.SPECIAL_V, dtype=np.float32)
    assert np.array_equal(v.astype(np.float64), np.array(P.SPECIAL_V)), 'a planted value is no fp32 number'
    h0, h1 = P.split(v / s, s)
    piece = dict(zip(P.SPECIAL_V, zip(h0.astype(np.float64), h1.astype(np.float64))))
    assert piece[1.0 + 2.0 ** -11][0] == 1.0 and piece[1.0 + 3 * 2.0 ** -11][0] == 1.0 + 2.0 ** -9          # h0 ties: down and up, to even
    assert piece[1.0 + 2.0 ** -12 + 2.0 ** -23] == (1.0, 0.5) and piece[1.0 + 2.0 ** -12 + 3 * 2.0 ** -23] == (1.0, 0.5 * (1 + 2.0 ** -9))
    t = 2.0 ** -24
    assert piece[5.5 * t][0] == 6 * t and piece[6.5 * t][0] == 6 * t and piece[-2.5 * t][0] == -2 * t          # subnormal h0 ties
    assert piece[3 * t + 2.0 ** -26] == (3 * t, 2.0 ** -15)                                                   # both subnormal, exact
    assert piece[2.0 ** -14 + 2.0 ** -36] == (2.0 ** -14, 0.0) and piece[2.0 ** -14 + 3 * 2.0 ** -36] == (2.0 ** -14, 2 * t)
    assert piece[2.0 ** -14 + 3 * 2.0 ** -37] == (2.0 ** -14, t) and piece[2.0 ** -20 + 3 * 2.0 ** -37] == (2.0 ** -20, t)
    assert piece[2.0 ** -13] == (2.0 ** -13, 0.0) and piece[2.0 ** -30] == (0.0, 2.0 ** -19)
    n_sub0 = int(((np.abs(h0) < 2.0 ** -14) & (h0 != 0)).sum())
    n_sub1 = int(((np.abs(h1) < 2.0 ** -14) & (h1 != 0)).sum())
    assert n_sub0 >= 4 and n_sub1 >= 4
    # every one of them survives planting for the four range scalars
    for mult in MULTS:
        x, bits = P.plant(P.wide(3, 37, 72), mult)
        sx = P.scale_for(bits)
        got = set((x.astype(np.float64) * float(sx)).ravel().tolist())
        assert all(float(q) in got for q in P.SPECIAL_V), mult
        assert (np.signbit(x) & (x == 0)).any()


def test_scale_for_edges():
    sc = lambda v: float(P.scale_for(P.bits_of(v)))
    assert float(P.scale_for(0)) == 2.0 ** 115                     # bits 0: exponent field 268 clamped to 242
    assert float(P.scale_for(0x00000123)) == 2.0 ** 115            # a denormal bound
    assert sc(2.0 ** -110) == 2.0 ** 115                           # 2^124 by the formula: clamped
    assert sc(2.0 ** -101) == 2.0 ** 115 and sc(2.0 ** -100) == 2.0 ** 114          # the clamp begins below 2^-101
    assert sc(1.0) == 2.0 ** 14 and sc(1.9999999) == 2.0 ** 14 and sc(2.0) == 2.0 ** 13
    assert sc(2.0 ** 120) == 2.0 ** -106
    assert float(P.scale_for(0x7f800000)) == 2.0 ** -114           # +inf: exponent field 255 -> scale field 13 (the lower clamp is never reached)
    assert sc(3.0e38) == 2.0 ** -113
    for v in (1e-30, 3e-5, 0.7, 5.0, 1e9, 2.0 ** 120):
        assert 2.0 ** 14 <= v * sc(v) < 2.0 ** 15


def test_all_zero_tensor_round_trips():
    x = np.zeros((5, 8), dtype=np.float32)
    x[2, 3] = -0.0
    s = P.scale_for(0)
    h0, h1 = P.split(x, s)
    assert not h0.view(np.uint16)[x.view(np.uint32) == 0].any() and not h1.view(np.uint16).any()
    for h in (h1, None):
        back = P.join(h0, h, s)
        assert (back == 0).all()
        # (two planes: -0 + 0 / 2048 = +0, the sign of a zero is carried by one-plane tensors only)
        assert np.array_equal(back.view(np.uint32), x.view(np.uint32) if h is None else np.zeros_like(x).view(np.uint32))


def test_tiny_and_huge_bounds():
    """Data at 2^120 and at 2^-110 (the clamped scale; part of it fp32 subnormals): the bounds hold, with the subnormal spacing of the fp32
    result added where it applies."""
    base = P.wide(5, 64, 96)
    e = int(np.floor(np.log2(float(np.abs(base).max()))))
    for target in (120, -110):
        x, bits = P.plant((base.astype(np.float64) * 2.0 ** (target - e)).astype(np.float32))
        s = P.scale_for(bits)
        assert float(s) == (2.0 ** -106 if target == 120 else 2.0 ** 115)
        assert np.array_equal((x * s).astype(np.float64), x.astype(np.float64) * float(s))
        h0, h1 = P.split(x, s)
        assert P.join_is_exact(h0, h1)
        for npl in (2, 1):
            err = np.abs(P.join(h0, h1 if npl == 2 else None, s).astype(np.float64) - x.astype(np.float64))
            assert (err <= P.round_trip_bound(x, s, npl)).all(), (target, npl)
        if target == -110:
            assert ((x != 0) & (np.abs(x) < 2.0 ** -126)).any()


def test_phys_is_a_bijection():
    for n in (32, 64, 96 * 64, 32 * 1031):
        e = np.arange(n)
        both = np.concatenate([P.phys(e, True), P.phys(e, True) + 32])
        assert np.array_equal(np.sort(both), np.arange(2 * n))
        assert np.array_equal(P.phys(e, False), e)
    assert P.phys(31, True) == 31 and P.phys(32, True) == 64 and P.phys(70, True) == 134


@pytest.mark.parametrize('K,RS,C', [(9, 1, 64), (40, 1, 40), (32, 9, 32), (5, 2, 8)])
@pytest.mark.parametrize('interleave', [0, 1])
def test_filter_planes_against_a_plain_loop(K, RS, C, interleave):
    w = P.wide(K + C, K * RS, C).reshape(K, RS, C)
    s = P.scale_for(P.bits_of(np.abs(w).max()))
    fwd, tr = P.filter_planes(w, s, interleave)
    Kp = (K + 3) & ~3
    want_f, want_t = np.zeros(2 * K * RS * C, np.uint16), np.zeros(2 * C * RS * Kp, np.uint16)
    il_f, il_t = bool(interleave) and C % 32 == 0, bool(interleave) and Kp % 32 == 0
    for k in range(K):
        for r in range(RS):
            for c in range(C):
                h0, h1 = P.split(w[k, r, c], s)
                a0, a1 = int(h0.view(np.uint16)), int(h1.view(np.uint16))
                e = (k * RS + r) * C + c
                if il_f:
                    want_f[(e // 32) * 64 + e % 32], want_f[(e // 32) * 64 + e % 32 + 32] = a0, a1
                else:
                    want_f[e], want_f[K * RS * C + e] = a0, a1
                e = (c * RS + r) * Kp + k
                if il_t:
                    want_t[(e // 32) * 64 + e % 32], want_t[(e // 32) * 64 + e % 32 + 32] = a0, a1
                else:
                    want_t[e], want_t[C * RS * Kp + e] = a0, a1
    assert np.array_equal(fwd, want_f) and np.array_equal(tr, want_t)
    assert fwd.size == 2 * K * RS * C and tr.size == 2 * C * RS * Kp
