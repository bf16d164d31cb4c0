"""The float64 model of the fused inference convolution (tests/_eval_conv.py) against torch, and the teeth of its comparison helpers: every
way the kernels' epilogue can go wrong that the GPU tests rely on them to catch -- planes swapped, a lane pair's store one channel quad off,
a residual or an affine coefficient taken from the wrong place, an unwritten row, a store past the end, a wrong range scalar -- applied to
an otherwise perfect synthetic output, must be reported.  No GPU."""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

from tests import _eval_conv as E
from tests import _planes as P

ALL_GEOMS = [c[1] for c in E.EX_CASES] + [c[0] for c in E.F32_CASES]


@pytest.mark.parametrize('geo', ALL_GEOMS, ids=[repr(E.Geom(*g)) for g in ALL_GEOMS])
def test_model_equals_torch_float64(geo):
    """Identity planes (the operands are the values themselves): conv64 + epilogue64 against F.conv2d in float64 + affine + residual + ReLU."""
    g = E.Geom(*geo)
    d = E.make_data(g, 11)
    z, za = E.conv64(d['x'], d['w'], g)
    x = torch.from_numpy(d['x'].astype(np.float64)).permute(0, 3, 1, 2)
    w = torch.from_numpy(d['w'].astype(np.float64)).view(g.cout, g.k, g.k, g.cin).permute(0, 3, 1, 2)
    sc, sh, bi, res = (torch.from_numpy(d[k].astype(np.float64)) for k in ('scale', 'shift', 'bias', 'res'))
    plain = F.conv2d(x, w, None, g.stride, g.pad, g.dil).permute(0, 2, 3, 1).reshape(g.m, g.cout)
    assert plain.shape == z.shape
    for bias, with_res, relu in ((False, False, False), (True, True, True), (True, False, False), (False, True, True)):
        y, mag = E.epilogue64(z, za, d['scale'], d['shift'], d['bias'] if bias else None, d['res'] if with_res else None, relu)
        want = (plain + bi) * sc + sh if bias else plain * sc + sh
        if with_res:
            want = want + res
        if relu:
            want = torch.relu(want)
        err = np.abs(y - want.numpy())
        assert (err <= 1e-12 * mag).all(), (g, bias, with_res, relu, float((err / mag).max()))
        assert (mag >= np.abs(y)).all()


@pytest.mark.parametrize('geo', ALL_GEOMS[:12], ids=[repr(E.Geom(*g)) for g in ALL_GEOMS[:12]])
def test_generated_operands_rebuild_exactly(geo):
    """join of the generated pieces is exact in fp32 (the model's x^, w^, r^ ARE what an exact kernel multiplies), under a bound at the
    maximum and 4 x above it; the one-plane value is h0 / s."""
    g = E.Geom(*geo)
    d = E.make_data(g, 12)
    for name in ('x', 'w', 'res'):
        for mult in ((1.0, 4.0) if name == 'x' else (2.0,)):
            op = E.Operand(d[name], E.times_pow2(E.amax_bits(d[name]), mult), 2)
            assert P.join_is_exact(op.h0, op.h1), (g, name, mult)
            assert (np.abs(op.seen - d[name]) <= P.bound2(d[name], op.s)).all()
            one = E.Operand(d[name], op.bits, 1)
            assert np.array_equal(one.seen, one.h0.astype(np.float64) / float(one.s))
            assert (np.abs(one.seen - d[name]) <= P.bound1(d[name], one.s)).all()


def test_rounding_of_the_contracted_bound():
    q = E.Fraction
    assert E._rn32(q(1) + q(1, 2 ** 24)) == np.float32(1.0)                                    # ties to even, down
    assert E._rn32(q(1) + q(3, 2 ** 24)) == np.float32(1.0 + 2.0 ** -22)                       # ... and up
    assert E._rn32(q(1) + q(1, 2 ** 24) + q(1, 2 ** 80)) == np.float32(1.0 + 2.0 ** -23)        # just above the tie: what a double rounding gets wrong
    r = np.random.RandomState(0)
    for v in (r.standard_normal(50) * 2.0 ** r.uniform(-30, 30, 50)).astype(np.float32):
        assert E._rn32(q(float(abs(v)))) == abs(v)
    # a product whose exact sum with the addend differs from the twice-rounded one: both patterns are offered, and they differ
    a, b, c = np.float32(1.0 + 2.0 ** -12), np.float32(1.0 + 2.0 ** -12), np.float32(2.0 ** -25)
    bits = E.bound_candidates(1, P.bits_of(1.0), P.bits_of(a), P.bits_of(b), P.bits_of(c))
    assert bits == {P.bits_of(np.float32(np.float32(a * b) + c)), P.bits_of(E._rn32(q(float(a)) * q(float(b)) + q(float(c))))} and len(bits) == 2
    with_res = E.bound_candidates(9 * 64, P.bits_of(0.75), P.bits_of(0.3), P.bits_of(1.7), P.bits_of(0.4), P.bits_of(3.5))
    without = E.bound_candidates(9 * 64, P.bits_of(0.75), P.bits_of(0.3), P.bits_of(1.7), P.bits_of(0.4))
    assert not (with_res & without)


def test_placement_follows_the_stride_rule():
    assert E.planes_stride(63, 40, 2) == 63 * 40 and E.planes_stride(63, 64, 2) == 32 and E.planes_stride(63, 64, 1) == 63 * 64
    assert E.planes_stride(2 ** 24, 32, 2) == 2 ** 29                    # 4 M C = 2^31: both planes no longer fit one 2 GiB descriptor
    t = np.arange(3 * 64, dtype=np.float32).reshape(3, 64)
    s = P.scale_for(P.bits_of(3 * 64))
    buf = E.encode_planes(t, s, 2)
    assert buf.size == 2 * 3 * 64
    h0, h1 = P.split(t, s)
    assert np.array_equal(buf[64:96], h0.ravel()[32:64].view(np.uint16)) and np.array_equal(buf[96:128], h1.ravel()[32:64].view(np.uint16))
    g0, g1, back = E.decode_planes(buf, 3, 64, 2, s)
    assert np.array_equal(g0, h0) and np.array_equal(g1, h1) and np.array_equal(back, t)


# ---- teeth --------------------------------------------------------------------------------------------------------------------------------------
class _Perfect:
    """A synthetic perfect kernel output for a small ragged geometry: the float64 reference rounded to fp32, in the buffers the GPU tests
    hand to the helpers -- fp32 and planes, with their guards."""

    def __init__(self, cout, nplanes):
        self.g = g = E.Geom(24, cout, 1, 1, 0, 1, 1, 9, 7)              # M = 63: ragged against every tile height
        self.npl = nplanes
        d = self.d = E.make_data(g, 21)
        self.x = E.Operand(d['x'], E.amax_bits(d['x']), nplanes)
        self.w = E.Operand(d['w'], E.amax_bits(d['w']), nplanes)
        self.r = E.Operand(d['res'], E.times_pow2(E.amax_bits(d['res']), 2.0), nplanes)
        self.z, self.za = E.conv64(self.x.seen, self.w.seen, g)
        self.cand = E.bound_candidates(g.klen, self.x.bits, self.w.bits, E.amax_bits(d['scale']), E.amax_bits(d['shift']), E.amax_bits(d['res']))
        self.cand_no_res = E.bound_candidates(g.klen, self.x.bits, self.w.bits, E.amax_bits(d['scale']), E.amax_bits(d['shift']))
        self.out_bits = min(self.cand)
        self.y64, self.mag = self.ref()
        self.y32 = self.y64.astype(np.float32)

    def ref(self, scale=None, shift=None, res=None):
        d = self.d
        return E.epilogue64(self.z, self.za, d['scale'] if scale is None else scale, d['shift'] if shift is None else shift, d['bias'],
                            self.r.seen if res is None else res, True)

    def f32_buf(self, y=None, pitch=None, c0=0):
        g = self.g
        pitch = pitch or g.cout
        buf = np.full(g.m * pitch + 2 * E.GUARD, np.nan, dtype=np.float32)
        buf[E.GUARD:E.GUARD + g.m * pitch].reshape(g.m, pitch)[:, c0:c0 + g.cout] = self.y32 if y is None else y
        return buf

    def plane_buf(self, y=None):
        g = self.g
        buf = np.full(2 * g.m * g.cout + 2 * E.GUARD, P.FILL16, dtype=np.uint16)
        return E.encode_planes(self.y32 if y is None else y, P.scale_for(self.out_bits), self.npl, out=buf, base=E.GUARD)

    def check_f32(self, buf, pitch=None, c0=0):
        return E.check_f32(buf, self.g.m, self.g.cout, pitch or self.g.cout, c0, self.y64, self.mag, 'synthetic fp32')

    def check_planes(self, buf, same=True):
        return E.check_planes(buf, self.g.m, self.g.cout, self.npl, self.out_bits, self.y64, self.mag, 'synthetic planes', same_as=self.y32 if same else None)


@pytest.fixture(scope='module', params=[(40, 2), (64, 2), (40, 1)], ids=['separate', 'interleaved', 'one-plane'])
def perfect(request):
    return _Perfect(*request.param)


def _fails(fn, *a, **k):
    with pytest.raises(AssertionError):
        fn(*a, **k)


def test_the_perfect_output_passes(perfect):
    p = perfect
    r, y = p.check_f32(p.f32_buf())
    assert r <= 2.0 ** -24 / E.TOL + 1e-9 and np.array_equal(y, p.y32)          # one rounding of the reference: 0.05 of the tolerance
    r, _ = p.check_f32(p.f32_buf(pitch=p.g.cout + 32, c0=16), p.g.cout + 32, 16)
    assert r <= 0.05
    assert p.check_planes(p.plane_buf()) <= 0.05
    E.check_bound(p.out_bits, p.cand, np.abs(p.y32).max(), 'synthetic')
    E.check_amax(E.amax_bits(p.y32), p.y32, 'synthetic')


def test_swapped_planes_of_one_channel_group_are_caught(perfect):
    p = perfect
    a0, a1 = E.plane_index(p.g.m, p.g.cout, p.npl)
    e = 17 * p.g.cout + 8 + np.arange(8)
    if p.npl == 1:                                                             # one plane: the group changes places with its neighbour
        a1 = np.roll(a0, -8)
    buf = p.plane_buf()
    buf[E.GUARD + a0[e]], buf[E.GUARD + a1[e]] = buf[E.GUARD + a1[e]].copy(), buf[E.GUARD + a0[e]].copy()
    _fails(p.check_planes, buf)
    _fails(p.check_planes, buf, same=False)


def test_a_lane_pairs_store_one_quad_late_is_caught(perfect):
    """The odd lane of a pair writes its 16 bytes (8 channels of the last plane) at element e instead of e - 4."""
    p = perfect
    a0, a1 = E.plane_index(p.g.m, p.g.cout, p.npl)
    at = a1 if p.npl == 2 else a0
    for row, c in ((30, 16), (p.g.m - 1, p.g.cout - 8)):                       # inside a row; the last piece of the tensor, whose late store leaves it
        e = row * p.g.cout + c + np.arange(8)
        buf = p.plane_buf()
        piece = buf[E.GUARD + at[e]].copy()
        buf[E.GUARD + at[e]] = P.FILL16                                        # never written where it belongs
        late = e + 4
        inside = late < p.g.m * p.g.cout
        buf[E.GUARD + at[late[inside]]] = piece[inside]
        buf[E.GUARD + at[e[-1]] + 1 + np.arange(int((~inside).sum()))] = piece[~inside]
        _fails(p.check_planes, buf)
        _fails(p.check_planes, buf, same=False)


def test_a_residual_dropped_in_the_last_channel_quad_is_caught(perfect):
    p = perfect
    y = p.y32.copy()
    res = p.r.seen.copy()
    res[:, -4:] = 0.0
    dropped = p.ref(res=res)[0].astype(np.float32)
    row = int(np.nonzero((dropped != p.y32).any(1))[0][0])                      # one row, the first in which the ReLU does not hide it
    y[row] = dropped[row]
    _fails(p.check_f32, p.f32_buf(y))
    _fails(p.check_planes, p.plane_buf(y), same=False)


def test_coefficients_of_channel_n_plus_4_are_caught(perfect):
    p = perfect
    y = p.ref(scale=np.roll(p.d['scale'], -4), shift=np.roll(p.d['shift'], -4))[0].astype(np.float32)
    _fails(p.check_f32, p.f32_buf(y))
    _fails(p.check_planes, p.plane_buf(y), same=False)
    y = p.ref(shift=np.roll(p.d['shift'], -4))[0].astype(np.float32)          # the shift alone
    _fails(p.check_f32, p.f32_buf(y))
    _fails(p.check_planes, p.plane_buf(y), same=False)


def test_an_unwritten_last_row_is_caught(perfect):
    p = perfect
    buf = p.f32_buf()
    buf[E.GUARD + (p.g.m - 1) * p.g.cout:E.GUARD + p.g.m * p.g.cout] = np.nan
    _fails(p.check_f32, buf)
    a0, a1 = E.plane_index(p.g.m, p.g.cout, p.npl)
    e = (p.g.m - 1) * p.g.cout + np.arange(p.g.cout)
    for at in (a0, a1)[:p.npl]:
        buf = p.plane_buf()
        buf[E.GUARD + at[e]] = P.FILL16
        _fails(p.check_planes, buf)
        _fails(p.check_planes, buf, same=False)


def test_a_store_past_the_end_is_caught(perfect):
    p = perfect
    buf = p.f32_buf()
    buf[E.GUARD + p.g.m * p.g.cout:E.GUARD + p.g.m * p.g.cout + 4] = 0.0
    _fails(p.check_f32, buf)
    buf = p.f32_buf(pitch=p.g.cout + 32, c0=16)
    buf[E.GUARD + 16 + p.g.cout:E.GUARD + 16 + p.g.cout + 4] = 0.0            # past the slice of row 0, inside the pitch
    _fails(p.check_f32, buf, p.g.cout + 32, 16)
    buf = p.plane_buf()
    end = E.GUARD + E.plane_halves(p.g.m, p.g.cout, p.npl)                    # one plane: where a second plane would begin
    buf[end:end + 4] = 0x3c00
    _fails(p.check_planes, buf)
    buf = p.plane_buf()
    buf[E.GUARD - 4:E.GUARD] = 0
    _fails(p.check_planes, buf)


def test_wrong_range_scalars_are_caught(perfect):
    p = perfect
    _fails(E.check_amax, p.out_bits, p.y32, 'the scale bound reported as the true maximum')
    _fails(E.check_amax, E.amax_bits(p.y32) + 1, p.y32, 'one ulp above')
    assert not (p.cand & p.cand_no_res)
    _fails(E.check_bound, min(p.cand_no_res), p.cand, np.abs(p.y32).max(), 'the bound without the residual term')
    _fails(E.check_bound, p.out_bits, p.cand, 2.0 * float(P.float_of(p.out_bits)), 'a bound below the maximum')


def test_conv_form_names_follow_the_header():
    """pylc_amd.lib.CONV_FORMS names the PYLC_CONV_FORM_* values of include/pylc_hip.h in order, and the query itself needs
    no GPU."""
    import os
    import re
    from pylc_amd import lib as L
    hdr = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), 'include', 'pylc_hip.h')).read()
    hdr = re.sub(r'/\*.*?\*/', '', hdr, flags=re.S)
    forms = sorted((int(v), n) for n, v in re.findall(r'PYLC_CONV_FORM_([A-Z0-9_]+)\s*=\s*(\d+)', hdr))
    assert [v for v, _ in forms] == list(range(len(L.CONV_FORMS)))
    assert [n.lower().replace('_', '-') for _, n in forms] == list(L.CONV_FORMS)
    assert 0 <= L.lib.pylc_debug_last_conv_form() < len(L.CONV_FORMS)          # (`none` until the process launches a conv)
    assert {c[0] for c in E.EX_CASES} <= set(L.CONV_FORMS)
