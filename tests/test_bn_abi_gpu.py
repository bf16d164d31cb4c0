"""Training-mode and synchronised BatchNorm kernels at the C ABI against fp64 (-m gpu): every stage of the forward
and backward chains judged on its own inputs with the derived worst-case rounding bounds of tests/_bn.py, per channel and per element,
on pitched NaN-filled buffers; the range bounds as true upper bounds equal to the header's formulas; the 1-bit ReLU mask unpacked;
SyncBN with the ranks simulated in one process (the all-reduce is a torch sum on the device).

Every test prints its worst figure as error / bound (lines BN-A .. BN-E; 1.0 = at the bound).  The implementing run on an MI355X, worst
over the cases of each section:
  BN-A  sum y 0.34, sum y^2 0.30, mean 0.35, invstd 0.36, scale 0.45, shift 0.27, running mean / var 0.33 / 0.40, out 0.73 (40 x 1536),
        bound_out against the formula 0.44 of its 4u; from-partial: bit-identical for 1, 7 and 300 row groups
  BN-B  sum g xhat 0.25, sum g 0.25, dy 0.60 (1000 x 64), dy_bound_out 0.26 of its 8u; amax_dy, g_amax, g_out exact
  BN-C  ours against 4 x torch's fp32 error + bound, per channel: out 0.19, dy 0.10, dgamma 0.14, dbeta 0.19, running mean / var 0.29 /
        0.32; our error / torch's, maximum over channels: dy 0.25-2.1 (363 x 48: 3.6e-4 against 1.7e-4), dgamma 0.07-0.78; elements
        within the chain's bound of the ReLU kink (no part in the gradient comparison): at most 7.6e-5 of a tensor
  BN-D  invstd 0.70, mean 0.49, scale 0.72, out 0.62, all-reduced sums 0.20,
        dy 0.45, pylc_bn_bwd_bound 0.29 of its 8u; one rank: every output and the dy bound bit-identical to pylc_bn_finalize_ex /
        dy_bound_out
  BN-E  skipped on the product library (EXPERIMENTAL=1 builds only)
"""
import ctypes as C

import pytest
import torch
import torch.nn.functional as F

from tests import _bn as B
from tests.conftest import needs_experimental

pytestmark = pytest.mark.gpu

EPS, MOM = 1e-5, 0.1
NAN = float('nan')


# ---- buffers -------------------------------------------------------------------------------------------------------------------------------
def _pitched(t, pitch, fill=NAN):
    """[M][C] values in an [M][pitch] buffer whose unused lanes hold `fill`; returns (buffer, view of the values)."""
    m, c = t.shape
    buf = torch.full((m, pitch), fill, device=t.device, dtype=t.dtype)
    buf[:, :c] = t
    return buf, buf[:, :c]


def _out(dev, m, c, p):
    return _pitched(torch.zeros(m, c, device=dev), p)


def _lanes_clean(buf, c, what):
    assert torch.isnan(buf[:, c:]).all(), '%s: a lane beyond C was written' % what
    assert not torch.isnan(buf[:, :c]).any(), '%s: a NaN reached the result' % what


class _Arena:
    """Small per-channel outputs carved out of one NaN-filled allocation with 8 floats between them: what lies between must stay NaN."""

    def __init__(self, dev, dtype=torch.float32):
        self.dev, self.dtype, self.parts, self.n = dev, dtype, [], 8

    def take(self, n, init=None):
        self.parts.append((self.n, n, init))
        self.n += -(-n // 8) * 8 + 8
        return len(self.parts) - 1

    def build(self):
        self.buf = torch.full((self.n,), NAN, device=self.dev, dtype=self.dtype)
        views = []
        for o, n, init in self.parts:
            if init is not None:
                self.buf[o:o + n] = init
            views.append(self.buf[o:o + n])
        return views

    def gaps_clean(self):
        keep = torch.ones(self.n, dtype=torch.bool, device=self.dev)
        for o, n, _ in self.parts:
            keep[o:o + n] = False
        return bool(torch.isnan(self.buf[keep]).all())


def _check(stage, err, bound, fig=None):
    """err <= bound everywhere (a zero bound asks for exact equality); the failure message names the stage and the worst index.  Returns
    the worst err / bound."""
    err, bound = err.double(), bound.double().expand_as(err)
    assert not torch.isnan(err).any(), '%s: NaN' % stage
    bad = err > bound
    if bad.any():
        i = torch.nonzero(bad & ((err - bound) == (err - bound)[bad].max()))[0].tolist()
        raise AssertionError('%s: index %s (of shape %s) err %.6g > bound %.6g; %d over the bound' %
                             (stage, i, tuple(err.shape), err[tuple(i)].item(), bound[tuple(i)].item(), int(bad.sum())))
    live = bound > 0
    r = (err[live] / bound[live]).max().item() if live.any() else 0.0
    if fig is not None:
        fig[stage.split(':')[-1].strip()] = max(fig.get(stage.split(':')[-1].strip(), 0.0), r)
    return r


def _report(tag, case, fig):
    print('%s %s  ' % (tag, case) + '  '.join('%s %.3f' % kv for kv in fig.items()))


def _f32(bits):
    return bits.view(torch.float32)


def _zero_u32(dev):
    return torch.zeros(1, dtype=torch.int32, device=dev)


def _bits_of(x, dev):
    return torch.tensor([float(x)], dtype=torch.float32, device=dev).view(torch.int32)


# ---- kernel launches -------------------------------------------------------------------------------------------------------------------------
def _L():
    from pylc_amd import lib as L
    L.init()
    return L


def k_stats(y, p):
    L = _L()
    m, c = y.shape
    ar = _Arena(y.device)
    ar.take(2 * c)
    sums, = ar.build()
    ws = torch.empty(L.lib.pylc_bn_workspace_floats(m, c), device=y.device)
    L.check(L.lib.pylc_bn_stats(L.ptr(y), m, c, p, L.ptr(sums), L.ptr(ws), L.stream()))
    assert ar.gaps_clean(), 'bn_stats wrote outside sums[2C]'
    return sums


class _Coef:
    """Outputs of a finalize: mean, invstd, scale, shift, running mean / var, bound (float), all from one arena."""
    names = ('mean', 'invstd', 'scale', 'shift', 'rm', 'rv')

    def __init__(self, dev, c, rm, rv):
        self.ar = _Arena(dev)
        for _ in range(4):
            self.ar.take(c)
        self.ar.take(c, rm)
        self.ar.take(c, rv)
        self.mean, self.invstd, self.scale, self.shift, self.rm, self.rv = self.ar.build()
        self.bound = _zero_u32(dev)

    def done(self, what):
        assert self.ar.gaps_clean(), '%s wrote outside its [C] outputs' % what
        for n in self.names:
            assert not torch.isnan(getattr(self, n)).any(), '%s: NaN in %s' % (what, n)
        return self

    def same_bits(self, other, what, names=None):
        for n in names or self.names + ('bound',):
            a, b = getattr(self, n), getattr(other, n)
            if not torch.equal(a, b):
                i = torch.nonzero(a != b)[0].item()
                raise AssertionError('%s: %s differs at channel %d: %r vs %r' % (what, n, i, a[i].item(), b[i].item()))


def k_finalize(sums, n, c, inp, clamp, y=None, yp=0, K=None, extra=None, mul=1.0, partial=None):
    """pylc_bn_finalize_ex, or with partial = (tensor, rows) pylc_bn_finalize_from_partial_ex."""
    L = _L()
    dev = inp.gamma.device
    co = _Coef(dev, c, inp.rm, inp.rv)
    tail = (L.ptr(inp.gamma), L.ptr(inp.beta), EPS, MOM, int(clamp), L.ptr(co.rm), L.ptr(co.rv), L.ptr(co.mean), L.ptr(co.invstd), L.ptr(co.scale),
            L.ptr(co.shift), L.ptr(extra), mul, L.ptr(co.bound), L.ptr(y), yp, int(n) if y is not None else 0, L.ptr(K), L.stream())
    if partial is None:
        L.check(L.lib.pylc_bn_finalize_ex(L.ptr(sums), float(n), c, *tail))
    else:
        L.check(L.lib.pylc_bn_finalize_from_partial_ex(L.ptr(partial), partial.shape[0], float(n), c, *tail))
    return co.done('bn_finalize')


def k_local_moments(sums, n, c, y, yp, K):
    L = _L()
    ar = _Arena(sums.device, torch.float64)
    ar.take(2 * c + 1)
    mom, = ar.build()
    L.check(L.lib.pylc_bn_local_moments(L.ptr(sums), float(n), c, L.ptr(y), yp if y is not None else 0, int(n) if y is not None else 0, L.ptr(K),
                                        L.ptr(mom), L.stream()))
    assert ar.gaps_clean(), 'bn_local_moments wrote outside moments[2C + 1]'
    assert not torch.isnan(mom).any(), 'bn_local_moments: NaN'
    return mom


def k_finalize_moments(mom, n, c, inp, clamp, K=None, extra=None, mul=1.0):
    L = _L()
    co = _Coef(mom.device, c, inp.rm, inp.rv)
    L.check(L.lib.pylc_bn_finalize_moments(L.ptr(mom), float(n), c, L.ptr(inp.gamma), L.ptr(inp.beta), EPS, MOM, int(clamp), L.ptr(co.rm), L.ptr(co.rv),
                                           L.ptr(co.mean), L.ptr(co.invstd), L.ptr(co.scale), L.ptr(co.shift), L.ptr(extra), mul, L.ptr(co.bound),
                                           L.ptr(K), L.stream()))
    return co.done('bn_finalize_moments')


def _extra(mask=None, g_amax=None):
    L = _L()
    ex = L.BnExtra()
    ex.nplanes = 2
    ex.relu_mask, ex.g_amax = L.ptr(mask), L.ptr(g_amax)
    return ex


def k_apply(y, p, co, res, relu, want_amax=False, bits=False):
    """pylc_bn_apply, or pylc_bn_apply_ex when the 1-bit mask is asked for.  Returns (out view, amax bits or None, mask bytes or None)."""
    L = _L()
    m, c = y.shape
    obuf, out = _out(y.device, m, c, p)
    amax = _zero_u32(y.device) if want_amax else None
    mask = torch.zeros(m * c // 8 + 16, dtype=torch.uint8, device=y.device) if bits else None
    if bits:
        mask[m * c // 8:] = 0xA5                                                   # guard bytes behind the mask
        ex = _extra(mask=mask)
        L.check(L.lib.pylc_bn_apply_ex(L.ptr(y), p, L.ptr(co.scale), L.ptr(co.shift), L.ptr(res), p if res is not None else 0, L.ptr(out), p, m, c,
                                       int(relu), L.ptr(amax), C.byref(ex), L.stream()))
        assert (mask[m * c // 8:] == 0xA5).all(), 'bn_apply: wrote behind the M*C/8 mask bytes'
        mask = mask[:m * c // 8]
    else:
        L.check(L.lib.pylc_bn_apply(L.ptr(y), p, L.ptr(co.scale), L.ptr(co.shift), L.ptr(res), p if res is not None else 0, L.ptr(out), p, m, c,
                                    int(relu), L.ptr(amax), L.stream()))
    _lanes_clean(obuf, c, 'bn_apply')
    return out, amax, mask


def _mask_args(mode, fwd_out, p, co, mask):
    """(out, out_pitch, scale, shift) of the backward entry points for a mask source: fp32 `out`, the 1-bit mask / no ReLU (neither), or the
    forward's coefficients to recompute the mask from y."""
    L = _L()
    if mode == 'out':
        return L.ptr(fwd_out), p, None, None
    if mode in ('bits', 'none'):
        return None, 0, None, None
    return None, 0, L.ptr(co.scale), L.ptr(co.shift)


def k_bwd_reduce(dout, y, p, co, mode, fwd_out=None, mask=None, gamma=None, n=0.0, use_ex=False, want_bound=False, sums_view=None):
    """Returns (sums[2C], g_amax bits or None, dy bound bits or None)."""
    L = _L()
    m, c = y.shape
    dev = y.device
    if sums_view is None:
        ar = _Arena(dev)
        ar.take(2 * c)
        sums_view, = ar.build()
    else:
        ar = None
    ws = torch.empty(L.lib.pylc_bn_workspace_floats(m, c), device=dev)
    o, op, sc, sh = _mask_args(mode, fwd_out, p, co, mask)
    relu = int(mode != 'none')
    g_amax = bound = None
    if use_ex or mode == 'bits' or want_bound:
        g_amax = _zero_u32(dev)
        bound = _zero_u32(dev) if want_bound else None
        ex = _extra(mask=mask if mode == 'bits' else None, g_amax=g_amax)
        L.check(L.lib.pylc_bn_bwd_reduce_ex(L.ptr(dout), p, o, op, L.ptr(y), p, L.ptr(co.mean), L.ptr(co.invstd), m, c, relu, L.ptr(sums_view), L.ptr(ws),
                                            sc, sh, L.ptr(gamma), float(n), C.byref(ex), L.ptr(bound), L.stream()))
    else:
        L.check(L.lib.pylc_bn_bwd_reduce(L.ptr(dout), p, o, op, L.ptr(y), p, L.ptr(co.mean), L.ptr(co.invstd), m, c, relu, L.ptr(sums_view), L.ptr(ws),
                                         sc, sh, L.stream()))
    if ar is not None:
        assert ar.gaps_clean(), 'bn_bwd_reduce wrote outside sums[2C]'
    assert not torch.isnan(sums_view).any(), 'bn_bwd_reduce: NaN in the sums'
    return sums_view, g_amax, bound


def k_bwd_apply(dout, y, p, co, gamma, sums, n, mode, fwd_out=None, mask=None, want_g=False, want_amax=False, use_ex=False):
    """Returns (dy view, g view or None, amax bits or None)."""
    L = _L()
    m, c = y.shape
    dev = y.device
    dybuf, dy = _out(dev, m, c, p)
    gbuf, gv = _out(dev, m, c, p) if want_g else (None, None)
    amax = _zero_u32(dev) if want_amax else None
    o, op, sc, sh = _mask_args(mode, fwd_out, p, co, mask)
    relu = int(mode != 'none')
    args = (L.ptr(dout), p, o, op, L.ptr(y), p, L.ptr(co.mean), L.ptr(co.invstd), L.ptr(gamma), L.ptr(sums), float(n), m, c, relu, L.ptr(dy), p,
            L.ptr(gv), p if want_g else 0, L.ptr(amax), sc, sh)
    if use_ex or mode == 'bits':
        ex = _extra(mask=mask if mode == 'bits' else None)
        L.check(L.lib.pylc_bn_bwd_apply_ex(*args, C.byref(ex), L.stream()))
    else:
        L.check(L.lib.pylc_bn_bwd_apply(*args, L.stream()))
    _lanes_clean(dybuf, c, 'bn_bwd_apply(dy)')
    if want_g:
        _lanes_clean(gbuf, c, 'bn_bwd_apply(g_out)')
    return dy, gv, amax


# ---- one shape's operands and forward, shared by the tests of sections A-C ---------------------------------------------------------------------
class _Case:
    def __init__(self, dev, m, c, extra):
        self.m, self.c, self.p, self.dev = m, c, c + extra, dev
        self.cpu = B.make_inputs(m, c)
        i = self.cpu
        self.ybuf, self.y = _pitched(i.y.to(dev), self.p)
        self.dbuf, self.dout = _pitched(i.dout.to(dev), self.p)
        self.rbuf, self.res = _pitched(i.res.to(dev), self.p)
        self.inp = B.Inputs(self.y, i.gamma.to(dev), i.beta.to(dev), self.dout, self.res, i.rm.to(dev), i.rv.to(dev))
        self.S1, self.S2, self.SA, self.n = B.stats64(self.y)
        self.refined, border = B.needs_refine(self.S1, self.S2, self.n)
        assert not border.any()
        self._fwd = {}

    def sums(self):
        if not hasattr(self, '_sums'):
            self._sums = k_stats(self.y, self.p)
        return self._sums

    def coef(self, clamp=False, **kw):
        key = ('coef', clamp)
        if kw:
            return k_finalize(self.sums(), self.m, self.c, self.inp, clamp, y=self.y, yp=self.p, **kw)
        if key not in self._fwd:
            self._fwd[key] = k_finalize(self.sums(), self.m, self.c, self.inp, clamp, y=self.y, yp=self.p)
        return self._fwd[key]

    def forward(self, way):
        """way: 'plain' (no residual, no ReLU), 'relu' (no residual), 'res' (residual + ReLU), 'bits' (the same with the 1-bit mask)."""
        if way not in self._fwd:
            co = self.coef()
            res = self.res if way in ('res', 'bits') else None
            self._fwd[way] = k_apply(self.y, self.p, co, res, relu=way != 'plain', want_amax=True, bits=way == 'bits')
        return self._fwd[way]


_CASES = {}


def _case(dev, m, c, extra):
    if (m, c, extra) not in _CASES:
        _CASES[(m, c, extra)] = _Case(dev, m, c, extra)
    return _CASES[(m, c, extra)]


def _coef_checks(stage, co, ref, S1, S2, SA, n, clamp, refined, inp, fig, skip=None):
    """The per-channel outputs of a finalize against fp64 coefficients `ref` with the bounds of tests/_bn.py; `skip`: channels left out."""
    dvar = B.d_var(S1, S2, SA, n, refined)
    keep = torch.ones_like(refined) if skip is None else ~skip
    if clamp:
        amb = B.clamp_ambiguous(dvar, ref.var, EPS) & keep
        assert not amb.any(), '%s: the inputs leave channel %d within dvar of the clamp' % (stage, torch.nonzero(amb)[0].item())
    rel = B.d_invstd_rel(dvar, ref.var, EPS, clamp)
    dmean = B.d_mean(S1, SA, n, ref.mean, refined)
    dscale = B.d_scale(ref.scale, rel)
    z = lambda t: torch.where(keep, t, torch.zeros_like(t))
    _check(stage + ': mean', z((co.mean.double() - ref.mean).abs()), dmean, fig)
    _check(stage + ': invstd', z((co.invstd.double() - ref.invstd).abs()), rel * ref.invstd, fig)
    _check(stage + ': scale', z((co.scale.double() - ref.scale).abs()), dscale, fig)
    _check(stage + ': shift', z((co.shift.double() - ref.shift).abs()), B.d_shift(ref, dmean, dscale), fig)
    _check(stage + ': running_mean', z((co.rm.double() - B.running64(inp.rm, ref.mean, MOM)).abs()), B.d_running(inp.rm, ref.mean, dmean, MOM), fig)
    dunb = dvar * (n / (n - 1.0) if n > 1 else 1.0)
    _check(stage + ': running_var', z((co.rv.double() - B.running64(inp.rv, ref.unbiased, MOM)).abs()), B.d_running(inp.rv, ref.unbiased, dunb, MOM), fig)
    if clamp:
        # a clamped channel stores exactly (float)(1 / sqrt((double)eps)): what ops/bn.py compares against bit-wise
        thr = torch.tensor(EPS, dtype=torch.float32, device=co.invstd.device).double().rsqrt().float()
        low = keep & (ref.var + dvar < B.eps64(EPS))
        assert (co.invstd[low] == thr).all(), '%s: a clamped channel does not hold (float)(1/sqrt((double)eps))' % stage


def _exact_amax(out, rounding):
    """What bound_out bounds.  Samuelson's inequality is ATTAINED when n - 1 values of a channel coincide -- always at n = 2, where
    |xhat| = sqrt(n - 1) = 1 for both rows once eps is negligible or clamped away -- so the bound holds for the exact output and the stored
    one may exceed it by the apply pass's own rounding (measured at 2 x 8, clamp: 12u of the bound, from 3u of |y scale| + |shift|, both
    large where two close values give a large invstd).  Harmless to the plane format: the bound only selects a power-of-two scale into
    [2^14, 2^15), a binade below fp16's range.  The term taken off is the elementwise apply bound, nothing else."""
    return (out.double().abs() - rounding).max().item()


def _bound_check(stage, bits, want, at_least, rel_u, fig):
    got = _f32(bits).item()
    assert got >= at_least, '%s: the bound %.9g is below the value it bounds, %.9g' % (stage, got, at_least)
    r = abs(got - want) / (rel_u * B.U * abs(want))
    assert r <= 1.0, '%s: bound %.9g, formula %.9g: %.2f of the %du allowed' % (stage, got, want, r, rel_u)
    fig[stage.split(':')[-1].strip()] = max(fig.get(stage.split(':')[-1].strip(), 0.0), r)


# ---- A: the forward chain --------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('m,c,extra', B.SHAPES)
def test_forward_chain_stage_by_stage(dev, m, c, extra):
    """pylc_bn_stats -> pylc_bn_finalize_ex (both clamp_eps values, bound_out, running statistics) -> pylc_bn_apply / _ex four ways."""
    cs = _case(dev, m, c, extra)
    fig = {}
    sums = cs.sums()
    dS1, dS2 = B.d_sums(cs.S2, cs.SA)
    _check('bn_stats: sum y', (sums[:c].double() - cs.S1).abs(), dS1, fig)
    _check('bn_stats: sum y^2', (sums[c:].double() - cs.S2).abs(), dS2, fig)
    res_amax = cs.res.abs().max().item()
    for clamp in (False, True):
        ref = B.coeffs64(cs.S1, cs.S2, cs.n, cs.inp.gamma, cs.inp.beta, EPS, clamp)
        # bound_extra (the residual's range) in one run, bound_mul (dropout's keep scale) in the other
        co = cs.coef(clamp, extra=_bits_of(res_amax, dev), mul=1.0) if not clamp else cs.coef(clamp, extra=None, mul=2.0)
        _coef_checks('bn_finalize_ex(clamp=%d)' % clamp, co, ref, cs.S1, cs.S2, cs.SA, cs.n, clamp, cs.refined, cs.inp, fig)
        if not clamp:
            cs.coef().same_bits(co, 'bn_finalize_ex with / without bound_extra', names=_Coef.names)
        for way in ('plain', 'relu', 'res', 'bits'):
            if way == 'bits' and c % 8:
                continue
            if clamp and way != 'relu':
                continue
            res = cs.res if way in ('res', 'bits') else None
            out, amax, mask = k_apply(cs.y, cs.p, co, res, relu=way != 'plain', want_amax=True, bits=way == 'bits') if clamp else cs.forward(way)
            pre = cs.y.double() * co.scale.double() + co.shift.double() + (res.double() if res is not None else 0.0)
            want = pre if way == 'plain' else pre.clamp(min=0.0)
            _check('bn_apply(%s): out' % way, (out.double() - want).abs(), B.apply_bound(cs.y, co.scale, co.shift, res), fig)
            assert torch.equal(_f32(amax), out.abs().max().reshape(1)), 'bn_apply(%s): amax_out is not max|out| of the stored output' % way
            if way == 'bits':
                assert torch.equal(out, cs.forward('res')[0]), 'bn_apply_ex(relu_mask): out differs from pylc_bn_apply'
                got = B.unpack_relu_bits(mask, m, c)
                bad = torch.nonzero(got != (out > 0))
                assert bad.numel() == 0, 'relu_mask: bit of element %s is not (out > 0)' % bad[0].tolist()
            if (not clamp and way == 'res') or (clamp and way == 'relu'):
                mul, extra_v = (1.0, res_amax) if not clamp else (2.0, 0.0)
                _bound_check('bn_finalize_ex(clamp=%d): bound_out' % clamp, co.bound, B.samuelson_bound64(cs.inp.gamma, cs.inp.beta, cs.n, extra_v, mul),
                             _exact_amax(out, B.apply_bound(cs.y, co.scale, co.shift, res)) * mul, 4, fig)
    _report('BN-A', '%dx%d+%d' % (m, c, extra), fig)


@pytest.mark.parametrize('m,c,extra', [(1000, 64, 0), (363, 48, 4), (75, 20, 0), (40, 1536, 0)])
def test_finalize_from_partial_has_the_bits_of_the_two_launch_path(dev, m, c, extra):
    """pylc_bn_finalize_from_partial_ex on partials built here (1, 7 and 300 row groups; 300 is no multiple of the 8 x 32 rows a block has in
    flight) against pylc_bn_stats_from_partial + pylc_bn_finalize_ex: the header says bit-identical."""
    L = _L()
    cs = _case(dev, m, c, extra)
    for groups in (1, 7, min(300, m)):
        parts = torch.tensor_split(cs.y.double(), groups)
        partial = torch.stack([torch.cat((q.sum(0), (q * q).sum(0))) for q in parts]).float().contiguous()
        ar = _Arena(dev)
        ar.take(2 * c)
        sums, = ar.build()
        L.check(L.lib.pylc_bn_stats_from_partial(L.ptr(partial), groups, c, L.ptr(sums), L.stream()))
        assert ar.gaps_clean()
        want = torch.stack([torch.cat((q.sum(0), (q * q).sum(0))) for q in parts]).float().double().sum(0).float()
        assert torch.equal(sums, want), 'bn_stats_from_partial(%d rows): not the fp64 column sum rounded once' % groups
        for clamp in (False, True):
            two = k_finalize(sums, m, c, cs.inp, clamp, y=cs.y, yp=cs.p, extra=_bits_of(0.5, dev), mul=2.0)
            one = k_finalize(None, m, c, cs.inp, clamp, y=cs.y, yp=cs.p, extra=_bits_of(0.5, dev), mul=2.0, partial=partial)
            one.same_bits(two, 'bn_finalize_from_partial_ex(%d rows, clamp=%d) vs the two launches' % (groups, clamp))
    print('BN-A partial %dx%d: bit-identical for 1, 7, %d row groups' % (m, c, min(300, m)))


# ---- B: the backward chain with non-zero sums --------------------------------------------------------------------------------------------------
def _backward_checks(tag, cs, co, mode, fwd_out, mask, fig, use_ex, want_g, want_bound, n=None, scale_sums=1.0):
    m, c = cs.m, cs.c
    n = float(m) if n is None else n
    gamma = cs.inp.gamma
    sums, g_amax, bound = k_bwd_reduce(cs.dout, cs.y, cs.p, co, mode, fwd_out, mask, gamma=gamma, n=n, use_ex=use_ex, want_bound=want_bound)
    ref_mask = None if mode == 'none' else (fwd_out > 0)
    g, sgx, sg, _, xh = B.backward64(cs.dout, ref_mask, cs.y, co.mean, co.invstd, gamma, n)
    dsgx, dsg = B.d_bwd_sums(g, xh)
    _check('%s bn_bwd_reduce(%s): sum g xhat' % (tag, mode), (sums[:c].double() - sgx).abs(), dsgx, fig)
    _check('%s bn_bwd_reduce(%s): sum g' % (tag, mode), (sums[c:].double() - sg).abs(), dsg, fig)
    if g_amax is not None:
        assert torch.equal(_f32(g_amax), g.abs().max().float().reshape(1)), '%s bn_bwd_reduce_ex(%s): g_amax is not max|g|' % (tag, mode)
    if scale_sums != 1.0:
        sums = sums * scale_sums                  # what a rank of three sees: all-reduced sums, n = 3 M
    dy, gv, amax = k_bwd_apply(cs.dout, cs.y, cs.p, co, gamma, sums, n, mode, fwd_out, mask, want_g=want_g, want_amax=True, use_ex=use_ex)
    want = B.backward64(cs.dout, ref_mask, cs.y, co.mean, co.invstd, gamma, n, sums=(sums[:c], sums[c:]))[3]
    _check('%s bn_bwd_apply(%s): dy' % (tag, mode), (dy.double() - want).abs(), B.dy_elem_bound(gamma, co.invstd, g, sums[:c], sums[c:], xh, n), fig)
    assert torch.equal(_f32(amax), dy.abs().max().reshape(1)), '%s bn_bwd_apply(%s): amax_dy is not max|dy| of the stored dy' % (tag, mode)
    if want_g:
        bad = torch.nonzero(gv.double() != g)
        assert bad.numel() == 0, '%s bn_bwd_apply(%s): g_out differs from dout * (out > 0) at %s' % (tag, mode, bad[:1].tolist())
    if bound is not None:
        _bound_check('%s bn_bwd_reduce_ex(%s): dy_bound_out' % (tag, mode), bound,
                     B.dy_bound64(gamma, co.invstd, _f32(g_amax).item(), (sums[:c], sums[c:]), n), dy.abs().max().item(), 8, fig)
    return sums


@pytest.mark.parametrize('m,c,extra', B.SHAPES)
def test_backward_chain_with_nonzero_sums(dev, m, c, extra):
    """pylc_bn_bwd_reduce / _ex -> pylc_bn_bwd_apply / _ex with every mask source; the reference mask is the STORED forward output's
    out > 0 in every mode, which pins "the recomputed mask is bit-identical to the forward" without a kink exclusion."""
    cs = _case(dev, m, c, extra)
    co = cs.coef()
    fig = {}
    y_out = cs.forward('relu')[0]
    r_out = cs.forward('res')[0]
    s_y = _backward_checks('', cs, co, 'y', y_out, None, fig, use_ex=False, want_g=False, want_bound=False)
    _backward_checks('', cs, co, 'out', r_out, None, fig, use_ex=True, want_g=True, want_bound=True)
    _backward_checks('', cs, co, 'none', None, None, fig, use_ex=False, want_g=True, want_bound=False)
    s_y2 = _backward_checks('ex', cs, co, 'y', y_out, None, fig, use_ex=True, want_g=True, want_bound=True)
    assert torch.equal(s_y, s_y2), 'bn_bwd_reduce_ex(dy_bound_out): the sums differ from pylc_bn_bwd_reduce'
    if c % 8 == 0:
        b_out, _, mask = cs.forward('bits')
        _backward_checks('', cs, co, 'bits', b_out, mask, fig, use_ex=True, want_g=True, want_bound=True)
    # what a rank of three sees: n = 3 M and the sums of three ranks
    _backward_checks('n=3M', cs, co, 'y', y_out, None, fig, use_ex=False, want_g=False, want_bound=False, n=3.0 * m, scale_sums=3.0)
    # sums aimed at the adjacent (gamma-grad, beta-grad) slots of a flat arena: nothing outside the 2C floats changes
    arena = torch.full((2 * c + 96,), NAN, device=dev)
    k_bwd_reduce(cs.dout, cs.y, cs.p, co, 'y', y_out, sums_view=arena[32:32 + 2 * c])
    assert torch.isnan(arena[:32]).all() and torch.isnan(arena[32 + 2 * c:]).all(), 'bn_bwd_reduce: wrote outside the 2C floats of the arena'
    assert torch.equal(arena[32:32 + 2 * c], s_y), 'bn_bwd_reduce into an arena: other bits than into its own buffer'
    dy_a = k_bwd_apply(cs.dout, cs.y, cs.p, co, cs.inp.gamma, arena[32:32 + 2 * c], m, 'y', y_out)[0]
    dy_b = k_bwd_apply(cs.dout, cs.y, cs.p, co, cs.inp.gamma, s_y, m, 'y', y_out)[0]
    assert torch.equal(dy_a, dy_b)
    _report('BN-B', '%dx%d+%d' % (m, c, extra), fig)


# ---- C: the op end to end against fp64 autograd, measured against torch's own fp32 BatchNorm -------------------------------------------------
@pytest.mark.parametrize('m,c,extra', B.SHAPES)
def test_op_against_fp64_autograd_per_channel(dev, m, c, extra):
    """ops.bn_act (residual + ReLU) against F.batch_norm + autograd in fp64, per channel: no worse than 4x torch's own fp32 BatchNorm on the
    device (the margin of tests/test_ops_gpu.py::test_bn_train_mean_1e3_sigma for another summation order) plus the bounds of tests/_bn.py."""
    from pylc_amd import ops
    i = B.make_inputs(m, c)
    nchw = lambda t: t.t().reshape(1, c, m, 1)
    S1, S2, SA, n = B.stats64(i.y)
    ref = B.coeffs64(S1, S2, n, i.gamma, i.beta, EPS, False)
    refined = B.needs_refine(S1, S2, n)[0]
    dvar = B.d_var(S1, S2, SA, n, refined)
    rel = B.d_invstd_rel(dvar, ref.var, EPS, False)
    dmean = B.d_mean(S1, SA, n, ref.mean, refined)
    dscale = B.d_scale(ref.scale, rel)
    dshift = B.d_shift(ref, dmean, dscale)
    pre = i.y.double() * ref.scale + ref.shift + i.res.double()
    out_bound = B.apply_bound(i.y, ref.scale, ref.shift, i.res) + i.y.double().abs() * dscale + dshift
    near = pre.abs() <= out_bound                 # may fall on either side of the ReLU: no part in the gradient comparison
    assert near.double().mean().item() <= 1e-3
    print('BN-C %dx%d+%d share of elements within the apply bound of the ReLU kink: %.2g' % (m, c, extra, near.double().mean().item()))
    dout = i.dout * (~near).float()
    # fp64
    y64, g64, b64, r64 = (nchw(t.double()).clone().requires_grad_(True) if t.dim() == 2 else t.double().clone().requires_grad_(True)
                          for t in (i.y, i.gamma, i.beta, i.res))
    rm64, rv64 = i.rm.double().clone(), i.rv.double().clone()
    o64 = F.relu(F.batch_norm(y64, rm64, rv64, g64, b64, True, MOM, B.eps64(EPS)) + r64)
    o64.backward(nchw(dout.double()))
    # torch fp32 on the device
    yt, gt, bt, rt = (nchw(t).to(dev).clone().requires_grad_(True) if t.dim() == 2 else t.to(dev).clone().requires_grad_(True)
                      for t in (i.y, i.gamma, i.beta, i.res))
    rmt, rvt = i.rm.to(dev), i.rv.to(dev)
    ot = F.relu(F.batch_norm(yt, rmt, rvt, gt, bt, True, MOM, EPS) + rt)
    ot.backward(nchw(dout).to(dev))
    # the op; the rows at pitch C + extra inside a wider NHWC buffer
    ybuf = torch.full((1, c + extra, m, 1), NAN, device=dev).contiguous(memory_format=torch.channels_last)
    ybuf[:, :c] = nchw(i.y).to(dev)
    yd = ybuf[:, :c].detach().requires_grad_(True)
    gd, bd = i.gamma.to(dev).requires_grad_(True), i.beta.to(dev).requires_grad_(True)
    rd = nchw(i.res).to(dev).contiguous(memory_format=torch.channels_last).requires_grad_(True)
    rmd, rvd = i.rm.to(dev), i.rv.to(dev)
    od = ops.bn_act(yd, gd, bd, rmd, rvd, rd, True, True)
    od.backward(nchw(dout).to(dev).contiguous(memory_format=torch.channels_last))
    assert torch.isnan(ybuf[:, c:]).all()
    rows = lambda t: t.detach().double().cpu().reshape(c, m).t()
    # per-channel bounds of the chain: each stage's own bound plus the first-order effect of the coefficient errors before it
    mask = pre > 0
    g, sgx, sg, dy_ref, xh = B.backward64(dout, mask, i.y, ref.mean, ref.invstd, i.gamma, n)
    dsgx, dsg = B.d_bwd_sums(g, xh)
    k = (i.gamma.double() * ref.invstd).abs()
    dsgx_chain = dsgx + sgx.abs() * rel + g.abs().sum(0) * ref.invstd * dmean
    dy_bound = (B.dy_elem_bound(i.gamma, ref.invstd, g, sgx, sg, xh, n).amax(0) + k / n * (xh.abs().amax(0) * dsgx_chain + dsg)
                + 2 * rel * (dy_ref.abs().amax(0) + k * xh.abs().amax(0) * sgx.abs() / n) + k * ref.invstd * dmean * sgx.abs() / n)
    fig = {}
    items = (('out', rows(od), rows(ot), rows(o64), out_bound.amax(0)),
             ('dy', rows(yd.grad), rows(yt.grad), rows(y64.grad), dy_bound),
             ('dres', rows(rd.grad), rows(rt.grad), rows(r64.grad), torch.zeros(c, dtype=torch.float64)),
             ('dgamma', gd.grad.double().cpu()[None], gt.grad.double().cpu()[None], g64.grad[None], dsgx_chain),
             ('dbeta', bd.grad.double().cpu()[None], bt.grad.double().cpu()[None], b64.grad[None], dsg),
             ('running_mean', rmd.double().cpu()[None], rmt.double().cpu()[None], rm64[None], B.d_running(i.rm, ref.mean, dmean, MOM)),
             ('running_var', rvd.double().cpu()[None], rvt.double().cpu()[None], rv64[None],
              B.d_running(i.rv, ref.unbiased, dvar * (n / (n - 1.0)), MOM)))
    for name, ours, theirs, want, bound in items:
        e_ours, e_torch = (ours - want).abs().amax(0), (theirs - want).abs().amax(0)
        cap = 4.0 * e_torch + bound
        worst = (e_ours / cap.clamp(min=1e-300)).max().item() if (cap > 0).any() else 0.0
        print('BN-C %dx%d+%d %-12s ours/torch %.3g / %.3g (max over channels)  worst ours/(4 torch + bound) %.3f' %
              (m, c, extra, name, e_ours.max().item(), e_torch.max().item(), worst))
        _check('bn_act end to end: %s per channel' % name, e_ours, cap, fig)
    _report('BN-C', '%dx%d+%d' % (m, c, extra), fig)


# ---- D: synchronised BatchNorm with simulated ranks --------------------------------------------------------------------------------------------
def _general_sync(m_per_rank, c, w):
    i = B.make_inputs(m_per_rank * w, c)
    return B.SyncInputs(i.y, i.y, torch.zeros(c), i.gamma, i.beta, i.dout, (m_per_rank,) * w)


def _invstd_interval(var, dvar, clamp):
    """Where dvar is no small fraction of var + eps the first-order bound is not a bound: the interval of invstd over var +- dvar, (1 +- u)."""
    e = B.eps64(EPS)
    f = (lambda v: v.clamp(min=e).rsqrt()) if clamp else (lambda v: (v + e).rsqrt())
    return f(var + dvar) * (1 - 2 * B.U), f((var - dvar).clamp(min=0.0)) * (1 + 2 * B.U)


def _sync_run(dev, s, run, clamp, extra, fig, tag):
    """One SyncBN forward and backward over len(s.shards) simulated ranks against the whole concatenated batch in fp64.
    run: 'shift' -- stat_shift set for ALL channels (K = 5 + |N| on the stat_shift channels of the case, 0 elsewhere), the sums taken over
    t = y - K and y handed to the refinement; 'plain' -- no stat_shift, sums over y (the stat_shift channels of the case are then ordinary
    ill-conditioned ones, mean ~ 12 sigma, and refine); 'noy' -- as 'shift' with y = NULL, no refinement source."""
    c = s.y.shape[1]
    p = c + extra
    w = len(s.shards)
    n = float(sum(s.shards))
    gamma, beta = s.gamma.to(dev), s.beta.to(dev)
    inp = B.Inputs(None, gamma, beta, None, None, torch.zeros(c, device=dev), torch.ones(c, device=dev))
    use_shift = run != 'plain'
    K = s.K.to(dev) if use_shift else None
    src = s.t if use_shift else s.y
    ys = [_pitched(q.to(dev), p)[1] for q in torch.split(s.y, list(s.shards))]
    ts = [_pitched(q.to(dev), p)[1] for q in torch.split(src, list(s.shards))]
    douts = [_pitched(q.to(dev), p)[1] for q in torch.split(s.dout, list(s.shards))]
    total = None
    for r in range(w):
        sums = k_stats(ts[r], p)
        mom = k_local_moments(sums, s.shards[r], c, ys[r] if run != 'noy' else None, p, K)
        assert mom[2 * c].item() == s.shards[r], '%s: moments[2C] of rank %d is not its row count' % (tag, r)
        total = mom.clone() if total is None else total + mom          # the SUM all-reduce
    assert total[2 * c].item() == n
    co = k_finalize_moments(total, total[2 * c].item(), c, inp, clamp, K=K, extra=None, mul=1.0)
    # the whole concatenated batch in fp64
    tall = src.to(dev)
    S1, S2, SA, _ = B.stats64(tall)
    ref = B.coeffs64(S1, S2, n, gamma, beta, EPS, clamp, K=K)
    refined, border = B.needs_refine(S1, S2, n)
    assert not border.any()
    if run == 'noy':
        refined = torch.zeros_like(refined)
    # a rank that refines hands over moments with no fp32 summation error; one that does not, the error of d_sums: the unrefined bound
    # covers a channel that is well-conditioned globally whatever its ranks did
    dvar = B.d_var(S1, S2, SA, n, refined)
    loose = dvar > 0.01 * (ref.var + B.eps64(EPS))      # 'noy', channels 8-10: only required to stay inside the unrefined interval
    if loose.any():
        assert run == 'noy' and c == 16 and set(torch.nonzero(loose).flatten().tolist()) <= {8, 9, 10}, (tag, loose)
        lo, hi = _invstd_interval(ref.var, dvar, clamp)
        got = co.invstd.double()
        assert ((got >= lo) & (got <= hi))[loose].all(), '%s: invstd of an unrefined ill-conditioned channel left [%s, %s]: %s' % (tag, lo[loose], hi[loose], got[loose])
    amb = B.clamp_ambiguous(dvar, ref.var, EPS) if clamp else torch.zeros_like(loose)
    assert not (amb & ~loose).any(), (tag, amb)
    _coef_checks(tag + ' bn_finalize_moments', co, ref, S1, S2, SA, n, clamp, refined, inp, fig, skip=loose)
    if c == 16 and run != 'noy':
        # the constant channel: variance exactly 0
        want = torch.tensor(B.eps64(EPS), dtype=torch.float64).rsqrt().float().item()
        assert co.invstd[11].item() == want, '%s: invstd of the constant channel is %r, not eps^-1/2 rounded (%r)' % (tag, co.invstd[11].item(), want)
    _bound_check(tag + ' bn_finalize_moments: bound_out', co.bound, B.samuelson_bound64(gamma, beta, n, 0.0, 1.0), 0.0, 4, fig)
    # forward apply and backward per rank, with the global coefficients
    local, g_amaxes, outs = [], [], []
    for r in range(w):
        out = k_apply(ys[r], p, co, None, relu=True)[0]
        outs.append(out)
        pre = ys[r].double() * co.scale.double() + co.shift.double()
        _check('%s bn_apply(rank %d): out' % (tag, r), (out.double() - pre.clamp(min=0.0)).abs(), B.apply_bound(ys[r], co.scale, co.shift), fig)
        assert _f32(co.bound).item() >= _exact_amax(out, B.apply_bound(ys[r], co.scale, co.shift)), '%s: bound_out below max|out| of rank %d' % (tag, r)
        sm, ga, _ = k_bwd_reduce(douts[r], ys[r], p, co, 'y', out, gamma=gamma, n=n, use_ex=True)
        local.append(sm)
        g_amaxes.append(ga)
    sums = local[0].clone()
    for r in range(1, w):
        sums = sums + local[r]                                         # fp32, in rank order
    yall, dall, oall = torch.cat(ys), torch.cat(douts), torch.cat(outs)
    g, sgx, sg, _, xh = B.backward64(dall, oall > 0, yall, co.mean, co.invstd, gamma, n)
    dsgx, dsg = B.d_bwd_sums(g, xh, extra_adds=w - 1)
    _check(tag + ' all-reduced bn_bwd_reduce_ex: sum g xhat', (sums[:c].double() - sgx).abs(), dsgx, fig)
    _check(tag + ' all-reduced bn_bwd_reduce_ex: sum g', (sums[c:].double() - sg).abs(), dsg, fig)
    if clamp:
        # ops/bn.py: where the clamp is active invstd does not depend on the batch and dy loses its xhat term
        thr = torch.tensor(EPS, dtype=torch.float32, device=dev).double().rsqrt().float()
        sums = torch.cat((sums[:c] * (co.invstd < thr), sums[c:]))
    L = _L()
    for r in range(w):
        bound = _zero_u32(dev)
        L.check(L.lib.pylc_bn_bwd_bound(L.ptr(sums), L.ptr(gamma), L.ptr(co.invstd), n, c, L.ptr(g_amaxes[r]), L.ptr(bound), L.stream()))
        dy = k_bwd_apply(douts[r], ys[r], p, co, gamma, sums, n, 'y', outs[r], use_ex=True)[0]
        assert torch.isfinite(dy).all(), '%s: dy of rank %d is not finite' % (tag, r)
        gr, _, _, want, xr = B.backward64(douts[r], outs[r] > 0, ys[r], co.mean, co.invstd, gamma, n, sums=(sums[:c], sums[c:]))
        _check('%s bn_bwd_apply_ex(rank %d): dy' % (tag, r), (dy.double() - want).abs(), B.dy_elem_bound(gamma, co.invstd, gr, sums[:c], sums[c:], xr, n), fig)
        assert torch.equal(_f32(g_amaxes[r]), gr.abs().max().float().reshape(1))
        _bound_check('%s bn_bwd_bound(rank %d): bound' % (tag, r), bound,
                     B.dy_bound64(gamma, co.invstd, _f32(g_amaxes[r]).item(), (sums[:c], sums[c:]), n), dy.abs().max().item(), 8, fig)
    return co


SYNC16 = [((288,) * w, run) for w in (1, 2, 3, 4) for run in ('shift', 'plain', 'noy')] + [((288, 150, 7), run) for run in ('shift', 'plain', 'noy')]


@pytest.mark.parametrize('shards,run', SYNC16)
def test_syncbn_simulated_ranks_16_channels(dev, shards, run):
    """The conditioning case (tests/_bn.py make_sync16): refined on every rank, on some ranks, alternating rank means, a constant channel,
    variances on both sides of the clamp, stat_shift channels."""
    fig = {}
    s = B.make_sync16(shards)
    for clamp in (False, True):
        _sync_run(dev, s, run, clamp, 4, fig, 'W=%d %s clamp=%d' % (len(shards), run, clamp))
    _report('BN-D', 'shards=%s %s' % (shards, run), fig)


@pytest.mark.parametrize('m,c,w', [(1, 256, 2), (1, 256, 4), (75, 20, 1), (75, 20, 2), (75, 20, 3), (75, 20, 4)])
def test_syncbn_simulated_ranks_general(dev, m, c, w):
    """One row per rank (the ASPP image-pool BatchNorm at one tile per rank, legal exactly when a group is set) and an odd vector count."""
    fig = {}
    s = _general_sync(m, c, w)
    for clamp in (False, True):
        _sync_run(dev, s, 'plain', clamp, 0, fig, 'W=%d %dx%d clamp=%d' % (w, m, c, clamp))
    _report('BN-D', '%d x (%dx%d)' % (w, m, c), fig)


@pytest.mark.parametrize('with_y', [True, False])
@pytest.mark.parametrize('with_shift', [True, False])
def test_syncbn_one_rank_has_the_bits_of_finalize_ex(dev, with_y, with_shift):
    """The header: "With one rank the result equals pylc_bn_finalize_ex bit for bit" -- every output, bound_out included; and
    pylc_bn_bwd_bound on the local sums equals dy_bound_out of pylc_bn_bwd_reduce_ex BIT FOR BIT (the two kernels evaluate the same fp32
    expression with its three terms in the same order)."""
    L = _L()
    s = B.make_sync16((288,))
    c, p, n = 16, 20, 288
    gamma, beta = s.gamma.to(dev), s.beta.to(dev)
    inp = B.Inputs(None, gamma, beta, None, None, 0.1 * gamma, 1 + 0.1 * beta.abs())
    K = s.K.to(dev) if with_shift else None
    y = _pitched(s.y.to(dev), p)[1]
    t = _pitched((s.t if with_shift else s.y).to(dev), p)[1]
    dout = _pitched(s.dout.to(dev), p)[1]
    sums = k_stats(t, p)
    for clamp in (False, True):
        extra = _bits_of(1.25, dev)
        one = k_finalize(sums, n, c, inp, clamp, y=y if with_y else None, yp=p, K=K, extra=extra, mul=2.0)
        mom = k_local_moments(sums, n, c, y if with_y else None, p, K)
        two = k_finalize_moments(mom, n, c, inp, clamp, K=K, extra=extra, mul=2.0)
        two.same_bits(one, 'local_moments + finalize_moments vs finalize_ex (y=%d shift=%d clamp=%d)' % (with_y, with_shift, clamp))
        out = k_apply(y, p, one, None, relu=True)[0]
        sm, g_amax, b1 = k_bwd_reduce(dout, y, p, one, 'y', out, gamma=gamma, n=n, want_bound=True)
        b2 = _zero_u32(dev)
        L.check(L.lib.pylc_bn_bwd_bound(L.ptr(sm), L.ptr(gamma), L.ptr(one.invstd), float(n), c, L.ptr(g_amax), L.ptr(b2), L.stream()))
        assert torch.equal(b1, b2), 'bn_bwd_bound %r vs dy_bound_out %r' % (_f32(b2).item(), _f32(b1).item())
    print('BN-D one rank: nine outputs and the dy bound bit-identical (y=%d shift=%d)' % (with_y, with_shift))


# ---- E: the combine stage alone (EXPERIMENTAL=1 builds) ----------------------------------------------------------------------------------------
@needs_experimental()
@pytest.mark.parametrize('rows', [1, 300])
def test_bwd_sums_from_partial_equals_column_sum_and_bound(dev, rows):
    L = _L()
    c, n = 48, 363.0
    i = B.make_inputs(363, c)
    g = torch.Generator().manual_seed(rows)
    partial = torch.randn(rows, 2 * c, generator=g).to(dev)
    gamma, invstd = i.gamma.to(dev), (1 + 0.1 * i.beta.abs()).to(dev)
    g_amax = _bits_of(3.5, dev)
    ar = _Arena(dev)
    ar.take(2 * c)
    sums, = ar.build()
    bound = _zero_u32(dev)
    L.check(L.lib.pylc_bn_bwd_sums_from_partial(L.ptr(partial), rows, c, L.ptr(sums), L.ptr(gamma), L.ptr(invstd), n, L.ptr(g_amax), L.ptr(bound),
                                                L.stream()))
    assert ar.gaps_clean()
    assert torch.equal(sums, partial.double().sum(0).float()), 'bn_bwd_sums_from_partial: not the fp64 column sum rounded once'
    b2 = _zero_u32(dev)
    L.check(L.lib.pylc_bn_bwd_bound(L.ptr(sums), L.ptr(gamma), L.ptr(invstd), n, c, L.ptr(g_amax), L.ptr(b2), L.stream()))
    assert torch.equal(bound, b2)
    fig = {}
    _bound_check('bn_bwd_sums_from_partial: dy_bound_out', bound, B.dy_bound64(gamma, invstd, 3.5, (sums[:c], sums[c:]), n), 0.0, 8, fig)
    _report('BN-E', '%d rows' % rows, fig)
