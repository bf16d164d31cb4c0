"""The optimiser kernels of pylc_amd/csrc/optim.hip at the C ABI against the fp64 statement and the float32 model of tests/_optim.py (-m gpu;
DESIGN.md section 5.18).  Every buffer sits inside a NaN-filled allocation with 64 guard floats before and after (16-byte aligned); the
guards must still be NaN afterwards; the workspace and out2 are NaN-filled before the call.  The tolerances are the derived bounds of
tests/_optim.py per element and bit equality with the float32 model; none is tuned to the device's output.

Sections print their worst figure as error / bound (1.0 = at the bound):
  OPT-A  pylc_grad_norm_clip: norm and coefficient, clipped / unclipped / zero gradient, n = 1 .. 2 x 2^20 + 3 (the stride loop wraps)
  OPT-B  non-finite gradients: the contract of include/pylc_hip.h (NaN -> norm NaN, coef NaN, every parameter NaN after the step;
         inf -> norm inf, coef 0)
  OPT-C  pylc_adamw_step: p, m, v per element against fp64, and bit for bit against adamw_f32
  OPT-D  pylc_adamw_step_ranges: bit-equal to pylc_adamw_step, seg_amax_bits = the maxima of the stored p, five segment tables
  OPT-E  pylc_sgd_step: against fp64 and bit for bit against sgd_f32; step 1 over a NaN-filled buffer
  OPT-F  FlatAdamW / FlatSGD with clip=None (coef == NULL through Python) against fp64
The implementing run on an MI355X, worst over the cases of each section:
  OPT-A  norm 0.124, coef 0.140 of the bound (L = 2 at the largest n: 0.059 / 0.062); g = 0 gives norm 0, coef 1 at every n
  OPT-B  as stated, for a NaN in a vector, in the tail and at n = 3; +inf, -inf and n = 2: one NaN, everything else bit-equal to coef 0
  OPT-C  p 0.725, m 0.967, v 0.990 (step 1000, n = 4197379); p, m, v BIT-EQUAL to adamw_f32 in all nine cases
  OPT-D  bit-equal to pylc_adamw_step and to adamw_f32, every segment maximum exact, twelve table / case pairs and the 4097-chunk case
  OPT-E  p 0.998, buf 0.984; bit-equal to sgd_f32 in all seven cases; no NaN out of the NaN-filled buffer at step 1
  OPT-F  AdamW 0.312, SGD 0.883
No bit-equality exception was found.  Blindness check: with a scratch library whose pylc_adamw_step runs with beta2 = 0.99 (kernel and
bias correction alike) all nine OPT-C cases fail and tests/test_ops_gpu.py::test_adamw_clip still passes.
"""
import numpy as np
import pytest
import torch

from tests import _optim as O

pytestmark = pytest.mark.gpu

NAN = float('nan')
GUARD = 64


def _L():
    from pylc_amd import lib as L
    L.init()
    return L


class _Buf:
    """n floats inside a NaN-filled allocation, GUARD floats on either side."""

    def __init__(self, dev, a=None, n=None):
        n = a.size if a is not None else n
        self.n = n
        self.whole = torch.full((n + 2 * GUARD,), NAN, device=dev)
        self.t = self.whole[GUARD:GUARD + n]
        if a is not None:
            self.t.copy_(torch.from_numpy(np.ascontiguousarray(a, dtype=np.float32)))
        assert self.t.data_ptr() % 16 == 0

    def np(self, what):
        assert torch.isnan(self.whole[:GUARD]).all() and torch.isnan(self.whole[GUARD + self.n:]).all(), '%s: a guard float was written' % what
        return self.t.cpu().numpy()


def _coef_buf(dev, coef):
    """out2-shaped [., coef] with a NaN in slot 0: the update kernels must read slot 1 only.  None -> NULL."""
    if coef is None:
        return None
    return torch.tensor([NAN, coef], device=dev)


def _ratio(got, ref, bound, what):
    err = np.abs(got.astype(np.float64) - ref)
    assert not np.isnan(err).any(), '%s: NaN' % what
    bad = err > bound
    if bad.any():
        i = int(np.argmax(np.where(bad, err - bound, -1.0)))
        raise AssertionError('%s: element %d is %.9g, fp64 says %.9g: err %.4g > bound %.4g; %d over the bound' %
                             (what, i, got[i], ref[i], err[i], bound[i], int(bad.sum())))
    live = bound > 0
    return float((err[live] / bound[live]).max()) if live.any() else 0.0


def _same_bits(got, want, what):
    g, w = got.view(np.uint32), np.ascontiguousarray(want, dtype=np.float32).view(np.uint32)
    both_nan = np.isnan(got) & np.isnan(want)
    ne = (g != w) & ~both_nan
    if ne.any():
        i = int(np.nonzero(ne)[0][0])
        raise AssertionError('%s: element %d is %#010x (%.9g), the float32 model says %#010x (%.9g); %d of %d differ' %
                             (what, i, g[i], got[i], w[i], want[i], int(ne.sum()), g.size))


# ---- OPT-A  pylc_grad_norm_clip ------------------------------------------------------------------------------------------------------------
def _clip(L, dev, g):
    gb = _Buf(dev, g)
    out2, ws = _Buf(dev, n=2), _Buf(dev, n=L.lib.pylc_sqnorm_workspace_floats(g.size))
    return gb, out2, ws


def _run_clip(L, gb, out2, ws, max_norm, what):
    out2.t.fill_(NAN)
    ws.t.fill_(NAN)
    L.check(L.lib.pylc_grad_norm_clip(L.ptr(gb.t), gb.n, max_norm, L.ptr(out2.t), L.ptr(ws.t), L.stream()))
    ws.np(what + ': workspace')
    gb.np(what + ': g')
    return out2.np(what + ': out2')


@pytest.mark.parametrize('n', O.CLIP_NS)
def test_opta_norm_and_clip_coefficient(dev, n):
    L = _L()
    assert L.lib.pylc_sqnorm_workspace_floats(n) == O.NORM_BLOCKS
    g, _ = O.norm_inputs(n)
    norm, _ = O.clip_ref(g, 1.0)
    bn = O.norm_bound(norm, n)
    gb, out2, ws = _clip(L, dev, g)
    worst = {}
    for name, max_norm in (('clipped', 0.5 * norm), ('unclipped', 2.0 * norm)):
        what = 'OPT-A n %d %s' % (n, name)
        got = _run_clip(L, gb, out2, ws, max_norm, what)
        _, coef = O.clip_ref(g, max_norm)
        worst['norm'] = _ratio(got[:1], np.array([norm]), np.array([bn]), what + ': norm')
        if name == 'unclipped':
            assert got[1] == 1.0, what + ': coef %r' % got[1]
        else:
            assert coef < 1.0
            worst['coef'] = _ratio(got[1:], np.array([coef]), np.array([O.coef_bound(norm, bn, max_norm)]), what + ': coef')
    zb, out2z, wsz = _clip(L, dev, np.zeros(n, np.float32))
    got = _run_clip(L, zb, out2z, wsz, 0.5, 'OPT-A n %d zero' % n)
    assert got[0] == 0.0 and got[1] == 1.0
    print('OPT-A n %7d (L %d): err / bound  %s;  g = 0: norm 0, coef 1' % (n, O.norm_trips(n)[0], '  '.join('%s %.3f' % kv for kv in worst.items())))


# ---- OPT-B  non-finite gradients -------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('n,at', [(100003, 777), (100003, 100002), (3, 1)])
def test_optb_nan_gradient_poisons_the_whole_step(dev, n, at):
    """include/pylc_hip.h: a NaN anywhere in g gives out[0] = NaN and out[1] = NaN, and the step that follows turns every element of p, m, v
    into NaN (torch's clip_grad_norm_ multiplies every gradient by the NaN coefficient)."""
    L = _L()
    x = O.adamw_inputs(n, 2, None)
    g = x.g.copy()
    g[at] = np.nan
    gb, out2, ws = _clip(L, dev, g)
    got = _run_clip(L, gb, out2, ws, 0.5, 'OPT-B nan')
    assert np.isnan(got[0]) and np.isnan(got[1])
    pb, mb, vb = _Buf(dev, x.p), _Buf(dev, x.m), _Buf(dev, x.v)
    L.check(L.lib.pylc_adamw_step(L.ptr(pb.t), L.ptr(gb.t), L.ptr(mb.t), L.ptr(vb.t), n, L.ptr(out2.t), 1e-2, 0.9, 0.999, 1e-8, 0.1, 2, L.stream()))
    for name, b in (('p', pb), ('m', mb), ('v', vb)):
        assert np.isnan(b.np('OPT-B nan ' + name)).all(), 'OPT-B: finite %s after a step with a NaN gradient' % name
    sp, sb = _Buf(dev, x.p), _Buf(dev, x.m)
    L.check(L.lib.pylc_sgd_step(L.ptr(sp.t), L.ptr(gb.t), L.ptr(sb.t), n, L.ptr(out2.t), 1e-2, 0.9, 2, L.stream()))
    assert np.isnan(sp.np('OPT-B nan sgd p')).all() and np.isnan(sb.np('OPT-B nan sgd buf')).all()
    print('OPT-B n %d NaN at %d: norm NaN, coef NaN, p / m / v / buf all NaN after the step' % (n, at))


@pytest.mark.parametrize('n,at,val', [(100003, 5, np.inf), (100003, 100001, -np.inf), (2, 0, np.inf)])
def test_optb_infinite_gradient_gives_coef_zero(dev, n, at, val):
    """include/pylc_hip.h: an infinity and no NaN gives out[0] = +inf, out[1] = 0; the step sees g * 0 -- zero for the finite elements, NaN
    at the infinite one: exactly the float32 model fed with coef = 0."""
    L = _L()
    x = O.adamw_inputs(n, 2, None)
    g = x.g.copy()
    g[at] = val
    gb, out2, ws = _clip(L, dev, g)
    got = _run_clip(L, gb, out2, ws, 0.5, 'OPT-B inf')
    assert got[0] == np.inf and got[1] == 0.0
    pb, mb, vb = _Buf(dev, x.p), _Buf(dev, x.m), _Buf(dev, x.v)
    L.check(L.lib.pylc_adamw_step(L.ptr(pb.t), L.ptr(gb.t), L.ptr(mb.t), L.ptr(vb.t), n, L.ptr(out2.t), 1e-2, 0.9, 0.999, 1e-8, 0.1, 2, L.stream()))
    with np.errstate(invalid='ignore'):
        want = O.adamw_f32(x.p, g, x.m, x.v, 0.0, 1e-2, 0.9, 0.999, 1e-8, 0.1, 2)
    for name, b, w in zip('pmv', (pb, mb, vb), want):
        a = b.np('OPT-B inf ' + name)
        assert np.isnan(a[at]) and np.isnan(w[at]) and int(np.isnan(a).sum()) == 1
        _same_bits(a, w, 'OPT-B inf ' + name)
    print('OPT-B n %d %r at %d: norm inf, coef 0, one NaN, the rest bit-equal to the model with coef 0' % (n, val, at))


# ---- OPT-C  pylc_adamw_step ------------------------------------------------------------------------------------------------------------------
def _adamw(L, dev, x, n, kw, ranges=None):
    pb, gb, mb, vb = _Buf(dev, x.p[:n]), _Buf(dev, x.g[:n]), _Buf(dev, x.m[:n]), _Buf(dev, x.v[:n])
    cb = _coef_buf(dev, kw['coef'])
    args = (L.ptr(pb.t), L.ptr(gb.t), L.ptr(mb.t), L.ptr(vb.t), n, L.ptr(cb), kw['lr'], kw['b1'], kw['b2'], kw['eps'], kw['wd'], kw['step'])
    amax = None
    if ranges is None:
        L.check(L.lib.pylc_adamw_step(*args, L.stream()))
    else:
        seg = torch.from_numpy(np.asarray(ranges, dtype=np.int64)).to(dev)
        count = len(ranges) - 1
        amax = torch.full((count + 2 * GUARD,), -1, dtype=torch.int32, device=dev)
        L.check(L.lib.pylc_adamw_step_ranges(*args, L.ptr(seg), count, L.ptr(amax[GUARD:]), L.stream()))
        a = amax.cpu().numpy()
        assert (a[:GUARD] == -1).all() and (a[GUARD + count:] == -1).all(), 'adamw_step_ranges wrote beside seg_amax_bits[count]'
        amax = a[GUARD:GUARD + count].view(np.uint32)
    gb.np('adamw: g')
    return pb.np('adamw: p'), mb.np('adamw: m'), vb.np('adamw: v'), amax


_adam_inputs = {}


def _case_inputs(case):
    """Inputs, fp64 reference, bounds and float32 model of a case, computed once and left unchanged."""
    if case not in _adam_inputs:
        kw = O.adamw_case_args(case)
        x = O.adamw_inputs(case[-1], case[0], case[4])
        _adam_inputs[case] = (kw, x, O.adamw_ref(x.p, x.g, x.m, x.v, **kw), O.adamw_bounds(x.p, x.g, x.m, x.v, **kw),
                              O.adamw_f32(x.p, x.g, x.m, x.v, **kw))
    return _adam_inputs[case]


@pytest.mark.parametrize('case', O.ADAMW_CASES, ids=lambda c: 'step%d-n%d' % (c[0], c[-1]))
def test_optc_adamw_step(dev, case):
    L = _L()
    kw, x, ref, bnd, model = _case_inputs(case)
    n = case[-1]
    got = _adamw(L, dev, x, n, kw)[:3]
    worst = {}
    for name, a, r, d, w in zip('pmv', got, ref, bnd, model):
        what = 'OPT-C %s: %s' % (case, name)
        assert np.isfinite(a).all(), what
        worst[name] = _ratio(a, r, d, what)
    for name, a, w in zip('pmv', got, model):
        _same_bits(a, w, 'OPT-C %s: %s' % (case, name))
    print('OPT-C step %6d betas %s eps %g lr,wd %s coef %s n %7d: err / bound  %s; bit-equal to adamw_f32' %
          (case[0], case[1], case[2], case[3], case[4], n, '  '.join('%s %.3f' % kv for kv in worst.items())))


# ---- OPT-D  pylc_adamw_step_ranges -----------------------------------------------------------------------------------------------------------
def _tables(n):
    c = O.ADAM_CHUNK
    return {'ragged': np.concatenate([[0], np.cumsum([4, 64, 8192, 12, 20000, 36, 8188, 4])]).tolist() + [n],
            'one': [0, n],
            'quads': list(range(0, 12000, 4)) + [12000] if n >= 12000 else None,          # 3000 four-float segments: 2048 in the first chunk
            'chunk_edges': [0, c, 2 * c, 3 * c + 8] if n >= 3 * c + 8 else None}


@pytest.mark.parametrize('table', ['ragged', 'one', 'quads', 'chunk_edges'])
@pytest.mark.parametrize('case', [O.ADAMW_CASES[6], O.ADAMW_CASES[0], O.ADAMW_CASES[7]], ids=lambda c: 'step%d-coef%s' % (c[0], c[4]))
def test_optd_adamw_step_ranges(dev, case, table):
    L = _L()
    kw, x, ref, bnd, model = _case_inputs(case)
    offs = _tables(100000)[table]
    n = offs[-1]
    assert n % 4 == 0 and all(o % 4 == 0 for o in offs)
    plain = _adamw(L, dev, x, n, kw)
    p, m, v, amax = _adamw(L, dev, x, n, kw, ranges=offs)
    for name, a, b, w in zip('pmv', (p, m, v), plain, model):
        _same_bits(a, b, 'OPT-D %s %s: %s against pylc_adamw_step' % (table, case, name))
        _same_bits(a, w[:n], 'OPT-D %s %s: %s against adamw_f32' % (table, case, name))
    want = np.array([np.abs(p[offs[i]:offs[i + 1]]).max() for i in range(len(offs) - 1)], dtype=np.float32).view(np.uint32)
    assert np.array_equal(amax, want), 'OPT-D %s: segment %d' % (table, int(np.nonzero(amax != want)[0][0]))
    print('OPT-D %-11s n %6d, %4d segments, step %d: bit-equal to pylc_adamw_step, every maximum exact' % (table, n, len(offs) - 1, case[0]))


def test_optd_a_block_takes_a_second_chunk(dev):
    """4097 chunks on 4096 blocks: block 0 walks chunk 0 and chunk 4096.  Against pylc_adamw_step and torch.max only (no fp64 at this size)."""
    L = _L()
    c = O.ADAM_CHUNK
    n = 4097 * c
    gen = torch.Generator(device=dev).manual_seed(11)
    g = torch.randn(n, device=dev, generator=gen) * 0.01
    p0 = torch.randn(n, device=dev, generator=gen) * 0.5
    m0 = torch.randn(n, device=dev, generator=gen) * 0.005
    v0 = torch.rand(n, device=dev, generator=gen) * 1e-4
    p0[n - 5], p0[n - 2] = 55.0, 77.0                               # the maxima of the last two segments lie in the wrapped chunk
    offs = [0, 4, c * 2048 + 12, 4096 * c, n - 4, n]
    seg = torch.tensor(offs, dtype=torch.int64, device=dev)
    coef = _coef_buf(dev, 0.37)
    hyper = (1e-2, 0.9, 0.999, 1e-8, 0.1, 7)
    p1, m1, v1 = p0.clone(), m0.clone(), v0.clone()
    L.check(L.lib.pylc_adamw_step(L.ptr(p1), L.ptr(g), L.ptr(m1), L.ptr(v1), n, L.ptr(coef), *hyper, L.stream()))
    amax = torch.full((len(offs) - 1 + 2,), -1, dtype=torch.int32, device=dev)
    L.check(L.lib.pylc_adamw_step_ranges(L.ptr(p0), L.ptr(g), L.ptr(m0), L.ptr(v0), n, L.ptr(coef), *hyper, L.ptr(seg), len(offs) - 1, L.ptr(amax[1:]),
                                         L.stream()))
    assert torch.equal(p0, p1) and torch.equal(m0, m1) and torch.equal(v0, v1)
    assert amax[0].item() == -1 and amax[-1].item() == -1
    want = torch.stack([p0[offs[i]:offs[i + 1]].abs().max() for i in range(len(offs) - 1)])
    assert torch.equal(amax[1:-1].view(torch.float32), want)
    assert float(want[-1]) > 70.0 and 50.0 < float(want[-2]) < 60.0
    print('OPT-D 4097 chunks (n %d): bit-equal to pylc_adamw_step, 5 maxima exact' % n)


# ---- OPT-E  pylc_sgd_step --------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('case', O.SGD_CASES, ids=lambda c: 'step%d-mu%g-n%d' % (c[0], c[2], c[3]))
def test_opte_sgd_step(dev, case):
    L = _L()
    step, coef, mu, n = case
    lr = 1e-2
    x = O.sgd_inputs(n)
    ref = O.sgd_ref(x.p, x.g, x.buf, coef, lr, mu, step)
    bnd = O.sgd_bounds(x.p, x.g, x.buf, coef, lr, mu, step)
    model = O.sgd_f32(x.p, x.g, x.buf, coef, lr, mu, step)
    pb, gb = _Buf(dev, x.p), _Buf(dev, x.g)
    bb = _Buf(dev, n=n) if step == 1 else _Buf(dev, x.buf)              # step 1: the buffer is NaN-filled and must be ignored
    cb = _coef_buf(dev, coef)
    L.check(L.lib.pylc_sgd_step(L.ptr(pb.t), L.ptr(gb.t), L.ptr(bb.t), n, L.ptr(cb), lr, mu, step, L.stream()))
    gb.np('OPT-E g')
    worst = {}
    for name, b, r, d, w in zip(('p', 'buf'), (pb, bb), ref, bnd, model):
        a = b.np('OPT-E %s: %s' % (case, name))
        assert not np.isnan(a).any(), 'OPT-E %s: NaN in %s' % (case, name)
        worst[name] = _ratio(a, r, d, 'OPT-E %s: %s' % (case, name))
        _same_bits(a, w, 'OPT-E %s: %s' % (case, name))
    print('OPT-E step %d coef %s mu %g n %7d: err / bound  %s; bit-equal to sgd_f32' % (step, coef, mu, n, '  '.join('%s %.3f' % kv for kv in worst.items())))


# ---- OPT-F  the Python optimisers without clipping ---------------------------------------------------------------------------------------------
class _Three(torch.nn.Module):
    def __init__(self):
        super().__init__()
        g = torch.Generator().manual_seed(3)
        self.a = torch.nn.Parameter(torch.randn(5, 3, generator=g))
        self.b = torch.nn.Parameter(torch.randn(7, generator=g))
        self.c = torch.nn.Parameter(torch.randn(2, 9, generator=g))


@pytest.mark.parametrize('kind', ['adamw', 'sgd'])
def test_optf_flat_optimisers_without_clip(dev, kind):
    from pylc_amd.optim import FlatArena, FlatAdamW, FlatSGD
    net = _Three().to(dev)
    arena = FlatArena(net)
    n = arena.numel
    assert n == 16 + 8 + 20
    p0 = arena.p.cpu().numpy().copy()
    g = (0.01 * np.random.RandomState(8).standard_normal(n)).astype(np.float32)
    for prm, o in zip(arena.params, arena.offsets):
        prm.grad.copy_(torch.from_numpy(g[o:o + prm.numel()]).view(prm.shape))
    g = arena.g.cpu().numpy().copy()                                  # the padding between parameters holds zeros
    z = np.zeros(n, np.float32)
    if kind == 'adamw':
        opt = FlatAdamW(arena, lr=1e-2, weight_decay=0.1, clip=None)
        opt.step()
        ref = O.adamw_ref(p0, g, z, z, None, 1e-2, 0.9, 0.999, 1e-8, 0.1, 1)
        bnd = O.adamw_bounds(p0, g, z, z, None, 1e-2, 0.9, 0.999, 1e-8, 0.1, 1)
        got = (arena.p, opt.m, opt.v)
    else:
        opt = FlatSGD(arena, lr=1e-2, momentum=0.9, clip=None)
        opt.step()
        ref = O.sgd_ref(p0, g, z, None, 1e-2, 0.9, 1)
        bnd = O.sgd_bounds(p0, g, z, None, 1e-2, 0.9, 1)
        got = (arena.p, opt.buf)
    worst = max(_ratio(a.cpu().numpy(), r, d, 'OPT-F %s' % kind) for a, r, d in zip(got, ref, bnd))
    assert torch.equal(net.b.detach(), arena.p[16:23]) and net.b.data_ptr() == arena.p[16:].data_ptr()
    print('OPT-F %s, clip None, three parameters: err / bound %.3f' % (kind, worst))
