"""The fp64 BatchNorm yardstick of tests/_bn.py checked without a GPU: against torch.nn.functional.batch_norm + autograd in fp64, against
the reference project's SyncBN rule restated here, the mask layout against a packer written from the header text, and the documented
accumulation (emulated in numpy) against the invstd bound on every input set tests/test_bn_abi_gpu.py uses."""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

from tests import _bn as B

EPS, MOM = 1e-5, 0.1


def _compose(inp, clamp, relu=True, res=True):
    """_bn.py end to end on [M][C] operands in fp64: (out, running mean, running var, dy, dgamma, dbeta, dres)."""
    S1, S2, _, n = B.stats64(inp.y)
    co = B.coeffs64(S1, S2, n, inp.gamma, inp.beta, EPS, clamp)
    pre = inp.y.double() * co.scale + co.shift + (inp.res.double() if res else 0.0)
    out = pre.clamp(min=0.0) if relu else pre
    mask = (pre > 0) if relu else None
    g, sgx, sg, dy, _ = B.backward64(inp.dout, mask, inp.y, co.mean, co.invstd, inp.gamma, n)
    if clamp:          # a clamped invstd does not depend on the batch: nothing flows through the variance there
        live = co.var > B.eps64(EPS)
        dy = B.backward64(inp.dout, mask, inp.y, co.mean, co.invstd, inp.gamma, n, sums=(sgx * live, sg))[3]
    return out, B.running64(inp.rm, co.mean, MOM), B.running64(inp.rv, co.unbiased, MOM), dy, sgx, sg, g


@pytest.mark.parametrize('m,c', [(75, 20), (5, 256), (2, 8), (363, 48)])
def test_composed_equals_torch_batch_norm_fp64(m, c):
    inp = B.make_inputs(m, c)
    out, rm, rv, dy, dgamma, dbeta, dres = _compose(inp, clamp=False)
    e = B.eps64(EPS)
    y = inp.y.double().t().reshape(1, c, m, 1).requires_grad_(True)                # [B, C, H, W] with the rows along H
    ga, be = inp.gamma.double().requires_grad_(True), inp.beta.double().requires_grad_(True)
    r = inp.res.double().t().reshape(1, c, m, 1).requires_grad_(True)
    rm_t, rv_t = inp.rm.double().clone(), inp.rv.double().clone()
    o = F.relu(F.batch_norm(y, rm_t, rv_t, ga, be, True, MOM, e) + r)
    o.backward(inp.dout.double().t().reshape(1, c, m, 1))
    rows = lambda t: t.detach().reshape(c, m).t()
    for name, got, want in (('out', out, rows(o)), ('running_mean', rm, rm_t), ('running_var', rv, rv_t), ('dy', dy, rows(y.grad)),
                            ('dgamma', dgamma, ga.grad), ('dbeta', dbeta, be.grad), ('dres', dres, rows(r.grad))):
        err = ((got - want).abs() / (1.0 + want.abs())).max().item()
        assert err < 1e-12, (name, err)


def test_clamp_variant_equals_the_explicit_formula():
    """inv_std = clamp(var, eps)^-1/2 written out (tests/test_round3_gpu.py::test_bn_clamp_eps_variant) and differentiated by autograd."""
    m, c = 252, 16
    inp = B.make_inputs(m, c)
    y = inp.y.clone()
    y[:, 0] = 1e-3 * inp.res[:, 0]           # variance ~1e-6 < eps
    y[:, 1] = 0.25                           # variance 0
    y[:, 2] = 3e-3 * inp.res[:, 2]           # variance ~1e-5
    inp = inp._replace(y=y)
    out, _, _, dy, dgamma, dbeta, _ = _compose(inp, clamp=True, relu=False, res=False)
    x64 = y.double().requires_grad_(True)
    ga, be = inp.gamma.double().requires_grad_(True), inp.beta.double().requires_grad_(True)
    mean = x64.mean(0, keepdim=True)
    var = ((x64 - mean) ** 2).mean(0, keepdim=True)
    ref = (x64 - mean) * var.clamp(min=B.eps64(EPS)) ** -0.5 * ga + be
    ref.backward(inp.dout.double())
    # the one-pass variance S2/n - mean^2 of stats64 against the two-pass one of the formula: 2^-53 mean^2 / (var + eps) of relative error
    for name, got, want in (('out', out, ref.detach()), ('dy', dy, x64.grad), ('dgamma', dgamma, ga.grad), ('dbeta', dbeta, be.grad)):
        err = ((got - want).abs() / (1.0 + want.abs())).max().item()
        assert err < 1e-10, (name, err)
    assert dy.isfinite().all()


SHARDS = [(288,), (150, 138), (288, 150, 7), (1, 1), (1, 1, 1, 1), (75, 75, 75, 75), (288, 288, 288)]


@pytest.mark.parametrize('shards', SHARDS)
@pytest.mark.parametrize('clamp', [False, True])
def test_summed_shard_moments_give_the_whole_batch_and_the_syncbn_rule(shards, clamp):
    m = sum(shards)
    s = B.make_sync16(shards)
    parts = torch.split(s.y.double(), list(shards))
    mom = [B.stats64(p) for p in parts]
    S1, S2, n = sum(a[0] for a in mom), sum(a[1] for a in mom), sum(a[3] for a in mom)
    assert n == m
    co = B.coeffs64(S1, S2, n, s.gamma, s.beta, EPS, clamp)
    W1, W2, _, wn = B.stats64(s.y)
    whole = B.coeffs64(W1, W2, wn, s.gamma, s.beta, EPS, clamp)
    for f in B.Coeffs._fields:
        a, b = getattr(co, f), getattr(whole, f)
        assert ((a - b).abs() <= 1e-12 * (1.0 + b.abs())).all(), f
    if not clamp:
        return
    # the synchronised BatchNorm of the reference project, in words: every rank sends [sum, sum of squares, count]; from the totals
    # mean = sum / size, sumvar = ssum - sum * mean, inv_std = clamp(sumvar / size, eps)^-1/2, and the running variance takes
    # sumvar / (size - 1)
    size = float(m)
    mean = S1 / size
    sumvar = S2 - S1 * mean
    inv_std = (sumvar / size).clamp(min=B.eps64(EPS)) ** -0.5
    scale_abs = 1.0 + mean * mean          # the cancellation in sumvar is relative to sum^2 / size
    assert ((co.mean - mean).abs() < 1e-12 * (1 + mean.abs())).all()
    assert ((co.invstd - inv_std).abs() <= 1e-9 * inv_std * scale_abs).all()
    assert ((co.unbiased - (sumvar / (size - 1)).clamp(min=0.0)).abs() <= 1e-12 * scale_abs).all()


def test_stat_shift_moments_describe_the_same_numbers():
    """Channels 14-15 of the SyncBN case: the moments of t = y - K with mean = K + S1/n give the coefficients of y (both on a 2^-12 grid)."""
    s = B.make_sync16((288, 288))
    assert torch.equal(s.t[:, 14:] + s.K[14:], s.y[:, 14:]) and s.y.abs()[:, 14:].max() < 8
    assert torch.equal((s.y.double()[:, 14:] - s.K.double()[14:]).float(), s.t[:, 14:])
    a = B.stats64(s.t)
    b = B.stats64(s.y)
    ca = B.coeffs64(a[0], a[1], a[3], s.gamma, s.beta, EPS, False, K=s.K)
    cb = B.coeffs64(b[0], b[1], b[3], s.gamma, s.beta, EPS, False)
    for f in B.Coeffs._fields:
        assert ((getattr(ca, f) - getattr(cb, f)).abs() <= 1e-11 * (1.0 + getattr(cb, f).abs()))[:16].all(), f


def _pack_relu_bits(bits):
    """Written from include/pylc_hip.h: M * C / 8 bytes; byte (row * C/4 + c/4) / 2 holds the nibbles of two adjacent channel quads (the
    quad's parity picks the nibble: even low, odd high); bit k of the nibble = channel 4 (c/4) + k."""
    m, c = bits.shape
    out = np.zeros(m * c // 8, dtype=np.uint8)
    for row in range(m):
        for ch in range(c):
            if bits[row, ch]:
                q = ch // 4
                out[(row * (c // 4) + q) // 2] |= 1 << ((q % 2) * 4 + ch % 4)
    return out


@pytest.mark.parametrize('m,c', [(1, 8), (5, 16), (7, 24), (3, 48)])
def test_unpack_relu_bits_round_trip(m, c):
    bits = np.random.RandomState(m * 100 + c).rand(m, c) > 0.5
    packed = torch.from_numpy(_pack_relu_bits(bits))
    assert torch.equal(B.unpack_relu_bits(packed, m, c), torch.from_numpy(bits))
    one = np.zeros((m, c), dtype=bool)
    one[m - 1, c - 3] = True                                                       # a single bit lands where the header says
    p = _pack_relu_bits(one)
    q = (c - 3) // 4
    assert p.sum() == p[((m - 1) * (c // 4) + q) // 2] == 1 << ((q % 2) * 4 + (c - 3) % 4)


def _emulated_ratio(y, gamma, beta, clamp):
    """Worst |invstd(emulated fp32 sums) - invstd(fp64)| / bound over the unrefined channels, and the refinement census."""
    S1, S2, SA, n = B.stats64(y)
    refined, border = B.needs_refine(S1, S2, n)
    co = B.coeffs64(S1, S2, n, gamma, beta, EPS, clamp)
    e1, e2 = B.emulate_sums32(y)
    dS1, dS2 = B.d_sums(S2, SA)
    assert ((e1 - S1).abs() <= dS1).all() and ((e2 - S2).abs() <= dS2).all()
    em = B.coeffs64(e1, e2, n, gamma, beta, EPS, clamp)
    dv = B.d_var(S1, S2, SA, n)
    amb = B.clamp_ambiguous(dv, co.var, EPS) if clamp else torch.zeros_like(border)
    bound = B.d_invstd_rel(dv, co.var, EPS, clamp) * co.invstd
    keep = ~refined & ~amb
    err = (em.invstd - co.invstd).abs()
    if clamp:
        exact = keep & (co.var + dv < B.eps64(EPS))          # clamped: the same constant whatever the sums
        assert (err[exact] == 0).all()
    k = keep & (bound > 0)
    return (err[k] / bound[k]).max().item() if k.any() else 0.0, refined, border, amb


@pytest.mark.parametrize('m,c,extra', B.SHAPES)
def test_emulated_accumulation_stays_inside_the_invstd_bound(m, c, extra):
    """The inputs keep THE REFERENCE ALONE inside the caps used on the GPU: fp32 per-slab partials, fp64 combine, fp32 sums."""
    inp = B.make_inputs(m, c)
    for clamp in (False, True):
        ratio, refined, border, amb = _emulated_ratio(inp.y, inp.gamma, inp.beta, clamp)
        print('BN-REF m=%d c=%d clamp=%d invstd err/bound %.3f refined %d' % (m, c, clamp, ratio, int(refined.sum())))
        assert ratio < 1.0
        # no channel sits where the kernel's fp32 sums could decide the refinement or the clamp the other way (a short column's sample
        # variance puts some of the outer channels above the threshold: those are judged with the refined bound on the GPU)
        assert not border.any() and not amb.any()
        if m >= 1000:
            assert not refined.any()


@pytest.mark.parametrize('shards', [(288,), (288, 288), (288, 150, 7), (288, 288, 288, 288), (75, 75, 75)])
def test_sync_case_conditioning(shards):
    """The 16-channel case is what its docstring says: which channels refine on which rank, which sit on which side of the clamp."""
    s = B.make_sync16(shards)
    parts = torch.split(s.t, list(shards))
    for k, p in enumerate(parts):
        S1, S2, _, n = B.stats64(p)
        refined, border = B.needs_refine(S1, S2, n)
        assert not border.any()
        if n >= 75:
            want = [8, 9, 10, 11] if k == 0 else [8, 9, 11]
            assert sorted(torch.nonzero(refined).flatten().tolist()) == want, (k, refined)
    S1, S2, SA, n = B.stats64(s.t)
    co = B.coeffs64(S1, S2, n, s.gamma, s.beta, EPS, True, K=s.K)
    assert co.var[11] == 0 and co.var[12] < 5e-6 and 1e-5 < co.var[13] < 2.4e-5
    assert not B.clamp_ambiguous(B.d_var(S1, S2, SA, n), co.var, EPS)[[0, 1, 2, 3, 4, 5, 6, 7, 12, 13, 14, 15]].any()
    if len(shards) > 1:
        assert co.var[9] > 2000 and co.var[10] > 50
    for clamp in (False, True):
        ratio, refined, border, amb = _emulated_ratio(s.t, s.gamma, s.beta, clamp)
        assert ratio < 1.0 and not border.any()
