"""The optimiser yardstick of tests/_optim.py checked without a GPU: the fp64 statement against torch's own
optimisers in float64, the float32 emulation inside the derived bounds, the bounds able to tell every listed wrong AdamW / SGD from the
right one on the inputs tests/test_optim_abi_gpu.py runs, the norm inputs' heavy elements, and the finding that at the reference's
lr = 1e-4, weight_decay = 5e-5 the decoupled decay is the identity in fp32."""
import numpy as np
import pytest
import torch

from tests import _optim as O

SMALL_CASES = [c for c in O.ADAMW_CASES if c[-1] <= 200000]


def _grads(n, steps):
    """Gradients that are NOT multiples of one another; the scales make the 0.5 clip bite at some steps and not at others."""
    r = np.random.RandomState(5)
    scales = [0.3, 1e-4, 0.02, 2e-3, 0.5][:steps]
    return [s * r.standard_normal(n) for s in scales]


def test_statement_equals_torch_adamw_and_clip_in_float64():
    n, steps = 301, 5
    r = np.random.RandomState(4)
    p0 = r.standard_normal(n)
    gs = _grads(n, steps)
    # hyper-parameters that float32 holds exactly, so that the statement (which takes them as float32 values) and torch see the same numbers
    lr, b1, b2, eps, wd, max_norm = 2.0 ** -7, 0.875, 0.96875, 2.0 ** -20, 0.125, 0.5
    pt = torch.tensor(p0, dtype=torch.float64, requires_grad=True)
    opt = torch.optim.AdamW([pt], lr=lr, betas=(b1, b2), eps=eps, weight_decay=wd)
    p, m, v = p0.copy(), np.zeros(n), np.zeros(n)
    clipped = []
    for step, g in enumerate(gs, 1):
        pt.grad = torch.tensor(g, dtype=torch.float64)
        norm_t = float(torch.nn.utils.clip_grad_norm_([pt], max_norm))
        opt.step()
        norm, coef = O.clip_ref(g, max_norm)
        clipped.append(coef < 1.0)
        assert abs(norm - norm_t) <= 1e-14 * norm
        # the statement adds the float32 1e-6 the kernel adds, torch the double: 5e-14 apart, against norms of 1e-3 and more
        assert np.abs(g * coef - pt.grad.numpy()).max() <= 1e-10 * np.abs(g).max()
        # step the statement with the clipped gradient torch used.  What remains between the two is the host's rounding of bc1 and
        # bc2_sqrt to float32 (u each, part of the statement): 2u of an update of at most lr / bc1 (|m_hat| <= sqrt(v_hat) for these
        # betas: (1 - b1) / sqrt(1 - b2) < 1), accumulating over the steps; allowed: 4u
        p, m, v = O.adamw_ref(p, pt.grad.numpy(), m, v, None, lr, b1, b2, eps, wd, step)
        assert np.abs(p - pt.detach().numpy()).max() <= step * 4 * O.U * lr / (1.0 - b1 ** step)
        st = opt.state[pt]
        assert np.abs(m - st['exp_avg'].numpy()).max() <= 1e-15 and np.abs(v - st['exp_avg_sq'].numpy()).max() <= 1e-15
    assert any(clipped) and not all(clipped), 'want clipped and unclipped steps, got %s' % clipped


def test_statement_equals_torch_sgd_momentum_in_float64():
    n = 257
    r = np.random.RandomState(6)
    p0, dirty = r.standard_normal(n), r.standard_normal(n)
    gs = _grads(n, 4)
    lr, mu = 2.0 ** -6, 0.875
    pt = torch.tensor(p0, dtype=torch.float64, requires_grad=True)
    opt = torch.optim.SGD([pt], lr=lr, momentum=mu)
    p, buf = p0.copy(), dirty                      # the statement ignores what the buffer held before step 1
    for step, g in enumerate(gs, 1):
        pt.grad = torch.tensor(g, dtype=torch.float64)
        opt.step()
        p, buf = O.sgd_ref(p, g, buf, None, lr, mu, step)
        assert np.abs(p - pt.detach().numpy()).max() <= 1e-14
        assert np.abs(buf - opt.state[pt]['momentum_buffer'].numpy()).max() <= 1e-14


@pytest.mark.parametrize('case', O.ADAMW_CASES, ids=lambda c: 'step%d-n%d' % (c[0], c[-1]))
def test_float32_adamw_stays_inside_the_bounds(case):
    kw = O.adamw_case_args(case)
    worst = {}
    for seed in range(3 if case[-1] <= 200000 else 1):
        x = O.adamw_inputs(case[-1], case[0], case[4], seed)
        ref = O.adamw_ref(x.p, x.g, x.m, x.v, **kw)
        got = O.adamw_f32(x.p, x.g, x.m, x.v, **kw)
        bnd = O.adamw_bounds(x.p, x.g, x.m, x.v, **kw)
        for name, a, b, d in zip('pmv', got, ref, bnd):
            err = np.abs(a.astype(np.float64) - b)
            assert np.isfinite(a).all()
            assert (err <= d).all(), '%s: worst err / bound %.3g' % (name, (err[err > d] / d[err > d]).max())
            live = d > 0
            worst[name] = max(worst.get(name, 0.0), float((err[live] / d[live]).max()) if live.any() else 0.0)
        assert len(x.planted) > 0
    print('OPT-cpu adamw %s: err / bound %s' % (case, '  '.join('%s %.3f' % kv for kv in worst.items())))


def test_planted_zero_gradient_gives_no_update():
    step, (b1, b2), eps, (lr, wd), coef, n = O.ADAMW_CASES[2]            # wd = 0: p must come back bit-unchanged where g = v = m = 0
    x = O.adamw_inputs(100003, step, coef)
    at = (x.g == 0) & (x.v == 0)
    assert at.any() and (x.m[at] == 0).all()
    pp, mm, vv = O.adamw_f32(x.p, x.g, x.m, x.v, coef, lr, b1, b2, eps, wd, step)
    assert np.array_equal(pp[at].view(np.uint32), x.p[at].view(np.uint32)) and not mm[at].any() and not vv[at].any()


@pytest.mark.parametrize('case', O.SGD_CASES, ids=lambda c: 'step%d-n%d' % (c[0], c[-1]))
def test_float32_sgd_stays_inside_the_bounds(case):
    step, coef, mu, n = case
    x = O.sgd_inputs(n)
    ref = O.sgd_ref(x.p, x.g, x.buf, coef, 1e-2, mu, step)
    got = O.sgd_f32(x.p, x.g, x.buf, coef, 1e-2, mu, step)
    bnd = O.sgd_bounds(x.p, x.g, x.buf, coef, 1e-2, mu, step)
    for a, b, d in zip(got, ref, bnd):
        assert (np.abs(a.astype(np.float64) - b) <= d).all()


@pytest.mark.parametrize('mutant', O.MUTANTS)
def test_bounds_tell_a_wrong_adamw(mutant):
    """On the GPU file's inputs the mutant lies at least 8 x the bound away from the statement in p, m or v on some element of some case.
    The decay mutants can only show where the decay is not the identity: (lr, wd) = (1e-2, 0.1)."""
    worst = 0.0
    for case in SMALL_CASES:
        kw = O.adamw_case_args(case)
        if mutant in ('no_decay', 'coupled_decay') and kw['wd'] * kw['lr'] < 1e-6:
            continue
        x = O.adamw_inputs(case[-1], case[0], case[4])
        ref = O.adamw_ref(x.p, x.g, x.m, x.v, **kw)
        mut = O.adamw_ref(x.p, x.g, x.m, x.v, mutant=mutant, **kw)
        bnd = O.adamw_bounds(x.p, x.g, x.m, x.v, **kw)
        for a, b, d in zip(mut, ref, bnd):
            live = d > 0
            if live.any():
                worst = max(worst, float((np.abs(a - b)[live] / d[live]).max()))
    print('OPT-cpu mutant %-20s worst distance / bound %.3g' % (mutant, worst))
    assert worst >= 8.0


def test_bounds_tell_a_momentum_buffer_that_is_not_reset():
    worst = 0.0
    for step, coef, mu, n in O.SGD_CASES:
        if step != 1 or mu == 0.0:
            continue
        x = O.sgd_inputs(n)
        ref = O.sgd_ref(x.p, x.g, x.buf, coef, 1e-2, mu, step)
        mut = O.sgd_ref(x.p, x.g, x.buf, coef, 1e-2, mu, step, mutant='no_reset')
        bnd = O.sgd_bounds(x.p, x.g, x.buf, coef, 1e-2, mu, step)
        worst = max(worst, max(float((np.abs(a - b) / d).max()) for a, b, d in zip(mut, ref, bnd)))
    print('OPT-cpu mutant no_reset: worst distance / bound %.3g' % worst)
    assert worst >= 8.0


def test_decay_is_the_identity_at_the_reference_settings():
    """lr = 1e-4, weight_decay = 5e-5: 1.f - lr * wd rounds to 1.f (lr wd = 5e-9 < 2^-25 = 3e-8), in the kernel's expression and in
    torch.optim.AdamW alike -- no test at those settings can see the decay path."""
    assert np.float32(1) - np.float32(1e-4) * np.float32(5e-5) == 1
    assert np.float32(1) - np.float32(1e-2) * np.float32(0.1) != 1
    p0 = torch.randn(1000, generator=torch.Generator().manual_seed(1)) * 3
    for foreach in (False, True):
        p = p0.clone().requires_grad_(True)
        opt = torch.optim.AdamW([p], lr=1e-4, weight_decay=5e-5, foreach=foreach)
        p.grad = torch.zeros_like(p)
        opt.step()
        assert torch.equal(p.detach().view(torch.int32), p0.view(torch.int32))


@pytest.mark.parametrize('n', O.CLIP_NS)
def test_norm_inputs_cannot_hide_a_dropped_element(n):
    g, heavy = O.norm_inputs(n)
    g64 = g.astype(np.float64)
    s = float((g64 ** 2).sum())
    norm = np.sqrt(s)
    bound = O.norm_bound(norm, n)
    n4 = n // 4
    want = {0} | set(range(4 * n4, n)) | ({4 * n4 - 1} if n4 else set())
    L, blocks = O.norm_trips(n)
    if n == O.CLIP_NS[-1]:
        assert L == 2 and blocks == O.NORM_BLOCKS
        want.add(4 * 256 * O.NORM_BLOCKS)
    assert set(heavy) == want
    worst = min((norm - np.sqrt(max(s - g64[i] ** 2, 0.0))) / bound for i in heavy)
    print('OPT-cpu norm n %d: L %d, a dropped heavy element moves the norm by >= %.0f x the bound' % (n, L, worst))
    assert worst > 100.0
    # and the fp32 emulation of the documented summation stays inside the bound
    parts = []
    tail = g[4 * n4:]
    q = g[:4 * n4].reshape(-1, 4)
    sq = q * q
    quad = ((sq[:, 0] + sq[:, 1]) + sq[:, 2]) + sq[:, 3]
    for b in range(blocks):
        th = np.zeros(256, np.float32)
        for t in range(L):
            lo = (t * blocks + b) * 256
            seg = quad[lo:lo + 256]
            th[:seg.size] = th[:seg.size] + seg
        if b == 0 and tail.size:
            th[:tail.size] = th[:tail.size] + tail * tail
        w = th.reshape(4, 64)
        for o in (32, 16, 8, 4, 2, 1):
            w = np.concatenate([w[:, :64 - o] + w[:, o:], w[:, 64 - o:]], 1)
        parts.append(((w[0, 0] + w[1, 0]) + w[2, 0]) + w[3, 0])
    got = np.float32(np.sqrt(np.sum(np.array(parts, np.float64))))
    assert abs(float(got) - norm) <= bound, (float(got), norm, bound)
