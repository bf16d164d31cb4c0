"""Frozen BatchNorm on the GPU (-m gpu): the one-pass backward kernel against the two training-mode launches it
replaces (bit identity), the op against fp64 torch, whole DeepLab fine-tuning steps against the CPU oracle, and the properties of the
mode -- running statistics untouched, eval / test unchanged, nothing synchronised, precision mode 3 refused."""
import ctypes as C
import os

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from tests import _data as D

pytestmark = pytest.mark.gpu


def rnd(seed, *shape, scale=1.0):
    return torch.from_numpy(np.random.RandomState(seed).standard_normal(shape).astype(np.float32) * scale)


def to_dev_nhwc(t, dev):
    return t.to(dev).contiguous(memory_format=torch.channels_last)


def rel_err(a, b):
    a, b = a.double().cpu(), b.double().cpu()
    return ((a - b).abs().max() / (b.abs().max() + 1e-30)).item()


# ---- A: the C ABI, bit for bit against pylc_bn_bwd_reduce + pylc_bn_bwd_apply on zero sums ---------------------------------------------------
def _pitched(t, pitch, fill=float('nan')):
    """[M][C] values in an [M][pitch] buffer whose unused lanes hold `fill`; returns (buffer, view of the values)."""
    m, c = t.shape
    buf = torch.full((m, pitch), fill, device=t.device)
    buf[:, :c] = t
    return buf, buf[:, :c]


class _AbiCase:
    """Operands of one backward on the device: a forward through pylc_bn_apply(_ex) leaves `out` and (residual + ReLU, C % 8 == 0) the
    1-bit mask; mode = 'y' (mask recomputed from y, or no ReLU), 'out' or 'bits'."""

    def __init__(self, dev, m, c, relu, mode, extra_pitch=0, drop_p=0.0, seed=0):
        from pylc_amd import lib as L
        from pylc_amd.lib import lib, check, ptr, stream
        L.init()
        self.m, self.c, self.relu, self.mode, self.drop_p, self.drop_seed = m, c, relu, mode, drop_p, 977 + seed
        p = c + extra_pitch
        self.p = p
        g = torch.Generator().manual_seed(1000 + 7 * m + c + seed)
        r = lambda *s: torch.randn(*s, generator=g)
        self.ybuf, self.y = _pitched((2.0 * r(m, c) + 0.5).to(dev), p)
        self.dbuf, self.dout = _pitched(r(m, c).to(dev), p)
        self.gamma, beta = (1 + 0.1 * r(c)).to(dev), (0.1 * r(c)).to(dev)
        rm, rv = (0.1 * r(c)).to(dev), (1 + 0.1 * r(c).abs()).to(dev)
        coef = torch.empty(4 * c, device=dev)
        self.mean, self.invstd, self.scale, self.shift = coef[:c], coef[c:2 * c], coef[2 * c:3 * c], coef[3 * c:]
        check(lib.pylc_bn_eval_coeffs_full(ptr(rm), ptr(rv), ptr(self.gamma), ptr(beta), 1e-5, c, ptr(self.scale), ptr(self.shift),
                                           ptr(self.mean), ptr(self.invstd), stream()))
        self.res = self.obuf = self.out = self.mask = None
        if mode in ('out', 'bits'):
            self.rbuf, self.res = _pitched(r(m, c).to(dev), p)
            self.obuf, self.out = _pitched(torch.zeros(m, c, device=dev), p)
            ex = self.extra(forward=True)
            if mode == 'bits':
                self.mask = torch.zeros(m * c // 8, dtype=torch.uint8, device=dev)
                ex.relu_mask = ptr(self.mask)
            check(lib.pylc_bn_apply_ex(ptr(self.y), p, ptr(self.scale), ptr(self.shift), ptr(self.res), p, ptr(self.out), p, m, c, int(relu),
                                       None, C.byref(ex), stream()))

    def extra(self, forward=False):
        from pylc_amd.lib import BnExtra, ptr
        ex = BnExtra()
        ex.nplanes, ex.drop_p, ex.drop_seed = 2, self.drop_p, self.drop_seed
        if self.mask is not None and not forward:
            ex.relu_mask = ptr(self.mask)
        return ex

    def outputs(self, want_g):
        dev, m, c, p = self.y.device, self.m, self.c, self.p
        dybuf, dy = _pitched(torch.zeros(m, c, device=dev), p)
        gbuf, gv = _pitched(torch.zeros(m, c, device=dev), p) if want_g else (None, None)
        return dybuf, dy, gbuf, gv, torch.zeros(1, dtype=torch.int32, device=dev)

    def mask_args(self):
        """(out, out_pitch, scale, shift) as the three entry points take them for this mask source."""
        from pylc_amd.lib import ptr
        if self.mode == 'out':
            return ptr(self.out), self.p, None, None
        if self.mode == 'bits' or not self.relu:
            return None, 0, None, None
        return None, 0, ptr(self.scale), ptr(self.shift)

    def two_pass(self, want_g):
        from pylc_amd.lib import lib, check, ptr, stream
        dev, m, c, p = self.y.device, self.m, self.c, self.p
        sums = torch.full((2 * c,), float('nan'), device=dev)
        ws = torch.empty(lib.pylc_bn_workspace_floats(m, c), device=dev)
        o, op, sc, sh = self.mask_args()
        ex = self.extra()
        check(lib.pylc_bn_bwd_reduce_ex(ptr(self.dout), p, o, op, ptr(self.y), p, ptr(self.mean), ptr(self.invstd), m, c, int(self.relu), ptr(sums),
                                        ptr(ws), sc, sh, None, 0.0, C.byref(ex), None, stream()))
        dybuf, dy, gbuf, gv, amax = self.outputs(want_g)
        zero = torch.zeros(2 * c, device=dev)
        check(lib.pylc_bn_bwd_apply_ex(ptr(self.dout), p, o, op, ptr(self.y), p, ptr(self.mean), ptr(self.invstd), ptr(self.gamma), ptr(zero), float(m),
                                       m, c, int(self.relu), ptr(dy), p, ptr(gv), p if want_g else 0, ptr(amax), sc, sh, C.byref(ex), stream()))
        return dybuf, gbuf, sums, amax

    def one_pass(self, want_g, want_sums=True, pass_y=True):
        from pylc_amd.lib import lib, check, ptr, stream
        dev, m, c, p = self.y.device, self.m, self.c, self.p
        sums = torch.full((2 * c,), float('nan'), device=dev)
        ws = torch.empty(lib.pylc_bn_workspace_floats(m, c), device=dev) if want_sums else None
        o, op, sc, sh = self.mask_args()
        ex = self.extra()
        dybuf, dy, gbuf, gv, amax = self.outputs(want_g)
        check(lib.pylc_bn_frozen_bwd(ptr(self.dout), p, o, op, ptr(self.y) if pass_y else None, p if pass_y else 0, ptr(self.mean), ptr(self.invstd),
                                     ptr(self.gamma), m, c, int(self.relu), ptr(dy), p, ptr(gv), p if want_g else 0, ptr(amax), sc, sh,
                                     ptr(sums) if want_sums else None, ptr(ws), C.byref(ex), stream()))
        return dybuf, gbuf, sums, amax


def _same(a, b):
    """torch.equal with NaN == NaN (the unused lanes of a pitched buffer)."""
    return (a is None and b is None) or torch.equal(torch.nan_to_num(a, nan=12345.0), torch.nan_to_num(b, nan=12345.0))


ABI_CASES = [(1024, 64, True, 'y', False, 0),         # ReLU from y
             (1000, 64, True, 'y', False, 0),         # ragged last slab
             (162, 256, True, 'out', True, 0),        # MS_OUT + g_out
             (363, 48, True, 'y', False, 0),
             (72, 728, False, 'y', False, 0),         # no ReLU
             (32, 2048, True, 'bits', True, 0),       # two column passes; MS_BITS + g_out
             (5, 256, True, 'y', False, 0),
             (75, 20, True, 'y', False, 0),           # odd vector count
             (2500, 8, True, 'y', False, 0),          # 128 row lanes, three slabs
             (363, 48, True, 'out', True, 4)]         # all pitches C + 4


@pytest.mark.parametrize('m,c,relu,mode,want_g,extra', ABI_CASES)
def test_abi_bit_identical_to_the_two_training_launches(dev, m, c, relu, mode, want_g, extra):
    case = _AbiCase(dev, m, c, relu, mode, extra)
    dy0, g0, s0, a0 = case.two_pass(want_g)
    dy1, g1, s1, a1 = case.one_pass(want_g)
    torch.cuda.synchronize()
    assert not torch.isnan(s0).any() and dy0[:, :c].abs().max() > 0
    assert torch.equal(dy1[:, :c], dy0[:, :c]) and torch.equal(s1, s0) and torch.equal(a1, a0)
    if want_g:
        assert torch.equal(g1[:, :c], g0[:, :c]) and g0[:, :c].abs().max() > 0
    if extra:
        # the unused lanes of the outputs were NaN before the launch and still are
        assert torch.isnan(dy1[:, c:]).all() and torch.isnan(g1[:, c:]).all() and _same(dy1, dy0) and _same(g1, g0)
    # the sums against fp64 torch (what the bit identity is worth): g = dout * mask, xhat = (y - mean) invstd
    gd = (g1[:, :c] if want_g else (case.dout * ((case.y * case.scale + case.shift) > 0) if relu else case.dout)).double()
    xh = (case.y.double() - case.mean.double()) * case.invstd.double()
    assert rel_err(s1[:c], (gd * xh).sum(0)) < 2e-5 and rel_err(s1[c:], gd.sum(0)) < 2e-5
    assert rel_err(dy1[:, :c], gd * (case.gamma * case.invstd).double()) < 1e-6


@pytest.mark.parametrize('m,c,mode,want_g', [(363, 48, 'y', False), (162, 256, 'out', True)])
def test_abi_dropout_variant(dev, m, c, mode, want_g):
    case = _AbiCase(dev, m, c, True, mode, drop_p=0.5, seed=3)
    dy0, g0, s0, a0 = case.two_pass(want_g)
    dy1, g1, s1, a1 = case.one_pass(want_g)
    assert torch.equal(dy1, dy0) and torch.equal(s1, s0) and torch.equal(a1, a0) and _same(g1, g0)
    plain = _AbiCase(dev, m, c, True, mode, seed=3).one_pass(want_g)[0]
    dropped = ((dy1 == 0) & (plain != 0)).float().sum() / (plain != 0).float().sum()
    assert 0.4 < float(dropped) < 0.6                                              # p = 0.5 of the live elements
    kept = (dy1 != 0)
    assert torch.equal(dy1[kept], 2 * plain[kept])                                 # keep scale 1 / (1 - p)


@pytest.mark.parametrize('m,c,relu,mode,want_g,pass_y', [(363, 48, True, 'y', False, True), (162, 256, True, 'out', True, False),
                                                         (32, 2048, True, 'bits', True, False), (72, 728, False, 'y', False, False)])
def test_abi_no_sums_variant(dev, m, c, relu, mode, want_g, pass_y):
    """Neither parameter takes a gradient: no reduction; y is read only for a recomputed mask (NULL otherwise)."""
    case = _AbiCase(dev, m, c, relu, mode)
    dy0, g0, _, a0 = case.one_pass(want_g)
    dy1, g1, s1, a1 = case.one_pass(want_g, want_sums=False, pass_y=pass_y)
    assert torch.equal(dy1, dy0) and _same(g1, g0) and torch.equal(a1, a0)
    assert torch.isnan(s1).all()                                                   # never passed, never written


def test_abi_refused_arguments_write_nothing(dev):
    from pylc_amd.lib import lib, ptr, stream
    t = torch.full((64, 8), float('nan'), device=dev)
    v = torch.ones(8, device=dev)
    src = torch.ones(64, 8, device=dev)
    ws = torch.full((lib.pylc_bn_workspace_floats(64, 8),), float('nan'), device=dev)
    sums = torch.full((16,), float('nan'), device=dev)

    def call(m, c):
        return lib.pylc_bn_frozen_bwd(ptr(src), 8, None, 0, ptr(src), 8, ptr(v), ptr(v), ptr(v), m, c, 0, ptr(t), 8, None, 0, None, None, None,
                                      ptr(sums), ptr(ws), None, stream())
    assert call(8, 6) == 1 and b'C % 4' in lib.pylc_last_error()                   # PYLC_ERR_ARG
    assert call(0, 8) == 1 and b'M > 0' in lib.pylc_last_error()
    torch.cuda.synchronize()
    assert torch.isnan(t).all() and torch.isnan(sums).all() and torch.isnan(ws).all()
    assert call(8, 8) == 0
    torch.cuda.synchronize()
    assert torch.equal(t[:8], torch.ones(8, 8, device=dev)) and torch.isnan(t[8:]).all() and torch.equal(sums[8:], torch.full((8,), 8.0, device=dev))


# ---- B: the op against fp64 torch -----------------------------------------------------------------------------------------------------------
def _op_case(dev, c, b, hw, relu, res):
    y = rnd(11, b, c, hw, hw, scale=2.0) + 0.5
    g, be = 1 + 0.1 * rnd(12, c), 0.1 * rnd(13, c)
    rm, rv = 0.1 * rnd(14, c), 1 + 0.1 * rnd(15, c).abs()
    r = rnd(16, b, c, hw, hw) if res else None
    return y, g, be, rm, rv, r


@pytest.mark.parametrize('c,b,hw,relu,res', [(64, 4, 16, True, False), (256, 2, 9, True, True), (48, 3, 11, True, False),
                                             (728, 2, 6, False, False), (2048, 2, 4, True, True), (256, 5, 1, True, False),
                                             (20, 3, 5, True, False)])
def test_op_against_fp64_torch(dev, c, b, hw, relu, res):
    from pylc_amd import ops
    y, g, be, rm, rv, r = _op_case(dev, c, b, hw, relu, res)
    yr, gr, ber = y.double().requires_grad_(True), g.double().requires_grad_(True), be.double().requires_grad_(True)
    rr = r.double().requires_grad_(True) if res else None
    o = F.batch_norm(yr, rm.double(), rv.double(), gr, ber, False, 0.1, 1e-5)
    if res:
        o = o + rr
    if relu:
        o = F.relu(o)
    do = rnd(17, *o.shape)
    o.backward(do.double())
    yd = to_dev_nhwc(y, dev).requires_grad_(True)
    gd, bed = g.to(dev).requires_grad_(True), be.to(dev).requires_grad_(True)
    rmd, rvd = rm.to(dev), rv.to(dev)
    rd = to_dev_nhwc(r, dev).requires_grad_(True) if res else None
    od = ops.bn_act(yd, gd, bed, rmd, rvd, rd, relu, True, frozen=True)
    assert od.dtype == torch.float32 and not ops.is_planes(od)
    od.backward(do.to(dev))
    assert rel_err(od, o) < 5e-6
    assert torch.equal(rmd.cpu(), rm) and torch.equal(rvd.cpu(), rv)               # running statistics: not written
    assert rel_err(yd.grad, yr.grad) < 2e-5
    assert rel_err(gd.grad, gr.grad) < 2e-5 and rel_err(bed.grad, ber.grad) < 2e-5
    if res:
        assert rel_err(rd.grad, rr.grad) < 1e-6
    # no parameter gradient wanted (the no-sums kernel): dy and the residual gradient are the same bits
    yd2 = to_dev_nhwc(y, dev).requires_grad_(True)
    rd2 = to_dev_nhwc(r, dev).requires_grad_(True) if res else None
    od2 = ops.bn_act(yd2, g.to(dev), be.to(dev), rmd, rvd, rd2, relu, True, frozen=True)
    od2.backward(do.to(dev))
    assert torch.equal(od2, od) and torch.equal(yd2.grad, yd.grad) and (not res or torch.equal(rd2.grad, rd.grad))


@pytest.mark.parametrize('c,b,hw,res,into', [(256, 2, 9, False, False), (48, 3, 11, True, False), (64, 2, 8, False, True)])
def test_op_fused_dropout(dev, c, b, hw, res, into):
    """out = mask * (1 / (1 - p)) * undropped with the mask recovered from out != 0, and the backward follows that mask."""
    from pylc_amd import ops, runtime
    prev = runtime.dropout_enabled
    runtime.dropout_enabled = True
    try:
        y, g, be, rm, rv, r = _op_case(dev, c, b, hw, True, res)
        do = rnd(17, b, c, hw, hw).to(dev)
        got = []
        for drop in (None, (0.5, 4242)):
            yd = to_dev_nhwc(y, dev).requires_grad_(True)
            gd, bed = g.to(dev).requires_grad_(True), be.to(dev).requires_grad_(True)
            rd = to_dev_nhwc(r, dev).requires_grad_(True) if res else None
            buf = [ops.empty_nhwc(b, c + 16, hw, hw, dev)] if into else None
            od = ops.bn_act(yd, gd, bed, rm.to(dev), rv.to(dev), rd, True, True, drop=drop, into=(buf, 16) if into else None, frozen=True)
            if into:
                assert od.data_ptr() == buf[0][:, 16:].data_ptr() and ops.pitch_of(od) == c + 16
            od.backward(do)
            got.append((od.detach().clone(), yd.grad.clone(), gd.grad.clone(), bed.grad.clone(), rd.grad.clone() if res else None))
    finally:
        runtime.dropout_enabled = prev
    (o0, dy0, dg0, db0, dr0), (o1, dy1, dg1, db1, dr1) = got
    keep = o1 != 0
    live = o0 != 0
    assert 0.4 < float((keep & live).float().sum() / live.float().sum()) < 0.6 and not (keep & ~live).any()
    zero = torch.zeros_like(o0)
    assert torch.equal(o1, torch.where(keep, 2 * o0, zero))
    assert torch.equal(dy1, torch.where(keep, 2 * dy0, zero))
    if res:
        assert torch.equal(dr1, torch.where(keep, 2 * dr0, zero))
    # parameter gradients in fp64 from that mask
    gg = (2 * do * keep).double().cpu()
    coef = (rv.double() + 1e-5).rsqrt()
    xh = (y.double() - rm.double().view(1, c, 1, 1)) * coef.view(1, c, 1, 1)
    assert rel_err(dg1, (gg * xh).sum((0, 2, 3))) < 2e-5 and rel_err(db1, gg.sum((0, 2, 3))) < 2e-5


def test_op_single_element_batch(dev):
    """One value per channel: the training-mode BatchNorm refuses it (torch's rule), the frozen one normalises it like any other."""
    from pylc_amd import ops
    c = 256
    y, g, be, rm, rv, _ = _op_case(dev, c, 1, 1, True, False)
    yr, gr, ber = y.double().requires_grad_(True), g.double().requires_grad_(True), be.double().requires_grad_(True)
    o = F.relu(F.batch_norm(yr, rm.double(), rv.double(), gr, ber, False, 0.1, 1e-5))
    do = rnd(17, 1, c, 1, 1)
    o.backward(do.double())
    yd, gd, bed = to_dev_nhwc(y, dev).requires_grad_(True), g.to(dev).requires_grad_(True), be.to(dev).requires_grad_(True)
    with pytest.raises(ValueError, match='more than 1 value'):
        ops.bn_act(yd, gd, bed, rm.to(dev), rv.to(dev), None, True, True)
    od = ops.bn_act(yd, gd, bed, rm.to(dev), rv.to(dev), None, True, True, frozen=True)
    od.backward(do.to(dev))
    assert rel_err(od, o) < 5e-6 and rel_err(yd.grad, yr.grad) < 2e-5 and rel_err(gd.grad, gr.grad) < 2e-5 and rel_err(bed.grad, ber.grad) < 2e-5


def test_group_calls_frozen_members_one_by_one(dev):
    from pylc_amd import ops
    y, g, be, rm, rv, _ = _op_case(dev, 64, 2, 8, True, False)
    spec = lambda: dict(y=to_dev_nhwc(y, dev).requires_grad_(True), gamma=g.to(dev), beta=be.to(dev), running_mean=rm.to(dev),
                        running_var=rv.to(dev), relu=True, frozen=True)
    a, b = ops.bn_act_group([spec(), spec()], None)
    sp = spec()
    sp.pop('frozen')
    want = ops.bn_act(frozen=True, **sp)
    assert torch.equal(a, want) and torch.equal(b, want) and type(a.grad_fn).__name__.startswith('FrozenBnActFn')


# ---- C: whole networks against the oracle ----------------------------------------------------------------------------------------------------
NORM_TOL = 2e-3
ORACLE_NORM_TOL = NORM_TOL / 4        # tests/test_class_counts_gpu.py's rule: the fp32 oracle within a quarter of the bound of its own fp64 evaluation
ORACLE_GRAD_TOL = 1.25e-2

RESNET_GRADS = ['backbone.bn1.weight', 'backbone.bn1.bias', 'backbone.layer1.0.bn3.weight', 'backbone.layer1.0.downsample.1.weight',
                'backbone.layer4.2.bn3.weight', 'aspp.bn1.weight', 'aspp.global_avg_pool.2.weight', 'decoder.bn1.weight', 'decoder.bn1.bias',
                'decoder.last_conv.1.weight', 'decoder.last_conv.8.weight', 'decoder.last_conv.8.bias']
XCEPTION_GRADS = ['backbone.bn1.weight', 'backbone.block1.rep.1.weight', 'backbone.block1.skipbn.weight', 'backbone.bn5.weight',
                  'decoder.bn1.weight', 'decoder.bn1.bias', 'decoder.last_conv.8.weight', 'decoder.last_conv.8.bias']

# tag -> (backbone, input channels, classes, weight salt, tile seed, mask seed, batch)
NET_CASES = {'resnet_bs2': ('resnet', 3, 9, 29, 709, 710, 2),
             'resnet_bs1': ('resnet', 3, 9, 29, 709, 710, 1),
             'xception_bs2': ('xception', 1, 11, 31, 711, 712, 2)}


def _frozen_oracle_step(cfg, w, x, y, dtype):
    """The frozen step of the oracle: the EVAL-mode forward (running statistics) under autograd, then the loss, clip_grad_norm_ and AdamW of
    oracle.step.train_step.  Returns (ce, dice, focal), logits, the pre-clip norm and the state, whose .grad are the clipped gradients."""
    import oracle
    from oracle import step as ostep
    sd = {k: (v.to(dtype) if v.is_floating_point() else v.clone()) for k, v in w.items()}
    sd = {k: v.clone() for k, v in sd.items()}
    opt = ostep.make_optimizer(sd, cfg)
    xin, yy = ostep._prep(cfg, x.clone().to(dtype), y.clone())
    logits = ostep.forward(sd, cfg, xin, False)
    total, ce, dsc, fl = oracle.multiloss(logits, yy, cfg.loss_weights, cfg.class_weights, cfg.weighted)
    opt.zero_grad()
    total.backward()
    gnorm = float(torch.nn.utils.clip_grad_norm_(ostep.trainable(sd), cfg.clip))
    opt.step()
    return (ce.item(), dsc.item(), fl.item()), logits.detach(), gnorm, sd


def _net_case(tag):
    import oracle
    from oracle import step as ostep
    backbone, ch, c, salt, s_x, s_y, b = NET_CASES[tag]
    cfg = ostep.StepConfig('deeplab', backbone, c, ch, dropout=False)
    x = D.tiles(s_x, 2, ch, 64, 64)
    y = D.blob_masks(s_y, 2, 64, 64, c, cell=8)
    w = ostep.calibrate_bn(oracle.formula_state(oracle.state_spec('deeplab', backbone, c, 3), salt=salt), cfg, x.clone())      # on the bs-2 batch
    return cfg, w, x[:b].clone(), y[:b].clone()


@pytest.mark.parametrize('tag', list(NET_CASES))
def test_frozen_network_step_against_oracle(dev, tag):
    """DeepLabV3+ fine-tuning steps (freeze_bn=True) against the oracle's frozen step, built as
    test_class_counts_gpu.test_network_step_against_oracle builds its cases: ResNet-101 3-ch 64^2, 9 classes, bs 2 and bs 1 (which the
    training-mode network refuses: one value per channel under the image pool's BatchNorm), Aligned Xception 1-ch 64^2, 11 classes, bs 2.

    The pre-clip norm is asserted only where the fp32 oracle is within ORACLE_NORM_TOL of its own fp64 evaluation, and every compared
    gradient tensor only where it is within ORACLE_GRAD_TOL; both conditions are asserted here with the threads the test runs on.  Measured on the CPU at 1 and 8
    threads: norm 1.1e-4 - 2.1e-4 (ResNet bs 2), 1.2e-4 - 3.1e-4 (bs 1), below 3e-6 (Xception); losses below 1e-5, logits below 1.2e-4;
    gradient tensors <= 1.1e-2 (ResNet), <= 4.7e-3 (Xception) of their largest entry.  Without the feature the flag is ignored and the
    step is the training-mode one (bs 2: CE 2.2059 instead of 2.3257, norm 12.8 instead of 90.1; bs 1 raises)."""
    from pylc_amd import runtime
    from pylc_amd.layers import BatchNorm2d, Conv2d, DepthwiseConv3x3
    from pylc_amd.model import Model, Meta
    from tests.test_truesize_oracle_gpu import LOGIT_TOL, LOSS_TOL, GRAD_CAP
    backbone, ch, c = NET_CASES[tag][:3]
    prev = runtime.dropout_enabled
    runtime.dropout_enabled = False
    try:
        cfg, w, x, y = _net_case(tag)
        (ce, dsc, fl), ref_logits, ref_norm, sd = _frozen_oracle_step(cfg, w, x, y, torch.float32)
        (ce64, dsc64, fl64), logits64, norm64, sd64 = _frozen_oracle_step(cfg, w, x, y, torch.float64)
        e_oracle = abs(ref_norm - norm64) / norm64
        print('FZ %s oracle alone: |g| fp32 %.5f vs fp64 %.5f: %.3g (bound %.3g); loss %.3g; logits %.3g'
              % (tag, ref_norm, norm64, e_oracle, ORACLE_NORM_TOL, max(abs(a - b) for a, b in zip((ce, dsc, fl), (ce64, dsc64, fl64))),
                 (ref_logits.double() - logits64).abs().max().item()))
        assert e_oracle < ORACLE_NORM_TOL, 'the fp32 oracle of this case is too far from its own fp64 evaluation for the norm to be compared'

        model = Model(Meta(arch='deeplab', backbone=backbone, ch=ch, n_classes=c, freeze_bn=True), dev).build()
        model.net.load_state_dict(w)
        assert model.net.freeze_bn is True
        seen = []
        hooks = [m.register_forward_hook(lambda mod, a, out: seen.append(hasattr(out, '_pylc_sums')))
                 for m in model.net.modules() if isinstance(m, (Conv2d, DepthwiseConv3x3))]
        # train-mode (frozen) logits
        model.net.train()
        with torch.no_grad():
            got_logits = model.net(model.pack_input(x)).float().cpu()
        e_logit = (got_logits - ref_logits).abs().max().item()
        model.train(x, y)
        torch.cuda.synchronize()
        got = [float(model.crit.ce), float(model.crit.dsc), float(model.crit.fl)]
        gnorm, coef = model.optim.norm.cpu().tolist()
        e_loss = max(abs(a - r) for a, r in zip(got, (ce, dsc, fl)))
        e_norm = abs(gnorm - ref_norm) / ref_norm
        print('FZ %s frozen step: HIP (%.6f %.6f %.6f) oracle (%.6f %.6f %.6f) max|diff| %.3g (bound %.3g); |g| %.5f vs %.5f: %.3g (bound %.3g); '
              'logits %.3g (bound %.3g)' % (tag, *got, ce, dsc, fl, e_loss, LOSS_TOL, gnorm, ref_norm, e_norm, NORM_TOL, e_logit, LOGIT_TOL))
        assert e_logit < LOGIT_TOL
        assert e_loss < LOSS_TOL
        assert e_norm < NORM_TOL
        params = dict(model.net.named_parameters())
        for k in (RESNET_GRADS if backbone == 'resnet' else XCEPTION_GRADS):
            ref_g, g64 = sd[k].grad.double(), sd64[k].grad
            got_g = (params[k].grad.double() * coef).cpu()
            assert got_g.shape == ref_g.shape, k
            amax = ref_g.abs().max().item()
            e = (ref_g - g64).abs().max().item() / g64.abs().max().item()
            err = (got_g - ref_g).abs().max().item()
            cos = float((got_g * ref_g).sum() / (got_g.norm() * ref_g.norm()))
            tol = min(max(2e-2, 4 * e), GRAD_CAP)
            print('FZ %s grad %-40s max|diff| %.3g = %.5f of |g|max %.3g (bound %.4f; oracle fp32 vs fp64 %.3g)   cos %.7f'
                  % (tag, k, err, err / amax, amax, tol, e, cos))
            assert e <= ORACLE_GRAD_TOL, (k, e)
            assert err <= tol * amax and cos > 0.999, (k, err, tol, amax, cos)
        # two more steps around a validation step: the statistics stay as loaded, nothing counted, no conv emitted statistics
        model.eval(x, y)
        assert model.net.freeze_bn is True and all(m.frozen for m in model.net.modules() if isinstance(m, BatchNorm2d))
        model.train(x, y)
        model.train(x, y)
        torch.cuda.synchronize()
        for h in hooks:
            h.remove()
        new = model.net.state_dict()
        n_stats = 0
        for k, v in w.items():
            if k.endswith('running_mean') or k.endswith('running_var'):
                assert torch.equal(new[k].cpu(), v), k
                n_stats += 1
            elif k.endswith('num_batches_tracked'):
                assert int(new[k]) == 0, k
        assert n_stats > 100 and len(seen) > 300 and not any(seen)
        assert not torch.equal(new['backbone.bn1.weight'].cpu(), w['backbone.bn1.weight'])        # ... while gamma learns
    finally:
        runtime.dropout_enabled = prev


# ---- D: eval / test unchanged ------------------------------------------------------------------------------------------------------------------
def test_eval_and_test_ignore_the_flag(dev):
    from pylc_amd.model import Model, Meta
    cfg, w, x, y = _net_case('resnet_bs2')
    outs = []
    for flag in (False, True):
        model = Model(Meta(arch='deeplab', backbone='resnet', ch=3, n_classes=9, freeze_bn=flag), dev).build()
        model.net.load_state_dict(w)
        model.net.eval()
        logits = model.test(x)[0].clone()
        ev = model.eval(x, y)[0].clone()
        outs.append((logits, ev, model.predict(x).clone()))
    for a, b in zip(*outs):
        assert torch.equal(a, b)


# ---- E: SyncBN ------------------------------------------------------------------------------------------------------------------------------
def test_frozen_step_under_a_one_rank_group(dev):
    """A one-rank process group (set up as tests/test_nets_gpu.py::test_distributed_code_path_single_rank does): the frozen step issues no
    BatchNorm collective -- the loss head's is the only one -- and its losses and gradient norm are those of the group-less step, bit for
    bit."""
    import subprocess
    import sys
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    code = r'''
import sys; sys.path.insert(0, %r)
import torch, pylc_amd
from pylc_amd import parallel, runtime
from pylc_amd.model import Model, Meta
from tests import _data as D
import oracle
from oracle import step as ostep
rank, world = parallel.init_from_env()
runtime.dropout_enabled = False
x = D.tiles(1, 2, 3, 64, 64); y = D.blob_masks(2, 2, 64, 64, 9, cell=8)
cfg = ostep.StepConfig('deeplab', 'resnet', 9, 3, dropout=False)
w = ostep.calibrate_bn(oracle.formula_state(oracle.state_spec('deeplab', 'resnet', 9, 3), salt=5), cfg, x.clone())
m = Model(Meta(freeze_bn=True), torch.device('cuda:0')).build()
m.net.load_state_dict(w)
if runtime.sync_group is not None:
    parallel.broadcast_parameters(m.arena)
before = runtime.collectives
m.train(x, y)
torch.cuda.synchronize()
print('RESULT', runtime.sync_group is not None, float(m.crit.ce), float(m.crit.dsc), float(m.crit.fl), float(m.optim.norm[0]))
print('COLLECTIVES', runtime.collectives - before)
''' % root
    res = {}
    for force in ('', '1'):
        env = dict(os.environ, MASTER_ADDR='127.0.0.1', PYLC_FORCE_PG=force, PYLC_COMM='torch')
        out = subprocess.run([sys.executable, '-c', code], env=env, capture_output=True, text=True, timeout=300)
        line = [l for l in out.stdout.splitlines() if l.startswith('RESULT')]
        assert out.returncode == 0 and line, out.stdout[-2000:] + out.stderr[-2000:]
        f = line[0].split()
        res[force] = (f[1], [float(v) for v in f[2:]])
        ncoll = int([l for l in out.stdout.splitlines() if l.startswith('COLLECTIVES')][0].split()[1])
        assert ncoll <= (2 if force else 0), ncoll          # the loss statistics' exchange; none per BatchNorm (226 in training mode)
    assert res[''][0] == 'False' and res['1'][0] == 'True'
    assert res[''][1] == res['1'][1], res


# ---- F: precision mode 3 ----------------------------------------------------------------------------------------------------------------------
def test_mode3_refuses_frozen_bn(dev):
    from pylc_amd import ops
    from pylc_amd.lib import lib, check, PylcError
    from pylc_amd.model import Model, Meta
    x = D.tiles(709, 1, 1, 64, 64)
    y = D.blob_masks(710, 1, 64, 64, 4, cell=8)
    model = Model(Meta(arch='deeplab', backbone='xception', ch=1, n_classes=4, freeze_bn=True), dev).build()
    yd = torch.zeros(1, 8, 2, 2, device=dev).contiguous(memory_format=torch.channels_last)
    v = torch.ones(8, device=dev)
    prev = lib.pylc_get_conv_precision()
    check(lib.pylc_set_conv_precision(3))
    try:
        with pytest.raises(ValueError, match='freeze_bn.*precision mode 3'):
            model.train(x, y)
        with pytest.raises(PylcError, match='freeze_bn.*precision mode 3'):
            ops.bn_act(yd, v, v, v, v, frozen=True)
    finally:
        check(lib.pylc_set_conv_precision(prev))
    assert model.iter == 0
