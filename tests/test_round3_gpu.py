"""Exports and switches of the shipped library that had no test of their own (VERDICT r2 'untested code'), and the ADVICE r2 fixes (-m gpu).

* pylc_sgd_step / FlatSGD against torch.optim.SGD(momentum=0.9) behind clip_grad_norm_ (models/model.py:246-251, :326);
* runtime.bn_clamp_eps: the vendored SyncBN's clamp(var, eps)^-1/2 (models/sync_batchnorm/batchnorm.py:125) against nn.BatchNorm2d's
  1/sqrt(var + eps);
* output_stride = 8 (models/backbone/resnet.py:64-66, models/modules/aspp.py:44-45) against the CPU oracle;
* a parameter without a gradient is SKIPPED by the flat optimisers (torch.optim semantics), not decayed;
* ResNet101.forward hands fp32 tensors to callers that did not opt into the fp16-plane format;
* a CU-masked stream runs kernels and gives the same results.
"""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu
from tests import _dw      # noqa: E402
from tests.conftest import needs_experimental      # noqa: E402


def rnd(seed, *shape, scale=1.0):
    return torch.from_numpy(np.random.RandomState(seed).standard_normal(shape).astype(np.float32) * scale)


def test_flat_sgd_matches_torch_sgd(dev):
    from pylc_amd import layers, optim
    torch.manual_seed(1)

    class Net(torch.nn.Module):
        def __init__(self):
            super().__init__()
            self.conv = layers.Conv2d(16, 24, 3, 1, 1, 1, bias=True)
            self.bn = layers.BatchNorm2d(24)
    net = Net().to(dev)
    ref = [p.detach().clone().cpu().requires_grad_(True) for p in net.parameters()]
    arena = optim.FlatArena(net)
    mine = optim.FlatSGD(arena, lr=1e-2, momentum=0.9, clip=0.5)
    theirs = torch.optim.SGD(ref, lr=1e-2, momentum=0.9)
    for step in range(4):
        mine.zero_grad()
        for i, (p, r) in enumerate(zip(net.parameters(), ref)):
            g = rnd(100 * step + i, *r.shape, scale=0.3 if step != 2 else 0.01)      # step 2: below the clip threshold
            r.grad = g.clone()
            p._pylc_grad.copy_(g.to(dev))
            arena.mark_delivered(p)
        n_ref = torch.nn.utils.clip_grad_norm_(ref, 0.5)
        theirs.step()
        mine.step()
        assert abs(mine.norm[0].item() - n_ref.item()) < 1e-5 * n_ref.item()
        for p, r in zip(net.parameters(), ref):
            assert (p.detach().cpu() - r.detach()).abs().max().item() < 5e-7, step


def test_parameter_without_gradient_is_skipped(dev):
    """torch.optim leaves a parameter whose .grad is None alone: no weight decay, no moment decay.  The flat kernels step the whole
    arena, so the optimiser restores the segments of parameters no backward kernel delivered a gradient for."""
    from pylc_amd import layers, optim
    torch.manual_seed(2)

    class Net(torch.nn.Module):
        def __init__(self):
            super().__init__()
            self.a = layers.Conv2d(8, 8, 3, 1, 1, 1)
            self.b = layers.Conv2d(8, 8, 3, 1, 1, 1)          # never receives a gradient
    for kind in ('adam', 'sgd'):
        net = Net().to(dev)
        arena = optim.FlatArena(net)
        opt = optim.FlatAdamW(arena, lr=1e-2, weight_decay=0.1) if kind == 'adam' else optim.FlatSGD(arena, lr=1e-2)
        state = (opt.m, opt.v) if kind == 'adam' else (opt.buf,)
        b0 = net.b.weight.detach().clone()
        a0 = net.a.weight.detach().clone()
        # step 1: both delivered (so that b has non-zero moments that a decay would move)
        for step in range(2):
            opt.zero_grad()
            for p in ((net.a.weight, net.b.weight) if step == 0 else (net.a.weight,)):
                p._pylc_grad.copy_(rnd(7 + step, *p.shape, scale=0.1).to(dev).permute(0, 2, 3, 1).contiguous().permute(0, 3, 1, 2))
                arena.mark_delivered(p)
            if step == 1:
                b1 = net.b.weight.detach().clone()
                o = arena.offsets[1]
                st1 = [s[o:o + b1.numel()].clone() for s in state]
            with pytest.warns(UserWarning) if step == 1 else _nowarn():
                opt.step()
        o = arena.offsets[1]
        assert not torch.equal(b0, b1) and not torch.equal(a0, net.a.weight)            # step 0 moved both
        assert torch.equal(net.b.weight.detach(), b1), kind                            # step 1 left b alone ...
        for s, s1 in zip(state, st1):
            assert torch.equal(s[o:o + b1.numel()], s1), kind                          # ... and its moments


class _nowarn:
    def __enter__(self):
        return None

    def __exit__(self, *a):
        return False


@pytest.mark.parametrize('clamp', [False, True])
def test_bn_clamp_eps_variant(dev, clamp):
    """batchnorm.py:125 computes inv_std = clamp(var, eps)^-1/2 where nn.BatchNorm2d computes (var + eps)^-1/2: the two differ by up to
    a factor sqrt(2) on channels whose variance is at or below eps, and agree to eps/var elsewhere."""
    from pylc_amd import ops
    b, c, h, w = 4, 16, 9, 7
    x = rnd(3, b, c, h, w)
    x[:, 0] *= 1e-3                      # variance ~1e-6 < eps
    x[:, 1] = 0.25                       # variance 0
    x[:, 2] *= 3e-3                      # variance ~1e-5 = eps
    ga, be = 1 + 0.1 * rnd(4, c), 0.1 * rnd(5, c)
    xd = x.to(dev).contiguous(memory_format=torch.channels_last).requires_grad_(True)
    gd, bd = ga.to(dev).requires_grad_(True), be.to(dev).requires_grad_(True)
    rm, rv = torch.zeros(c, device=dev), torch.ones(c, device=dev)
    out = ops.bn_act(xd, gd, bd, rm, rv, None, False, True, 1e-5, 0.1, None, clamp)
    dy = rnd(6, b, c, h, w)
    out.backward(dy.to(dev).contiguous(memory_format=torch.channels_last))
    x64 = x.double().requires_grad_(True)
    g64, b64 = ga.double().requires_grad_(True), be.double().requires_grad_(True)
    mean = x64.mean((0, 2, 3), keepdim=True)
    var = ((x64 - mean) ** 2).mean((0, 2, 3), keepdim=True)
    inv = var.clamp(min=1e-5) ** -0.5 if clamp else (var + 1e-5) ** -0.5             # batchnorm.py:125  /  torch.nn.BatchNorm2d
    ref = (x64 - mean) * inv * g64[None, :, None, None] + b64[None, :, None, None]
    ref.backward(dy.double())
    tol = 2e-5
    assert (out.detach().double().cpu() - ref.detach()).abs().max().item() < tol * ref.detach().abs().max().item()
    for got, want in ((xd.grad, x64.grad), (gd.grad, g64.grad), (bd.grad, b64.grad)):
        assert (got.double().cpu() - want).abs().max().item() < 5e-5 * want.abs().max().item()
    # the variants really differ on the low-variance channels (otherwise this test pins nothing)
    other = ops.bn_act(xd.detach(), gd.detach(), bd.detach(), torch.zeros(c, device=dev), torch.ones(c, device=dev), None, False, True, 1e-5, 0.1,
                       None, not clamp)
    d = (other - out.detach()).abs().amax((0, 2, 3))
    assert d[0].item() > 1e-3 and d[2].item() > 1e-3 and d[5].item() < 1e-4


@pytest.mark.parametrize('backbone,ch', [('resnet', 3), ('xception', 1)])
def test_output_stride_8_forward_matches_oracle(dev, backbone, ch):
    """DeepLab(output_stride=8) (resnet.py:64-66 strides (1,2,1,1) / dilations (1,1,2,4); xception.py:112-115; aspp.py:44-45 dilations
    (1,12,24,36)): eval-mode logits against the CPU oracle, and one training step runs (finite gradients everywhere)."""
    import oracle
    from oracle import step as ostep
    from oracle.nets import deeplab_forward
    from pylc_amd import DeepLab, runtime, ops
    from tests import _data as D
    runtime.dropout_enabled = False
    cfg = ostep.StepConfig('deeplab', backbone, 9, ch, dropout=False)
    x = D.tiles(31, 2, ch, 64, 80)
    w = oracle.formula_state(oracle.state_spec('deeplab', backbone, 9, 3), salt=4)
    xin, _ = ostep._prep(cfg, x.clone())
    sd = {k: v.clone() for k, v in w.items()}
    with torch.no_grad():
        deeplab_forward(sd, xin, backbone, True, False, None, 8, momentum=1.0)         # calibrate the running statistics at stride 8
        for k, t in sd.items():
            if k.endswith('num_batches_tracked'):
                t.zero_()
        want = deeplab_forward({k: v.clone() for k, v in sd.items()}, xin, backbone, False, False, None, 8)
    net = DeepLab(backbone=backbone, output_stride=8, n_classes=9, in_channels=ch).to(dev)
    net.load_state_dict(sd)
    net.eval()
    with torch.no_grad():
        got = net(xin.to(dev)).float().cpu()
    err = (got - want).abs().max().item()
    print('output_stride 8 (%s): eval logits max|diff| %.3g (|ref| max %.3g)' % (backbone, err, want.abs().max().item()))
    assert tuple(got.shape) == tuple(want.shape) and err < 1e-3
    net.train()
    out = net(xin.to(dev))
    out.float().square().mean().backward()
    ops.sync_side_streams()
    assert all(p.grad is not None and bool(torch.isfinite(p.grad).all()) for p in net.parameters())


def test_resnet_boundary_hands_out_fp32_unless_opted_in(dev):
    """a planes tensor is float32-typed bytes that only pylc_amd's kernels can read; the encoder's public forward converts
    unless the caller (DeepLab) opts in, and the conversion is differentiable."""
    from pylc_amd import ops, optim, runtime
    from pylc_amd.nets.encoder_resnet import ResNet101
    runtime.dropout_enabled = False
    torch.manual_seed(3)
    prev = ops.PLANES_MIN_PIXELS
    ops.PLANES_MIN_PIXELS = 0
    try:
        net = ResNet101().to(dev)
        arena = optim.FlatArena(net)          # prepared filter planes: the convs take the fp16-plane kernels
        net.train()
        x4 = ops.pack_nchw(rnd(9, 2, 3, 64, 64).to(dev), 4)
        f_pl, low_pl = net(x4, keep_planes=True)
        assert ops.is_planes(f_pl) and ops.is_planes(low_pl)
        f, low = net(x4)
        assert not ops.is_planes(f) and not ops.is_planes(low)
        assert torch.equal(f, ops.from_planes(f_pl)) and torch.equal(low, ops.from_planes(low_pl))
        # a foreign (torch) op on the exported features computes on real values, and gradients flow back through the conversion
        arena.g.zero_()
        (f.mean() + low.mean()).backward()
        ops.sync_side_streams()
        assert float(net.conv1.weight.grad.abs().sum()) > 0 and bool(torch.isfinite(arena.g).all())
    finally:
        ops.PLANES_MIN_PIXELS = prev


@needs_experimental()
def test_cu_masked_stream_runs_kernels(dev):
    from pylc_amd import ops
    from pylc_amd.lib import PylcError
    x = rnd(11, 2, 64, 40, 40).to(dev).contiguous(memory_format=torch.channels_last)
    w = rnd(12, 64, 64, 3, 3, scale=0.05).to(dev).contiguous(memory_format=torch.channels_last)
    want = ops.conv2d(x, w, None, 1, 1, 1)
    torch.cuda.synchronize()
    st = ops.cu_masked_stream(dev, 64)
    with torch.cuda.stream(st):
        got = ops.conv2d(x, w, None, 1, 1, 1)
    st.synchronize()
    assert torch.equal(got, want)
    with pytest.raises(PylcError):
        ops.cu_masked_stream(dev, 60)            # not a multiple of 8


@pytest.mark.parametrize('c,b,h,w,planes', [(256, 2, 12, 12, False), (728, 2, 9, 7, False), (64, 3, 10, 6, False), (2048, 2, 4, 4, True),
                                             (1024, 4, 32, 32, True), (8, 2, 5, 5, False)])
def test_relu_bit_mask_equals_rereading_out(dev, c, b, h, w, planes):
    """BatchNorm + residual + ReLU (resnet.py:47-51): the backward driven by the 1-bit mask the forward leaves (bn.hip relu_nibble) must
    equal, bit for bit, the backward that re-reads `out` for its mask -- dy, the residual gradient, dgamma, dbeta -- for vector-column
    counts that fill a wave (C = 256), exceed a block (2048), are not a multiple of anything convenient (728, 8) or share a wave between
    rows (64); with fp32 and with fp16-plane outputs."""
    from pylc_amd import ops, runtime
    from pylc_amd.lib import lib, check
    prev, prev_min, prev_bits = lib.pylc_get_conv_precision(), ops.PLANES_MIN_PIXELS, runtime.no_relu_bits
    check(lib.pylc_set_conv_precision(2))
    ops.PLANES_MIN_PIXELS = 0
    try:
        y = rnd(1, b, c, h, w, scale=2.0).to(dev).contiguous(memory_format=torch.channels_last)
        res = rnd(2, b, c, h, w).to(dev).contiguous(memory_format=torch.channels_last)
        dout = rnd(3, b, c, h, w).to(dev).contiguous(memory_format=torch.channels_last)
        ga, be = (1 + 0.1 * rnd(4, c)).to(dev), (0.1 * rnd(5, c)).to(dev)
        got = {}
        for bits in (False, True):
            runtime.no_relu_bits = not bits
            yy, rr = y.clone().requires_grad_(True), res.clone().requires_grad_(True)
            g, bt = ga.clone().requires_grad_(True), be.clone().requires_grad_(True)
            out = ops.bn_act(yy, g, bt, torch.zeros(c, device=dev), torch.ones(c, device=dev), rr, True, True, out_planes=planes)
            assert ops.is_planes(out) == planes
            fn = out.grad_fn
            assert (fn.saved_tensors[4] is not None) == bits and (fn.saved_tensors[1] is None) == bits       # the mask replaces `out`
            out.backward(dout)
            vis = ops.as_nhwc(out).detach()          # (as_nhwc BEFORE detach: detach() drops the fp16-plane marker)
            got[bits] = (vis.clone(), yy.grad.clone(), rr.grad.clone(), g.grad.clone(), bt.grad.clone())
        for name, a, b_ in zip(('out', 'dy', 'dres', 'dgamma', 'dbeta'), got[False], got[True]):
            assert torch.equal(a, b_), name
        # and the mask is the right one: gradient of the residual = dout where out > 0
        assert torch.equal(got[True][2], torch.where(got[True][0] > 0, dout, torch.zeros_like(dout)))
    finally:
        runtime.no_relu_bits = prev_bits
        ops.PLANES_MIN_PIXELS = prev_min
        check(lib.pylc_set_conv_precision(prev))


@pytest.mark.parametrize('planes_min', [0, 1 << 30])
def test_residual_gradient_formed_in_the_dgrad_epilogue(dev, planes_min):
    """Identity bottlenecks (resnet.py:36-51): with the 1-bit mask, bn3's backward parks (dout, mask) on the gradient link and conv1's
    dgrad adds relu'(dout) in its epilogue (pylc_conv2d_dgrad_add) instead of bn3 writing the masked gradient and conv1 accumulating
    into it.  Same arithmetic, so every gradient must be bit-identical to the written-out path -- on the fp16-plane kernels (fused
    epilogue) and on the fp32-operand kernels (where the parked pair is written out by pylc_relu_bwd_bits and accumulated as before)."""
    from pylc_amd import ops, optim, runtime
    from pylc_amd.lib import lib, check
    from pylc_amd.nets.encoder_resnet import Bottleneck
    prev, prev_min, prev_fuse, prev_drop = lib.pylc_get_conv_precision(), ops.PLANES_MIN_PIXELS, runtime.fuse_res_grad, runtime.dropout_enabled
    check(lib.pylc_set_conv_precision(2))
    ops.PLANES_MIN_PIXELS = planes_min
    runtime.dropout_enabled = False
    try:
        torch.manual_seed(4)
        net = torch.nn.Sequential(Bottleneck(256, 64, 1, 1, False), Bottleneck(256, 64, 1, 1, False), Bottleneck(256, 64, 1, 2, False)).to(dev)
        for b in net:
            b.out_planes = True
        arena = optim.FlatArena(net)
        net.train()
        x0 = rnd(1, 2, 256, 24, 20).to(dev).contiguous(memory_format=torch.channels_last)
        dout = rnd(2, 2, 256, 24, 20).to(dev).contiguous(memory_format=torch.channels_last)
        got = {}
        for fuse in (False, True):
            runtime.fuse_res_grad = fuse
            arena.g.zero_()
            x = x0.clone().requires_grad_(True)
            out = ops.export_activation(net(x))
            out.backward(dout)
            ops.sync_side_streams()
            torch.cuda.synchronize()
            got[fuse] = (x.grad.clone(), arena.g.clone())
        assert torch.equal(got[False][0], got[True][0]) and torch.equal(got[False][1], got[True][1])
        assert float(got[True][0].abs().sum()) > 0
    finally:
        runtime.fuse_res_grad, runtime.dropout_enabled = prev_fuse, prev_drop
        ops.PLANES_MIN_PIXELS = prev_min
        check(lib.pylc_set_conv_precision(prev))


@needs_experimental()
@pytest.mark.parametrize('planes_min', [0])
def test_bn_backward_sums_taken_in_the_dgrad_epilogue(dev, planes_min):
    """A conv dgrad that writes the complete gradient of a BatchNorm output takes that BatchNorm's backward sums (sum g, sum g xhat, max |g|)
    from its output tile (pylc_conv2d_dgrad_bn) and the BatchNorm backward skips its reduction pass (pylc_bn_bwd_reduce_ex): three identity
    bottlenecks (conv -> bn -> relu -> conv chains with a single consumer, and block outputs whose gradient is completed by the last
    dgrad of their gradient link, with the residual branch formed in the same epilogue).  The sums are the same numbers added in another
    order, so gradients agree to fp32 summation noise -- and the fused path really ran (launch counters)."""
    from pylc_amd import ops, optim, runtime
    from pylc_amd.lib import lib, check
    from pylc_amd.nets.encoder_resnet import Bottleneck
    prev, prev_min, prev_fuse, prev_drop = lib.pylc_get_conv_precision(), ops.PLANES_MIN_PIXELS, runtime.fuse_bn_sums, runtime.dropout_enabled
    check(lib.pylc_set_conv_precision(2))
    ops.PLANES_MIN_PIXELS = planes_min
    runtime.dropout_enabled = False
    try:
        torch.manual_seed(4)
        net = torch.nn.Sequential(Bottleneck(256, 64, 1, 1, False), Bottleneck(256, 64, 1, 1, False), Bottleneck(256, 64, 1, 2, False)).to(dev)
        for b in net:
            b.out_planes = True
        arena = optim.FlatArena(net)
        net.train()
        x0 = rnd(1, 2, 256, 40, 36).to(dev).contiguous(memory_format=torch.channels_last)
        dout = rnd(2, 2, 256, 40, 36).to(dev).contiguous(memory_format=torch.channels_last)
        got = {}
        for fuse in (False, True):
            runtime.fuse_bn_sums = fuse
            arena.g.zero_()
            ops.bn_timing = []
            x = x0.clone().requires_grad_(True)
            out = ops.export_activation(net(x))
            out.backward(dout)
            ops.sync_side_streams()
            torch.cuda.synchronize()
            kinds = [k[0] for k in ops.bn_timing]
            ops.bn_timing = None
            fused = sum(k.startswith('bwd_sums') for k in kinds)
            # 9 BatchNorms: with the fusion all but the last block's bn3 (whose dout comes from outside) take their sums from a dgrad
            assert fused == (8 if fuse else 0), kinds
            got[fuse] = (x.grad.clone(), arena.g.clone())
        for a, b in zip(got[False], got[True]):
            err = (a - b).abs().max().item()
            assert err <= 2e-5 * a.abs().max().item(), (err, a.abs().max().item())
    finally:
        runtime.fuse_bn_sums, runtime.dropout_enabled = prev_fuse, prev_drop
        ops.PLANES_MIN_PIXELS = prev_min
        ops.bn_timing = None
        check(lib.pylc_set_conv_precision(prev))


@pytest.mark.parametrize('mode', [2, 3])
@pytest.mark.parametrize('case', [(256, 48, 1, 1, 0, 2, 40, 36), (64, 64, 3, 1, 1, 2, 48, 48), (128, 64, 3, 1, 0, 2, 70, 66), (64, 128, 3, 1, 1, 2, 33, 47),
                                  (256, 64, 1, 1, 0, 4, 128, 128),
                                  # large grids (3x3: >= 512 patches, gg_plhn_kernel) -- 1x1, 3x3 padded, 3x3 valid with ragged patches and 48 of 64 columns,
                                  # dgrad into 64 channels, a strided 1x1
                                  (256, 64, 1, 1, 0, 8, 128, 128), (64, 64, 3, 1, 1, 8, 128, 128), (128, 48, 3, 1, 0, 9, 124, 126), (64, 128, 3, 1, 1, 8, 128, 132),
                                  (128, 64, 1, 2, 0, 8, 256, 258)])
def test_narrow_wave_layout_is_bit_identical(dev, case, mode):
    """Launches with at most 64 output channels (forward: Cout <= 64; dgrad: Cin <= 64) take gg_pl_kernel<.., NARROW>: 32 x 64 wave tiles,
    every wave in the first 64 columns, instead of half the waves multiplying zero filter rows -- or, 3x3 with unit steps on large grids, gg_plhn_kernel:
    four waves of 64 x 64 on a 16 x 16 patch whose halo is kept in LDS, two blocks per CU.  Same reduction order per output element:
    y, dx and dw must equal the wide form (debug flag 65536) bit for bit; the BatchNorm statistics partials to fp32 summation order."""
    from pylc_amd import ops, layers, optim
    from pylc_amd.lib import lib, check
    cin, cout, k, st, pad, B, H, W = case
    prev, prev_min = lib.pylc_get_conv_precision(), ops.PLANES_MIN_PIXELS
    check(lib.pylc_set_conv_precision(mode))
    ops.PLANES_MIN_PIXELS = 0
    try:
        torch.manual_seed(3)
        conv = layers.Conv2d(cin, cout, k, st, pad, 1, bn=True).to(dev)
        arena = optim.FlatArena(conv)
        conv.train()
        x0 = rnd(5, B, cin, H, W, scale=2.0).to(dev).contiguous(memory_format=torch.channels_last)
        got = {}
        for narrow in (False, True, 'gg_pl_kernel', 'gg_plh_kernel'):
            lib.pylc_debug_pp_flags({False: 65536 | 16384, True: 0, 'gg_pl_kernel': 16777216, 'gg_plh_kernel': 131072}[narrow])      # wide (and not the halo kernel: with one-plane operands its 32-deep chunks are another K order than gg_pl_kernel's 64-deep ones) | default (on large grids gg_plhn_kernel for 3x3 / unit steps) | gg_pl_kernel<.., NARROW> always | the wide halo kernel
            x = x0.clone().requires_grad_(True)
            y = conv(x)
            sums = y._pylc_sums.clone()
            dy = rnd(6, *y.shape).to(dev).contiguous(memory_format=torch.channels_last)
            y.backward(dy)
            ops.sync_side_streams()
            torch.cuda.synchronize()
            yv = ops.from_planes(y).detach() if ops.is_planes(y) else y.detach().clone()      # (precision mode 3: y leaves the conv as one fp16 plane)
            got[narrow] = (yv, sums, x.grad.clone(), conv.weight.grad.detach().clone())
        bad = []
        # reference: gg_pl_kernel<.., NARROW>.  With f16x3 operands (mode 2) every form is held to it bit for bit.  With one-plane operands (mode 3)
        # the halo kernels reduce in 32-channel chunks and the per-tap kernels in 64-channel ones (128-byte LDS rows) -- another K order, measured
        # 4e-7 apart on dx: there the default is compared with the wide halo kernel when it is the narrow one, with the per-tap form otherwise
        halo_case = k == 3 and st == 1 and B >= 8
        pairs = [('gg_pl_kernel', o) for o in (True, False, 'gg_plh_kernel')] if mode == 2 else [('gg_plh_kernel' if halo_case else 'gg_pl_kernel', True)]
        for base, other in pairs:
            for name, a, b in zip(('y', 'stats', 'dx', 'dw'), got[base], got[other]):
                if name == 'stats':      # per-tile column sums: the same values added over other wave tiles / tile heights (another fp32 order, other partial rows)
                    a, b = a.double().sum(0), b.double().sum(0)      # (partials per tile: 128 / 256 / 512 rows each)
                    if not (a - b).abs().max().item() <= 2e-6 * a.abs().max().item(): bad.append((name, base, other))
                elif not torch.equal(a, b):
                    bad.append((name, base, other, ((a - b).abs().max() / a.abs().max()).item()))
        assert not bad, bad
        ref = torch.nn.functional.conv2d(x0.double().cpu(), conv.weight.detach().double().cpu(), None, st, pad, 1)
        assert ((got[True][0].double().cpu() - ref).abs().max() / ref.abs().max()).item() < (3e-6 if mode == 2 else 4e-3)
    finally:
        lib.pylc_debug_pp_flags(0)
        ops.PLANES_MIN_PIXELS = prev_min
        check(lib.pylc_set_conv_precision(prev))


# ---- one-plane fp16 depthwise convs (precision mode 3): the LDS-tiled kernels and the strip kernels against an fp64 reference ----------
def _half_scale(bound):
    """The power of two pylc's kernels derive from a range bound (slab.h half_scale_for): bound -> [2^14, 2^15)."""
    e = int(np.floor(np.log2(float(bound))))
    return 2.0 ** (14 - e)


def _to_half_plane(t_nhwc, bound):
    return (t_nhwc.double() * _half_scale(bound)).to(torch.float16)


def _bits(v, dev):
    return torch.tensor([np.float32(v).view(np.int32)], dtype=torch.int32, device=dev)


@pytest.mark.parametrize('tiles', [3, 0])
@pytest.mark.parametrize('c,b,h,w,stride,dil', [(728, 2, 19, 37, 1, 1), (64, 2, 33, 16, 1, 1), (8, 1, 5, 3, 1, 1), (256, 1, 64, 64, 1, 1),
                                                (128, 2, 38, 20, 2, 1), (728, 1, 16, 34, 2, 1), (1536, 1, 17, 21, 1, 2), (8, 2, 9, 40, 1, 2)])
def test_half_depthwise_kernels_against_fp64(dev, c, b, h, w, stride, dil, tiles):
    """pylc_dwconv3x3_{fwd,dgrad,wgrad}_h -- the LDS-tiled kernels (stride 1, stride 2, dilation 2) and the strip kernels behind the A/B knob
    -- against torch's fp64 depthwise conv on the values the kernels see (the fp16 tensors, de-scaled): ragged tiles, a partial channel chunk
    (728 = 5 x 128 + 88), fewer channels than a chunk, accumulating and fp32 data gradients, the statistics partials."""
    import ctypes as C
    import torch.nn.functional as F
    from pylc_amd import lib as L, ops
    from pylc_amd.lib import lib, check, ptr, stream
    L.init()
    lib.pylc_debug_dw_tiles(tiles)
    try:
        d = ops._dw_desc(torch.empty(b, c, h, w, device='meta'), stride, dil, c, c)
        if not lib.pylc_dwconv3x3_half_ok(C.byref(d)):
            assert not tiles and (stride, dil) != (1, 1)          # only the tiled kernels cover stride 2 / dilation 2
            pytest.skip('no strip form of this geometry')
        oh, ow = d.OH, d.OW
        x = rnd(1, b, h, w, c, scale=1.5).to(dev)            # NHWC
        dy = rnd(2, b, oh, ow, c, scale=0.02).to(dev)
        wt = rnd(3, c, 1, 3, 3, scale=0.4).to(dev)
        old = rnd(4, b, h, w, c, scale=0.01).to(dev)
        xb, dyb, ob = float(x.abs().max()) * 1.1, float(dy.abs().max()) * 1.3, float(old.abs().max()) * 1.05
        x_h, dy_h, old_h = _to_half_plane(x, xb), _to_half_plane(dy, dyb), _to_half_plane(old, ob)
        xq, dyq, oldq = x_h.double() / _half_scale(xb), dy_h.double() / _half_scale(dyb), old_h.double() / _half_scale(ob)      # what the kernels see
        wa = float(wt.abs().max())
        xb_t, dyb_t, ob_t, wa_t = _bits(xb, dev), _bits(dyb, dev), _bits(ob, dev), _bits(wa, dev)      # kept alive: the kernels read them later
        x64 = xq.permute(0, 3, 1, 2).clone().requires_grad_(True)
        w64 = wt.double().clone().requires_grad_(True)
        y64 = F.conv2d(x64, w64, padding=dil, dilation=dil, stride=stride, groups=c)          # fixed_padding(k = 3): `dil` on every side
        assert tuple(y64.shape[2:]) == (oh, ow)
        dx64, dw64 = torch.autograd.grad(y64, (x64, w64), dyq.permute(0, 3, 1, 2))
        y_ref, dx_ref, dw_ref = y64.detach().permute(0, 2, 3, 1), dx64.permute(0, 2, 3, 1), dw64.view(c, 3, 3)
        # forward + statistics
        rows = lib.pylc_dwconv3x3_fwd_h_stats_rows(C.byref(d))
        assert rows > 0
        y_h = torch.zeros(b, oh, ow, c, dtype=torch.float16, device=dev)
        yb = torch.zeros(1, dtype=torch.int32, device=dev)
        sums = torch.full((rows, 2 * c), float('nan'), device=dev)
        check(lib.pylc_dwconv3x3_fwd_h(C.byref(d), ptr(x_h), ptr(xb_t), ptr(wt), ptr(wa_t), ptr(y_h), ptr(yb), ptr(sums), stream()))
        bound = yb.view(torch.float32).item()
        assert abs(bound - 9 * wa * xb) <= 1e-5 * bound and float(y_ref.abs().max()) <= bound
        assert yb.item() == _dw.bound_bits(np.float32(wa), np.float32(xb))          # by bits: every consumer derives its scale from them (tests/_dw.py)
        y = y_h.double() / _half_scale(bound)
        assert (y - y_ref).abs().max().item() <= 2.0 ** -10 * bound            # one fp16 rounding at the tensor's scale (+ fp32 accumulation)
        st = sums.double().sum(0)
        assert torch.isfinite(st).all()
        # the statistics are those of the ROUNDED halves -- the tensor the BatchNorm behind this conv normalises --, so they
        # are compared with sums over what was stored, to fp32 accumulation accuracy (against the unrounded fp64 conv they differ by fp16's 2^-11)
        ref1, ref2 = y.sum((0, 1, 2)), (y * y).sum((0, 1, 2))
        assert (st[:c] - ref1).abs().max().item() <= 2e-5 * (y.abs().sum((0, 1, 2)).max().item() + 1)
        assert ((st[c:] - ref2).abs() / (ref2 + 1e-6)).max().item() <= 2e-5
        # dgrad: fresh half output, accumulating half output, accumulating / fresh fp32 output
        dx_h = torch.zeros(b, h, w, c, dtype=torch.float16, device=dev)
        dxb = torch.zeros(1, dtype=torch.int32, device=dev)
        check(lib.pylc_dwconv3x3_dgrad_h(C.byref(d), ptr(dy_h), ptr(dyb_t), ptr(wt), ptr(wa_t), ptr(dx_h), ptr(dxb), 0, None, stream()))
        bd = dxb.view(torch.float32).item()
        assert dxb.item() == _dw.bound_bits(np.float32(wa), np.float32(dyb))
        assert (dx_h.double() / _half_scale(bd) - dx_ref).abs().max().item() <= 2.0 ** -10 * bd
        acc_h = old_h.clone()
        dxb2 = torch.zeros(1, dtype=torch.int32, device=dev)
        check(lib.pylc_dwconv3x3_dgrad_h(C.byref(d), ptr(dy_h), ptr(dyb_t), ptr(wt), ptr(wa_t), ptr(acc_h), ptr(dxb2), 1, ptr(ob_t), stream()))
        bd2 = dxb2.view(torch.float32).item()
        assert abs(bd2 - (bd + ob)) <= 1e-5 * bd2
        assert dxb2.item() == _dw.bound_bits(np.float32(wa), np.float32(dyb), np.float32(ob))
        assert (acc_h.double() / _half_scale(bd2) - (dx_ref + oldq)).abs().max().item() <= 2.0 ** -10 * bd2
        dx32 = old.clone()
        check(lib.pylc_dwconv3x3_dgrad_h(C.byref(d), ptr(dy_h), ptr(dyb_t), ptr(wt), ptr(wa_t), ptr(dx32), None, 1, None, stream()))
        assert (dx32.double() - (dx_ref + old.double())).abs().max().item() <= 1e-5 * bd
        dx32 = torch.full_like(old, float('nan'))
        check(lib.pylc_dwconv3x3_dgrad_h(C.byref(d), ptr(dy_h), ptr(dyb_t), ptr(wt), ptr(wa_t), ptr(dx32), None, 0, None, stream()))
        assert (dx32.double() - dx_ref).abs().max().item() <= 1e-5 * bd
        # dgrad + ReLU'd residual gradient under the 1-bit mask (one bit per element, element e -> bit e & 7 of byte e >> 3)
        if lib.pylc_dwconv3x3_dgrad_h_add_ok(C.byref(d)):
            keep = torch.from_numpy(np.random.RandomState(5).rand(b, h, w, c) > 0.4).to(dev)
            mask = (keep.view(-1, 8).to(torch.int32) << torch.arange(8, device=dev, dtype=torch.int32)).sum(1).to(torch.uint8)
            dx32 = torch.full_like(old, float('nan'))
            check(lib.pylc_dwconv3x3_dgrad_h_add(C.byref(d), ptr(dy_h), ptr(dyb_t), ptr(wt), ptr(wa_t), ptr(dx32), ptr(old), ptr(mask), stream()))
            assert (dx32.double() - (dx_ref + old.double() * keep)).abs().max().item() <= 1e-5 * bd
        else:
            assert not (tiles & 1) or (stride, dil) != (1, 1)
        # wgrad
        nbytes = lib.pylc_dwconv3x3_wgrad_workspace(C.byref(d))
        ws = torch.empty(nbytes // 4, device=dev)
        dw = torch.full((c, 1, 3, 3), float('nan'), device=dev)
        check(lib.pylc_dwconv3x3_wgrad_h(C.byref(d), ptr(x_h), ptr(xb_t), ptr(dy_h), ptr(dyb_t), ptr(dw), ptr(ws), nbytes, stream()))
        scale = float(b * oh * ow) ** 0.5 * xb * dyb
        assert (dw.double().view(c, 3, 3) - dw_ref).abs().max().item() <= 1e-5 * scale + 1e-6 * dw_ref.abs().max().item()
    finally:
        lib.pylc_debug_dw_tiles(3)


def test_bias_gradient_under_training_batchnorm_is_exact_zero(dev):
    """A conv bias whose only consumer is a TRAINING-mode BatchNorm (unet.py:112-118) has a mathematically zero gradient (the batch mean
    removes the bias): the HIP path returns exact zeros without a pass over dy, torch's autograd returns rounding noise of the same
    cancellation; with the BatchNorm in eval mode (running statistics) the gradient is real and is computed."""
    import torch.nn.functional as F
    from pylc_amd import layers, ops, runtime
    torch.manual_seed(3)
    conv = layers.Conv2d(16, 32, 3, 1, 1, bias=True, init='torch', bn=True).to(dev)
    bn = layers.BatchNorm2d(32).to(dev)
    x = rnd(7, 2, 16, 20, 24).to(dev).contiguous(memory_format=torch.channels_last)
    dout = rnd(8, 2, 32, 20, 24).to(dev).contiguous(memory_format=torch.channels_last)
    w_ref, b_ref = conv.weight.detach().double().cpu(), conv.bias.detach().double().cpu()
    for training in (True, False):
        conv.train(); bn.train(training)
        conv.zero_grad(); bn.zero_grad()
        out = ops.as_nhwc(bn(conv(x), relu=True))
        out.backward(dout)
        ops.sync_side_streams()
        wr, br = w_ref.clone().requires_grad_(True), b_ref.clone().requires_grad_(True)
        yr = F.conv2d(x.double().cpu(), wr, br, padding=1)
        orf = F.relu(F.batch_norm(yr, bn.running_mean.double().cpu().clone(), bn.running_var.double().cpu().clone(), bn.weight.double().cpu(), bn.bias.double().cpu(),
                                  training, 0.1, bn.eps)) if not training else \
            F.relu(F.batch_norm(yr, None, None, bn.weight.double().cpu(), bn.bias.double().cpu(), True, 0.1, bn.eps))
        orf.backward(dout.double().cpu())
        scale = wr.grad.abs().max().item()
        assert (conv.weight.grad.double().cpu() - wr.grad).abs().max().item() < 1e-4 * scale
        if training:
            assert float(conv.bias.grad.abs().max()) == 0.0 and br.grad.abs().max().item() < 1e-9 * max(scale, 1.0)
        else:
            assert br.grad.abs().max().item() > 1e-3
            assert (conv.bias.grad.double().cpu() - br.grad).abs().max().item() < 1e-4 * br.grad.abs().max().item()


def test_fold_input_affine_and_range_product(dev):
    """pylc_conv1x1_fold_input_affine: W (s (.) x + t) == (W diag s) x + W t on random data, with the folded filter's range; pylc_range_product."""
    from pylc_amd import lib as L
    from pylc_amd.lib import lib, check, ptr, stream
    L.init()
    cout, cin = 40, 728
    w, s, t, b0 = rnd(1, cout, cin).to(dev), (1 + 0.3 * rnd(2, cin)).to(dev), rnd(3, cin).to(dev), rnd(4, cout).to(dev)
    x = rnd(5, 17, cin).to(dev)
    for bias_in in (None, b0):
        w2, b2 = torch.empty_like(w), torch.empty(cout, device=dev)
        amax = torch.full((1,), -1, dtype=torch.int32, device=dev)
        check(lib.pylc_conv1x1_fold_input_affine(ptr(w), ptr(s), ptr(t), ptr(bias_in), cout, cin, ptr(w2), ptr(b2), ptr(amax), stream()))
        ref = (x.double() * s.double() + t.double()) @ w.double().t() + (0 if bias_in is None else bias_in.double())
        got = x.double() @ w2.double().t() + b2.double()
        assert (got - ref).abs().max().item() < 1e-4 * ref.abs().max().item()
        assert torch.equal(w2, w * s) and amax.view(torch.float32).item() == w2.abs().max().item()
    a, b = torch.tensor([np.float32(3.5).view(np.int32)], device=dev), torch.tensor([np.float32(0.25).view(np.int32)], device=dev)
    out = torch.zeros(1, dtype=torch.int32, device=dev)
    check(lib.pylc_range_product(ptr(a), ptr(b), 9.0, None, ptr(out), stream()))
    exact = 9.0 * 3.5 * 0.25
    assert exact <= out.view(torch.float32).item() <= exact * (1 + 4e-7)            # a bound: never below, at most an ulp or two above
    c = torch.tensor([np.float32(0.125).view(np.int32)], device=dev)
    check(lib.pylc_range_product(ptr(a), ptr(b), 9.0, ptr(c), ptr(out), stream()))
    assert exact + 0.125 <= out.view(torch.float32).item() <= (exact + 0.125) * (1 + 4e-7)


def test_grouped_batchnorm_node_equals_separate_layers(dev):
    """layers.bn_group / ops.GroupBnActFn (the node that lets the ASPP's parallel BatchNorms share one SyncBN message): without a process group
    the members run BnActFn's own code, so outputs (written into slices of one concat buffer), input gradients, parameter gradients and
    running statistics must be bit-identical to calling the BatchNorm modules one by one."""
    from pylc_amd import ops, layers
    torch.manual_seed(4)
    cs = (32, 64, 32)
    convs = [layers.Conv2d(16, c, 1, bn=True).to(dev) for c in cs]
    x = rnd(11, 2, 16, 12, 20).to(dev).contiguous(memory_format=torch.channels_last)
    dout = rnd(12, 2, sum(cs), 12, 20).to(dev).contiguous(memory_format=torch.channels_last)
    got = {}
    for grouped in (False, True):
        torch.manual_seed(5)
        bns = [layers.BatchNorm2d(c).to(dev) for c in cs]
        with torch.no_grad():
            for i, bn in enumerate(bns):
                bn.weight.add_(0.1 * rnd(20 + i, bn.num_features).to(dev))
        for m in convs + bns:
            m.train(); m.zero_grad()
        xi = x.clone().requires_grad_(True)
        buf = [ops.empty_nhwc(2, sum(cs), 12, 20, dev)]
        ys = [conv(xi) for conv in convs]
        offs = [0, cs[0], cs[0] + cs[1]]
        if grouped:
            parts = layers.bn_group([(bn, y, dict(relu=True, into=(buf, o))) for bn, y, o in zip(bns, ys, offs)])
        else:
            parts = [bn(y, relu=True, into=(buf, o)) for bn, y, o in zip(bns, ys, offs)]
        out = ops.concat_slices(buf, parts)
        out.backward(dout)
        ops.sync_side_streams()
        got[grouped] = [out.detach().clone(), xi.grad.clone()] + [p.grad.clone() for m in convs + bns for p in m.parameters()] + \
                       [bn.running_var.clone() for bn in bns]
    assert len(got[True]) == len(got[False])
    for a, b in zip(got[False], got[True]):
        assert torch.equal(a, b)


def test_gradient_ranges_come_with_the_kernels_that_write_them(dev):
    """pylc_bilinear_bwd_separable / pylc_multiloss_bwd return max|gradient written| (amax_bits) -- bit-equal to what a pass over the same
    tensor finds -- and a U-Net training step with those fused ranges (and the bound on its 1x1 up-conv outputs, ops.bound_conv_output)
    takes fewer stand-alone range passes and ends at the same parameters as with runtime.fused_grad_ranges off."""
    from pylc_amd import ops, runtime
    from pylc_amd.lib import lib, check, ptr, stream
    b, c, h, w = 2, 12, 9, 7
    dy = rnd(3, b, 4 * h, 4 * w, c).to(dev)
    dx = torch.empty(b, h, w, c, device=dev)
    ws = torch.empty(lib.pylc_bilinear_bwd_workspace(b, w, c, 4 * h) // 4, device=dev)
    amax = torch.full((1,), 123, dtype=torch.int32, device=dev)
    check(lib.pylc_bilinear_bwd_separable(ptr(dy), c, ptr(dx), c, b, h, w, c, 4 * h, 4 * w, ptr(ws), ptr(amax), stream()))
    assert amax.view(torch.float32).item() == dx.abs().max().item() > 0
    dx2 = torch.empty_like(dx)
    check(lib.pylc_bilinear_bwd_separable(ptr(dy), c, ptr(dx2), c, b, h, w, c, 4 * h, 4 * w, ptr(ws), None, stream()))
    assert torch.equal(dx, dx2)
    # loss backward: 9 classes in a 12-float pitch
    n_cls, n = 9, 2 * 16 * 16
    zz = rnd(5, 2, 16, 16, 12, scale=2.0).to(dev)
    tgt = torch.from_numpy(np.random.RandomState(6).randint(0, n_cls, (2, 16, 16))).to(dev)
    st = torch.empty(3 + 3 * n_cls, device=dev)
    wsl = torch.empty(lib.pylc_multiloss_workspace_floats(n, n_cls), device=dev)
    check(lib.pylc_multiloss_stats(ptr(zz), 12, ptr(tgt), n, n_cls, None, ptr(st), ptr(wsl), stream()))
    dl, dl2 = torch.empty_like(zz), torch.empty_like(zz)
    am = torch.full((1,), 77, dtype=torch.int32, device=dev)
    check(lib.pylc_multiloss_bwd(ptr(zz), 12, ptr(tgt), n, n_cls, None, ptr(st), float(n), 0.5, 0.5, 0.5, None, ptr(dl), 12, ptr(am), stream()))
    check(lib.pylc_multiloss_bwd(ptr(zz), 12, ptr(tgt), n, n_cls, None, ptr(st), float(n), 0.5, 0.5, 0.5, None, ptr(dl2), 12, None, stream()))
    assert am.view(torch.float32).item() == dl.abs().max().item() > 0
    assert torch.equal(dl, dl2)

    from pylc_amd.model import Model, Meta
    prev, prev_min = lib.pylc_get_conv_precision(), ops.PLANES_MIN_PIXELS
    check(lib.pylc_set_conv_precision(2))
    ops.PLANES_MIN_PIXELS = 0
    x = torch.from_numpy(np.random.RandomState(1).randint(0, 256, (2, 3, 252, 252)).astype(np.float32)).to(dev)
    y = torch.from_numpy(np.random.RandomState(2).randint(0, 9, (2, 256, 256)).astype(np.int64)).to(dev)      # cropped by 94 per side: the 68 x 68 output
    res = {}
    try:
        for fused in (True, False):
            torch.manual_seed(0)
            runtime.fused_grad_ranges = fused
            m = Model(Meta(arch='unet', ce_weight=1.0, dice_weight=0.0, focal_weight=0.0, report=10**9), dev).build()
            ops.amax_passes[:] = [0, 0]
            for _ in range(2):
                m.train(x, y)
            torch.cuda.synchronize()
            res[fused] = (ops.amax_passes[0], torch.cat([p.detach().flatten() for p in m.net.parameters()]).clone())
    finally:
        runtime.fused_grad_ranges = True
        ops.PLANES_MIN_PIXELS = prev_min
        check(lib.pylc_set_conv_precision(prev))
    assert res[True][0] < res[False][0], (res[True][0], res[False][0])
    a, bb = res[True][1], res[False][1]
    assert torch.isfinite(a).all()
    assert (a - bb).abs().max().item() <= 2e-4 * bb.abs().max().item()      # same arithmetic up to the power-of-two operand scales


def test_adamw_returns_the_parameter_ranges_of_the_next_step(dev):
    """pylc_adamw_step_ranges: same update as pylc_adamw_step bit for bit, and per-segment max|p| equal to a pass over the updated arena
    (segments from 4 floats to several chunks, one ending mid-chunk)."""
    from pylc_amd.lib import lib, check, ptr, stream
    sizes = [4, 64, 8192, 12, 20000, 36, 8188, 4, 70000]
    offs = np.concatenate([[0], np.cumsum(sizes)]).astype(np.int64)
    n = int(offs[-1])
    p0, g = rnd(1, n).to(dev), rnd(2, n, scale=0.1).to(dev)
    m0, v0 = rnd(3, n, scale=0.01).to(dev), rnd(4, n, scale=0.01).abs().to(dev)
    coef = torch.tensor([1.0, 0.7], device=dev)
    seg = torch.from_numpy(offs).to(dev)
    p1, m1, v1 = p0.clone(), m0.clone(), v0.clone()
    check(lib.pylc_adamw_step(ptr(p1), ptr(g), ptr(m1), ptr(v1), n, ptr(coef), 1e-2, 0.9, 0.999, 1e-8, 5e-2, 3, stream()))
    p2, m2, v2 = p0.clone(), m0.clone(), v0.clone()
    amax = torch.full((len(sizes),), 99, dtype=torch.int32, device=dev)
    check(lib.pylc_adamw_step_ranges(ptr(p2), ptr(g), ptr(m2), ptr(v2), n, ptr(coef), 1e-2, 0.9, 0.999, 1e-8, 5e-2, 3, ptr(seg), len(sizes), ptr(amax),
                                     stream()))
    assert torch.equal(p1, p2) and torch.equal(m1, m2) and torch.equal(v1, v2)
    ref = torch.zeros_like(amax)
    check(lib.pylc_amax_segments(ptr(p2), ptr(seg), len(sizes), ptr(ref), stream()))
    assert torch.equal(amax, ref)
    want = torch.stack([p2[int(offs[i]):int(offs[i + 1])].abs().max() for i in range(len(sizes))])
    assert torch.equal(amax.view(torch.float32), want)


@pytest.mark.parametrize('mode', [2, 3])
def test_image_pool_over_planes_equals_pool_of_the_converted_tensor(dev, mode):
    """pylc_gap_fwd_planes (aspp.py:59-63 on the fp16 planes the backbone's last BatchNorm leaves): bit-identical to pylc_from_planes followed
    by pylc_gap_fwd, for two planes (f16x3) and one (precision mode 3); ops.global_avg_pool takes that path for a planes tensor."""
    from pylc_amd import ops
    from pylc_amd.lib import lib, check
    prev = lib.pylc_get_conv_precision()
    check(lib.pylc_set_conv_precision(mode))
    try:
        b, c, h, w = 3, 72, 13, 9
        x = rnd(11, b, c, h, w, scale=3.0).to(dev)
        xp = ops.to_planes(x)
        ref = ops.global_avg_pool(ops.from_planes(xp))
        got = ops.global_avg_pool(xp)
        assert got.shape == (b, c, 1, 1) and torch.equal(got, ref)
        assert (got.flatten(1) - x.mean((2, 3))).abs().max().item() < (2e-3 if mode == 3 else 1e-5) * 3.0
    finally:
        check(lib.pylc_set_conv_precision(prev))
