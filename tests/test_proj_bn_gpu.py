"""The fused projection-pair BatchNorm node (ops.BnPairFn, pylc_bn_*_pair) on the GPU (-m gpu):
relu(bn3(y3) + bn_ds(y_ds)) of a projection bottleneck as ONE node against the two BatchNorm nodes it replaces (bit identity: same
arithmetic in the same order), against an fp64 torch restatement, and at block / network level with the runtime knob on versus off."""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

from tests import _data as D

pytestmark = pytest.mark.gpu


def rnd(seed, *shape, scale=1.0):
    return torch.from_numpy(np.random.RandomState(seed).standard_normal(shape).astype(np.float32) * scale)


def rel_err(a, b):
    a, b = a.double().cpu(), b.double().cpu()
    return ((a - b).abs().max() / (b.abs().max() + 1e-30)).item()


def same_bits(a, b):
    """Equality of the BYTES (an fp16-plane tensor is float32-typed: its words may be NaN patterns)."""
    return a.shape == b.shape and torch.equal(a.contiguous().view(torch.int32) if a.dtype == torch.float32 else a,
                                              b.contiguous().view(torch.int32) if b.dtype == torch.float32 else b)


class _Mode2:
    """Precision mode 2 with a chosen planes threshold; restores every global it touches."""

    def __init__(self, planes_min):
        self.planes_min = planes_min

    def __enter__(self):
        from pylc_amd import ops, runtime
        from pylc_amd import lib as L
        from pylc_amd.lib import lib, check
        L.init()
        self.prev = (lib.pylc_get_conv_precision(), ops.PLANES_MIN_PIXELS, runtime.fuse_proj_bn, runtime.dropout_enabled, runtime.bn_clamp_eps)
        check(lib.pylc_set_conv_precision(2))
        ops.PLANES_MIN_PIXELS = self.planes_min
        runtime.dropout_enabled = False
        return self

    def __exit__(self, *a):
        from pylc_amd import ops, runtime
        from pylc_amd.lib import lib, check
        ops.bn_timing = None
        ops.PLANES_MIN_PIXELS, runtime.fuse_proj_bn, runtime.dropout_enabled, runtime.bn_clamp_eps = self.prev[1:]
        check(lib.pylc_set_conv_precision(self.prev[0]))
        return False


# ---- the slab rule of the row-slab kernels (pylc_amd/csrc/slab.h make_slab), mirrored to CHOOSE a shape -------------------------------------
def _slabs(m, c, limit=512):
    cv = c // 4
    cols = min(cv, 256)
    rl = 256 // cols
    rps = max(-(-m // limit), rl * 8)
    rps = -(-rps // rl) * rl
    return -(-m // rps), rps


def _ragged_multi_slab_m(c):
    """An M at which the reduce runs three slabs, the last one short and not a multiple of the row batch."""
    from pylc_amd.lib import lib
    _, rps = _slabs(1, c)
    m = 2 * rps + 37
    n, rps2 = _slabs(m, c)
    assert rps2 == rps and n == 3 and m % rps not in (0, rps) and n <= lib.pylc_bn_workspace_floats(m, c) // (2 * c)
    return m


# (b, h, w, c): M = b*h*w
SHAPES = {
    'M70_C8': (2, 5, 7, 8),            # the smallest C the mask format takes; rows not a multiple of any row batch
    'M70_C40': (2, 5, 7, 40),          # CV = 10: not a power of two, inactive lanes in a block
    'M1030_C264': (2, 5, 103, 264),    # 43 slabs of 24 rows, the last one 22
    'M70_C64': (2, 5, 7, 64),          # C % 32 == 0: the chunk-interleaved plane format
    'M38_C1032': (2, 19, 1, 1032),     # CV = 258 > 256: a second column round with two active columns
    'ragged_C40': None,                # filled below from the slab rule (three slabs, ragged last)
}


def _shape(name):
    if name == 'ragged_C40':
        m = _ragged_multi_slab_m(40)
        assert m == 437
        return (1, 19, 23, 40)
    return SHAPES[name]


def _leaf(t, dev, extra):
    """Device copy of an [B,C,H,W] tensor with NHWC memory at pitch C + extra, as a leaf that takes a gradient."""
    from pylc_amd import ops
    b, c, h, w = t.shape
    buf = ops.empty_nhwc(b, c, h, w, dev, pitch=c + extra)
    buf.copy_(t.to(dev))
    return buf.requires_grad_(True)


def _pair_case(dev, shape, planes, extra, fused):
    """One forward + backward of relu(bn3(y3) + bn_ds(y_ds)) through the pair node (fused) or the two BnActFn nodes; returns every
    result by name.  planes: `out` and both dy as fp16 planes.  extra: pitch beyond C of y_ds and dout."""
    from pylc_amd import ops
    b, h, w, c = shape
    m = b * h * w
    y3 = 2.0 * rnd(1, b, c, h, w) + 0.5
    y2 = 1.5 * rnd(2, b, c, h, w) - 0.3
    y2[:, min(3, c - 1)] = 1000.0 + 0.5 * rnd(3, b, h, w)          # |mean| >> sigma: the shortcut's variance is re-measured (bn.hip kRefineRatio)
    dout = rnd(4, b, c, h, w)
    y3d, y2d, doutd = _leaf(y3, dev, 0), _leaf(y2, dev, extra), _leaf(dout, dev, extra).detach()
    if planes:
        y3d._pylc_dy_pl = True          # what the producing conv asks for (ops.conv2d): dy as fp16 planes
        y2d._pylc_dy_pl = True
    par = [(1 + 0.1 * rnd(5 + i, c)).to(dev).requires_grad_(True) if i % 2 == 0 else (0.1 * rnd(5 + i, c)).to(dev).requires_grad_(True) for i in range(4)]
    g3, b3, g2, b2 = par
    rm3, rv3, rm2, rv2 = (0.1 * rnd(9, c)).to(dev), (1 + 0.1 * rnd(10, c).abs()).to(dev), (0.1 * rnd(11, c)).to(dev), (1 + 0.1 * rnd(12, c).abs()).to(dev)
    if fused:
        out = ops.bn_act_pair(y3d, g3, b3, rm3, rv3, 1e-5, 0.1, y2d, g2, b2, rm2, rv2, 1e-5, 0.1, out_planes=planes)
        fn = out.grad_fn
        coef3, coef2, mask = fn.saved_tensors[2], fn.saved_tensors[3], fn.saved_tensors[4]
    else:
        res = ops.bn_act(y2d, g2, b2, rm2, rv2, None, False, True)
        out = ops.bn_act(y3d, g3, b3, rm3, rv3, res, True, True, out_planes=planes)
        coef3, mask, coef2 = out.grad_fn.saved_tensors[2], out.grad_fn.saved_tensors[4], res.grad_fn.saved_tensors[2]
    assert ops.is_planes(out) == planes and mask is not None
    got = {'out': out.detach().clone(), 'out_range': (ops.planes_amax(out) if planes else out._pylc_amax[0]).clone(), 'mask': mask.clone(),
           'coef3': coef3.clone(), 'coef_ds': coef2.clone()}
    out.backward(doutd)
    torch.cuda.synchronize()
    got.update(rm3=rm3, rv3=rv3, rm_ds=rm2, rv_ds=rv2, dgamma3=g3.grad, dbeta3=b3.grad, dgamma_ds=g2.grad, dbeta_ds=b2.grad,
               dy3=y3d.grad, dx_ds=y2d.grad)
    return got


@pytest.mark.parametrize('planes', [False, True])
@pytest.mark.parametrize('name,extra', [('M70_C8', 0), ('M70_C40', 0), ('M1030_C264', 0), ('ragged_C40', 0), ('M38_C1032', 0), ('M70_C64', 0), ('M70_C40', 8),
                                        ('M1030_C264', 24)])
def test_pair_node_equals_the_two_batchnorm_nodes(dev, name, extra, planes):
    """Every result of the pair node -- out (fp32 or both planes) and its range, the mask bits, mean / invstd / scale / shift and the
    running statistics of both BatchNorms, dgamma / dbeta of both, dy3 and dx_ds (fp32 or planes) -- has the bits of the unfused
    sequence; dbeta of the shortcut IS bn3's (one sum)."""
    shape = _shape(name)
    with _Mode2(0):
        ref = _pair_case(dev, shape, planes, extra, fused=False)
        got = _pair_case(dev, shape, planes, extra, fused=True)
    for k in ref:
        assert same_bits(ref[k], got[k]), k
    assert same_bits(got['dbeta_ds'], got['dbeta3'])
    assert float(got['dgamma_ds'].abs().sum()) > 0 and float(got['mask'].float().sum()) > 0


@pytest.mark.parametrize('name', ['M70_C8', 'M70_C40', 'M1030_C264'])
def test_pair_node_against_fp64(dev, name):
    """Batch-statistics BatchNorm of both inputs, add, ReLU and the backward restated in fp64 torch; the bounds are those
    tests/test_ops_gpu.py::test_bn_train applies to the unfused kernels."""
    from pylc_amd import ops
    b, h, w, c = _shape(name)
    y3, y2 = 2.0 * rnd(21, b, c, h, w) + 0.5, 1.5 * rnd(22, b, c, h, w) - 0.3
    par = [1 + 0.1 * rnd(23, c), 0.1 * rnd(24, c), 1 + 0.1 * rnd(25, c), 0.1 * rnd(26, c)]
    run = [0.1 * rnd(27, c), 1 + 0.1 * rnd(28, c).abs(), 0.1 * rnd(29, c), 1 + 0.1 * rnd(30, c).abs()]
    dout = rnd(31, b, c, h, w)
    y3r, y2r = y3.double().requires_grad_(True), y2.double().requires_grad_(True)
    parr = [p.double().requires_grad_(True) for p in par]
    runr = [r.double().clone() for r in run]
    o = F.relu(F.batch_norm(y3r, runr[0], runr[1], parr[0], parr[1], True, 0.1, 1e-5) + F.batch_norm(y2r, runr[2], runr[3], parr[2], parr[3], True, 0.1, 1e-5))
    o.backward(dout.double())
    with _Mode2(1 << 30):
        y3d, y2d = _leaf(y3, dev, 0), _leaf(y2, dev, 0)
        pard = [p.to(dev).requires_grad_(True) for p in par]
        rund = [r.to(dev) for r in run]
        od = ops.bn_act_pair(y3d, pard[0], pard[1], rund[0], rund[1], 1e-5, 0.1, y2d, pard[2], pard[3], rund[2], rund[3], 1e-5, 0.1)
        od.backward(dout.to(dev).contiguous(memory_format=torch.channels_last))
        torch.cuda.synchronize()
    errs = {'out': (rel_err(od, o), 5e-6), 'dy3': (rel_err(y3d.grad, y3r.grad), 2e-5), 'dx_ds': (rel_err(y2d.grad, y2r.grad), 2e-5)}
    for i, k in enumerate(('rm3', 'rv3', 'rm_ds', 'rv_ds')):
        errs[k] = (rel_err(rund[i], runr[i]), 1e-6 if i % 2 == 0 else 2e-6)
    for i, k in enumerate(('dgamma3', 'dbeta3', 'dgamma_ds', 'dbeta_ds')):
        errs[k] = (rel_err(pard[i].grad, parr[i].grad), 2e-5)
    print(name, {k: '%.3g' % v[0] for k, v in errs.items()})
    for k, (e, tol) in errs.items():
        assert e < tol, (k, e, tol)


# ---- block level ----------------------------------------------------------------------------------------------------------------------------
def _block_run(dev, net, arena, x0, dout, fuse):
    from pylc_amd import ops, runtime
    runtime.fuse_proj_bn = fuse
    arena.g.zero_()
    x = x0.clone().requires_grad_(True)
    ops.bn_timing = []
    out = ops.export_activation(net(x))
    out.backward(dout)
    ops.sync_side_streams()
    torch.cuda.synchronize()
    kinds = [(k[0], k[1], k[2]) for k in ops.bn_timing]
    ops.bn_timing = None
    bufs = [b_.clone() for b_ in net.buffers()]
    return out.detach().clone(), x.grad.clone(), arena.g.clone(), bufs, kinds


def _two_blocks(dev, s, seed=4):
    from pylc_amd import optim
    from pylc_amd.nets.encoder_resnet import Bottleneck
    torch.manual_seed(seed)
    net = torch.nn.Sequential(Bottleneck(32, 16, s, 1, True), Bottleneck(64, 16, 1, 1, False)).to(dev)
    for blk in net:
        blk.out_planes = True
    return net, optim.FlatArena(net)


def _reset_running(net):
    for m_ in net.modules():
        if hasattr(m_, 'running_mean'):
            m_.running_mean.zero_()
            m_.running_var.fill_(1.0)


@pytest.mark.parametrize('planes_min', [1 << 30, 0])
@pytest.mark.parametrize('s', [1, 2])
def test_block_knob_on_equals_knob_off(dev, s, planes_min):
    """Projection + identity bottleneck: output, input gradient, the whole gradient arena and the running statistics are the same with
    the pair node and with the two nodes, on fp32 activations and on fp16 planes; the +proj passes run exactly when the knob is on, and
    then neither a +gres pass nor a stand-alone apply of the shortcut (the only plain `apply` over 64 channels) does."""
    with _Mode2(planes_min):
        net, arena = _two_blocks(dev, s)
        net.train()
        x0 = rnd(1, 2, 32, 18, 14).to(dev).contiguous(memory_format=torch.channels_last)
        ho, wo = (18 + s - 1) // s, (14 + s - 1) // s
        dout = rnd(2, 2, 64, ho, wo).to(dev).contiguous(memory_format=torch.channels_last)
        got = {}
        for fuse in (False, True):
            _reset_running(net)
            got[fuse] = _block_run(dev, net, arena, x0, dout, fuse)
    for i, what in enumerate(('out', 'dx', 'arena')):
        assert torch.equal(got[False][i], got[True][i]), what
    for a, b_ in zip(got[False][3], got[True][3]):
        assert torch.equal(a, b_)
    assert float(got[True][1].abs().sum()) > 0
    on, off = [k[0] for k in got[True][4]], [k[0] for k in got[False][4]]
    m = 2 * ho * wo
    planes = planes_min == 0          # a plane output: one read of the shortcut's y for the residual's range (the two nodes measure it while writing)
    assert sorted(k for k in on if k.endswith('+proj')) == ['apply+res+bits+proj'] + ['apply_range+proj'] * planes + ['bwd_apply+proj', 'bwd_reduce(+sums)+proj']
    assert not [k for k in off if '+proj' in k]
    assert not [k for k in on if '+gres' in k] and [k for k in off if '+gres' in k] == ['bwd_apply+gres']
    assert ('apply', m, 64) not in got[True][4] and got[False][4].count(('apply', m, 64)) == 1
    assert len(off) - len(on) == 3 - planes          # apply (a read-only range pass with planes), bwd_reduce and bwd_apply of the shortcut are gone


def _fallback_equal(dev, net, arena, x0, dout):
    got = {}
    for fuse in (False, True):
        _reset_running(net)
        got[fuse] = _block_run(dev, net, arena, x0, dout, fuse)
    for i in range(3):
        assert torch.equal(got[False][i], got[True][i])
    assert [k[0] for k in got[True][4]] == [k[0] for k in got[False][4]] and not [k for k in got[True][4] if '+proj' in k[0]]
    return got


@pytest.mark.parametrize('case', ['frozen', 'clamp_eps', 'c_not_multiple_of_8', 'identity_only'])
def test_fallbacks_take_the_two_node_path(dev, case):
    """Frozen BatchNorm, the clamped inverse deviation and a block whose C % 8 != 0 run the two BatchNorm nodes whatever the knob says:
    same passes, same bits.  Identity blocks never see the pair node."""
    from pylc_amd import optim, runtime
    from pylc_amd.layers import BatchNorm2d, Conv2d, Named
    from pylc_amd.nets.encoder_resnet import Bottleneck
    with _Mode2(1 << 30):
        cout = 64
        if case == 'c_not_multiple_of_8':
            # 60 output channels (BatchNorm needs C % 4 == 0; the mask format C % 8 == 0): conv3 / bn3 / shortcut of one block re-made at that width
            torch.manual_seed(5)
            blk = Bottleneck(32, 16, 1, 1, True)
            cout = 60
            blk.conv3, blk.bn3 = Conv2d(16, cout, 1, bn=True), BatchNorm2d(cout)
            blk.downsample = Named(_0=Conv2d(32, cout, 1, 1, bn=True), _1=BatchNorm2d(cout))
            net = torch.nn.Sequential(blk).to(dev)
            arena = optim.FlatArena(net)
            assert not blk.pair_eligible()
        elif case == 'identity_only':
            torch.manual_seed(6)
            net = torch.nn.Sequential(Bottleneck(64, 16, 1, 1, False), Bottleneck(64, 16, 1, 1, False)).to(dev)
            arena = optim.FlatArena(net)
        else:
            net, arena = _two_blocks(dev, 1)
        net.train()
        if case == 'frozen':
            for m_ in net.modules():
                if isinstance(m_, BatchNorm2d):
                    m_.frozen = True
                elif isinstance(m_, Conv2d):
                    m_.bn_frozen = True
        if case == 'clamp_eps':
            runtime.bn_clamp_eps = True
        cin = 64 if case == 'identity_only' else 32
        x0 = rnd(1, 2, cin, 18, 14).to(dev).contiguous(memory_format=torch.channels_last)
        dout = rnd(2, 2, cout, 18, 14).to(dev).contiguous(memory_format=torch.channels_last)
        _fallback_equal(dev, net, arena, x0, dout)


def test_eval_mode_takes_the_two_node_path(dev):
    """eval(): the inference fusion (conv epilogue) with autograd off, the eval-mode BatchNorm nodes with it on -- never the pair node."""
    from pylc_amd import ops, runtime
    with _Mode2(1 << 30):
        net, arena = _two_blocks(dev, 2)
        net.eval()
        x0 = rnd(1, 2, 32, 18, 14).to(dev).contiguous(memory_format=torch.channels_last)
        dout = rnd(2, 2, 64, 9, 7).to(dev).contiguous(memory_format=torch.channels_last)
        outs = {}
        for fuse in (False, True):
            runtime.fuse_proj_bn = fuse
            ops.bn_timing = []
            with torch.no_grad():
                outs[fuse] = ops.export_activation(net(x0)).clone()
            assert not [k for k in ops.bn_timing if '+proj' in k[0]]
            ops.bn_timing = None
        assert torch.equal(outs[False], outs[True])
        _fallback_equal(dev, net, arena, x0, dout)


# ---- network level --------------------------------------------------------------------------------------------------------------------------
def test_two_training_steps_knob_on_equals_knob_off(dev):
    """Two Model.train steps of DeepLabV3+/ResNet-101 on 2x3x96x96 tiles from the same weights: every parameter and BatchNorm buffer is
    the same with the pair node and without (fp32 activations: 96x96 tiles are below the planes threshold)."""
    import oracle
    from pylc_amd import ops, runtime
    from pylc_amd.model import Model, Meta
    x = D.tiles(1, 2, 3, 96, 96)
    y = D.blob_masks(2, 2, 96, 96, 9, cell=8)
    w = oracle.formula_state(oracle.state_spec('deeplab', 'resnet', 9, 3), salt=5)
    states, seen = {}, {}
    with _Mode2(ops.PLANES_MIN_PIXELS):
        for fuse in (False, True):
            runtime.fuse_proj_bn = fuse
            runtime.manual_seed(7)
            model = Model(Meta(), dev).build()
            model.net.load_state_dict(w)
            model.train(x, y)
            ops.bn_timing = []
            model.train(x, y)
            torch.cuda.synchronize()
            seen[fuse] = [k[0] for k in ops.bn_timing]
            ops.bn_timing = None
            states[fuse] = {k: v.detach().clone() for k, v in model.net.state_dict().items()}
    assert sum(k.endswith('+proj') for k in seen[True]) == 12 and not [k for k in seen[False] if '+proj' in k]      # four projection blocks
    assert sum('+gres' in k for k in seen[False]) - sum('+gres' in k for k in seen[True]) == 4
    assert states[False].keys() == states[True].keys()
    for k in states[False]:
        assert torch.equal(states[False][k], states[True][k]), k
