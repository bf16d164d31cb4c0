"""Every class count 2..16 (PYLC_MAX_CLASSES) through the kernels that hold one instantiation per count (-m gpu).

The reference ships two schemas, 9 and 11 classes, and the rest of the suite follows it; a `Meta(n_classes=5)` of a user's own runs
`multiloss_stats_kernel<5>`, `stitch_argmax_kernel<5>` and a head conv with Cout 5 at pitch 8.  Here every count runs once, against references
that already exist.  Per section, what is compared and its bound.  Every test prints its figures next to its bounds (lines `CC1` .. `CC5` under
`pytest -s`).  MEASURED SO FAR: on an MI355X every test of sections 1 - 4 and the DeepLab steps at 2 and 5 classes passed within these
bounds, but that run kept the figures of one case only, the DeepLab step at 16 classes with the weights of salt 20 + 16: eval logits
1.5e-4 (rms 3.2e-5), losses 1.2e-6, pre-clip norm 3.1e-3 -- over its bound, because the fp32 oracle of that case is itself 1.8e-3 off its
fp64 evaluation (test_network_step_against_oracle; the case now takes the next salt).  The worst figure of each line over the sweep still
belongs here.

  1  loss head through ops.multiloss (C x weighted / unweighted; 874 pixels, one class absent) against oracle.multiloss on fp64 leaves:
     losses within 2e-6 max(1, |v|), logits.grad within 1e-5 of its largest entry (test_multiloss_golden's bounds; the fp32 oracle is within
     1.6e-7 / 3.6e-7), the same for the single-term weights of the validation path and for grad_scale = 3; lanes [C, round4(C)) of the
     gradient buffer exact zeros.
  2  the same, same bounds, through the C ABI: pitch = dpitch = round4(C) + 4 with 1e9 in the unused logit lanes and NaN in dlogits (lanes
     [C, round4) zero, lanes from round4 up still NaN, amax_bits the bits of max |dlogits|); the two-shard wire format (stats of two half
     batches added, finalize and both backward calls on the global count); C = 1 and 17 refused by name before anything is written.
  3  conv 1x1 256 -> C with bias -> bilinear 12 x 10 -> 48 x 40 -> weighted loss head -> backward, in the default conv precision, against the
     same chain in fp64 torch: logits / loss / dx / dw / db within 3.0e-6 / 2e-6 / 4e-6 / 5e-6 / 2e-6 (test_head_chain derives them; fp32
     torch on the CPU: 7.4e-7 / 1.4e-7 / 5.1e-7 / 5.2e-7 / 3.4e-7).
  4  pylc_stitch_argmax at stride = tile and tile / 2 (exact off the oracle's near-ties, which the seeds leave empty), first-maximum ties.
     (pylc_logits_score and the overlap stitcher sweep C in tests/test_score_gpu.py and tests/test_unet_inference_gpu.py.)
  5  DeepLabV3+/ResNet-101 (64^2, bs 2) and U-Net (256^2 -> 68^2, bs 1) at 2, 5 and 16 classes against oracle.step: eval logits 1e-3 with the
     argmax exact off near-ties, losses 1e-3, pre-clip norm 2e-3 (at weights for which the fp32 oracle is within 5e-4 of its own fp64 norm), head filter / bias gradients within 2e-2 of their largest entry at cosine
     > 0.999, Model.predict == argmax of Model.test.

Targets stay inside [0, C): the loss kernels index the class weights with them."""
import functools

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from tests import _data as D
from tests.test_ops_gpu import rnd, rel_err, to_dev_nhwc

pytestmark = pytest.mark.gpu

ALL_C = range(2, 17)
LOSS_REL = 2e-6           # test_multiloss_golden's bounds (C = 9 / 11); the fp32 oracle itself is within 1.6e-7 / 3.6e-7 of the fp64 one on these inputs
GRAD_REL = 1e-5
HALF = (0.5, 0.5, 0.5)


def r4(c):
    return (c + 3) & ~3


def _padded(t):
    """the [B, round4(C), H, W] view of an NHWC tensor with pitch round4(C) (test_conv_fwd_bwd's view of its padded logits)"""
    return torch.as_strided(t, (t.shape[0], r4(t.shape[1]), t.shape[2], t.shape[3]), t.stride(), t.storage_offset())


# ---- 1 / 2: the loss head --------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _loss_inputs(c):
    z = torch.from_numpy((np.random.RandomState(300 + c).standard_normal((2, c, 19, 23)) * 3).astype(np.float32))      # 874 pixels: four blocks
    t = D.blob_masks(301 + c, 2, 19, 23, c, cell=4)
    if c > 2:
        t[t == c - 1] = 0            # the last class is absent: a Dice term with zero count, a class weight that is never read
    return z, t, torch.from_numpy(D.class_weights(c))


@functools.lru_cache(maxsize=None)
def _loss_ref(c, weighted, weights=HALF):
    """oracle.multiloss on float64 leaves: ([total, ce, dice, focal], d total / d logits); shared by the tests below, which only read it"""
    import oracle
    z, t, cw = _loss_inputs(c)
    zr = z.double().requires_grad_(True)
    out = oracle.multiloss(zr, t, weights, cw.double(), weighted)
    out[0].backward()
    return [v.item() for v in out], zr.grad.detach()


def _loss_err(got, want):
    return max(abs(a - b) / max(1.0, abs(b)) for a, b in zip(got, want))


@pytest.mark.parametrize('weighted', [False, True], ids=['unweighted', 'weighted'])
@pytest.mark.parametrize('c', ALL_C)
def test_multiloss_every_class_count(dev, c, weighted):
    from pylc_amd import ops
    z, t, cw = _loss_inputs(c)
    want, g = _loss_ref(c, weighted)
    assert 0 <= int(t.min()) and int(t.max()) < c
    zd = to_dev_nhwc(z, dev).requires_grad_(True)
    raw = []
    zd.register_hook(raw.append)                 # the buffer pylc_multiloss_bwd wrote (autograd may copy it into .grad)
    losses = ops.multiloss(zd, t.to(dev), cw.to(dev) if weighted else None, *HALF)
    losses[0].backward(retain_graph=True)
    el, eg = _loss_err(losses.detach().cpu().tolist(), want), rel_err(zd.grad, g)
    dl = raw[0]
    assert tuple(dl.shape) == tuple(z.shape) and ops.pitch_of(dl) == r4(c)
    pad = float(_padded(dl)[:, c:].abs().max()) if r4(c) > c else 0.0
    zd.grad = None
    (3 * losses[0]).backward()                   # grad_scale
    e3 = rel_err(zd.grad, 3 * g)
    print('CC1 C %2d %s: losses %.3g (bound %.3g)  grad %.3g  grad x3 %.3g (bound %.3g)  pad lanes %g'
          % (c, 'w' if weighted else 'u', el, LOSS_REL, eg, e3, GRAD_REL, pad))
    assert el < LOSS_REL and eg < GRAD_REL and e3 < GRAD_REL
    assert pad == 0.0


@pytest.mark.parametrize('c', [2, 5, 16])
def test_multiloss_single_terms(dev, c):
    """MultiLoss.ce_loss / dice_loss / focal_loss, the three calls of the validation path: loss weights (1,0,0), (0,1,0), (0,0,1)"""
    from pylc_amd.loss import MultiLoss
    z, t, cw = _loss_inputs(c)
    crit = MultiLoss({'weighted': True, 'weights': cw.numpy(), 'ce': 0.5, 'dice': 0.5, 'focal': 0.5}, {'n_classes': c}).to(dev)
    for k, name in enumerate(('ce_loss', 'dice_loss', 'focal_loss')):
        weights = tuple(1.0 if i == k else 0.0 for i in range(3))
        want, g = _loss_ref(c, True, weights)
        zd = to_dev_nhwc(z, dev).requires_grad_(True)
        loss = getattr(crit, name)(zd, t.to(dev))
        loss.backward()
        el, eg = _loss_err([loss.item()], [want[0]]), rel_err(zd.grad, g)
        print('CC1 C %2d %s: loss %.3g (bound %.3g)  grad %.3g (bound %.3g)' % (c, name, el, LOSS_REL, eg, GRAD_REL))
        assert abs(want[0] - want[1 + k]) < 1e-12            # (the reference's total IS the single term)
        assert el < LOSS_REL and eg < GRAD_REL


def _abi_buffers(dev, c, pitch, dpitch):
    """pixel rows of _loss_inputs(c) at `pitch` with 1e9 in the unused lanes (test_score_gpu._nchw_view's filling), NaN dlogits at `dpitch`"""
    z, t, cw = _loss_inputs(c)
    n = z.shape[0] * z.shape[2] * z.shape[3]
    buf = torch.full((n, pitch), 1e9, dtype=torch.float32)
    buf[:, :c] = z.permute(0, 2, 3, 1).reshape(n, c)
    dl = torch.full((n, dpitch), float('nan'), dtype=torch.float32, device=dev)
    return buf.to(dev), t.reshape(n).contiguous().to(dev), cw.to(dev), dl, n


def _abi_loss(dev, c, pitch, dpitch, shards):
    """stats -> (sum over shards) -> finalize -> bwd per shard, all on the global pixel count: (losses, dlogits [N, dpitch], amax bits per shard)"""
    from pylc_amd import lib as L
    from pylc_amd.lib import lib, check, ptr, stream
    L.init()
    buf, t, cw, dl, n = _abi_buffers(dev, c, pitch, dpitch)
    k = 3 + 3 * c
    bounds = [n * i // shards for i in range(shards + 1)]
    parts = []
    for lo, hi in zip(bounds[:-1], bounds[1:]):
        stats = torch.full((k,), float('nan'), device=dev)
        ws = torch.empty(lib.pylc_multiloss_workspace_floats(hi - lo, c), device=dev)
        check(lib.pylc_multiloss_stats(ptr(buf[lo:]), pitch, ptr(t[lo:]), hi - lo, c, ptr(cw), ptr(stats), ptr(ws), stream()))
        parts.append(stats)
    stats = torch.stack(parts).sum(0)
    losses = torch.full((4,), float('nan'), device=dev)
    check(lib.pylc_multiloss_finalize(ptr(stats), float(n), c, *HALF, ptr(losses), stream()))
    amax = torch.full((shards,), -1, dtype=torch.int32, device=dev)
    for i, (lo, hi) in enumerate(zip(bounds[:-1], bounds[1:])):
        check(lib.pylc_multiloss_bwd(ptr(buf[lo:]), pitch, ptr(t[lo:]), hi - lo, c, ptr(cw), ptr(stats), float(n), *HALF, None,
                                     ptr(dl[lo:]), dpitch, ptr(amax[i:]), stream()))
    torch.cuda.synchronize()
    return losses.cpu().tolist(), dl.cpu(), amax.cpu(), bounds


def _check_abi(c, tag, losses, dl, amax, bounds, dpitch):
    want, g = _loss_ref(c, True)
    got_g = dl[:, :c].reshape(2, 19, 23, c).permute(0, 3, 1, 2)
    el, eg = _loss_err(losses, want), rel_err(got_g, g)
    print('CC2 C %2d %s (dpitch %d): losses %.3g (bound %.3g)  grad %.3g (bound %.3g)' % (c, tag, dpitch, el, LOSS_REL, eg, GRAD_REL))
    assert el < LOSS_REL and eg < GRAD_REL
    assert torch.equal(dl[:, c:r4(c)], torch.zeros(dl.shape[0], r4(c) - c))          # the channel padding up to round4(C) is zeroed
    assert torch.isnan(dl[:, r4(c):]).all()                                          # and nothing beyond it is touched
    for i, (lo, hi) in enumerate(zip(bounds[:-1], bounds[1:])):                      # the range the conv backward scales its operand with
        assert amax[i:i + 1].view(torch.float32).item() == dl[lo:hi, :c].abs().max().item()


@pytest.mark.parametrize('c', ALL_C)
def test_multiloss_abi_wide_pitch(dev, c):
    """pitch = dpitch = round4(C) + 4: a channel slice of a wider buffer.  Cstore = round4(C) at every C, C % 4 == 0 included."""
    p = r4(c) + 4
    _check_abi(c, 'wide pitch', *_abi_loss(dev, c, p, p, 1), p)


@pytest.mark.parametrize('c', ALL_C)
def test_multiloss_abi_two_shards(dev, c):
    """MultiLossFn's wire format with a group: each half batch's statistics, added, give the global losses, and each half's backward on the
    summed statistics and the global pixel count gives its pixels' share of the global gradient.  Pitch round4(C), the networks' own."""
    _check_abi(c, 'two shards', *_abi_loss(dev, c, r4(c), r4(c), 2), r4(c))


def test_multiloss_abi_refuses_class_counts_outside_2_16(dev):
    from pylc_amd import lib as L
    from pylc_amd.lib import lib, ptr, stream
    L.init()
    n = 1024
    x = torch.randn(n, 20, device=dev)
    t = torch.zeros(n, dtype=torch.int64, device=dev)
    cw = torch.ones(20, device=dev)
    stats = torch.full((3 + 3 * 17,), 5.0, device=dev)
    ws = torch.full((1024 * (3 + 3 * 17),), 5.0, device=dev)
    dl = torch.full((n, 20), 77.0, device=dev)
    amax = torch.full((1,), 1234, dtype=torch.int32, device=dev)
    for c in (1, 17):
        assert lib.pylc_multiloss_stats(ptr(x), 20, ptr(t), n, c, ptr(cw), ptr(stats), ptr(ws), stream()) == 1          # PYLC_ERR_ARG
        assert b'n_classes=%d' % c in lib.pylc_last_error(), lib.pylc_last_error()
        assert lib.pylc_multiloss_bwd(ptr(x), 20, ptr(t), n, c, ptr(cw), ptr(stats), float(n), *HALF, None, ptr(dl), 20, ptr(amax), stream()) == 1
        assert b'n_classes=%d' % c in lib.pylc_last_error(), lib.pylc_last_error()
    torch.cuda.synchronize()                                          # nothing faulted
    assert (stats == 5.0).all() and (ws == 5.0).all() and (dl == 77.0).all() and int(amax) == 1234      # and nothing was written


# ---- 3: the head as the networks compose it ----------------------------------------------------------------------------------------------
# fp32 torch against fp64 torch on the CPU, worst over C = 2..16 on exactly these inputs (max |diff| / max |ref|; the loss relative to max(1, |v|)):
#   logits 7.4e-7, loss 1.4e-7, dx 5.1e-7, dw 5.2e-7, db 3.4e-7.
# Bound = 4 x that (another summation order, and an f16x3 product that is fp32-equivalent, not fp32), never below the per-op bounds of
# test_conv_fwd_bwd (y 2e-6, dx 4e-6, dw 5e-6, db 2e-6) and, for the loss, of the loss head (LOSS_REL):
CHAIN_BOUNDS = {'logits': max(4 * 7.4e-7, 2e-6), 'loss': max(4 * 1.4e-7, LOSS_REL), 'dx': max(4 * 5.1e-7, 4e-6), 'dw': max(4 * 5.2e-7, 5e-6),
                'db': max(4 * 3.4e-7, 2e-6)}


def _chain_inputs(c):
    return (rnd(400 + c, 2, 256, 12, 10), rnd(401 + c, c, 256, 1, 1, scale=(2.0 / 256) ** 0.5), rnd(402 + c, c, scale=0.1),
            D.blob_masks(403 + c, 2, 48, 40, c, cell=4), torch.from_numpy(D.class_weights(c)))


@pytest.mark.parametrize('c', ALL_C)
def test_head_chain(dev, c):
    """conv 1x1 256 -> C with bias (pitch round4(C): three pad lanes at C = 2, none at 16) -> bilinear at that pitch -> weighted loss head, and
    back: the dlogits the loss head wrote are the dy of the separable bilinear backward, whose output feeds dgrad, wgrad and the bias column
    sum.  Reference: F.conv2d, F.interpolate(bilinear, align_corners=True), oracle.multiloss in fp64.

    fp32 torch differs from fp64 torch by at most 7.4e-7 (logits), 1.4e-7 (loss), 5.1e-7 (dx), 5.2e-7 (dw), 3.4e-7 (db) over the sweep; the
    bounds are 4 x that, floored by the per-op bounds: 3.0e-6, 2e-6, 4e-6, 5e-6, 2e-6 (CHAIN_BOUNDS)."""
    import oracle
    from pylc_amd import ops
    x, w, b, t, cw = _chain_inputs(c)
    xr, wr, br = (v.double().requires_grad_(True) for v in (x, w, b))
    zr = F.interpolate(F.conv2d(xr, wr, br), size=(48, 40), mode='bilinear', align_corners=True)
    tot = oracle.multiloss(zr, t, HALF, cw.double(), True)[0]
    tot.backward()

    xd, wd = to_dev_nhwc(x, dev).requires_grad_(True), to_dev_nhwc(w, dev).requires_grad_(True)
    bd = b.to(dev).requires_grad_(True)
    y = ops.conv2d(xd, wd, bd)
    z = ops.bilinear(y, 48, 40)
    assert tuple(z.shape) == tuple(zr.shape) and ops.pitch_of(y) == ops.pitch_of(z) == r4(c)
    losses = ops.multiloss(z, t.to(dev), cw.to(dev), *HALF)
    losses[0].backward()
    torch.cuda.synchronize()
    err = {'logits': rel_err(z, zr), 'loss': abs(losses[0].item() - tot.item()) / max(1.0, abs(tot.item())), 'dx': rel_err(xd.grad, xr.grad),
           'dw': rel_err(wd.grad, wr.grad), 'db': rel_err(bd.grad, br.grad)}
    print('CC3 C %2d: ' % c + '  '.join('%s %.3g (bound %.3g)' % (k, v, CHAIN_BOUNDS[k]) for k, v in err.items()))
    for k, v in err.items():
        assert v < CHAIN_BOUNDS[k], (k, v, CHAIN_BOUNDS[k])
    if r4(c) > c:                                # the pad lanes of both logit buffers are exact zeros
        assert float(_padded(y.detach())[:, c:].abs().max()) == 0.0 and float(_padded(z.detach())[:, c:].abs().max()) == 0.0


# ---- 4: pylc_stitch_argmax ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('c', ALL_C)
def test_stitch_every_class_count(dev, c):
    """rows 2, cols 3, tile 16 at stride 16 (no blend) and 8 (reconstruct()'s blend of softmaxes) against oracle.stitch_classes wherever the
    top-1 / top-2 gap of oracle.stitch_scores exceeds 1e-5 (test_stitch_matches_reference_fixture's rule).  768 and 1536 pixels: the seeds
    were chosen on the CPU so that the oracle alone leaves at least 99.9 % of them decided, i.e. all of them."""
    import oracle
    from pylc_amd import inference
    rows, cols, tile = 2, 3, 16
    tiles = (np.random.RandomState(502 + c).standard_normal((rows * cols, c, tile, tile)) * 3).astype(np.float32)
    for stride in (16, 8):
        scores = oracle.stitch_scores(tiles, rows, cols, tile, stride)
        top2 = np.sort(scores, axis=0)[-2:]
        decided = (top2[1] - top2[0]) > 1e-5
        assert decided.mean() >= 0.999
        mask = inference.stitch_logits(torch.from_numpy(tiles).to(dev), rows, cols, tile, stride).cpu().numpy()
        want = oracle.stitch_classes(tiles, rows, cols, tile, stride)
        assert mask.shape == want.shape == scores.shape[1:] and mask.dtype == np.uint8
        assert np.array_equal(mask[decided], want[decided])


@pytest.mark.parametrize('c', ALL_C)
def test_stitch_ties_take_the_first_maximum(dev, c):
    """stride == tile: no softmax on that path, the mask is the argmax of the raw logits; with logits from {-1, 0, 1} 35 % (C = 2), 43 % (3)
    and from C = 4 on most of the pixels tie"""
    from pylc_amd import inference
    rows, cols, tile = 2, 3, 16
    tiles = np.random.RandomState(520 + c).randint(-1, 2, (rows * cols, c, tile, tile)).astype(np.float32)
    full = tiles.reshape(rows, cols, c, tile, tile).transpose(2, 0, 3, 1, 4).reshape(c, rows * tile, cols * tile)
    srt = np.sort(full, 0)
    assert (srt[-1] == srt[-2]).mean() > (0.5 if c > 3 else 0.3)
    mask = inference.stitch_logits(torch.from_numpy(tiles).to(dev), rows, cols, tile, tile).cpu().numpy()
    assert np.array_equal(mask, full.argmax(0).astype(np.uint8))


# ---- 5: whole networks at other class counts --------------------------------------------------------------------------------------------------
NET_CASES = [(arch, c) for arch in ('deeplab', 'unet') for c in (2, 5, 16)]
NORM_TOL = 2e-3
ORACLE_NORM_TOL = NORM_TOL / 4      # what the fp32 oracle's own norm may differ from its fp64 evaluation for a case to be asked NORM_TOL of
NET_SALT = {('deeplab', 16): 21 + 16}     # every other case: 20 + C


@pytest.mark.parametrize('arch,c', NET_CASES)
def test_network_step_against_oracle(dev, arch, c):
    """DeepLabV3+/ResNet-101 (3-ch 64^2, bs 2) and U-Net (3-ch 256^2 -> 68^2, bs 1; the loss-head gradient is the last conv's dy, with the
    range the loss kernel emitted) at 2, 5 and 16 classes against oracle.step, built as test_truesize_oracle_gpu._case builds its cases.
    The oracle alone leaves 98.1 - 99.9 % of the pixels decided at these six cases, so _check_eval keeps its own min_decided (0.9).

    The pre-clip norm is a condition on the case before it is a check of the kernels.  At 64^2 and bs 2 the train-mode ResNet-101 puts 32
    values under each BatchNorm of layer4 / the ASPP and two under the image pool's, and the fp32 oracle's norm differs from the SAME step
    evaluated in fp64 by 4e-5 .. 3.5e-3 depending on the weights, and by up to 2.6e-3 between 1 and 8 host threads (measured over the salts
    36 .. 43 and four data seeds at C = 16).  With salt 20 + 16 the fp32 oracle is 1.6e-3 (1 thread) / 1.8e-3 (4 - 16 threads) off its fp64
    norm 17.00569, and the HIP step (16.98361) is 1.3e-3 off it on the other side: 3.1e-3 apart, both as near the truth as each other.
    A bound of 2e-3 against the fp32 oracle says something only where that oracle is itself well inside it, so the weights are those of the
    first salt 20 + C, 21 + C, .. at which the fp32 oracle's norm is within ORACLE_NORM_TOL = 5e-4 (a quarter of the bound) of the fp64
    one at 1, 4, 8 and 16 threads -- the oracle alone, on the CPU: 20 + C everywhere (DeepLab 2.8e-4 / 3.2e-4 at C = 2 / 5, U-Net 4.9e-5 /
    4.8e-5 / 4.9e-5) but DeepLab C = 16, where it is 21 + C (3.0e-4).  The test asserts that condition with the threads it runs on."""
    import oracle
    from oracle import step as ostep
    from pylc_amd import runtime
    from pylc_amd.model import Model, Meta
    from tests.test_truesize_oracle_gpu import _oracle_step, _check_eval, LOGIT_TOL, LOSS_TOL
    runtime.dropout_enabled = False
    backbone, b, hw = ('resnet', 2, 64) if arch == 'deeplab' else (None, 1, 256)
    cfg = ostep.StepConfig(arch, backbone, c, 3, dropout=False)
    x = D.tiles(600 + c, b, 3, hw, hw)
    y = D.blob_masks(601 + c, b, hw, hw, c, cell=8)
    w = ostep.calibrate_bn(oracle.formula_state(oracle.state_spec(arch, backbone, c, 3), salt=NET_SALT.get((arch, c), 20 + c)), cfg, x.clone())
    model = Model(Meta(arch=arch, backbone=backbone or 'resnet', ch=3, n_classes=c), dev).build()
    model.net.load_state_dict(w)
    tag = '%s C %2d' % (arch, c)

    e_eval = _check_eval(model, cfg, w, x, LOGIT_TOL, 'CC5 ' + tag)
    model.net.eval()
    mask = model.predict(x)
    logits = model.test(x)[0]
    assert mask.dtype == torch.uint8 and tuple(mask.shape) == (b,) + tuple(logits.shape[2:]) and logits.shape[1] == c
    assert torch.equal(mask.cpu().long(), logits.float().cpu().argmax(1))

    (ce, dsc, fl), ref_norm, sd = _oracle_step(cfg, w, x, y)
    w64 = {k: v.double() if v.is_floating_point() else v.clone() for k, v in w.items()}
    norm64 = ostep.train_step(w64, ostep.make_optimizer(w64, cfg), cfg, x.double(), y.clone())[5]
    e_oracle = abs(ref_norm - norm64) / norm64
    print('CC5 %s oracle alone: |g| fp32 %.5f vs fp64 %.5f: %.3g (bound %.3g)' % (tag, ref_norm, norm64, e_oracle, ORACLE_NORM_TOL))
    assert e_oracle < ORACLE_NORM_TOL, 'the fp32 oracle of this case is too far from its own fp64 evaluation for the norm to be compared'
    model.net.train()
    model.train(x, y)
    torch.cuda.synchronize()
    got = [float(model.crit.ce), float(model.crit.dsc), float(model.crit.fl)]
    gnorm, coef = model.optim.norm.cpu().tolist()
    e_loss = max(abs(a - r) for a, r in zip(got, (ce, dsc, fl)))
    e_norm = abs(gnorm - ref_norm) / ref_norm
    print('CC5 %s train step: HIP (%.6f %.6f %.6f) oracle (%.6f %.6f %.6f) max|diff| %.3g (bound %.3g); |g| %.5f vs %.5f: %.3g (bound %.3g); '
          'eval %.3g' % (tag, *got, ce, dsc, fl, e_loss, LOSS_TOL, gnorm, ref_norm, e_norm, NORM_TOL, e_eval))
    assert e_loss < LOSS_TOL
    assert e_norm < NORM_TOL
    head = 'decoder.last_conv.8.weight' if arch == 'deeplab' else [k for k, v in w.items() if k.endswith('weight') and v.dim() == 4][-1]
    params = dict(model.net.named_parameters())
    for k in (head, head[:-len('weight')] + 'bias'):
        ref_g = sd[k].grad.double()                               # clipped in place by the oracle's clip_grad_norm_
        got_g = (params[k].grad.double() * coef).cpu()
        assert got_g.shape == ref_g.shape and ref_g.shape[0] == c, k
        amax = ref_g.abs().max().item()
        err = (got_g - ref_g).abs().max().item()
        cos = float((got_g * ref_g).sum() / (got_g.norm() * ref_g.norm()))
        print('CC5 %s grad %-28s max|diff| %.3g = %.5f of |g|max %.3g (bound 0.02)   cos %.7f (bound 0.999)' % (tag, k, err, err / amax, amax, cos))
        assert err <= 2e-2 * amax and cos > 0.999, (k, err, amax, cos)
