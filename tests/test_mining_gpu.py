"""GPU suite of hard-pixel mining (csrc/mining.hip) against the yardstick tests/_mining.py: the loss map within the
derived bound of its fp64 statement with exact sentinels, the selection from planted maps bit for bit (info included), the fused path bit
for bit against the two calls it fuses and against itself, MultiLoss(hard_mining=) against the hand composition, and whole training steps.

Sizes come from the kernels' geometry (tests/_mining.py): 1, 3, 63, 65, 255, 257, one block's span -+ 1, one round of a grid + 5 and two
rounds + 1027 -- of the nll kernel's grid (262144 pixels a round) for the tests that start from logits, of the map passes' grid (1048576)
for the selection.  The fp64 statement of a (class count, size) pair is computed once and shared by every case that needs it.

Worst figures measured on the MI355X (the MG1 lines every run prints; DESIGN.md section 5.22 quotes them): |gpu - fp64| / bound of the loss
map 0.764 (C = 2), 0.673 (C = 9), 0.558 (C = 16), worst absolute error 3.0e-6; everything else is exact."""
import functools
import math

import numpy as np
import pytest
import torch

from tests import _data as D
from tests import _mining as M

pytestmark = pytest.mark.gpu

INF = float('inf')
LW = {'weighted': True, 'ce': 0.5, 'dice': 0.5, 'focal': 0.5}


# ---- shared statements -------------------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _statement(c, n):
    """(z, t, nll_ref, bound) of a (class count, size) pair, computed once and never written to"""
    z, t = M.logits_and_targets(c, n)
    ref, bound = M.nll_ref(z, t), M.nll_bound(z, t)
    for a in (z, t, ref, bound):
        a.setflags(write=False)
    return z, t, ref, bound


def _device_logits(dev, z, pitch):
    """[1, C, 1, N] logits with NHWC memory of the given pitch (what a net returns: pitch C or padded)"""
    n, c = z.shape
    buf = torch.full((1, 1, n, pitch), 1e30, device=dev)               # the pad lanes hold a number no result may depend on
    buf[..., :c] = torch.from_numpy(z.copy()).to(dev)                  # (the shared statement is read-only)
    return buf.permute(0, 3, 1, 2)[:, :c]


def _variants(dev, t, c, u8, n):
    """the four (ignore, weights) settings of one target type: (ignore_index, target on the device, host target, host weights or None)"""
    out = []
    for ign in (False, True):
        th = M.targets_with(t, c, ign, u8)
        td = torch.from_numpy(th).to(dev).reshape(1, 1, n)
        for wt in (False, True):
            out.append((255 if ign else None, td, th, M.weights_for(n) if wt else None))
    return out


def _bits(a):
    return a.contiguous().view(torch.int32)


def _same_bits(a, b):
    return a.shape == b.shape and torch.equal(_bits(a), _bits(b))


# ---- 1: the loss map --------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('u8', [True, False], ids=['uint8', 'int64'])
@pytest.mark.parametrize('extra', [0, 3])
@pytest.mark.parametrize('c', M.CLASSES)
def test_loss_map_against_the_fp64_statement(dev, c, extra, u8):
    from pylc_amd import mining
    worst, worst_abs = 0.0, 0.0
    for n in M.NLL_SIZES:
        z, t, ref, bound = _statement(c, n)
        zd = _device_logits(dev, z, c + extra)
        for ign, td, th, u in _variants(dev, t, c, u8, n):
            ud = None if u is None else torch.from_numpy(u).to(dev).reshape(1, 1, n)
            got = mining.pixel_nll(zd, td, ign, ud)
            assert got.dtype == torch.float32 and tuple(got.shape) == (1, 1, n)
            g = got.cpu().numpy().reshape(-1)
            want, part = M.expected_map(ref, th, c, ign, u)
            assert np.array_equal(g[~part], want[~part].astype(np.float32)), (n, ign, u is not None)         # the sentinels are exact
            assert not np.signbit(g[part & ~np.isnan(g)]).any()                  # no -0 (a NaN's sign bit says nothing)
            fin = part & np.isfinite(ref)
            assert np.array_equal(np.isnan(g[part]), np.isnan(ref[part])) and np.array_equal(g[part] == np.inf, ref[part] == np.inf)
            err = np.abs(g[fin].astype(np.float64) - ref[fin])
            if fin.any():
                worst, worst_abs = max(worst, float((err / bound[fin]).max())), max(worst_abs, float(err.max()))
            assert (err <= bound[fin]).all(), (n, ign, u is not None, float((err / bound[fin]).max()))
            if n >= M.BLOCK - 1:                                                 # the planted rows and both sentinels are there
                assert (g[fin] == 0).any() and (g[part] == np.inf).any() and np.isnan(g[part]).any() and (g == -2).any()
                assert (g == -1).any() == (ign is not None or u is not None)
    print('MG1 C=%d pitch=%d %s: worst |gpu - fp64| / bound = %.3f, worst absolute error %.3g' % (c, c + extra, 'uint8' if u8 else 'int64', worst,
                                                                                                worst_abs))


# ---- 2: the selection from planted maps ---------------------------------------------------------------------------------------------------------------
def _planted(kind, n):
    rs = np.random.RandomState(9000 + n % 9973)
    if kind == 'equal':
        return np.full(n, np.float32(math.log(9.0)), np.float32)
    if kind == 'tie':                                         # rank k of keep = 0.25 falls inside the group of 1.0
        return rs.choice(np.array([2.0, 1.0, 0.5], np.float32), n, p=[0.1, 0.5, 0.4])
    if kind == 'lowbit':                                      # the lowest mantissa bits alone differ
        return (np.uint32(0x3F800000) + rs.randint(0, 4, n).astype(np.uint32)).view(np.float32)
    if kind == 'topdigit':                                    # bits 30..20 alone differ
        return ((rs.randint(0, 2040, n).astype(np.uint32) << np.uint32(20)) | np.uint32(0x5A5A5)).view(np.float32)
    if kind == 'special':
        pool = np.array([0.0, -0.0, 1e-45, 1e-40, np.inf, np.nan, -1.0, -2.0, -0.5, 1.0, 3.0, 1.1754944e-38, 0.25, -np.inf], np.float32)
        return pool[rs.randint(0, pool.size, n)]
    if kind == 'none':                                        # no candidate at all
        return np.array([-1.0, -2.0, np.nan, -3.5], np.float32)[rs.randint(0, 4, n)]
    assert kind == 'random'
    return np.abs(rs.standard_normal(n)).astype(np.float32)


# (keep, min_kept, thresh): k = 1; k = n_valid; min_kept above n_valid; a cap below tau_k; a cap above it; a cap alone; the plain quarter
def _settings(n):
    return [(1e-12, 0, None), (1.0, 0, None), (0.25, n + 10, None), (0.25, 0, 0.5), (0.25, 0, 0.05), (None, 0, 0.5), (None, 7, 0.3),
            (0.25, 0, None)]


def _cap(thresh):
    return np.float32(np.inf) if thresh is None else -np.log(np.float32(thresh))


@pytest.mark.parametrize('kind', ['equal', 'tie', 'lowbit', 'topdigit', 'special', 'none', 'random'])
def test_selection_from_planted_maps_is_bit_exact(dev, kind):
    from pylc_amd import mining
    runs = 0
    for n in M.MAP_SIZES:
        v = _planted(kind, n)
        vd = torch.from_numpy(v).to(dev)
        u = M.weights_for(n, seed=3)
        ud = torch.from_numpy(u).to(dev)
        big = n > M.BLOCK + 1
        for si, (keep, min_kept, thresh) in enumerate(_settings(n)):
            if big and si not in (0, 1, 3, 7):                # the two multi-round sizes: rank 1, rank n_valid, a cap below, the quarter
                continue
            for wt in ((False, True) if not big else (si % 2 == 1,)):
                want, winfo = M.select_ref(v, 0.0 if keep is None else keep, min_kept, _cap(thresh), u if wt else None)
                got, info = mining.select(vd, keep, min_kept, thresh, ud if wt else None)
                assert info.dtype == torch.int64 and info.cpu().tolist() == winfo.tolist(), (n, si, wt, info.cpu().tolist(), winfo.tolist())
                assert np.array_equal(got.cpu().numpy().view(np.uint32), want.view(np.uint32)), (n, si, wt)
                runs += 1
                if kind == 'random' and n >= 257 and not wt:
                    tau_k = np.sort(v)[v.size - M.compute_k(v.size, 0.25, 0)]
                    assert _cap(0.5) < tau_k < _cap(0.05)                      # the two caps do lie on either side of tau_k
                if si == 1 and kind != 'none':                                 # keep = 1.0: the input weights, bit for bit, at candidates
                    cand = (v >= 0) & ((M.weight_class(u) == 0) if wt else True)
                    src = u if wt else np.ones(n, np.float32)
                    assert np.array_equal(got.cpu().numpy()[cand].view(np.uint32), src[cand].view(np.uint32)) and winfo[2] == cand.sum()
                if kind == 'tie' and si == 7 and n >= 257 and not wt:
                    assert winfo[2] > winfo[1] and M.bits_of(1.0) == winfo[3]   # the tie group straddles rank k and is kept whole
                if kind == 'none':
                    assert winfo.tolist() == [0, 0, 0, M.INF_BITS]
    assert runs >= 100


# ---- 3: the fused path -------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('u8', [True, False], ids=['uint8', 'int64'])
@pytest.mark.parametrize('extra', [0, 3])
@pytest.mark.parametrize('c', M.CLASSES)
def test_fused_path_equals_the_two_calls_bit_for_bit(dev, c, extra, u8):
    from pylc_amd import mining
    rules = [dict(keep=0.25), dict(thresh=0.7, min_kept=100), dict(keep=0.1, thresh=0.5)]
    for n in M.NLL_SIZES:
        z, t, _, _ = _statement(c, n)
        zd = _device_logits(dev, z, c + extra)
        for vi, (ign, td, th, u) in enumerate(_variants(dev, t, c, u8, n)):
            ud = None if u is None else torch.from_numpy(u).to(dev).reshape(1, 1, n)
            rule = rules[(vi + n) % 3]
            nll = mining.pixel_nll(zd, td, ign, ud)
            w2, i2 = mining.select(nll, pixel_weights=ud, **rule)
            w1, i1, nll1 = mining.hard_pixel_weights(zd, td, ignore_index=ign, pixel_weights=ud, return_nll=True, **rule)
            assert _same_bits(nll1, nll) and _same_bits(w1, w2) and torch.equal(i1, i2), (n, vi)
            w0, i0 = mining.hard_pixel_weights(zd, td, ignore_index=ign, pixel_weights=ud, **rule)       # the map in the workspace; a second run
            assert _same_bits(w0, w1) and torch.equal(i0, i1), (n, vi)
            # and against the yardstick on the device's own map
            want, winfo = M.select_ref(nll.cpu().numpy(), rule.get('keep', 0.0), rule.get('min_kept', 0), _cap(rule.get('thresh')), u)
            assert i1.cpu().tolist() == winfo.tolist() and np.array_equal(w1.cpu().numpy().view(np.uint32), want.view(np.uint32)), (n, vi)
            if n >= 257:
                assert winfo[0] > 0 and winfo[2] >= winfo[1] > 0


def test_fused_path_past_two_rounds_of_the_map_grid(dev):
    from pylc_amd import mining
    c, n = 2, M.MAP_SIZES[-1]
    z, t = M.logits_and_targets(c, n)
    zd = _device_logits(dev, z, c)
    td = torch.from_numpy(M.targets_with(t, c, True, True)).to(dev).reshape(1, 1, n)
    nll = mining.pixel_nll(zd, td, 255)
    w2, i2 = mining.select(nll, keep=0.25)
    w1, i1 = mining.hard_pixel_weights(zd, td, keep=0.25, ignore_index=255)
    assert _same_bits(w1, w2) and torch.equal(i1, i2)
    want, winfo = M.select_ref(nll.cpu().numpy(), 0.25, 0, INF)
    assert i1.cpu().tolist() == winfo.tolist() and np.array_equal(w1.cpu().numpy().view(np.uint32), want.view(np.uint32))


# ---- 4: the layers -----------------------------------------------------------------------------------------------------------------------------------
def _leaf(dev, z):
    return z.to(dev).contiguous(memory_format=torch.channels_last).requires_grad_(True)


def test_multiloss_with_hard_mining_is_the_hand_composition(dev):
    import pylc_amd  # noqa: F401
    from pylc_amd import mining
    from pylc_amd.loss import MultiLoss
    c, b, h, w = 9, 2, 33, 37
    rs = np.random.RandomState(77)
    z = torch.from_numpy((rs.standard_normal((b, c, h, w)) * 3).astype(np.float32))
    y = D.blob_masks(78, b, h, w, c, cell=5)
    y[:, :4, :9] = 255
    yd = y.to(torch.uint8).to(dev)
    conf = torch.from_numpy(rs.uniform(0.5, 2.0, (b, h, w)).astype(np.float32)).to(dev)
    lw = dict(LW, weights=D.class_weights(c))
    for spec, eps, u in (({'keep': 0.25}, 0.0, None), ({'thresh': 0.6, 'min_kept': 50}, 0.0, conf), ({'keep': 0.25}, 0.1, conf)):
        mined = MultiLoss(lw, {'n_classes': c}, ignore_index=255, label_smoothing=eps, hard_mining=spec).to(dev)
        plain = MultiLoss(lw, {'n_classes': c}, ignore_index=255, label_smoothing=eps).to(dev)
        z1, z2 = _leaf(dev, z), _leaf(dev, z)
        l1 = mined(z1, yd, u)
        l1.backward()
        m, info = mining.hard_pixel_weights(z2, yd, ignore_index=255, pixel_weights=u, **spec)
        assert not m.requires_grad and torch.equal(info, mined.mined)
        l2 = plain(z2, yd, m)
        l2.backward()
        assert _same_bits(l1.detach(), l2.detach()) and _same_bits(z1.grad, z2.grad), spec
        assert _same_bits(mined.ce, plain.ce) and _same_bits(mined.dsc, plain.dsc) and _same_bits(mined.fl, plain.fl)
        n_valid, k, kept, _ = info.cpu().tolist()
        assert 0 < k <= kept < n_valid and int((m > 0).sum()) == kept
        # the validation terms stay unmined
        assert _same_bits(mined.all_losses(z1.detach(), yd), plain.all_losses(z1.detach(), yd))
        op_w, op_info = torch.ops.pylc_hip.hard_pixel_weights(z2.detach(), yd, u, spec.get('keep'), spec.get('min_kept', 0), spec.get('thresh'), 255)
        assert _same_bits(op_w, m) and torch.equal(op_info, info)
    # keep = 1.0 and no threshold: the unmined loss, bit for bit -- with and without an ignore label
    for ign, tgt in ((255, yd), (None, D.blob_masks(79, b, h, w, c, cell=5).to(dev))):
        full = MultiLoss(lw, {'n_classes': c}, ignore_index=ign, hard_mining={'keep': 1.0}).to(dev)
        plain = MultiLoss(lw, {'n_classes': c}, ignore_index=ign).to(dev)
        z1, z2 = _leaf(dev, z), _leaf(dev, z)
        l1, l2 = full(z1, tgt), plain(z2, tgt)
        l1.backward()
        l2.backward()
        assert _same_bits(l1.detach(), l2.detach()) and _same_bits(z1.grad, z2.grad), ign
        assert full.mined[2] == full.mined[1] == full.mined[0] > 0
    with pytest.raises(ValueError, match='soft target'):
        full(z1, torch.full((b, c, h, w), 1.0 / c, device=dev))
    # a NaN row and a bad weight are not hidden by the mining: the loss goes NaN, the bad pixel is counted
    zn = z.clone()
    zn[0, :, 20, 20] = float('nan')
    crit = MultiLoss(lw, {'n_classes': c}, ignore_index=255, hard_mining={'keep': 0.25}).to(dev)
    assert torch.isnan(crit(_leaf(dev, zn), yd))
    ub = conf.clone()
    ub[1, 20, 20] = -1.0
    crit(_leaf(dev, z), yd, ub)
    assert int(crit.bad_targets.item()) == 1


# ---- 5: whole steps ----------------------------------------------------------------------------------------------------------------------------------
def _model(dev, arch, c, **meta):
    import oracle
    from pylc_amd import runtime
    from pylc_amd.model import Model, Meta
    runtime.dropout_enabled = False
    backbone = 'resnet' if arch == 'deeplab' else None
    model = Model(Meta(arch=arch, backbone=backbone or 'resnet', ch=3, n_classes=c, weighted=True, weights=D.class_weights(c).tolist(), **meta),
                  dev).build()
    model.net.load_state_dict(oracle.formula_state(oracle.state_spec(arch, backbone, c, 3), salt=5))
    return model


def _sampled(model):
    return [p.detach().reshape(-1)[::97].clone() for p in model.net.parameters()]


@pytest.mark.parametrize('arch', ['deeplab', 'unet'])
def test_network_step_with_hard_mining(dev, arch, capsys):
    c = 9
    b, hw = (2, 64) if arch == 'deeplab' else (1, 256)
    x = D.tiles(1080, b, 3, hw, hw)
    y = D.blob_masks(1081, b, hw, hw, c, cell=8)
    plain, full, quarter = _model(dev, arch, c), _model(dev, arch, c, hard_mining={'keep': 1.0}), _model(dev, arch, c, hard_mining={'keep': 0.25})
    # Model.eval stays unmined
    for m in (plain, full, quarter):
        m.eval(x, y)
    assert plain.loss.flush() == quarter.loss.flush() and quarter.crit.mined is None
    lp, lf, lq = plain.train(x, y), full.train(x, y), quarter.train(x, y)
    assert _same_bits(lp, lf)                                  # keep = 1.0: the plain step's loss and parameter bytes
    for p, q in zip(_sampled(plain), _sampled(full)):
        assert _same_bits(p, q)
    n_valid, k, kept, _ = quarter.crit.mined.cpu().tolist()
    assert bool(torch.isfinite(lq)) and kept >= k == math.ceil(0.25 * n_valid) and n_valid == quarter.crop_target(y).numel()
    assert any(not torch.equal(p, q) for p, q in zip(_sampled(plain), _sampled(quarter)))
    torch.cuda.synchronize()
    for m in (full, quarter):
        assert all(torch.isfinite(p).all() for p in m.net.parameters())
    assert 'hard mining: kept %d / %d pixels' % (kept, n_valid) in capsys.readouterr().out     # Model.log at the first step's report
