"""CPU suite (-m "not gpu") of the soft targets of the loss head: the fp64 statement tests/_soft_targets.soft_multiloss
that the GPU suite (tests/test_soft_targets_gpu.py) compares the kernels with, proven here against independent formulas -- F.cross_entropy
with probability targets, with label smoothing and with class weights, the statement of the pixel weights on one-hot rows, the closed-form
gradient written out in numpy; the new entry points' declarations and host-side argument checks; the operators' registrations;
Meta.label_smoothing and its way through a checkpoint; the Python layer's refusals that need no device."""
import os
import re

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from tests import _data as D
from tests._pixel_weights import weighted_multiloss
from tests._soft_targets import bad_rows, smoothed_rows, soft_multiloss, taking_part, teacher_rows
from tests.test_cpu_ignore_label import ignore_blobs

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

NEW_ENTRY_POINTS = ('pylc_multiloss_stats_soft', 'pylc_multiloss_bwd_soft', 'pylc_multiloss_stats_ls', 'pylc_multiloss_bwd_ls')
CLASSES = (9, 3, 11, 2, 16)
HALF = (0.5, 0.5, 0.5)


def _inputs(c, seed=0):
    """logits [2,C,13,11], a strictly positive unnormalised volume q, a uniform weight map u, class weights -- all float64"""
    rs = np.random.RandomState(900 + c + seed)
    z = torch.from_numpy(rs.standard_normal((2, c, 13, 11)) * 3)
    q = torch.from_numpy(rs.gamma(0.7, 1.0, (2, c, 13, 11)) + 1e-3)
    u = torch.from_numpy(rs.uniform(0.05, 3.0, (2, 13, 11)))
    cw = torch.from_numpy(D.class_weights(c)).double()
    return rs, z, q, u, cw


def _bchw(v):
    return v[None, :, None, None]


# ---- the statement against independent formulas ------------------------------------------------------------------------------------------------
def test_statement_ce_is_torch_cross_entropy_with_probability_targets():
    for c in CLASSES:
        _, z, q, _, _ = _inputs(c)
        qn = q / q.sum(1, keepdim=True)                      # normalised in fp64: then the mean over N is the division by sum q
        got = soft_multiloss(z, qn)[1]
        want = F.cross_entropy(z, qn)
        assert abs(got.item() - want.item()) < 1e-12, c


def test_statement_ce_is_torch_cross_entropy_with_label_smoothing():
    for c in CLASSES:
        t = D.blob_masks(910 + c, 2, 13, 11, c, cell=3)
        _, z, _, _, _ = _inputs(c)
        for eps in (0.05, 0.2, 0.0):
            e = float(np.float32(eps))
            got = soft_multiloss(z, smoothed_rows(t, c, eps, None))[1]
            want = F.cross_entropy(z, t, label_smoothing=e)
            assert abs(got.item() - want.item()) < 1e-12, (c, eps)
        # with an ignore label: the mean over the labelled pixels
        t_ign = t.clone()
        t_ign[ignore_blobs(911 + c, t.shape, 0.3, cell=3)] = 255
        got = soft_multiloss(z, smoothed_rows(t_ign, c, 0.2, 255))[1]
        want = F.cross_entropy(z, t_ign, label_smoothing=float(np.float32(0.2)), ignore_index=255)
        assert abs(got.item() - want.item()) < 1e-12, c


def test_statement_weighted_ce_numerator_is_torch_cross_entropy_sum():
    for c in CLASSES:
        _, z, q, _, cw = _inputs(c)
        ce = soft_multiloss(z, q, None, HALF, cw)[1]
        num = ce * (_bchw(cw) * q).sum()
        want = F.cross_entropy(z, q, weight=cw, reduction='sum')
        assert abs(num.item() - want.item()) < 1e-12 * abs(want.item()), c


def test_statement_on_one_hot_rows_is_the_weighted_statement():
    for c in CLASSES:
        _, z, _, u, cw = _inputs(c)
        t = D.blob_masks(920 + c, 2, 13, 11, c, cell=3)
        t[ignore_blobs(921 + c, t.shape, 0.3, cell=3)] = 255
        q = smoothed_rows(t, c, 0.0, 255)
        assert set(q.unique().tolist()) == {0.0, 1.0}
        for w in (None, cw):
            zr, zq = z.clone().requires_grad_(True), z.clone().requires_grad_(True)
            got = soft_multiloss(zr, q, u.float(), HALF, w)
            want = weighted_multiloss(zq, t, u.float(), 255, HALF, w)
            assert max(abs(a.item() - b.item()) for a, b in zip(got, want)) < 1e-12
            got[0].backward()
            want[0].backward()
            assert float((zr.grad - zq.grad).abs().max()) < 1e-12


def closed_form_gradient(z, q, u, weights, cw):
    """d total / d z of DESIGN.md section 5.21 in numpy float64 from [N,C] rows of pixels that all take part:
      u_n [ ce_norm (W_n p_c - w_c q_c) + w_d p_c (g_c - sum_k g_k p_k) + w_f inv_n p_c (q_c f'(x_c) - sum_k q_k f'(x_k) p_k) ]"""
    w_ce, w_d, w_f = weights
    n, c = z.shape
    e = np.exp(z - z.max(1, keepdims=True))
    p = e / e.sum(1, keepdims=True)
    un = u[:, None]
    ce_norm = w_ce / (un * cw[None, :] * q).sum()
    inv_n = 1.0 / (un * q).sum()
    inter = (un * p * q).sum(0)
    card = (un * p).sum(0) + (un * q).sum(0)
    a = -2.0 / (card + 1.0) / c
    b = (2.0 * inter + 1.0) / (card + 1.0) ** 2 / c
    g = q * a[None, :] + b[None, :]
    x = p + 1e-8
    fprime = 0.5 * (1 - x) * np.log(x) - 0.25 * (1 - x) ** 2 / x
    big_w = (cw[None, :] * q).sum(1, keepdims=True)
    d = (ce_norm * (big_w * p - cw[None, :] * q) + w_d * p * (g - (g * p).sum(1, keepdims=True))
         + w_f * inv_n * p * (q * fprime - (q * fprime * p).sum(1, keepdims=True)))
    return un * d


def test_statement_gradient_is_the_closed_form():
    for c in CLASSES:
        _, z, q, u, cw = _inputs(c)
        for w in (None, cw):
            for weights in (HALF, (1.0, 0.0, 0.0), (0.0, 1.0, 0.0), (0.0, 0.0, 1.0), (0.3, 0.9, 0.2)):
                zr = z.clone().requires_grad_(True)
                soft_multiloss(zr, q, u, weights, w)[0].backward()
                rows = [v.permute(0, 2, 3, 1).reshape(-1, c).numpy() for v in (z, q)]
                want = closed_form_gradient(rows[0], rows[1], u.reshape(-1).numpy(), weights, np.ones(c) if w is None else w.numpy())
                got = zr.grad.permute(0, 2, 3, 1).reshape(-1, c).numpy()
                assert np.abs(got - want).max() < 1e-10, (c, weights)
        assert q.grad is None and not q.requires_grad


def test_statement_drops_zero_rows_bad_rows_and_zero_weights():
    c = 4
    _, z, q, u, cw = _inputs(c)
    q, u = q.clone(), u.clone()
    zero = ignore_blobs(930, (2, 13, 11), 0.3, cell=3)
    q.permute(0, 2, 3, 1)[zero] = 0.0
    u[0, :3] = 0.0
    q[1, 2, 5, 5], q[1, 0, 6, 6], q[1, 1, 7, 7] = -1e-3, float('nan'), float('inf')
    part = taking_part(q, u)
    assert int(bad_rows(q).sum()) == 3 and 0 < int(part.sum()) < part.numel() - int(zero.sum())
    # the same as a problem in which those pixels have u = 0 and harmless rows
    gone = ~part.reshape(2, 13, 11)
    q_clean = torch.where(gone[:, None], torch.ones_like(q), q)
    u_clean = torch.where(gone, torch.zeros_like(u), u)
    zr, zq = z.clone().requires_grad_(True), z.clone().requires_grad_(True)
    got, want = soft_multiloss(zr, q, u, HALF, cw), soft_multiloss(zq, q_clean, u_clean, HALF, cw)
    assert [v.item() for v in got] == [v.item() for v in want] and all(np.isfinite(v.item()) for v in got)
    got[0].backward()
    want[0].backward()
    assert torch.equal(zr.grad, zq.grad) and float(zr.grad.permute(0, 2, 3, 1)[gone].abs().max()) == 0.0
    # nothing takes part: zeros
    zr = z.clone().requires_grad_(True)
    out = soft_multiloss(zr, torch.zeros_like(q), u)
    out[0].backward()
    assert all(v.item() == 0.0 for v in out) and float(zr.grad.abs().max()) == 0.0


def test_teacher_rows_and_smoothed_rows():
    rs = np.random.RandomState(940)
    t = torch.from_numpy(rs.standard_normal((2, 5, 4, 3)).astype(np.float32) * 4)
    for temp in (0.5, 1.0, 1.7):
        q = teacher_rows(t, temp)
        assert float((q.sum(1) - 1).abs().max()) < 1e-12 and taking_part(q).all()
        assert float((q - torch.softmax(t.double() / temp, 1)).abs().max()) < 1e-6          # (inv_T is rounded to float32)
    t[0, 1, 2, 1], t[1, 4, 0, 0] = float('inf'), float('nan')
    assert int(bad_rows(teacher_rows(t, 1.0)).sum()) == 2
    lab = torch.tensor([[[0, 4, 255, 7, -1]]])
    q = smoothed_rows(lab, 5, 0.2, 255)
    e = float(np.float32(0.2))
    assert q.shape == (1, 5, 1, 5) and q[0, :, 0, 2:].abs().max() == 0
    assert q[0, 0, 0, 0] == (1 - e) + e / 5 and q[0, 1, 0, 0] == e / 5 and abs(q[0, :, 0, 1].sum().item() - 1) < 1e-15


# ---- the C ABI: declared, bound, argument errors before any launch ---------------------------------------------------------------------------------
def test_new_entry_points_are_declared_and_bound_and_the_abi_version_stays():
    from pylc_amd import lib as L
    hdr = re.sub(r'/\*.*?\*/', '', open(os.path.join(ROOT, 'include', 'pylc_hip.h')).read(), flags=re.S)
    for name in NEW_ENTRY_POINTS:
        m = re.search(r'\b%s\s*\(([^;]*)\)\s*;' % name, hdr)
        assert m, name
        assert name in L.SIGNATURES and hasattr(L.lib, name), name
        assert len(m.group(1).split(',')) == len(L.SIGNATURES[name][1]), name          # as many parameters as the binding passes
    assert L.ABI_VERSION == 15 and L.lib.pylc_abi_version() == 15


P = 64                                              # a non-NULL, aligned "pointer": every call below returns before anything is launched


def soft_refusals():
    """(keyword overrides, text of the error) of pylc_multiloss_stats_soft and _bwd_soft"""
    inf, nan = float('inf'), float('nan')
    return (({'soft': None}, b'soft is NULL'), ({'logits': None}, b'NULL'), ({'c': 1}, b'n_classes=1'), ({'c': 17}, b'n_classes=17'),
            ({'kind': 2}, b'kind=2'), ({'kind': -1}, b'kind=-1'), ({'inv_t': 0.0}, b'inv_T'), ({'inv_t': -1.0}, b'inv_T'),
            ({'inv_t': inf}, b'inv_T'), ({'inv_t': nan}, b'inv_T'), ({'n': 0}, b'N=0'), ({'n': -100}, b'N=-100'), ({'n': 101}, b'N=101'),
            ({'h': 0}, b'H=0'), ({'w': -2}, b'W=-2'), ({'h': 7}, b'multiple of H*W=70'), ({'sb': -1}, b'stride'), ({'sc': -100}, b'stride'),
            ({'sh': -10}, b'stride'), ({'sw': -1}, b'stride'), ({'pitch': 8}, b'pitch=8'), ({'soft': 66}, b'aligned'), ({'pw': 65}, b'aligned'))


def ls_refusals():
    """(keyword overrides, text of the error) of pylc_multiloss_stats_ls and _bwd_ls: those of _w, and the smoothing"""
    return (({'eps': 1.0}, b'smoothing=1'), ({'eps': -0.1}, b'smoothing=-0.1'), ({'eps': float('nan')}, b'smoothing=nan'),
            ({'eps': float('inf')}, b'smoothing=inf'), ({'tbytes': 2}, b'target_bytes=2'), ({'tbytes': 4}, b'target_bytes=4'),
            ({'target': None}, b'target is NULL'), ({'pitch': 8}, b'pitch=8'), ({'n': 0}, b'N=0'), ({'n': -5}, b'N=-5'), ({'c': 1}, b'n_classes=1'),
            ({'c': 17}, b'n_classes=17'), ({'logits': None}, b'NULL'), ({'target': 60, 'tbytes': 8}, b'aligned'), ({'pw': 66}, b'aligned'))


def test_soft_entry_points_refuse_bad_arguments_on_the_host():
    from pylc_amd import lib as L
    lib = L.lib

    def stats(logits=P, pitch=12, n=100, h=10, w=10, c=9, soft=P, sb=900, sc=100, sh=10, sw=1, kind=0, inv_t=1.0, cw=None, pw=None, st=P, ws=P,
              bad=None):
        return lib.pylc_multiloss_stats_soft(logits, pitch, n, h, w, c, soft, sb, sc, sh, sw, kind, inv_t, cw, pw, st, ws, bad, None)

    def bwd(logits=P, pitch=12, n=100, h=10, w=10, c=9, soft=P, sb=900, sc=100, sh=10, sw=1, kind=0, inv_t=1.0, cw=None, pw=None, st=P, dl=P,
            dpitch=12, amax=None):
        return lib.pylc_multiloss_bwd_soft(logits, pitch, n, h, w, c, soft, sb, sc, sh, sw, kind, inv_t, cw, pw, st, 0.5, 0.5, 0.5, None, dl, dpitch,
                                           amax, None)

    for call, name in ((stats, b'multiloss_stats_soft'), (bwd, b'multiloss_bwd_soft')):
        for kw, text in soft_refusals():
            assert call(**kw) == 1, (name, kw)                                     # PYLC_ERR_ARG
            msg = lib.pylc_last_error()
            assert name in msg and text in msg, (kw, msg)
    assert bwd(dpitch=8) == 1 and b'dpitch=8' in lib.pylc_last_error()
    assert stats(st=None) == 1 and stats(ws=None) == 1 and bwd(st=None) == 1 and bwd(dl=None) == 1
    assert stats(bad=68) == 1 and b'aligned' in lib.pylc_last_error()


def test_smoothing_entry_points_refuse_bad_arguments_on_the_host():
    from pylc_amd import lib as L
    lib = L.lib

    def stats(logits=P, pitch=12, target=P, tbytes=1, n=100, c=9, ign=255, cw=None, pw=None, eps=0.1, st=P, ws=P, bad=None):
        return lib.pylc_multiloss_stats_ls(logits, pitch, target, tbytes, n, c, ign, cw, pw, eps, st, ws, bad, None)

    def bwd(logits=P, pitch=12, target=P, tbytes=1, n=100, c=9, ign=255, cw=None, pw=None, eps=0.1, st=P, dl=P, dpitch=12, amax=None):
        return lib.pylc_multiloss_bwd_ls(logits, pitch, target, tbytes, n, c, ign, cw, pw, eps, st, 0.5, 0.5, 0.5, None, dl, dpitch, amax, None)

    for call, name in ((stats, b'multiloss_stats_ls'), (bwd, b'multiloss_bwd_ls')):
        for kw, text in ls_refusals():
            assert call(**kw) == 1, (name, kw)
            msg = lib.pylc_last_error()
            assert name in msg and text in msg, (kw, msg)
    assert bwd(dpitch=8) == 1 and b'dpitch=8' in lib.pylc_last_error()
    assert stats(st=None) == 1 and stats(ws=None) == 1 and bwd(st=None) == 1 and bwd(dl=None) == 1
    assert stats(bad=68) == 1 and b'aligned' in lib.pylc_last_error()


# ---- operators -------------------------------------------------------------------------------------------------------------------------------------
def test_soft_operators_are_registered_and_trace_under_fake_tensors():
    import pylc_amd  # noqa: F401
    from pylc_amd import torch_ops
    from torch._subclasses.fake_tensor import FakeTensorMode
    assert torch_ops.REGISTERED[-2:] == ('multiloss_weighted', 'multiloss_weighted_backward')          # the pinned tail stays
    assert torch_ops.REGISTERED[-4:-2] == ('multiloss_soft', 'multiloss_soft_backward') and len(set(torch_ops.REGISTERED)) == len(torch_ops.REGISTERED)
    for name in torch_ops.REGISTERED[-4:-2]:
        assert hasattr(torch.ops.pylc_hip, name), name
    with FakeTensorMode():
        z, q, u = torch.empty(2, 9, 8, 8), torch.empty(2, 9, 8, 8), torch.empty(2, 8, 8)
        for kind, pw in (('probs', None), ('logits', u)):
            losses, stats, bad = torch.ops.pylc_hip.multiloss_soft(z, q, kind, 1.5, pw, None, 0.5, 0.5, 0.5)
            assert tuple(losses.shape) == (4,) and tuple(stats.shape) == (30,) and tuple(bad.shape) == (1,) and bad.dtype == torch.int64
            dl = torch.ops.pylc_hip.multiloss_soft_backward(losses, z, q, kind, 1.5, pw, stats, torch.empty(9), 0.5, 0.5, 0.5)
            assert tuple(dl.shape) == (2, 9, 8, 8)


# ---- Meta and checkpoints --------------------------------------------------------------------------------------------------------------------
def test_meta_label_smoothing_round_trips_through_update_and_a_checkpoint(tmp_path):
    from pylc_amd.model import Model, Meta
    from pylc_amd import checkpoint as ck
    assert Meta().label_smoothing == 0.0 and Meta(label_smoothing=0.1).label_smoothing == 0.1
    assert Meta().update({'label_smoothing': 0.1}).label_smoothing == 0.1 and Meta(label_smoothing=0.1).update(Meta()).label_smoothing == 0.0
    m = Model(Meta(arch='deeplab', backbone='xception', n_classes=4, ch=1, label_smoothing=0.1), 'cpu').build()
    assert m.crit.label_smoothing == 0.1
    assert Model(Meta(arch='deeplab', backbone='xception', n_classes=4, ch=1), 'cpu').build().crit.label_smoothing == 0.0
    path = str(tmp_path / 'checkpoint.pth')
    ck.save(m, path)
    raw = ck.load_reference_file(path)
    assert raw['meta'].label_smoothing == 0.1 and ck.meta_from_reference(raw['meta']).label_smoothing == 0.1
    del raw['meta'].__dict__['label_smoothing']                    # a file written before the field existed
    old = ck.meta_from_reference(raw['meta'])
    assert old.label_smoothing == 0.0 and old.n_classes == 4
    ref = ck.load_reference_file(os.path.join(os.path.dirname(__file__), 'golden', 'ref_checkpoint_tiny.pth'))
    assert ck.meta_from_reference(ref['meta']).label_smoothing == 0.0


# ---- the Python layer's refusals that need no device --------------------------------------------------------------------------------------------
def test_python_argument_rules_without_gpu():
    from pylc_amd import lib as L, ops
    from pylc_amd.loss import MultiLoss
    from pylc_amd.model import Model, Meta
    lw = {'weighted': False, 'weights': None, 'ce': 0.5, 'dice': 0.5, 'focal': 0.5}
    for eps in (1.0, -0.1, 1.5, float('nan')):
        with pytest.raises(ValueError, match='label_smoothing'):
            MultiLoss(lw, {'n_classes': 4}, label_smoothing=eps)
        with pytest.raises(ValueError, match='label_smoothing'):
            Model(Meta(arch='deeplab', backbone='xception', n_classes=4, ch=1, label_smoothing=eps), 'cpu').build()
    assert MultiLoss(lw, {'n_classes': 4}).label_smoothing == 0.0 and MultiLoss(lw, {'n_classes': 4}, 255, 0.1).label_smoothing == 0.1
    for temp in (0.0, -1.0, float('inf'), float('nan'), 'meta', None, 1e-39):
        with pytest.raises(L.PylcError, match='temperature'):
            ops.soft_inv_temperature(temp)
    assert ops.soft_inv_temperature(2.0) == 0.5 and ops.SOFT_KINDS == {'probs': 0, 'logits': 1}
    crit = MultiLoss(lw, {'n_classes': 4})
    pred = torch.zeros(2, 4, 8, 8)
    for soft in (torch.zeros(2, 4, 8, 9), torch.zeros(2, 5, 8, 8), torch.zeros(2, 4, 8, 8, dtype=torch.float64), torch.zeros(1, 4, 8, 8)):
        with pytest.raises(ValueError, match='soft target'):
            crit(pred, soft)
        with pytest.raises(ValueError, match='soft target'):
            crit.distill(pred, soft)
    with pytest.raises(ValueError, match='Invalid input shape'):
        crit(torch.zeros(2, 3, 8, 8), torch.zeros(2, 3, 8, 8))
    with pytest.raises(TypeError, match='torch.Tensor'):
        crit.distill(None, torch.zeros(2, 4, 8, 8))

    def build(**kw):
        return Model(Meta(arch='deeplab', backbone='xception', n_classes=4, ch=1, **kw), 'cpu').build()
    x, q = torch.zeros(2, 1, 8, 8), torch.full((2, 4, 8, 8), 0.25)
    m = build()
    with pytest.raises(ValueError, match="'probs' or 'logits'"):
        m.train(x, q, soft='labels')
    with pytest.raises(ValueError, match='meta.temperature is unset'):
        m.train(x, q, soft='logits', temperature='meta')
    for temp in (0.0, -2.0, float('inf'), 'T'):
        with pytest.raises(ValueError, match='temperature'):
            m.train(x, q, soft='logits', temperature=temp)
    with pytest.raises(ValueError, match=r'float \[B,4,H,W\]'):
        m.train(x, torch.zeros(2, 5, 8, 8))
    with pytest.raises(ValueError, match='border_weight'):
        build(border_weight={'w0': 10.0, 'sigma': 2.0, 'radius': 3}).train(x, q)
    with pytest.raises(ValueError, match='B,H,W'):
        m._soft_weights(q, torch.ones(8, 8))
    with pytest.raises(ValueError, match='do not match'):
        m._soft_weights(q, torch.ones(2, 8, 9))
    # the crop of a soft target is a view of the caller's tensor: never a copy
    mu = Model(Meta(arch='unet', n_classes=4, ch=1, pad_size=2), 'cpu')
    big = torch.rand(2, 4, 12, 12)
    got = mu._soft_target(big)
    assert tuple(got.shape) == (2, 4, 8, 8) and got.data_ptr() == big[:, :, 2:, 2:].data_ptr() and got.stride() == big.stride()
    assert m._soft_target(q).data_ptr() == q.data_ptr()
