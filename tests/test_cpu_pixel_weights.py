"""CPU suite (-m "not gpu") of the per-pixel loss weights and the border-weight map: the fp64 statement
tests/_pixel_weights.weighted_multiloss that the GPU suite (tests/test_pixel_weights_gpu.py) compares the kernels with, proven here against
the statement of the ignore label and against torch; boundary.border_profile; the new entry points' declarations and host-side argument
checks; the operators' registrations; Meta.border_weight and its way through a checkpoint; the Python layer's refusals."""
import os
import re

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from tests import _data as D
from tests._pixel_weights import taking_part, weighted_multiloss
from tests.test_cpu_ignore_label import ignore_blobs, masked_multiloss

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

NEW_ENTRY_POINTS = ('pylc_multiloss_stats_w', 'pylc_multiloss_bwd_w', 'pylc_boundary_weights', 'pylc_weights_from_d2')
CASES = ((9, 255), (3, -100), (11, 0), (2, 255), (16, None))


def _inputs(c, ignore, seed=0):
    rs = np.random.RandomState(30 + c + seed)
    z = torch.from_numpy(rs.standard_normal((2, c, 13, 11)) * 3)
    t = D.blob_masks(60 + c, 2, 13, 11, c, cell=3)
    if ignore is not None:
        t[ignore_blobs(61 + c, t.shape, 0.3, cell=3)] = ignore
    cw = torch.from_numpy(D.class_weights(c)).double()
    return rs, z, t, cw


# ---- the statement ---------------------------------------------------------------------------------------------------------------------------
def test_statement_with_unit_weights_is_the_masked_statement():
    for c, ignore in CASES:
        _, z, t, cw = _inputs(c, ignore)
        for w in (None, cw):
            zr, zq = z.clone().requires_grad_(True), z.clone().requires_grad_(True)
            got = weighted_multiloss(zr, t, torch.ones(t.shape, dtype=torch.float32), ignore, (0.5, 0.5, 0.5), w)
            want = masked_multiloss(zq, t, ignore, (0.5, 0.5, 0.5), w)
            assert max(abs(a.item() - b.item()) for a, b in zip(got, want)) < 1e-12
            got[0].backward()
            want[0].backward()
            assert float((zr.grad - zq.grad).abs().max()) < 1e-12


def test_statement_with_zero_one_weights_is_the_masked_statement_with_those_pixels_ignored():
    for c, ignore in CASES:
        _, z, t, cw = _inputs(c, ignore)
        off = ignore_blobs(62 + c, t.shape, 0.4, cell=3)
        u = (~off).float()
        marker = -1 if ignore is None else ignore            # (-1 is no class: masked_multiloss removes it as out of range)
        t_off = torch.where(off, torch.full_like(t, marker), t)
        assert 0 < int(taking_part(t, u, c, ignore).sum()) < int(taking_part(t, torch.ones_like(u), c, ignore).sum())
        for w in (None, cw):
            got = weighted_multiloss(z, t, u, ignore, (0.5, 0.5, 0.5), w)
            want = masked_multiloss(z, t_off, ignore, (0.5, 0.5, 0.5), w)
            assert max(abs(a.item() - b.item()) for a, b in zip(got, want)) < 1e-12


def test_statement_ce_is_the_weighted_mean_of_torch_cross_entropy():
    for c, ignore in CASES:
        rs, z, t, cw = _inputs(c, ignore)
        u = torch.from_numpy(rs.uniform(0.05, 3.0, t.shape).astype(np.float32))
        for w in (None, cw):
            keep = taking_part(t, u, c, ignore)
            safe = torch.where(keep, t, torch.zeros_like(t))
            per = F.cross_entropy(z, safe, weight=w, reduction='none')          # w_t * nll per pixel
            wt = torch.ones_like(per) if w is None else w[safe]
            ud = torch.where(keep, u.double(), torch.zeros_like(per))
            want = (ud * per).sum() / (ud * wt).sum()
            got = weighted_multiloss(z, t, u, ignore, (0.5, 0.5, 0.5), w)[1]
            assert abs(got.item() - want.item()) < 1e-12


def test_statement_removes_bad_weights_and_gives_zero_without_a_pixel():
    c, ignore = 4, 255
    _, z, t, _ = _inputs(c, ignore)
    u = torch.ones(t.shape, dtype=torch.float32)
    u[0, 0, 0], u[0, 1, 1], u[1, 2, 2], u[1, 3, 3] = float('nan'), float('inf'), -1.0, 0.0
    t = t.clone()
    t[0, 0, 0] = t[0, 1, 1] = t[1, 2, 2] = t[1, 3, 3] = 1
    want = weighted_multiloss(z, torch.where(torch.isfinite(u) & (u > 0), t, torch.full_like(t, 255)), torch.ones_like(u), ignore)
    got = weighted_multiloss(z, t, u, ignore)
    assert [v.item() for v in got] == [v.item() for v in want] and all(np.isfinite(v.item()) for v in got)
    zr = z.clone().requires_grad_(True)
    out = weighted_multiloss(zr, t, torch.zeros_like(u), ignore)
    out[0].backward()
    assert all(v.item() == 0.0 for v in out) and float(zr.grad.abs().max()) == 0.0


# ---- border_profile ----------------------------------------------------------------------------------------------------------------------------
def test_border_profile_values_shape_and_refusals():
    from pylc_amd import boundary
    for radius, w0, sigma in ((1, 10.0, 5.0), (3, 10.0, 2.0), (10, 2.5, 0.7), (254, 10.0, 5.0), (7, 1e-3, 100.0)):
        tab = boundary.border_profile(radius, w0, sigma)
        assert tab.dtype == np.float32 and tab.shape == (radius * radius + 2,)
        d2 = np.arange(radius * radius + 1, dtype=np.float64)
        exact = 1.0 + w0 * np.exp(-d2 / (2.0 * sigma * sigma))
        # one float32 rounding of the float64 value: half a unit in the last place of the result (exp in float64 is far inside that)
        assert (np.abs(tab[:-1].astype(np.float64) - exact) <= 0.5 * np.spacing(tab[:-1]).astype(np.float64) * (1 + 1e-6)).all()
        assert tab[-1] == 1.0 and tab[0] == np.float32(1.0 + w0)
        assert (np.diff(tab) <= 0).all() and (tab >= 1.0).all()
    assert np.array_equal(boundary.border_profile(5, w0=0.0), np.ones(27, np.float32))
    assert np.array_equal(boundary.border_profile(3), boundary.border_profile(3, 10.0, 5.0))
    for kw in ({'w0': -1.0}, {'w0': float('nan')}, {'w0': float('inf')}, {'sigma': 0.0}, {'sigma': -2.0}, {'sigma': float('nan')},
               {'sigma': float('inf')}):
        with pytest.raises(ValueError, match='w0|sigma'):
            boundary.border_profile(3, **kw)
    for radius in (0, 255, -3):
        with pytest.raises(ValueError, match='radius'):
            boundary.border_profile(radius)
    for radius in (2.0, True, None):
        with pytest.raises(TypeError, match='radius'):
            boundary.border_profile(radius)


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


def loss_w_refusals():
    """(keyword overrides, text of the error) of pylc_multiloss_stats_w and _bwd_w: those of _ex, and the weights' alignment"""
    return (({'tbytes': 2}, b'target_bytes=2'), ({'tbytes': 0}, b'target_bytes=0'), ({'tbytes': 4}, b'target_bytes=4'),
            ({'target': None}, b'target is NULL'), ({'pitch': 8}, b'pitch=8'), ({'n': 0}, b'N=0'), ({'n': -5}, b'N=-5'),
            ({'c': 1}, b'n_classes=1'), ({'c': 17}, b'n_classes=17'), ({'logits': None}, b'NULL'), ({'target': 60, 'tbytes': 8}, b'aligned'),
            ({'pw': 66}, b'aligned'), ({'pw': 65}, b'aligned'))


def test_weighted_loss_entry_points_refuse_bad_arguments_on_the_host():
    from pylc_amd import lib as L
    lib = L.lib

    def stats(logits=P, pitch=12, target=P, tbytes=1, n=100, c=9, ign=255, cw=None, pw=P, st=P, ws=P, bad=None):
        return lib.pylc_multiloss_stats_w(logits, pitch, target, tbytes, n, c, ign, cw, pw, st, ws, bad, None)

    def bwd(logits=P, pitch=12, target=P, tbytes=1, n=100, c=9, ign=255, cw=None, pw=P, st=P, dl=P, dpitch=12, amax=None):
        return lib.pylc_multiloss_bwd_w(logits, pitch, target, tbytes, n, c, ign, cw, pw, st, 0.5, 0.5, 0.5, None, dl, dpitch, amax, None)

    for call, name in ((stats, b'multiloss_stats_w'), (bwd, b'multiloss_bwd_w')):
        for kw, text in loss_w_refusals():
            assert call(**kw) == 1, (name, kw)                                     # PYLC_ERR_ARG
            msg = lib.pylc_last_error()
            assert name in msg and text in msg, (kw, msg)
    assert bwd(dpitch=8) == 1 and b'dpitch=8' in lib.pylc_last_error()
    assert stats(st=None) == 1 and stats(ws=None) == 1 and bwd(st=None) == 1 and bwd(dl=None) == 1
    assert stats(bad=68) == 1 and b'aligned' in lib.pylc_last_error()


def boundary_weight_refusals():
    """keyword overrides that pylc_boundary_weights refuses: those of pylc_boundary_distance, and the table"""
    return ({'mask': None}, {'table': None}, {'out': None}, {'ws': None}, {'b': 0}, {'h': 0}, {'w': -1}, {'b': 1 << 11, 'h': 1 << 10, 'w': 1 << 10},
            {'radius': 0}, {'radius': 255}, {'radius': -1}, {'ign': 256}, {'ign': -2}, {'table': 66}, {'out': 65}, {'ws': 62})


def from_d2_refusals():
    return ({'d2': None}, {'table': None}, {'out': None}, {'n': 0}, {'n': -1}, {'n': 1 << 31}, {'radius': 0}, {'radius': 255}, {'d2': 66},
            {'table': 65}, {'out': 62})


def test_border_weight_entry_points_refuse_bad_arguments_on_the_host():
    from pylc_amd import lib as L
    lib = L.lib

    def bw(mask=P, b=1, h=8, w=8, radius=3, ign=-1, table=P, out=P, ws=P):
        return lib.pylc_boundary_weights(mask, b, h, w, radius, ign, table, out, ws, None)

    def fd(d2=P, n=64, radius=3, table=P, out=P):
        return lib.pylc_weights_from_d2(d2, n, radius, table, out, None)

    for kw in boundary_weight_refusals():
        assert bw(**kw) == 1 and b'boundary_weights' in lib.pylc_last_error(), kw
    for kw in from_d2_refusals():
        assert fd(**kw) == 1 and b'weights_from_d2' in lib.pylc_last_error(), kw


# ---- operators -------------------------------------------------------------------------------------------------------------------------------------
def test_weighted_operators_are_registered_and_trace_under_fake_tensors():
    import pylc_amd  # noqa: F401
    from pylc_amd import torch_ops
    from torch._subclasses.fake_tensor import FakeTensorMode
    assert torch_ops.REGISTERED[-2:] == ('multiloss_weighted', 'multiloss_weighted_backward')
    for name in torch_ops.REGISTERED[-2:]:
        assert hasattr(torch.ops.pylc_hip, name), name
    with FakeTensorMode():
        z, t, u = torch.empty(2, 9, 8, 8), torch.empty(2, 8, 8, dtype=torch.uint8), torch.empty(2, 8, 8)
        for ignore in (255, None):
            losses, stats, bad = torch.ops.pylc_hip.multiloss_weighted(z, t, u, None, 0.5, 0.5, 0.5, ignore)
            assert tuple(losses.shape) == (4,) and tuple(stats.shape) == (30,) and tuple(bad.shape) == (1,) and bad.dtype == torch.int64
            dl = torch.ops.pylc_hip.multiloss_weighted_backward(losses, z, t, u, stats, torch.empty(9), 0.5, 0.5, 0.5, ignore)
            assert tuple(dl.shape) == (2, 9, 8, 8)


# ---- Meta and checkpoints --------------------------------------------------------------------------------------------------------------------
BORDER = {'w0': 10.0, 'sigma': 2.0, 'radius': 3}


def test_meta_border_weight_round_trips_through_update_and_a_checkpoint(tmp_path):
    from pylc_amd.model import Model, Meta
    from pylc_amd import boundary, checkpoint as ck
    assert Meta().border_weight is None and Meta(border_weight=dict(BORDER)).border_weight == BORDER
    assert Meta().update({'border_weight': dict(BORDER)}).border_weight == BORDER
    assert Meta(border_weight=dict(BORDER)).update(Meta()).border_weight is None
    m = Model(Meta(arch='deeplab', backbone='xception', n_classes=4, ch=1, ignore_index=255, border_weight=dict(BORDER)), 'cpu').build()
    radius, ign, table = m._border
    assert (radius, ign) == (3, 255) and np.array_equal(table.numpy(), boundary.border_profile(3, 10.0, 2.0))
    assert Model(Meta(arch='deeplab', backbone='xception', n_classes=4, ch=1), 'cpu').build()._border is None
    path = str(tmp_path / 'checkpoint.pth')
    ck.save(m, path)
    raw = ck.load_reference_file(path)
    assert raw['meta'].border_weight == BORDER and ck.meta_from_reference(raw['meta']).border_weight == BORDER
    assert ck.meta_from_reference(raw['meta']).ignore_index == 255
    del raw['meta'].__dict__['border_weight']                      # a file written before the field existed
    old = ck.meta_from_reference(raw['meta'])
    assert old.border_weight is None and old.n_classes == 4
    ref = ck.load_reference_file(os.path.join(os.path.dirname(__file__), 'golden', 'ref_checkpoint_tiny.pth'))
    assert ck.meta_from_reference(ref['meta']).border_weight is None


# ---- the Python layer's refusals that need no device --------------------------------------------------------------------------------------------
def test_python_argument_rules_without_gpu():
    from pylc_amd import boundary
    from pylc_amd.model import Model, Meta
    mask = torch.zeros((8, 8), dtype=torch.uint8)
    with pytest.raises(TypeError, match='uint8'):
        boundary.border_weights(mask.long(), 3)
    with pytest.raises(ValueError, match='radius'):
        boundary.border_weights(mask, 0)
    with pytest.raises(TypeError, match='radius'):
        boundary.border_weights(mask, 2.5)
    with pytest.raises(ValueError, match='ignore_index'):
        boundary.border_weights(mask, 3, ignore_index=256)
    with pytest.raises(ValueError, match='H,W'):
        boundary.border_weights(torch.zeros(8, dtype=torch.uint8), 3)
    with pytest.raises(ValueError, match='sigma'):
        boundary.border_weights(mask, 3, sigma=0.0)
    with pytest.raises(ValueError, match='no CPU fallback'):
        boundary.border_weights(mask, 3)
    d2 = torch.zeros((8, 8), dtype=torch.int32)
    with pytest.raises(ValueError, match='int32'):
        boundary.weights_from_distance(d2.long(), 3, boundary.border_profile(3))
    with pytest.raises(ValueError, match='radius'):
        boundary.weights_from_distance(d2, 300, boundary.border_profile(3))
    with pytest.raises(ValueError, match='no CPU fallback'):
        boundary.weights_from_distance(d2, 3, boundary.border_profile(3))
    for table in (boundary.border_profile(4), boundary.border_profile(3).astype(np.float64), np.ones((11, 1), np.float32), [1.0] * 11):
        with pytest.raises(ValueError, match=r'float32 \[11\]'):
            boundary._check_table(table, 3, 'cpu')
    assert boundary._check_table(boundary.border_profile(3), 3, 'cpu').dtype == torch.float32

    def build(**kw):
        return Model(Meta(arch='deeplab', backbone='xception', n_classes=4, ch=1, **kw), 'cpu').build()
    for bad in ({'w0': 1.0, 'sigma': 2.0}, {'w0': 1.0, 'sigma': 2.0, 'radius': 3, 'more': 1}, (10.0, 5.0, 3), 'border'):
        with pytest.raises(ValueError, match='border_weight'):
            build(border_weight=bad)
    for ignore in (-100, 256, -1):
        with pytest.raises(ValueError, match='ignore_index=%d' % ignore):
            build(border_weight=dict(BORDER), ignore_index=ignore)
    with pytest.raises(ValueError, match='sigma'):
        build(border_weight={'w0': 1.0, 'sigma': 0.0, 'radius': 3})
    with pytest.raises(ValueError, match='radius'):
        build(border_weight={'w0': 1.0, 'sigma': 1.0, 'radius': 255})
    assert build(border_weight=dict(BORDER))._border[1] is None and build(border_weight=dict(BORDER), ignore_index=0)._border[1] == 0
    m = build(border_weight=None)
    with pytest.raises(ValueError, match='B,H,W'):
        m._train_weights(torch.zeros((2, 8, 8), dtype=torch.uint8), torch.ones(8, 8))
    with pytest.raises(ValueError, match='do not match'):
        m._train_weights(torch.zeros((2, 8, 8), dtype=torch.uint8), torch.ones(2, 8, 9))
    got = m._train_weights(torch.zeros((2, 8, 8), dtype=torch.uint8), torch.full((2, 8, 8), 2, dtype=torch.float64))
    assert got.dtype == torch.float32 and got.is_contiguous() and float(got.min()) == 2.0
