"""CPU suite (-m "not gpu") of hard-pixel mining: the yardstick tests/_mining.py proven against independent statements
-- F.cross_entropy in fp64, torch.topk, mmsegmentation's OHEM rule written out in numpy --, the bound on a float32 evaluation shown to hold
and to mean something on the very inputs the GPU suite uses, the edge cases of the selection, every refused argument at the C ABI, in
pylc_amd.mining and in MultiLoss / Model, the declarations and bindings of the four entry points, Meta.hard_mining through a checkpoint
and the operator's registration."""
import ctypes
import math
import os
import re

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from tests import _mining as M

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
INF = float('inf')
NAN = float('nan')


# ---- the loss map ----------------------------------------------------------------------------------------------------------------------------------
def test_nll_ref_is_torch_cross_entropy_in_fp64():
    for c in M.CLASSES:
        rs = np.random.RandomState(100 + c)
        z = (rs.standard_normal((997, c)) * 4.0).astype(np.float32)
        z[::5] = rs.uniform(-30, 30, z[::5].shape).astype(np.float32)
        z[3::11] = -200.0
        t = rs.randint(0, c, 997)
        z[3::11, 0] = 200.0
        want = F.cross_entropy(torch.from_numpy(z).double(), torch.from_numpy(t), reduction='none').numpy()
        got = M.nll_ref(z, t)
        assert got.dtype == np.float64 and np.abs(got - want).max() < 1e-12, c
        assert (got >= 0).all() and not np.signbit(got).any()


def test_float32_chain_lies_within_the_bound_on_the_gpu_suites_inputs():
    worst = 0.0
    for c in M.CLASSES:
        for n in M.NLL_SIZES:
            z, t = M.logits_and_targets(c, n)
            ref, f32, bound = M.nll_ref(z, t), M.nll_f32(z, t), M.nll_bound(z, t)
            fin = np.isfinite(ref)
            assert f32.dtype == np.float32 and np.array_equal(np.isnan(ref), np.isnan(f32)) and np.array_equal(ref == np.inf, f32 == np.inf)
            err = np.abs(f32[fin].astype(np.float64) - ref[fin])
            assert (err <= bound[fin]).all(), (c, n, float((err / bound[fin]).max()))
            if fin.any():
                worst = max(worst, float((err / bound[fin]).max()))
            # the bound means something: a few units of float32 resolution at the magnitudes involved, 0 where the value is compared exactly
            lse = M._chain(z, t, np.float64)[1]
            assert (bound[fin] <= 1.01 * M.U * (2 + 1.4 * (c - 1) + 4 * math.log(c) + np.abs(lse[fin]) + np.abs(ref[fin])) + 1e-12).all()
            assert (bound[~fin] == 0).all()
            if n >= 257:
                assert (ref[fin] == 0).any() and (ref == np.inf).any() and np.isnan(ref).any() and ref[fin].max() > 20.0      # the planted rows
    print('float32 numpy chain against fp64: worst error / bound = %.3f' % worst)
    assert worst <= 1.0


def test_expected_map_judges_the_target_first():
    nll = np.array([0.5, 0.25, 1.5, 2.5, 3.5, 4.5], np.float64)
    t = np.array([0, 255, 9, 1, 1, 255])
    u = np.array([1.0, NAN, 0.0, 0.0, -1.0, 2.0], np.float32)
    got, part = M.expected_map(nll, t, 3, 255, u)
    assert got.tolist() == [0.5, -1.0, -2.0, -1.0, -2.0, -1.0] and part.tolist() == [True, False, False, False, False, False]
    got, part = M.expected_map(nll, t, 3, None, None)
    assert got.tolist() == [0.5, -2.0, -2.0, 2.5, 3.5, -2.0]


# ---- the selection -----------------------------------------------------------------------------------------------------------------------------------
def test_select_ref_is_topk_without_ties():
    rs = np.random.RandomState(5)
    for n, keep in ((1000, 0.25), (777, 0.1), (5, 0.5), (64, 1.0)):
        v = rs.permutation(n).astype(np.float32) / np.float32(7.0)          # distinct
        out, info = M.select_ref(v, keep, 0, INF)
        k = int(math.ceil(keep * n))
        idx = torch.topk(torch.from_numpy(v), k).indices.numpy()
        want = np.zeros(n, np.float32)
        want[idx] = 1.0
        assert np.array_equal(out, want) and info.tolist() == [n, k, k, M.bits_of(np.sort(v)[n - k])]


def test_select_ref_is_mmsegmentations_rule_with_ties_kept():
    """OHEMPixelSampler's threshold branch, with `>=` on the loss where it has `<` on the probability (p = exp(-nll) is decreasing, so the
    k-th smallest probability is the k-th largest loss and max over probabilities is min over losses): sort the valid pixels, take the
    min_kept-th as the floor threshold, combine it with thresh, keep every pixel at or beyond the result."""
    rs = np.random.RandomState(6)
    for n, min_kept, thresh in ((5000, 300, 0.7), (5000, 4000, 0.7), (5000, 0, 0.3), (100, 100000, 0.5)):
        v = np.abs(rs.standard_normal(n)).astype(np.float32)
        v[::3] = np.float32(0.25)                                            # many ties
        valid = rs.rand(n) > 0.2
        m = np.where(valid, v, np.float32(-1.0))
        cap = np.float32(-np.log(np.float32(thresh)))
        out, info = M.select_ref(m, 0.0, min_kept, cap)
        loss = m[valid]
        desc = np.sort(loss)[::-1]
        floor = desc[min(min_kept, loss.size) - 1] if min_kept > 0 else np.float32(np.inf)
        tau = min(floor, cap)
        want = np.where(valid & (m >= tau), np.float32(1), np.float32(0))
        assert np.array_equal(out, want) and info[0] == valid.sum() and info[1] == min(min_kept, valid.sum())
        assert info[2] == want.sum() >= info[1] and info[3] == M.bits_of(tau)


def test_select_ref_keeps_every_tie_at_tau():
    v = np.array([3, 1, 2, 2, 2, 0.5, 2, 0.1], np.float32)
    out, info = M.select_ref(v, 0.25, 0, INF)                                # k = 2: the 3 and one of the four 2s -> all four are kept
    assert out.tolist() == [1, 0, 1, 1, 1, 0, 1, 0] and info.tolist() == [8, 2, 5, M.bits_of(2.0)]


def test_select_ref_edge_cases():
    v = np.array([0.5, 4.0, -1.0, 1.5, NAN, -2.0, 0.0, -0.0, INF, -0.5], np.float32)
    u = np.array([2.0, 3.0, 5.0, 0.0, 7.0, 9.0, 0.5, 0.25, NAN, 11.0], np.float32)
    # candidates without weights: 0.5 4.0 1.5 0.0 -0.0 inf (6); NaN, -2, -0.5 pass through, -1 gives 0
    out, info = M.select_ref(v, 1e-12, 0, INF)                               # k = 1
    assert info.tolist() == [6, 1, 1, M.INF_BITS] and out[:4].tolist() == [0, 0, 0, 0] and out[8] == 1 and out[[4, 5, 9]].tolist() == [1, 1, 1]
    out, info = M.select_ref(v, 1.0, 0, INF)                                 # k = n_valid: every candidate, -0 as +0
    assert info.tolist() == [6, 6, 6, 0] and out.tolist() == [1, 1, 0, 1, 1, 1, 1, 1, 1, 1]
    assert M.select_ref(v, 0.25, 100, INF)[1].tolist() == [6, 6, 6, 0]       # min_kept above n_valid
    out, info = M.select_ref(v, 1.0, 0, INF, u)                              # weights: 1.5 sits under 0, inf under NaN
    assert info.tolist() == [4, 4, 4, 0]
    assert np.array_equal(out.view(np.uint32), np.array([2.0, 3.0, 0, 0, 7.0, 9.0, 0.5, 0.25, NAN, 11.0], np.float32).view(np.uint32))
    out, info = M.select_ref(v, 0.0, 0, 1.0, u)                              # a cap alone: k = 0, tau = the cap
    assert info.tolist() == [4, 0, 1, M.bits_of(1.0)] and out[:2].tolist() == [0, 3.0]
    none = np.array([-1.0, -2.0, NAN, -7.0], np.float32)                     # no candidate: tau is reported as +inf whatever the cap
    out, info = M.select_ref(none, 0.5, 3, 0.25)
    assert info.tolist() == [0, 0, 0, M.INF_BITS] and out[0] == 0 and out[[1, 2, 3]].tolist() == [1, 1, 1]
    assert M.compute_k(10, 0.25, 0) == 3 and M.compute_k(10, 0.3, 0) == 3 and M.compute_k(10, 0.0, 0) == 0 and M.compute_k(0, 1.0, 5) == 0
    assert M.compute_k(3, 0.1, 2) == 2 and M.compute_k(10 ** 9, 1.0, 0) == 10 ** 9


# ---- refused arguments ------------------------------------------------------------------------------------------------------------------------------
def _abi():
    from pylc_amd import lib as L
    buf = (ctypes.c_char * 4096)()
    base = (ctypes.addressof(buf) + 255) & ~255                              # host memory: never touched, every call below is refused first
    return L, base


def test_c_abi_refuses_bad_arguments_and_launches_nothing():
    L, p = _abi()
    lib = L.lib
    imin = -2 ** 31
    good_l = dict(logits=p, pitch=12, target=p, tb=1, n=100, c=9, ign=imin, pw=p)
    good_s = dict(keep=0.25, min_kept=0, cap=INF, out=p, info=p, ws=p)

    def nll(**kw):
        a = dict(good_l, **kw)
        return lib.pylc_pixel_nll(a['logits'], a['pitch'], a['target'], a['tb'], a['n'], a['c'], a['ign'], a['pw'], a.get('nll', p), None)

    def sel(**kw):
        a = dict(good_s, **kw)
        return lib.pylc_hard_select(a.get('nll', p), a.get('n', 100), a.get('pw', p), a['keep'], a['min_kept'], a['cap'], a['out'], a['info'],
                                    a['ws'], None)

    def fused(**kw):
        a = dict(good_l, **good_s)
        a.update(kw)
        return lib.pylc_hard_pixel_weights(a['logits'], a['pitch'], a['target'], a['tb'], a['n'], a['c'], a['ign'], a['pw'], a['keep'],
                                           a['min_kept'], a['cap'], a.get('nll', p), a['out'], a['info'], a['ws'], None)

    logits_side = [dict(c=1), dict(c=17), dict(tb=4), dict(tb=0), dict(target=None), dict(pitch=8), dict(n=0), dict(n=-5), dict(n=2 ** 31),
                   dict(logits=None), dict(logits=p + 2), dict(pw=p + 2), dict(tb=8, target=p + 4)]
    select_side = [dict(keep=-0.1), dict(keep=1.5), dict(keep=NAN), dict(min_kept=-1), dict(cap=NAN), dict(cap=-1.0), dict(cap=-INF),
                   dict(keep=0.0, min_kept=0, cap=INF), dict(out=None), dict(info=None), dict(ws=None), dict(info=p + 4), dict(ws=p + 8),
                   dict(out=p + 1), dict(pw=p + 2), dict(n=0), dict(n=2 ** 31)]
    for kw in logits_side + [dict(nll=None), dict(nll=p + 1)]:
        assert nll(**kw) == 1, kw
        assert L.lib.pylc_last_error().decode().startswith('pixel_nll:'), kw
    for kw in select_side + [dict(nll=None), dict(nll=p + 2)]:
        assert sel(**kw) == 1, kw
        assert L.lib.pylc_last_error().decode().startswith('hard_select:'), kw
    for kw in logits_side + select_side + [dict(nll=p + 2)]:
        assert fused(**kw) == 1, kw
        assert L.lib.pylc_last_error().decode().startswith('hard_pixel_weights:'), kw
    assert lib.pylc_mining_workspace_bytes(0) == 0 and lib.pylc_mining_workspace_bytes(2 ** 31) == 0 and lib.pylc_mining_workspace_bytes(-1) == 0
    for n in (1, 1000, 2 ** 31 - 1):
        got = lib.pylc_mining_workspace_bytes(n)
        assert got >= 4 * n + 4 * (2048 + 1024 + 1024) and got % 256 == 0


def test_mining_module_refuses_bad_arguments_before_any_launch():
    from pylc_amd import mining, lib as L
    assert mining.selection(0.25) == (0.25, 0, INF) and mining.selection(None, 5, 0.7) == (0.0, 5, float(-np.log(np.float32(0.7))))
    assert mining.selection(1, 0, None) == (1.0, 0, INF) and mining.selection(np.float32(0.5), np.int64(3)) == (0.5, 3, INF)
    for kw in (dict(), dict(keep=0.0), dict(keep=-0.5), dict(keep=1.01), dict(keep=NAN), dict(keep='0.5'), dict(keep=True),
               dict(thresh=0.0), dict(thresh=1.0), dict(thresh=NAN), dict(thresh=-0.2), dict(thresh=1.0 - 1e-12), dict(thresh='x'),
               dict(keep=0.5, min_kept=-1), dict(keep=0.5, min_kept=1.5), dict(keep=0.5, min_kept=None), dict(keep=0.5, min_kept=2 ** 63),
               dict(min_kept=10)):
        with pytest.raises(ValueError):
            mining.selection(**kw)
    assert mining.check_spec(None) is None and mining.check_spec({'keep': 0.5}) == {'keep': 0.5}
    assert mining.check_spec({'thresh': 0.7, 'min_kept': 100}) == {'thresh': 0.7, 'min_kept': 100}
    for spec in ({}, {'keep': 2.0}, {'keep': 0.5, 'ratio': 1}, 0.25, [('keep', 0.5)], {'min_kept': 4}, {'thresh': 0.0}):
        with pytest.raises(ValueError, match='hard_mining|keep|thresh'):
            mining.check_spec(spec)
    z, t, u = torch.zeros(2, 4, 8, 8), torch.zeros(2, 8, 8, dtype=torch.int64), torch.ones(2, 8, 8)
    bad_calls = [
        lambda: mining.pixel_nll(z[0], t),
        lambda: mining.pixel_nll(torch.zeros(2, 17, 8, 8), t),
        lambda: mining.pixel_nll(torch.zeros(2, 1, 8, 8), t),
        lambda: mining.pixel_nll(z, t.int()),
        lambda: mining.pixel_nll(z, t[:, :4]),
        lambda: mining.pixel_nll(z, t, ignore_index=2 ** 31),
        lambda: mining.pixel_nll(z, t, ignore_index=2.5),
        lambda: mining.pixel_nll(z, t, pixel_weights=u.double()),
        lambda: mining.pixel_nll(z, t, pixel_weights=u[:1]),
        lambda: mining.hard_pixel_weights(z, t),
        lambda: mining.hard_pixel_weights(z, t, keep=1.5),
        lambda: mining.hard_pixel_weights(z, t, keep=0.5, min_kept=-2),
        lambda: mining.hard_pixel_weights(z, t.float(), keep=0.5),
        lambda: mining.select(u, keep=0.0),
        lambda: mining.select(u.double(), keep=0.5),
        lambda: mining.select(torch.zeros(0), keep=0.5),
        lambda: mining.select(u, keep=0.5, pixel_weights=u[:1]),
        lambda: mining.select(u, thresh=1.5),
    ]
    for call in bad_calls:
        with pytest.raises(ValueError):
            call()
    for call in (lambda: mining.pixel_nll(z, t), lambda: mining.hard_pixel_weights(z, t, keep=0.5), lambda: mining.select(u, keep=0.5)):
        with pytest.raises(L.PylcError, match='no CPU fallback'):          # a host tensor with good arguments: refused, nothing is initialised
            call()
    assert mining.expected_k(10, 0.25) == 3 and mining.expected_k(10, None, 4) == 4


def test_loss_and_model_layers_refuse_bad_settings():
    from pylc_amd.loss import MultiLoss
    from pylc_amd.model import Model, Meta
    lw = {'weighted': False, 'weights': None, 'ce': 0.5, 'dice': 0.5, 'focal': 0.5}
    assert MultiLoss(lw, {'n_classes': 4}).hard_mining is None and MultiLoss(lw, {'n_classes': 4}).mined is None
    assert MultiLoss(lw, {'n_classes': 4}, hard_mining={'keep': 0.25, 'min_kept': 10}).hard_mining == {'keep': 0.25, 'min_kept': 10}
    for spec in ({}, {'keep': 0.0}, {'keep': 0.5, 'top': 3}, {'thresh': 1.0}, {'keep': 0.5, 'min_kept': -1}, 'ohem'):
        with pytest.raises(ValueError):
            MultiLoss(lw, {'n_classes': 4}, hard_mining=spec)
        with pytest.raises(ValueError):
            Model(Meta(arch='deeplab', backbone='xception', n_classes=4, ch=1, hard_mining=spec), 'cpu').build()
    crit = MultiLoss(lw, {'n_classes': 4}, hard_mining={'keep': 0.25})
    pred = torch.zeros(2, 4, 8, 8)
    with pytest.raises(ValueError, match='soft target'):
        crit(pred, torch.full((2, 4, 8, 8), 0.25))
    with pytest.raises(ValueError, match='match target'):
        crit(pred, torch.zeros(2, 8, 9, dtype=torch.int64))
    with pytest.raises(ValueError, match='uint8 or int64'):
        crit(pred, torch.zeros(2, 8, 8, dtype=torch.int32))
    assert crit.mined is None
    model = Model(Meta(arch='deeplab', backbone='xception', n_classes=4, ch=1, hard_mining={'keep': 0.25}), 'cpu').build()
    with pytest.raises(ValueError, match='soft target'):           # refused by Model.train before the network runs
        model.train(torch.zeros(1, 1, 64, 64), torch.full((1, 4, 64, 64), 0.25))
    assert model.iter == 0


# ---- declarations, bindings, exports ---------------------------------------------------------------------------------------------------------------
def test_header_binding_and_library_agree_on_the_four_entry_points():
    from pylc_amd import lib as L
    hdr = open(os.path.join(ROOT, 'include', 'pylc_hip.h')).read()
    hdr = re.sub(r'/\*.*?\*/', '', hdr, flags=re.S)
    dll = ctypes.CDLL(L.LIB_PATH)
    for name, res in (('pylc_mining_workspace_bytes', ctypes.c_size_t), ('pylc_pixel_nll', ctypes.c_int), ('pylc_hard_select', ctypes.c_int),
                      ('pylc_hard_pixel_weights', ctypes.c_int)):
        m = re.search(r'\b%s\s*\(([^)]*)\)\s*;' % name, hdr)
        assert m, name
        assert name in L.SIGNATURES and hasattr(dll, name) and hasattr(L.lib, name), name
        assert len(m.group(1).split(',')) == len(L.SIGNATURES[name][1]) and L.SIGNATURES[name][0] is res, name
    assert L.ABI_VERSION == 15 and dll.pylc_abi_version() == 15
    assert 'mining.hip' in open(os.path.join(ROOT, 'pylc_amd', 'csrc', 'Makefile')).read()


# ---- Meta and checkpoints ---------------------------------------------------------------------------------------------------------------------------
def test_meta_hard_mining_round_trips_through_update_and_a_checkpoint(tmp_path):
    from pylc_amd.model import Model, Meta
    from pylc_amd import checkpoint as ck
    spec = {'keep': 0.25, 'min_kept': 1000, 'thresh': 0.7}
    assert Meta().hard_mining is None and Meta(hard_mining=spec).hard_mining == spec
    assert Meta().update({'hard_mining': spec}).hard_mining == spec and Meta(hard_mining=spec).update(Meta()).hard_mining is None
    m = Model(Meta(arch='deeplab', backbone='xception', n_classes=4, ch=1, hard_mining=spec), 'cpu').build()
    assert m.crit.hard_mining == spec and m.crit.hard_mining is not spec
    assert Model(Meta(arch='deeplab', backbone='xception', n_classes=4, ch=1), 'cpu').build().crit.hard_mining is None
    path = str(tmp_path / 'checkpoint.pth')
    ck.save(m, path)
    raw = ck.load_reference_file(path)
    assert raw['meta'].hard_mining == spec and ck.meta_from_reference(raw['meta']).hard_mining == spec
    del raw['meta'].__dict__['hard_mining']                        # a file written before the field existed
    old = ck.meta_from_reference(raw['meta'])
    assert old.hard_mining is None and old.n_classes == 4
    ref = ck.load_reference_file(os.path.join(os.path.dirname(__file__), 'golden', 'ref_checkpoint_tiny.pth'))
    assert ck.meta_from_reference(ref['meta']).hard_mining is None


# ---- the operator ----------------------------------------------------------------------------------------------------------------------------------
def test_hard_pixel_weights_operator_is_registered():
    import pylc_amd  # noqa: F401
    from pylc_amd import torch_ops
    from torch._subclasses.fake_tensor import FakeTensorMode
    assert 'hard_pixel_weights' in torch_ops.REGISTERED and len(set(torch_ops.REGISTERED)) == len(torch_ops.REGISTERED)
    assert hasattr(torch.ops.pylc_hip, 'hard_pixel_weights')
    schema = str(torch.ops.pylc_hip.hard_pixel_weights.default._schema)
    assert 'float? keep' in schema and 'float? thresh' in schema and 'Int? ignore_index' in schema and 'Tensor? pixel_weights' in schema
    with FakeTensorMode():
        z, t = torch.empty(2, 9, 8, 10), torch.empty(2, 8, 10, dtype=torch.int64)
        w, info = torch.ops.pylc_hip.hard_pixel_weights(z, t, None, 0.25, 0, None, None)
        assert tuple(w.shape) == (2, 8, 10) and w.dtype == torch.float32 and tuple(info.shape) == (4,) and info.dtype == torch.int64
        w, info = torch.ops.pylc_hip.hard_pixel_weights(z.requires_grad_(True), t, torch.empty(2, 8, 10), None, 100, 0.7, 255)
        assert not w.requires_grad and not info.requires_grad                # nothing differentiable comes out
