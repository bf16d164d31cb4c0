"""CPU suite (-m "not gpu") for the window-weighted blend (pylc_amd.inference.blend_window, csrc/blend.hip).  The
reference has no such window, so the statement of tests/_window.py -- what the GPU tests compare the kernels with -- is pinned here:
against the unweighted statement with a table of ones, on hand-worked cases, and on a synthetic scene with border errors that shows
what the window is for.  Then the named windows, every argument error that needs no device, the bindings, and the seeds of the GPU
comparisons with float64."""
import ctypes
import inspect
import types

import numpy as np
import pytest
import torch

from tests import _window as Wn
from tests._blend import blend_mean_np
from tests.test_cpu_overlap_tile import overlap_origins, softmax0


def _logits(seed, h, w, out, stride, c=3):
    n = len(overlap_origins(h, out, stride)) * len(overlap_origins(w, out, stride))
    return (np.random.RandomState(seed).standard_normal((n, c, out, out)) * 3).astype(np.float32)


# ---- the statement ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('members', [1, 2])
@pytest.mark.parametrize('stride', [16, 8, 5, 1])
def test_uniform_table_is_the_unweighted_statement(stride, members):
    h, w, out = 37, 53, 16
    ls = [_logits(10 * stride + m, h, w, out, stride) for m in range(members)]
    got, got_m = Wn.blend_window_np(ls, h, w, out, stride, np.ones(out, np.float32))
    want, want_m = blend_mean_np(ls, h, w, out, stride)
    assert np.abs(got - want).max() < 1e-12
    assert np.array_equal(got_m, want_m)
    # and the axis sums of a table of ones are the integer cover counts
    for n in (16, 37, 53):
        assert np.array_equal(Wn.window_sums_f32(np.ones(out, np.float32), n, out, stride), Wn.cover_counts(n, out, stride).astype(np.float32))


def test_hand_worked_two_tiles_on_a_strip():
    """A 24-pixel strip, tile 16, stride 8: two tiles (origins 0 and 8) overlapping by half, a triangular table, one probability per tile.
    (The statement's tiles are square: the strip is 16 rows of the same numbers, and the row weight cancels.)"""
    out, w = 16, 24
    tri = (np.minimum(np.arange(out) + 1, out - np.arange(out)) / 8.0).astype(np.float32)         # 1/8 .. 1 .. 1/8
    za, zb = 1.25, -0.5                                                 # class-1 logit of tile A and of tile B (class 0: 0)
    logits = np.zeros((2, 2, out, out), np.float32)
    logits[0, 1], logits[1, 1] = za, zb
    pa, pb = 1 / (1 + np.exp(-za)), 1 / (1 + np.exp(-zb))
    probs, mask = Wn.blend_window_np([logits], out, w, out, 8, tri)
    t = tri.astype(np.float64)
    want = np.empty(w)
    want[:8] = pa                                                       # tile A alone: (w * p) / w
    want[16:] = pb
    want[8:16] = (t[8:16] * pa + t[0:8] * pb) / (t[8:16] + t[0:8])
    assert np.abs(probs[1] - want[None, :]).max() < 1e-15 and np.abs(probs.sum(0) - 1).max() < 1e-15
    # x = 8: A's weight 1, B's 1/8; x = 15: A's 1/8, B's 1 -- the blend leans on the tile whose middle is near
    assert abs(probs[1, 0, 8] - (pa + pb / 8) / (1 + 1 / 8)) < 1e-15 and abs(probs[1, 0, 15] - (pa / 8 + pb) / (1 / 8 + 1)) < 1e-15
    assert np.array_equal(mask[0], (want > 0.5).astype(np.uint8))
    sx = Wn.window_sums_f32(tri, w, out, 8)
    assert np.array_equal(sx[:8], tri[:8]) and np.array_equal(sx[16:], tri[8:]) and np.array_equal(sx[8:16], tri[8:] + tri[:8])


def test_hand_worked_single_tile():
    """n == out: one tile, the clamped last one; every pixel gets its probabilities back whatever the table"""
    out = 16
    logits = _logits(3, out, out, out, out)
    assert logits.shape[0] == 1
    for win in (Wn.window_np('hann', out), Wn.random_table(1, out)):
        probs, _ = Wn.blend_window_np([logits], out, out, out, 5, win)
        assert np.abs(probs - softmax0(logits[0].astype(np.float64))).max() < 1e-15
        assert np.array_equal(Wn.window_sums_f32(win, out, out, 5), win)


def test_hand_worked_clamped_last_tile():
    """37 = 16 + 16 + 5: the origins are 0, 16 and 21 (not 32); pixels 21 .. 31 have tiles 1 and 2, pixels 32 .. 36 tile 2 alone"""
    n, out = 37, 16
    assert overlap_origins(n, out, out) == [0, 16, 21]
    win = Wn.random_table(2, out)
    s = Wn.window_sums_f32(win, n, out, out)
    assert np.array_equal(s[:16], win) and np.array_equal(s[16:21], win[:5])
    assert np.array_equal(s[21:32], win[5:16] + win[:11]) and np.array_equal(s[32:], win[11:])
    # one probability per tile column, along x on a 16 x 37 image
    z = np.array([0.5, -1.0, 2.0])
    logits = np.zeros((3, 2, out, out), np.float32)
    for j in range(3):
        logits[j, 1] = z[j]
    p = 1 / (1 + np.exp(-z))
    probs, _ = Wn.blend_window_np([logits], out, n, out, out, win)
    t = win.astype(np.float64)
    want = np.concatenate([np.full(16, p[0]), np.full(5, p[1]), (t[5:16] * p[1] + t[:11] * p[2]) / (t[5:16] + t[:11]), np.full(5, p[2])])
    assert np.abs(probs[1] - want[None, :]).max() < 1e-15
    # stride 5: 0, 5, 10, 15, 20, then 21 for the clamped one; the sums visit them in that order
    assert overlap_origins(n, out, 5) == [0, 5, 10, 15, 20, 21]
    s5 = Wn.window_sums_f32(win, n, out, 5)
    y = 30                                                              # tiles 3 (ly 15), 4 (ly 10) and the last (ly 9)
    assert s5[y] == np.float32(np.float32(win[15] + win[10]) + win[9])


def test_asymmetric_table_is_indexed_after_the_mirror_back():
    """the weight belongs to the placed position: a mirrored member whose logits are the mirrored member-0 logits is the same member"""
    h, w, out, stride = 16, 40, 16, 8
    l0 = _logits(8, h, w, out, stride)
    l1 = np.ascontiguousarray(l0[:, :, :, ::-1])
    win = Wn.random_table(5, out)
    one, _ = Wn.blend_window_np([l0], h, w, out, stride, win)
    two, _ = Wn.blend_window_np([l0, l1], h, w, out, stride, win)
    assert np.abs(one - two).max() < 1e-15
    wrong, _ = Wn.blend_window_np([l0], h, w, out, stride, np.ascontiguousarray(win[::-1]))
    assert np.abs(one - wrong).max() > 1e-3                            # and the table's direction matters


def test_float32_models():
    acc = np.random.RandomState(0).random_sample((5, 7, 4)).astype(np.float32)
    sy, sx = Wn.random_table(3, 5) * 3, Wn.random_table(4, 7) * 2
    probs, conf, mask = Wn.finalize_f32(acc, 2, sy, sx)
    for y, x, c in ((0, 0, 0), (4, 6, 3), (2, 3, 1)):
        assert probs[c, y, x] == np.float32(acc[y, x, c] / np.float32(np.float32(2) * np.float32(sy[y] * sx[x])))
    assert np.array_equal(conf, probs.max(0)) and np.array_equal(mask, probs.argmax(0))
    tie = np.full((1, 1, 3), 0.5, np.float32)
    assert Wn.finalize_f32(tie, 1, np.ones(1, np.float32), np.ones(1, np.float32))[2][0, 0] == 0     # the first maximum


# ---- the named windows ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('out', [1, 2, 16, 324, 512])
def test_named_windows(out):
    from pylc_amd import inference
    for spec in ('uniform', 'hann', 'gauss', ('gauss', 0.25)):
        tab = inference.window_table(spec, out)
        assert tab.dtype == np.float32 and tab.shape == (out,)
        assert np.array_equal(tab, Wn.window_np(spec, out))              # the package builds what the statement states
        assert np.array_equal(tab, tab[::-1]) and (tab > 0).all() and tab.max() <= 1.0
        if out > 2 and spec != 'uniform':
            assert tab[out // 2] > tab[0] and (np.diff(tab[:out // 2 + 1]) >= 0).all()      # it falls off towards the edge
    assert np.array_equal(inference.window_table('uniform', out), np.ones(out, np.float32))
    assert np.array_equal(inference.window_table(('gauss', 0.125), out), inference.window_table('gauss', out))


def test_gauss_closed_form():
    out = 512
    i = np.arange(out, dtype=np.float64)
    want = np.exp(-((i - 255.5) ** 2) / (2 * 64.0 ** 2))                # sigma = 0.125 * 512 = 64, centre (out - 1) / 2
    assert np.abs(Wn.window_f64('gauss', out) - want).max() < 1e-12
    assert np.abs(Wn.window_f64('hann', out) - np.sin(np.pi * (i + 0.5) / out) ** 2).max() < 1e-12
    assert Wn.window_f64('hann', out).min() > 9e-6                      # sin^2(pi / 1024): above the 2^-20 ratio rule


# ---- refused arguments -----------------------------------------------------------------------------------------------------------------------
BAD_WINDOWS = [('hamming', 'named window'), (('hann', 2.0), 'named window'), (('gauss',), 'named window'), (('gauss', 0.1, 0.2), 'named window'),
               (('gauss', 0.0), 'sigma_frac'), (('gauss', -0.125), 'sigma_frac'), (('gauss', float('inf')), 'sigma_frac'),
               (('gauss', float('nan')), 'sigma_frac'), (('gauss', 'wide'), 'sigma_frac'), (('gauss', 1e-3), 'non-positive'),
               (np.ones(15, np.float32), r'\[16\]'), (np.ones((16, 1), np.float32), r'\[16\]'), (torch.ones(17), r'\[16\]'),
               (np.array(['a'] * 16), r'\[16\]'), (3.0, 'window is None'), (True, 'window is None'),
               (np.r_[np.ones(15), np.nan].astype(np.float32), 'non-finite'), (np.r_[np.ones(15), np.inf].astype(np.float32), 'non-finite'),
               (np.r_[np.ones(15), 0.0].astype(np.float32), 'non-positive'), (np.r_[np.ones(15), -1.0].astype(np.float32), 'non-positive'),
               (np.r_[np.ones(15), 1e-60], 'non-positive'),                                       # positive in float64, zero as float32
               (np.r_[np.ones(15), 2.0 ** -21].astype(np.float32), r'2\*\*-20'), (torch.tensor([1.0] * 15 + [1e-7]), r'2\*\*-20')]


@pytest.mark.parametrize('k', range(len(BAD_WINDOWS)))
def test_blend_window_refuses(k):
    """window_table is blend_window's validation: it raises before the device (here: one that does not exist) is touched"""
    from pylc_amd import inference
    spec, word = BAD_WINDOWS[k]
    with pytest.raises(ValueError, match=word):
        inference.window_table(spec, 16)
    with pytest.raises(ValueError, match=word):
        inference.blend_window(spec, 16, 'cuda:0')
    with pytest.raises(ValueError, match='output tile'):
        inference.window_table('hann', 0)


def test_blend_window_accepts():
    from pylc_amd import inference
    tab = np.r_[np.ones(15), 2.0 ** -20].astype(np.float32)             # the ratio rule's edge is allowed
    assert np.array_equal(inference.window_table(tab, 16), tab)
    assert np.array_equal(inference.window_table(torch.from_numpy(tab).double(), 16), tab)
    assert np.array_equal(inference.window_table([1, 2, 3], 3), np.array([1, 2, 3], np.float32))
    got = inference.blend_window(Wn.random_table(1, 16), 16, 'cpu')     # a caller table is taken as given, on the device asked for
    assert got.dtype == torch.float32 and np.array_equal(got.numpy(), Wn.random_table(1, 16))
    a, b = inference.blend_window('hann', 16, 'cpu'), inference.blend_window('hann', 16, 'cpu')
    assert a is b and inference.blend_window(('gauss', 0.125), 16, 'cpu') is inference.blend_window(('gauss', 0.125), 16, 'cpu')
    assert inference.blend_window('hann', 32, 'cpu') is not a


def test_pipeline_argument_errors():
    """the window is checked before the model or the device are touched, in all four entry points"""
    from pylc_amd import inference, photo
    deeplab = types.SimpleNamespace(meta=types.SimpleNamespace(arch='deeplab', ch=3, pad_size=0))
    unet = types.SimpleNamespace(meta=types.SimpleNamespace(arch='unet', ch=3, pad_size=94))
    img = torch.zeros((3, 64, 64), dtype=torch.uint8)
    photo_img = np.zeros((64, 64, 3), np.uint8)
    for spec, word in BAD_WINDOWS[:9] + [(np.ones(15, np.float32), r'\[64\]'), (np.r_[np.ones(63), 0.0], 'non-positive')]:
        with pytest.raises(ValueError, match=word):
            inference.predict_blend_mean(deeplab, img, 64, 64, window=spec)
        with pytest.raises(ValueError, match=word):
            inference.predict_image(deeplab, img, 64, blend='mean', window=spec)
        with pytest.raises(ValueError, match=word):
            inference.predict_overlap_tile(unet, img, 252, window=spec)                   # out = 252 - 2 * 94 = 64
        with pytest.raises(ValueError, match=word):
            inference.predict_image(unet, img, 252, window=spec)
        for model, tile in ((deeplab, 64), (unet, 252)):
            with pytest.raises(ValueError, match=word):
                photo.segment_photo(model, photo_img, tile=tile, blend='mean', window=spec)
    with pytest.raises(ValueError, match="window needs blend='mean'"):
        inference.predict_image(deeplab, img, 64, window='hann')
    with pytest.raises(ValueError, match="window needs blend='mean'"):
        inference.predict_image(deeplab, img, 64, blend='reference', window='uniform')
    with pytest.raises(ValueError, match="flip, window needs blend='mean'"):
        inference.predict_image(deeplab, img, 64, flip=True, window='hann')
    with pytest.raises(ValueError, match="window needs blend='mean' on a DeepLab"):
        photo.segment_photo(deeplab, photo_img, tile=64, window='gauss')


# ---- window=None -----------------------------------------------------------------------------------------------------------------------------
class _Recorder:
    """stands in for the loaded library: records the entry points called"""

    def __init__(self):
        self.calls = []

    def __getattr__(self, name):
        def fn(*args):
            self.calls.append(name)
            return 0
        return fn


def test_window_none_enters_nothing_new(monkeypatch):
    from pylc_amd import inference, photo
    for fn in (inference.predict_image, inference.predict_overlap_tile, inference.predict_blend_mean, photo.segment_photo):
        params = inspect.signature(fn).parameters
        assert params['window'].default is None and list(params)[-1] == 'window'
    rec = _Recorder()
    monkeypatch.setattr(inference, 'lib', rec)
    monkeypatch.setattr(inference, 'ptr', lambda t: None)
    monkeypatch.setattr(inference, 'stream', lambda: None)
    acc = torch.zeros((20, 24, 4))
    inference._blend_finalize(acc, 4, 20, 24, 16, 8, 3, 1, True, True)
    assert rec.calls == ['pylc_blend_finalize']
    del rec.calls[:]
    inference._blend_finalize(acc, 4, 20, 24, 16, 8, 3, 1, True, True, 2.0)
    assert rec.calls == ['pylc_ensemble_finalize']
    del rec.calls[:]
    inference._blend_finalize(acc, 4, 20, 24, 16, 8, 3, 1, True, True, None, torch.ones(16))
    assert rec.calls == ['pylc_blend_window_sums', 'pylc_blend_window_sums', 'pylc_blend_finalize_w']
    del rec.calls[:]
    inference._blend_finalize(acc, 4, 20, 24, 16, 8, 3, 1, True, True, 2.0, torch.ones(16))      # the resample step has divided already
    assert rec.calls == ['pylc_ensemble_finalize']
    # the sweep: one batch of two tiles through a stand-in for the network
    run = types.SimpleNamespace(ncls=3, cp=4, dev=torch.device('cpu'), mine=lambda n, batch: [(0, 2)])
    run.batches = lambda mine, tile, out, stride, member, img: ((k, b, torch.zeros((b, 3, 16, 16))) for k, b in mine)
    monkeypatch.setattr(inference.ops, 'as_nhwc', lambda y: y)
    monkeypatch.setattr(inference.ops, 'pitch_of', lambda y: 4)
    img = torch.zeros((3, 16, 24))
    for beta, win, want in ((None, None, 'pylc_blend_accumulate'), (0.5, None, 'pylc_blend_accumulate_t'),
                            (None, torch.ones(16), 'pylc_blend_accumulate_w'), (0.5, torch.ones(16), 'pylc_blend_accumulate_w')):
        del rec.calls[:]
        inference._blend_sweep(run, img, 16, 16, 8, 8, 2, beta, win)
        assert rec.calls == [want, want]                               # one launch per member, nothing else


def test_bindings_exist():
    from pylc_amd import lib as L
    dll = ctypes.CDLL(L.LIB_PATH)
    for name, nargs in (('pylc_blend_accumulate_w', 15), ('pylc_blend_window_sums', 6), ('pylc_blend_finalize_w', 12),
                        ('pylc_blend_resample_accumulate_w', 15)):
        assert hasattr(dll, name)
        assert len(L.SIGNATURES[name][1]) == nargs and L.SIGNATURES[name][0] is ctypes.c_int
    assert L.lib.pylc_abi_version() == L.ABI_VERSION
    header = open(L.LIB_PATH.rsplit('/pylc_amd/', 1)[0] + '/include/pylc_hip.h').read()
    assert 'NaN / inf probabilities, not a fault' in header             # what a zero in a table reaching the ABI gives


def check_entry_points_refuse():
    """Every refused argument of the four entry points returns PYLC_ERR_ARG before any launch (nothing is dereferenced: the addresses
    are made up).  Also run by tests/test_window_gpu.py on the device."""
    from pylc_amd.lib import lib
    one = 1 << 12

    def refused(rc, word):
        assert rc == 1 and word in lib.pylc_last_error(), lib.pylc_last_error()

    def acc_w(logits=one, pitch=4, first=0, n=1, h=37, w=53, out=16, stride=8, c=3, flip=0, acc=one, acc_pitch=4, win=one, beta=1.0):
        return lib.pylc_blend_accumulate_w(logits, pitch, first, n, h, w, out, stride, c, flip, acc, acc_pitch, win, beta, None)
    refused(acc_w(win=None), b'win')
    refused(acc_w(win=one + 2), b'win')
    for beta in (0.0, -1.0, float('inf'), float('nan')):
        refused(acc_w(beta=beta), b'inv_temperature')
    for kw in ({'logits': None}, {'logits': one + 4}, {'pitch': 2}, {'pitch': 6}):
        refused(acc_w(**kw), b'logits')
    for kw in ({'acc': None}, {'acc': one + 8}, {'acc_pitch': 2}, {'acc_pitch': 5}):
        refused(acc_w(**kw), b'acc must')
    refused(acc_w(flip=2), b'flip')
    refused(acc_w(stride=0), b'stride')
    refused(acc_w(stride=17), b'stride')
    refused(acc_w(h=15), b'smaller')
    refused(acc_w(out=0), b'out=')
    refused(acc_w(first=-1), b'outside')
    refused(acc_w(n=0), b'outside')
    refused(acc_w(first=20, n=5), b'outside')                           # the grid is 4 x 6
    refused(acc_w(c=1, pitch=4), b'n_classes')
    refused(acc_w(c=17, pitch=20, acc_pitch=20), b'n_classes')

    def sums(win=one, out=16, stride=8, n=37, s=one + 256):
        return lib.pylc_blend_window_sums(win, out, stride, n, s, None)
    refused(sums(win=None), b'NULL')
    refused(sums(s=None), b'NULL')
    refused(sums(win=one + 1), b'aligned')
    refused(sums(s=one + 2), b'aligned')
    refused(sums(s=one), b'alias')
    refused(sums(out=0), b'out=')
    refused(sums(stride=0), b'stride')
    refused(sums(stride=17), b'stride')
    refused(sums(n=15), b'smaller')

    def fin(acc=one, pitch=4, h=37, w=53, c=3, members=1, sy=one, sx=one, mask=one, probs=None, conf=None):
        return lib.pylc_blend_finalize_w(acc, pitch, h, w, c, members, sy, sx, mask, probs, conf, None)
    for kw in ({'acc': None}, {'mask': None}, {'acc': one + 4}, {'pitch': 2}, {'pitch': 7}):
        refused(fin(**kw), b'acc must')
    refused(fin(mask=one + 1), b'mask')
    for kw in ({'sy': None}, {'sx': None}, {'sy': one + 2}, {'sx': one + 1}):
        refused(fin(**kw), b'sum_y')
    refused(fin(members=0), b'members')
    refused(fin(h=0), b'H=')
    refused(fin(w=-3), b'W=')
    refused(fin(c=1), b'n_classes')
    refused(fin(c=17, pitch=20), b'n_classes')

    def res(acc=one, pitch=4, hs=28, ws=40, members=1, weight=1.0, c=3, sy=one, sx=one, ens=one + 256, ens_pitch=4, h=37, w=53, add=0):
        return lib.pylc_blend_resample_accumulate_w(acc, pitch, hs, ws, members, weight, c, sy, sx, ens, ens_pitch, h, w, add, None)
    refused(res(acc=None), b'NULL')
    refused(res(ens=None), b'NULL')
    for kw in ({'acc': one + 4}, {'pitch': 2}, {'pitch': 6}):
        refused(res(**kw), b'acc_s must')
    for kw in ({'ens': one + 260}, {'ens_pitch': 2}, {'ens_pitch': 6}):
        refused(res(**kw), b'ens must')
    refused(res(ens=one), b'alias')
    for kw in ({'sy': None}, {'sx': None}, {'sy': one + 2}, {'sx': one + 3}):
        refused(res(**kw), b'sum_y_s')
    refused(res(members=0), b'members')
    for weight in (0.0, -1.0, float('inf'), float('nan')):
        refused(res(weight=weight), b'weight')
    refused(res(hs=0), b'Hs=')
    refused(res(ws=0), b'Ws=')
    refused(res(h=0), b'add=')
    refused(res(add=2), b'add=')
    refused(res(c=1), b'n_classes')
    refused(res(c=17, pitch=20, ens_pitch=20), b'n_classes')


def test_entry_point_errors_without_gpu():
    check_entry_points_refuse()


# ---- what the window is for ----------------------------------------------------------------------------------------------------------------
def test_border_error_scene_is_repaired():
    """Two classes, per-tile logits right in the tile's interior and pushed towards the wrong class within 4 pixels of each tile's
    border (what zero padding does), stride = out / 2: the Hann-weighted blend has strictly fewer wrong pixels than the equal-weight
    one.  Measured: see DESIGN.md 5.25."""
    truth, logits = Wn.border_error_scene()
    h, w = truth.shape
    out, stride = logits.shape[2], logits.shape[2] // 2
    wrong = {}
    for name in ('uniform', 'hann', 'gauss'):
        wrong[name] = int((Wn.blend_window_np([logits], h, w, out, stride, Wn.window_np(name, out))[1] != truth).sum())
    plain = int((blend_mean_np([logits], h, w, out, stride)[1] != truth).sum())
    print('border-error scene %dx%d, tile %d, stride %d: %d wrong pixels equal-weight, %d Hann, %d Gauss'
          % (h, w, out, stride, wrong['uniform'], wrong['hann'], wrong['gauss']))
    assert plain == wrong['uniform']
    assert wrong['hann'] < wrong['uniform']


# ---- the seeds of the GPU comparisons with float64 -------------------------------------------------------------------------------------------
@pytest.mark.parametrize('stride', Wn.STRIDES)
@pytest.mark.parametrize('c', Wn.CLASSES)
def test_gpu_case_seeds_are_decided(c, stride):
    """tests/test_window_gpu.py compares masks where the float64 statement decides at 1e-5 and asks for a decided share >= 0.999:
    guaranteed here for exactly its seeds and windows"""
    l0, l1 = Wn.case_logits(c, stride)
    for name in Wn.WINDOWS:
        probs, _ = Wn.blend_window_np([l0, l1], Wn.H, Wn.W, Wn.OUT, stride, Wn.case_window(name))
        share = Wn.decided(probs).mean()
        assert share >= 0.999, (c, stride, name, share)
        assert np.abs(probs.sum(0) - 1).max() < 1e-12
    tab = Wn.case_window('random')
    assert not np.array_equal(tab, tab[::-1]) and tab.min() >= 0.05     # asymmetric, within the ratio rule
