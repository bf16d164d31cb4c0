"""The Python driver of the loss head, pinned without a GPU: host tensors go through ops.misc.multiloss_forward / multiloss_backward with the
library, the pointer / stream helpers and the collective replaced by recorders, and every path is held to the entry points it calls, the
arguments that tell the paths apart, the tensors it saves and the LossState it leaves.  The expected table was written from the code that had
one copy of the forward per option and passed on it unchanged; a path that starts to call an equivalent entry point fails here."""
import pytest
import torch

from pylc_amd import lib as L
from pylc_amd.ops import misc

B, C, H, W = 1, 9, 5, 7
N = B * H * W
PITCH = 12
WEIGHTS = (0.5, 0.3, 0.2)
NO_IGNORE = -2 ** 31
ST, WORLD, GROUP = 7, 4, 'a group'
WS, GS = 'workspace', 'grad scale'          # pointers of tensors the driver allocates and keeps to itself: any int


class Recorder:
    """stands in for the library: every entry point returns PYLC_OK and is noted with its arguments"""

    def __init__(self):
        self.calls = []

    def __getattr__(self, name):
        if name == 'pylc_multiloss_workspace_floats':            # host only
            return getattr(L.lib, name)
        return lambda *a: self.calls.append((name, a)) or 0


@pytest.fixture
def rec(monkeypatch):
    r = Recorder()
    r.checked, r.reduced = [], []
    monkeypatch.setattr(misc, 'lib', r)
    monkeypatch.setattr(misc, 'check', r.checked.append)
    monkeypatch.setattr(misc, 'ptr', lambda t: None if t is None else t.data_ptr())
    monkeypatch.setattr(misc, 'stream', lambda: ST)
    monkeypatch.setattr(misc, 'ranges_needed', lambda: False)
    monkeypatch.setattr(L, 'init', lambda: None)
    monkeypatch.setattr(misc._runtime, 'sync_all_reduce', lambda t, g: r.reduced.append((t, g)))
    monkeypatch.setattr(misc._runtime, 'shard_check', None)
    monkeypatch.setattr(misc.dist, 'get_world_size', lambda g=None: WORLD)
    return r


def tensors():
    g = torch.Generator().manual_seed(3)
    t = {'z': torch.randn(B, H, W, PITCH, generator=g).permute(0, 3, 1, 2)[:, :C],          # NHWC memory, pitch 12
         'cw': torch.rand(C, generator=g) + 0.5,
         'i64': torch.randint(0, C, (B, H, W), generator=g),
         'pw': torch.rand(B, H, W, generator=g),
         'bad': torch.zeros(1, dtype=torch.int64),
         'soft': torch.rand(B, H, W, C, generator=g).permute(0, 3, 1, 2)}                        # a channels-last view: strides (315, 1, 63, 9)
    t['u8'] = t['i64'].to(torch.uint8)
    return t


SOFT_STRIDES = (H * W * C, 1, W * C, C)

# name: (keywords of multiloss_forward (tensors by their key above), statistics entry, its arguments between (logits, pitch) and (stats, ws),
#        whether bad follows ws, finalize entry, LossState.ignore, LossState.soft, key of the saved target, backward entry,
#        its arguments between (logits, pitch) and stats)
PATHS = {
    'plain': (dict(target='i64', bad='pw'),                      # bad is neither read nor checked: a float [1,5,7] tensor passes
              'pylc_multiloss_stats', ('i64', N, C, 'cw'), False, 'pylc_multiloss_finalize', None, None, 'i64',
              'pylc_multiloss_bwd', ('i64', N, C, 'cw')),
    'ignore_u8': (dict(target='u8', ignore_index=255, bad='bad'),
                  'pylc_multiloss_stats_ex', ('u8', 1, N, C, 255, 'cw'), True, 'pylc_multiloss_finalize_ex', 255, None, 'u8',
                  'pylc_multiloss_bwd_ex', ('u8', 1, N, C, 255, 'cw')),
    'ignore_i64': (dict(target='i64', ignore_index=-100),
                   'pylc_multiloss_stats_ex', ('i64', 8, N, C, -100, 'cw'), True, 'pylc_multiloss_finalize_ex', -100, None, 'i64',
                   'pylc_multiloss_bwd_ex', ('i64', 8, N, C, -100, 'cw')),
    'weighted_index': (dict(target='u8', ignore_index=3, pixel_weights='pw', bad='bad'),
                       'pylc_multiloss_stats_w', ('u8', 1, N, C, 3, 'cw', 'pw'), True, 'pylc_multiloss_finalize_ex', 3, None, 'u8',
                       'pylc_multiloss_bwd_w', ('u8', 1, N, C, 3, 'cw', 'pw')),
    'weighted': (dict(target='i64', pixel_weights='pw'),
                 'pylc_multiloss_stats_w', ('i64', 8, N, C, NO_IGNORE, 'cw', 'pw'), True, 'pylc_multiloss_finalize_ex', NO_IGNORE, None, 'i64',
                 'pylc_multiloss_bwd_w', ('i64', 8, N, C, NO_IGNORE, 'cw', 'pw')),
    'soft_probs_view': (dict(target=None, soft_target='soft', bad='bad'),
                        'pylc_multiloss_stats_soft', (N, H, W, C, 'soft') + SOFT_STRIDES + (0, 1.0, 'cw', None), True,
                        'pylc_multiloss_finalize_ex', None, ('probs', 1.0), 'soft',
                        'pylc_multiloss_bwd_soft', (N, H, W, C, 'soft') + SOFT_STRIDES + (0, 1.0, 'cw', None)),
    'soft_logits_t2': (dict(target=None, soft_target='soft', soft_kind='logits', temperature=2.0, pixel_weights='pw'),
                       'pylc_multiloss_stats_soft', (N, H, W, C, 'soft') + SOFT_STRIDES + (1, 0.5, 'cw', 'pw'), True,
                       'pylc_multiloss_finalize_ex', None, ('logits', 0.5), 'soft',
                       'pylc_multiloss_bwd_soft', (N, H, W, C, 'soft') + SOFT_STRIDES + (1, 0.5, 'cw', 'pw')),
    'smooth': (dict(target='u8', label_smoothing=0.1, bad='bad'),
               'pylc_multiloss_stats_ls', ('u8', 1, N, C, NO_IGNORE, 'cw', None, 0.1), True, 'pylc_multiloss_finalize_ex', NO_IGNORE,
               ('smooth', 0.1), 'u8', 'pylc_multiloss_bwd_ls', ('u8', 1, N, C, NO_IGNORE, 'cw', None, 0.1)),
    'smooth_weighted': (dict(target='i64', label_smoothing=0.1, ignore_index=255, pixel_weights='pw'),
                        'pylc_multiloss_stats_ls', ('i64', 8, N, C, 255, 'cw', 'pw', 0.1), True, 'pylc_multiloss_finalize_ex', 255,
                        ('smooth', 0.1), 'i64', 'pylc_multiloss_bwd_ls', ('i64', 8, N, C, 255, 'cw', 'pw', 0.1)),
}


def resolve(args, t, extra):
    """the expected argument tuple with tensor keys replaced by pointers"""
    table = dict(extra, **{k: v.data_ptr() for k, v in t.items()})
    return tuple(table[a] if isinstance(a, str) else a for a in args)


def same(got, want):
    """argument tuples equal; WS / GS match any pointer"""
    assert len(got) == len(want), (got, want)
    for i, (g, w) in enumerate(zip(got, want)):
        if w in (WS, GS):
            assert isinstance(g, int) and g != 0, (i, got, want)
        else:
            assert g == w and type(g) is type(w), (i, got, want)


@pytest.mark.parametrize('group', (None, GROUP), ids=('single', 'group'))
@pytest.mark.parametrize('path', sorted(PATHS))
def test_each_path_calls_its_entry_points_and_leaves_its_state(rec, path, group):
    kw, stats_fn, stats_mid, has_bad, fin_fn, ignore, soft, saved_key, bwd_fn, bwd_mid = PATHS[path]
    t = tensors()
    kw = {k: t[v] if isinstance(v, str) and v in t else v for k, v in kw.items()}
    target = kw.pop('target')
    losses, saved, state, rest = misc.multiloss_forward(None, t['z'], target, t['cw'], *WEIGHTS, group, **kw)

    assert rest == () and losses.shape == (4,) and losses.dtype == torch.float32
    logits, saved_target, stats = saved[:3]
    assert logits is t['z'] and saved[3] is t['cw']
    k = 3 + 3 * C
    assert stats.shape == (k + (2 if group else 0),) and stats.dtype == torch.float32
    want_saved = t[saved_key]
    assert saved_target.data_ptr() == want_saved.data_ptr() and saved_target.stride() == want_saved.stride()
    assert saved_target.dtype == want_saved.dtype and saved_target.shape == want_saved.shape
    pw = kw.get('pixel_weights')
    assert len(saved) == (4 if pw is None else 5)
    if pw is not None:
        assert saved[4].data_ptr() == pw.data_ptr() and not saved[4].requires_grad

    n_global = float(N) * (WORLD if group else 1) if path == 'plain' else None
    assert type(state) is misc.LossState
    assert state.cfg == (n_global,) + WEIGHTS + (group,) and state.ignore == ignore and state.soft == soft
    assert type(state.ignore) is type(ignore)

    extra = {'stats': stats.data_ptr(), 'losses': losses.data_ptr()}
    bad = kw.get('bad')
    assert [name for name, _ in rec.calls] == [stats_fn, fin_fn] and rec.checked == [0, 0]
    head = (t['z'].data_ptr(), PITCH)
    tail = (stats.data_ptr(), WS) + ((None if bad is None else bad.data_ptr(),) if has_bad else ()) + (ST,)
    same(rec.calls[0][1], head + resolve(stats_mid, t, extra) + tail)
    if path == 'plain':
        same(rec.calls[1][1], (stats.data_ptr(), n_global, C) + WEIGHTS + (losses.data_ptr(), ST))
    else:
        same(rec.calls[1][1], (stats.data_ptr(), C) + WEIGHTS + (losses.data_ptr(), ST))
    if group:
        assert len(rec.reduced) == 1 and rec.reduced[0][0] is stats and rec.reduced[0][1] is group
        assert stats[k:].tolist() == [float(B), float(B * B)]
        pend = misc._runtime.shard_check
        assert pend['world'] == WORLD and len(pend['pairs']) == 1 and pend['pairs'][0].data_ptr() == stats[k:].data_ptr()
    else:
        assert rec.reduced == [] and misc._runtime.shard_check is None

    del rec.calls[:], rec.checked[:]
    (dl,) = misc.multiloss_backward(state, saved, None, torch.ones(4))
    assert dl.shape == (B, C, H, W) and misc.pitch_of(dl) == PITCH
    assert [name for name, _ in rec.calls] == [bwd_fn] and rec.checked == [0]
    mid = resolve(bwd_mid, t, extra) + (stats.data_ptr(),) + ((n_global,) if path == 'plain' else ())
    same(rec.calls[0][1], head + mid + WEIGHTS + (GS, dl.data_ptr(), PITCH, None, ST))


def test_single_bad_arguments_keep_their_exception(rec):
    t = tensors()
    fwd = lambda target, **kw: misc.multiloss_forward(None, t['z'], target, t['cw'], *WEIGHTS, None, **kw)
    f32 = t['i64'].float()
    for target, kw, text in ((t['u8'], {}, 'target must be int64 [B,H,W] matching the logits'),
                             (f32, {'ignore_index': 255}, 'target must be uint8 or int64 [B,H,W] matching the logits'),
                             (f32, {'label_smoothing': 0.1}, 'target must be uint8 or int64 [B,H,W] matching the logits'),
                             (None, {'label_smoothing': 0.1}, 'target must be uint8 or int64 [B,H,W] matching the logits'),
                             (t['i64'], {'pixel_weights': t['pw'][:, :4]}, 'pixel_weights must be float32 [B,H,W] matching the logits, on their device'),
                             (t['i64'], {'pixel_weights': t['pw'].double(), 'label_smoothing': 0.1},
                              'pixel_weights must be float32 [B,H,W] matching the logits, on their device'),
                             (t['i64'], {'ignore_index': 255, 'bad': t['pw']}, 'bad must be an int64 [1] tensor on the device of the logits'),
                             (t['i64'], {'pixel_weights': t['pw'], 'bad': t['pw']}, 'bad must be an int64 [1] tensor on the device of the logits'),
                             (t['i64'], {'label_smoothing': 0.1, 'bad': t['pw']}, 'bad must be an int64 [1] tensor on the device of the logits'),
                             (None, {'soft_target': t['soft'], 'bad': t['pw']}, 'bad must be an int64 [1] tensor on the device of the logits'),
                             (t['i64'], {'label_smoothing': 1.0}, 'label_smoothing must lie in [0, 1), got 1.0'),
                             (t['i64'], {'soft_target': t['soft']}, 'pass target=None with a soft_target: the rows of the soft tensor are the target'),
                             (None, {'soft_target': t['soft'][:, :4]}, 'soft_target must be float32 [B,C,H,W] matching the logits, on their device')):
        with pytest.raises(L.PylcError) as e:
            fwd(target, **kw)
        assert str(e.value) == text, (kw, str(e.value))
    with pytest.raises(AttributeError):                   # the hard paths take the target as a tensor before they judge it
        fwd(None)
    assert rec.calls == []
