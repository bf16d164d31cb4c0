"""Hard-pixel mining (csrc/mining.hip): a pixel-weight map taken from the step's own logits -- the pixels the model
currently gets most wrong -- for the loss head's pixel_weights.  Two standard rules, alone or together:

    keep     bootstrapped (top-k) cross-entropy: the fraction `keep` of the candidate pixels with the largest loss -log p_t;
    thresh   OHEM (mmsegmentation's OHEMPixelSampler): every pixel whose true-class probability is at most `thresh`, and at least
             `min_kept` pixels.

Definitions (include/pylc_hip.h): nll_n = lse - z_t in float32 with the loss head's operation order; a candidate is a pixel the weighted
loss head would take (valid target, 0 < u <= FLT_MAX) whose nll is not NaN.  With n_valid candidates,
k = min(n_valid, max(min_kept, ceil(keep * n_valid))), tau_k the k-th largest candidate nll (+inf for k == 0) and
tau = min(tau_k, -log(thresh)): a candidate with nll >= tau keeps its weight (1 without weights; every tie at tau is kept), the other
candidates, ignored pixels and pixels of weight 0 get 0, and everything else -- a bad target, a bad weight, a NaN row -- passes its input
weight through, so the loss that follows still counts the bad pixel and still goes NaN on the NaN row.  info is an int64 [4] device
tensor: n_valid, k, the number of kept pixels, the IEEE bits of tau.  The selection is an exact radix select with integer counts: no
sort, no host read, bitwise reproducible.  Nothing here synchronises with the host; no gradient flows through any of it."""
import math

import numpy as np
import torch

from . import lib as L
from .lib import lib, check, ptr, stream

NO_IGNORE = -2 ** 31            # the ignore value no uint8 target and no class index equals (ops.MultiLossFn.NO_IGNORE)
MAX_PIXELS = 2 ** 31 - 1
SPEC_KEYS = ('keep', 'min_kept', 'thresh')


def selection(keep=None, min_kept=0, thresh=None):
    """The checked selection rule as the C ABI takes it: (keep as a float, 0.0 for None; min_kept as an int; the cap -logf(thresh) in float32,
    +inf for None).  keep lies in (0, 1], thresh in (0, 1), min_kept is a non-negative integer, and at least one of keep and thresh is
    given.  ValueError otherwise."""
    if keep is None and thresh is None:
        raise ValueError('hard mining needs keep (a fraction in (0, 1]) or thresh (a probability in (0, 1)), or both')
    k = 0.0
    if keep is not None:
        if isinstance(keep, bool) or not isinstance(keep, (int, float, np.floating, np.integer)) or not 0.0 < float(keep) <= 1.0:
            raise ValueError('keep must be a fraction in (0, 1], got %r' % (keep,))
        k = float(keep)
    cap = float('inf')
    if thresh is not None:
        if isinstance(thresh, bool) or not isinstance(thresh, (int, float, np.floating, np.integer)) or not 0.0 < float(thresh) < 1.0:
            raise ValueError('thresh must be a probability in (0, 1), got %r' % (thresh,))
        cap = float(-np.log(np.float32(thresh)))
        if not cap > 0.0:                   # a threshold that rounds to 1.0f
            raise ValueError('thresh must be a probability in (0, 1) in float32, got %r' % (thresh,))
    if isinstance(min_kept, bool) or not isinstance(min_kept, (int, np.integer)) or not 0 <= int(min_kept) < 2 ** 63:
        raise ValueError('min_kept must be a non-negative integer, got %r' % (min_kept,))
    return k, int(min_kept), cap


def check_spec(spec):
    """A hard_mining setting -- None, or a dict with the optional keys 'keep', 'min_kept', 'thresh' -- checked and returned as a fresh dict
    of exactly those it holds (None stays None).  ValueError otherwise."""
    if spec is None:
        return None
    if not isinstance(spec, dict) or not set(spec) <= set(SPEC_KEYS):
        raise ValueError("hard_mining is None or a dict with the optional keys 'keep', 'min_kept', 'thresh', got %r" % (spec,))
    selection(spec.get('keep'), spec.get('min_kept', 0), spec.get('thresh'))
    return dict(spec)


def _ignore(ignore_index):
    if ignore_index is None:
        return NO_IGNORE
    if isinstance(ignore_index, bool) or int(ignore_index) != ignore_index or not -2 ** 31 <= int(ignore_index) < 2 ** 31:
        raise ValueError('ignore_index must be an int that fits 32 bits, got %r' % (ignore_index,))
    return int(ignore_index)


def _logits_args(logits, target, pixel_weights):
    """The checked inputs of the two logits entry points: (x, pitch, target, pixel_weights, b, c, h, w)."""
    from . import ops
    if not torch.is_tensor(logits) or logits.dim() != 4:
        raise ValueError('expected [B,C,H,W] logits, got %s' % (tuple(logits.shape) if torch.is_tensor(logits) else type(logits),))
    b, c, h, w = logits.shape
    if not 2 <= c <= 16:
        raise ValueError('n_classes=%d unsupported (2..16)' % c)
    if not 1 <= b * h * w <= MAX_PIXELS:
        raise ValueError('the logits hold %d pixels (1..2^31-1)' % (b * h * w))
    if not torch.is_tensor(target) or target.dtype not in (torch.uint8, torch.int64) or tuple(target.shape) != (b, h, w):
        raise ValueError('target must be uint8 or int64 [B,H,W] matching the logits %s, got %s' % (
            (b, h, w), (target.dtype, tuple(target.shape)) if torch.is_tensor(target) else type(target)))
    if target.device != logits.device:
        raise ValueError('logits and target must be on the same device. Got: {} and {}'.format(logits.device, target.device))
    if pixel_weights is not None:
        if (not torch.is_tensor(pixel_weights) or pixel_weights.dtype != torch.float32 or tuple(pixel_weights.shape) != (b, h, w)
                or pixel_weights.device != logits.device):
            raise ValueError('pixel_weights must be float32 [B,H,W] matching the logits, on their device')
        pixel_weights = pixel_weights.detach().contiguous()
    ptr(logits)                              # a host tensor is refused here, before anything is initialised
    L.init()
    x = ops.as_nhwc(logits.detach())
    return x, ops.pitch_of(x), target.contiguous(), pixel_weights, b, c, h, w


def _workspace(n, device):
    return torch.empty(lib.pylc_mining_workspace_bytes(n), device=device, dtype=torch.uint8)


def pixel_nll(logits, target, ignore_index=None, pixel_weights=None):
    """The loss map of a batch of logits [B,C,H,W] (NHWC memory, any pitch, detached) in one launch: float32 [B,H,W] with nll = -log p_t at
    candidates and NaN rows, -1 at ignored pixels and pixels of weight 0, -2 at bad pixels (a target outside 0..C-1 that is not
    ignore_index; a negative, NaN or infinite weight on a valid target).  target: uint8 or int64 [B,H,W]."""
    ign = _ignore(ignore_index)
    x, pitch, target, pw, b, c, h, w = _logits_args(logits, target, pixel_weights)
    out = torch.empty((b, h, w), device=x.device, dtype=torch.float32)
    check(lib.pylc_pixel_nll(ptr(x), pitch, ptr(target), target.element_size(), b * h * w, c, ign, ptr(pw), ptr(out), stream()))
    return out


def select(nll, keep=None, min_kept=0, thresh=None, pixel_weights=None):
    """The selection alone, from a loss map that exists (float32, any shape; what pixel_nll returns, or any map of non-negative scores with
    -1 for 'leave out' and -2 / NaN for 'pass through'): (weights, info), weights float32 of the map's shape."""
    k, mk, cap = selection(keep, min_kept, thresh)
    if not torch.is_tensor(nll) or nll.dtype != torch.float32 or not 1 <= nll.numel() <= MAX_PIXELS:
        raise ValueError('nll must be a float32 tensor of 1..2^31-1 entries')
    if pixel_weights is not None:
        if (not torch.is_tensor(pixel_weights) or pixel_weights.dtype != torch.float32 or pixel_weights.shape != nll.shape
                or pixel_weights.device != nll.device):
            raise ValueError('pixel_weights must be float32 of the map\'s shape %s, on its device' % (tuple(nll.shape),))
        pixel_weights = pixel_weights.detach().contiguous()
    ptr(nll)
    L.init()
    nll = nll.detach().contiguous()
    n = nll.numel()
    out = torch.empty_like(nll)
    info = torch.empty(4, device=nll.device, dtype=torch.int64)
    ws = _workspace(n, nll.device)
    check(lib.pylc_hard_select(ptr(nll), n, ptr(pixel_weights), k, mk, cap, ptr(out), ptr(info), ptr(ws), stream()))
    return out, info


def hard_pixel_weights(logits, target, keep=None, min_kept=0, thresh=None, ignore_index=None, pixel_weights=None, return_nll=False):
    """pixel_nll and select fused -- the kernel that computes the loss map takes the first histogram; four launches and one memset:
    (weights, info), and the map with return_nll.  Bit for bit what the two calls give."""
    k, mk, cap = selection(keep, min_kept, thresh)
    ign = _ignore(ignore_index)
    x, pitch, target, pw, b, c, h, w = _logits_args(logits, target, pixel_weights)
    n = b * h * w
    out = torch.empty((b, h, w), device=x.device, dtype=torch.float32)
    nll = torch.empty((b, h, w), device=x.device, dtype=torch.float32) if return_nll else None
    info = torch.empty(4, device=x.device, dtype=torch.int64)
    ws = _workspace(n, x.device)
    check(lib.pylc_hard_pixel_weights(ptr(x), pitch, ptr(target), target.element_size(), n, c, ign, ptr(pw), k, mk, cap, ptr(nll), ptr(out),
                                      ptr(info), ptr(ws), stream()))
    return (out, info, nll) if return_nll else (out, info)


def expected_k(n_valid, keep=None, min_kept=0):
    """k as the device computes it, in Python floats (IEEE double product, ceil)."""
    return min(int(n_valid), max(int(min_kept), int(math.ceil((0.0 if keep is None else float(keep)) * int(n_valid)))))
