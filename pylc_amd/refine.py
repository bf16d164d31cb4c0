"""Edge-aware refinement of class probabilities: the guided filter (He, Sun, Tang, PAMI 2013) of a probability volume, guided by the
photograph's luma, on the device (csrc/refine.hip; the reference has nothing of the kind).

The networks predict at output stride 4..16 and upsample: their class borders are smooth and sit a few pixels off the image's edges.
The filter regresses every class's probability on the image intensity inside a (2*radius+1)^2 window (stage 1: coefficients a_c, b_c
per pixel) and averages the regressions that cover a pixel (stage 2: q_c = mean(a_c) * g + mean(b_c)); class borders move onto the
intensity edges, flat regions take the window mean.  `eps`, in units of the guide scaled to [0, 1], decides what counts as an edge: an
intensity step well above sqrt(eps) is kept, texture below it is smoothed over.  Windows are clipped to the image (He et al.'s
boxfilter / N); a window whose guide is constant has a_c = 0 exactly, whatever eps.

The output is again mask / probs / confidence, so the sieve, PhotoEvaluator, calibration and the soft-target loop take it unchanged.
The raw q is linear in p and sums to 1 over the classes wherever p does; next to strong edges it can leave [0, 1] by a few hundredths,
which clip=True (default) removes from the returned volume (the mask is always the argmax of the raw q).

Memory: the coefficients a, b are two fp32 [C,H,W] volumes beside the input, 2 * 4 * C * H * W bytes -- 0.9 GB on a 3072 x 4096
photograph with 9 classes, next to the 0.45 GB volume itself (the ensemble's note in inference.predict_blend_mean counts the rest).
No autograd: like the sieve this is post-processing."""
import torch

from . import lib as L
from .lib import lib, check, ptr, stream

MAX_RADIUS = 64
EPS_RANGE = (1e-6, 1.0)
SPEC_KEYS = ('radius', 'eps', 'clip')


def check_spec(refine):
    """A refine spec -> (radius, eps, clip).  The spec is a dict with 'radius' (int 1..64) and 'eps' (float in [1e-6, 1]) and an optional
    'clip' (bool, default True).  ValueError, with the offending value, for anything else."""
    if not isinstance(refine, dict):
        raise ValueError("refine is None or a dict {'radius': 8, 'eps': 1e-3[, 'clip': True]}, got %r" % (refine,))
    unknown = sorted(k for k in refine if k not in SPEC_KEYS)
    if unknown:
        raise ValueError('refine: unknown key %r (keys: %s)' % (unknown[0], ', '.join(SPEC_KEYS)))
    for k in ('radius', 'eps'):
        if k not in refine:
            raise ValueError('refine needs %r, got %r' % (k, refine))
    clip = refine.get('clip', True)
    if not isinstance(clip, bool):
        raise ValueError("refine['clip'] is True or False, got %r" % (clip,))
    return _check_radius(refine['radius']), _check_eps(refine['eps']), clip


def _check_radius(radius):
    if isinstance(radius, bool) or not isinstance(radius, int) or not 1 <= radius <= MAX_RADIUS:
        raise ValueError('radius is an int in [1, %d], got %r' % (MAX_RADIUS, radius))
    return radius


def _check_eps(eps):
    if isinstance(eps, bool) or not isinstance(eps, (int, float)) or not EPS_RANGE[0] <= eps <= EPS_RANGE[1]:
        raise ValueError('eps is a number in [%g, %g] (units of the guide scaled to [0, 1]), got %r' % (EPS_RANGE[0], EPS_RANGE[1], eps))
    return float(eps)


def _check_image(image):
    if not torch.is_tensor(image) or image.dtype != torch.uint8:
        raise ValueError('the guide image must be a uint8 tensor, got %s' % (image.dtype if torch.is_tensor(image) else type(image).__name__))
    if image.dim() != 3 or image.shape[0] not in (1, 3) or image.numel() == 0:
        raise ValueError('an image must be [ch,H,W] with ch 1 or 3 and at least one pixel, got %s' % (tuple(image.shape),))
    if image.shape[1] * image.shape[2] >= 2 ** 31:
        raise ValueError('an image must have fewer than 2^31 pixels, got %s' % (tuple(image.shape),))


def _check_probs(probs):
    if not torch.is_tensor(probs) or probs.dtype != torch.float32:
        raise ValueError('probs must be a float32 tensor, got %s' % (probs.dtype if torch.is_tensor(probs) else type(probs).__name__))
    if probs.dim() != 3 or probs.numel() == 0:
        raise ValueError('probs must be [C,H,W] with at least one pixel, got %s' % (tuple(probs.shape),))
    if not 2 <= probs.shape[0] <= 16:
        raise ValueError('probs has %d classes (2..16)' % probs.shape[0])
    if probs.shape[1] * probs.shape[2] >= 2 ** 31:
        raise ValueError('probs must have fewer than 2^31 pixels per class, got %s' % (tuple(probs.shape),))


def _check_guide(guide, h, w):
    """the guide of an [.,h,w] volume: an [h,w] uint8 luma, or a [ch,h,w] uint8 image whose luma is taken"""
    if torch.is_tensor(guide) and guide.dim() == 3:
        _check_image(guide)
    elif not torch.is_tensor(guide) or guide.dtype != torch.uint8 or guide.dim() != 2:
        raise ValueError('the guide must be a uint8 [H,W] luma or a uint8 [ch,H,W] image, got %s'
                         % ('%s %s' % (guide.dtype, tuple(guide.shape)) if torch.is_tensor(guide) else type(guide).__name__))
    if tuple(guide.shape[-2:]) != (h, w):
        raise ValueError('the guide is %dx%d, the probabilities are %dx%d' % (guide.shape[-2], guide.shape[-1], h, w))


def _on_device(t, what):
    if not t.is_cuda:
        raise ValueError('%s must be on the HIP device (got %s); there is no CPU fallback' % (what, t.device))
    return t


def _strided(probs):
    """probs as the kernel reads it: (tensor, plane stride, row pitch) in elements -- a view with unit stride along x, a row pitch >= W
    and a plane stride of at least one plane (a window of a larger volume) is read in place, anything else through one contiguous copy"""
    c, h, w = probs.shape
    sc, sy, sx = probs.stride()
    if sx == 1 and sy >= w and sc >= (h - 1) * sy + w:
        return probs, sc, sy
    probs = probs.contiguous()
    return probs, h * w, w


def luma(image):
    """Device uint8 [ch,H,W], ch 1 or 3 -> uint8 [H,W]: (77 R + 150 G + 29 B + 128) >> 8; a 1-channel image is its own guide (a copy)."""
    _check_image(image)
    image = _on_device(image, 'an image').contiguous()
    L.init()
    ch, h, w = image.shape
    out = torch.empty((h, w), device=image.device, dtype=torch.uint8)
    check(lib.pylc_luma_u8(ptr(image), ch, h, w, ptr(out), stream()))
    return out


def _guide_of(guide):
    return luma(guide) if guide.dim() == 3 else _on_device(guide, 'the guide').contiguous()


def _coeffs(probs, g, radius, eps):
    c, h, w = probs.shape
    probs, plane, pitch = _strided(probs)
    a = torch.empty((c, h, w), device=probs.device)
    b = torch.empty((c, h, w), device=probs.device)
    check(lib.pylc_guided_coeffs(ptr(probs), plane, pitch, ptr(g), c, h, w, radius, eps, ptr(a), ptr(b), stream()))
    return a, b


def guided_coeffs(probs, guide, radius, eps):
    """Stage 1: device float32 [C,H,W] probabilities (a strided window view is read in place) and a guide (uint8 [H,W] luma or uint8
    [ch,H,W] image) -> the regression coefficients (a, b), float32 [C,H,W] each."""
    radius, eps = _check_radius(radius), _check_eps(eps)
    _check_probs(probs)
    _check_guide(guide, probs.shape[1], probs.shape[2])
    _on_device(probs, 'probs')
    _on_device(guide, 'the guide')
    L.init()
    return _coeffs(probs, _guide_of(guide), radius, eps)


def guided_refine(probs, guide, radius=8, eps=1e-3, return_probs=False, return_confidence=False, clip=True):
    """The guided filter of a probability volume: device float32 [C,H,W] and a guide (uint8 [H,W] luma, or a uint8 [ch,H,W] image whose
    luma is taken) -> the uint8 mask [H,W] (first maximum of the raw q), or the tuple (mask[, probs][, conf]) in that order: probs
    float32 [C,H,W] (clamped to [0, 1] with clip=True, raw with clip=False), conf float32 [H,W] the maximum clamped to [0, 1].  Two
    launches (three with an image guide); without return_probs no refined volume is written.  All argument errors come before any launch."""
    radius, eps = _check_radius(radius), _check_eps(eps)
    if not isinstance(clip, bool):
        raise ValueError('clip is True or False, got %r' % (clip,))
    _check_probs(probs)
    _check_guide(guide, probs.shape[1], probs.shape[2])
    _on_device(probs, 'probs')
    _on_device(guide, 'the guide')
    L.init()
    g = _guide_of(guide)
    c, h, w = probs.shape
    a, b = _coeffs(probs, g, radius, eps)
    mask = torch.empty((h, w), device=probs.device, dtype=torch.uint8)
    out = torch.empty((c, h, w), device=probs.device) if return_probs else None
    conf = torch.empty((h, w), device=probs.device) if return_confidence else None
    check(lib.pylc_guided_apply(ptr(a), ptr(b), ptr(g), c, h, w, radius, int(clip), ptr(mask), ptr(out), ptr(conf), stream()))
    res = (mask,) + ((out,) if return_probs else ()) + ((conf,) if return_confidence else ())
    return res if len(res) > 1 else mask
