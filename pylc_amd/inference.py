"""Sliding-window inference over a full-resolution (already fitted) image, entirely on the GPU.

Counterpart of the reference's test path, test.py:50-110: Extractor(...).extract(fit=True, stride=tile//2)
(utils/extract.py:106-231, :279-310) -> Model.test per batch of 8 tiles (test.py:69,81-84) -> utils.reconstruct
(utils/tools.py:209-319) -> colourize + resize.  The reference moves every logit tile to the host and stitches in numpy;
here tiles are cut (and normalised) straight from the device image, logits stay in HBM, and one kernel blends the
overlaps and takes the argmax, so only the uint8 class mask (1 byte per pixel) ever needs to leave the GPU.

Reading the image file stays with the caller; resizing a photograph to a multiple of the tile size (utils/tools.py:77-206) and the
steps after the stitch are pylc_amd.photo (segment_photo); the functions here take the fitted image.

A U-Net of valid convolutions returns the centred (tile - 2*pad)^2 square of its window, which reconstruct() cannot stitch; its
images take the overlap-tile path instead (predict_overlap_tile, csrc/overlap_tile.hip): mirror-padded windows around output tiles
that cover the image exactly, at any image size, blended by the mean of the tiles' softmax probabilities."""
import contextlib
import ctypes as C

import numpy as np
import torch
import torch.distributed as dist

from . import ops, lib as L
from .lib import lib, check, ptr, stream
from .runtime import runtime


# ---- multi-GPU inference: replicas, no data-path collective except the final gather (SURVEY.md section 8e "Inference") ------------
def shard_batches(n_tiles, batch, rank, world):
    """Tile batches of one image dealt round-robin over the ranks (test.py:69-84 walks them serially): the (first tile, count)
    pairs this rank runs, in order."""
    starts = list(range(0, n_tiles, batch))
    return [(k, min(batch, n_tiles - k)) for i, k in enumerate(starts) if i % world == rank]


def gather_tiles(local, n_tiles, batch, group, dst=0):
    """Collect the per-rank logit tiles on rank `dst`.  local: [n_local_tiles, ...] in the order of shard_batches().  Every rank
    contributes one equally sized slab (the collective needs equal shapes: short shards are zero-padded), rank dst puts the tiles
    back into image order.  Returns [n_tiles, ...] on dst, None elsewhere."""
    world, rank = dist.get_world_size(group), dist.get_rank(group)
    counts = [sum(c for _, c in shard_batches(n_tiles, batch, r, world)) for r in range(world)]
    slab = local.new_zeros((max(counts),) + tuple(local.shape[1:]))
    slab[:local.shape[0]] = local
    parts = [torch.empty_like(slab) for _ in range(world)] if rank == dst else None
    dist.gather(slab, parts, dst=dst, group=group)
    if rank != dst:
        return None
    out = local.new_empty((n_tiles,) + tuple(local.shape[1:]))
    for r in range(world):
        pos = 0
        for k, c in shard_batches(n_tiles, batch, r, world):
            out[k:k + c] = parts[r][pos:pos + c]
            pos += c
    return out


def tile_grid(h, w, tile, stride):
    if h < tile or w < tile or (h - tile) % stride or (w - tile) % stride:
        raise ValueError('image %dx%d is not fitted to tile %d / stride %d (utils/tools.py:151-206 adjust_to_tile)' % (h, w, tile, stride))
    return (h - tile) // stride + 1, (w - tile) // stride + 1


# ---- the one driver: an image prepared for a model, the network's eval mode, this rank's tile batches through the network ------------
class _TileRun:
    """What every full-image path prepares from (model, image) before its first tile: the image on the model's device (uint8 stays
    uint8 -- a photograph: a quarter of the bytes to upload, normalised straight from them -- everything else goes to float32), the
    channel check, the normalisation statistics as the cutter takes them, the class count and its NHWC pitch, and this process's place
    in `group` (world 1, rank 0 without one)."""

    def __init__(self, model, image, group):
        self.model, self.dev = model, model.device
        u8 = image.dtype == torch.uint8
        self.img = image.to(self.dev, dtype=torch.uint8 if u8 else torch.float32).contiguous()
        if self.img.shape[0] != model.meta.ch:
            raise ValueError('model expects %d-channel images' % model.meta.ch)
        self.h, self.w = self.img.shape[1:]
        mean, std, denom = model._stats(model.meta.normalize_default)
        if denom != 255.0:              # the tile cutter divides by 255: fold the grayscale-defaults branch's missing division into std
            std = [v * denom / 255.0 for v in std]
        self.mean = (C.c_float * 3)(*[float(v) for v in mean])
        self.std = (C.c_float * 3)(*[float(v) for v in std])
        self.ncls = model.meta.n_classes
        self.cp = (self.ncls + 3) & ~3
        self.world = dist.get_world_size(group) if group is not None else 1
        self.rank = dist.get_rank(group) if group is not None else 0

    def mine(self, n_tiles, batch):
        """this rank's (first tile, count) batches of an image of n_tiles"""
        return shard_batches(n_tiles, batch, self.rank, self.world)

    def batches(self, mine, tile, out, stride, member=0, img=None):
        """For each (first tile, count) of `mine`: the windows cut from the image (or from `img`, another size of it) by the any-size
        cutter -- the fitted grid is its case out == tile on a fitted image -- mirrored along x for member 1, through the network.
        Yields (first tile, count, the network's output).  Call under _eval_mode."""
        img = self.img if img is None else img
        cimg, h, w = img.shape
        for k, b in mine:
            x4 = ops.empty_nhwc(b, 4, tile, tile, self.dev)
            check(lib.pylc_image_pack_tiles_reflect_ex(ptr(img), int(img.dtype == torch.uint8), cimg, h, w, tile, out, stride, k, b, self.mean,
                                                       self.std, ptr(x4), stream(), member))
            yield k, b, self.model.net(x4)


@contextlib.contextmanager
def _eval_mode(model):
    """The network in eval mode with current weight ranges and prepared filter planes (optim.refresh_if_changed has the reason), no
    autograd; its mode comes back whatever happens inside."""
    was_training = model.net.training
    model.net.eval()
    try:
        model._refresh_for_inference()
        with torch.no_grad():
            yield
    finally:
        model.net.train(was_training)


def predict_image(model, image, tile=512, stride=None, batch=8, group=None, blend='reference', flip=False, return_probs=False,
                  return_confidence=False, scales=None, scale_weights=None, temperature=None, refine=None, window=None):
    """image: [C,H,W] raw 0..255, uint8 or float (host or device), fitted.  Returns the uint8 class mask [H,W] (device).

    group=None (default): LOCAL -- this process runs every tile and returns the mask, also inside a data-parallel job (a rank-0-only
    validation preview must not hang in a collective).  With an explicit process group the call is a COLLECTIVE that every rank of the
    group must make: the tile batches are dealt round-robin over the ranks -- every rank holds the image and a replica of the model --
    and the logit tiles are gathered to rank 0, which stitches; the other ranks return None.

    blend='reference' (default) is the reference's reconstruct() with its quirks (csrc/stitch.hip); it has no probabilities, so flip,
    return_probs and return_confidence raise ValueError with it.  blend='mean' is the streaming mean-probability blend
    (predict_blend_mean, csrc/blend.hip): image uint8 or float, any H, W >= tile, any stride in [1, tile] (default tile // 2); returns the
    mask, or the tuple (mask[, probs][, conf]) in that order -- probs fp32 [n_classes,H,W], conf fp32 [H,W] its maximum over the classes.
    flip=True adds the horizontally mirrored windows as a second ensemble member.  scales=(0.75, 1.0, 1.25) runs the multi-scale ensemble
    (predict_blend_mean: the image at every scale, the probabilities resampled back and averaged with scale_weights); like flip it needs
    blend='mean'.  temperature (resolve_temperature: None, a positive float, or 'meta' for model.meta.temperature) divides the logits
    before every tile's softmax (pylc_blend_accumulate_t); like flip it needs blend='mean' and composes with flip and scales.
    refine ({'radius': 8, 'eps': 1e-3}, pylc_amd.refine.check_spec) passes the mean probabilities through the guided filter with the uint8
    image's luma as the guide (predict_blend_mean): the mask, probs and conf returned are the refined ones; like flip it
    needs blend='mean'.  window ('hann', 'gauss', ('gauss', sigma_frac), 'uniform' or a table of `tile` positive floats; blend_window,
    DESIGN.md 5.25) weighs every tile's probabilities by a separable window that falls off towards the tile's edge; like flip it needs
    blend='mean', composes with the other keywords, and pays only where tiles overlap (stride < tile).

    A U-Net model (meta.arch == 'unet') takes predict_overlap_tile instead (any image size, stride default tile - 2*pad); its blend
    always was the mean, so `blend` is ignored and the other keywords pass through."""
    if blend not in ('reference', 'mean'):
        raise ValueError("blend is 'reference' or 'mean', got %r" % (blend,))
    if model.meta.arch == 'unet':
        return predict_overlap_tile(model, image, tile, stride, batch, group, return_probs, flip, return_confidence, scales, scale_weights,
                                    temperature, refine, window)
    if blend == 'mean':
        return predict_blend_mean(model, image, tile, tile, stride, batch, group, flip, return_probs, return_confidence, scales, scale_weights,
                                  temperature, refine, window)
    asked = [k for k, v in (('flip', flip), ('return_probs', return_probs), ('return_confidence', return_confidence),
                            ('scales', scales is not None), ('scale_weights', scale_weights is not None),
                            ('temperature', temperature is not None), ('refine', refine is not None), ('window', window is not None)) if v]
    if asked:
        raise ValueError("%s needs blend='mean': the reference stitch mixes logits and probabilities, its scores are not probabilities"
                         % ', '.join(asked))
    L.init()
    stride = tile // 2 if stride is None else stride          # test.py:63
    run = _TileRun(model, image, group)
    rows, cols = tile_grid(run.h, run.w, tile, stride)
    n, cp = rows * cols, run.cp
    mine = run.mine(n, batch)
    logits = torch.empty((sum(c for _, c in mine), tile, tile, cp), device=run.dev)
    with _eval_mode(model):
        pos = 0
        for _, b, y in run.batches(mine, tile, tile, stride):  # [b, ncls, tile', tile'] NHWC memory, pitch cp
            if y.shape[2] != tile or y.shape[3] != tile:
                raise ValueError('sliding-window stitching needs a same-size network (DeepLab); got %s' % (tuple(y.shape),))
            p = ops.pitch_of(y)
            logits[pos:pos + b].copy_(torch.as_strided(y, (b, tile, tile, cp), (tile * tile * p, tile * p, p, 1), y.storage_offset()))
            pos += b
    if run.world > 1:
        logits = gather_tiles(logits, n, batch, group)
        if logits is None:
            return None
    mask = torch.empty((run.h, run.w), device=run.dev, dtype=torch.uint8)
    check(lib.pylc_stitch_argmax(ptr(logits), cp, rows, cols, tile, stride, run.ncls, ptr(mask), stream()))
    return mask


def stitch_logits(logits_tiles, rows, cols, tile, stride):
    """[n, C, tile, tile] logits (any layout, device) -> uint8 class mask, reconstruct() semantics."""
    L.init()
    n, c = logits_tiles.shape[:2]
    cp = (c + 3) & ~3
    buf = torch.zeros((n, tile, tile, cp), device=logits_tiles.device)
    buf[..., :c] = logits_tiles.permute(0, 2, 3, 1)
    mask = torch.empty((rows * stride + tile - stride, cols * stride + tile - stride), device=buf.device, dtype=torch.uint8)
    check(lib.pylc_stitch_argmax(ptr(buf), cp, rows, cols, tile, stride, c, ptr(mask), stream()))
    return mask


# ---- overlap tiles for the valid-convolution U-Net (config.py:225-236: input_size 512, output_size 324, mirror padding) -------------
def overlap_tile_grid(h, w, out, stride, pad=0):
    """Output-tile origins (row_origins, col_origins) of an h x w image: o_i = min(i*stride, n - out) for i = 0 .. ceil((n - out) /
    stride) along an axis of length n -- the last tile moved back to end at the image edge.  Tile (i, j) covers [o_i, o_i + out) x
    [o_j, o_j + out) and reads the input window `pad` wider on every side, mirrored (reflect-101) beyond the image."""
    if stride < 1:
        raise ValueError('overlap tiles: stride %d < 1' % stride)
    if stride > out:
        raise ValueError('overlap tiles: stride %d > output tile %d would leave pixels uncovered (need stride <= out)' % (stride, out))
    if h < out or w < out:
        raise ValueError('overlap tiles: image %dx%d is smaller than the output tile %d (need H, W >= out)' % (h, w, out))
    if pad >= h or pad >= w:
        raise ValueError('overlap tiles: pad %d >= image side of %dx%d (need pad < H and pad < W: one mirror reflection)' % (pad, h, w))

    def axis(n):
        return [min(i * stride, n - out) for i in range(-(-(n - out) // stride) + 1)]
    return axis(h), axis(w)


def overlap_tile_out(net, tile, pad):
    """Output tile side out = tile - 2*pad, checked against what the U-Net returns for a `tile` window (UNet.output_size): only
    then does the output sit centred in its window, at offset pad (512 -> 324 and 256 -> 68 pass, 572 -> 388 and 252 -> 68 do not)."""
    out = tile - 2 * pad
    got = net.output_size(tile)
    if got != out:
        raise ValueError('overlap tiles: a %d px window gives a %d px U-Net output, not tile - 2*pad = %d (pad %d): the output would not be '
                         'centred in its window' % (tile, got, out, pad))
    return out


def predict_overlap_tile(model, image, tile=512, stride=None, batch=8, group=None, return_probs=False, flip=False, return_confidence=False,
                         scales=None, scale_weights=None, temperature=None, refine=None, window=None):
    """Full-image U-Net inference by overlap tiles.  image: [C,H,W] raw 0..255, uint8 or float, host or device, any H, W >= out
    (out = tile - 2*meta.pad_size; no fitting).  stride in [1, out], default out.  Returns the uint8 class mask [H,W] (device), or
    (mask, probs) with probs the fp32 mean softmax probabilities [n_classes,H,W] when return_probs.

    The mirrored windows are cut and normalised on the device (predict_image's statistics), run through model.net in eval mode in
    batches of `batch`, and every logit tile stays in HBM until one kernel blends them: each pixel's class scores are the mean of the
    softmax probabilities of the tiles covering it, its class their argmax.  `group`: predict_image's contract (batches dealt over the
    ranks, logit tiles gathered to rank 0, which stitches and returns; the other ranks return None).

    flip=True (the mirrored windows as a second ensemble member), return_confidence=True (the tuple grows by conf, fp32 [H,W], the
    maximum probability) or scales (the multi-scale ensemble) move the call to the streaming accumulator, predict_blend_mean; without
    them it is the one-launch stitch.  So do temperature, refine and window (predict_image's keywords; the window table has `out`
    entries and pays with stride < out)."""
    if model.meta.arch != 'unet':
        raise ValueError('predict_overlap_tile needs a U-Net (meta.arch == "unet"), got %r' % model.meta.arch)
    if window is not None:
        window_table(window, tile - 2 * model.meta.pad_size)          # argument errors before the device is touched
    L.init()
    pad = model.meta.pad_size
    out = overlap_tile_out(model.net, tile, pad)
    if (flip or return_confidence or scales is not None or scale_weights is not None or temperature is not None or refine is not None
            or window is not None):
        return predict_blend_mean(model, image, tile, out, stride, batch, group, flip, return_probs, return_confidence, scales, scale_weights,
                                  temperature, refine, window)
    stride = out if stride is None else int(stride)
    run = _TileRun(model, image, group)
    row_o, col_o = overlap_tile_grid(run.h, run.w, out, stride, pad)
    n, cp, ncls = len(row_o) * len(col_o), run.cp, run.ncls
    mine = run.mine(n, batch)
    logits = torch.empty((sum(c for _, c in mine), out, out, cp), device=run.dev)
    with _eval_mode(model):
        pos = 0
        for _, b, y in run.batches(mine, tile, out, stride):
            logits[pos:pos + b, :, :, :ncls].copy_(ops.as_nhwc(y).permute(0, 2, 3, 1))     # [b, ncls, out, out], NHWC memory
            pos += b
    if run.world > 1:
        logits = gather_tiles(logits, n, batch, group)
        if logits is None:
            return None
    return _stitch_overlap(logits, cp, n, run.h, run.w, out, stride, ncls, return_probs)


SCALE_RANGE = (0.5, 2.0)    # where the plain bilinear resize still reads every source pixel (no area prefilter)


def scaled_size(n, s):
    """The length of an axis of n pixels at scale s, rounded half up: int(n * s + 0.5)."""
    return int(n * s + 0.5)


def resize_image(image, oh, ow):
    """[C,H,W] raw image, uint8 or float, C 1 or 3 (host or device) -> float32 device [C,oh,ow] by half-pixel-centre bilinear
    interpolation without antialiasing (pylc_resize_bilinear_image: F.interpolate(mode='bilinear', align_corners=False) with double
    coordinates), the resize of the published multi-scale protocol.  Any ratio; below 1/2 it skips source pixels."""
    L.init()
    dev = image.device if image.is_cuda else torch.device('cuda')
    u8 = image.dtype == torch.uint8
    img = image.to(dev, dtype=torch.uint8 if u8 else torch.float32).contiguous()
    if img.dim() != 3 or img.shape[0] not in (1, 3):
        raise ValueError('resize_image needs a [C,H,W] image of 1 or 3 channels, got %s' % (tuple(img.shape),))
    if oh < 1 or ow < 1:
        raise ValueError('resize_image: output size %dx%d' % (oh, ow))
    cimg, h, w = img.shape
    out = torch.empty((cimg, int(oh), int(ow)), device=dev)
    check(lib.pylc_resize_bilinear_image(ptr(img), int(u8), cimg, h, w, ptr(out), int(oh), int(ow), stream()))
    return out


def ensemble_plan(scales, scale_weights, h, w, out):
    """The multi-scale ensemble's members for an h x w image and output tile `out`: [(scale, scaled h, scaled w, weight)] in the order
    given.  ValueError for an empty sequence, a scale outside SCALE_RANGE, weights of another length or not positive, and a scale at
    which a side falls below the output tile."""
    scales = [float(s) for s in scales]
    if not scales:
        raise ValueError('scales is empty: give at least one scale, or None for the single-scale blend')
    weights = [1.0] * len(scales) if scale_weights is None else [float(v) for v in scale_weights]
    if len(weights) != len(scales):
        raise ValueError('scale_weights has %d entries for %d scales' % (len(weights), len(scales)))
    plan = []
    for s, wgt in zip(scales, weights):
        if not SCALE_RANGE[0] <= s <= SCALE_RANGE[1]:
            raise ValueError('scale %r outside [%g, %g]: the bilinear resize has no area prefilter' % (s, SCALE_RANGE[0], SCALE_RANGE[1]))
        if not 0.0 < wgt < float('inf'):
            raise ValueError('scale weight %r for scale %r is not a positive number' % (wgt, s))
        hs, ws = scaled_size(h, s), scaled_size(w, s)
        if hs < out or ws < out:
            raise ValueError('scale %r takes the %dx%d image to %dx%d, below the output tile %d (need H, W >= out at every scale)'
                             % (s, h, w, hs, ws, out))
        plan.append((s, hs, ws, wgt))
    return plan


def resolve_temperature(model, temperature):
    """The inference keyword `temperature` as an inverse temperature: None stays None (the plain entry point), a positive finite number T
    gives 1 / T, 'meta' takes model.meta.temperature and raises ValueError when no validation pass has stored one."""
    if temperature is None:
        return None
    if isinstance(temperature, str):
        if temperature != 'meta':
            raise ValueError("temperature is None, a positive number or 'meta', got %r" % (temperature,))
        temperature = getattr(model.meta, 'temperature', None)
        if temperature is None:
            raise ValueError("temperature='meta', but model.meta.temperature is unset: train with calibration_bins, or pass a number")
    t = float(temperature)
    if not (t > 0.0 and t != float('inf')):
        raise ValueError('temperature must be a positive finite number, got %r' % (temperature,))
    return 1.0 / t


WINDOW_MIN_RATIO = 2.0 ** -20       # min / max of a window table: below it a tile's edge has no say and fp32 sums lose the small terms
_window_cache = {}


def window_table(spec, out):
    """The window `spec` as a host float32 numpy table [out], validated; needs no device.  Named windows are built in float64 and rounded
    once: 'uniform' all ones; 'hann' 0.5 - 0.5*cos(2*pi*(i + 0.5)/out), the half-sample offset keeping every entry positive; 'gauss' or
    ('gauss', sigma_frac) exp(-0.5*((i - (out - 1)/2)/(sigma_frac*out))**2), sigma_frac default 0.125 (nnU-Net's and MONAI's).  A 1-D
    tensor or array of `out` floats is taken as given.  ValueError for an unknown name, a sigma_frac that is not positive and finite, a
    wrong length, a non-finite or non-positive entry, or min / max < 2**-20."""
    out = int(out)
    if out < 1:
        raise ValueError('window: output tile %d < 1' % out)
    name, sigma = spec, None
    if isinstance(spec, (tuple, list)) and len(spec) > 0 and isinstance(spec[0], str):
        if len(spec) != 2 or spec[0] != 'gauss':
            raise ValueError("window: a named window is 'uniform', 'hann', 'gauss' or ('gauss', sigma_frac), got %r" % (spec,))
        name, sigma = spec
    if isinstance(name, str):
        i = np.arange(out, dtype=np.float64)
        if name == 'uniform' and sigma is None:
            tab = np.ones(out)
        elif name == 'hann' and sigma is None:
            tab = 0.5 - 0.5 * np.cos(2.0 * np.pi * (i + 0.5) / out)
        elif name == 'gauss':
            try:
                sigma = 0.125 if sigma is None else float(sigma)
            except (TypeError, ValueError):
                raise ValueError('window: sigma_frac must be a positive finite number, got %r' % (spec[1],))
            if not (sigma > 0.0 and sigma != float('inf')):
                raise ValueError('window: sigma_frac must be a positive finite number, got %r' % (spec[1],))
            tab = np.exp(-0.5 * ((i - (out - 1) / 2.0) / (sigma * out)) ** 2)
        else:
            raise ValueError("window: a named window is 'uniform', 'hann', 'gauss' or ('gauss', sigma_frac), got %r" % (spec,))
        what = 'window %r at %d entries' % (spec, out)
    else:
        if torch.is_tensor(spec):
            tab = spec.detach().cpu().numpy()
        elif isinstance(spec, (np.ndarray, list, tuple)):
            tab = np.asarray(spec)
        else:
            raise ValueError('window is None, a name, (\'gauss\', sigma_frac) or a 1-D table of floats, got %r' % (type(spec).__name__,))
        if tab.ndim != 1 or tab.shape[0] != out or tab.dtype.kind not in 'fiu':
            raise ValueError('window: a table has one float per pixel of the output tile, [%d]; got %s of %s' % (out, tuple(tab.shape), tab.dtype))
        what = 'window table'
    with np.errstate(over='ignore'):
        tab = np.ascontiguousarray(tab.astype(np.float32))
    if not np.isfinite(tab).all():
        raise ValueError('%s has a non-finite entry' % what)
    if not (tab > 0).all():
        raise ValueError('%s has a non-positive entry (%g): a zero weight divides by zero where it is a pixel\'s only one' % (what, tab.min()))
    if float(tab.min()) / float(tab.max()) < WINDOW_MIN_RATIO:
        raise ValueError('%s: min / max = %g is below 2**-20' % (what, float(tab.min()) / float(tab.max())))
    return tab


def blend_window(spec, out, device):
    """The window of the window-weighted blend as the float32 device table [out] that pylc_blend_accumulate_w and
    pylc_blend_window_sums read.  spec: window_table's -- 'uniform', 'hann', 'gauss', ('gauss', sigma_frac), or a 1-D tensor / array of
    `out` positive floats; its ValueErrors are raised before the device is touched.  Named windows are cached per (spec, out, device)."""
    named = isinstance(spec, str) or (isinstance(spec, (tuple, list)) and len(spec) > 0 and isinstance(spec[0], str))
    key = None
    if named:
        try:
            key = (spec if isinstance(spec, str) else (spec[0],) + tuple(float(v) for v in spec[1:]), int(out), str(torch.device(device)))
        except (TypeError, ValueError):
            key = None                                                  # window_table raises on it
        if key in _window_cache:
            return _window_cache[key]
    tab = torch.from_numpy(window_table(spec, out)).to(device)
    if key is not None:
        _window_cache[key] = tab
    return tab


def _window_sums(win, out, stride, n):
    """pylc_blend_window_sums: the table [n] of an axis of length n"""
    sums = torch.empty((n,), device=win.device)
    check(lib.pylc_blend_window_sums(ptr(win), out, stride, n, ptr(sums), stream()))
    return sums


def _blend_sweep(run, img, tile, out, stride, batch, members, beta=None, win=None):
    """predict_blend_mean's sweep over one device image [C,H,W] (uint8 or float32; run.img or another size of it): this rank's share of
    the tile batches, member-major, into a zeroed accumulation image [H,W,cp], which it returns.  The network is in eval mode already.
    beta: None, or the inverse temperature of pylc_blend_accumulate_t.  win: None, or blend_window's table: pylc_blend_accumulate_w."""
    h, w = img.shape[1:]
    row_o, col_o = overlap_tile_grid(h, w, out, stride, (tile - out) // 2)
    mine = run.mine(len(row_o) * len(col_o), batch)
    ncls, cp = run.ncls, run.cp
    acc = torch.zeros((h, w, cp), device=run.dev)
    for member in range(members):                   # member-major: the sums of member 0 are complete before member 1 adds to them
        for k, b, y in run.batches(mine, tile, out, stride, member, img):
            y = ops.as_nhwc(y)                                  # [b, ncls, out, out], NHWC memory
            if tuple(y.shape[1:]) != (ncls, out, out):
                raise ValueError('the network returned %s for %d px windows, not %d classes of %d px' % (tuple(y.shape), tile, ncls, out))
            p = ops.pitch_of(y)
            if p % 4 or y.data_ptr() % 16:                      # a pitch the 16-byte loads cannot take: one relayout to pitch cp
                y2 = ops.zeros_nhwc(b, ncls, out, out, run.dev, pitch=cp)
                y2.copy_(y)
                y, p = y2, cp
            if win is not None:
                check(lib.pylc_blend_accumulate_w(ptr(y), p, k, b, h, w, out, stride, ncls, member, ptr(acc), cp, ptr(win),
                                                  1.0 if beta is None else beta, stream()))
            elif beta is None:
                check(lib.pylc_blend_accumulate(ptr(y), p, k, b, h, w, out, stride, ncls, member, ptr(acc), cp, stream()))
            else:
                check(lib.pylc_blend_accumulate_t(ptr(y), p, k, b, h, w, out, stride, ncls, member, ptr(acc), cp, stream(), beta))
    return acc


def predict_blend_mean(model, image, tile, out, stride=None, batch=8, group=None, flip=False, return_probs=False, return_confidence=False,
                       scales=None, scale_weights=None, temperature=None, refine=None, window=None):
    """The streaming mean-probability blend (csrc/blend.hip) for a network that maps a `tile` window to its centred `out`
    square (DeepLab: out = tile; U-Net: out = tile - 2*pad).  image: [C,H,W] raw 0..255, uint8 or float, any H, W >= out; stride in
    [1, out], default tile // 2 for a same-size network and out otherwise.

    Windows are cut by pylc_image_pack_tiles_reflect_ex, each batch's logits go straight from the network's output (at its own pitch) into
    pylc_blend_accumulate, which adds their softmax probabilities into one fp32 image [H,W,cp]; pylc_blend_finalize divides by the number
    of covering tiles and members once at the end.  No logit tile outlives its batch.  flip=True runs a second sweep, member-major: all
    tiles unflipped, then all tiles cut and accumulated mirrored.  The tiles are visited in ascending index within and across batches, so
    the result does not depend on `batch`.

    scales (csrc/multiscale.hip): None is the single-scale blend above.  A sequence of floats in [0.5, 2.0] runs the
    multi-scale ensemble, for each scale s in the order given: the image resized to (scaled_size(H, s), scaled_size(W, s)) by
    resize_image (a scale whose size is (H, W) takes the image as it is, in its own dtype); the sweep above, flip included, at that size
    with the same tile and stride; pylc_blend_resample_accumulate, which divides that size's sums by their counts, resamples the
    probabilities bilinearly to H x W and adds scale_weights[k] (default 1.0 each) times them into one ensemble image [H,W,cp]; the
    scaled accumulation image is then freed.  pylc_ensemble_finalize divides by the sum of the weights.  scales=(1.0,) gives the bytes
    of scales=None.  Memory: the ensemble image plus one scaled accumulation image, (1 + s^2) * H*W*cp*4 bytes -- on a 3072 x 4096
    photograph with 9 classes 0.6 + 2.4 GB at s = 2 and 0.6 + 0.94 GB at 1.25.  ValueError for an empty sequence, a scale outside the
    range, weights of another length or not positive, and a scale that takes a side of the image below `out`.

    `group`: every rank accumulates its share of the batches into its own image, dist.all_reduce sums them (results then differ from one
    process's by fp32 summation order only; a one-rank group equals no group bit for bit), rank 0 finalizes, the others return None.
    With scales every rank resamples its own partial sums into its own ensemble image -- the divisor of a pixel is a constant of the
    geometry, so the step is linear -- and one all_reduce of the ensemble image runs at the end.
    temperature: None, a positive number T or 'meta' (resolve_temperature); with one, every tile's term is softmax(logits / T) through
    pylc_blend_accumulate_t, at every member and scale.  T = 1 gives the bytes of None.
    refine: None, or a spec {'radius': 8, 'eps': 1e-3[, 'clip': True]} (pylc_amd.refine.check_spec; csrc/refine.hip).  With
    one the finalizer is asked for the probability volume, and rank 0 passes it through refine.guided_refine with the luma of the image
    the blend ran on (one pylc_luma_u8 launch) as the guide: mask, probs and conf are the refined ones, at every combination of flip,
    scales and temperature.  The image must be uint8 (ValueError otherwise).  Memory: the filter's coefficients are two more volumes the
    size of probs, 2 * 4 * C * H * W bytes -- 0.9 GB on a 3072 x 4096 photograph with 9 classes -- allocated after the accumulation
    images above are done with.  None enters nothing new.
    window: None, or blend_window's spec.  With one, a tile's probabilities count win[ly] * win[lx] times at the pixel at
    (ly, lx) of the placed tile -- the same table for every member and scale -- through pylc_blend_accumulate_w, and the finalizer (with
    scales: every size's resample step) divides by members * sum_y[y] * sum_x[x], two per-axis tables of pylc_blend_window_sums,
    (H + W) * 4 bytes more.  'uniform' gives the bytes of None.  A pixel that one tile covers gets that tile's probabilities back to a
    rounding, so the knob pays only with stride < out; it is not refused otherwise.  flip, temperature, group and refine compose as
    above (the accumulate step stays linear in the per-rank images).  None enters nothing new.
    Returns mask, or (mask[, probs][, conf])."""
    beta = resolve_temperature(model, temperature)                     # before any launch
    if window is not None:
        window_table(window, out)                                      # its errors too
    spec = None
    if refine is not None:
        from . import refine as _refine
        spec = _refine.check_spec(refine)
        if not torch.is_tensor(image) or image.dtype != torch.uint8:
            raise ValueError('refine needs a uint8 image (its luma is the guide), got %s'
                             % (image.dtype if torch.is_tensor(image) else type(image).__name__))
    if stride is None:
        stride = tile // 2 if out == tile else out
    stride = int(stride)
    if scales is None and scale_weights is not None:
        raise ValueError('scale_weights needs scales')
    plan = None if scales is None else ensemble_plan(scales, scale_weights, image.shape[1], image.shape[2], out)    # before any launch
    L.init()
    run = _TileRun(model, image, group)
    img, h, w, ncls, cp = run.img, run.h, run.w, run.ncls, run.cp
    overlap_tile_grid(h, w, out, stride, (tile - out) // 2)            # the geometry's errors before the network's mode is touched
    members = 2 if flip else 1
    win = None if window is None else blend_window(window, out, run.dev)
    acc = ens = None
    with _eval_mode(model):
        if plan is None:
            acc = _blend_sweep(run, img, tile, out, stride, batch, members, beta, win)
        else:
            ens = torch.empty((h, w, cp), device=run.dev)             # the first scale's launch writes every channel below ncls
            for k, (_, hs, ws, wgt) in enumerate(plan):
                acc_s = _blend_sweep(run, img if (hs, ws) == (h, w) else resize_image(img, hs, ws), tile, out, stride, batch, members, beta, win)
                if win is None:
                    check(lib.pylc_blend_resample_accumulate(ptr(acc_s), cp, hs, ws, out, stride, members, wgt, ncls, ptr(ens), cp, h, w,
                                                             int(k > 0), stream()))
                else:
                    sy, sx = _window_sums(win, out, stride, hs), _window_sums(win, out, stride, ws)
                    check(lib.pylc_blend_resample_accumulate_w(ptr(acc_s), cp, hs, ws, members, wgt, ncls, ptr(sy), ptr(sx), ptr(ens), cp, h, w,
                                                               int(k > 0), stream()))
                    del sy, sx
                del acc_s
    if run.world > 1:
        if plan is not None:
            ens[..., ncls:] = 0                                   # the padding channels were never written: keep the collective off garbage
        dist.all_reduce(acc if plan is None else ens, group=group)
        if run.rank != 0:
            return None
    total = None if plan is None else sum(p[3] for p in plan)
    if spec is None:
        return _blend_finalize(acc if plan is None else ens, cp, h, w, out, stride, ncls, members, return_probs, return_confidence, total, win)
    _, probs = _blend_finalize(acc if plan is None else ens, cp, h, w, out, stride, ncls, members, True, False, total, win)
    del acc, ens
    return _refine.guided_refine(probs, img, spec[0], spec[1], return_probs, return_confidence, spec[2])


def _blend_finalize(acc, cp, h, w, out, stride, ncls, members, return_probs, return_confidence, total_weight=None, win=None):
    """mask[, probs][, conf] from a blend's sums (divided by the geometry's counts or, with the window table `win`, by the two axis
    tables of its sums) or, with total_weight, from an ensemble image (the resample step has divided already)"""
    mask = torch.empty((h, w), device=acc.device, dtype=torch.uint8)
    probs = torch.empty((ncls, h, w), device=acc.device) if return_probs else None
    conf = torch.empty((h, w), device=acc.device) if return_confidence else None
    if total_weight is None and win is not None:
        sy, sx = _window_sums(win, out, stride, h), _window_sums(win, out, stride, w)
        check(lib.pylc_blend_finalize_w(ptr(acc), cp, h, w, ncls, members, ptr(sy), ptr(sx), ptr(mask), ptr(probs), ptr(conf), stream()))
    elif total_weight is None:
        check(lib.pylc_blend_finalize(ptr(acc), cp, h, w, out, stride, ncls, members, ptr(mask), ptr(probs), ptr(conf), stream()))
    else:
        check(lib.pylc_ensemble_finalize(ptr(acc), cp, h, w, ncls, total_weight, ptr(mask), ptr(probs), ptr(conf), stream()))
    res = (mask,) + ((probs,) if return_probs else ()) + ((conf,) if return_confidence else ())
    return res if len(res) > 1 else mask


def _stitch_overlap(buf, cp, n, h, w, out, stride, ncls, return_probs):
    mask = torch.empty((h, w), device=buf.device, dtype=torch.uint8)
    probs = torch.empty((ncls, h, w), device=buf.device) if return_probs else None
    check(lib.pylc_stitch_overlap_argmax(ptr(buf), cp, n, h, w, out, stride, ncls, ptr(mask), ptr(probs), stream()))
    return (mask, probs) if return_probs else mask


def stitch_overlap_logits(logits_tiles, h, w, out, stride, return_probs=False):
    """[n, C, out, out] logits of the overlap_tile_grid(h, w, out, stride) tiles in row-major order (any layout, device) -> uint8 class
    mask [h, w] (and the mean probabilities [C, h, w] when return_probs): predict_overlap_tile's blend."""
    L.init()
    row_o, col_o = overlap_tile_grid(h, w, out, stride)
    n, c = logits_tiles.shape[:2]
    if n != len(row_o) * len(col_o) or tuple(logits_tiles.shape[2:]) != (out, out):
        raise ValueError('stitch_overlap_logits: %s logits for a %dx%d grid of %d px tiles' % (tuple(logits_tiles.shape), len(row_o), len(col_o), out))
    cp = (c + 3) & ~3
    buf = torch.zeros((n, out, out, cp), device=logits_tiles.device)
    buf[..., :c] = logits_tiles.permute(0, 2, 3, 1)
    return _stitch_overlap(buf, cp, n, h, w, out, stride, c, return_probs)


def colourize(mask, palette_rgb, out_h=None, out_w=None):
    """uint8 class mask [h,w] -> RGB uint8 [out_h,out_w,3] via the schema palette, nearest-neighbour resized."""
    L.init()
    h, w = mask.shape
    oh, ow = out_h or h, out_w or w
    pal = torch.as_tensor(palette_rgb, dtype=torch.uint8, device=mask.device).contiguous()
    out = torch.empty((oh, ow, 3), device=mask.device, dtype=torch.uint8)
    check(lib.pylc_colourize_resize(ptr(mask.contiguous()), h, w, ptr(pal), ptr(out), oh, ow, stream()))
    return out
