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
import ctypes as C

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


def predict_image(model, image, tile=512, stride=None, batch=8, group=None, blend='reference', flip=False, return_probs=False,
                  return_confidence=False):
    """image: [C,H,W] raw 0..255 float tensor (host or device), fitted.  Returns the uint8 class mask [H,W] (device).

    group=None (default): LOCAL -- this process runs every tile and returns the mask, also inside a data-parallel job (a rank-0-only
    validation preview must not hang in a collective).  With an explicit process group the call is a COLLECTIVE that every rank of the
    group must make: the tile batches are dealt round-robin over the ranks -- every rank holds the image and a replica of the model --
    and the logit tiles are gathered to rank 0, which stitches; the other ranks return None.

    blend='reference' (default) is the reference's reconstruct() with its quirks (csrc/stitch.hip); it has no probabilities, so flip,
    return_probs and return_confidence raise ValueError with it.  blend='mean' is the streaming mean-probability blend
    (predict_blend_mean, csrc/blend.hip): image uint8 or float, any H, W >= tile, any stride in [1, tile] (default tile // 2); returns the
    mask, or the tuple (mask[, probs][, conf]) in that order -- probs fp32 [n_classes,H,W], conf fp32 [H,W] its maximum over the classes.
    flip=True adds the horizontally mirrored windows as a second ensemble member.

    A U-Net model (meta.arch == 'unet') takes predict_overlap_tile instead (any image size, stride default tile - 2*pad); its blend
    always was the mean, so `blend` is ignored and the other keywords pass through."""
    if blend not in ('reference', 'mean'):
        raise ValueError("blend is 'reference' or 'mean', got %r" % (blend,))
    if model.meta.arch == 'unet':
        return predict_overlap_tile(model, image, tile, stride, batch, group, return_probs, flip, return_confidence)
    if blend == 'mean':
        return predict_blend_mean(model, image, tile, tile, stride, batch, group, flip, return_probs, return_confidence)
    asked = [k for k, v in (('flip', flip), ('return_probs', return_probs), ('return_confidence', return_confidence)) if v]
    if asked:
        raise ValueError("%s needs blend='mean': the reference stitch mixes logits and probabilities, its scores are not probabilities"
                         % ', '.join(asked))
    L.init()
    stride = tile // 2 if stride is None else stride          # test.py:63
    dev = model.device
    img = image.to(dev, dtype=torch.float32).contiguous()
    cimg, h, w = img.shape
    if cimg != model.meta.ch:
        raise ValueError('model expects %d-channel images' % model.meta.ch)
    rows, cols = tile_grid(h, w, tile, stride)
    n = rows * cols
    mean, std, denom = model._stats(model.meta.normalize_default)
    if denom != 255.0:                  # the tile cutter divides by 255: fold the grayscale-defaults branch's missing division into std
        std = [v * denom / 255.0 for v in std]
    world = dist.get_world_size(group) if group is not None else 1
    rank = dist.get_rank(group) if group is not None else 0
    mine = shard_batches(n, batch, rank, world)
    m = (C.c_float * 3)(*[float(v) for v in mean])
    s = (C.c_float * 3)(*[float(v) for v in std])
    ncls = model.meta.n_classes
    cp = (ncls + 3) & ~3
    logits = torch.empty((sum(c for _, c in mine), tile, tile, cp), device=dev)
    was_training = model.net.training
    model.net.eval()
    with torch.no_grad():
        pos = 0
        for k, b in mine:
            x4 = ops.empty_nhwc(b, 4, tile, tile, dev)
            check(lib.pylc_image_pack_tiles(ptr(img), cimg, h, w, tile, stride, k, b, m, s, ptr(x4), stream()))
            y = model.net(x4)                                  # [b, ncls, tile', tile'] NHWC memory, pitch cp
            if y.shape[2] != tile or y.shape[3] != tile:
                raise ValueError('sliding-window stitching needs a same-size network (DeepLab); got %s' % (tuple(y.shape),))
            logits[pos:pos + b].copy_(torch.as_strided(y, (b, tile, tile, cp), (tile * tile * ops.pitch_of(y), tile * ops.pitch_of(y), ops.pitch_of(y), 1),
                                                       y.storage_offset()))
            pos += b
    model.net.train(was_training)
    if world > 1:
        logits = gather_tiles(logits, n, batch, group)
        if logits is None:
            return None
    mask = torch.empty((rows * stride + tile - stride, cols * stride + tile - stride), device=dev, dtype=torch.uint8)
    check(lib.pylc_stitch_argmax(ptr(logits), cp, rows, cols, tile, stride, ncls, ptr(mask), stream()))
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


def predict_overlap_tile(model, image, tile=512, stride=None, batch=8, group=None, return_probs=False, flip=False, return_confidence=False):
    """Full-image U-Net inference by overlap tiles.  image: [C,H,W] raw 0..255, uint8 or float, host or device, any H, W >= out
    (out = tile - 2*meta.pad_size; no fitting).  stride in [1, out], default out.  Returns the uint8 class mask [H,W] (device), or
    (mask, probs) with probs the fp32 mean softmax probabilities [n_classes,H,W] when return_probs.

    The mirrored windows are cut and normalised on the device (predict_image's statistics), run through model.net in eval mode in
    batches of `batch`, and every logit tile stays in HBM until one kernel blends them: each pixel's class scores are the mean of the
    softmax probabilities of the tiles covering it, its class their argmax.  `group`: predict_image's contract (batches dealt over the
    ranks, logit tiles gathered to rank 0, which stitches and returns; the other ranks return None).

    flip=True (the mirrored windows as a second ensemble member) or return_confidence=True (the tuple grows by conf, fp32 [H,W], the
    maximum probability) move the call to the streaming accumulator, predict_blend_mean; without them it is the one-launch stitch."""
    if model.meta.arch != 'unet':
        raise ValueError('predict_overlap_tile needs a U-Net (meta.arch == "unet"), got %r' % model.meta.arch)
    L.init()
    pad = model.meta.pad_size
    out = overlap_tile_out(model.net, tile, pad)
    if flip or return_confidence:
        return predict_blend_mean(model, image, tile, out, stride, batch, group, flip, return_probs, return_confidence)
    stride = out if stride is None else int(stride)
    dev = model.device
    u8 = image.dtype == torch.uint8            # a photograph: a quarter of the bytes to upload, normalised straight from them
    img = image.to(dev, dtype=torch.uint8 if u8 else torch.float32).contiguous()
    cimg, h, w = img.shape
    if cimg != model.meta.ch:
        raise ValueError('model expects %d-channel images' % model.meta.ch)
    row_o, col_o = overlap_tile_grid(h, w, out, stride, pad)
    n = len(row_o) * len(col_o)
    mean, std, denom = model._stats(model.meta.normalize_default)
    if denom != 255.0:                  # the tile cutter divides by 255: fold the grayscale-defaults branch's missing division into std
        std = [v * denom / 255.0 for v in std]
    world = dist.get_world_size(group) if group is not None else 1
    rank = dist.get_rank(group) if group is not None else 0
    mine = shard_batches(n, batch, rank, world)
    m = (C.c_float * 3)(*[float(v) for v in mean])
    s = (C.c_float * 3)(*[float(v) for v in std])
    ncls = model.meta.n_classes
    cp = (ncls + 3) & ~3
    logits = torch.empty((sum(c for _, c in mine), out, out, cp), device=dev)
    was_training = model.net.training
    model.net.eval()
    try:
        model._refresh_for_inference()
        with torch.no_grad():
            pos = 0
            for k, b in mine:
                x4 = ops.empty_nhwc(b, 4, tile, tile, dev)
                check(lib.pylc_image_pack_tiles_reflect(ptr(img), int(u8), cimg, h, w, tile, out, stride, k, b, m, s, ptr(x4), stream()))
                y = ops.as_nhwc(model.net(x4))                     # [b, ncls, out, out], NHWC memory
                logits[pos:pos + b, :, :, :ncls].copy_(y.permute(0, 2, 3, 1))
                pos += b
    finally:
        model.net.train(was_training)
    if world > 1:
        logits = gather_tiles(logits, n, batch, group)
        if logits is None:
            return None
    return _stitch_overlap(logits, cp, n, h, w, out, stride, ncls, return_probs)


def predict_blend_mean(model, image, tile, out, stride=None, batch=8, group=None, flip=False, return_probs=False, return_confidence=False):
    """The streaming mean-probability blend (csrc/blend.hip) for a network that maps a `tile` window to its centred `out`
    square (DeepLab: out = tile; U-Net: out = tile - 2*pad).  image: [C,H,W] raw 0..255, uint8 or float, any H, W >= out; stride in
    [1, out], default tile // 2 for a same-size network and out otherwise.

    Windows are cut by pylc_image_pack_tiles_reflect_ex, each batch's logits go straight from the network's output (at its own pitch) into
    pylc_blend_accumulate, which adds their softmax probabilities into one fp32 image [H,W,cp]; pylc_blend_finalize divides by the number
    of covering tiles and members once at the end.  No logit tile outlives its batch.  flip=True runs a second sweep, member-major: all
    tiles unflipped, then all tiles cut and accumulated mirrored.  The tiles are visited in ascending index within and across batches, so
    the result does not depend on `batch`.

    `group`: every rank accumulates its share of the batches into its own image, dist.all_reduce sums them (results then differ from one
    process's by fp32 summation order only; a one-rank group equals no group bit for bit), rank 0 finalizes, the others return None.
    Returns mask, or (mask[, probs][, conf])."""
    L.init()
    if stride is None:
        stride = tile // 2 if out == tile else out
    stride = int(stride)
    dev = model.device
    u8 = image.dtype == torch.uint8
    img = image.to(dev, dtype=torch.uint8 if u8 else torch.float32).contiguous()
    cimg, h, w = img.shape
    if cimg != model.meta.ch:
        raise ValueError('model expects %d-channel images' % model.meta.ch)
    row_o, col_o = overlap_tile_grid(h, w, out, stride, (tile - out) // 2)
    n = len(row_o) * len(col_o)
    mean, std, denom = model._stats(model.meta.normalize_default)
    if denom != 255.0:                  # the tile cutter divides by 255: fold the grayscale-defaults branch's missing division into std
        std = [v * denom / 255.0 for v in std]
    world = dist.get_world_size(group) if group is not None else 1
    rank = dist.get_rank(group) if group is not None else 0
    mine = shard_batches(n, batch, rank, world)
    m = (C.c_float * 3)(*[float(v) for v in mean])
    s = (C.c_float * 3)(*[float(v) for v in std])
    ncls = model.meta.n_classes
    cp = (ncls + 3) & ~3
    acc = torch.zeros((h, w, cp), device=dev)
    members = 2 if flip else 1
    was_training = model.net.training
    model.net.eval()
    try:
        model._refresh_for_inference()
        with torch.no_grad():
            for member in range(members):                   # member-major: the sums of member 0 are complete before member 1 adds to them
                for k, b in mine:
                    x4 = ops.empty_nhwc(b, 4, tile, tile, dev)
                    check(lib.pylc_image_pack_tiles_reflect_ex(ptr(img), int(u8), cimg, h, w, tile, out, stride, k, b, m, s, ptr(x4), stream(),
                                                               member))
                    y = ops.as_nhwc(model.net(x4))                     # [b, ncls, out, out], NHWC memory
                    if tuple(y.shape[1:]) != (ncls, out, out):
                        raise ValueError('the network returned %s for %d px windows, not %d classes of %d px' % (tuple(y.shape), tile, ncls, out))
                    p = ops.pitch_of(y)
                    if p % 4 or y.data_ptr() % 16:                      # a pitch the 16-byte loads cannot take: one relayout to pitch cp
                        y2 = ops.zeros_nhwc(b, ncls, out, out, dev, pitch=cp)
                        y2.copy_(y)
                        y, p = y2, cp
                    check(lib.pylc_blend_accumulate(ptr(y), p, k, b, h, w, out, stride, ncls, member, ptr(acc), cp, stream()))
    finally:
        model.net.train(was_training)
    if world > 1:
        dist.all_reduce(acc, group=group)
        if rank != 0:
            return None
    return _blend_finalize(acc, cp, h, w, out, stride, ncls, members, return_probs, return_confidence)


def _blend_finalize(acc, cp, h, w, out, stride, ncls, members, return_probs, return_confidence):
    mask = torch.empty((h, w), device=acc.device, dtype=torch.uint8)
    probs = torch.empty((ncls, h, w), device=acc.device) if return_probs else None
    conf = torch.empty((h, w), device=acc.device) if return_confidence else None
    check(lib.pylc_blend_finalize(ptr(acc), cp, h, w, out, stride, ncls, members, ptr(mask), ptr(probs), ptr(conf), stream()))
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
