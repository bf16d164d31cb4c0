"""Whole photographs: the reference's test path (test.py:23-115) from a decoded image to the scaled-size class mask, its colour
image and the reference's scores, with every pixel-sized step on the GPU.

For each photograph the reference
  1. reads it and, with --scale, resizes it by cv2.INTER_AREA (get_image, utils/tools.py:77-148);
  2. fits it to the tile grid by a second INTER_AREA resize (adjust_to_tile, utils/tools.py:151-206, through
     Extractor.extract(fit=True, stride=tile//2), utils/extract.py:106-160);
  3. tiles, runs the network and stitches, colourises the mask and nearest-resizes it back to the scaled size
     (utils/tools.py:209-319);
  4. reads a ground-truth mask at the same scale by INTER_NEAREST, class-encodes both masks through the schema palette
     (class_encode, utils/tools.py:412-449) and scores them per image or, with --aggregate_metrics, over all images
     (utils/evaluate.py:64-176).

Here steps 1-2 are pylc_resize_area_u8 (csrc/photo.hip: OpenCV's INTER_AREA weights and fp32 order), step 3 is predict_image's sliding
window on the fitted uint8 image plus pylc_colourize_resize, and step 4 is pylc_class_encode_resize and pylc_confusion_matrix.  Decoding
the image file is the caller's (PIL, imageio or cv2).

A U-Net takes only the scale step and then predict_overlap_tile, which accepts any size: no fit and no resize back.  The reference has
nothing to match there -- it cannot run a U-Net on a photograph at all (reconstruct() assumes same-size tiles).  A DeepLab asked for
blend='mean' takes the same route through the streaming mean-probability blend (inference.predict_blend_mean), which
is what gives it probabilities, a confidence map and a flip ensemble."""
import math

import numpy as np
import torch

from . import boundary, metrics, regions, lib as L
from .inference import predict_blend_mean, predict_image, predict_overlap_tile
from .lib import lib, check, ptr, stream

MAX_CLASSES = 16            # PYLC_MAX_CLASSES (include/pylc_hip.h)


# ---- geometry (host) ---------------------------------------------------------------------------------------------------------------
def scaled_size(h, w, tile, scale=None):
    """get_image's --scale arithmetic (utils/tools.py:125-134), literally: (int(scale * h), int(scale * w)), the scale first raised to
    tile / min_dim when the short side is below the tile.  No scale (None or 0): the size itself."""
    if not scale:
        return h, w
    min_dim = min(h, w)
    if min_dim < tile:
        scale = tile / min_dim
    return int(scale * h), int(scale * w)


def fit_geometry(h, w, tile, stride, scale=None):
    """The reference's meta.extract sizes for an h x w photograph (utils/extract.py:160-170): w_full, h_full, w_scaled, h_scaled, w_fitted,
    h_fitted, offset.  adjust_to_tile (utils/tools.py:182-204) restated in the same Python float arithmetic:
    w_fitted = (w_scaled // tile) * tile, h_fitted = (ceil(w_fitted / aspect) // tile) * tile with aspect = w_scaled / h_scaled.

    Raises ValueError when tile % stride != 0, when a resize would upscale (the scale step does exactly when the short side is below the
    tile, or when scale > 1; the GPU resize downscales only), or when a fitted side would be 0."""
    if stride <= 0 or stride > tile or tile % stride:
        raise ValueError('tile %d is not a multiple of stride %d (adjust_to_tile, utils/tools.py:180)' % (tile, stride))
    h_s, w_s = scaled_size(h, w, tile, scale)
    if h_s > h or w_s > w:
        raise ValueError('photograph %dx%d (HxW) at scale %s would be upscaled to %dx%d (short side below the tile %d?): INTER_AREA '
                         'downscales only here' % (h, w, scale, h_s, w_s, tile))
    if h_s == 0 or w_s == 0:
        raise ValueError('photograph %dx%d (HxW) at scale %s has a side of 0' % (h, w, scale))
    aspect = w_s / h_s
    w_f = (w_s // tile) * tile
    h_f = (math.ceil(w_f / aspect) // tile) * tile
    if w_f == 0 or h_f == 0:
        raise ValueError('photograph %dx%d (HxW, scaled %dx%d) fits to %dx%d tiles of %d: a side of 0' % (h, w, h_s, w_s, h_f, w_f, tile))
    if h_f > h_s:
        raise ValueError('fitting %dx%d to %dx%d would upscale' % (h_s, w_s, h_f, w_f))
    # adjust_to_tile then crops h_resized - int(h_resized / tile) * tile rows off the top; h_f is already a multiple of the tile, so the
    # crop -- the reference's `offset` -- is always 0
    offset = h_f - int(h_f / tile) * tile
    assert offset == 0
    return {'w_full': w, 'h_full': h, 'w_scaled': w_s, 'h_scaled': h_s, 'w_fitted': w_f, 'h_fitted': h_f, 'offset': offset}


# ---- device steps --------------------------------------------------------------------------------------------------------------
def _upload_photo(image, device):
    """[H,W,3] RGB or [H,W] / [H,W,1] grayscale uint8 (numpy or tensor) -> contiguous device uint8 [H,W,C] (one copy)."""
    t = torch.from_numpy(np.ascontiguousarray(image)) if isinstance(image, np.ndarray) else torch.as_tensor(image)
    if t.dtype != torch.uint8:
        raise TypeError('a photograph must be uint8, got %s' % t.dtype)
    if t.dim() == 2:
        t = t.unsqueeze(-1)
    if t.dim() != 3 or t.shape[2] not in (1, 3):
        raise ValueError('a photograph must be [H,W,3] RGB or [H,W] / [H,W,1] grayscale, got %s' % (tuple(t.shape),))
    return t.to(device).contiguous()


def resize_area(img, oh, ow, planar=False):
    """cv2.resize(INTER_AREA) of a device uint8 image, [H,W,C] interleaved (planar=False) or [C,H,W] (planar=True), to [C,oh,ow]."""
    L.init()
    if img.dtype != torch.uint8:
        raise TypeError('resize_area needs uint8, got %s' % img.dtype)
    img = img.contiguous()
    c, h, w = img.shape if planar else (img.shape[2], img.shape[0], img.shape[1])
    out = torch.empty((c, oh, ow), device=img.device, dtype=torch.uint8)
    check(lib.pylc_resize_area_u8(ptr(img), int(planar), c, h, w, ptr(out), oh, ow, stream()))
    return out


def fit_image(image, tile, stride, scale=None, device='cuda'):
    """Upload a photograph once and run the reference's two INTER_AREA resizes on the device: the --scale step when there is one, then the
    fit to the tile grid.  Two launches, as two cv2.resize calls: the uint8 rounding between them is part of the reference's result.
    Returns (device uint8 [C, h_fitted, w_fitted], fit_geometry dict)."""
    L.init()
    shape = tuple(image.shape)
    geom = fit_geometry(shape[0], shape[1], tile, stride, scale)
    img = _upload_photo(image, device)
    h, w = geom['h_full'], geom['w_full']
    h_s, w_s = geom['h_scaled'], geom['w_scaled']
    if (h_s, w_s) != (h, w):
        scaled = resize_area(img, h_s, w_s)
        return resize_area(scaled, geom['h_fitted'], geom['w_fitted'], planar=True), geom
    return resize_area(img, geom['h_fitted'], geom['w_fitted']), geom


def _palette_tensor(palette, n_min, device):
    pal = torch.as_tensor(np.asarray(palette, dtype=np.uint8)).reshape(-1, 3)
    if pal.shape[0] < n_min or pal.shape[0] > MAX_CLASSES:
        raise ValueError('palette needs %d..%d RGB entries, got %d' % (n_min, MAX_CLASSES, pal.shape[0]))
    return pal.to(device).contiguous()


def encode_mask(rgb, palette, out_hw=None, device=None, unmatched=1, ignore_index=None):
    """class_encode of an RGB mask [H,W,3] (uint8, numpy or tensor, host or device) through `palette` ([n][3]), nearest-resized to
    out_hw = (oh, ow) first (cv2.INTER_NEAREST; default: its own size).  The last matching palette index wins, unmatched colours give
    `unmatched`: 1 as in the reference (utils/tools.py:412-449), any int 0..255, or 'ignore' for the value of `ignore_index`.  For a
    ground truth, out_hw is the photograph's (h_scaled, w_scaled).  Returns device uint8 [oh, ow]."""
    if isinstance(unmatched, str):
        if unmatched != 'ignore' or ignore_index is None:
            raise ValueError("unmatched is an int 0..255, or 'ignore' together with an ignore_index")
        unmatched = ignore_index
    unmatched = int(unmatched)
    if not 0 <= unmatched <= 255:
        raise ValueError('unmatched=%d does not fit a uint8 mask (0..255)' % unmatched)
    L.init()
    dev = device or (rgb.device if torch.is_tensor(rgb) and rgb.is_cuda else torch.device('cuda'))
    t = _upload_photo(rgb, dev)
    if t.shape[2] != 3:
        raise ValueError('encode_mask needs an RGB mask [H,W,3], got %s' % (tuple(t.shape),))
    h, w = t.shape[:2]
    oh, ow = out_hw if out_hw is not None else (h, w)
    pal = _palette_tensor(palette, 1, dev)
    out = torch.empty((oh, ow), device=dev, dtype=torch.uint8)
    if unmatched == 1:
        check(lib.pylc_class_encode_resize(ptr(t), h, w, ptr(pal), pal.shape[0], ptr(out), oh, ow, stream()))
    else:
        check(lib.pylc_class_encode_resize_ex(ptr(t), h, w, ptr(pal), pal.shape[0], ptr(out), oh, ow, unmatched, stream()))
    return out


def _colourize(mask, pal, oh, ow):
    out = torch.empty((oh, ow, 3), device=mask.device, dtype=torch.uint8)
    check(lib.pylc_colourize_resize(ptr(mask), mask.shape[0], mask.shape[1], ptr(pal), ptr(out), oh, ow, stream()))
    return out


def _encode(rgb, pal):
    out = torch.empty(rgb.shape[:2], device=rgb.device, dtype=torch.uint8)
    check(lib.pylc_class_encode_resize(ptr(rgb), rgb.shape[0], rgb.shape[1], ptr(pal), pal.shape[0], ptr(out), rgb.shape[0], rgb.shape[1],
                                       stream()))
    return out


class PhotoResult:
    """segment_photo's output.  mask: device uint8 [h_scaled, w_scaled] class indices; rgb: device uint8 [h_scaled, w_scaled, 3] when a
    palette was given (else None); geometry: fit_geometry's dict; probs: the mean softmax probabilities [n_classes, h_scaled, w_scaled]
    when asked (else None); confidence: their maximum over the classes, fp32 [h_scaled, w_scaled], when asked (else None).  tile and
    scale are what the ground truth's size is checked with (PhotoEvaluator.add).  n_sieved: with min_region, a device int64 scalar, the
    number of mask pixels the sieve replaced (else None)."""

    def __init__(self, mask, rgb, geometry, probs, tile, scale, confidence=None, n_sieved=None):
        self.mask, self.rgb, self.geometry, self.probs, self.tile, self.scale = mask, rgb, geometry, probs, tile, scale
        self.confidence = confidence
        self.n_sieved = n_sieved


def _sieve_result(res, pal, min_region, connectivity, fill, ignore_index):
    """The small-region sieve (regions.sieve) as segment_photo's last step: on the scaled-size mask, the colour image
    recoloured from the sieved mask; probs and confidence stay what the network said."""
    res.mask, res.n_sieved = regions.sieve(res.mask, min_region, connectivity, fill, ignore_index, return_changed=True)
    if res.rgb is not None:
        # a constant fill may lie outside the palette (fill='ignore'): colour through 256 entries, black past the palette's own
        pal256 = torch.zeros((256, 3), device=pal.device, dtype=torch.uint8)
        pal256[:pal.shape[0]] = pal
        res.rgb = _colourize(res.mask, pal256, res.mask.shape[0], res.mask.shape[1])
    return res


def segment_photo(model, image, tile=512, stride=None, scale=None, palette=None, batch=8, group=None, return_probs=False, blend='reference',
                  flip=False, return_confidence=False, min_region=0, region_connectivity=4, region_fill='neighbour', ignore_index=None,
                  scales=None, scale_weights=None, temperature=None, refine=None, window=None):
    """A decoded photograph ([H,W,3] RGB or [H,W] / [H,W,1] grayscale uint8, numpy or tensor) -> PhotoResult at the scaled size.

    DeepLab, blend='reference' (default): fit (stride default tile // 2, test.py:63), predict_image's sliding window on the uint8 fitted
    image, pylc_colourize_resize back to (h_scaled, w_scaled), then pylc_class_encode_resize of that colour image: the reference's round
    trip (colourize, resize, class_encode), repeated palette colours included.  Without a palette the identity palette (k, k, k) gives the
    nearest-resized mask.  The reference stitch has no probabilities: flip, return_probs and return_confidence need blend='mean'.

    U-Net, and DeepLab with blend='mean': the scale step only, then the mean-probability blend at the scaled size (predict_overlap_tile,
    stride default its output tile; for DeepLab predict_image(blend='mean'), stride default tile // 2); no fit, no resize back.
    return_probs / return_confidence fill PhotoResult.probs / .confidence; flip=True adds the mirrored windows as a second member.
    scales / scale_weights: the multi-scale ensemble of predict_blend_mean on the scaled-size image, every scale in
    [0.5, 2.0] relative to it; on a DeepLab it needs blend='mean', as flip does.  temperature (None, a positive number, or 'meta' for
    model.meta.temperature) divides the logits before every tile's softmax, under the same condition.
    refine ({'radius': 8, 'eps': 1e-3}) passes the mean probabilities through the guided filter with the scaled-size
    photograph's luma as the guide, under the same condition: mask, probs and confidence are the refined ones, and the order is refine ->
    colourize / encode -> sieve.  window ('hann', 'gauss', ('gauss', sigma_frac), 'uniform' or a table of one float per pixel of the output
    tile; inference.blend_window) weighs every tile's probabilities by a window that falls off towards the tile's edge,
    under the same condition; it pays only with stride below the output tile, and refine and the sieve act on its result.

    min_region > 1: regions of the final mask below that many pixels are sieved (regions.sieve with region_connectivity, region_fill and
    ignore_index; one pass), PhotoResult.rgb is recoloured from the sieved mask and PhotoResult.n_sieved counts the replaced pixels.  A
    region_fill of 'ignore' (or of ignore_index itself) leaves unlabelled pixels, which a palette has no colour for: rgb is black (0, 0, 0)
    there.  0 (default): the path without it, launch for launch.

    The model's channel count must match the image's; the network runs in eval mode and gets its mode back.  `group`: predict_image's
    contract -- every rank fits its own copy and runs its share of the tile batches, rank 0 stitches, resizes and returns, the others
    return None."""
    shape = tuple(image.shape)
    ch = 1 if len(shape) == 2 else shape[2]
    if ch != model.meta.ch:
        raise ValueError('model expects %d-channel images, the photograph has %d' % (model.meta.ch, ch))
    if blend not in ('reference', 'mean'):
        raise ValueError("blend is 'reference' or 'mean', got %r" % (blend,))
    unet = model.meta.arch == 'unet'
    if not unet and blend == 'reference':
        asked = [k for k, v in (('flip', flip), ('return_probs', return_probs), ('return_confidence', return_confidence),
                                ('scales', scales is not None), ('scale_weights', scale_weights is not None),
                                ('temperature', temperature is not None), ('refine', refine is not None),
                                ('window', window is not None)) if v]
        if asked:
            raise ValueError("%s needs blend='mean' on a DeepLab: the reference sliding-window stitch mixes logits and probabilities, its "
                             "scores are not probabilities" % ', '.join(asked))
    from .inference import resolve_temperature
    resolve_temperature(model, temperature)          # argument errors before any launch
    if refine is not None:
        from .refine import check_spec
        check_spec(refine)
    if window is not None:
        from .inference import window_table
        window_table(window, tile - 2 * model.meta.pad_size if unet else tile)
    sieving = int(min_region) > 1
    if sieving:
        regions._check_mask(torch.empty((1, 1), dtype=torch.uint8), region_connectivity, ignore_index)
        regions._fill_value(region_fill, ignore_index)
    L.init()
    dev = model.device
    pal = _palette_tensor(palette, model.meta.n_classes, dev) if palette is not None else None
    if unet or blend == 'mean':
        h_s, w_s = scaled_size(shape[0], shape[1], tile, scale)
        if h_s > shape[0] or w_s > shape[1] or h_s == 0 or w_s == 0:
            raise ValueError('photograph %dx%d (HxW) at scale %s gives %dx%d: INTER_AREA downscales only here' % (shape[0], shape[1], scale,
                                                                                                                   h_s, w_s))
        geom = {'w_full': shape[1], 'h_full': shape[0], 'w_scaled': w_s, 'h_scaled': h_s, 'w_fitted': w_s, 'h_fitted': h_s,
                'offset': 0}                      # Extractor.extract(fit=False): (img, w_scaled, h_scaled, 0)
        img = resize_area(_upload_photo(image, dev), h_s, w_s)      # at its own size: a relayout to [C,H,W]
        if unet:
            got = predict_overlap_tile(model, img, tile, stride, batch, group, return_probs, flip, return_confidence, scales, scale_weights,
                                       temperature, refine, window)
        else:
            got = predict_blend_mean(model, img, tile, tile, stride, batch, group, flip, return_probs, return_confidence, scales,
                                     scale_weights, temperature, refine, window)
        if got is None:
            return None
        got = list(got) if isinstance(got, tuple) else [got]
        mask = got.pop(0)
        probs = got.pop(0) if return_probs else None
        conf = got.pop(0) if return_confidence else None
        rgb = None
        if pal is not None:
            rgb = _colourize(mask, pal, h_s, w_s)
            mask = _encode(rgb, pal)
        res = PhotoResult(mask, rgb, geom, probs, tile, scale, conf)
        return _sieve_result(res, pal, int(min_region), region_connectivity, region_fill, ignore_index) if sieving else res
    stride = tile // 2 if stride is None else stride          # test.py:63
    img, geom = fit_image(image, tile, stride, scale, dev)
    fitted = predict_image(model, img, tile, stride, batch, group)           # the uint8 fitted image is cut as uint8
    if fitted is None:
        return None
    h_s, w_s = geom['h_scaled'], geom['w_scaled']
    enc = pal if pal is not None else torch.arange(model.meta.n_classes, device=dev, dtype=torch.uint8)[:, None].expand(-1, 3).contiguous()
    rgb = _colourize(fitted, enc, h_s, w_s)
    mask = _encode(rgb, enc)
    res = PhotoResult(mask, rgb if pal is not None else None, geom, None, tile, scale)
    return _sieve_result(res, pal, int(min_region), region_connectivity, region_fill, ignore_index) if sieving else res


# ---- scores ----------------------------------------------------------------------------------------------------------------------
class PhotoEvaluator:
    """The reference's Evaluator over segment_photo results, counts on the device (one int64 [C, C] matrix; nothing pixel-sized reaches the
    host).  add() scores one image as Evaluator.evaluate() does (validate() overwrites the first C pixels: force_coverage);
    aggregate() is the --aggregate_metrics result, where validate() overwrites the first C pixels of the CONCATENATION only
    (utils/evaluate.py:150-176): the first image's counts with that coverage, every later image's without.

    boundary_radius (an int, or 'auto' for boundary.default_radius of each image's scaled size): add() also accumulates the image's band
    counts (boundary.boundary_counts; no coverage overwrite applies to them), and add() / aggregate() return
    boundary.boundary_scores' keys next to the four above.  None (default): nothing changes.

    calibration_bins (1..32): add() needs result.confidence (segment_photo(..., return_confidence=True)) and also accumulates the image's
    reliability counts (calibration.reliability_counts; no coverage overwrite applies to them); add() / aggregate()
    return 'ece', 'mce' and 'class_ece' next to the other keys.  None (default): nothing changes."""

    def __init__(self, n_classes, palette, ignore_index=None, boundary_radius=None, calibration_bins=None):
        self.n_classes = int(n_classes)
        # with an ignore label (0..255) a ground-truth colour outside the palette is encoded as it, and only the other pixels are scored
        self.ignore_index = None if ignore_index is None else int(ignore_index)
        self.palette = np.asarray(palette, dtype=np.uint8).reshape(-1, 3)
        if self.palette.shape[0] != self.n_classes:
            raise ValueError('palette has %d entries for %d classes' % (self.palette.shape[0], self.n_classes))
        self.cm = None
        self.count = 0
        if boundary_radius is not None and boundary_radius != 'auto':
            boundary_radius = boundary._check_radius(boundary_radius)
        if boundary_radius is not None:
            boundary._check_ignore(self.ignore_index)
        self.boundary_radius = boundary_radius
        self.boundary_counts = None        # int64 [C*C + 3C + 1] over the images added so far
        self.calibration_bins = None
        if calibration_bins is not None:
            from . import calibration
            self.calibration_bins = calibration._check_bins(calibration_bins)
        self.reliability_counts = None     # int64 [3*C*bins + 3] over the images added so far

    def add(self, result, gt_rgb):
        """Encode the ground-truth RGB mask ([H,W,3] uint8, full size) at the result's scaled size (get_image(scale, INTER_NEAREST)) and
        score the result's mask against it.  A ground truth whose scaled size differs is an error (utils/evaluate.py:96-101).  Returns the
        image's {'f1', 'iou', 'mcc', 'cmatrix'}."""
        if self.calibration_bins is not None and result.confidence is None:
            raise ValueError('a PhotoEvaluator with calibration_bins needs result.confidence: segment_photo(..., return_confidence=True)')
        g = result.geometry
        h_s, w_s = scaled_size(gt_rgb.shape[0], gt_rgb.shape[1], result.tile, result.scale)
        if (h_s, w_s) != (g['h_scaled'], g['w_scaled']):
            raise ValueError('ground truth mask dims (%dpx x %dpx) do not match predicted mask dims (%dpx x %dpx)' % (w_s, h_s, g['w_scaled'],
                                                                                                                    g['h_scaled']))
        ign = self.ignore_index
        y_true = encode_mask(gt_rgb, self.palette, (h_s, w_s), result.mask.device, unmatched=1 if ign is None else ign)
        y_pred = result.mask
        if y_pred.shape != y_true.shape:
            raise ValueError('predicted mask %s vs ground truth %s' % (tuple(y_pred.shape), tuple(y_true.shape)))
        cm = metrics.confusion_matrix(y_true, y_pred, self.n_classes, force_coverage=True, ignore_index=ign)
        plain = None if self.cm is None else metrics.confusion_matrix(y_true, y_pred, self.n_classes, force_coverage=False, ignore_index=ign)
        band = None
        if self.boundary_radius is not None:
            r = boundary.default_radius(h_s, w_s) if self.boundary_radius == 'auto' else self.boundary_radius
            band = boundary.boundary_counts(y_true, y_pred, self.n_classes, r, ign)
        rel = None
        if self.calibration_bins is not None:
            from . import calibration
            rel = calibration.reliability_counts(result.confidence, y_pred, y_true, self.n_classes, self.calibration_bins, ign)
        return self.add_counts(cm, plain, band, rel)

    def add_counts(self, cm_coverage, cm_plain=None, boundary_counts=None, reliability_counts=None):
        """Accumulate one image given its count matrices with and without the coverage overwrite (device tensors, or host arrays for
        counts made elsewhere); cm_plain is needed from the second image on.  boundary_counts: the image's band counts, needed exactly
        when the evaluator has a boundary radius; reliability_counts: the image's reliability counts, needed exactly when it has
        calibration_bins.  Returns the image's scores (those of cm_coverage, and of its own band counts)."""
        if (boundary_counts is None) != (self.boundary_radius is None):
            raise ValueError('add_counts: band counts are given exactly when the evaluator has a boundary_radius')
        if (reliability_counts is None) != (self.calibration_bins is None):
            raise ValueError('add_counts: reliability counts are given exactly when the evaluator has calibration_bins')
        if self.cm is None:
            self.cm = cm_coverage.clone() if torch.is_tensor(cm_coverage) else np.array(cm_coverage, dtype=np.int64)
        else:
            if cm_plain is None:
                raise ValueError('add_counts: every image after the first needs its counts without coverage')
            self.cm += cm_plain
        self.count += 1
        out = metrics.scores(cm_coverage)
        if boundary_counts is not None:
            if self.boundary_counts is None:
                self.boundary_counts = boundary_counts.clone() if torch.is_tensor(boundary_counts) else np.array(boundary_counts, dtype=np.int64)
            else:
                self.boundary_counts += boundary_counts
            out.update(boundary.boundary_scores(boundary_counts, self.n_classes))
        if reliability_counts is not None:
            from . import calibration
            if self.reliability_counts is None:
                self.reliability_counts = (reliability_counts.clone() if torch.is_tensor(reliability_counts)
                                           else np.array(reliability_counts, dtype=np.int64))
            else:
                self.reliability_counts += reliability_counts
            r = calibration.reliability_scores(reliability_counts, self.n_classes, self.calibration_bins)
            out.update(ece=r['ece'], mce=r['mce'], class_ece=r['class_ece'])
        return out

    def aggregate(self):
        if self.cm is None:
            raise ValueError('aggregate evaluation: no images added')
        out = metrics.scores(self.cm)
        if self.boundary_counts is not None:
            out.update(boundary.boundary_scores(self.boundary_counts, self.n_classes))
        if self.reliability_counts is not None:
            from . import calibration
            r = calibration.reliability_scores(self.reliability_counts, self.n_classes, self.calibration_bins)
            out.update(ece=r['ece'], mce=r['mce'], class_ece=r['class_ece'])
        return out
