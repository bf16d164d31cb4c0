"""ReLU, dropout, pooling, concat, bilinear resize, global average pool, image pack, MultiLoss."""
from . import _core
from ._core import *      # noqa: F401,F403  (layout / planes / range / stream helpers, lib bindings, torch)


# Every operator below is a pair of plain driver functions -- forward(needs_input_grad, arguments) -> (outputs, tensors to save, backward-state
# record, non-differentiable outputs); backward(record, saved tensors, needs_input_grad, gradient) -> gradients of the leading arguments --
# and a Function that only adapts them to autograd (_core._adapt / _adapt_back).  pylc_amd.torch_ops calls the drivers directly.
def relu_forward(needs, x):
    L.init()
    x = as_nhwc(x)
    b, c, h, w = x.shape
    out = empty_nhwc(b, c, h, w, x.device)
    check(lib.pylc_relu_fwd(ptr(x), pitch_of(x), ptr(out), c, b * h * w, c, stream()))
    return out, (out,), None, ()           # the backward reads the saved output alone: no record


def relu_backward(state, saved, needs, dout):
    (out,) = saved
    dout = as_nhwc(dout)
    b, c, h, w = out.shape
    dx = empty_nhwc(b, c, h, w, out.device)
    check(lib.pylc_relu_bwd(ptr(dout), pitch_of(dout), ptr(out), c, ptr(dx), c, b * h * w, c, stream()))
    return (dx,)


class ReluFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x):
        return _adapt(ctx, relu_forward(ctx.needs_input_grad, x))

    @staticmethod
    def backward(ctx, dout):
        return _adapt_back(ctx, relu_backward, dout)


def relu(x):
    return ReluFn.apply(x)


class DropoutState:
    __slots__ = ('p', 'seed')

    def __init__(self, p, seed):
        self.p, self.seed = p, seed


def dropout_forward(needs, x, p, seed):
    """The dropout mask is a function of the seed: the backward is the same pass over the gradient."""
    L.init()
    x = as_nhwc(x)
    b, c, h, w = x.shape
    out = empty_nhwc(b, c, h, w, x.device)
    check(lib.pylc_dropout(ptr(x), pitch_of(x), ptr(out), c, b * h * w, c, p, seed, stream()))
    return out, (), DropoutState(p, seed), ()


def dropout_backward(state, saved, needs, dout):
    return (dropout_forward(needs, dout, state.p, state.seed)[0],)


class DropoutFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x, p, seed):
        return _adapt(ctx, dropout_forward(ctx.needs_input_grad, x, p, seed))

    @staticmethod
    def backward(ctx, dout):
        return _adapt_back(ctx, dropout_backward, dout)


def dropout(x, p, seed):
    out = DropoutFn.apply(x, p, seed)
    if ranges_needed() and 0.0 <= p < 1.0:
        binades = 0
        while (1 << binades) * (1.0 - p) < 1.0:      # 1 / (1 - p) <= 2^binades
            binades += 1
        inherit_amax(out, x, binades)
    return out


# ----------------------------------------------------------------------------------------------
# pooling / resize
# ----------------------------------------------------------------------------------------------
class PoolState:
    """cfg: (b, c, h, w, k, stride, pad, oh, ow); link: the gradient link of x when a skip connection may park its crop gradient on it."""
    __slots__ = ('cfg', 'link')

    def __init__(self, cfg, link=None):
        self.cfg, self.link = cfg, link


def maxpool_forward(needs, x, k, stride, pad, link=None, planes_bound=None):
    """Saves the uint8 argmax indices (None when x takes no gradient)."""
    L.init()
    x = as_nhwc(x)
    if pitch_of(x) != x.shape[1]:
        x = x.contiguous(memory_format=torch.channels_last)
    b, c, h, w = x.shape
    oh, ow = (h + 2 * pad - k) // stride + 1, (w + 2 * pad - k) // stride + 1
    y = empty_nhwc(b, c, oh, ow, x.device)
    idx = torch.empty((b, oh, ow, c), device=x.device, dtype=torch.uint8) if needs[0] else None
    if planes_bound is not None:       # the pooled tensor as fp16 planes (its only reader is a conv that takes them)
        check(lib.pylc_maxpool_fwd_planes(ptr(x), ptr(y), pstride(b * oh * ow, c), nplanes(), ptr(planes_bound), ptr(idx), b, h, w, c, k, stride, pad,
                                          oh, ow, stream()))
    else:
        check(lib.pylc_maxpool_fwd(ptr(x), ptr(y), ptr(idx), b, h, w, c, k, stride, pad, oh, ow, stream()))
    link = link if needs[0] else None
    if link is not None:
        link.pool_armed = True
    return y, (idx,), PoolState((b, c, h, w, k, stride, pad, oh, ow), link), ()


def maxpool_backward(state, saved, needs, dy):
    (idx,) = saved
    b, c, h, w, k, stride, pad, oh, ow = state.cfg
    dy = as_nhwc(dy)
    if pitch_of(dy) != c:
        dy = dy.contiguous(memory_format=torch.channels_last)
    dx = empty_nhwc(b, c, h, w, dy.device)
    link = state.link
    crop = None
    if link is not None:
        link.pool_armed = False
        crop, link.crop = link.crop, None
    if crop is not None:        # the skip connection's gradient (centre crop) is summed in the same pass
        g, c0, h0, w0 = crop
        check(lib.pylc_maxpool_bwd_add(ptr(dy), ptr(idx), ptr(dx), b, h, w, c, k, stride, pad, oh, ow, g.data_ptr() + 4 * c0, pitch_of(g),
                                       h0, w0, g.shape[2], g.shape[3], stream()))
    else:
        check(lib.pylc_maxpool_bwd(ptr(dy), ptr(idx), ptr(dx), b, h, w, c, k, stride, pad, oh, ow, stream()))
    return (dx,)


class MaxPoolFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, *args):
        return _adapt(ctx, maxpool_forward(ctx.needs_input_grad, *args))

    @staticmethod
    def backward(ctx, dy):
        return _adapt_back(ctx, maxpool_backward, dy)


def maxpool(x, k, stride, pad=0, link=None, out_planes=False):
    """out_planes: the pooled tensor has ONE reader, a conv that takes fp16 planes (the U-Net's next block): written as planes directly."""
    b, c, h, w = x.shape
    oh, ow = (h + 2 * pad - k) // stride + 1, (w + 2 * pad - k) // stride + 1
    if (out_planes and (torch.is_grad_enabled() or _runtime.eval_planes) and ranges_needed() and not _runtime.no_planes and not is_planes(x) and c % 8 == 0
            and planes_ok(c, b * oh * ow) and b * oh * ow >= _core.PLANES_MIN_PIXELS and _runtime.pool_planes):
        bound = amax_of(x)                 # the maxima are bounded by the input's range
        return mark_planes(MaxPoolFn.apply(x, k, stride, pad, link, bound), bound)
    y = MaxPoolFn.apply(x, k, stride, pad, link)
    return inherit_amax(y, x) if ranges_needed() else y


class CropConcatFn(torch.autograd.Function):
    """U-Net's `torch.cat([up, center_crop(bridge)], 1)` (unet.py:145-152) without the copies that can be avoided: `up` was
    written into the leading channels of the concat buffer by its conv (conv2d(out=[buffer])); the crop of `bridge` is copied
    behind it.  Backward: up's gradient is a channel slice (a view) of the buffer's gradient; the bridge's gradient is
    non-zero only inside the crop window, so when a max-pool also reads `bridge` (always, in the U-Net) it is parked on the
    shared link and summed by the pool's backward kernel -- no zero-padded tensor, no autograd add."""

    @staticmethod
    def forward(ctx, up, bridge, holder, link):
        L.init()
        buf = holder[0]
        bridge = as_nhwc(bridge)
        b, cu, th, tw = up.shape
        cb, hh, ww = bridge.shape[1:]
        if (tuple(buf.shape) != (b, cu + cb, th, tw) or pitch_of(buf) != cu + cb or up.data_ptr() != buf.data_ptr() or cu % 4 or cb % 4
                or th > hh or tw > ww):
            raise L.PylcError('crop_concat: `up` must be the leading channels of the [B, C_up + C_bridge, h, w] buffer')
        h0, w0 = (hh - th) // 2, (ww - tw) // 2
        check(lib.pylc_crop_copy(ptr(bridge), pitch_of(bridge), hh, ww, h0, w0, buf.data_ptr() + 4 * cu, cu + cb, b, th, tw, cb, stream()))
        ctx.geom = (cu, cb, hh, ww, h0, w0)
        ctx.link = link if ctx.needs_input_grad[1] else None
        return buf

    @staticmethod
    def backward(ctx, dy):
        cu, cb, hh, ww, h0, w0 = ctx.geom
        dy = as_nhwc(dy)
        d_up = dy[:, :cu] if ctx.needs_input_grad[0] else None
        d_bridge = None
        if ctx.needs_input_grad[1]:
            link = ctx.link
            if link is not None and link.pool_armed and link.crop is None:
                link.crop = (dy, cu, h0, w0)
            else:
                d_bridge = zeros_nhwc(dy.shape[0], cb, hh, ww, dy.device)
                d_bridge[:, :, h0:h0 + dy.shape[2], w0:w0 + dy.shape[3]] = dy[:, cu:]
        return d_up, d_bridge, None, None


def crop_concat(up, bridge, holder, link=None):
    return CropConcatFn.apply(up, bridge, holder, link)


class UpCatPlanesFn(torch.autograd.Function):
    """U-Net up path, `torch.cat([upsample_x2(z), center_crop(bridge)], 1)` (unet.py:135-152), written in ONE pass as the fp16-plane tensor the
    block's first conv reads (pylc_upsample2_crop_concat_planes): no fp32 concat buffer, no range pass, no conversion.  Backward: z's gradient
    is the bilinear backward of the first C1 channels of the concat gradient, the bridge's gradient is handled as in CropConcatFn (summed by the
    max-pool backward through the shared link)."""

    @staticmethod
    def forward(ctx, z, bridge, bound, link):
        L.init()
        z, bridge = as_nhwc(z), as_nhwc(bridge)
        b, c1, h, w = z.shape
        c2, hh, ww = bridge.shape[1:]
        oh, ow = 2 * h, 2 * w
        out = empty_nhwc(b, c1 + c2, oh, ow, z.device)
        check(lib.pylc_upsample2_crop_concat_planes(ptr(z), pitch_of(z), b, h, w, c1, ptr(bridge), pitch_of(bridge), hh, ww, c2, ptr(out),
                                                    pstride(b * oh * ow, c1 + c2), nplanes(), ptr(bound), stream()))
        ctx.geom = (b, c1, h, w, c2, hh, ww, (hh - oh) // 2, (ww - ow) // 2)
        ctx.link = link if ctx.needs_input_grad[1] else None
        return out

    @staticmethod
    def backward(ctx, dy):
        b, c1, h, w, c2, hh, ww, h0, w0 = ctx.geom
        dy = as_nhwc(dy)
        oh, ow = 2 * h, 2 * w
        dz = d_bridge = None
        if ctx.needs_input_grad[0]:
            dz = empty_nhwc(b, c1, h, w, dy.device)
            tmp = torch.empty(lib.pylc_bilinear_bwd_workspace(b, w, c1, oh) // 4, device=dy.device, dtype=torch.float32)
            amax = torch.empty(1, dtype=torch.int32, device=dy.device) if ranges_needed() and _runtime.fused_grad_ranges else None
            check(lib.pylc_bilinear_bwd_separable(ptr(dy), pitch_of(dy), ptr(dz), c1, b, h, w, c1, oh, ow, ptr(tmp), ptr(amax), stream()))
            if amax is not None:
                tag_amax(dz, amax)          # the 1x1 conv's backward reads dz: its range comes from the pass that wrote it
        if ctx.needs_input_grad[1]:
            link = ctx.link
            if link is not None and link.pool_armed and link.crop is None:
                link.crop = (dy, c1, h0, w0)
            else:
                d_bridge = zeros_nhwc(b, c2, hh, ww, dy.device)
                d_bridge[:, :, h0:h0 + oh, w0:w0 + ow] = dy[:, c1:]
        return dz, d_bridge, None, None


def upsample2_crop_concat(z, bridge, link=None):
    """cat([upsample_x2_bilinear(z), center_crop(bridge)], 1) as one fp16-plane tensor (training graphs and plane-tensor inference with ranged
    arithmetic, channel counts that are multiples of 8); None when that form does not apply -- the caller then uses bilinear(into=) +
    crop_concat."""
    c1, c2 = z.shape[1], bridge.shape[1]
    pixels = z.shape[0] * 4 * z.shape[2] * z.shape[3]
    if not ((torch.is_grad_enabled() or _runtime.eval_planes) and ranges_needed() and not _runtime.no_planes and c1 % 8 == 0 and c2 % 8 == 0 and planes_ok(c1 + c2, pixels)
            and pixels >= _core.PLANES_MIN_PIXELS and not is_planes(z) and _runtime.upcat_planes):
        return None
    bound = torch.maximum(amax_of(z), amax_of(bridge))          # float bit patterns of non-negative values: integer order = float order
    out = UpCatPlanesFn.apply(z, bridge, bound, link)
    return mark_planes(out, bound)


class ConcatSlicesFn(torch.autograd.Function):
    """torch.cat(parts, 1) (aspp.py:80, decoder.py:47) without the copy: every part was WRITTEN into its channel slice of one NHWC
    buffer by the kernel that produced it (bn_act / bilinear `into=`); the "concat" is the buffer.  Backward: each part's gradient is a
    channel-slice view of the buffer's gradient."""

    @staticmethod
    def forward(ctx, holder, *parts):
        buf = holder[0]
        c0 = 0
        offs = []
        for p in parts:
            if p.data_ptr() != buf.data_ptr() + 4 * c0 or tuple(p.shape[2:]) != tuple(buf.shape[2:]) or pitch_of(p) != pitch_of(buf):
                raise L.PylcError('concat_slices: part at channel %d is not that slice of the buffer' % c0)
            offs.append((c0, p.shape[1]))
            c0 += p.shape[1]
        if c0 != buf.shape[1]:
            raise L.PylcError('concat_slices: the parts cover %d of %d channels' % (c0, buf.shape[1]))
        ctx.offs = offs
        return buf

    @staticmethod
    def backward(ctx, dy):
        dy = as_nhwc(dy)
        return (None,) + tuple(dy[:, c0:c0 + c] for c0, c in ctx.offs)


def concat_slices(holder, parts):
    out = ConcatSlicesFn.apply(holder, *parts)
    if ranges_needed():
        tags = [getattr(t, '_pylc_amax', None) for t in parts]
        if all(tg is not None and tg[1] == t._version for tg, t in zip(tags, parts)):
            a = tags[0][0]
            for tg in tags[1:]:
                a = torch.maximum(a, tg[0])
            tag_amax(out, a)
    return out


class ShapeState:
    """The record of a node whose backward needs the input's shape alone (BilinearFn, GapFn): shape = (b, c, h, w); GapFn: the armed gradient
    link of x."""
    __slots__ = ('shape', 'res_link')

    def __init__(self, shape, res_link=None):
        self.shape, self.res_link = shape, res_link


def bilinear_forward(needs, x, oh, ow, into=None):
    L.init()
    x = as_nhwc(x)
    b, c, h, w = x.shape
    cp = pitch_of(x)
    cc = _r4(c)
    if cc > cp:
        raise L.PylcError('bilinear: channel count %d needs a pitch >= %d' % (c, cc))
    if into is not None:               # channels [c0, c0 + c) of a concat buffer: into = ([buffer], c0)
        y, yp = concat_slice(into, b, c, oh, ow, 'bilinear', c % 4 == 0)
    else:
        y, yp = empty_nhwc(b, c, oh, ow, x.device, cc), cc
    check(lib.pylc_bilinear_fwd(ptr(x), cp, ptr(y), yp, b, h, w, cc, oh, ow, stream()))
    return y, (), ShapeState((b, c, h, w)), ()


def bilinear_backward(state, saved, needs, dy):
    b, c, h, w = state.shape
    oh, ow = dy.shape[2:]
    dy = as_nhwc(dy)
    cc = _r4(c)
    if pitch_of(dy) < cc:
        t = zeros_nhwc(b, c, oh, ow, dy.device, cc)
        t.copy_(dy)
        dy = t
    dx = empty_nhwc(b, c, h, w, dy.device, cc)
    if oh >= 2 * h and ow >= 2 * w:      # up-sampling: one axis at a time (10 + 10 instead of 100 candidate taps per element at x4)
        tmp = torch.empty(lib.pylc_bilinear_bwd_workspace(b, w, cc, oh) // 4, device=dy.device, dtype=torch.float32)
        amax = torch.empty(1, dtype=torch.int32, device=dy.device) if ranges_needed() and _runtime.fused_grad_ranges else None
        check(lib.pylc_bilinear_bwd_separable(ptr(dy), pitch_of(dy), ptr(dx), cc, b, h, w, cc, oh, ow, ptr(tmp), ptr(amax), stream()))
        if amax is not None:
            tag_amax(dx, amax)
    else:
        check(lib.pylc_bilinear_bwd(ptr(dy), pitch_of(dy), ptr(dx), cc, b, h, w, cc, oh, ow, stream()))
    return (dx,)


class BilinearFn(torch.autograd.Function):
    """F.interpolate(mode='bilinear', align_corners=True) to an explicit output size."""

    @staticmethod
    def forward(ctx, *args):
        return _adapt(ctx, bilinear_forward(ctx.needs_input_grad, *args))

    @staticmethod
    def backward(ctx, dy):
        return _adapt_back(ctx, bilinear_backward, dy)


def bilinear(x, oh, ow, into=None):
    y = BilinearFn.apply(x, oh, ow, into)
    return inherit_amax(y, x) if ranges_needed() else y       # interpolation weights are a convex combination


def gap_forward(needs, x, res_link=None):
    L.init()
    b, c, h, w = x.shape
    y = empty_nhwc(b, c, 1, 1, x.device)
    if is_planes(x) and c % 8 == 0 and _runtime.gap_planes:
        # the backbone's last BatchNorm left fp16 planes for the atrous convs: pool them as they are (same bits as converting first)
        check(lib.pylc_gap_fwd_planes(ptr(x), pstride(b * h * w, c), nplanes(), ptr(planes_amax(x)), ptr(y), b, h * w, c, stream()))
    else:
        x = as_nhwc(x)
        if pitch_of(x) != x.shape[1]:
            x = x.contiguous(memory_format=torch.channels_last)
        check(lib.pylc_gap_fwd(ptr(x), ptr(y), b, h * w, c, stream()))
    return y, (), ShapeState((b, c, h, w), res_link.arm() if (res_link is not None and needs[0]) else None), ()


def gap_backward(state, saved, needs, dy):
    b, c, h, w = state.shape
    dy = dy.reshape(b, c).contiguous()
    link = state.res_link
    sink = _link_sink(link)
    dx = sink if sink is not None else empty_nhwc(b, c, h, w, dy.device)
    check(lib.pylc_gap_bwd_acc(ptr(dy), ptr(dx), b, h * w, c, 1 if sink is not None else 0, stream()))
    return (link.hand_over(dx) if link is not None else dx,)


class GapFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, *args):
        return _adapt(ctx, gap_forward(ctx.needs_input_grad, *args))

    @staticmethod
    def backward(ctx, dy):
        return _adapt_back(ctx, gap_backward, dy)


def global_avg_pool(x, res_link=None):
    return GapFn.apply(x, res_link)


# ----------------------------------------------------------------------------------------------
# image ingest
# ----------------------------------------------------------------------------------------------
def image_pack(img, mean3, std3, denom=255.0):
    """Raw [B,1|3,H,W] 0..255 tiles -> normalised NHWC4 network input (Model.normalize_image + x3 stack): ((x - mean) / std) / denom."""
    L.init()
    b, c, h, w = img.shape
    img = img.contiguous()
    out = empty_nhwc(b, 4, h, w, img.device)
    m = (C.c_float * 3)(*[float(v) for v in mean3])
    s = (C.c_float * 3)(*[float(v) for v in std3])
    u8 = img.dtype == torch.uint8          # tiles as stored in the database: normalise straight from bytes
    src = img if u8 else img.float()
    check(lib.pylc_image_pack_denom(ptr(src), int(u8), b, c, h, w, m, s, float(denom), ptr(out), stream()))
    return out


def pack_nchw(x, pitch):
    """Already-normalised NCHW fp32 -> NHWC with `pitch` channels (extra channels zero)."""
    L.init()
    b, c, h, w = x.shape
    x = x.contiguous()
    out = zeros_nhwc(b, pitch, h, w, x.device)
    check(lib.pylc_nchw_to_nhwc(ptr(x), ptr(out), pitch, b, h, w, c, stream()))
    return out


# ----------------------------------------------------------------------------------------------
# MultiLoss
# ----------------------------------------------------------------------------------------------
_shard_pairs = {}


def _shard_pair(b, dev):
    """[b, b^2] as a cached device tensor (exact in fp32 for any realistic per-rank tile count)."""
    key = (int(b), str(dev))
    if key not in _shard_pairs:
        _shard_pairs[key] = torch.tensor([float(b), float(b) * float(b)], device=dev)
    return _shard_pairs[key]


SHARD_PAIRS_MAX = 64        # pending pairs folded into one device scalar beyond this many (runs that never call Model.log)


def note_shard_pair(pair, world):
    """Remember the reduced [sum b, sum b^2] pair of ONE data-parallel loss exchange until the host next looks (check_equal_shards).  Every
    step's pair is kept -- a short final batch on some ranks that is followed by full-size steps before the next Model.log() must still be
    reported (the pair used to be overwritten, so only the last step before a log was ever checked).  No host synchronisation
    here: the pairs are views of the steps' statistics messages; past SHARD_PAIRS_MAX of them they are folded on the device into the
    largest violation seen."""
    pend = _runtime.shard_check
    if pend is None:
        pend = _runtime.shard_check = {'pairs': [], 'world': world, 'worst': None}
    pend['pairs'].append(pair)
    pend['world'] = world
    if len(pend['pairs']) >= SHARD_PAIRS_MAX:
        _fold_shard_pairs(pend)


def _shard_violation(pairs, world):
    """max over steps of |world * sum b^2 - (sum b)^2| (zero iff every rank held the same count), with the offending (sum b, sum b^2)"""
    p = torch.stack([q.double() for q in pairs])
    viol = (p[:, 1] * world - p[:, 0] * p[:, 0]).abs()
    k = torch.argmax(viol)
    return torch.stack([viol[k], p[k, 0], p[k, 1]])


def _fold_shard_pairs(pend):
    v = _shard_violation(pend['pairs'], pend['world'])
    pend['pairs'] = []
    pend['worst'] = v if pend['worst'] is None else torch.where(v[0] > pend['worst'][0], v, pend['worst'])      # (no host read)


def check_equal_shards():
    """Raise if ANY data-parallel loss exchange since the last call saw different tile counts on different ranks (the pairs that rode on
    them, see MultiLossFn.forward / note_shard_pair).  One tiny D2H copy: called where the host reads the loss log anyway (Model.log)."""
    pend, _runtime.shard_check = _runtime.shard_check, None
    if pend is None:
        return
    if isinstance(pend, tuple):          # (pair, world): the one-pair form (kept for callers that set it directly)
        pend = {'pairs': [pend[0]], 'world': pend[1], 'worst': None}
    world = pend['world']
    cands = [] if pend['worst'] is None else [pend['worst']]
    if pend['pairs']:
        cands.append(_shard_violation(pend['pairs'], world))
    if not cands:
        return
    viol, sb, sb2 = max((tuple(float(x) for x in c.cpu().tolist()) for c in cands), key=lambda t: t[0])
    if viol > 0.5:
        raise RuntimeError('data-parallel ranks hold different batch sizes (sum b = %g, sum b^2 = %g over %d ranks in one of the steps since the '
                           'last check): SyncBN and the loss head need equal shards -- use a drop_last loader' % (sb, sb2, world))


class MultiLossFn(torch.autograd.Function):
    """Returns a [4] tensor (total, ce, dice, focal); only total carries gradient.

    ignore_index (an int; None: the plain path): targets may be uint8 or int64, pixels whose target equals the index or lies outside
    0..C-1 are skipped (pylc_multiloss_*_ex) and the number of valid pixels is read on the device from the
    (all-reduced) statistics.  bad: an int64 [1] device tensor that the number of out-of-range targets other than the index is ADDED
    into (optional).

    pixel_weights (float32 [B,H,W] on the logits' device; None: the paths above, untouched): a weight u_n per pixel (pylc_multiloss_*_w,
    DESIGN.md section 5.16) -- a saved tensor, no gradient flows into it.  A pixel with u_n == 0 is skipped like an ignored one; negative,
    NaN and infinite weights are skipped and counted in `bad`.  Without an ignore_index the kernels get INT32_MIN as the ignore value, which
    no uint8 target and no class index equals.

    Soft targets (with every keyword below at its default the paths above run call for call):
    soft_target, a float32 [B,C,H,W] tensor on the logits' device, replaces `target` (pass None for it) by a row q_n of C non-negative
    numbers per pixel -- soft_kind='probs': the tensor holds q; 'logits': it holds teacher logits t and q = softmax(t / temperature), taken
    in registers (pylc_multiloss_*_soft).  Only the teacher is softened: the logits are not divided by the temperature and the loss is not
    scaled by its square.  The tensor is read IN PLACE through its four strides (planar, channels-last, a batch slice, a row of windows
    unfolded out of a whole photograph's volume): no contiguous copy is made, and it is saved as it came.  q is used as given and is NOT
    renormalised: CE divides by sum u w_c q_c, Focal by sum u q_c.  A row that sums to exactly 0 leaves its pixel out; a row with a
    negative, NaN or infinite entry (a non-finite teacher logit) leaves it out and is counted in `bad`.  No gradient flows into q.
    label_smoothing (0 <= eps < 1, hard targets only): q_c = (1 - eps) o_c + eps / C through pylc_multiloss_*_ls, the target read and
    judged as on the paths above."""

    NO_IGNORE = -2 ** 31

    @staticmethod
    def forward(ctx, *args):
        return _adapt(ctx, multiloss_forward(ctx.needs_input_grad, *args))

    @staticmethod
    def backward(ctx, dlosses):
        return _adapt_back(ctx, multiloss_backward, dlosses)


class LossState:
    """cfg: (n_global or None, w_ce, w_dice, w_focal, group); ignore: the ignore label the kernels ran with (None: the plain path);
    soft: None, or where the target rows came from -- ('probs', 1.0) / ('logits', 1 / T): the saved `target` is the soft tensor, read through
    its strides; ('smooth', eps): a hard target smoothed by eps."""
    __slots__ = ('cfg', 'ignore', 'soft')

    def __init__(self, cfg, ignore=None, soft=None):
        self.cfg, self.ignore, self.soft = cfg, ignore, soft


SOFT_KINDS = {'probs': 0, 'logits': 1}


def _check_bad(bad, logits):
    if bad is not None and (bad.dtype != torch.int64 or bad.numel() != 1 or bad.device != logits.device):
        raise L.PylcError('bad must be an int64 [1] tensor on the device of the logits')


def _check_pixel_weights(pixel_weights, logits):
    b, c, h, w = logits.shape
    if (not torch.is_tensor(pixel_weights) or pixel_weights.dtype != torch.float32 or tuple(pixel_weights.shape) != (b, h, w)
            or pixel_weights.device != logits.device):
        raise L.PylcError('pixel_weights must be float32 [B,H,W] matching the logits, on their device')
    return pixel_weights.detach().contiguous()


def soft_inv_temperature(temperature):
    """1 / T of a positive finite temperature (PylcError otherwise)"""
    try:
        t = float(temperature)
    except (TypeError, ValueError):
        t = float('nan')
    if not (0.0 < t < float('inf')) or not (0.0 < 1.0 / t < 3.0e38):
        raise L.PylcError('temperature must be a positive finite number, got %r' % (temperature,))
    return 1.0 / t


def _soft_strides(soft):
    return tuple(int(v) for v in soft.stride())


def _check_labels(target, logits):
    b, c, h, w = logits.shape
    if target is None or target.dtype not in (torch.uint8, torch.int64) or tuple(target.shape) != (b, h, w):
        raise L.PylcError('target must be uint8 or int64 [B,H,W] matching the logits')


def multiloss_forward(needs, logits, target, class_weights, w_ce, w_dice, w_focal, group, ignore_index=None, bad=None, pixel_weights=None,
                      soft_target=None, soft_kind='probs', temperature=1.0, label_smoothing=0.0):
    """Saves (logits, target, stats, class_weights[, pixel_weights]); with a soft_target that tensor, as it came, is the saved target.
    Each path states its argument rules and names its statistics entry point with the arguments between (logits, pitch) and the outputs;
    the allocation, the exchange and the finalisation below them are one.  n_global stays None on every path but the plain one, whose
    finalisation takes the pixel count from the host and which neither reads nor checks `bad`."""
    L.init()
    logits = as_nhwc(logits)
    b, c, h, w = logits.shape
    n = b * h * w
    dev = logits.device
    n_global = state_soft = None
    if soft_target is not None or label_smoothing != 0.0:
        eps = float(label_smoothing)
        if not 0.0 <= eps < 1.0:
            raise L.PylcError('label_smoothing must lie in [0, 1), got %r' % (label_smoothing,))
        _check_bad(bad, logits)
        if pixel_weights is not None:
            pixel_weights = _check_pixel_weights(pixel_weights, logits)
        if soft_target is not None:
            if eps != 0.0:
                raise L.PylcError('label_smoothing applies to hard targets: it cannot be combined with a soft_target')
            if target is not None:
                raise L.PylcError('pass target=None with a soft_target: the rows of the soft tensor are the target')
            if ignore_index is not None:
                raise L.PylcError('ignore_index has no meaning with a soft_target: a row that sums to 0 leaves its pixel out')
            if soft_kind not in SOFT_KINDS:
                raise L.PylcError("soft_kind is 'probs' or 'logits', got %r" % (soft_kind,))
            inv_t = soft_inv_temperature(temperature)
            if (not torch.is_tensor(soft_target) or soft_target.dtype != torch.float32 or tuple(soft_target.shape) != (b, c, h, w)
                    or soft_target.device != dev):
                raise L.PylcError('soft_target must be float32 [B,C,H,W] matching the logits, on their device')
            target = soft_target.detach()                           # a view as it came: read through its strides, never copied
            state_soft = (soft_kind, inv_t if soft_kind == 'logits' else 1.0)
            stats_fn, mid = lib.pylc_multiloss_stats_soft, (n, h, w, c, ptr(target), *_soft_strides(target), SOFT_KINDS[soft_kind], state_soft[1],
                                                            ptr(class_weights), ptr(pixel_weights))
        else:
            _check_labels(target, logits)
            target = target.contiguous()
            ignore_index = MultiLossFn.NO_IGNORE if ignore_index is None else int(ignore_index)
            state_soft = ('smooth', eps)
            stats_fn, mid = lib.pylc_multiloss_stats_ls, (ptr(target), target.element_size(), n, c, ignore_index, ptr(class_weights),
                                                          ptr(pixel_weights), eps)
    else:
        target = target.contiguous()
        if pixel_weights is not None:
            pixel_weights = _check_pixel_weights(pixel_weights, logits)
            if ignore_index is None:
                ignore_index = MultiLossFn.NO_IGNORE
        if ignore_index is not None:
            ignore_index = int(ignore_index)
            _check_labels(target, logits)
            _check_bad(bad, logits)
            stats_fn, mid = lib.pylc_multiloss_stats_ex, (ptr(target), target.element_size(), n, c, ignore_index, ptr(class_weights))
            if pixel_weights is not None:
                stats_fn, mid = lib.pylc_multiloss_stats_w, mid + (ptr(pixel_weights),)
        else:
            if target.dtype != torch.int64 or tuple(target.shape) != (b, h, w):
                raise L.PylcError('target must be int64 [B,H,W] matching the logits')
            n_global = float(n)
            stats_fn, mid = lib.pylc_multiloss_stats, (ptr(target), n, c, ptr(class_weights))
    plain = n_global is not None
    st = stream()
    k = 3 + 3 * c
    # data parallel: two more floats ride on the statistics message -- this rank's tile count b and b^2 -- so that unequal shards are
    # DETECTED without a collective of their own (sum b^2 * world == (sum b)^2 iff all equal; Model.train checks the reduced pair at its
    # report interval).  A separate all_gather triggered by a rank-local condition would desynchronise the ranks' collective sequences
    # in exactly the case it is meant to catch.
    stats = torch.empty(k + (2 if group is not None else 0), device=dev)
    ws = torch.empty(lib.pylc_multiloss_workspace_floats(n, c), device=dev)
    check(stats_fn(ptr(logits), pitch_of(logits), *mid, ptr(stats), ptr(ws), *(() if plain else (ptr(bad),)), st))
    if group is not None:
        stats[k:].copy_(_shard_pair(b, dev), non_blocking=True)
        _runtime.sync_all_reduce(stats, group)   # Dice / weighted CE are not shard-decomposable
        world = dist.get_world_size(group)
        note_shard_pair(stats[k:], world)
        if plain:
            n_global *= world
    losses = torch.empty(4, device=dev)
    if plain:
        check(lib.pylc_multiloss_finalize(ptr(stats), n_global, c, w_ce, w_dice, w_focal, ptr(losses), st))
    else:                                                           # n_valid (sum u, sum u q): from the reduced class counts
        check(lib.pylc_multiloss_finalize_ex(ptr(stats), c, w_ce, w_dice, w_focal, ptr(losses), st))
    saved = (logits, target, stats, class_weights) + (() if pixel_weights is None else (pixel_weights,))
    return losses, saved, LossState((n_global, w_ce, w_dice, w_focal, group), ignore_index, state_soft), ()


def multiloss_backward(state, saved, needs, dlosses):
    logits, target, stats, cw = saved[:4]
    pw = saved[4] if len(saved) > 4 else None
    n_global, w_ce, w_dice, w_focal, group = state.cfg
    b, c, h, w = logits.shape
    n = b * h * w
    # the loss is already the GLOBAL loss; each rank back-propagates its own pixels' share and the
    # gradient all-reduce SUMS the shares (pylc_amd/parallel.py)
    gs = dlosses[0:1].contiguous().float()
    cp = _r4(c)
    dl = empty_nhwc(b, c, h, w, logits.device, cp)
    amax = torch.empty(1, dtype=torch.int32, device=logits.device) if ranges_needed() and _runtime.fused_grad_ranges else None
    ignore = state.ignore
    soft = state.soft
    if soft is not None and soft[0] == 'smooth':
        check(lib.pylc_multiloss_bwd_ls(ptr(logits), pitch_of(logits), ptr(target), target.element_size(), n, c, int(ignore), ptr(cw), ptr(pw),
                                        soft[1], ptr(stats), w_ce, w_dice, w_focal, ptr(gs), ptr(dl), cp, ptr(amax), stream()))
    elif soft is not None:
        check(lib.pylc_multiloss_bwd_soft(ptr(logits), pitch_of(logits), n, h, w, c, ptr(target), *_soft_strides(target), SOFT_KINDS[soft[0]],
                                          soft[1], ptr(cw), ptr(pw), ptr(stats), w_ce, w_dice, w_focal, ptr(gs), ptr(dl), cp, ptr(amax),
                                          stream()))
    elif ignore is None:
        check(lib.pylc_multiloss_bwd(ptr(logits), pitch_of(logits), ptr(target), n, c, ptr(cw), ptr(stats), n_global,
                                     w_ce, w_dice, w_focal, ptr(gs), ptr(dl), cp, ptr(amax), stream()))
    elif pw is None:
        check(lib.pylc_multiloss_bwd_ex(ptr(logits), pitch_of(logits), ptr(target), target.element_size(), n, c, int(ignore), ptr(cw),
                                        ptr(stats), w_ce, w_dice, w_focal, ptr(gs), ptr(dl), cp, ptr(amax), stream()))
    else:
        check(lib.pylc_multiloss_bwd_w(ptr(logits), pitch_of(logits), ptr(target), target.element_size(), n, c, int(ignore), ptr(cw),
                                       ptr(pw), ptr(stats), w_ce, w_dice, w_focal, ptr(gs), ptr(dl), cp, ptr(amax), stream()))
    if amax is not None:
        tag_amax(dl, amax)              # (read by a conv backward directly when the net has no logits up-sampling: the U-Net)
    return (dl,)


def multiloss(logits, target, class_weights, w_ce, w_dice, w_focal, group=None, ignore_index=None, bad=None, pixel_weights=None,
              soft_target=None, soft_kind='probs', temperature=1.0, label_smoothing=0.0):
    """[total, ce, dice, focal] (MultiLossFn).  soft_target / soft_kind / temperature / label_smoothing: the soft-target paths described
    there; at their defaults the call is the one it was."""
    if soft_target is None and label_smoothing == 0.0:
        return MultiLossFn.apply(logits, target, class_weights, w_ce, w_dice, w_focal, group, ignore_index, bad, pixel_weights)
    return MultiLossFn.apply(logits, target, class_weights, w_ce, w_dice, w_focal, group, ignore_index, bad, pixel_weights, soft_target,
                             soft_kind, temperature, label_smoothing)


__all__ = [n for n in dir() if not n.startswith('__')]      # everything, underscore helpers included: the package re-exports it (pylc_amd/ops/__init__.py)
