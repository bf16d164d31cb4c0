"""BatchNorm (+ residual + ReLU + dropout) operators, SyncBN message driver (models/sync_batchnorm/batchnorm.py:48-125 is the math)."""
from . import _core
from ._core import *      # noqa: F401,F403  (layout / planes / range / stream helpers, lib bindings, torch)


def _bn_extra(**kw):
    ex = L.BnExtra()
    ex.nplanes = nplanes()
    for k, v in kw.items():
        setattr(ex, k, v)
    return ex


class BnState:
    """What bn_act_backward reads besides the saved tensors (y, out, coef, out_bound, mask, y_bound), and what the conv / depthwise node that
    consumes the output reads and writes through its `bn_src.st`: sole, pre_sums, bn_emit_ok, y_shape, cfg.  The defaults are the plain
    functional case."""
    __slots__ = ('cfg', 'g_param', 'b_param', 'y_shape', 'clamp', 'bn_emit_ok', 'sole', 'pre_sums', 'want_amax', 'out_pl', 'drop', 'dy_pl', 'res_link')

    def __init__(self, cfg, g_param, b_param, y_shape=None, clamp=(False, 1e-5), bn_emit_ok=False, sole=False, want_amax=False, out_pl=False,
                 drop=(0.0, 0), dy_pl=False, res_link=None):
        self.cfg, self.g_param, self.b_param, self.y_shape = cfg, g_param, b_param, y_shape      # cfg: (relu, training, group, n_global, has residual)
        self.clamp, self.want_amax, self.out_pl, self.drop, self.dy_pl, self.res_link = clamp, want_amax, out_pl, drop, dy_pl, res_link
        # a conv dgrad that writes this output's complete gradient may take the backward sums in its epilogue (conv2d_backward) and leave them in
        # pre_sums; `sole` = the caller says the output has ONE consumer
        self.bn_emit_ok, self.sole, self.pre_sums = bn_emit_ok, sole, None


def bn_node_of(x):
    """The BnActFn node that produced x in a graph that takes gradients (else None), recognised by the type of its record: what ops.conv2d /
    ops.dwconv3x3 hand their node as bn_src."""
    src = x.grad_fn if (torch.is_grad_enabled() and x.requires_grad) else None
    return src if isinstance(getattr(src, 'st', None), BnState) else None


class BnActFn(torch.autograd.Function):
    """out = [dropout](act(BN(y) (+ residual))).  Training: batch statistics (all-reduced over `group` when given --
    the SyncBN exchange of models/sync_batchnorm/batchnorm.py:48-125 as one RCCL all-reduce of
    [sum, sumsq, count]); eval: running statistics.

    out_planes: write the output as fp16 planes (ops.is_planes) for a conv that copies its operand tiles (conv_pl.hip); the scale
    comes from a range BOUND that the statistics give before the apply pass runs (pylc_bn_finalize*_ex).  The backward hands dy back as
    planes when the conv that produced y asked for it (y._pylc_dy_pl).  drop = (p, seed): the nn.Dropout that follows the activation
    in the reference (aspp.py:86, decoder.py:33,37), fused into both passes."""

    @staticmethod
    def forward(ctx, *args):
        ctx.set_materialize_grads(False)
        return _adapt(ctx, _drive_collectives([bn_act_forward(ctx.needs_input_grad, *args)], args[10])[0])

    @staticmethod
    def backward(ctx, dout, *_unused):
        return _drive_collectives([bn_act_backward(ctx.st, ctx.saved_tensors, ctx.needs_input_grad, dout)], ctx.st.cfg[2])[0]


def bn_act_forward(needs, y, gamma, beta, running_mean, running_var, residual, relu, training, eps, momentum, group, clamp_eps, pre_sums=None,
                   want_amax=False, res_link=None, out_planes=False, drop=None, dy_planes=False, into=None, sole=False, defer=False):
    """Drives BnActFn's forward kernels.  Generator: yields the tensor of each collective (the SyncBN moments) instead of all-reducing it, so
    that the BatchNorms of parallel branches can share one message (GroupBnActFn).  needs: needs_input_grad of the arguments.  Returns (out |
    (out, bound | amax) | (out, bound, coef), tensors to save, BnState, non-differentiable outputs)."""
    L.init()
    # precision mode 3 with half activations: y may arrive as ONE fp16 plane (written by the conv / depthwise epilogue); it is read as such
    y_bound = planes_amax(y) if (is_planes(y) and nplanes() == 1 and half_acts() and training) else None
    if y_bound is None:
        y = as_nhwc(y)
    b, c, h, w = y.shape
    m = b * h * w
    dev = y.device
    st = stream()
    yp = c if y_bound is not None else pitch_of(y)
    refine_y = y if (_runtime.bn_refine and y_bound is None) else None        # the second-pass variance refinement reads an fp32 y
    coef = torch.empty(4 * c, device=dev)            # mean | invstd | scale | shift
    mean, invstd, scale, shift = coef[:c], coef[c:2 * c], coef[2 * c:3 * c], coef[3 * c:]
    n_global = float(m)
    if training and m == 1 and group is None:
        # torch.nn.BatchNorm2d's behaviour (the ASPP image-pool branch normalises over the batch only: B must be > 1)
        raise ValueError('Expected more than 1 value per channel when training, got input size %s' % (tuple(y.shape),))
    drop_p, drop_seed = drop if (drop is not None and training) else (0.0, 0)
    out_planes = bool(out_planes and training and planes_ok(c, m) and m >= _core.PLANES_MIN_PIXELS)
    res = res_pl = res_amax = None
    if residual is not None:
        if is_planes(residual) and training:
            res_pl, res_amax = residual, planes_amax(residual)
        else:
            res = as_nhwc(residual)
            if out_planes:
                res_amax = amax_of(res)
    bound = amax_slot(dev) if out_planes else None
    mul = 1.0 / (1.0 - drop_p) if drop_p > 0 else 1.0
    if training:
        partial = pre_sums if (pre_sums is not None and pre_sums.dim() == 2 and pre_sums.shape[1] == 2 * c) else None
        kshift = getattr(partial, '_pylc_shift', None) if partial is not None else None
        if partial is not None and group is None:
            # statistics came out of the conv epilogue as per-tile partials: combine + coefficients in one launch
            check(lib.pylc_bn_finalize_from_partial_ex(ptr(partial), partial.shape[0], n_global, c, ptr(gamma), ptr(beta), eps, momentum,
                                                       int(clamp_eps), ptr(running_mean), ptr(running_var), ptr(mean), ptr(invstd),
                                                       ptr(scale), ptr(shift), ptr(res_amax), mul, ptr(bound),
                                                       ptr(refine_y), yp, m, ptr(kshift), st))
        else:
            sums = torch.empty(2 * c, device=dev)                     # [sum | sumsq]
            if partial is not None:
                check(lib.pylc_bn_stats_from_partial(ptr(partial), partial.shape[0], c, ptr(sums), st))
            else:
                if y_bound is not None:          # no statistics came with the half tensor: take them from an fp32 copy (rare)
                    y, y_bound = from_planes(mark_planes(y, y_bound)), None
                ws = torch.empty(lib.pylc_bn_workspace_floats(m, c), device=dev)
                check(lib.pylc_bn_stats(ptr(y), m, c, yp, ptr(sums), ptr(ws), st))
            if group is not None:
                # SyncBN: this rank's moments in fp64 [sum | sumsq | count], ONE all-reduce, coefficients from the global moments
                moments = torch.empty(2 * c + 1, device=dev, dtype=torch.float64)
                check(lib.pylc_bn_local_moments(ptr(sums), float(m), c, ptr(refine_y), yp, m, ptr(kshift),
                                                ptr(moments), st))
                yield moments                                         # all-reduced (SUM) by the driver, alone or with other layers' moments
                n_global = float(m) * dist.get_world_size(group)      # equal shards (checked by parallel.init_from_env / DataParallel setup)
                check(lib.pylc_bn_finalize_moments(ptr(moments), n_global, c, ptr(gamma), ptr(beta), eps, momentum, int(clamp_eps),
                                                   ptr(running_mean), ptr(running_var), ptr(mean), ptr(invstd), ptr(scale), ptr(shift),
                                                   ptr(res_amax), mul, ptr(bound), ptr(kshift), st))
            else:
                check(lib.pylc_bn_finalize_ex(ptr(sums), n_global, c, ptr(gamma), ptr(beta), eps, momentum, int(clamp_eps),
                                              ptr(running_mean), ptr(running_var), ptr(mean), ptr(invstd), ptr(scale), ptr(shift),
                                              ptr(res_amax), mul, ptr(bound), ptr(refine_y), yp, m, ptr(kshift), st))
    else:
        check(lib.pylc_bn_eval_coeffs_full(ptr(running_mean), ptr(running_var), ptr(gamma), ptr(beta), eps, c,
                                           ptr(scale), ptr(shift), ptr(mean), ptr(invstd), st))
    if defer and training and y_bound is not None and out_planes and residual is None and drop_p == 0 and into is None:
        # Deferred apply (precision mode 3, half activations): the ONLY consumer is a depthwise conv that applies scale / shift / ReLU to
        # its LDS patch (pylc_dwconv3x3_*_h_bn), so no pass runs and no output is written here -- the result aliases y and travels with
        # the coefficients (ops.bn_act: `_pylc_defer`).  The backward is the ordinary one (ReLU mask recomputed from y).
        state = BnState((relu, training, group, n_global, False), gamma, beta, (b, c, h, w), (bool(clamp_eps), float(eps)), False, True, want_amax,
                      True, (0.0, 0), bool(dy_planes and planes_ok(c, m) and yp == c), res_link)
        return (torch.as_strided(y, y.shape, y.stride()), bound, coef), (y, None, coef, bound, None, y_bound), state, (bound, coef)
    if into is not None:               # write into channels [c0, c0 + c) of a caller-owned concat buffer: into = ([buffer], c0)
        out, op_ = concat_slice(into, b, c, h, w, 'bn_act', not out_planes)
    else:
        out, op_ = empty_nhwc(b, c, h, w, dev), c
    amax = amax_slot(dev) if (want_amax and not out_planes) else None
    # a ReLU behind a residual add: its mask cannot be recomputed from y, so this pass leaves one bit per element for the backward
    # (bn.hip "1-bit ReLU masks") instead of the backward re-reading `out` twice
    mask = None
    if training and relu and residual is not None and c % 8 == 0 and drop_p == 0 and any(needs) and not _runtime.no_relu_bits:
        mask = torch.empty(m * c // 8, dtype=torch.uint8, device=dev)
    tm = _bn_time('apply%s%s%s' % ('+res' if residual is not None else '', '+bits' if mask is not None else '', '+drop' if drop_p > 0 else ''), m, c,
                  # algorithmic bytes: 4 B per fp32 / two-plane element, 2 B per one-plane (precision mode 3) element, 1/8 B per mask bit
                  m * c * ((2 if y_bound is not None else 4) + (2 * nplanes() if out_planes else 4)
                           + (0 if residual is None else (2 * nplanes() if res_pl is not None else 4)) + (0.125 if mask is not None else 0)))
    tm.__enter__()
    if out_planes or res_pl is not None or drop_p > 0 or mask is not None or y_bound is not None:
        ex = _bn_extra(drop_p=drop_p, drop_seed=drop_seed)
        if mask is not None:
            ex.relu_mask = ptr(mask)
        if y_bound is not None:
            ex.y_half_bound = ptr(y_bound)
        if out_planes:
            ex.out_planes, ex.out_plane_stride, ex.out_bound = ptr(out), pstride(m, c), ptr(bound)
        if res_pl is not None:
            ex.res_planes, ex.res_plane_stride, ex.res_amax = ptr(res_pl), pstride(m, c), ptr(res_amax)
        check(lib.pylc_bn_apply_ex(ptr(y), yp, ptr(scale), ptr(shift), ptr(res), pitch_of(res) if res is not None else (c if res_pl is not None else 0),
                                   None if out_planes else ptr(out), op_, m, c, int(relu), ptr(amax), C.byref(ex), st))
    else:
        check(lib.pylc_bn_apply(ptr(y), yp, ptr(scale), ptr(shift), ptr(res), pitch_of(res) if res is not None else 0,
                                ptr(out), op_, m, c, int(relu), ptr(amax), st))
    tm.__exit__()
    # ReLU mask in backward: without a residual it is recomputed from y (y*scale + shift > 0, the forward's own
    # expression), so `out` is neither kept alive for it nor read again
    saved = (y, out if (relu and residual is not None and mask is None) else None, coef, bound, mask, y_bound)
    # bn_emit_ok: possible for a training-mode pass without fused dropout over a dense fp32 y
    state = BnState((relu, training, group, n_global, residual is not None), gamma, beta, (b, c, h, w), (bool(clamp_eps), float(eps)),
                  bool(training and drop_p == 0 and into is None and yp == c and c % 8 == 0 and any(needs) and y_bound is None), bool(sole),
                  want_amax, out_planes, (drop_p, drop_seed), bool(dy_planes and training and planes_ok(c, m) and yp == c), res_link)
    tagv = bound if out_planes else (amax if want_amax else None)
    return (out, saved, state, ()) if tagv is None else ((out, tagv), saved, state, (tagv,))


def bn_act_backward(state, saved, needs, dout):
    """Drives BnActFn's backward kernels.  Generator (as bn_act_forward): yields the [sum g xhat | sum g] message of a synchronised layer.
    Returns one gradient per entry of `needs`."""
    if dout is None:
        return (None,) * len(needs)
    y, out, coef, out_bound, mask, y_bound = saved
    relu, training, group, n_global, has_res = state.cfg
    gamma, beta = state.g_param, state.b_param
    # precision mode 3 with half activations: dout may arrive as ONE fp16 plane (a dgrad's output); read as such unless a gradient link
    # is going to accumulate fp32 values into what this pass hands on
    a_bound = None
    if is_planes(dout) and nplanes() == 1 and half_acts() and training and not (state.res_link is not None and state.res_link.armed):
        a_bound = planes_amax(dout)
    else:
        dout = as_nhwc(dout)
    b, c, h, w = y.shape
    m = b * h * w
    dev = y.device
    st = stream()
    mean, invstd = coef[:c], coef[c:2 * c]
    scale, shift = (coef[2 * c:3 * c], coef[3 * c:]) if (relu and out is None and mask is None) else (None, None)
    # [dgamma | dbeta] go straight into the flat gradient arena when gamma/beta own adjacent slots there
    tg, tb = _grad_target(gamma), _grad_target(beta)
    direct = (tg is not None and tb is not None and tb.data_ptr() == tg.data_ptr() + 4 * c
              and needs[1] and needs[2])
    sums = torch.as_strided(tg, (2 * c,), (1,)) if direct else torch.empty(2 * c, device=dev)
    ws = torch.empty(lib.pylc_bn_workspace_floats(m, c), device=dev)
    out_pl = state.out_pl and out is not None
    drop_p, drop_seed = state.drop
    dy_pl = state.dy_pl
    use_ex = out_pl or drop_p > 0 or dy_pl or mask is not None or a_bound is not None or y_bound is not None
    op = (c if out_pl else pitch_of(out)) if out is not None else 0
    dout_pitch = c if a_bound is not None else pitch_of(dout)
    y_pitch = c if y_bound is not None else pitch_of(y)
    ex = None
    dy_bound = None
    msrc = 0.125 if mask is not None else (4 if (relu and out is not None) else 0)         # bytes per element read for the ReLU mask
    pre, state.pre_sums = state.pre_sums, None
    e_in = (2 if a_bound is not None else 4) + (2 if y_bound is not None else 4)          # dout + y: one fp16 plane each in precision mode 3
    tm = _bn_time('bwd_sums(from dgrad)' if pre is not None else 'bwd_reduce(+sums)', m, c, m * c * (e_in + msrc) if pre is None else 0)
    tm.__enter__()
    if pre is not None:
        # the conv dgrad that produced `dout` took the per-tile sums in its epilogue: only the combine (and the dy bound) is left
        part, rows, g_amax = pre
        if use_ex:
            ex = _bn_extra(drop_p=drop_p, drop_seed=drop_seed)
            if mask is not None:
                ex.relu_mask = ptr(mask)
            ex.y_half_bound, ex.dout_half_bound = ptr(y_bound), ptr(a_bound)
            if out_pl:
                ex.out_planes, ex.out_plane_stride, ex.out_bound = ptr(out), pstride(m, c), ptr(out_bound)
            if dy_pl:
                dy_bound = amax_slot(dev)
                ex.g_amax = ptr(g_amax)
        local_bound = dy_pl and not (training and group is not None)
        check(lib.pylc_bn_bwd_sums_from_partial(ptr(part), rows, c, ptr(sums), ptr(gamma), ptr(invstd), n_global, ptr(g_amax),
                                                ptr(dy_bound) if local_bound else None, st))
    elif use_ex:
        ex = _bn_extra(drop_p=drop_p, drop_seed=drop_seed)
        if mask is not None:
            ex.relu_mask = ptr(mask)
        ex.y_half_bound, ex.dout_half_bound = ptr(y_bound), ptr(a_bound)
        if out_pl:
            ex.out_planes, ex.out_plane_stride, ex.out_bound = ptr(out), pstride(m, c), ptr(out_bound)
        if dy_pl:
            g_amax, dy_bound = amax_slot(dev), amax_slot(dev)
            ex.g_amax = ptr(g_amax)
        local_bound = dy_pl and not (training and group is not None)
        check(lib.pylc_bn_bwd_reduce_ex(ptr(dout), dout_pitch, None if out_pl else ptr(out), op, ptr(y), y_pitch, ptr(mean), ptr(invstd),
                                        m, c, int(relu), ptr(sums), ptr(ws), ptr(scale), ptr(shift), ptr(gamma), n_global, C.byref(ex),
                                        ptr(dy_bound) if local_bound else None, st))
    else:
        check(lib.pylc_bn_bwd_reduce(ptr(dout), pitch_of(dout), ptr(out), op, ptr(y), pitch_of(y), ptr(mean), ptr(invstd),
                                     m, c, int(relu), ptr(sums), ptr(ws), ptr(scale), ptr(shift), st))
    tm.__exit__()
    local_sums = sums
    if training and group is not None:
        sums = local_sums.clone()          # parameter grads stay local (the gradient all-reduce sums them later)
        yield sums
        if dy_pl:
            check(lib.pylc_bn_bwd_bound(ptr(sums), ptr(gamma), ptr(invstd), n_global, c, ptr(g_amax), ptr(dy_bound), st))
    clamp_eps, eps = state.clamp
    if training and clamp_eps:
        # batchnorm.py:125 inv_std = clamp(var, eps)^-1/2: where the clamp is active inv_std no longer depends on the batch, so autograd
        # sends nothing through the variance there -- dy loses its xhat * sum(g xhat) / n term on those channels (dgamma keeps the sum).
        # The finalize kernels store exactly (float)(1 / sqrt((double)eps)) for a clamped channel.
        thr = torch.tensor(eps, dtype=torch.float32, device=dev).double().rsqrt().float()
        sums = torch.cat((sums[:c] * (invstd < thr), sums[c:]))
    if not training:
        sums_apply = torch.zeros(2 * c, device=dev)   # running statistics are constants: dy = gamma*invstd*g
        if dy_pl:
            check(lib.pylc_bn_bwd_bound(ptr(sums_apply), ptr(gamma), ptr(invstd), n_global, c, ptr(g_amax), ptr(dy_bound), st))
    else:
        sums_apply = sums
    dy = empty_nhwc(b, c, h, w, dev)
    want_res = has_res and needs[5]
    # without a ReLU (and without dropout) the residual's gradient IS dout: hand the tensor on instead of having the kernel write a
    # copy (unless a conv is going to accumulate its dgrad into the buffer, which must then be ours)
    res_is_dout = want_res and not relu and drop_p == 0 and not (state.res_link is not None and state.res_link.armed)
    # with the 1-bit mask and a gradient link, the residual's gradient relu'(dout) is not written out at all: the (dout, mask) pair is
    # parked on the link and the conv dgrad that consumes it forms the masked gradient in its epilogue (pylc_conv2d_dgrad_add)
    lk = state.res_link
    park_masked = (want_res and relu and mask is not None and drop_p == 0 and lk is not None and lk.armed and lk.buf is None
                   and lk.masked is None and a_bound is None and pitch_of(dout) == c and _runtime.fuse_res_grad)
    g_out = empty_nhwc(b, c, h, w, dev) if (want_res and not res_is_dout and not park_masked) else None
    amax_dy = amax_slot(dev) if (state.want_amax and not dy_pl) else None
    tm = _bn_time('bwd_apply%s' % ('+gres' if g_out is not None else ''), m, c,
                  m * c * (e_in + (2 * nplanes() if dy_pl else 4) + msrc + (4 if g_out is not None else 0)))
    tm.__enter__()
    if use_ex:
        if dy_pl:
            ex.dy_planes, ex.dy_plane_stride, ex.dy_bound = ptr(dy), pstride(m, c), ptr(dy_bound)
        check(lib.pylc_bn_bwd_apply_ex(ptr(dout), dout_pitch, None if out_pl else ptr(out), op, ptr(y), y_pitch, ptr(mean), ptr(invstd),
                                       ptr(gamma), ptr(sums_apply), n_global, m, c, int(relu), None if dy_pl else ptr(dy), c,
                                       ptr(g_out), c if g_out is not None else 0, ptr(amax_dy), ptr(scale), ptr(shift), C.byref(ex), st))
    else:
        check(lib.pylc_bn_bwd_apply(ptr(dout), pitch_of(dout), ptr(out), op, ptr(y), pitch_of(y), ptr(mean), ptr(invstd),
                                    ptr(gamma), ptr(sums_apply), n_global, m, c, int(relu), ptr(dy), c,
                                    ptr(g_out), c if g_out is not None else 0, ptr(amax_dy), ptr(scale), ptr(shift), st))
    tm.__exit__()
    if dy_pl:
        mark_planes(dy, dy_bound)   # the conv backward that receives dy reads it as planes (autograd hands the tensor on unchanged:
                                    # y has ONE consumer, this BatchNorm)
    elif amax_dy is not None:
        tag_amax(dy, amax_dy)       # the conv backward that receives dy reuses it (when autograd hands the tensor on unchanged)
    if training:
        dy._pylc_zero_colsum = True   # batch statistics: dy sums to zero over the rows of every channel (conv2d_backward: bias gradient)
    dgamma = dbeta = None
    if direct:
        _deliver_grad(gamma, tg)
        _deliver_grad(beta, tb)
    else:
        if needs[1]:
            if tg is not None:
                tg.copy_(local_sums[:c])
                dgamma = _deliver_grad(gamma, tg)
            else:
                dgamma = local_sums[:c].clone()
        if needs[2]:
            if tb is not None:
                tb.copy_(local_sums[c:])
                dbeta = _deliver_grad(beta, tb)
            else:
                dbeta = local_sums[c:].clone()
    if g_out is not None and a_bound is not None:
        mark_planes(g_out, a_bound)      # the residual's gradient leaves in dout's format and scale
    if res_is_dout:
        g_out = dout
    if park_masked:
        lk.masked = (dout, mask)
    if g_out is not None and lk is not None and lk.armed and lk.buf is None and tuple(g_out.shape) == tuple(y.shape):
        lk.buf = g_out         # the first conv's dgrad accumulates into it and returns it as x's whole gradient
        g_out = None
    return (dy, dgamma, dbeta, None, None, g_out) + (None,) * (len(needs) - 6)


class FrozenBnActFn(torch.autograd.Function):
    """out = [dropout](act(y*scale + shift (+ residual))) with the coefficients of the RUNNING statistics, inside a training graph: the
    BatchNorm of a fine-tuning step (DeepLab(freeze_bn=True)).  The statistics are constants, so nothing is reduced in the forward, no
    running statistic is written, no collective is issued, one value per channel is legal, and the backward is ONE pass
    (pylc_bn_frozen_bwd: dy = gamma invstd g, with [dgamma | dbeta] from the same walk) instead of the training mode's two.
    All operands and results are fp32."""

    @staticmethod
    def forward(ctx, y, gamma, beta, running_mean, running_var, residual, relu, eps, want_amax, res_link, drop, into):
        L.init()
        ctx.set_materialize_grads(False)
        ctx.res_link = res_link
        y = as_nhwc(y)
        b, c, h, w = y.shape
        m = b * h * w
        dev = y.device
        st = stream()
        yp = pitch_of(y)
        coef = torch.empty(4 * c, device=dev)            # mean | invstd | scale | shift
        mean, invstd, scale, shift = coef[:c], coef[c:2 * c], coef[2 * c:3 * c], coef[3 * c:]
        # every call: gamma and beta move with each optimiser step
        check(lib.pylc_bn_eval_coeffs_full(ptr(running_mean), ptr(running_var), ptr(gamma), ptr(beta), eps, c,
                                           ptr(scale), ptr(shift), ptr(mean), ptr(invstd), st))
        drop_p, drop_seed = drop if drop is not None else (0.0, 0)
        res = as_nhwc(residual) if residual is not None else None
        if into is not None:               # write into channels [c0, c0 + c) of a caller-owned concat buffer: into = ([buffer], c0)
            out, op_ = concat_slice(into, b, c, h, w, 'bn_act')
        else:
            out, op_ = empty_nhwc(b, c, h, w, dev), c
        amax = amax_slot(dev) if want_amax else None
        needs_grad = any(ctx.needs_input_grad)
        mask = None          # a ReLU behind a residual add: one bit per element for the backward (bn.hip "1-bit ReLU masks")
        if relu and res is not None and c % 8 == 0 and drop_p == 0 and needs_grad and not _runtime.no_relu_bits:
            mask = torch.empty(m * c // 8, dtype=torch.uint8, device=dev)
        tm = _bn_time('frozen_apply%s%s%s' % ('+res' if res is not None else '', '+bits' if mask is not None else '', '+drop' if drop_p > 0 else ''),
                      m, c, m * c * (8 + (4 if res is not None else 0) + (0.125 if mask is not None else 0)))
        tm.__enter__()
        if drop_p > 0 or mask is not None:
            ex = _bn_extra(drop_p=drop_p, drop_seed=drop_seed)
            if mask is not None:
                ex.relu_mask = ptr(mask)
            check(lib.pylc_bn_apply_ex(ptr(y), yp, ptr(scale), ptr(shift), ptr(res), pitch_of(res) if res is not None else 0,
                                       ptr(out), op_, m, c, int(relu), ptr(amax), C.byref(ex), st))
        else:
            check(lib.pylc_bn_apply(ptr(y), yp, ptr(scale), ptr(shift), ptr(res), pitch_of(res) if res is not None else 0,
                                    ptr(out), op_, m, c, int(relu), ptr(amax), st))
        tm.__exit__()
        # y is read again for the sums (a parameter takes a gradient) or for a ReLU mask recomputed from it; `out` only as the mask of
        # a residual ReLU that left no bits
        mask_out = relu and res is not None and mask is None
        need_y = ctx.needs_input_grad[1] or ctx.needs_input_grad[2] or (relu and res is None)
        ctx.save_for_backward(y if (needs_grad and need_y) else None, out if (needs_grad and mask_out) else None, coef, mask)
        ctx.cfg = (bool(relu), res is not None, (b, c, h, w))
        ctx.g_param, ctx.b_param = gamma, beta
        ctx.want_amax = want_amax
        ctx.drop = (drop_p, drop_seed)
        if want_amax:
            ctx.mark_non_differentiable(amax)
            return out, amax
        return out

    @staticmethod
    def backward(ctx, dout, *_unused):
        if dout is None:
            return (None,) * 12
        y, out, coef, mask = ctx.saved_tensors
        relu, has_res, (b, c, h, w) = ctx.cfg
        gamma, beta = ctx.g_param, ctx.b_param
        dout = as_nhwc(dout)
        m = b * h * w
        dev = dout.device
        st = stream()
        mean, invstd = coef[:c], coef[c:2 * c]
        scale, shift = (coef[2 * c:3 * c], coef[3 * c:]) if (relu and out is None and mask is None) else (None, None)
        want_sums = ctx.needs_input_grad[1] or ctx.needs_input_grad[2]
        # [dgamma | dbeta] go straight into the flat gradient arena when gamma/beta own adjacent slots there
        tg, tb = _grad_target(gamma), _grad_target(beta)
        direct = (tg is not None and tb is not None and tb.data_ptr() == tg.data_ptr() + 4 * c
                  and ctx.needs_input_grad[1] and ctx.needs_input_grad[2])
        sums = ws = None
        if want_sums:
            sums = torch.as_strided(tg, (2 * c,), (1,)) if direct else torch.empty(2 * c, device=dev)
            ws = torch.empty(lib.pylc_bn_workspace_floats(m, c), device=dev)
        drop_p, drop_seed = ctx.drop
        lk = ctx.res_link
        armed = lk is not None and lk.armed
        want_res = has_res and ctx.needs_input_grad[5]
        # without a ReLU (and without dropout) the residual's gradient IS dout: hand the tensor on (unless a conv is going to accumulate
        # its dgrad into the buffer, which must then be ours)
        res_is_dout = want_res and not relu and drop_p == 0 and not armed
        g_out = empty_nhwc(b, c, h, w, dev) if (want_res and not res_is_dout) else None
        dy = empty_nhwc(b, c, h, w, dev)
        amax_dy = amax_slot(dev) if ctx.want_amax else None
        ex = None
        if drop_p > 0 or mask is not None:
            ex = _bn_extra(drop_p=drop_p, drop_seed=drop_seed)
            if mask is not None:
                ex.relu_mask = ptr(mask)
        msrc = 0.125 if mask is not None else (4 if out is not None else 0)
        tm = _bn_time('frozen_bwd%s%s' % ('' if want_sums else '(no sums)', '+gres' if g_out is not None else ''), m, c,
                      m * c * (8 + (4 if y is not None else 0) + msrc + (4 if g_out is not None else 0)))
        tm.__enter__()
        check(lib.pylc_bn_frozen_bwd(ptr(dout), pitch_of(dout), ptr(out), pitch_of(out) if out is not None else 0,
                                     ptr(y), pitch_of(y) if y is not None else 0, ptr(mean), ptr(invstd), ptr(gamma), m, c, int(relu),
                                     ptr(dy), c, ptr(g_out), c if g_out is not None else 0, ptr(amax_dy), ptr(scale), ptr(shift),
                                     ptr(sums), ptr(ws), C.byref(ex) if ex is not None else None, st))
        tm.__exit__()
        if amax_dy is not None:
            tag_amax(dy, amax_dy)       # the conv backward that receives dy reuses it
        dgamma = dbeta = None
        if direct:
            _deliver_grad(gamma, tg)
            _deliver_grad(beta, tb)
        else:
            if ctx.needs_input_grad[1]:
                if tg is not None:
                    tg.copy_(sums[:c])
                    dgamma = _deliver_grad(gamma, tg)
                else:
                    dgamma = sums[:c].clone()
            if ctx.needs_input_grad[2]:
                if tb is not None:
                    tb.copy_(sums[c:])
                    dbeta = _deliver_grad(beta, tb)
                else:
                    dbeta = sums[c:].clone()
        if res_is_dout:
            g_out = dout
        if g_out is not None and armed and lk.buf is None and lk.masked is None:
            lk.buf = g_out           # the first conv's dgrad accumulates into it and returns it as x's whole gradient
            g_out = None
        return (dy if ctx.needs_input_grad[0] else None, dgamma, dbeta, None, None, g_out) + (None,) * 6


def proj_pair_eligible(fuse, training, frozen, group, clamp_eps, drop, channels, fp32_y, relu_bits, needs_grad=True):
    """May relu(bn3(y3) + bn_ds(y_ds)) of a projection bottleneck run as ONE node (BnPairFn)?  Plain values only (no tensors, no device):
    the runtime knob; both BatchNorms in training mode and not frozen; no SyncBN group; torch's 1/sqrt(var + eps) (not the clamped form);
    no fused dropout; C % 8 == 0 and the 1-bit ReLU masks on (the pair's backward reads the mask); y3 and y_ds fp32 (not the one-plane half
    activations of precision mode 3); a graph that takes gradients (the mask is what the forward leaves for it).  Anything else takes the
    two-node path."""
    return bool(fuse and training and not frozen and group is None and not clamp_eps and drop is None and channels % 8 == 0 and fp32_y
                and relu_bits and needs_grad)


def _pair_finalize(y, yp, pre_sums, gamma, beta, running_mean, running_var, eps, momentum, coef, res_amax, bound, m, c, st):
    """The statistics -> coefficients step of bn_act_forward for a training-mode BatchNorm without a group: the same launches."""
    mean, invstd, scale, shift = coef[:c], coef[c:2 * c], coef[2 * c:3 * c], coef[3 * c:]
    refine_y = y if _runtime.bn_refine else None
    partial = pre_sums if (pre_sums is not None and pre_sums.dim() == 2 and pre_sums.shape[1] == 2 * c) else None
    kshift = getattr(partial, '_pylc_shift', None) if partial is not None else None
    if partial is not None:
        check(lib.pylc_bn_finalize_from_partial_ex(ptr(partial), partial.shape[0], float(m), c, ptr(gamma), ptr(beta), eps, momentum, 0,
                                                   ptr(running_mean), ptr(running_var), ptr(mean), ptr(invstd), ptr(scale), ptr(shift),
                                                   ptr(res_amax), 1.0, ptr(bound), ptr(refine_y), yp, m, ptr(kshift), st))
    else:
        sums = torch.empty(2 * c, device=y.device)                     # [sum | sumsq]
        ws = torch.empty(lib.pylc_bn_workspace_floats(m, c), device=y.device)
        check(lib.pylc_bn_stats(ptr(y), m, c, yp, ptr(sums), ptr(ws), st))
        check(lib.pylc_bn_finalize_ex(ptr(sums), float(m), c, ptr(gamma), ptr(beta), eps, momentum, 0, ptr(running_mean), ptr(running_var),
                                      ptr(mean), ptr(invstd), ptr(scale), ptr(shift), ptr(res_amax), 1.0, ptr(bound), ptr(refine_y), yp, m,
                                      None, st))


def _pair_param_grads(ctx, gi, bi, gamma, beta, tg, tb, direct, sums, c):
    """[dgamma | dbeta] of one BatchNorm of the pair, delivered as bn_act_backward delivers them."""
    dgamma = dbeta = None
    if direct:
        _deliver_grad(gamma, tg)
        _deliver_grad(beta, tb)
        return None, None
    if ctx.needs_input_grad[gi]:
        if tg is not None:
            tg.copy_(sums[:c])
            dgamma = _deliver_grad(gamma, tg)
        else:
            dgamma = sums[:c].clone()
    if ctx.needs_input_grad[bi]:
        if tb is not None:
            tb.copy_(sums[c:])
            dbeta = _deliver_grad(beta, tb)
        else:
            dbeta = sums[c:].clone()
    return dgamma, dbeta


class BnPairFn(torch.autograd.Function):
    """out = relu(BN3(y) + BNds(y2)): the tail of a projection bottleneck (resnet.py:36-51 with a downsample branch) as ONE node, training
    mode, batch statistics, no group.  Both BatchNorms are finalised exactly as BnActFn does it (coefficients, running statistics, variance
    refinement); the shortcut's normalised tensor and the residual gradient relu'(out) dout are formed in registers (pylc_bn_*_pair) and
    never written: the results are bit for bit those of the two BnActFn nodes, the range bound of a plane output included (the maximum of
    the shortcut's normalised values is taken by one read pass over y2, pylc_bn_affine_amax)."""

    @staticmethod
    def forward(ctx, y, y2, gamma, beta, running_mean, running_var, gamma2, beta2, running_mean2, running_var2, eps, momentum, eps2, momentum2,
                pre_sums, pre_sums2, want_amax, out_planes, dy_planes, dy_planes2):
        L.init()
        ctx.set_materialize_grads(False)
        y, y2 = as_nhwc(y), as_nhwc(y2)
        b, c, h, w = y.shape
        if tuple(y2.shape) != (b, c, h, w) or c % 8:
            raise L.PylcError('bn_act_pair: shapes %s / %s (need equal shapes, C %% 8 == 0)' % (tuple(y.shape), tuple(y2.shape)))
        m = b * h * w
        dev = y.device
        st = stream()
        yp, yp2 = pitch_of(y), pitch_of(y2)
        if m == 1:
            raise ValueError('Expected more than 1 value per channel when training, got input size %s' % (tuple(y.shape),))
        out_planes = bool(out_planes and planes_ok(c, m) and m >= _core.PLANES_MIN_PIXELS)
        coef, coef2 = torch.empty(4 * c, device=dev), torch.empty(4 * c, device=dev)            # mean | invstd | scale | shift
        bound = amax_slot(dev) if out_planes else None
        _pair_finalize(y2, yp2, pre_sums2, gamma2, beta2, running_mean2, running_var2, eps2, momentum2, coef2, None, None, m, c, st)
        res_amax = None
        if out_planes:
            # the residual's part of the output bound: max |y2 * scale2 + shift2|, the number the two-node path measures while it writes the
            # shortcut's output -- one read of y2 (4 B per element), so that the plane scale of the block output is that path's
            res_amax = amax_slot(dev)
            tm = _bn_time('apply_range+proj', m, c, m * c * 4)
            tm.__enter__()
            check(lib.pylc_bn_affine_amax(ptr(y2), yp2, ptr(coef2[2 * c:3 * c]), ptr(coef2[3 * c:]), m, c, ptr(res_amax), st))
            tm.__exit__()
        _pair_finalize(y, yp, pre_sums, gamma, beta, running_mean, running_var, eps, momentum, coef, res_amax, bound, m, c, st)
        out = empty_nhwc(b, c, h, w, dev)
        amax = amax_slot(dev) if (want_amax and not out_planes) else None
        mask = torch.empty(m * c // 8, dtype=torch.uint8, device=dev)
        tm = _bn_time('apply+res+bits+proj', m, c, m * c * (4 + (2 * nplanes() if out_planes else 4) + 4 + 0.125))
        tm.__enter__()
        ex = _bn_extra()
        ex.relu_mask = ptr(mask)
        if out_planes:
            ex.out_planes, ex.out_plane_stride, ex.out_bound = ptr(out), pstride(m, c), ptr(bound)
        tw = L.BnTwin()
        tw.y, tw.y_pitch, tw.scale, tw.shift = ptr(y2), yp2, ptr(coef2[2 * c:3 * c]), ptr(coef2[3 * c:])
        check(lib.pylc_bn_apply_pair(ptr(y), yp, ptr(coef[2 * c:3 * c]), ptr(coef[3 * c:]), None if out_planes else ptr(out), c, m, c, ptr(amax),
                                     C.byref(ex), C.byref(tw), st))
        tm.__exit__()
        ctx.save_for_backward(y, y2, coef, coef2, mask)
        ctx.params = (gamma, beta, gamma2, beta2)
        ctx.want_amax = want_amax
        ctx.dy_pl = bool(dy_planes and planes_ok(c, m) and yp == c)
        ctx.dy_pl2 = bool(dy_planes2 and planes_ok(c, m) and yp2 == c)
        if out_planes:
            ctx.mark_non_differentiable(bound)
            return out, bound
        if want_amax:
            ctx.mark_non_differentiable(amax)
            return out, amax
        return out

    @staticmethod
    def backward(ctx, dout, *_unused):
        if dout is None:
            return (None,) * 20
        y, y2, coef, coef2, mask = ctx.saved_tensors
        gamma, beta, gamma2, beta2 = ctx.params
        dout = as_nhwc(dout)
        b, c, h, w = y.shape
        m = b * h * w
        dev = y.device
        st = stream()
        yp, yp2 = pitch_of(y), pitch_of(y2)
        n = float(m)
        # [dgamma | dbeta] of each BatchNorm go straight into the flat gradient arena when its gamma / beta own adjacent slots there
        tg, tb, tg2, tb2 = _grad_target(gamma), _grad_target(beta), _grad_target(gamma2), _grad_target(beta2)
        direct = (tg is not None and tb is not None and tb.data_ptr() == tg.data_ptr() + 4 * c
                  and ctx.needs_input_grad[2] and ctx.needs_input_grad[3])
        direct2 = (tg2 is not None and tb2 is not None and tb2.data_ptr() == tg2.data_ptr() + 4 * c
                   and ctx.needs_input_grad[6] and ctx.needs_input_grad[7])
        sums = torch.as_strided(tg, (2 * c,), (1,)) if direct else torch.empty(2 * c, device=dev)
        sums2 = torch.as_strided(tg2, (2 * c,), (1,)) if direct2 else torch.empty(2 * c, device=dev)
        ws = torch.empty(lib.pylc_bn_workspace_floats(m, c), device=dev)
        ws2 = torch.empty(lib.pylc_bn_workspace_floats(m, c), device=dev)
        dy_pl, dy_pl2 = ctx.dy_pl, ctx.dy_pl2
        g_amax = amax_slot(dev) if (dy_pl or dy_pl2) else None
        dy_bound = amax_slot(dev) if dy_pl else None
        dy_bound2 = amax_slot(dev) if dy_pl2 else None
        ex = _bn_extra()
        ex.relu_mask, ex.g_amax = ptr(mask), ptr(g_amax)
        tw = L.BnTwin()
        tw.y, tw.y_pitch, tw.mean, tw.invstd, tw.gamma = ptr(y2), yp2, ptr(coef2[:c]), ptr(coef2[c:2 * c]), ptr(gamma2)
        tw.sums, tw.workspace, tw.dy_bound_out = ptr(sums2), ptr(ws2), ptr(dy_bound2)
        # one walk over dout, the mask bits, y and y2 (12 1/8 B per element) where the two nodes read (dout, bits, y) and (g, y2)
        tm = _bn_time('bwd_reduce(+sums)+proj', m, c, m * c * (12 + 0.125))
        tm.__enter__()
        check(lib.pylc_bn_bwd_reduce_pair(ptr(dout), pitch_of(dout), ptr(y), yp, ptr(coef[:c]), ptr(coef[c:2 * c]), m, c, ptr(sums), ptr(ws),
                                          ptr(gamma), n, C.byref(ex), ptr(dy_bound), C.byref(tw), st))
        tm.__exit__()
        dy, dy2 = empty_nhwc(b, c, h, w, dev), empty_nhwc(b, c, h, w, dev)
        amax_dy = amax_slot(dev) if (ctx.want_amax and not dy_pl) else None
        amax_dy2 = amax_slot(dev) if (ctx.want_amax and not dy_pl2) else None
        tm = _bn_time('bwd_apply+proj', m, c, m * c * (12 + 0.125 + (2 * nplanes() if dy_pl else 4) + (2 * nplanes() if dy_pl2 else 4)))
        tm.__enter__()
        if dy_pl:
            ex.dy_planes, ex.dy_plane_stride, ex.dy_bound = ptr(dy), pstride(m, c), ptr(dy_bound)
        if dy_pl2:
            tw.dy_planes, tw.dy_plane_stride, tw.dy_bound = ptr(dy2), pstride(m, c), ptr(dy_bound2)
        else:
            tw.dy = ptr(dy2)
        tw.dy_pitch, tw.amax_dy = c, ptr(amax_dy2)
        check(lib.pylc_bn_bwd_apply_pair(ptr(dout), pitch_of(dout), ptr(y), yp, ptr(coef[:c]), ptr(coef[c:2 * c]), ptr(gamma), ptr(sums), n, m, c,
                                         None if dy_pl else ptr(dy), c, ptr(amax_dy), C.byref(ex), C.byref(tw), st))
        tm.__exit__()
        for t, pl, bnd, amx in ((dy, dy_pl, dy_bound, amax_dy), (dy2, dy_pl2, dy_bound2, amax_dy2)):
            if pl:
                mark_planes(t, bnd)     # the conv backward that receives it reads it as planes (each y has ONE consumer, this node)
            elif amx is not None:
                tag_amax(t, amx)
            t._pylc_zero_colsum = True    # batch statistics: each dy sums to zero over the rows of every channel
        dgamma, dbeta = _pair_param_grads(ctx, 2, 3, gamma, beta, tg, tb, direct, sums, c)
        dgamma2, dbeta2 = _pair_param_grads(ctx, 6, 7, gamma2, beta2, tg2, tb2, direct2, sums2, c)
        return (dy, dy2, dgamma, dbeta, None, None, dgamma2, dbeta2) + (None,) * 12


def bn_act_pair(y, gamma, beta, running_mean, running_var, eps, momentum, y2, gamma2, beta2, running_mean2, running_var2, eps2, momentum2,
                out_planes=False):
    """relu(BN(y) + BN2(y2)) of a projection bottleneck as one node (BnPairFn); callers check proj_pair_eligible first.  Tags and marks the
    output as bn_act does."""
    pre, pre2 = getattr(y, '_pylc_sums', None), getattr(y2, '_pylc_sums', None)
    dy_ok = not _runtime.no_planes and _runtime.planes_dy
    dy_pl, dy_pl2 = bool(getattr(y, '_pylc_dy_pl', False)) and dy_ok, bool(getattr(y2, '_pylc_dy_pl', False)) and dy_ok
    ranged = ranges_needed()
    out_planes = bool(out_planes) and ranged and not _runtime.no_planes
    args = (y, y2, gamma, beta, running_mean, running_var, gamma2, beta2, running_mean2, running_var2, eps, momentum, eps2, momentum2, pre, pre2)
    if not ranged:
        return BnPairFn.apply(*args, False, False, False, False)
    out, tagv = BnPairFn.apply(*args, True, out_planes, dy_pl, dy_pl2)
    if is_planes_candidate(out_planes, True, y):
        mark_planes(out, tagv)
    else:
        tag_amax(out, tagv)
    return out


def _drive_collectives(gens, group):
    """Run BatchNorm generators (bn_act_forward / bn_act_backward) in lockstep: whatever they yield in one round is all-reduced as ONE message
    (a lone generator: its own tensor, no copy).  Returns their return values."""
    results = [None] * len(gens)
    live = list(range(len(gens)))
    while live:
        msgs = []
        for i in list(live):
            try:
                msgs.append(next(gens[i]))
            except StopIteration as e:
                results[i] = e.value
                live.remove(i)
        if len(msgs) == 1:
            _runtime.sync_all_reduce(msgs[0], group)
        elif msgs:
            flat = torch.cat([t.reshape(-1) for t in msgs])        # one dtype per round: fp64 moments (forward), fp32 sums (backward)
            _runtime.sync_all_reduce(flat, group)
            o = 0
            for t in msgs:
                t.copy_(flat[o:o + t.numel()].view_as(t))
                o += t.numel()
    return results


class GroupBnActFn(torch.autograd.Function):
    """Several BatchNorm(+act) layers over PARALLEL branches (the ASPP's five, aspp.py:73-86) as one autograd node, so that under SyncBN their
    statistics travel in one all-reduce per direction instead of one per layer: the members run BnActFn's own drivers (same kernels, same order
    per layer) with the collectives of a round concatenated.  apply(group, n, nargs, *member_args) -> the members' outputs, flattened."""

    @staticmethod
    def forward(ctx, group, n, nargs, *flat):
        ctx.set_materialize_grads(False)
        needs = ctx.needs_input_grad[3:]
        results = _drive_collectives([bn_act_forward(needs[i * nargs:(i + 1) * nargs], *flat[i * nargs:(i + 1) * nargs]) for i in range(n)], group)
        saved, outs, nondiff = [], [], []
        ctx.members, ctx.group = [], group      # per member: (its BnState, its needs_input_grad, its slice of the saved tensors, its number of outputs)
        for i, (r, sv, st, nd) in enumerate(results):
            r = r if isinstance(r, tuple) else (r,)
            ctx.members.append((st, needs[i * nargs:(i + 1) * nargs], slice(len(saved), len(saved) + len(sv)), len(r)))
            saved.extend(sv)
            outs.extend(r)
            nondiff.extend(nd)
        return _adapt(ctx, (tuple(outs), saved, None, nondiff))

    @staticmethod
    def backward(ctx, *grads):
        saved = ctx.saved_tensors
        gens, k = [], 0
        for st, needs, sl, nout in ctx.members:
            gens.append(bn_act_backward(st, saved[sl], needs, grads[k]))
            k += nout
        results = _drive_collectives(gens, ctx.group)
        return (None, None, None) + tuple(g for r in results for g in r)


def _bn_args(y, gamma, beta, running_mean, running_var, residual=None, relu=True, training=True, eps=1e-5, momentum=0.1, group=None,
             clamp_eps=False, res_link=None, out_planes=False, drop=None, into=None, sole=False, defer=False, frozen=False):
    """bn_act's keyword arguments (a frozen layer never gets here) -> BnActFn's positional list."""
    ranged = ranges_needed()
    pre = getattr(y, '_pylc_sums', None) if training else None
    dy_pl = ranged and bool(getattr(y, '_pylc_dy_pl', False)) and not _runtime.no_planes and _runtime.planes_dy
    out_planes = bool(out_planes) and ranged and not _runtime.no_planes and into is None
    if drop is not None and not (training and _runtime.dropout_enabled and drop[0] > 0):
        drop = None
    defer = bool(defer and _runtime.defer_bn_apply and training and out_planes and residual is None and drop is None
                 and nplanes() == 1 and half_dw() and is_planes(y))
    return [y, gamma, beta, running_mean, running_var, residual, relu, training, eps, momentum, group, clamp_eps, pre, ranged, res_link,
            out_planes, drop, dy_pl, into, sole, defer]


def _bn_result(res, args):
    """What a BnActFn node (or a member of a GroupBnActFn node) returned for the positional list `args` -> the marked or tagged output."""
    y, relu, training, ranged, out_planes = args[0], args[6], args[7], args[13], args[15]
    if not ranged:
        return res
    if len(res) == 3:
        # deferred apply: `out` aliases y (the BatchNorm's INPUT, one fp16 plane); what a consumer needs to form the output travels here.
        # NOT marked as planes: only DwConv3x3Fn understands it (anything else goes through ops.materialize_deferred)
        out, bound, coef = res
        out._pylc_defer = (coef, bool(relu), planes_amax(y), bound, out._version)
        return out
    out, tagv = res
    if is_planes_candidate(out_planes, training, y):
        mark_planes(out, tagv)
    else:
        tag_amax(out, tagv)
    return out


def bn_act_group(specs, group):
    """bn_act for the BatchNorms of parallel branches, as one node (GroupBnActFn).  specs: one dict per layer with the keyword arguments of
    bn_act (y, gamma, beta, running_mean, running_var + options); returns the outputs in order.  Frozen members (frozen=True) exchange
    nothing: each is its own bn_act call."""
    if any(sp.get('frozen') for sp in specs):
        rest = [sp for sp in specs if not sp.get('frozen')]
        outs = iter(bn_act_group(rest, group) if rest else [])
        return [bn_act(**sp) if sp.get('frozen') else next(outs) for sp in specs]
    lists = [_bn_args(**dict(sp, group=group, defer=False)) for sp in specs]
    outs = GroupBnActFn.apply(group, len(lists), len(lists[0]), *[a for args in lists for a in args])
    n = len(outs) // len(lists)          # outputs per member: out alone, or (out, its range tag) with ranged arithmetic
    return [_bn_result(outs[i * n] if n == 1 else outs[i * n:(i + 1) * n], args) for i, args in enumerate(lists)]


def bn_act(y, gamma, beta, running_mean, running_var, residual=None, relu=True, training=True, eps=1e-5, momentum=0.1,
           group=None, clamp_eps=False, res_link=None, out_planes=False, drop=None, into=None, sole=False, defer=False, frozen=False):
    """frozen: the BatchNorm of a fine-tuning step (FrozenBnActFn) -- running statistics as constants inside a training graph, the fused
    dropout still applied, no statistic written, no collective; fp32 in and out (out_planes / defer / sole, and a producer's wish for a
    plane dy, are ignored)."""
    if frozen:
        if lib.pylc_get_conv_precision() == 3:
            raise L.PylcError('frozen BatchNorm (freeze_bn) is not available in conv precision mode 3: its half activations are scaled with '
                              'range bounds taken from batch statistics, which a frozen BatchNorm does not compute')
        if drop is not None and not (_runtime.dropout_enabled and drop[0] > 0):
            drop = None
        ranged = ranges_needed()
        res = FrozenBnActFn.apply(y, gamma, beta, running_mean, running_var, residual, relu, eps, ranged, res_link, drop, into)
        if ranged:
            out, tagv = res
            tag_amax(out, tagv)
            return out
        return res
    args = _bn_args(y, gamma, beta, running_mean, running_var, residual, relu, training, eps, momentum, group, clamp_eps, res_link, out_planes,
                    drop, into, sole, defer)
    return _bn_result(BnActFn.apply(*args), args)


def materialize_deferred(x):
    """The fp16-plane output of a BatchNorm whose apply pass was deferred (bn_act(defer=True)), for a consumer that cannot apply it itself:
    the pass pylc_bn_apply_ex would have made (no autograd: callers are inside a Function's forward)."""
    coef, relu, y_bound, bound, _ = x._pylc_defer
    b, c, h, w = x.shape
    m = b * h * w
    out = empty_nhwc(b, c, h, w, x.device)
    ex = _bn_extra()
    ex.y_half_bound = ptr(y_bound)
    ex.out_planes, ex.out_plane_stride, ex.out_bound = ptr(out), pstride(m, c), ptr(bound)
    check(lib.pylc_bn_apply_ex(ptr(x), c, ptr(coef[2 * c:3 * c]), ptr(coef[3 * c:]), None, 0, None, c, m, c, int(relu), None, C.byref(ex), stream()))
    return mark_planes(out, bound)


def is_planes_candidate(out_planes, training, y):
    """Mirror of bn_act_forward's decision whether the output was written as planes."""
    b, c, h, w = y.shape
    return bool(out_planes and training and planes_ok(c, b * h * w) and b * h * w >= _core.PLANES_MIN_PIXELS)


__all__ = [n for n in dir() if not n.startswith('__')]      # everything, underscore helpers included: the package re-exports it (pylc_amd/ops/__init__.py)
