"""The pooling / resize yardstick of tests/_resize.py checked without a GPU: the bilinear model against
F.interpolate(align_corners=True) in fp64 (continuity bound for the float32 source coordinate) and against torch's own fp32 CPU result
(forward bound), its transpose against autograd, the adjoint identity, the max-pool model against F.max_pool2d(return_indices=True) with the
codes converted, and the global average pool's summation order inside its bound."""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

from tests import _resize as R

PAIRS = R.RESIZE_PAIRS_BWD


def _nchw(a, dtype):
    return torch.from_numpy(np.ascontiguousarray(a)).to(dtype).permute(0, 3, 1, 2)


def _nhwc(t):
    return t.permute(0, 2, 3, 1).contiguous().numpy()


def test_lerp_rule():
    i0, i1, w0, w1 = R.lerp_f32(np.arange(29), 8, 29)
    assert i0[0] == 0 and w1[0] == 0 and i0[-1] == 7 and i1[-1] == 7            # corners map to corners; at the border i1 == i0
    assert (i1 - i0 <= 1).all() and (w0 + w1 == 1).all()
    i0, i1, w0, w1 = R.lerp_f32(np.arange(4), 5, 1)                             # out == 1: scale 0, everything reads pixel 0
    assert not i0.any() and not w1.any()
    i0, i1, w0, w1 = R.lerp_f32(np.arange(8), 1, 8)                             # in == 1
    assert not i0.any() and not i1.any() and (w0 == 1).all()


@pytest.mark.parametrize('size,out', PAIRS)
def test_bilinear_model_against_torch(size, out):
    (H, W), (OH, OW) = size, out
    x = R.wide(H * 100 + OW, 2, H, W, 4)
    y64 = R.bilinear64(x, OH, OW)
    t64 = _nhwc(F.interpolate(_nchw(x, torch.float64), size=(OH, OW), mode='bilinear', align_corners=True))
    for c in range(4):                                                          # per channel: the scales differ by 2^12
        err = np.abs(y64[..., c] - t64[..., c]).max()
        assert err <= R.continuity_bound(x[..., c:c + 1], OH, OW), (c, err)
    bound = R.bilinear_fwd_bound(x, OH, OW)
    t32 = _nhwc(F.interpolate(_nchw(x, torch.float32), size=(OH, OW), mode='bilinear', align_corners=True)).astype(np.float64)
    assert (np.abs(t32 - y64) <= bound + 1e-300).all(), (np.abs(t32 - y64) / (bound + 1e-300)).max()
    m32 = R.bilinear_f32(x, OH, OW).astype(np.float64)
    assert (np.abs(m32 - y64) <= bound).all()


@pytest.mark.parametrize('size,out', PAIRS)
def test_bilinear_transpose_against_autograd_and_adjoint_identity(size, out):
    (H, W), (OH, OW) = size, out
    x = R.wide(H + OW, 2, H, W, 4)
    dy = R.wide(H + OW + 1, 2, OH, OW, 4)
    dx = R.bilinear_bwd64(dy, H, W)
    lhs, rhs = (dy.astype(np.float64) * R.bilinear64(x, OH, OW)).sum(), (dx * x.astype(np.float64)).sum()
    scale = (np.abs(dy.astype(np.float64)) * np.abs(R.bilinear64(np.abs(x), OH, OW))).sum()
    assert abs(lhs - rhs) <= 1e-13 * scale
    xt = _nchw(x, torch.float64).requires_grad_(True)
    F.interpolate(xt, size=(OH, OW), mode='bilinear', align_corners=True).backward(_nchw(dy, torch.float64))
    ag = _nhwc(xt.grad)
    # the float32 weights are off by at most d = 2u (n_in - 1) + u per output position and axis; an input pixel collects at most n_out of them
    Ah, Aw = R.lerp_matrix(H, OH)[0], R.lerp_matrix(W, OW)[0]
    dh, dw = (2 * (H - 1) + 1) * R.U, (2 * (W - 1) + 1) * R.U
    for c in range(4):
        tol = np.abs(dy[..., c]).max() * (dh * OH * np.abs(Aw).sum(0).max() + dw * OW * np.abs(Ah).sum(0).max()) * 2
        assert np.abs(ag[..., c] - dx[..., c]).max() <= tol
    for sep in (False, True):
        assert (R.bilinear_bwd_bound(dy, H, W, sep) >= 0).all()


@pytest.mark.parametrize('k,s,pad,H,W', [(3, 2, 1, 16, 16), (3, 2, 1, 15, 9), (3, 2, 1, 1, 7), (3, 2, 1, 2, 2), (2, 2, 0, 12, 12), (2, 2, 0, 21, 13),
                                         (2, 2, 0, 2, 3)])
def test_maxpool_model_against_torch(k, s, pad, H, W):
    x = R.pool_input(H + W, 2, H, W, 4)
    y, idx = R.maxpool_fwd(x, k, s, pad)
    ty, ti = F.max_pool2d(_nchw(x, torch.float32), k, s, pad, return_indices=True)
    assert np.array_equal(y.view(np.uint32), _nhwc(ty).view(np.uint32))
    OH, OW = y.shape[1:3]
    code = idx.astype(np.int64)
    h = np.arange(OH)[None, :, None, None] * s - pad + code // k
    w = np.arange(OW)[None, None, :, None] * s - pad + code % k
    assert np.array_equal(h * W + w, _nhwc(ti))
    dy = R.wide(3, 2, OH, OW, 4)
    dx, mag, cnt = R.maxpool_bwd64(dy, idx, H, W, k, s, pad)
    xt = _nchw(x[..., [0, 1, 3]], torch.float64).requires_grad_(True)              # (not the -inf channel: nothing to differentiate)
    F.max_pool2d(xt, k, s, pad).backward(_nchw(dy[..., [0, 1, 3]], torch.float64))
    assert np.abs(_nhwc(xt.grad) - dx[..., [0, 1, 3]]).max() <= 1e-12
    if k == 2:
        assert cnt.max() <= 1 and not R.maxpool_bwd_bound(mag, cnt).any()
        assert not dx[:, 2 * OH:].any() and not dx[:, :, 2 * OW:].any()


@pytest.mark.parametrize('hw', [1, 15, 16, 17, 127, 128, 129, 1000])
def test_gap_summation_order_inside_its_bound(hw):
    x = R.wide(hw, 3, hw, 8)
    ref = x.astype(np.float64).mean(1)
    t = _nhwc(_nchw(x.reshape(3, hw, 1, 8), torch.float64).mean((2, 3), keepdim=True)).reshape(3, 8)
    assert np.abs(ref - t).max() <= 1e-12 * np.abs(x).max()
    lanes = np.zeros((16, 3, 8), np.float32)
    for r in range(hw):
        lanes[r % 16] = lanes[r % 16] + x[:, r]
    s = lanes[0]
    for k in range(1, 16):
        s = s + lanes[k]
    got = s * (np.float32(1) / np.float32(hw))
    assert (np.abs(got.astype(np.float64) - ref) <= R.gap_fwd_bound(x)).all()
