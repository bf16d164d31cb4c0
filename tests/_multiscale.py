"""The multi-scale ensemble of csrc/multiscale.hip stated in float64 numpy: what tests/test_cpu_multiscale.py and
tests/test_multiscale_gpu.py compare the kernels and the inference paths against.  Not a test module."""
import numpy as np


def axis_np(n, ns):
    """The coordinate rule along one axis, destination length n, source length ns: s = (i + 0.5) * (ns / n) - 0.5 clamped to
    [0, ns - 1]; (i0 = floor(s), i1 = min(i0 + 1, ns - 1), f = s - i0)."""
    s = (np.arange(n) + 0.5) * (float(ns) / n) - 0.5
    s = np.clip(s, 0.0, float(ns - 1))
    i0 = np.floor(s).astype(np.int64)
    return i0, np.minimum(i0 + 1, ns - 1), s - i0


def resize_bilinear_np(img, oh, ow):
    """img [..., H, W] (any dtype) -> float64 [..., oh, ow]: half-pixel-centre bilinear interpolation without antialiasing,
    (1-fy)*((1-fx)*v00 + fx*v01) + fy*((1-fx)*v10 + fx*v11)."""
    img = np.asarray(img, dtype=np.float64)
    y0, y1, fy = axis_np(oh, img.shape[-2])
    x0, x1, fx = axis_np(ow, img.shape[-1])
    fy = fy[:, None]
    top = (1 - fx) * img[..., y0[:, None], x0[None, :]] + fx * img[..., y0[:, None], x1[None, :]]
    bot = (1 - fx) * img[..., y1[:, None], x0[None, :]] + fx * img[..., y1[:, None], x1[None, :]]
    return (1 - fy) * top + fy * bot


def ensemble_np(probs_list, sizes, weights, h, w):
    """probs_list[k]: the probabilities [C, sizes[k][0], sizes[k][1]] of scale k (float64, e.g. tests/_blend.py:blend_mean_np's); every one is resampled
    to h x w and their mean with `weights` is taken.  Returns (probs [C, h, w] float64, uint8 first-maximum mask)."""
    assert len(probs_list) == len(sizes) == len(weights)
    ens = np.zeros((probs_list[0].shape[0], h, w))
    for p, (hs, ws), wgt in zip(probs_list, sizes, weights):
        assert p.shape[1:] == (hs, ws)
        ens += wgt * resize_bilinear_np(p, h, w)
    ens /= float(sum(weights))
    return ens, ens.argmax(0).astype(np.uint8)


# ---- the kernel cases of tests/test_multiscale_gpu.py (the CPU suite checks that the statement decides them) --------------------------------
BASE, OUT = (37, 53), 16                        # tests/test_blend_gpu.py's image and output tile: the last tile row and column are clamped
STRIDES = (16, 8, 5)
CLASSES = (2, 3, 9, 16)
SCALE_SETS = {'near': [(28, 40), (37, 53), (46, 66)], 'far': [(19, 27), (74, 106)]}       # scales 0.75 / 1 / 1.25 and 0.5 / 2 of BASE
WEIGHT_SETS = ((1.0, 1.0, 1.0), (2.0, 1.0, 0.5))
SEED = 1000                                     # a base at which the statement leaves at most one pixel of a case undecided
MARGIN = 2e-6                                   # a pixel is decided when the statement's top two probabilities differ by more


def case_logits(c, stride, name):
    """{size: (l0, l1)}: for every size of SCALE_SETS[name] the fp32 logits 3 * randn of the two ensemble members (l1: the mirrored
    windows') on that size's tile grid; one member is l0 alone."""
    from tests.test_cpu_overlap_tile import overlap_origins
    rs = np.random.RandomState(SEED + 100 * c + stride + (0 if name == 'near' else 50))
    got = {}
    for hs, ws in SCALE_SETS[name]:
        n = len(overlap_origins(hs, OUT, stride)) * len(overlap_origins(ws, OUT, stride))
        got[(hs, ws)] = tuple((rs.standard_normal((n, c, OUT, OUT)) * 3).astype(np.float32) for _ in range(2))
    return got


def decided(probs):
    top2 = np.sort(probs, axis=0)[-2:]
    return (top2[1] - top2[0]) > MARGIN
