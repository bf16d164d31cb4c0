"""The yardstick of the guided-filter refinement, numpy only: the integer luma, the fp64 statement of the
definition in include/pylc_hip.h, a float32 model with the kernel's operation order (direct separable sums: x ascending within a row,
then rows ascending), the generator of the GPU test's cases and the synthetic border scene.  The CPU suite (tests/test_cpu_refine.py)
pins the statement against independent forms and measures the model's distance from it; the GPU suite (tests/test_refine_gpu.py)
compares the kernels with the statement within 4 x that distance."""
import numpy as np

# ---- the GPU test's cases ---------------------------------------------------------------------------------------------------------------
# the issue's sizes, then the kernel's own edges: strips of 64 columns (63 / 64 / 65 are among the issue's), row blocks of 64, 128 and 256
SIZES = [(1, 1), (1, 37), (37, 1), (5, 7), (17, 16), (33, 65), (64, 64), (65, 63), (127, 130), (96, 131), (150, 140), (600, 515),
         (63, 66), (128, 20), (129, 9), (255, 5), (256, 3), (257, 2)]
RADII = [1, 2, 4, 8, 16, 33, 64]
CLASSES = [2, 3, 9, 16]
EPSS = [1e-6, 1e-4, 1e-2]

# The largest |float32 model - fp64 statement| over SIZES x RADII x CLASSES x EPSS (measure_gap32 over all of them, run once; the CPU
# suite re-measures a subset and checks that it stays below): of q, and of the coefficients scaled by (var + eps) -- the error of a
# grows as 1 / eps in near-flat windows, that of q does not.  The GPU tolerances are 4 x these.
GAP32_Q = 6.97e-6         # measured 6.966e-6: 37 x 1, 2 classes, r = 1, eps = 1e-6 (windows of 3 pixels, var of 1e-3)
GAP32_A = 5.80e-7         # measured 5.799e-7
GAP32_B = 5.45e-7         # measured 5.445e-7
# near ties: at most NEAR_TIE_SHARE of a case's pixels have an fp64 top-two margin of q below NEAR_TIE_MARGIN (>= 8 x tol_q; the mask
# comparison leaves out the pixels below 8 x tol_q).  case_reference draws its inputs so.
NEAR_TIE_MARGIN = 2.5e-4
NEAR_TIE_SHARE = 1e-3


def tolerances():
    """(tol_q, tol_a, tol_b) of the GPU comparison"""
    return 4 * GAP32_Q, 4 * GAP32_A, 4 * GAP32_B


def luma_np(img):
    """uint8 [ch,H,W], ch 1 or 3 -> uint8 [H,W]: (77 R + 150 G + 29 B + 128) >> 8 in integers; one channel is its own guide"""
    img = np.asarray(img)
    assert img.dtype == np.uint8 and img.ndim == 3 and img.shape[0] in (1, 3)
    if img.shape[0] == 1:
        return img[0].copy()
    v = img.astype(np.int64)
    return ((77 * v[0] + 150 * v[1] + 29 * v[2] + 128) >> 8).astype(np.uint8)


# ---- window sums ---------------------------------------------------------------------------------------------------------------------------
def _axis_sum_direct(x, r, axis):
    """sum over the 2r+1 window clipped to the array along `axis`, by adding the window's values in ascending order (zeros outside)"""
    x = np.moveaxis(x, axis, -1)
    n = x.shape[-1]
    pad = np.zeros(x.shape[:-1] + (n + 2 * r,), x.dtype)
    pad[..., r:r + n] = x
    out = np.zeros(x.shape, x.dtype)
    for k in range(max(0, r - n + 1), min(2 * r, r + n - 1) + 1):          # the other shifts add zeros only
        out += pad[..., k:k + n]
    return np.moveaxis(out, -1, axis)


def _axis_sum_prefix(x, r, axis):
    """the same from a prefix sum (fp64 or integers only: the big cases of the statement, where the direct form takes too long)"""
    x = np.moveaxis(x, axis, -1)
    n = x.shape[-1]
    c = np.concatenate([np.zeros(x.shape[:-1] + (1,), x.dtype), np.cumsum(x, axis=-1)], axis=-1)
    i = np.arange(n)
    out = c[..., np.minimum(i + r, n - 1) + 1] - c[..., np.maximum(i - r, 0)]
    return np.moveaxis(out, -1, axis)


def box_sum(x, r, prefix=False):
    """[..., H, W] -> the sums over the (2r+1)^2 windows clipped to the image: along x first, then along y"""
    f = _axis_sum_prefix if prefix else _axis_sum_direct
    return f(f(x, r, -1), r, -2)


def window_count(h, w, r):
    """int64 [h, w]: the pixel count of every clipped window"""
    def axis(n):
        i = np.arange(n)
        return np.minimum(i + r, n - 1) - np.maximum(i - r, 0) + 1
    return np.outer(axis(h), axis(w)).astype(np.int64)


# ---- the statement (fp64) and the model (float32) -------------------------------------------------------------------------------------------
def guide_sums(g, r):
    """the exact integer sums of a uint8 guide: (n, S_g, S_gg, D = n S_gg - S_g^2), int64 [H, W]"""
    gi = np.asarray(g).astype(np.int64)
    n = window_count(gi.shape[0], gi.shape[1], r)
    sg, sgg = box_sum(gi, r, prefix=True), box_sum(gi * gi, r, prefix=True)      # integers: the prefix form is exact
    return n, sg, sgg, n * sgg - sg * sg


def statement(p, g, r, eps, prefix=False, sums=None):
    """The definition in fp64.  p [C,H,W] (taken to fp64 as it is), g uint8 [H,W].  Returns a dict: a, b, q [C,H,W], var, n [H,W], mask
    (first maximum of q), conf.  sums: stage_sums(p, g, r, np.float64, prefix) of the same inputs, to share it between values of eps."""
    n, sg, sgg, d, sp, sgp = sums if sums is not None else stage_sums(p, g, r, np.float64, prefix)
    nf = n.astype(np.float64)
    var = d / (65025.0 * nf * nf)
    cov = (nf * sgp - sg * sp) / (255.0 * nf * nf)
    a = np.where(d == 0, 0.0, cov / (var + eps))
    b = sp / nf - a * (sg / (255.0 * nf))
    q = box_sum(a, r, prefix) / nf * (np.asarray(g).astype(np.float64) / 255.0) + box_sum(b, r, prefix) / nf
    return {'a': a, 'b': b, 'q': q, 'var': var, 'n': n, 'mask': np.argmax(q, axis=0).astype(np.uint8),
            'conf': np.clip(q.max(axis=0), 0.0, 1.0)}


def stage_sums(p, g, r, dtype, prefix=False):
    """(n, S_g, S_gg, D, S_p, S_gp): the integer sums and the sums of p and g * p in `dtype`"""
    n, sg, sgg, d = guide_sums(g, r)
    p = np.asarray(p).astype(dtype)
    gp = (np.asarray(g).astype(dtype) * p).astype(dtype)
    return n, sg, sgg, d, box_sum(p, r, prefix), box_sum(gp, r, prefix)


def model32(p, g, r, eps, sums=None):
    """The float32 model: the kernel's operations in the kernel's order.  Returns a dict a, b, q (float32)."""
    f = np.float32
    n, sg, sgg, d, sp, sgp = sums if sums is not None else stage_sums(p, g, r, f)
    nf, sgf = n.astype(f), sg.astype(f)
    with np.errstate(all='ignore'):
        var = d.astype(f) / (f(65025) * nf * nf)
        cov = (nf * sgp - sgf * sp) / (f(255) * nf * nf)
        mean_i = sgf / (f(255) * nf)
        a = np.where(d == 0, f(0), cov / (var + f(eps))).astype(f)
        b = np.where(d == 0, sp / nf, sp / nf - a * mean_i).astype(f)
        q = (box_sum(a, r) / nf) * (np.asarray(g).astype(f) / f(255)) + box_sum(b, r) / nf
    assert a.dtype == f and b.dtype == f and q.dtype == f
    return {'a': a, 'b': b, 'q': q}


# ---- inputs --------------------------------------------------------------------------------------------------------------------------------
def case_guide(h, w):
    """uint8 [h, w]: texture (a ramp plus noise of a few grey levels), a saturated slab (255) in the upper left and a black slab (0) in the
    lower right -- flat windows of both kinds at the small radii, windows that straddle a slab's edge at all of them"""
    rng = np.random.default_rng(1000003 * h + 1009 * w)
    yy, xx = np.mgrid[0:h, 0:w]
    g = 60 + 120 * (xx / max(w - 1, 1)) + 40 * np.sin(yy / 7.0) + rng.normal(0, 12, (h, w))
    g = np.clip(np.rint(g), 0, 255).astype(np.uint8)
    g[:h // 3, :w // 2] = 255
    g[h - h // 3:, w // 2:] = 0
    return g


def case_probs(h, w, c, salt=0):
    """float32 [c, h, w], softmax-like: a background led by class 0 with five rectangles (a third of the area) led by other classes --
    at the small radii the borders of the rectangles are decided pixel by pixel, at the large ones the background wins with a margin
    (window means of unstructured noise, or of regions of similar area, tie there over whole curves) -- blocky logit noise and pixel
    noise on top, softmax over the classes in fp64.  salt: another draw of the noise (case_reference)."""
    rng = np.random.default_rng(7919 * h + 104729 * w + c + 15485863 * salt)
    cell = 6
    yy, xx = np.mgrid[0:h, 0:w]
    region = np.zeros((h, w), int)
    for k in range(5):
        y0, x0 = (0.1 + 0.5 * (k % 2)) * h, (0.05 + (k // 2) / 3.0) * w
        region[(yy >= y0) & (yy < y0 + 0.3 * h) & (xx >= x0) & (xx < x0 + 0.22 * w)] = 1 + k % (c - 1)
    coarse = rng.normal(0, 1.5, (c, -(-h // cell), -(-w // cell)))
    z = np.repeat(np.repeat(coarse, cell, axis=1), cell, axis=2)[:, :h, :w] + rng.normal(0, 0.7, (c, h, w))
    z += 4.0 * (region[None] == np.arange(c)[:, None, None])
    z -= z.max(axis=0, keepdims=True)
    e = np.exp(z)
    return (e / e.sum(axis=0, keepdims=True)).astype(np.float32)


def top2_margin(q):
    """[C,H,W] -> [H,W]: the largest value minus the second largest"""
    s = np.sort(q, axis=0)
    return s[-1] - s[-2]


def case_reference(h, w, c, r):
    """For one (size, classes, radius): the inputs (g, p) and, for every eps of EPSS, the fp64 statement (the big size takes the prefix
    form).  The mask comparison leaves out pixels whose fp64 top-two margin is below 8 x tol_q; so that these stay rare in EVERY case --
    in an image of 37 pixels one is too many, and with windows that hold the whole image two classes tie on every pixel of one grey
    level -- the generator rejects a draw of p in which more than NEAR_TIE_SHARE of the pixels lie below NEAR_TIE_MARGIN at some eps, and
    takes the next salt.  Deterministic: the same case gives the same draw."""
    g = case_guide(h, w)
    prefix = h * w > 40000
    for salt in range(64):
        p = case_probs(h, w, c, salt)
        sums = stage_sums(p, g, r, np.float64, prefix)
        refs = {eps: statement(p, g, r, eps, prefix, sums) for eps in EPSS}
        if max(float((top2_margin(ref['q']) < NEAR_TIE_MARGIN).mean()) for ref in refs.values()) <= NEAR_TIE_SHARE:
            return g, p, refs
    raise AssertionError('no draw without near ties for %dx%d, %d classes, r=%d' % (h, w, c, r))


def measure_gap32(sizes=SIZES, radii=RADII, classes=CLASSES):
    """(gap_q, gap_a, gap_b): the largest |model32 - statement| of q and of the coefficients scaled by (var + eps) over the cases"""
    gq = ga = gb = 0.0
    for h, w in sizes:
        for c in classes:
            for r in radii:
                g, p, refs = case_reference(h, w, c, r)
                s32 = stage_sums(p, g, r, np.float32)
                for eps, ref in refs.items():
                    got = model32(p, g, r, eps, s32)
                    scale = ref['var'] + eps
                    gq = max(gq, float(np.abs(got['q'] - ref['q']).max()))
                    ga = max(ga, float((np.abs(got['a'] - ref['a']) * scale).max()))
                    gb = max(gb, float((np.abs(got['b'] - ref['b']) * scale).max()))
    return gq, ga, gb


# ---- the synthetic border scene --------------------------------------------------------------------------------------------------------------
def _blur(x, sigma):
    k = np.arange(-int(4 * sigma), int(4 * sigma) + 1)
    wgt = np.exp(-0.5 * (k / sigma) ** 2)
    wgt /= wgt.sum()
    for axis in (-1, -2):
        pad = [(0, 0)] * x.ndim
        pad[axis] = (len(k) // 2, len(k) // 2)
        xp = np.pad(x, pad, mode='edge')
        x = sum(wv * np.take(xp, np.arange(i, i + x.shape[axis]), axis=axis) for i, wv in enumerate(wgt))
    return x


def border_scene(h=96, w=128, shift=3, sigma=3.0, seed=5):
    """Three classes whose borders lie on image edges: grey levels 70 / 170 / 230 with noise of sigma 5.  Returns (guide uint8 [h,w],
    truth uint8 [h,w], p float32 [3,h,w]): p is the one-hot truth rolled by `shift` pixels along both axes and Gaussian-blurred with
    `sigma` -- a network's smooth, displaced borders."""
    rng = np.random.default_rng(seed)
    yy, xx = np.mgrid[0:h, 0:w]
    truth = np.ones((h, w), np.uint8)
    truth[xx < 45 + 6 * np.sin(yy / 12.0)] = 0
    truth[(yy > 60 + 5 * np.sin(xx / 15.0)) & (truth == 1)] = 2
    levels = np.array([70.0, 170.0, 230.0])
    g = np.clip(np.rint(levels[truth] + rng.normal(0, 5, (h, w))), 0, 255).astype(np.uint8)
    onehot = (truth[None] == np.arange(3)[:, None, None]).astype(np.float64)
    p = _blur(np.roll(onehot, (shift, shift), axis=(1, 2)), sigma)
    p /= p.sum(axis=0, keepdims=True)
    return g, truth, p.astype(np.float32)
