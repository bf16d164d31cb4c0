"""The window-weighted mean-probability blend (csrc/blend.hip) stated in numpy: what tests/test_cpu_window.py and
tests/test_window_gpu.py compare the kernels and the inference paths against.  The blend itself in float64 from the float32 table
values; the per-axis sums and the finalizer's division as float32 models, operation for operation.  Not a test module."""
import numpy as np

from tests.test_cpu_overlap_tile import overlap_origins, softmax0


def window_f64(spec, out):
    """the named windows before rounding, float64 [out]"""
    i = np.arange(out, dtype=np.float64)
    if spec == 'uniform':
        return np.ones(out)
    if spec == 'hann':
        return 0.5 - 0.5 * np.cos(2.0 * np.pi * (i + 0.5) / out)
    sigma = 0.125 if spec == 'gauss' else spec[1]
    assert spec == 'gauss' or spec[0] == 'gauss'
    return np.exp(-0.5 * ((i - (out - 1) / 2.0) / (sigma * out)) ** 2)


def window_np(spec, out):
    """'uniform', 'hann', 'gauss' or ('gauss', sigma_frac): the float64 table rounded once to float32"""
    return window_f64(spec, out).astype(np.float32)


def random_table(seed, out):
    """a seeded asymmetric positive table, entries in [0.05, 1)"""
    return (0.05 + 0.95 * np.random.RandomState(seed).random_sample(out)).astype(np.float32)


def blend_window_np(members, h, w, out, stride, win, mirrored=None):
    """tests/_blend.py:blend_mean_np with a tile's softmax counted win2d = win[:, None] * win[None, :] times, the table indexed by the
    position inside the placed tile (a mirrored member's logits are mirrored back first): acc += win2d * softmax, cnt += win2d, both in
    float64 from the float32 table values.  Returns (probs [C, h, w] float64, uint8 first-maximum mask)."""
    rows, cols = overlap_origins(h, out, stride), overlap_origins(w, out, stride)
    mirrored = [k > 0 for k in range(len(members))] if mirrored is None else mirrored
    win = np.asarray(win)
    assert win.dtype == np.float32 and win.shape == (out,)
    win2d = win.astype(np.float64)[:, None] * win.astype(np.float64)[None, :]
    acc = np.zeros((members[0].shape[1], h, w))
    cnt = np.zeros((h, w))
    for logits, mir in zip(members, mirrored):
        assert logits.shape[0] == len(rows) * len(cols) and logits.shape[2:] == (out, out)
        for i, oy in enumerate(rows):
            for j, ox in enumerate(cols):
                t = logits[i * len(cols) + j].astype(np.float64)
                acc[:, oy:oy + out, ox:ox + out] += win2d * softmax0(t[:, :, ::-1] if mir else t)
                cnt[oy:oy + out, ox:ox + out] += win2d
    probs = acc / cnt
    return probs, probs.argmax(0).astype(np.uint8)


def window_sums_f32(win, n, out, stride):
    """float32 model of pylc_blend_window_sums along an axis of length n: for every coordinate the fp32 sum, from 0, of win[y - o_i] over
    the covering tiles in ascending index (the clamped last tile has the largest index and the largest origin, so it comes last)."""
    win = np.asarray(win, dtype=np.float32)
    sums = np.zeros(n, np.float32)
    for o in overlap_origins(n, out, stride):
        sums[o:o + out] = sums[o:o + out] + win
    return sums


def cover_counts(n, out, stride):
    """the integer number of tiles covering every coordinate of an axis"""
    cnt = np.zeros(n, np.int64)
    for o in overlap_origins(n, out, stride):
        cnt[o:o + out] += 1
    return cnt


def finalize_f32(acc, members, sy, sx):
    """float32 model of pylc_blend_finalize_w.  acc: float32 [h, w, >= C] sums (C = acc.shape[2] here), sy [h], sx [w] float32.
    fn = float32(members) * (sy[y] * sx[x]); p = acc / fn in float32; class = first maximum.  Returns (probs [C, h, w] float32, conf
    [h, w] float32, mask uint8)."""
    acc = np.asarray(acc, dtype=np.float32)
    fn = np.float32(members) * (np.asarray(sy, np.float32)[:, None] * np.asarray(sx, np.float32)[None, :])
    assert fn.dtype == np.float32
    probs = np.ascontiguousarray((acc / fn[:, :, None]).transpose(2, 0, 1))
    assert probs.dtype == np.float32
    mask = probs.argmax(0).astype(np.uint8)
    return probs, probs.max(0), mask


# ---- the cases of tests/test_window_gpu.py's comparison with the float64 statement (the CPU suite checks that the statement decides them) ----
H, W, OUT = 37, 53, 16                          # tests/test_blend_gpu.py's image and output tile: the last tile row and column are clamped
STRIDES = (16, 8, 5)
CLASSES = (2, 3, 9, 16)
WINDOWS = ('hann', 'gauss', 'random')           # 'random': random_table(TABLE_SEED, OUT), asymmetric
TABLE_SEED = 77
SEED = 5000
MARGIN = 1e-5                                   # a pixel is decided when the statement's top two probabilities differ by more


def case_window(name, out=OUT):
    return random_table(TABLE_SEED, out) if name == 'random' else window_np(name, out)


def case_logits(c, stride, h=H, w=W):
    """(l0, l1): the fp32 logits 3 * randn of the two ensemble members (l1: the mirrored windows') on the h x w tile grid"""
    n = len(overlap_origins(h, OUT, stride)) * len(overlap_origins(w, OUT, stride))
    rs = np.random.RandomState(SEED + 100 * c + stride + 7 * (h - H))
    return tuple((rs.standard_normal((n, c, OUT, OUT)) * 3).astype(np.float32) for _ in range(2))


def decided(probs, margin=MARGIN):
    top2 = np.sort(probs, axis=0)[-2:]
    return (top2[1] - top2[0]) > margin


# ---- the synthetic scene: what the window is for ------------------------------------------------------------------------------------------
def border_error_scene(seed=0, h=96, w=128, out=32, stride=16, border=4):
    """Two classes, a known truth (class 1 inside a disc and right of a slanted line), and per-tile logits that are right in the tile's
    interior (+-2 with noise of sigma 1.5) and pushed towards the wrong class within `border` pixels of each tile's edge (a bias of 3
    towards the wrong class: what zero padding does to a same-size network's border predictions).  Returns (truth [h, w] uint8,
    logits [n, 2, out, out] float32) on the overlap grid of (h, w, out, stride)."""
    rs = np.random.RandomState(seed)
    yy, xx = np.mgrid[0:h, 0:w]
    truth = (((yy - 40) ** 2 + (xx - 45) ** 2 < 30 ** 2) | (xx - 0.5 * yy > 90)).astype(np.uint8)
    rows, cols = overlap_origins(h, out, stride), overlap_origins(w, out, stride)
    ly, lx = np.mgrid[0:out, 0:out]
    edge = np.minimum(np.minimum(ly, out - 1 - ly), np.minimum(lx, out - 1 - lx)) < border
    logits = np.zeros((len(rows) * len(cols), 2, out, out), np.float32)
    for i, oy in enumerate(rows):
        for j, ox in enumerate(cols):
            t = truth[oy:oy + out, ox:ox + out].astype(np.float64)
            sign = 2 * t - 1                                            # +1 where class 1 is right
            z = sign * 2.0 + rs.standard_normal((out, out)) * 1.5
            z = np.where(edge, z - sign * 3.0, z)
            logits[i * len(cols) + j, 1] = (z / 2).astype(np.float32)
            logits[i * len(cols) + j, 0] = (-z / 2).astype(np.float32)
    return truth, logits
