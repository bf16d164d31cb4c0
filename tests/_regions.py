"""The statement of pylc_amd.regions in numpy, and the masks its tests run on.  numpy only: the GPU tests must
not depend on a library nobody has checked on the GPU machine.

Region: a maximal set of pixels of one value connected through 4- or 8-neighbours; pixels equal to ignore_index belong to none.
Label: the minimum linear index y * W + x of the pixel's region, -1 at ignored pixels.  sizes[r]: the pixel count of the region rooted
at r, 0 elsewhere.  Sieve: every pixel of a region smaller than min_size takes a constant, or the value of the region's largest
neighbour of at least min_size (4-neighbour contact; ties to the smaller root: the maximum of size << 32 | (0xFFFFFFFF - root))."""
import numpy as np


def _pairs(h, w, connectivity):
    """slices (a, b) of the two ends of every neighbour pair: b = a + (dy, dx)"""
    offs = [(0, 1), (1, 0)] + ([(1, 1), (1, -1)] if connectivity == 8 else [])
    out = []
    for dy, dx in offs:
        a = (slice(0, h - dy), slice(max(0, -dx), w - max(0, dx)))
        b = (slice(dy, h), slice(max(0, dx), w + min(0, dx)))
        out.append((a, b))
    return out


def label_ref(mask, connectivity=4, ignore_index=None):
    """int32 [H, W] labels.  Minimum propagation over same-value neighbour pairs alternated with pointer jumping (L = L[L]) until nothing
    changes.  A label is always the index of a pixel of the same region, and both steps only lower it.  After the jumps every label is a
    root (L[L] == L); a pair whose ends still differ then lowers the larger ROOT to the smaller one, which carries the minimum to every
    pixel under that root at the next jumps: the number of rounds is logarithmic even on a serpentine.  At the fixed point every pair
    agrees, so a region holds one label, and that is its minimum index, whose own label can never have dropped below itself."""
    assert connectivity in (4, 8)
    m = np.ascontiguousarray(mask)
    h, w = m.shape
    valid = np.ones((h, w), bool) if ignore_index is None else m != ignore_index
    idx = np.arange(h * w, dtype=np.int64).reshape(h, w)
    ia, ib = [], []
    for a, b in _pairs(h, w, connectivity):
        same = (m[a] == m[b]) & valid[a] & valid[b]
        ia.append(idx[a][same])
        ib.append(idx[b][same])
    ia, ib = np.concatenate(ia), np.concatenate(ib)
    lab = idx.reshape(-1).copy()
    while ia.size:
        ra, rb = lab[ia], lab[ib]
        differ = ra != rb
        if not differ.any():
            break
        ia, ib, ra, rb = ia[differ], ib[differ], ra[differ], rb[differ]       # a pair that agrees once agrees for good
        np.minimum.at(lab, np.maximum(ra, rb), np.minimum(ra, rb))
        while True:                                    # pointer jumping to the end: each jump at least halves a chain
            nxt = lab[lab]
            if np.array_equal(nxt, lab):
                break
            lab = nxt
    lab = lab.reshape(h, w)
    lab[~valid] = -1
    return lab.astype(np.int32)


def sizes_ref(labels):
    flat = np.asarray(labels).reshape(-1)
    return np.bincount(flat[flat >= 0], minlength=flat.size).astype(np.int32)


def sieve_ref(mask, min_size, connectivity=4, fill='neighbour', ignore_index=None):
    """One sieve pass: (new uint8 mask, number of pixels whose value was replaced by a different one)."""
    m = np.ascontiguousarray(mask)
    h, w = m.shape
    lab = label_ref(m, connectivity, ignore_index).astype(np.int64)
    size = sizes_ref(lab).astype(np.int64)
    size_px = np.where(lab >= 0, size[np.maximum(lab, 0)], 0)
    small = (lab >= 0) & (size_px < min_size)
    out = m.copy()
    if fill != 'neighbour':
        out[small] = int(fill)
        return out, int((out != m).sum())
    best = np.zeros(h * w, dtype=np.uint64)
    for a, b in _pairs(h, w, 4):                       # 4-neighbour contact for both connectivities
        for p, q in ((a, b), (b, a)):
            cond = small[p] & (lab[q] >= 0) & (lab[q] != lab[p]) & (size_px[q] >= min_size)
            key = (size_px[q].astype(np.uint64) << np.uint64(32)) | (np.uint64(0xFFFFFFFF) - lab[q].astype(np.uint64))
            np.maximum.at(best, lab[p][cond], key[cond])
    win = best[np.maximum(lab, 0)]
    take = small & (win > 0)
    root = (np.uint64(0xFFFFFFFF) - (win & np.uint64(0xFFFFFFFF))).astype(np.int64)
    out[take] = m.reshape(-1)[root[take]]
    return out, int((out != m).sum())


def region_table_ref(mask, connectivity=4, ignore_index=None):
    lab = label_ref(mask, connectivity, ignore_index)
    size = sizes_ref(lab)
    root = np.flatnonzero(size > 0)
    return {'root': root, 'cls': np.asarray(mask).reshape(-1)[root], 'size': size[root]}


# ---- masks ------------------------------------------------------------------------------------------------------------------------------
def noise(h, w, c, seed=0):
    return np.random.default_rng(seed).integers(0, c, (h, w)).astype(np.uint8)


def _box(a, r):
    """box filter of radius r with edge clamping (cumulative sums), float64"""
    for ax in (0, 1):
        n = a.shape[ax]
        idx = np.clip(np.arange(-r, n + r), 0, n - 1)
        c = np.cumsum(np.take(a, idx, axis=ax), axis=ax)
        c = np.concatenate([np.zeros_like(np.take(c, [0], axis=ax)), c], axis=ax)
        a = np.take(c, np.arange(2 * r + 1, n + 2 * r + 1), axis=ax) - np.take(c, np.arange(0, n), axis=ax)
    return a


def blobs(h, w, c=9, seed=0, radius=6, noise_frac=0.0):
    """class = argmax of c box-filtered noise fields (twice filtered: smooth blobs), then noise_frac of the pixels replaced by random
    classes"""
    rng = np.random.default_rng(seed)
    f = np.stack([_box(_box(rng.standard_normal((h, w)), radius), radius) for _ in range(c)])
    m = f.argmax(0).astype(np.uint8)
    if noise_frac:
        hit = rng.random((h, w)) < noise_frac
        m[hit] = rng.integers(0, c, int(hit.sum())).astype(np.uint8)
    return m


def constant(h, w, v=3):
    return np.full((h, w), v, np.uint8)


def checkerboard(h, w):
    return ((np.arange(h)[:, None] + np.arange(w)[None, :]) & 1).astype(np.uint8)


def stripes_h(h, w):
    return np.broadcast_to((np.arange(h)[:, None] & 1).astype(np.uint8), (h, w)).copy()


def stripes_v(h, w):
    return np.broadcast_to((np.arange(w)[None, :] & 1).astype(np.uint8), (h, w)).copy()


def serpentine(h, w):
    """a 1-pixel path of 1s from pixel 0: every even row in full, joined alternately at the right and the left end"""
    m = np.zeros((h, w), np.uint8)
    m[0::2] = 1
    for k, y in enumerate(range(1, h, 2)):
        m[y, w - 1 if k % 2 == 0 else 0] = 1
    return m


def spiral(h, w):
    """a 1-pixel square spiral of 1s from the top-left corner inwards: the walk turns right when the pixel two ahead is taken, which leaves a
    1-pixel gap between its turns"""
    m = np.zeros((h, w), np.uint8)
    y, x, d = 0, 0, 0
    m[0, 0] = 1
    dirs = ((0, 1), (1, 0), (0, -1), (-1, 0))
    while True:
        for _ in range(2):
            dy, dx = dirs[d]
            ny, nx, fy, fx = y + dy, x + dx, y + 2 * dy, x + 2 * dx
            free = 0 <= ny < h and 0 <= nx < w and not m[ny, nx] and not (0 <= fy < h and 0 <= fx < w and m[fy, fx])
            if free:
                break
            d = (d + 1) % 4
        if not free:
            return m
        y, x = ny, nx
        m[y, x] = 1


def diagonal(h, w):
    """a diagonal line of 1s on a background of 0s: min(h, w) regions at connectivity 4, one at 8"""
    m = np.zeros((h, w), np.uint8)
    k = np.arange(min(h, w))
    m[k, k] = 1
    return m


def specks(h, w, seed=0, n=12):
    """a uniform two-class field (left half 1, right half 2) with single pixels and 2-pixel slivers of class 3 planted in it, one of them
    on the class border; returns (mask, clean field)"""
    clean = np.ones((h, w), np.uint8)
    clean[:, w // 2:] = 2
    m = clean.copy()
    rng = np.random.default_rng(seed)
    for _ in range(n):
        y, x = int(rng.integers(0, h)), int(rng.integers(0, w - 1))
        m[y, x] = 3
        if rng.random() < 0.5:
            m[y, x + 1] = 3
    m[h // 2, w // 2 - 1] = 3
    return m, clean


def patterns(h, w):
    """name -> mask, every pattern that fits h x w"""
    out = {'noise2': noise(h, w, 2, 1), 'noise16': noise(h, w, 16, 2), 'constant': constant(h, w), 'checkerboard': checkerboard(h, w),
           'stripes_h': stripes_h(h, w), 'stripes_v': stripes_v(h, w), 'diagonal': diagonal(h, w)}
    if h >= 3 and w >= 3:
        out['serpentine'] = serpentine(h, w)
        out['spiral'] = spiral(h, w)
        out['specks'] = specks(h, w, 3)[0]
    if h >= 16 and w >= 16:
        out['blobs9'] = blobs(h, w, 9, 4, radius=3, noise_frac=0.02)
    return out
