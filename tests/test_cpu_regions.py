"""CPU suite (-m "not gpu") for pylc_amd.regions: the numpy statement of the rules (tests/_regions.py, what the GPU tests compare with
bit for bit) against a pure-Python flood fill and scipy.ndimage, hand-worked sieve cases, the bindings of the three entry points and the
argument errors that need no device."""
import numpy as np
import pytest
import torch

from tests import _regions as R


def flood_ref(mask, connectivity, ignore_index):
    """labels by a pure-Python flood fill in raster order: the first unlabelled pixel met is its region's minimum index"""
    h, w = mask.shape
    lab = np.full((h, w), -2, np.int32)
    nb = [(-1, 0), (1, 0), (0, -1), (0, 1)] + ([(-1, -1), (-1, 1), (1, -1), (1, 1)] if connectivity == 8 else [])
    for y in range(h):
        for x in range(w):
            if lab[y, x] != -2:
                continue
            if ignore_index is not None and mask[y, x] == ignore_index:
                lab[y, x] = -1
                continue
            lab[y, x] = y * w + x
            stack = [(y, x)]
            while stack:
                cy, cx = stack.pop()
                for dy, dx in nb:
                    ny, nx = cy + dy, cx + dx
                    if 0 <= ny < h and 0 <= nx < w and lab[ny, nx] == -2 and mask[ny, nx] == mask[y, x]:
                        lab[ny, nx] = y * w + x
                        stack.append((ny, nx))
    return lab


@pytest.mark.parametrize('connectivity', [4, 8])
@pytest.mark.parametrize('ignore_index', [None, 0, 255])
def test_label_ref_matches_flood_fill(connectivity, ignore_index):
    rng = np.random.default_rng(7)
    masks = [rng.integers(0, c, (h, w)).astype(np.uint8) for h, w, c in ((1, 1, 2), (1, 9, 2), (8, 1, 2), (5, 7, 3), (12, 12, 2), (12, 11, 3),
                                                                          (9, 12, 4), (12, 12, 1))]
    masks += [m for hw in ((12, 12), (7, 11), (3, 3)) for m in R.patterns(*hw).values()]
    if ignore_index == 255:
        masks = [np.where(rng.random(m.shape) < 0.15, 255, m).astype(np.uint8) for m in masks]
    for m in masks:
        got = R.label_ref(m, connectivity, ignore_index)
        assert got.dtype == np.int32 and np.array_equal(got, flood_ref(m, connectivity, ignore_index)), m


def test_issue_statements():
    """what the issue states about the rules"""
    lab = R.label_ref(R.serpentine(65, 65))
    assert (lab[R.serpentine(65, 65) == 1] == 0).all()                                     # one region with root 0
    cb = R.checkerboard(8, 8)
    assert len(np.unique(R.label_ref(cb, 4))) == 64 and len(np.unique(R.label_ref(cb, 8))) == 2
    # a uniform two-class field with planted specks is restored, except the speck on the class border: to the larger side
    clean = np.ones((40, 60), np.uint8)
    clean[:, 29:] = 2                                                                     # 29 columns of 1s, 31 of 2s
    m = clean.copy()
    for y, x in ((3, 4), (3, 5), (10, 50), (25, 12), (26, 12), (39, 59), (0, 17), (20, 28)):
        m[y, x] = 3
    out, n = R.sieve_ref(m, 4)
    want = clean.copy()
    want[20, 28] = 2
    assert np.array_equal(out, want) and n == 8


@pytest.mark.parametrize('connectivity', [4, 8])
def test_label_ref_matches_scipy(connectivity):
    ndi = pytest.importorskip('scipy.ndimage')
    structure = np.ones((3, 3), int) if connectivity == 8 else None
    for name, m in R.patterns(64, 96).items():
        for ign in (None, 0):
            want = np.full(m.shape, -1, np.int64)
            idx = np.arange(m.size).reshape(m.shape)
            for v in np.unique(m):
                if v == ign:
                    continue
                comp, n = ndi.label(m == v, structure=structure)
                roots = np.asarray(ndi.minimum(idx, comp, np.arange(1, n + 1))).astype(np.int64)
                want[comp > 0] = roots[comp[comp > 0] - 1]
            assert np.array_equal(R.label_ref(m, connectivity, ign), want), (name, ign)


# ---- hand-worked sieve cases (also run on the device: tests/test_regions_gpu.py) ----------------------------------------------------------
def hand_cases():
    """name -> (mask, kwargs of the sieve, expected mask, expected n_changed)"""
    cases = {}
    # a speck on the border of two unequal sides: the larger side (2: 12 pixels against 7) takes it
    m = np.array([[1, 1, 2, 2, 2],
                  [1, 3, 2, 2, 2],
                  [1, 1, 2, 2, 2],
                  [1, 1, 2, 2, 2]], np.uint8)
    w = m.copy()
    w[1, 1] = 2
    cases['unequal_sides'] = (m, dict(min_size=2), w, 1)
    # between two EQUAL sides (7 and 7 pixels): the side with the earlier root (1, root 0) wins
    m = np.array([[1, 1, 3, 2, 2],
                  [1, 1, 1, 2, 2],
                  [1, 1, 2, 2, 2]], np.uint8)
    w = m.copy()
    w[0, 2] = 1
    cases['equal_sides'] = (m, dict(min_size=2), w, 1)
    # a small region enclosed by small regions is kept; its small neighbours, touching the large background, go
    m = np.zeros((7, 7), np.uint8)
    m[2:5, 2:5] = 1
    m[3, 3] = 2
    w = np.zeros((7, 7), np.uint8)
    w[3, 3] = 2
    cases['enclosed_by_small'] = (m, dict(min_size=9), w, 8)
    # a constant fill counts only the pixels whose value differs: the speck of 5s goes, the speck of 0s "changes" to 0
    m = np.full((4, 6), 7, np.uint8)
    m[0, 0] = 5
    m[3, 5] = 0
    w = np.full((4, 6), 7, np.uint8)
    w[0, 0] = 0
    w[3, 5] = 0
    cases['constant_fill'] = (m, dict(min_size=2, fill=0), w, 1)
    # min_size = H*W + 1: every region is small, none has a large neighbour, nothing changes under the neighbour rule
    m = np.array([[1, 1, 2], [3, 1, 2], [3, 3, 2]], np.uint8)
    cases['all_small'] = (m, dict(min_size=10), m.copy(), 0)
    # ... and everything becomes the constant under a constant fill
    cases['all_small_constant'] = (m, dict(min_size=10, fill=255), np.full((3, 3), 255, np.uint8), 9)
    # an ignore value inside the class range: 0 is no region, lends no value and is not changed; the speck enclosed by 0s and the
    # edge is kept, the speck touching the 1s is taken by them
    m = np.array([[2, 0, 1, 1, 1],
                  [0, 0, 1, 3, 1],
                  [1, 1, 1, 1, 1],
                  [0, 1, 1, 1, 1]], np.uint8)
    w = m.copy()
    w[1, 3] = 1
    cases['ignore_in_range'] = (m, dict(min_size=2, ignore_index=0), w, 1)
    # diagonal specks: two 1-pixel regions at connectivity 4 (both go), one 2-pixel region at connectivity 8 (stays at min_size 2)
    m = np.zeros((5, 5), np.uint8)
    m[1, 1] = m[2, 2] = 4
    cases['diagonal_conn4'] = (m, dict(min_size=2, connectivity=4), np.zeros((5, 5), np.uint8), 2)
    cases['diagonal_conn8'] = (m, dict(min_size=2, connectivity=8), m.copy(), 0)
    return cases


@pytest.mark.parametrize('name', sorted(hand_cases()))
def test_sieve_ref_hand_cases(name):
    m, kw, want, n_want = hand_cases()[name]
    out, n = R.sieve_ref(m, **kw)
    assert out.dtype == np.uint8 and np.array_equal(out, want), (out, want)
    assert n == n_want


def test_sieve_ref_cleans_noise():
    """the blob map of the issue: the sieve raises the agreement with the clean map"""
    clean = R.blobs(300, 400, 9, 11, radius=10)
    rng = np.random.default_rng(3)
    hit = rng.random(clean.shape) < 0.02
    noisy = clean.copy()
    noisy[hit] = rng.integers(0, 9, int(hit.sum()))
    out, n = R.sieve_ref(noisy, 16)
    assert n > 0 and (noisy == clean).mean() < 0.983 and (out == clean).mean() > 0.99


# ---- the package side that needs no device -------------------------------------------------------------------------------------------------
def test_bindings_exist():
    import ctypes
    from pylc_amd import lib as L
    dll = ctypes.CDLL(L.LIB_PATH)
    for name, nargs in (('pylc_label_regions', 7), ('pylc_region_sizes', 4), ('pylc_sieve_regions', 12)):
        assert hasattr(dll, name)
        assert len(L.SIGNATURES[name][1]) == nargs and L.SIGNATURES[name][0] is ctypes.c_int


def test_entry_point_errors_without_gpu():
    """argument validation happens on the host before any launch"""
    from pylc_amd.lib import lib
    one = 1 << 12                                     # any non-NULL address: nothing is dereferenced
    assert lib.pylc_label_regions(None, 4, 4, 4, -1, one, None) == 1
    assert b'NULL' in lib.pylc_last_error()
    assert lib.pylc_label_regions(one, 4, 4, 6, -1, one, None) == 1
    assert lib.pylc_label_regions(one, 1 << 16, 1 << 15, 4, -1, one, None) == 1
    assert lib.pylc_label_regions(one, 4, 0, 4, -1, one, None) == 1
    assert lib.pylc_label_regions(one, 4, 4, 4, 256, one, None) == 1
    assert lib.pylc_region_sizes(one, 0, one, None) == 1
    assert lib.pylc_region_sizes(one, 1 << 31, one, None) == 1
    assert lib.pylc_sieve_regions(one, one, one, 4, 4, 0, -1, -1, one, 2 * one, None, None) == 1
    assert lib.pylc_sieve_regions(one, one, one, 4, 4, 2, -1, 256, one, 2 * one, None, None) == 1
    assert lib.pylc_sieve_regions(one, one, one, 4, 4, 2, -1, -1, one, one, None, None) == 1
    assert b'alias' in lib.pylc_last_error()


def test_python_argument_errors():
    from pylc_amd import regions
    import pylc_amd
    assert pylc_amd.regions is regions
    m = torch.zeros((4, 5), dtype=torch.uint8)
    with pytest.raises(TypeError):
        regions.label_regions(m.to(torch.int64))
    with pytest.raises(TypeError):
        regions.sieve(m.float(), 4)
    with pytest.raises(TypeError):
        regions.region_sizes(m)
    with pytest.raises(ValueError):
        regions.label_regions(m[None])                                # not 2-D
    with pytest.raises(ValueError):
        regions.label_regions(m, connectivity=6)
    with pytest.raises(ValueError):
        regions.label_regions(m, ignore_index=256)
    with pytest.raises(ValueError):
        regions.sieve(m, 4, fill='ignore')                            # without an ignore_index
    with pytest.raises(ValueError):
        regions.sieve(m, 4, fill='nearest')
    with pytest.raises(ValueError):
        regions.sieve(m, 4, fill=300)
    with pytest.raises(ValueError):
        regions.sieve(m, 4, iterations=0)
    with pytest.raises(ValueError):
        regions.region_table(m, connectivity=5)
    for call in (lambda: regions.label_regions(m), lambda: regions.sieve(m, 4), lambda: regions.sieve(m, 1),
                 lambda: regions.region_sizes(m.to(torch.int32)), lambda: regions.region_table(m)):
        with pytest.raises(ValueError, match='device'):               # a host tensor: there is no CPU path
            call()
