"""Overlap-tile geometry of the U-Net inference path (pylc_amd.inference.overlap_tile_grid, UNet.output_size) and the numpy
restatement of its blend (mean of the covering tiles' softmax probabilities, argmax) that tests/test_unet_inference_gpu.py checks the
HIP stitch against -- itself checked here against a brute-force per-pixel loop.  No GPU needed."""
import numpy as np
import pytest


def overlap_origins(n, out, stride):
    """o_i = min(i*stride, n - out), i = 0 .. ceil((n - out) / stride): restated, not imported."""
    k = -(-(n - out) // stride)
    return [min(i * stride, n - out) for i in range(k + 1)]


def softmax0(a):
    a = a - a.max(0, keepdims=True)
    e = np.exp(a)
    return e / e.sum(0, keepdims=True)


def stitch_overlap_np(logits, h, w, out, stride):
    """logits [n, C, out, out] of the row-major tile grid -> (mean probabilities [C, h, w] in float64, uint8 argmax mask)."""
    rows, cols = overlap_origins(h, out, stride), overlap_origins(w, out, stride)
    assert logits.shape[0] == len(rows) * len(cols)
    acc = np.zeros((logits.shape[1], h, w))
    cnt = np.zeros((h, w))
    for i, oy in enumerate(rows):
        for j, ox in enumerate(cols):
            acc[:, oy:oy + out, ox:ox + out] += softmax0(logits[i * len(cols) + j].astype(np.float64))
            cnt[oy:oy + out, ox:ox + out] += 1
    probs = acc / cnt
    return probs, probs.argmax(0).astype(np.uint8)


GRIDS = [(150, 200, 68, 68), (150, 200, 68, 34), (150, 200, 68, 25), (324, 648, 324, 324), (331, 647, 324, 162), (700, 900, 324, 324),
         (68, 69, 68, 1), (3072, 4096, 324, 324)]


@pytest.mark.parametrize('h,w,out,stride', GRIDS)
def test_grid_covers_every_pixel_and_ends_at_the_edge(h, w, out, stride):
    from pylc_amd.inference import overlap_tile_grid
    rows, cols = overlap_tile_grid(h, w, out, stride, pad=94 if min(h, w) > 94 else 0)
    assert (rows, cols) == (overlap_origins(h, out, stride), overlap_origins(w, out, stride))
    for org, n in ((rows, h), (cols, w)):
        assert org[0] == 0 and min(org) >= 0
        assert org[-1] + out == n                                     # the last tile ends exactly at the edge
        assert all(b > a for a, b in zip(org, org[1:]))               # ascending, no duplicate tile
        assert all(b - a <= stride for a, b in zip(org, org[1:]))
        cover = np.zeros(n, np.int64)
        for o in org:
            cover[o:o + out] += 1
        assert cover.min() >= 1                                       # every pixel covered
        assert cover.max() <= -(-out // stride) + 1                   # the stitch kernel's per-axis bound


@pytest.mark.parametrize('k,out', [(1, 324), (3, 324), (4, 68), (9, 68)])
def test_fitted_size_gives_exact_tiles(k, out):
    from pylc_amd.inference import overlap_tile_grid
    rows, cols = overlap_tile_grid(k * out, (k + 1) * out, out, out, pad=0)
    assert rows == [i * out for i in range(k)] and cols == [i * out for i in range(k + 1)]


@pytest.mark.parametrize('h,w,out,stride,pad,what', [
    (67, 200, 68, 68, 0, 'need H, W >= out'),
    (200, 60, 68, 68, 0, 'need H, W >= out'),
    (94, 200, 68, 68, 94, 'pad < H'),
    (200, 90, 68, 68, 94, 'pad < W'),
    (150, 200, 68, 69, 94, 'need stride <= out'),
    (150, 200, 68, 0, 94, 'stride 0 < 1'),
    (150, 200, 68, -3, 94, 'stride -3 < 1'),
])
def test_invalid_geometry_raises(h, w, out, stride, pad, what):
    from pylc_amd.inference import overlap_tile_grid
    with pytest.raises(ValueError) as e:
        overlap_tile_grid(h, w, out, stride, pad=pad)
    assert what in str(e.value)


def test_unet_output_size_and_centred_tiles():
    import pylc_amd
    from pylc_amd.inference import overlap_tile_out
    net = pylc_amd.UNet(in_channels=3, n_classes=9)
    for tile, out in ((512, 324), (256, 68), (1024, 836), (572, 388), (252, 68)):
        assert net.output_size(tile) == out
    for tile in (512, 256, 1024):
        assert overlap_tile_out(net, tile, 94) == tile - 188
    for tile in (572, 252):                           # the output is not centred at pad = 94 in its window
        with pytest.raises(ValueError, match='centred'):
            overlap_tile_out(net, tile, 94)
    with pytest.raises(ValueError):
        net.output_size(100)                          # the feature maps vanish
    assert pylc_amd.UNet(in_channels=1, n_classes=2, padding=True).output_size(512) == 512


def test_numpy_stitch_matches_brute_force():
    rs = np.random.RandomState(12)
    for h, w, out, stride, c in ((23, 31, 8, 3, 5), (17, 20, 9, 9, 3), (9, 14, 9, 4, 2)):
        rows, cols = overlap_origins(h, out, stride), overlap_origins(w, out, stride)
        logits = rs.standard_normal((len(rows) * len(cols), c, out, out)).astype(np.float32) * 2
        probs, mask = stitch_overlap_np(logits, h, w, out, stride)
        for y in range(h):
            for x in range(w):
                ps = []
                for i, oy in enumerate(rows):
                    for j, ox in enumerate(cols):
                        if oy <= y < oy + out and ox <= x < ox + out:
                            v = logits[i * len(cols) + j, :, y - oy, x - ox].astype(np.float64)
                            e = np.exp(v - v.max())
                            ps.append(e / e.sum())
                assert ps
                want = np.mean(ps, axis=0)
                assert np.abs(probs[:, y, x] - want).max() < 1e-12
                assert mask[y, x] == int(np.argmax(want))
        assert np.abs(probs.sum(0) - 1).max() < 1e-12
