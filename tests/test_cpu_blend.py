"""The streaming mean-probability blend without a GPU: the overlap-tile geometry contains the fitted sliding-window grid, the float64
statement of the blend (tests/_blend.py) reduces to the one-member numpy blend, the keywords that need blend='mean' are refused before
the library is touched, and the new entry points are declared and bound."""
import os
import re
from types import SimpleNamespace

import numpy as np
import pytest

from tests._blend import blend_mean_np
from tests.test_cpu_overlap_tile import overlap_origins, stitch_overlap_np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ('pylc_blend_accumulate', 'pylc_blend_finalize', 'pylc_image_pack_tiles_flip', 'pylc_image_pack_tiles_reflect_ex')


@pytest.mark.parametrize('h,w,tile,stride,grid', [(3072, 4096, 512, 256, (11, 15)), (128, 192, 64, 32, (3, 5)), (64, 96, 32, 16, (3, 5)),
                                                   (512, 512, 512, 256, (1, 1)), (1024, 1536, 512, 512, (2, 3)), (96, 160, 32, 8, (9, 17))])
def test_fitted_grid_is_a_special_case_of_the_overlap_grid(h, w, tile, stride, grid):
    from pylc_amd.inference import overlap_tile_grid, tile_grid
    rows, cols = tile_grid(h, w, tile, stride)
    assert (rows, cols) == grid
    row_o, col_o = overlap_tile_grid(h, w, tile, stride)
    assert row_o == [i * stride for i in range(rows)] and col_o == [j * stride for j in range(cols)]      # the clamp is never active


def test_unfitted_size_keeps_the_overlap_grid_only():
    from pylc_amd.inference import overlap_tile_grid, tile_grid
    with pytest.raises(ValueError):
        tile_grid(100, 150, 64, 32)
    assert overlap_tile_grid(100, 150, 64, 32) == ([0, 32, 36], [0, 32, 64, 86])


@pytest.mark.parametrize('h,w,out,stride,c', [(23, 31, 8, 3, 5), (17, 20, 9, 9, 3), (37, 53, 16, 5, 9), (16, 16, 16, 16, 2)])
def test_one_member_statement_is_the_numpy_blend(h, w, out, stride, c):
    n = len(overlap_origins(h, out, stride)) * len(overlap_origins(w, out, stride))
    logits = (np.random.RandomState(h + w + c).standard_normal((n, c, out, out)) * 3).astype(np.float32)
    want_p, want_m = stitch_overlap_np(logits, h, w, out, stride)
    got_p, got_m = blend_mean_np([logits], h, w, out, stride)
    assert np.abs(got_p - want_p).max() < 1e-12 and np.array_equal(got_m, want_m)
    # two members, the second the mirrored tiles of the first: mirrored back, the mean of two equal terms
    two_p, two_m = blend_mean_np([logits, logits[:, :, :, ::-1]], h, w, out, stride)
    assert np.abs(two_p - want_p).max() < 1e-12 and np.array_equal(two_m, want_m)
    assert np.abs(two_p.sum(0) - 1).max() < 1e-12


@pytest.mark.parametrize('kw', ['flip', 'return_probs', 'return_confidence'])
def test_reference_blend_refuses_what_needs_probabilities(kw):
    """Checked from the arguments alone, before the library is initialised: no GPU, no real model."""
    import torch
    from pylc_amd import inference, photo
    model = SimpleNamespace(meta=SimpleNamespace(arch='deeplab', ch=3, n_classes=9))
    with pytest.raises(ValueError, match="blend='mean'"):
        inference.predict_image(model, torch.zeros(3, 128, 192), 64, **{kw: True})
    with pytest.raises(ValueError, match="blend='mean'"):
        inference.predict_image(model, torch.zeros(3, 128, 192), 64, blend='reference', **{kw: True})
    with pytest.raises(ValueError, match="blend='mean'"):
        photo.segment_photo(model, np.zeros((128, 192, 3), np.uint8), tile=64, **{kw: True})
    with pytest.raises(ValueError, match="'reference' or 'mean'"):
        inference.predict_image(model, torch.zeros(3, 128, 192), 64, blend='max')
    with pytest.raises(ValueError, match="'reference' or 'mean'"):
        photo.segment_photo(model, np.zeros((128, 192, 3), np.uint8), tile=64, blend='max')


def test_photo_result_keeps_its_positional_constructor():
    from pylc_amd.photo import PhotoResult
    r = PhotoResult('m', 'rgb', {'g': 1}, 'p', 512, 0.5)
    assert (r.mask, r.rgb, r.geometry, r.probs, r.tile, r.scale, r.confidence) == ('m', 'rgb', {'g': 1}, 'p', 512, 0.5, None)
    assert PhotoResult('m', None, {}, None, 512, None, confidence='c').confidence == 'c'


def test_new_entry_points_are_declared_and_bound():
    import ctypes
    from pylc_amd import lib as L
    hdr = re.sub(r'/\*.*?\*/', '', open(os.path.join(ROOT, 'include', 'pylc_hip.h')).read(), flags=re.S)
    dll = ctypes.CDLL(L.LIB_PATH)
    for name in NEW:
        assert re.search(r'\b%s\s*\(' % name, hdr), name
        assert name in L.SIGNATURES and hasattr(dll, name), name
    # trailing `int flip` on the cutters; the accumulator's and the finalizer's argument counts as the header states them
    assert len(L.SIGNATURES['pylc_image_pack_tiles_flip'][1]) == len(L.SIGNATURES['pylc_image_pack_tiles_ex'][1]) + 1
    assert len(L.SIGNATURES['pylc_image_pack_tiles_reflect_ex'][1]) == len(L.SIGNATURES['pylc_image_pack_tiles_reflect'][1]) + 1
    assert len(L.SIGNATURES['pylc_blend_accumulate'][1]) == 13 and len(L.SIGNATURES['pylc_blend_finalize'][1]) == 12
    assert 'blend.hip' in open(os.path.join(ROOT, 'pylc_amd', 'csrc', 'Makefile')).read()
