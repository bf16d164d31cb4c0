"""Masks as sets of regions: connected-region labels, region sizes, the small-region sieve and a region table, on the device
(csrc/regions.hip; the reference has nothing of the kind).

A region is a maximal set of pixels of one value connected through 4- or 8-neighbours; pixels equal to `ignore_index` belong to no region.
A pixel's label is the linear index y * W + x of the first pixel of its region in raster order (-1 at ignored pixels), sizes[r] is the
pixel count of the region rooted at r (0 at every other index).  Everything is exact integer work and canonical: two runs give the same
bytes, and a CPU statement of the rules (tests/_regions.py) can be compared bit for bit.

The sieve replaces every region smaller than `min_size`, either by a constant or by the value of its largest neighbour of at least
`min_size` pixels (4-neighbour contact; equal sizes go to the smaller root; a small region without such a neighbour stays).  Ignored
pixels are never changed and never lend a value.  With fill='ignore' the small regions become unlabelled: after a confidence cut of
pseudo-labels, the islands the cut leaves behind fall below the size and go too."""
import numpy as np
import torch

from . import lib as L
from .lib import lib, check, ptr, stream


def _check_mask(mask, connectivity, ignore_index):
    if not torch.is_tensor(mask) or mask.dtype != torch.uint8:
        raise TypeError('a mask must be a uint8 tensor, got %s' % (mask.dtype if torch.is_tensor(mask) else type(mask).__name__))
    if mask.dim() != 2 or mask.numel() == 0:
        raise ValueError('a mask must be [H,W] with at least one pixel, got %s' % (tuple(mask.shape),))
    if mask.numel() >= 2 ** 31:
        raise ValueError('a mask must have fewer than 2^31 pixels, got %s' % (tuple(mask.shape),))
    if connectivity not in (4, 8):
        raise ValueError('connectivity is 4 or 8, got %r' % (connectivity,))
    if ignore_index is not None and not 0 <= int(ignore_index) <= 255:
        raise ValueError('ignore_index=%r does not fit a uint8 mask (0..255)' % (ignore_index,))
    return -1 if ignore_index is None else int(ignore_index)


def _on_device(t, what):
    if not t.is_cuda:
        raise ValueError('%s must be on the HIP device (got %s); there is no CPU fallback' % (what, t.device))
    return t.contiguous()


def label_regions(mask, connectivity=4, ignore_index=None):
    """Device uint8 [H,W] -> int32 [H,W]: the minimum linear index of each pixel's region, -1 at pixels equal to ignore_index."""
    ign = _check_mask(mask, connectivity, ignore_index)
    mask = _on_device(mask, 'a mask')
    L.init()
    h, w = mask.shape
    labels = torch.empty((h, w), device=mask.device, dtype=torch.int32)
    check(lib.pylc_label_regions(ptr(mask), h, w, connectivity, ign, ptr(labels), stream()))
    return labels


def region_sizes(labels):
    """label_regions' labels -> int32 [H*W]: the pixel count of the region rooted at each index, 0 at every index that is no root."""
    if not torch.is_tensor(labels) or labels.dtype != torch.int32:
        raise TypeError('labels must be an int32 tensor (label_regions), got %s' % (labels.dtype if torch.is_tensor(labels) else type(labels).__name__))
    if labels.numel() == 0 or labels.numel() >= 2 ** 31:
        raise ValueError('labels must hold 1 .. 2^31 - 1 pixels, got %s' % (tuple(labels.shape),))
    labels = _on_device(labels, 'labels')
    L.init()
    sizes = torch.empty((labels.numel(),), device=labels.device, dtype=torch.int32)
    check(lib.pylc_region_sizes(ptr(labels), labels.numel(), ptr(sizes), stream()))
    return sizes


def _fill_value(fill, ignore_index):
    """-1 for the neighbour rule, else the constant"""
    if isinstance(fill, str):
        if fill == 'neighbour':
            return -1
        if fill != 'ignore' or ignore_index is None:
            raise ValueError("fill is 'neighbour', an int 0..255, or 'ignore' together with an ignore_index")
        return int(ignore_index)
    fill = int(fill)
    if not 0 <= fill <= 255:
        raise ValueError('fill=%d does not fit a uint8 mask (0..255)' % fill)
    return fill


def sieve(mask, min_size, connectivity=4, fill='neighbour', ignore_index=None, iterations=1, return_changed=False):
    """A new uint8 mask in which every region of fewer than min_size pixels is replaced: by the value of its largest neighbouring region
    of at least min_size pixels (fill='neighbour'; none: kept), by a constant (fill=0..255), or by ignore_index (fill='ignore').
    iterations=k repeats label + sieve k times on its own output; the count is fixed, nothing is read back from the device.
    return_changed: also a device int64 scalar, the number of pixels whose value was replaced (summed over the iterations).
    min_size <= 1 returns a clone without launching anything."""
    ign = _check_mask(mask, connectivity, ignore_index)
    fill_v = _fill_value(fill, ignore_index)
    if int(iterations) < 1:
        raise ValueError('iterations=%r: at least 1' % (iterations,))
    min_size = int(min_size)
    if min_size >= 2 ** 31:
        raise ValueError('min_size=%d does not fit an int32' % min_size)
    mask = _on_device(mask, 'a mask')
    changed = torch.zeros((), device=mask.device, dtype=torch.int64) if return_changed else None
    if min_size <= 1:
        return (mask.clone(), changed) if return_changed else mask.clone()
    L.init()
    h, w = mask.shape
    best = torch.empty((h * w,), device=mask.device, dtype=torch.int64) if fill_v < 0 else None
    cur = mask
    for _ in range(int(iterations)):
        labels = label_regions(cur, connectivity, ignore_index)
        sizes = region_sizes(labels)
        out = torch.empty_like(cur)
        check(lib.pylc_sieve_regions(ptr(cur), ptr(labels), ptr(sizes), h, w, min_size, ign, fill_v, ptr(best), ptr(out), ptr(changed),
                                     stream()))
        cur = out
    return (cur, changed) if return_changed else cur


def region_table(mask, connectivity=4, ignore_index=None):
    """The regions of a mask as host numpy arrays: 'root' (int64), 'cls' (uint8) and 'size' (int64), one row per region in ascending root
    order, and 'per_class': {'value', 'n_regions', 'pixels', 'largest'}, one row per value present among the regions.  One compaction on
    the device and one device-to-host copy of the compact rows."""
    labels = label_regions(mask, connectivity, ignore_index)
    sizes = region_sizes(labels)
    root = torch.nonzero(sizes, as_tuple=False).reshape(-1)            # ascending
    rows = torch.stack([root, mask.contiguous().reshape(-1)[root].to(torch.int64), sizes[root].to(torch.int64)]).cpu().numpy()
    root, cls, size = rows[0], rows[1].astype(np.uint8), rows[2]
    value = np.unique(cls)
    n_regions = np.bincount(cls, minlength=256)[value]
    pixels = np.bincount(cls, weights=size.astype(np.float64), minlength=256)[value].astype(np.int64)      # exact: below 2^31 in all
    largest = np.zeros(256, np.int64)
    np.maximum.at(largest, cls, size)
    return {'root': root, 'cls': cls, 'size': size,
            'per_class': {'value': value, 'n_regions': n_regions.astype(np.int64), 'pixels': pixels, 'largest': largest[value]}}
