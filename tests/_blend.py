"""The mean-probability blend of csrc/blend.hip stated in float64 numpy: what tests/test_cpu_blend.py and tests/test_blend_gpu.py
compare the kernels and the inference paths against.  Not a test module."""
import numpy as np

from tests.test_cpu_overlap_tile import overlap_origins, softmax0


def blend_mean_np(members, h, w, out, stride, mirrored=None):
    """members: a list of logit arrays [n, C, out, out], one per ensemble member, each the row-major tile grid of
    overlap_origins(h, out, stride) x overlap_origins(w, out, stride).  mirrored[m] says that member m's tiles hold the logits of the
    horizontally mirrored windows (default: every member but the first, predict_image(flip=True)'s second sweep); they are mirrored
    back before they are placed.  Every pixel's score is the float64 mean of softmax over the tiles that cover it and over the members.
    Returns (probs [C, h, w] float64, uint8 first-maximum mask)."""
    rows, cols = overlap_origins(h, out, stride), overlap_origins(w, out, stride)
    mirrored = [k > 0 for k in range(len(members))] if mirrored is None else mirrored
    acc = np.zeros((members[0].shape[1], h, w))
    cnt = np.zeros((h, w))
    for logits, mir in zip(members, mirrored):
        assert logits.shape[0] == len(rows) * len(cols) and logits.shape[2:] == (out, out)
        for i, oy in enumerate(rows):
            for j, ox in enumerate(cols):
                t = logits[i * len(cols) + j].astype(np.float64)
                acc[:, oy:oy + out, ox:ox + out] += softmax0(t[:, :, ::-1] if mir else t)
                cnt[oy:oy + out, ox:ox + out] += 1
    probs = acc / cnt
    return probs, probs.argmax(0).astype(np.uint8)
