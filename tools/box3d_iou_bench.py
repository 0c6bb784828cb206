"""Timing of the rotated 3D box IoU of matched pairs (mfx_box3d_iou_pairs) on KITTI-like boxes, both input forms, at the training size
(400 pairs = B 8 x MAX_OBJECTS 40 rounded up) and at 65536 pairs: 20 warm-up + 100 timed launches of the C entry on preallocated buffers
between two hipEvents.  Prints one JSON line; carries no threshold."""
import json
import math
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from monoflex_amd import lib as L
from monoflex_amd.ops import _ptr, _stream

WARM, ITERS = 20, 100
lib = L.load()


def boxes(n, rng):
    a = np.zeros((n, 7), np.float32)
    a[:, 0], a[:, 1], a[:, 2] = rng.uniform(-30, 30, n), rng.uniform(-1, 3, n), rng.uniform(5, 70, n)
    a[:, 3:6] = rng.uniform(0.5, 5.0, (n, 3))
    a[:, 6] = rng.uniform(-math.pi, math.pi, n)
    b = a.copy()
    b[:, :3] += rng.uniform(-1.5, 1.5, (n, 3)).astype(np.float32)
    b[:, 6] += rng.uniform(-0.5, 0.5, n).astype(np.float32)
    return a, b


def corners(r):
    c, s = np.cos(r[:, 6:7]), np.sin(r[:, 6:7])
    sx, sy, sz = (np.array(v, np.float32) for v in ([-1, -1, 1, 1, -1, -1, 1, 1], [1, 1, 1, 1, -1, -1, -1, -1], [-1, 1, 1, -1, -1, 1, 1, -1]))
    x, y, z = 0.5 * r[:, 3:4] * sx, 0.5 * r[:, 4:5] * sy, 0.5 * r[:, 5:6] * sz
    return np.stack((c * x + s * z + r[:, 0:1], y + r[:, 1:2], -s * x + c * z + r[:, 2:3]), axis=2).astype(np.float32)


def timed(fn):
    for _ in range(WARM):
        fn()
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(ITERS):
        fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b) * 1e3 / ITERS                         # microseconds per launch


res = {"what": "rotated 3D box IoU of matched pairs (mfx_box3d_iou_pairs)", "warmup": WARM, "launches": ITERS}
rng = np.random.default_rng(0)
for n in (400, 65536):
    ra, rb = boxes(n, rng)
    for form, (x, y) in enumerate(((ra, rb), (corners(ra), corners(rb)))):
        x, y = torch.from_numpy(x).cuda(), torch.from_numpy(y).cuda()
        out = torch.empty(n, device="cuda")
        us = timed(lambda: L.check(lib.mfx_box3d_iou_pairs(_ptr(x), _ptr(y), n, form, _ptr(out), _stream()), "mfx_box3d_iou_pairs"))
        res["N%d_form%d" % (n, form)] = {"us": round(us, 2), "Mpairs_per_s": round(n / us, 2), "mean_iou": round(float(out.mean()), 4)}
print(json.dumps(res))
