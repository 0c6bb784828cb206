"""Timing of deformable PSROI pooling (mfx_dcn_v2_psroi_pooling_forward / _backward) at (2,16,38,50), 300 ROIs, pooled 7, 4 samples per
part, scale 1/16, with and without offsets: 20 warm-up + 100 timed launches of the C entry on preallocated outputs between two hipEvents.
`bytes` is the compulsory traffic of a launch (every operand read once, every result written once; the backward's gradient buffers
twice: zero fill + accumulation).  Prints one JSON line."""
import ctypes
import json
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from monoflex_amd import lib as L
from monoflex_amd.ops import _ptr, _stream

B, C, H, W, N, P, S, SCALE, TSTD = 2, 16, 38, 50, 300, 7, 4, 1.0 / 16, 0.1
WARM, ITERS = 20, 100
rng = np.random.default_rng(0)
x = torch.from_numpy(rng.standard_normal((B, C, H, W)).astype(np.float32)).cuda()
r = np.zeros((N, 5), np.float32)
r[:, 0] = rng.integers(0, B, N)
r[:, 1], r[:, 2] = rng.uniform(-40, W / SCALE - 60, N), rng.uniform(-40, H / SCALE - 60, N)
r[:, 3], r[:, 4] = r[:, 1] + rng.uniform(16, 400, N), r[:, 2] + rng.uniform(16, 300, N)
rois = torch.from_numpy(r).cuda()
trans = torch.from_numpy(rng.standard_normal((N, 2, P, P)).astype(np.float32)).cuda()
go = torch.from_numpy(rng.standard_normal((N, C, P, P)).astype(np.float32)).cuda()
out, cnt = torch.empty_like(go), torch.empty_like(go)
gi, gt = torch.empty_like(x), torch.empty_like(trans)
lib = L.load()


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


res = {"what": "deformable PSROI pooling, input (%d,%d,%d,%d), %d ROIs, pooled %d, %d samples per part, scale 1/16" % (B, C, H, W, N, P, S),
       "warmup": WARM, "launches": ITERS}
for name, no_trans in (("no_trans", 1), ("offsets", 0)):
    t = None if no_trans else trans

    def fwd():
        L.check(lib.mfx_dcn_v2_psroi_pooling_forward(_ptr(x), _ptr(rois), _ptr(t), _ptr(out), _ptr(cnt), B, C, H, W, N, N, 2, no_trans, SCALE, C, 1, P, P,
                                                     S, TSTD, _stream()), "forward")

    def bwd():
        L.check(lib.mfx_dcn_v2_psroi_pooling_backward(_ptr(go), _ptr(x), _ptr(rois), _ptr(t), _ptr(cnt), _ptr(gi), _ptr(gt) if t is not None else None,
                                                      B, C, H, W, N, N, 2, no_trans, SCALE, C, 1, P, P, S, TSTD, _stream()), "backward")
    f_us = timed(fwd)
    b_us = timed(bwd)
    f_bytes = 4 * (x.numel() + rois.numel() + (0 if no_trans else trans.numel()) + 2 * out.numel())
    b_bytes = 4 * (2 * go.numel() + rois.numel() + 2 * gi.numel() + (0 if no_trans else x.numel() + 3 * trans.numel()))
    res[name] = {"forward_us": round(f_us, 2), "backward_us": round(b_us, 2), "forward_bytes": f_bytes, "backward_bytes": b_bytes,
                 "forward_GBps": round(f_bytes / f_us / 1e3, 2), "backward_GBps": round(b_bytes / b_us / 1e3, 2),
                 "kept_fraction": round(float(cnt.sum()) / (cnt.numel() * S * S), 3)}
print(json.dumps(res))
