"""Timing of the duplicate suppression (mfx_box_nms; TEST.USE_NMS '2d' / '3d') at the inference size B = 8, K = 50, next to the launch it
follows, mfx_decode_boxes_cfg, on the same rows.  Three inputs: `decoded` = the rows the decode gives on a seeded random head map (few boxes
meet: the early-out's case), `clustered` = ten boxes per image with four near-copies each (what the operator is for), `identical` = fifty
copies of one box (every pair takes the full clip: the worst case).  Per input and kind: 20 warm-up launches, then REPS windows of ITERS
launches of the C entry on preallocated buffers between two device events, the entries taking turns inside a repetition; the median window
and the spread are printed as one JSON line.  Back-to-back launches of one small kernel: the figure is the larger of the kernel's time and
the launch rate.  Carries no threshold.      python tools/box_nms_bench.py [--iters N] [--reps R]"""
import argparse
import ctypes
import json
import math
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from monoflex_amd import lib as L, ops
from monoflex_amd.ops import _ptr, _stream

ap = argparse.ArgumentParser()
ap.add_argument("--iters", type=int, default=5000)
ap.add_argument("--reps", type=int, default=5)
args = ap.parse_args()
WARM, B, K, H, W, LD, REG_OFF, THRESH = 20, 8, 50, 96, 320, 64, 8, 0.5
lib = L.load()
dev = "cuda"
rng = np.random.default_rng(0)


def window(fn, n):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(n):
        fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b) * 1e3 / n                              # microseconds per launch


def clustered(copies, jitter):
    det = np.zeros((B, K, 14), np.float32)
    for b in range(B):
        for c in range(K // copies):
            x1, y1 = rng.uniform(0, 1000), rng.uniform(100, 250)
            base = np.array([c % 3, 0, x1, y1, x1 + rng.uniform(30, 200), y1 + rng.uniform(25, 120), 1.5, 1.6, 3.9,
                             rng.uniform(-25, 25), 1.7, rng.uniform(8, 60), rng.uniform(-math.pi, math.pi), 0])
            for k in range(copies):
                r = base.copy()
                r[2:6] += rng.normal(0, 2.0, 4) * jitter
                r[6:9] *= 1 + rng.uniform(-0.05, 0.05, 3) * jitter
                r[9:12] += rng.normal(0, 0.1, 3) * jitter
                r[12] += rng.uniform(-0.1, 0.1) * jitter
                r[13] = rng.uniform(0.2, 0.95)
                det[b, c * copies + k] = r
    return det


# the decode's own rows on a seeded random head map (runs/monoflex.yaml decode: mfx_decode_boxes_cfg)
hm = torch.from_numpy(rng.normal(0, 1.5, (B, H, W, LD)).astype(np.float32)).to(dev)
calib = torch.tensor([[721.5, 721.5, 609.6, 172.9, -0.06, 0.003]] * B, dtype=torch.float32, device=dev)
pad = torch.zeros((B, 2), dtype=torch.int32, device=dev)
size = torch.tensor([1280, 384], dtype=torch.int32, device=dev)
scores, index = ops.decode_topk(hm, 0, 3, K)
from monoflex_amd.config import get_cfg
cfg = L.decode_cfg(L.head_decode_settings(get_cfg(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "runs", "monoflex.yaml"))), True)
det_d = torch.empty((B, K, 14), dtype=torch.float32, device=dev)
topk_d = torch.empty((B, K, 5), dtype=torch.float32, device=dev)
valid_d = torch.empty((B, K), dtype=torch.int32, device=dev)


def decode():
    L.check(lib.mfx_decode_boxes_cfg(_ptr(hm), LD, REG_OFF, _ptr(scores), _ptr(index), 3, B, H, W, K, _ptr(calib), _ptr(pad), _ptr(size),
                                     ctypes.c_float(0.0), ctypes.byref(cfg), _ptr(det_d), _ptr(topk_d), _ptr(valid_d), None, _stream()),
            "mfx_decode_boxes_cfg")


decode()
torch.cuda.synchronize()
inputs = {"decoded": det_d.clone(), "clustered": torch.from_numpy(clustered(5, 1.0)).to(dev), "identical": torch.from_numpy(clustered(K, 0.0)).to(dev)}
valid = torch.ones((B, K), dtype=torch.int32, device=dev)
out = torch.empty_like(valid)


def nms(det, kind):
    return lambda: L.check(lib.mfx_box_nms(_ptr(det), _ptr(valid), B, K, kind, ctypes.c_float(THRESH), 0, _ptr(out), _stream()), "mfx_box_nms")


entries = {"decode_boxes_cfg": decode}
kept = {}
for name, det in inputs.items():
    for kind, kid in L.NMS_KINDS.items():
        entries["nms_%s_%s" % (kind, name)] = nms(det, kid)
        entries["nms_%s_%s" % (kind, name)]()
        torch.cuda.synchronize()
        kept["nms_%s_%s" % (kind, name)] = int(out.sum())
for fn in entries.values():
    window(fn, WARM)
samples = {n: [] for n in entries}
for _ in range(args.reps):
    for n, fn in entries.items():
        samples[n].append(window(fn, args.iters))
res = {"what": "mfx_box_nms next to mfx_decode_boxes_cfg, B %d, K %d, thresh %.1f, per class, all %d rows valid" % (B, K, THRESH, B * K),
       "warmup": WARM, "launches_per_window": args.iters, "windows": args.reps, "rows_kept_of_%d" % (B * K): kept,
       "us_per_launch": {n: {"median": round(float(np.median(v)), 2), "min": round(min(v), 2), "max": round(max(v), 2)} for n, v in samples.items()}}
print(json.dumps(res))
