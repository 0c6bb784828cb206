"""Timing of the several-modes-and-oracle box decode (mfx_decode_boxes_multi) at the inference size B = 8, K = 50 on a 96 x 320 map, next to
the launch it replaces, mfx_decode_boxes_cfg, on the same top-K of a seeded random head map: one mode, the eight modes, the eight modes plus
'oracle' against a table of M = 40 objects per image (an object on every second detection's box), and 'oracle' alone.  20 warm-up
launches, then REPS windows of ITERS launches of the C entry on preallocated buffers between two device events, the entries taking turns
inside a repetition; the median window and the spread are printed as one JSON line.  Back-to-back launches of one small kernel: the figure
is the larger of the kernel's time and the launch rate.  The second part times OUTPUT_DEPTH 'oracle' of one batch end to end, host clock
around a synchronised call: PostProcessor.decode_oracle (five launches, ten copies to the host, the Python loop) against
decode_device(gt_rows=...) (one launch).  Carries no threshold.      python tools/decode_multi_bench.py [--iters N] [--reps R]"""
import argparse
import ctypes
import json
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from monoflex_amd import lib as L, ops
from monoflex_amd.ops import _ptr, _stream

ap = argparse.ArgumentParser()
ap.add_argument("--iters", type=int, default=5000)
ap.add_argument("--reps", type=int, default=5)
args = ap.parse_args()
WARM, B, K, H, W, LD, REG_OFF, THRESH, M = 20, 8, 50, 96, 320, 64, 8, 0.2, 40
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


hm = torch.from_numpy(rng.normal(0, 1.5, (B, H, W, LD)).astype(np.float32)).to(dev)
calib = torch.tensor([[721.5, 721.5, 609.6, 172.9, -0.06, 0.003]] * B, dtype=torch.float32, device=dev)
pad = torch.zeros((B, 2), dtype=torch.int32, device=dev)
size = torch.tensor([1280, 384], dtype=torch.int32, device=dev)
scores, index = ops.decode_topk(hm, 0, 3, K)
from monoflex_amd.config import get_cfg
from monoflex_amd.model.head.detector_infer import make_post_processor
yaml = os.path.join(ROOT, "runs", "monoflex.yaml")
cfg = L.decode_cfg(L.head_decode_settings(get_cfg(yaml)), True)
heads = L.HeadSet([L.HEAD_KEYS], [[L.HEAD_WIDTHS[k] for k in L.HEAD_KEYS]]).layout()
det1 = torch.empty((B, K, 14), dtype=torch.float32, device=dev)
det9 = torch.empty((B, 9, K, 14), dtype=torch.float32, device=dev)
unc9 = torch.empty((B, 9, K, 2), dtype=torch.float32, device=dev)
topk_d = torch.empty((B, K, 5), dtype=torch.float32, device=dev)
valid_d = torch.empty((B, K), dtype=torch.int32, device=dev)
choice_d = torch.empty((B, K), dtype=torch.int32, device=dev)


def single():
    L.check(lib.mfx_decode_boxes_cfg(_ptr(hm), LD, REG_OFF, _ptr(scores), _ptr(index), 3, B, H, W, K, _ptr(calib), _ptr(pad), _ptr(size),
                                     ctypes.c_float(THRESH), ctypes.byref(cfg), _ptr(det1), _ptr(topk_d), _ptr(valid_d), None, _stream()),
            "mfx_decode_boxes_cfg")


single()
torch.cuda.synchronize()
# the ground truth: an object on every second detection's box, its depth the detection's own
rows = det1.cpu().numpy()
gt = np.zeros((B, M, 8), dtype=np.float32)
for b in range(B):
    for n, i in enumerate(range(0, K, 2)[:M]):
        gt[b, n] = (1, rows[b, i, 0], *rows[b, i, 2:6], rows[b, i, 11], 0)
gt_rows = torch.from_numpy(gt).to(dev)


def multi(mask, with_unc=True):
    oracle = bool(mask >> 8)
    return lambda: L.check(lib.mfx_decode_boxes_multi(_ptr(hm), LD, REG_OFF, _ptr(scores), _ptr(index), 3, B, H, W, K, _ptr(calib), _ptr(pad),
                                                      _ptr(size), ctypes.c_float(THRESH), ctypes.byref(cfg), ctypes.byref(heads), mask,
                                                      _ptr(gt_rows) if oracle else None, M if oracle else 0, _ptr(det9), _ptr(topk_d), _ptr(valid_d),
                                                      _ptr(unc9) if with_unc else None, _ptr(choice_d) if oracle else None, _stream()),
                           "mfx_decode_boxes_multi")


entries = {"decode_boxes_cfg": single, "multi_1_mode": multi(1, False), "multi_8_modes": multi(0xff), "multi_8_modes_oracle": multi(0x1ff),
           "multi_oracle_alone": multi(0x100)}
for fn in entries.values():
    window(fn, WARM)
matched = int((choice_d >= 0).sum())
samples = {n: [] for n in entries}
for _ in range(args.reps):
    for n, fn in entries.items():
        samples[n].append(window(fn, args.iters))

# 'oracle' of one batch, end to end (host clock, synchronised): the host form against the device form
from monoflex_amd.structures.params_3d import Calibration, ParamsList
post = make_post_processor(get_cfg(yaml, ["MODEL.HEAD.OUTPUT_DEPTH", "oracle"]))
Pm = np.array([[721.5, 0, 609.6, 721.5 * 0.06], [0, 721.5, 172.9, -721.5 * 0.003], [0, 0, 1, 0]], dtype=np.float64)
targets = []
for b in range(B):
    t = ParamsList(image_size=(1280, 384), is_train=False)
    t.add_field("pad_size", torch.zeros(2, dtype=torch.int64))
    t.add_field("calib", Calibration(Pm))
    g = torch.from_numpy(gt[b])
    loc = torch.zeros(M, 3)
    loc[:, 2] = g[:, 6]
    for k, v in (("reg_mask", g[:, 0].to(torch.uint8)), ("cls_ids", g[:, 1].long()), ("gt_bboxes", g[:, 2:6].clone()), ("locations", loc)):
        t.add_field(k, v)
    targets.append(t)
p, c, s = post.prepare_targets(targets, dev)


def wall(fn, reps=20):
    fn()
    torch.cuda.synchronize()
    out = []
    for _ in range(reps):
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        out.append((time.perf_counter() - t0) * 1e6)
    return {"median": round(float(np.median(out)), 1), "min": round(min(out), 1), "max": round(max(out), 1)}


host = wall(lambda: post.decode_oracle(hm, p, c, s, None, targets))
device = wall(lambda: post.decode_device(hm, p, c, s, gt_rows=ops.oracle_gt_rows(targets, dev)))
device_table_ready = wall(lambda: post.decode_device(hm, p, c, s, gt_rows=gt_rows))
res = {"what": "mfx_decode_boxes_multi next to mfx_decode_boxes_cfg, B %d, K %d, %d x %d map, M %d, threshold %.1f" % (B, K, H, W, M, THRESH),
       "warmup": WARM, "launches_per_window": args.iters, "windows": args.reps, "oracle_matched_of_%d" % (B * K): matched,
       "us_per_launch": {n: {"median": round(float(np.median(v)), 2), "min": round(min(v), 2), "max": round(max(v), 2)} for n, v in samples.items()},
       "oracle_batch_wall_us": {"host_form_decode_oracle": host, "device_form_with_table_build": device, "device_form_table_ready": device_table_ready}}
print(json.dumps(res))
