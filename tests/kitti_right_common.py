"""Shared by the CPU and GPU tests of right-camera samples (DATASETS.USE_RIGHT_IMAGE): the reference's goldens for the
right view, a restatement of the right view on top of oracle/kitti_encode_ref.py for fuzzing, the host build of the
device functions with the view flag, and a generated KITTI directory that has image_3/ and a real P3.
Comparison rules are those of tests/kitti_common.py; nothing here adds a tolerance."""
import ctypes
import os
import subprocess

import numpy as np
import torch

from monoflex_amd import lib as L
from monoflex_amd import synthetic as S
from monoflex_amd.data import encode as E
from monoflex_amd.data.datasets import kitti_utils as KU
from oracle import kitti_encode_ref as K

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLD_R = np.load(os.path.join(ROOT, "tests", "golden", "kitti_encode_right.npz"))
NAMES_R = [str(n) for n in GOLD_R["names"]]
P3 = np.asarray(S.KITTI_P3, dtype=np.float64)                      # the matrix the fixture was recorded with (asserted in the CPU tests)
RAISED = [n for n in NAMES_R if int(GOLD_R[n + "_raised"])]
KEPT = [n for n in NAMES_R if not int(GOLD_R[n + "_raised"])]
CLASSES = ("Car", "Pedestrian", "Cyclist")
GOLD_FIELDS = ("hm", "cls_ids", "target_centers", "reg_mask", "trunc_mask", "reg_weight", "keypoints_depth_mask", "pad_size", "edge_len",
               "edge_indices", "occlusions", "truncations", "gt_bboxes", "dimensions", "locations", "rotys", "keypoints", "offset_3D",
               "2d_bboxes", "alphas", "orientations")
ORACLE_ERRORS = (TypeError, ValueError, AssertionError, IndexError)     # what tests/kitti_common.oracle_fields treats as "the reference fails"
NP_DTYPES = {torch.float32: np.float32, torch.float64: np.float64, torch.int32: np.int32, torch.int64: np.int64, torch.uint8: np.uint8}
FUZZ_SEEDS = range(1000, 1300)


def golden_right_sample(name):
    """(label lines, width, height, flip, seed of the image_3 frame) of one recorded case."""
    w, h, flip, iseed = (int(v) for v in GOLD_R[name + "_meta"])
    text = str(GOLD_R[name + "_labels"])
    return (text.split("\n") if text else []), w, h, bool(flip), iseed


def golden_right_fields(name):
    return {k: GOLD_R[name + "_" + k] for k in GOLD_FIELDS}


def right_view_objects(lines, P, img_w, img_h):
    """The objects of a right-camera sample: read as usual, then every 2D box regenerated from the eight projected 3D corners,
    clamped with Python's max / min and cast to float32; xmin .. ymax become those float32 scalars (reference kitti.py:243-250)."""
    P = np.asarray(P, dtype=np.float64).reshape(3, 4)
    objs = K.read_objects(lines)
    for o in objs:
        with np.errstate(divide="ignore", invalid="ignore"):
            c2, _ = K.project(P, K.corners3d(o))
        o.box2d = np.array([max(c2[:, 0].min(), 0), max(c2[:, 1].min(), 0),
                            min(c2[:, 0].max(), img_w - 1), min(c2[:, 1].max(), img_h - 1)], dtype=np.float32)
        o.xmin, o.ymin, o.xmax, o.ymax = o.box2d
    return objs


def encode_right_sample(lines, P, img_w, img_h, do_flip=False, **kw):
    """oracle.kitti_encode_ref.encode_sample on the right-view objects. encode_sample reads its objects through the module-level
    `read_objects`; that name is substituted for this one call. Raises what the restatement raises."""
    objs = right_view_objects(lines, P, img_w, img_h)
    original = K.read_objects
    K.read_objects = lambda _lines, *a, **k: objs
    try:
        return K.encode_sample(lines, P, img_w, img_h, do_flip=do_flip, **kw)
    finally:
        K.read_objects = original


def right_oracle_fields(lines, w, h, flip, P=P3):
    try:
        return encode_right_sample(lines, P, w, h, do_flip=flip)
    except ORACLE_ERRORS:
        return None                                              # inputs the reference itself fails on


def build_views_shim(directory):
    """Compiles tests/shim/kitti_encode_views_host.cpp (-ffp-contract=off, like the device build) -> ctypes library."""
    so = os.path.join(str(directory), "libkitti_views_shim.so")
    cmd = ["g++", "-O2", "-std=c++17", "-ffp-contract=off", "-shared", "-fPIC", "-o", so,
           os.path.join(ROOT, "tests", "shim", "kitti_encode_views_host.cpp")]
    r = subprocess.run(cmd, capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    lib = ctypes.CDLL(so)
    lib.shim_kitti_encode_views.argtypes = [ctypes.POINTER(L.KittiDesc), ctypes.c_void_p]
    lib.shim_kitti_encode_views.restype = None
    lib.shim_right_view_box.argtypes = [ctypes.c_void_p] + [ctypes.c_double] * 4 + [ctypes.c_float] * 3 + [ctypes.c_int] * 2 + [ctypes.c_void_p]
    lib.shim_right_view_box.restype = None
    return lib


def shim_right_view_box(shim, line, P, img_w, img_h):
    """right_view_box of kitti_encode_math.h on one label line -> (4,) float32."""
    o = K.Obj(line)
    P = np.ascontiguousarray(P, dtype=np.float64).reshape(12)
    box = np.full(4, 77, dtype=np.float32)
    shim.shim_right_view_box(P.ctypes.data, o.h, o.w, o.l, o.ry, float(o.t[0]), float(o.t[1]), float(o.t[2]), img_w, img_h, box.ctypes.data)
    return box


def shim_encode_records(shim, records, Ps, sizes, flips, params, rights=None):
    """Host twin of monoflex_amd.data.encode.encode_targets: same packing, same descriptor, the device functions compiled for the CPU."""
    inp = E.pack_inputs(records, Ps, sizes, flips, params)
    dims, B = params.dims(), len(records)
    out = {name: np.full((B,) + tuple(dims.get(s, s) for s in shape), 77, dtype=NP_DTYPES[dt])      # poison: every element must be written
           for name, (_, shape, dt) in E.TARGET_FIELDS.items()}
    d = L.KittiDesc()
    for k, a in inp.items():
        setattr(d, k, a.ctypes.data)
    for name, (member, _, _) in E.TARGET_FIELDS.items():
        setattr(d, member, out[name].ctypes.data)
    d.B, d.max_objs, d.in_w, d.in_h, d.down, d.num_classes = B, params.max_objs, params.in_w, params.in_h, params.down, params.num_classes
    d.filter_trunc, d.filter_size, d.edge_ratio = params.filter_trunc, params.filter_size, params.edge_ratio
    right = None if rights is None else np.asarray(rights, dtype=np.int32).reshape(B).copy()
    shim.shim_kitti_encode_views(ctypes.byref(d), None if right is None else right.ctypes.data)
    return out


def run_views_shim(shim, samples, rights, params=None):
    """samples: [(lines, w, h, flip)], rights: [0/1] or None -> {field: (B, ...) numpy}; right samples get P3, left ones KITTI_P2."""
    params = params or E.EncodeParams()
    recs = [KU.read_label_records(lines, CLASSES) for lines, _, _, _ in samples]
    return shim_encode_records(shim, recs, view_matrices(rights, len(samples)), [(w, h) for _, w, h, _ in samples],
                               [f for _, _, _, f in samples], params, rights)


def view_matrices(rights, B):
    return [P3 if (rights is not None and rights[b]) else S.KITTI_P2 for b in range(B)]


def mixed_fuzz_batch(seeds):
    """For every seed of tests/kitti_common.fuzz_sample its label set twice, as the left and as the right view, with the flip the
    seed draws: rows alternate left / right, and flipped / unflipped samples of both views occur.
    -> samples [(lines, w, h, flip)], rights [0/1], refs [restated fields or None]."""
    from tests.kitti_common import fuzz_sample, oracle_fields
    samples, rights, refs = [], [], []
    for seed in seeds:
        lines, w, h, flip = fuzz_sample(seed)
        samples += [(lines, w, h, flip)] * 2
        rights += [0, 1]
        refs += [oracle_fields(lines, w, h, flip), right_oracle_fields(lines, w, h, flip)]
    return samples, rights, refs


def left_frame_seed(i):
    return 700 + i


def right_frame_seed(i):
    return 800 + i


def make_kitti_dir(path, cases, splits=("train",), right_images=True, right_seed_of=right_frame_seed):
    """KITTI-format folder with image_2/, image_3/ (other pixels than image_2/), label_2/, calib/ (P2 = KITTI_P2, P3 = P3 above).
    cases: [(label lines, width, height)]; frame i of image_3/ is frame_pixels(right_seed_of(i), width, height)."""
    from PIL import Image
    path = str(path)
    frames = (("image_2", left_frame_seed), ("image_3", right_seed_of)) if right_images else (("image_2", left_frame_seed),)
    for d in ("label_2", "calib", "ImageSets") + tuple(folder for folder, _ in frames):
        os.makedirs(os.path.join(path, d))
    for i, (lines, w, h) in enumerate(cases):
        for folder, seed_of in frames:
            Image.fromarray(frame_pixels(seed_of(i), w, h)).save(os.path.join(path, folder, "%06d.png" % i))
        with open(os.path.join(path, "label_2", "%06d.txt" % i), "w") as f:
            f.write("".join(l + "\n" for l in lines))
        with open(os.path.join(path, "calib", "%06d.txt" % i), "w") as f:
            f.write("P2: " + " ".join("%.12e" % v for v in np.asarray(S.KITTI_P2).reshape(-1)) + "\n")
            f.write("P3: " + " ".join("%.12e" % v for v in P3.reshape(-1)) + "\n")
            f.write("R0_rect: 1 0 0 0 1 0 0 0 1\nTr_velo_to_cam: 1 0 0 0 0 1 0 0 0 0 1 0\n")
    for s in splits:
        with open(os.path.join(path, "ImageSets", s + ".txt"), "w") as f:
            f.write("".join("%06d\n" % i for i in range(len(cases))))
    return path


def frame_pixels(seed, w, h):
    return np.random.RandomState(seed).randint(0, 256, (h, w, 3)).astype(np.uint8)


def right_cfg():
    """runs/monoflex.yaml with the setting switched on the way a user does it: a trailing command-line `opts` pair."""
    from monoflex_amd.config import get_cfg
    cfg = get_cfg(os.path.join(ROOT, "runs", "monoflex.yaml"))
    cfg.merge_from_list(["DATASETS.USE_RIGHT_IMAGE", "True"])
    return cfg


def assert_frame_is_the_recorded_one(image, name):
    """(3, in_h, in_w) network input against the reference pipeline's checksum samples of the image_3 frame of that case."""
    flat = np.asarray(image, dtype=np.float64).ravel()
    np.testing.assert_allclose(flat[GOLD_R[name + "_img_idx"]], GOLD_R[name + "_img_samples"], rtol=0, atol=1e-6, err_msg=name)
