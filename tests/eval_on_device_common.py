"""Shared by the CPU and GPU tests of the evaluation on the device (TEST.EVAL_ON_DEVICE): the host build of the record rule
(tests/shim/kitti_eval_pack_host.cpp), the text round trip it must equal, and the generated validation directory.
Every comparison of records is exact: the rule restates what writing and parsing a result file does to a value."""
import ctypes
import os
import subprocess

import numpy as np

from monoflex_amd import synthetic as S
from monoflex_amd.data import evaluation as EV

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def build_pack_shim(directory):
    so = os.path.join(str(directory), "libkitti_eval_pack_shim.so")
    r = subprocess.run(["g++", "-O2", "-std=c++17", "-ffp-contract=off", "-shared", "-fPIC", "-o", so,
                        os.path.join(ROOT, "tests", "shim", "kitti_eval_pack_host.cpp")], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    lib = ctypes.CDLL(so)
    for fn in (lib.shim_kitti_pack_round4, lib.shim_kitti_pack_records):
        fn.argtypes, fn.restype = [ctypes.c_void_p, ctypes.c_long, ctypes.c_void_p], None
    return lib


def text_records(rows, path):
    """(n,14) decode rows -> (n,16) records through the real result file: generate_kitti_3d_detection, then parse_label_text."""
    EV.generate_kitti_3d_detection(np.asarray(rows, dtype=np.float32).reshape(-1, 14), str(path))
    with open(str(path)) as f:
        return EV.parse_label_text(f.read())


def same_bits(a, b):
    a, b = np.ascontiguousarray(a, dtype=np.float64), np.ascontiguousarray(b, dtype=np.float64)
    return a.shape == b.shape and np.array_equal(a.view(np.uint64), b.view(np.uint64))


def make_val_dir(path, n=5, ids=None):
    """The generated directory of test_gpu_kitti_eval.py::test_inference_loop_end_to_end with n frames; `ids`: their image ids in
    split-file order (default 0..n-1)."""
    from PIL import Image
    path, ids = str(path), list(range(n)) if ids is None else list(ids)
    for d in ("image_2", "label_2", "calib", "ImageSets"):
        os.makedirs(os.path.join(path, d))
    P = " ".join("%.12e" % v for v in np.asarray(S.KITTI_P2).reshape(-1))
    for i, idx in enumerate(ids):
        Image.fromarray(np.random.RandomState(i).randint(0, 256, (375, 1242, 3)).astype(np.uint8)).save(os.path.join(path, "image_2", "%06d.png" % idx))
        with open(os.path.join(path, "label_2", "%06d.txt" % idx), "w") as f:
            f.write("\n".join(S.synthetic_kitti_labels(70 + i, 1242, 375, 8, z_range=(5, 38), occl_max=1)))
        with open(os.path.join(path, "calib", "%06d.txt" % idx), "w") as f:
            f.write("P2: " + P + "\nP3: " + P + "\n")
    with open(os.path.join(path, "ImageSets", "val.txt"), "w") as f:
        f.write("".join("%06d\n" % idx for idx in ids))
    return path


def write_label_dir(path, label_sets, ids=None):
    """label_2/ + a split file for label line lists -> (label_dir, split file)."""
    path, ids = str(path), list(range(len(label_sets))) if ids is None else list(ids)
    os.makedirs(os.path.join(path, "label_2"))
    for idx, lines in zip(ids, label_sets):
        with open(os.path.join(path, "label_2", "%06d.txt" % idx), "w") as f:
            f.write("\n".join(lines))
    with open(os.path.join(path, "val.txt"), "w") as f:
        f.write("".join("%06d\n" % idx for idx in ids))
    return os.path.join(path, "label_2"), os.path.join(path, "val.txt")
