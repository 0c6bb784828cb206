"""Shared by the CPU and GPU tests of the resident split (monoflex_amd/data/resident.py, mfx_kitti_*_indexed): the generated
five-frame KITTI directory, and the host build of the indexed mapping (tests/shim/kitti_resident_host.cpp).  Comparisons are
exact everywhere: the indexed path runs the arithmetic of the batch path on the same inputs."""
import ctypes
import os
import subprocess

import numpy as np

from monoflex_amd import lib as L
from monoflex_amd import synthetic as S
from monoflex_amd.data import encode as E
from tests.kitti_right_common import make_kitti_dir
from tests.kitti_settings_common import NP_DTYPES

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
# odd width whose row bytes are no multiple of 4 (1241), no padding at all (1280x384), a tiny frame with an empty label file
SIZES = [(1242, 375), (1224, 370), (1241, 376), (1280, 384), (33, 17)]
# label seeds whose eight objects encode with status == 0 flipped and unflipped, as left and as right view, under the yaml and
# the config/defaults.py encoder settings (test_resident_cpu.py::test_fixture_samples_encode_cleanly re-checks it on the host)
LABEL_SEEDS = [52000, 52100, 52200, 52300]
N_OBJECTS = 8


def fixture_cases():
    """[(label lines, width, height)] of the five frames."""
    cases = [(S.synthetic_kitti_labels(seed, w, h, N_OBJECTS), w, h) for seed, (w, h) in zip(LABEL_SEEDS, SIZES)]
    return cases + [([], SIZES[4][0], SIZES[4][1])]


def make_tree(path, right_images=False):
    """The fixture as a KITTI folder with train and val splits over the same five frames."""
    return make_kitti_dir(path, fixture_cases(), splits=("train", "val"), right_images=right_images)


def build_resident_shim(directory):
    so = os.path.join(str(directory), "libkitti_resident_shim.so")
    cmd = ["g++", "-O2", "-std=c++17", "-ffp-contract=off", "-shared", "-fPIC", "-o", so,
           os.path.join(ROOT, "tests", "shim", "kitti_resident_host.cpp")]
    r = subprocess.run(cmd, capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    lib = ctypes.CDLL(so)
    lib.shim_kitti_encode_indexed.argtypes = [ctypes.POINTER(L.KittiDesc), ctypes.c_void_p, ctypes.c_int32, ctypes.c_void_p,
                                              ctypes.POINTER(L.KittiEncodeCfg)]
    lib.shim_kitti_encode_indexed.restype = None
    lib.shim_kitti_preprocess_indexed.argtypes = [ctypes.c_void_p] * 6 + [ctypes.c_int] * 4 + [ctypes.c_void_p] * 2 + [ctypes.c_int]
    lib.shim_kitti_preprocess_indexed.restype = None
    return lib


def shim_encode_indexed(shim, store, index, flips, params, rights=None, cfg="params"):
    """store: E.pack_inputs of all N store rows (its `flip` is unused); index / flips: per batch slot; rights: per store row.
    Outputs start poisoned, so every element must be written."""
    B, N, dims = len(index), len(store["n_obj"]), params.dims()
    out = {name: np.full((B,) + tuple(dims.get(s, s) for s in shape), 77, dtype=NP_DTYPES[dt])
           for name, (_, shape, dt) in E.TARGET_FIELDS.items()}
    idx, flip = np.asarray(index, dtype=np.int32).copy(), np.asarray([int(bool(f)) for f in flips], dtype=np.int32)
    d = L.KittiDesc()
    for k in ("records", "n_obj", "P", "img_wh"):
        setattr(d, k, store[k].ctypes.data)
    d.flip = flip.ctypes.data
    for name, (member, _, _) in E.TARGET_FIELDS.items():
        setattr(d, member, out[name].ctypes.data)
    d.B, d.max_objs, d.in_w, d.in_h, d.down, d.num_classes = B, params.max_objs, params.in_w, params.in_h, params.down, params.num_classes
    d.filter_trunc, d.filter_size, d.edge_ratio = params.filter_trunc, params.filter_size, params.edge_ratio
    right = None if rights is None else np.asarray(rights, dtype=np.int32).reshape(N).copy()
    c = params.encode_cfg() if isinstance(cfg, str) else cfg
    shim.shim_kitti_encode_indexed(ctypes.byref(d), idx.ctypes.data, N, None if right is None else right.ctypes.data,
                                   None if c is None else ctypes.byref(c))
    return out


def shim_frames_indexed(shim, pixels, offsets, img_wh, index, flips, to_bgr, in_w, in_h, mean, std):
    idx, flip = np.asarray(index, dtype=np.int32).copy(), np.asarray([int(bool(f)) for f in flips], dtype=np.int32)
    out = np.full((len(idx), 3, in_h, in_w), 77, dtype=np.float32)
    m3, s3 = np.asarray(mean, dtype=np.float32), np.asarray(std, dtype=np.float32)
    shim.shim_kitti_preprocess_indexed(pixels.ctypes.data, offsets.ctypes.data, img_wh.ctypes.data, idx.ctypes.data, flip.ctypes.data,
                                       out.ctypes.data, len(idx), len(offsets), in_w, in_h, m3.ctypes.data, s3.ctypes.data, int(to_bgr))
    return out
