"""Host build of the box decode (tests/shim/decode_row_host.cpp around monoflex_amd/csrc/box_decode_math.h) for the CPU tests: the arithmetic
of decode.hip's decode_boxes_kernel compiled with g++ -ffp-contract=off, called with the inputs of ops.decode_boxes."""
import ctypes
import os
import subprocess

import numpy as np

from monoflex_amd import lib as L

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def build(folder):
    """Compile the shim into `folder` -> run(d, cfg, heads, **edit) -> (det (B,K,14), topk (B,K,5), valid (B,K), unc (B,K,2)) float32 / int32.
    `d` is a case dict of tests/decode_cases.py; `edit` overrides ncls, K, ld or reg_off as passed to the entry.  A refused call raises
    ValueError with the message."""
    so = os.path.join(str(folder), "libdecode_row_shim.so")
    r = subprocess.run(["g++", "-O2", "-std=c++17", "-ffp-contract=off", "-shared", "-fPIC", "-o", so,
                        os.path.join(ROOT, "tests", "shim", "decode_row_host.cpp")], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    lib = ctypes.CDLL(so)
    P, I = ctypes.c_void_p, ctypes.c_int
    lib.shim_decode_boxes.argtypes = [P, I, I, P, P, I, I, I, I, I, P, P, P, ctypes.c_float, ctypes.POINTER(L.DecodeCfg), ctypes.POINTER(L.HeadLayout),
                                      P, P, P, P, ctypes.c_char_p]
    lib.shim_decode_boxes.restype = I

    def run(d, cfg, heads, **edit):
        hmap = np.ascontiguousarray(d["hmap"], dtype=np.float32)
        scores, index = np.ascontiguousarray(d["scores"], dtype=np.float32), np.ascontiguousarray(d["index"], dtype=np.int32)
        calib, pad = np.ascontiguousarray(d["calib"], dtype=np.float32), np.ascontiguousarray(d["pad"], dtype=np.int32)
        size = np.ascontiguousarray(d["img_size"], dtype=np.int32)
        B, H, W, ld = hmap.shape
        ncls, K = scores.shape[1:]
        det, topk, unc = (np.full((B, K, n), 7.75e8, dtype=np.float32) for n in (14, 5, 2))
        valid = np.full((B, K), -1, dtype=np.int32)
        why = ctypes.create_string_buffer(160)
        rc = lib.shim_decode_boxes(hmap.ctypes.data, edit.get("ld", ld), edit.get("reg_off", d["reg_off"]), scores.ctypes.data, index.ctypes.data,
                                   edit.get("ncls", ncls), B, H, W, edit.get("K", K), calib.ctypes.data, pad.ctypes.data, size.ctypes.data,
                                   float(d["threshold"]), None if cfg is None else ctypes.byref(cfg), None if heads is None else ctypes.byref(heads),
                                   det.ctypes.data, topk.ctypes.data, valid.ctypes.data, unc.ctypes.data, why)
        if rc:
            raise ValueError(why.value.decode())
        return det, topk, valid, unc
    return run
