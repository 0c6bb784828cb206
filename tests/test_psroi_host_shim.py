"""CPU check of the pooling kernels' arithmetic: monoflex_amd/csrc/psroi_math.h compiled for the host by tests/shim/psroi_host.cpp
(test-only loops over the same per-bin functions the gfx950 kernels call, in float) against tests/psroi_ref.py in float64, forward and
both gradients, on the randomized cases of the GPU test.  Bound: 4x the error of the reference arithmetic evaluated in float32
(tests/psroi_ref.py, computed here on every run); output_count must be equal."""
import ctypes
import os
import subprocess

import numpy as np
import pytest

from tests import psroi_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
_F, _I, _P = ctypes.c_float, ctypes.c_int, ctypes.c_void_p


@pytest.fixture(scope="module")
def shim(tmp_path_factory):
    so = str(tmp_path_factory.mktemp("shim") / "libpsroi_shim.so")
    cmd = ["g++", "-O2", "-std=c++17", "-shared", "-fPIC", "-o", so, os.path.join(ROOT, "tests", "shim", "psroi_host.cpp")]
    r = subprocess.run(cmd, capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    lib = ctypes.CDLL(so)
    lib.shim_psroi_forward.argtypes = [_P] * 5 + [_I] * 7 + [_F] + [_I] * 4 + [_F]
    lib.shim_psroi_backward.argtypes = [_P] * 7 + [_I] * 7 + [_F] + [_I] * 4 + [_F]
    lib.shim_psroi_forward.restype = lib.shim_psroi_backward.restype = None
    return lib


def _p(a):
    return a.ctypes.data_as(_P) if a is not None else None


def run_shim(shim, d, no_trans):
    scale, output_dim, _, pooled, part, S, trans_std = d["args"]
    x, rois, go = [np.ascontiguousarray(d[k], dtype=np.float32) for k in ("input", "rois", "grad_out")]
    trans = None if no_trans else np.ascontiguousarray(d["trans"], dtype=np.float32)
    B, C, H, W = x.shape
    N = rois.shape[0]
    tc = 2 if no_trans else trans.shape[1]
    out = np.full((N, output_dim, pooled, pooled), 77, dtype=np.float32)           # poison: every element must be written
    cnt = np.full_like(out, 77)
    shim.shim_psroi_forward(_p(x), _p(rois), _p(trans), _p(out), _p(cnt), B, C, H, W, N, tc, int(no_trans), scale, output_dim, pooled, part, S, trans_std)
    gi = np.zeros_like(x)
    gt = None if no_trans else np.zeros_like(trans)
    shim.shim_psroi_backward(_p(go), _p(x), _p(rois), _p(trans), _p(cnt), _p(gi), _p(gt), B, C, H, W, N, tc, int(no_trans), scale, output_dim,
                             pooled, part, S, trans_std)
    return out, cnt, gi, gt


@pytest.mark.parametrize("no_trans", [True, False], ids=["no_trans", "offsets"])
@pytest.mark.parametrize("i", range(len(R.CASES)))
def test_shim_forward_and_grad_input_vs_float64(shim, i, no_trans):
    case = R.CASES[i]
    d = R.case_inputs(case)
    R.check_case_conditions(case, d, no_trans, need_grid=False)
    ref, err = R.reference_pair(d, no_trans)
    out, cnt, gi, _ = run_shim(shim, d, no_trans)
    what = "shim case %d %s" % (i, "no_trans" if no_trans else "offsets")
    assert np.array_equal(cnt.astype(np.float64), ref["count"]), what
    R.compare("output", out, ref["output"], err["output"], what)
    R.compare("grad_input", gi, ref["grad_input"], err["grad_input"], what)


@pytest.mark.parametrize("i", range(len(R.GOFF_CASES)))
def test_shim_grad_offset_vs_float64(shim, i):
    case = R.GOFF_CASES[i]
    d = R.case_inputs(case)
    R.check_case_conditions(case, d, False, need_grid=True)
    ref, err = R.reference_pair(d, False)
    out, cnt, gi, gt = run_shim(shim, d, False)
    what = "shim grad_offset case %d" % i
    assert np.array_equal(cnt.astype(np.float64), ref["count"]), what
    R.compare("output", out, ref["output"], err["output"], what)
    R.compare("grad_input", gi, ref["grad_input"], err["grad_input"], what)
    R.compare("grad_offset", gt, ref["grad_offset"], err["grad_offset"], what)
    assert np.abs(ref["grad_offset"]).max() > 1e-2
