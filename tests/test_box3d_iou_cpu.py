"""Rotated 3D box IoU (the logged `3D_IoU`; reference get_iou_3d, model/layers/iou_loss.py:99-136) without a GPU: the float64 reference
of tests/box3d_iou_ref.py against closed forms, then the kernel arithmetic of csrc/box3d_iou_math.h (compiled for the host) and the
extended per-object loss arithmetic (value slot 21) against that reference.

Bound everywhere: 1e-4 * max(1, |ref|) -- the project's bound for logged means (test_loss_golden.py) -- on EVERY generated pair: the
intersection area is continuous in the inputs, so no case is filtered."""
import ctypes
import math
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

import box3d_iou_ref as R                                           # noqa: E402

TOL = 1e-4


def close(have, ref):
    have, ref = np.asarray(have, dtype=np.float64), np.asarray(ref, dtype=np.float64)
    return np.abs(have - ref) <= TOL * np.maximum(1.0, np.abs(ref))


def known_answers():
    """(box a, box b, IoU in closed form) rows."""
    out = []
    # axis-aligned: product of the three interval overlaps.  a: x [-2, 2], z [19, 21], y [0.25, 1.75]; b: x [-1, 2], z [19.5, 22.5], y [0, 2]
    a, b = (0.0, 1.0, 20.0, 4.0, 1.5, 2.0, 0.0), (0.5, 1.0, 21.0, 3.0, 2.0, 3.0, 0.0)
    inter = 3.0 * 1.5 * 1.5
    out.append((a, b, inter / (4 * 1.5 * 2 + 3 * 2 * 3 - inter)))
    out.append((a, a, 1.0))                                          # identical
    r = (3.0, 1.2, 33.0, 3.9, 1.6, 1.7, 0.7)
    out.append((r, r, 1.0))                                          # identical, rotated
    out.append((a, (10.0, 1.0, 20.0, 4.0, 1.5, 2.0, 0.3), 0.0))      # disjoint in the plane
    out.append((a, (0.0, 3.0, 20.0, 4.0, 1.5, 2.0, 0.0), 0.0))       # disjoint in height
    s = 2.0                                                          # square of side s over itself turned by 45 degrees: 2 (sqrt 2 - 1) s^2
    inter = 2 * (math.sqrt(2) - 1) * s * s
    out.append(((5.0, 1.0, 40.0, s, 1.0, s, 0.0), (5.0, 1.0, 40.0, s, 1.0, s, math.pi / 4), inter / (2 * s * s - inter)))
    return out


# ---- the float64 reference against closed forms -----------------------------------------------------------------------------------
def test_reference_known_answers():
    for a, b, want in known_answers():
        assert abs(R.iou_boxes(a, b) - want) <= 1e-12, (a, b, R.iou_boxes(a, b), want)
    sq = [(-1, -1), (-1, 1), (1, 1), (1, -1)]
    dia = [(math.sqrt(2) * math.cos(t), math.sqrt(2) * math.sin(t)) for t in (0, math.pi / 2, math.pi, 1.5 * math.pi)]
    assert abs(R.intersection_area(sq, dia) - 2 * (math.sqrt(2) - 1) * 4) <= 1e-12
    assert abs(R.intersection_area(sq, sq[::-1]) - 4.0) <= 1e-12                      # orientation of either ring does not matter


def test_reference_symmetries():
    a, b = R.random_pairs(200, 1)
    for p, q in zip(a.astype(np.float64), b.astype(np.float64)):
        base = R.iou_boxes(p, q)
        assert 0.0 <= base <= 1.0 + 1e-12
        assert abs(R.iou_boxes(q, p) - base) <= 1e-12                                 # symmetric in (a, b)
        half = p.copy(); half[6] += math.pi                                           # a half turn is the same box
        assert abs(R.iou_boxes(half, q) - base) <= 1e-9
        quarter = p.copy(); quarter[6] += math.pi / 2; quarter[3], quarter[5] = p[5], p[3]      # a quarter turn with l and w swapped too
        assert abs(R.iou_boxes(quarter, q) - base) <= 1e-9


# ---- the kernel arithmetic, compiled for the host -----------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def iou_shim(tmp_path_factory):
    so = str(tmp_path_factory.mktemp("shim") / "libbox3d_iou_shim.so")
    r = subprocess.run(["g++", "-O2", "-std=c++17", "-ffp-contract=off", "-shared", "-fPIC", "-o", so,
                        os.path.join(ROOT, "tests", "shim", "box3d_iou_host.cpp")], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    lib = ctypes.CDLL(so)
    lib.shim_box3d_iou_pairs.argtypes = [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_int, ctypes.c_int, ctypes.c_void_p]
    lib.shim_box3d_iou_pairs.restype = None

    def run(a, b):
        a, b = np.ascontiguousarray(a, dtype=np.float32), np.ascontiguousarray(b, dtype=np.float32)
        out = np.full(a.shape[0], np.nan, dtype=np.float32)
        lib.shim_box3d_iou_pairs(a.ctypes.data, b.ctypes.data, a.shape[0], 0 if a.ndim == 2 else 1, out.ctypes.data)
        return out
    return run


def test_kernel_math_known_answers(iou_shim):
    rows = known_answers()
    a, b = np.array([r[0] for r in rows], dtype=np.float32), np.array([r[1] for r in rows], dtype=np.float32)
    want = np.array([r[2] for r in rows])
    for have in (iou_shim(a, b), iou_shim(b, a), iou_shim(R.corner_tables(a), R.corner_tables(b))):
        assert close(have, want).all(), (have, want)
    # a half turn / a quarter turn with l and w swapped describe the same box
    p, q = R.random_pairs(300, 2)
    base = iou_shim(p, q)
    half = p.copy(); half[:, 6] += np.float32(math.pi)
    quarter = p.copy(); quarter[:, 6] += np.float32(math.pi / 2); quarter[:, 3], quarter[:, 5] = p[:, 5], p[:, 3]
    assert close(iou_shim(half, q), base).all() and close(iou_shim(quarter, q), base).all()
    assert close(iou_shim(q, p), base).all()


@pytest.mark.parametrize("maker,n,seed", [(R.random_pairs, 2500, 3), (R.near_identical_pairs, 700, 4)])
def test_kernel_math_matches_float64_reference(iou_shim, maker, n, seed):
    a, b = maker(n, seed)
    ref0 = R.iou_pairs(a.astype(np.float64), b.astype(np.float64))
    have0 = iou_shim(a, b)
    err0 = np.abs(have0 - ref0)
    print("form 0: %d pairs, %d overlapping, max |err| %.3g" % (n, int((ref0 > 0).sum()), err0.max()))
    assert np.isfinite(have0).all() and close(have0, ref0).all(), (int(err0.argmax()), a[err0.argmax()], b[err0.argmax()], err0.max())
    ca, cb = R.corner_tables(a), R.corner_tables(b)
    ref1 = R.iou_pairs(ca.astype(np.float64), cb.astype(np.float64))
    have1 = iou_shim(ca, cb)
    err1 = np.abs(have1 - ref1)
    print("form 1: max |err| %.3g, max |form 1 - form 0| %.3g" % (err1.max(), np.abs(have1 - have0).max()))
    assert np.isfinite(have1).all() and close(have1, ref1).all(), (int(err1.argmax()), err1.max())
    assert close(have1, have0).all()                                 # the two forms of the same boxes agree
    if maker is R.random_pairs:
        assert (ref0 > 0.05).sum() > n // 10                         # the set does exercise overlapping boxes
    else:
        assert ref0.min() > 0.9


def test_kernel_math_degenerate_inputs(iou_shim):
    z = np.zeros((1, 7), dtype=np.float32)
    a, _ = R.random_pairs(4, 5)
    bad = a.copy()
    bad[0, 3] = 0.0                                                  # zero length
    bad[1, 4] = -1.0                                                 # negative height
    bad[2, 0] = np.nan
    bad[3, 2] = np.inf
    for x, y in ((z, z), (bad, a), (a, bad), (bad, bad)):
        out = iou_shim(x, y)
        assert np.isfinite(out).all() and (out >= 0).all(), out
        out = iou_shim(R.corner_tables(x), R.corner_tables(y))
        assert np.isfinite(out).all() and (out >= 0).all(), out
    assert iou_shim(z, z)[0] == 0.0 and iou_shim(np.zeros((1, 8, 3)), np.zeros((1, 8, 3)))[0] == 0.0


# ---- the Python surface on CPU tensors ----------------------------------------------------------------------------------------------
def test_get_iou_3d_on_cpu_tensors_matches_reference():
    from model.layers.iou_loss import get_iou_3d                     # the reference's import path
    from monoflex_amd.model.layers.iou_loss import get_iou_3d as same
    assert get_iou_3d is same
    a, b = R.random_pairs(300, 6)
    n, _ = R.near_identical_pairs(100, 7)
    a, b = np.concatenate((a, n)), np.concatenate((b, _))
    ca, cb = R.corner_tables(a), R.corner_tables(b)
    out = get_iou_3d(torch.from_numpy(ca), torch.from_numpy(cb))
    assert out.shape == (400,) and out.dtype == torch.float32
    assert close(out.numpy(), R.iou_pairs(ca.astype(np.float64), cb.astype(np.float64))).all()
    assert get_iou_3d(torch.zeros(0, 8, 3), torch.zeros(0, 8, 3)).shape == (0,)
    with pytest.raises(ValueError):
        get_iou_3d(torch.zeros(3, 7), torch.zeros(3, 7))


def test_box3d_iou_op_refuses_cpu_tensors():
    from monoflex_amd import ops
    with pytest.raises(RuntimeError, match="CPU tensor"):
        ops.box3d_iou(torch.zeros(2, 7), torch.zeros(2, 7))


# ---- value slot 21 of the per-object loss arithmetic -----------------------------------------------------------------------------------
from test_loss_golden import case_inputs, evaluator, object_loss_shim, run_object_shim          # noqa: E402,F401  (the fixture and its driver)


def shim_on_prepared(shim, ev, reg_nchw, tv):
    """run_object_shim on an already prepared (and possibly edited) target table."""
    from monoflex_amd import lib as L
    rows = tv["object_rows"].contiguous()
    reg = reg_nchw.permute(0, 2, 3, 1).contiguous()
    B, H, W, C = reg.shape
    vals, G = torch.zeros(L.OBJ_VALUES), torch.zeros(rows.shape[0], L.OBJ_TERMS, 64)
    cfg = ev.object_loss_cfg()
    shim.shim_object_loss(reg.data_ptr(), B, H, W, C, 0, rows.data_ptr(), rows.shape[0], ctypes.byref(cfg), vals.data_ptr(), G.data_ptr())
    return vals[:L.OBJ_TERMS], vals[L.OBJ_TERMS:], G


@pytest.mark.parametrize("name", ["b2", "b1_many"])
def test_object_loss_slot_is_the_mean_iou_on_golden_cases(name, object_loss_shim):
    from monoflex_amd.structures.params_3d import make_train_target
    tg, cls, reg = case_inputs(name)
    ev = evaluator()
    targets = [make_train_target(t) for t in tg]
    terms, logged, dreg, G, rows = run_object_shim(object_loss_shim, ev, reg, targets)
    _, tv = ev.prepare_targets(targets)
    ref = R.mean_iou_of_case(ev, reg, tv)
    print("%s: logged[11] %.6g, float64 mean IoU %.6g" % (name, float(logged[11]), ref))
    assert close(float(logged[11]), ref)
    assert float(logged[12:].abs().max()) == 0.0                     # the two spare slots stay zero


@pytest.mark.parametrize("name", ["b2", "b1_many", "b3_empty_middle_mixed_calib"])
def test_object_loss_slot_on_overlapping_boxes(name, object_loss_shim):
    """The golden cases decode random maps, whose boxes miss their targets; here the targets are moved onto the predictions."""
    ev = evaluator()
    cls, reg, heat, tv = R.overlapping_loss_case(ev, name)
    ref = R.mean_iou_of_case(ev, reg, tv)
    terms, logged, G = shim_on_prepared(object_loss_shim, ev, reg, tv)
    print("%s: logged[11] %.6g, float64 mean IoU %.6g" % (name, float(logged[11]), ref))
    assert ref > 0.2                                                 # the case does what it is for
    assert close(float(logged[11]), ref)
    # the tensor-op form of the loss logs the same value (CPU tensors: the host restatement of get_iou_3d), in the reference's key order
    ev.fused_object_loss = False
    _, logs = ev({"cls": cls, "reg": reg}, (heat, tv))
    assert list(logs)[:2] == ["2D_IoU", "3D_IoU"] and close(logs["3D_IoU"], ref)
    # values only: the other outputs are what the same arithmetic gives without the new slot (pinned on the goldens by test_loss_golden)
    assert float(G[..., 50:].abs().max()) == 0.0 and bool(torch.isfinite(G).all())


def test_object_loss_slot_without_objects(object_loss_shim):
    from monoflex_amd import synthetic as S
    from monoflex_amd.structures.params_3d import make_train_target
    reg = torch.randn(1, 50, 96, 320, generator=torch.Generator().manual_seed(1))
    targets = [make_train_target(S.synthetic_train_target(9, n_obj=0))]
    terms, logged, dreg, G, rows = run_object_shim(object_loss_shim, evaluator(), reg, targets)
    assert float(logged[11]) == 0.0
    ev = evaluator()
    ev.fused_object_loss = False
    cls = torch.sigmoid(torch.randn(1, 3, 96, 320, generator=torch.Generator().manual_seed(2)) - 3).clamp(1e-4, 1 - 1e-4)
    _, logs = ev({"cls": cls, "reg": reg}, targets)
    assert logs["3D_IoU"] == 0.0
