"""OUTPUT_DEPTH 'oracle' without a GPU: the rule every lane of decode_boxes_multi_kernel runs (csrc/decode_oracle_math.h, compiled for the
host by tests/shim/decode_oracle_host.cpp) against a float32 numpy restatement of the reference's get_oracle_depths
(model/head/detector_infer.py:239-278; box_iou, engine/visualize_infer.py:23-27) written here from the reference's text.

Expected everywhere: the choice per detection EXACTLY (-1 = the detection keeps the 'mean' row, else the column 0..3 of the single estimate it
takes; 0 = direct).  Three sets of cases: the rows the reference's own PostProcessor recorded (tests/golden/decode_only.npz), built cases on a
dyadic grid (every coordinate a multiple of 1/8, every depth of 1/4: each expression is exact in float32 and float64 alike) that hit every
branch of the rule -- asserted on the restatement's answer --, and seeded random cases whose IoUs keep a margin from 0.5."""
import ctypes
import math
import os
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
F = np.float32
COLUMN_MODES = ("direct", "keypoints_center", "keypoints_02", "keypoints_13")


# ---- the restatement ------------------------------------------------------------------------------------------------------------------------
def box_iou(a, b):
    """visualize_infer.py:23-27 on float32 scalars (0 / 0 = NaN)."""
    with np.errstate(invalid="ignore", divide="ignore"):
        inter = max(min(a[2], b[2]) - max(a[0], b[0]), 0) * max(min(a[3], b[3]) - max(a[1], b[1]), 0)
        return inter / ((a[2] - a[0]) * (a[3] - a[1]) + (b[2] - b[0]) * (b[3] - b[1]) - inter)


def gt_table(cls, boxes, depth, mask=None, slots=None):
    """(M, 8) float32 = reg_mask, cls_id, x1, y1, x2, y2, depth, 0; `slots` pads with empty slots."""
    n = len(cls)
    M = n if slots is None else slots
    t = np.zeros((M, 8), dtype=F)
    t[:n, 0] = 1 if mask is None else mask
    t[:n, 1], t[:n, 2:6], t[:n, 6] = cls, np.asarray(boxes, dtype=F).reshape(n, 4), depth
    return t


def restate(boxes, cls, score, thr, d, has_direct, gt, details=False):
    """get_oracle_depths over the detections with score >= thr (detector_infer.py:102-119 keeps those alone) -> choice (N,) [, per detection
    (nearest slot of the table, its distances, the IoU, the depth differences)]."""
    boxes, d, gt = np.asarray(boxes, dtype=F), np.asarray(d, dtype=F), np.asarray(gt, dtype=F)
    slots = np.nonzero(gt[:, 0] != 0)[0]                              # the reference's masked tensors, in slot order
    gcls, gbox, gdep = gt[slots, 1].astype(np.int64), gt[slots, 2:6], gt[slots, 6]
    gcen = (gbox[:, :2] + gbox[:, 2:]) / F(2)
    first = 0 if has_direct else 1                                    # pred_combined_depths has three columns without depth_uncertainty
    choice, info = -np.ones(len(boxes), dtype=np.int32), [None] * len(boxes)
    for i in range(len(boxes)):
        if not score[i] >= thr or len(slots) == 0:
            continue
        cen = (boxes[i, :2] + boxes[i, 2:]) / F(2)
        dis = np.sum((cen.reshape(1, 2) - gcen) ** 2, axis=1, dtype=F)
        dis[gcls != int(cls[i])] = 9999
        near = int(np.argmin(dis))
        iou = box_iou(boxes[i], gbox[near])
        diff = np.abs(d[i, first:] - gdep[near])
        info[i] = (int(slots[near]), dis, iou, diff)
        if iou < 0.5:
            continue
        choice[i] = first + int(np.argmin(diff))
    return (choice, info) if details else choice


# ---- the shim -----------------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def shim(tmp_path_factory):
    so = str(tmp_path_factory.mktemp("shim") / "libdecode_oracle_shim.so")
    r = subprocess.run(["g++", "-O2", "-std=c++17", "-ffp-contract=off", "-shared", "-fPIC", "-o", so,
                        os.path.join(ROOT, "tests", "shim", "decode_oracle_host.cpp")], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    lib = ctypes.CDLL(so)
    V, I = ctypes.c_void_p, ctypes.c_int
    lib.shim_oracle_choose.argtypes, lib.shim_oracle_choose.restype = [V, V, V, ctypes.c_float, V, I, V, I, I, V], None
    lib.shim_oracle_nearest.argtypes, lib.shim_oracle_nearest.restype = [V, I, V, I], I
    lib.shim_oracle_iou_2d.argtypes, lib.shim_oracle_iou_2d.restype = [V, V], ctypes.c_float
    lib.shim_oracle_centre_dis.argtypes, lib.shim_oracle_centre_dis.restype = [V, V], ctypes.c_float
    return lib


def run_shim(lib, boxes, cls, score, thr, d, has_direct, gt):
    boxes, d, gt = (np.ascontiguousarray(a, dtype=F) for a in (boxes, d, gt))
    cls, score = np.ascontiguousarray(cls, dtype=np.int32), np.ascontiguousarray(score, dtype=F)
    out = np.full(len(boxes), -7, dtype=np.int32)
    lib.shim_oracle_choose(boxes.ctypes.data, cls.ctypes.data, score.ctypes.data, thr, d.ctypes.data, int(has_direct), gt.ctypes.data,
                           gt.shape[0], len(boxes), out.ctypes.data)
    return out


# ---- 1: the rows the reference recorded -----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n,matched", [(0, 19), (1, 5)])
def test_reference_fixtures(shim, n, matched):
    """The recorded rows of 'mean' and of the four single-estimate modes + the recorded ground truth -> the shim's choice per row reproduces
    the recorded 'oracle' rows exactly.  (All recorded rows passed the score threshold; column 13 is the scaled score, so the threshold is
    not exercised here.  direct is never the choice, and the keypoint columns partly coincide on the depth clamp.)"""
    g = np.load(os.path.join(ROOT, "tests", "golden", "decode_only.npz"))
    rows = {m: g["case%d_result_%s" % (n, m)] for m in ("mean",) + COLUMN_MODES}
    want = g["case%d_result_oracle" % n]
    gt = gt_table(g["case%d_gt_cls" % n], g["case%d_gt_boxes" % n], g["case%d_gt_depth" % n], slots=g["case%d_gt_cls" % n].shape[0] + 2)
    mean = rows["mean"]
    d = np.stack([rows[m][:, 11] for m in COLUMN_MODES], axis=1)
    args = (mean[:, 2:6], mean[:, 0].astype(np.int32), np.ones(len(mean), dtype=F), 0.5, d, True, gt)
    got = run_shim(shim, *args)
    assert np.array_equal(got, restate(*args))
    assert int((got >= 0).sum()) == matched and not (got == 0).any()
    picked = np.stack([rows["mean" if c < 0 else COLUMN_MODES[c]][i] for i, c in enumerate(got)])
    assert np.array_equal(picked, want)


# ---- 2: built cases on a dyadic grid --------------------------------------------------------------------------------------------------------
def _det(box, cls, d, score=0.9):
    return dict(box=box, cls=cls, d=d, score=score)


def built_cases():
    """name -> (detections, has_direct, table).  Coordinates in 1/8 px, depths in 1/4 m."""
    car = [16.0, 16.0, 80.0, 48.0]                                   # 64 x 32
    D = [10.0, 20.0, 30.0, 40.0]
    cases = {}
    # every choice: the same box matched to objects whose depth sits next to each column; one detection far from everything
    cases["each_column"] = (
        [_det([16.0 + 200 * k, 16.0, 80.0 + 200 * k, 48.0], 0, D) for k in range(4)] + [_det([16.0, 300.0, 80.0, 332.0], 0, D)], True,
        gt_table([0] * 4, [[16.125 + 200 * k, 16.0, 80.125 + 200 * k, 48.0] for k in range(4)], [10.25, 19.75, 30.5, 47.0], slots=6))
    cases["no_valid_slot"] = ([_det(car, 0, D)], True, gt_table([0, 0], [car, car], [10.0, 10.0], mask=0))
    # objects of another class only: the first valid slot (slot 1: slot 0 is masked out) is "nearest" and is tested -- here it matches
    cases["other_class_only"] = ([_det(car, 0, D), _det([200.0, 16.0, 264.0, 48.0], 0, D)], True,
                                 gt_table([0, 1, 2], [car, car, [200.0, 16.0, 264.0, 48.0]], [10.0, 30.25, 10.0], mask=[0, 1, 1]))
    # a same-class object 104 px away (dis = 10816 > 9999) would match (IoU 296 / 504); the earlier other-class slot, at 9999, is nearer
    cases["beyond_9999"] = ([_det([0.0, 0.0, 400.0, 200.0], 0, D)], True,
                            gt_table([1, 0], [[600.0, 300.0, 664.0, 332.0], [104.0, 0.0, 504.0, 200.0]], [20.0, 20.0]))
    # two same-class objects at -8 / +8 px: equal distances, the first wins (its depth selects column 2, the other's column 3)
    cases["distance_tie"] = ([_det(car, 0, D)], True, gt_table([0, 0], [[8.0, 16.0, 72.0, 48.0], [24.0, 16.0, 88.0, 48.0]], [30.0, 40.0]))
    # depth 25 is equally far from columns 1 and 2: the first wins
    cases["depth_tie"] = ([_det(car, 0, D)], True, gt_table([0], [car], [25.0]))
    # intersection 64, union 128
    cases["iou_half"] = ([_det([0.0, 0.0, 8.0, 8.0], 0, D)], True, gt_table([0], [[0.0, 0.0, 8.0, 16.0]], [40.0]))
    cases["iou_below_half"] = ([_det([0.0, 0.0, 8.0, 8.0], 0, D)], True, gt_table([0], [[0.0, 0.0, 8.0, 16.125]], [40.0]))
    # two empty boxes: 0 / 0
    cases["zero_over_zero"] = ([_det([4.0, 4.0, 4.0, 4.0], 0, D)], True, gt_table([0], [[4.0, 4.0, 4.0, 4.0]], [20.0]))
    # without depth_uncertainty the direct column is not offered although it is the closest
    cases["three_columns"] = ([_det(car, 0, D), _det([200.0, 16.0, 264.0, 48.0], 0, D)], False,
                              gt_table([0, 0], [car, [200.0, 16.0, 264.0, 48.0]], [10.0, 36.0]))
    cases["below_threshold"] = ([_det(car, 0, D, score=0.125), _det(car, 0, D, score=0.25)], True, gt_table([0], [car], [20.0]))
    return cases


THRESHOLD = 0.25


def _arrays(dets):
    return (np.array([x["box"] for x in dets], dtype=F), np.array([x["cls"] for x in dets], dtype=np.int32),
            np.array([x["score"] for x in dets], dtype=F), THRESHOLD, np.array([x["d"] for x in dets], dtype=F))


def test_built_cases(shim):
    seen = set()
    answers = {}
    for name, (dets, has_direct, gt) in built_cases().items():
        b, c, s, thr, d = _arrays(dets)
        assert np.array_equal(b * 8, np.round(b * 8)) and np.array_equal(gt[:, 2:6] * 8, np.round(gt[:, 2:6] * 8))       # the dyadic grid
        assert np.array_equal(d * 4, np.round(d * 4)) and np.array_equal(gt[:, 6] * 4, np.round(gt[:, 6] * 4))
        want, info = restate(b, c, s, thr, d, has_direct, gt, details=True)
        got = run_shim(shim, b, c, s, thr, d, has_direct, gt)
        assert np.array_equal(got, want), (name, got.tolist(), want.tolist())
        answers[name] = (want.tolist(), info)
        seen |= set(want.tolist())
    # ... and the cases are what they claim to be, by the restatement's own answer
    assert seen == {-1, 0, 1, 2, 3}
    assert answers["each_column"][0] == [0, 1, 2, 3, -1]
    assert answers["no_valid_slot"][0] == [-1] and answers["no_valid_slot"][1][0] is None
    want, info = answers["other_class_only"]
    assert want == [2, -1] and info[0][0] == 1 and info[1][0] == 1 and (info[0][1] == 9999).all()      # slot 1 is tested by both; one matches
    want, info = answers["beyond_9999"]
    assert want == [-1] and info[0][0] == 0 and info[0][2] == 0
    b = _arrays(built_cases()["beyond_9999"][0])[0][0]
    far = built_cases()["beyond_9999"][2][1, 2:6]
    assert ((b[0] + b[2]) / 2 - (far[0] + far[2]) / 2) ** 2 > 9999 and box_iou(b, far) >= 0.5          # it would have matched
    want, info = answers["distance_tie"]
    assert want == [2] and info[0][0] == 0 and info[0][1][0] == info[0][1][1] == 64
    want, info = answers["depth_tie"]
    assert want == [1] and info[0][3][1] == info[0][3][2] == 5
    assert answers["iou_half"][0] == [3] and answers["iou_half"][1][0][2] == 0.5
    assert answers["iou_below_half"][0] == [-1] and 0.49 < answers["iou_below_half"][1][0][2] < 0.5
    assert answers["zero_over_zero"][0] == [1] and math.isnan(answers["zero_over_zero"][1][0][2])
    assert answers["three_columns"][0] == [1, 3]
    dets, has_direct, gt = built_cases()["three_columns"]
    assert restate(*_arrays(dets), True, gt).tolist() == [0, 3]                                        # with the direct column offered
    assert answers["below_threshold"][0] == [-1, 1]                                                    # the same box at the threshold is matched


def test_pair_arithmetic(shim):
    """The IoU and the centre distance on the host are the restatement's float32 values, NaN included."""
    rng = np.random.default_rng(11)
    for _ in range(2000):
        p, q = (rng.uniform(0, 300, 2).astype(F) for _ in range(2))
        a = np.concatenate((p, p + rng.uniform(0, 120, 2).astype(F))).astype(F)
        b = np.concatenate((q, q + rng.uniform(0, 120, 2).astype(F))).astype(F)
        if rng.random() < 0.5:
            b = (a + rng.uniform(-6, 6, 4)).astype(F)
        got, want = shim.shim_oracle_iou_2d(a.ctypes.data, b.ctypes.data), F(box_iou(a, b))
        assert got == want or (math.isnan(got) and math.isnan(want))
        ca, cb = (a[:2] + a[2:]) / F(2), (b[:2] + b[2:]) / F(2)
        assert shim.shim_oracle_centre_dis(a.ctypes.data, b.ctypes.data) == np.sum((ca - cb) ** 2, dtype=F)
    z = np.zeros(4, dtype=F)
    assert math.isnan(shim.shim_oracle_iou_2d(z.ctypes.data, z.ctypes.data))


# ---- 3: seeded random cases -----------------------------------------------------------------------------------------------------------------
RANDOM_K, RANDOM_M = 50, 12
RANDOM_SEEDS = (1, 2, 10)                                             # one per image; chosen so that every case meets random_case's condition


def random_case(seed):
    """K detections, M slots (nine valid).  Two thirds of the detections are jittered copies of an object.  -> the arrays, the margin (four
    times the largest |float32 - float64| of box_iou over all the case's (detection, object) pairs) and whether the case is usable:
    every (detection, nearest object) IoU at least the margin away from 0.5, and the minimum of every distance list and of every
    depth-difference list attained once (the literal 9999 of other-class slots apart)."""
    rng = np.random.default_rng(seed)
    K, M = RANDOM_K, RANDOM_M
    p = rng.uniform(0, 1000, (M, 2))
    gbox = np.concatenate((p, p + rng.uniform(20, 200, (M, 2))), axis=1).astype(F)
    gt = gt_table(rng.integers(0, 3, M), gbox, rng.uniform(2, 60, M).astype(F), mask=(rng.random(M) < 0.75).astype(F))
    gt[[0, 5], 0] = (0, 1)
    src = rng.integers(0, M, K)
    boxes = (gbox[src] + rng.uniform(-1, 1, (K, 4)) * np.tile(gbox[src, 2:] - gbox[src, :2], (1, 2)) * rng.choice([0.05, 0.15, 0.3], (K, 1))).astype(F)
    far = rng.random(K) < 1 / 3
    q = rng.uniform(0, 1000, (K, 2))
    boxes[far] = np.concatenate((q, q + rng.uniform(20, 200, (K, 2))), axis=1).astype(F)[far]
    cls = np.where(rng.random(K) < 0.8, gt[src, 1], rng.integers(0, 3, K)).astype(np.int32)
    score = rng.uniform(0.1, 1.0, K).astype(F)
    d = rng.uniform(2, 60, (K, 4)).astype(F)
    f64 = lambda a, b: float(box_iou(a.astype(np.float64), b.astype(np.float64)))
    valid = np.nonzero(gt[:, 0] != 0)[0]
    margin = 4 * max(abs(float(box_iou(boxes[i], gt[j, 2:6])) - f64(boxes[i], gt[j, 2:6])) for i in range(K) for j in valid)
    choice, info = restate(boxes, cls, np.ones(K, dtype=F), 0.5, d, True, gt, details=True)
    ok = True
    for i in range(K):
        near, dis, iou, diff = info[i]
        diff3 = np.abs(d[i, 1:] - gt[near, 6])
        ok &= abs(f64(boxes[i], gt[near, 2:6]) - 0.5) >= margin and abs(float(iou) - 0.5) >= margin
        ok &= int((dis == dis.min()).sum()) == 1 or float(dis.min()) == 9999     # (the literal may repeat: then the first slot, by rule)
        ok &= int((diff == diff.min()).sum()) == 1 and int((diff3 == diff3.min()).sum()) == 1
    return dict(boxes=boxes, cls=cls, score=score, d=d, gt=gt, margin=margin, ok=bool(ok))


@pytest.mark.parametrize("has_direct", [True, False])
def test_random_cases(shim, has_direct):
    assert len(RANDOM_SEEDS) == 3
    matched = 0
    for seed in RANDOM_SEEDS:
        c = random_case(seed)
        assert c["ok"] and 0 <= c["margin"] < 1e-5, (seed, c["margin"])                                # no case is dropped: the seeds are fixed
        args = (c["boxes"], c["cls"], c["score"], 0.3, c["d"], has_direct, c["gt"])
        want = restate(*args)
        got = run_shim(shim, *args)
        assert np.array_equal(got, want), (seed, np.nonzero(got != want)[0].tolist())
        assert int((want >= 0).sum()) >= 8 and int((want < 0).sum()) >= 8
        matched += int((want >= 0).sum())
    assert matched >= 30
