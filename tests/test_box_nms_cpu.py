"""Duplicate suppression (TEST.USE_NMS '2d' / '3d', TEST.NMS_THRESH, TEST.NMS_CLASS_AGNOSTIC) without a GPU: the configuration keys and the
refusals at construction, the float64 restatement (tests/box_nms_ref.py) on cases with known answers, then ops.box_nms on CPU tensors and
the kernel's own per-image function (csrc/box_nms_math.h compiled for the host) against that restatement on the shared case table.

Expected everywhere: the mask EXACTLY.  The table keeps every pair IoU at least a margin away from every threshold (3D: 1e-4, the bound
mfx_box3d_iou_pairs is held to; 2D: four times the largest float32-float64 difference of _box_iou over the case's own boxes), so that
rounding cannot flip a comparison."""
import ctypes
import math
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "tests")):
    if p not in sys.path:
        sys.path.insert(0, p)

import box_nms_ref as N                                             # noqa: E402

YAML_FILE = os.path.join(ROOT, "runs", "monoflex.yaml")
KIND_ID = {"2d": 1, "3d": 2}


# ---- configuration ------------------------------------------------------------------------------------------------------------------------
def test_defaults_are_the_references():
    from monoflex_amd.config import get_cfg
    for cfg in (get_cfg(), get_cfg(YAML_FILE)):
        T = cfg.TEST
        assert T.USE_NMS == 'none' and T.NMS_THRESH == -1. and T.NMS_CLASS_AGNOSTIC is False and T.EVAL_DEPTH_METHODS == []


def test_keys_from_opts_and_from_a_yaml(tmp_path):
    from monoflex_amd.config import get_cfg
    from monoflex_amd.model.head.detector_infer import make_post_processor
    cfg = get_cfg(YAML_FILE, ["TEST.USE_NMS", "3d", "TEST.NMS_THRESH", "0.45", "TEST.NMS_CLASS_AGNOSTIC", "True",
                              "TEST.EVAL_DEPTH_METHODS", "['soft', 'hard']"])
    assert (cfg.TEST.USE_NMS, cfg.TEST.NMS_THRESH, cfg.TEST.NMS_CLASS_AGNOSTIC, cfg.TEST.EVAL_DEPTH_METHODS) == ('3d', 0.45, True, ['soft', 'hard'])
    post = make_post_processor(cfg)
    assert (post.use_nms, post.nms_thresh, post.nms_class_agnostic) == ('3d', 0.45, True)
    y = tmp_path / "nms.yaml"
    y.write_text("TEST:\n  USE_NMS: '2d'\n  NMS_THRESH: 0.3\n  NMS_CLASS_AGNOSTIC: False\n  EVAL_DEPTH_METHODS: ['direct']\n  DETECTIONS_PER_IMG: 40\n")
    assert get_cfg(str(y)).TEST.USE_NMS == '2d'
    cfg = get_cfg(YAML_FILE)
    cfg.merge_from_file(str(y))                                      # the experiment file, then the user's
    assert (cfg.TEST.USE_NMS, cfg.TEST.NMS_THRESH, cfg.TEST.NMS_CLASS_AGNOSTIC, cfg.TEST.EVAL_DEPTH_METHODS) == ('2d', 0.3, False, ['direct'])
    assert cfg.TEST.DETECTIONS_PER_IMG == 40
    post = make_post_processor(cfg)
    assert (post.use_nms, post.nms_thresh, post.nms_class_agnostic) == ('2d', 0.3, False)
    none = make_post_processor(get_cfg(YAML_FILE))
    assert none.use_nms == 'none'


@pytest.mark.parametrize("opts,error,word", [
    (["TEST.USE_NMS", "bev"], ValueError, "USE_NMS"),
    (["TEST.USE_NMS", "3d"], ValueError, "NMS_THRESH"),                                   # the default threshold, -1: "not set"
    (["TEST.USE_NMS", "2d", "TEST.NMS_THRESH", "1.0"], ValueError, "NMS_THRESH"),
    (["TEST.USE_NMS", "3d", "TEST.NMS_THRESH", "1.5"], ValueError, "NMS_THRESH"),
    (["TEST.USE_NMS", "3d", "TEST.NMS_THRESH", "0.5", "TEST.DETECTIONS_PER_IMG", "129"], NotImplementedError, "DETECTIONS_PER_IMG"),
])
def test_refused_at_construction(opts, error, word):
    from monoflex_amd.config import get_cfg
    from monoflex_amd.model.head.detector_infer import make_post_processor
    with pytest.raises(error, match=word):
        make_post_processor(get_cfg(YAML_FILE, opts))


def test_accepted_at_construction():
    from monoflex_amd.config import get_cfg
    from monoflex_amd.model.head.detector_infer import make_post_processor
    make_post_processor(get_cfg(YAML_FILE, ["TEST.USE_NMS", "3d", "TEST.NMS_THRESH", "0.0", "TEST.DETECTIONS_PER_IMG", "128"]))
    make_post_processor(get_cfg(YAML_FILE, ["TEST.NMS_THRESH", "7", "TEST.DETECTIONS_PER_IMG", "200"]))      # 'none': the other keys are not read


# ---- the restatement on known answers -------------------------------------------------------------------------------------------------------
def test_reference_known_answers():
    assert N.iou_2d((0, 0, 2, 2), (1, 0, 3, 2)) == pytest.approx(1 / 3, abs=1e-15) and N.iou_2d((0, 0, 2, 2), (5, 5, 6, 6)) == 0.0
    assert math.isnan(N.iou_2d((1, 0, 1, 2), (1, 0, 1, 2)))
    for t in N.THRESHOLDS:
        c = N.case("chain", t)
        r = 0.75 * (1 - t) / (1 + t)
        ab, ac = (1 - r) / (1 + r), max(0.0, (1 - 2 * r) / (1 + 2 * r))
        for kind in N.KINDS:
            m = c["iou"][kind][0]                                    # slots C, A, B
            assert m[1, 2] == pytest.approx(ab, abs=1e-5) and m[2, 0] == pytest.approx(ab, abs=1e-5) and m[1, 0] == pytest.approx(ac, abs=1e-5)
            assert ab > t > ac
            assert N.expected("chain", kind, False, t)[1].tolist() == [[1, 1, 0], [1, 1, 1]]     # C is kept: the suppressed B suppresses nothing
            assert N.expected("chain", kind, True, t)[1].tolist() == [[1, 1, 0], [1, 1, 0]]
    for kind in N.KINDS:
        for t in N.THRESHOLDS:
            assert np.nonzero(N.expected("identical", kind, False, t)[1][0])[0].tolist() == [17]
            assert np.nonzero(N.expected("identical_equal", kind, True, t)[1][0])[0].tolist() == [0]
            assert N.expected("class_pair", kind, False, t)[1].tolist() == [[1, 1]] and N.expected("class_pair", kind, True, t)[1].tolist() == [[1, 0]]
            assert N.expected("degenerate_2d", kind, True, t)[1].tolist() == ([[1, 1]] if kind == "2d" else [[1, 0]])


def test_the_table_means_something():
    """Every clustered image sees a suppression and a survivor under every setting; ties are decided by slot order; invalid rows stay
    invalid; every case stays clear of the thresholds by its margins."""
    tie_cases = 0
    for name, kind, agnostic, t in N.table():
        c, want = N.expected(name, kind, agnostic, t)
        assert c["gap"][kind] >= c["margin"][kind]
        assert not (want & (c["valid"] == 0)).any()
        if name in N.CLUSTERED:
            for b in range(want.shape[0]):
                assert 1 <= want[b].sum() < c["valid"][b].sum(), (name, kind, agnostic, t, b)
        tie_cases += int((N.expected(name, kind, agnostic, t, tie_to_higher_slot=True)[1] != want).any())
    assert tie_cases >= 1
    assert N.case("empty_image")["valid"][1].sum() == 0 and N.case("clusters")["valid"].mean() == pytest.approx(0.8, abs=0.1)
    print("settings whose mask depends on the tie rule: %d; margins %s" % (tie_cases, {n: N.case(n, 0.5 if n == "chain" else None)["margin"] for n in N.CASES}))


# ---- ops.box_nms on CPU tensors ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name,kind,agnostic,thresh", N.table())
def test_op_on_cpu_tensors(name, kind, agnostic, thresh):
    from monoflex_amd import ops
    c, want = N.expected(name, kind, agnostic, thresh)
    det, valid = torch.from_numpy(c["det"]), torch.from_numpy(c["valid"])
    before = det.clone()
    got = ops.box_nms(det, valid, kind, thresh, class_agnostic=agnostic)
    assert got.dtype == torch.int32 and got.shape == valid.shape and torch.equal(det, before)
    assert np.array_equal(got.numpy(), want)


def test_op_refuses_bad_arguments():
    from monoflex_amd import ops
    det, valid = torch.zeros(1, 4, 14), torch.ones(1, 4, dtype=torch.int32)
    with pytest.raises(ValueError, match="kind"):
        ops.box_nms(det, valid, "bev", 0.5)
    for t in (-0.1, 1.0, float("nan")):
        with pytest.raises(ValueError, match="thresh"):
            ops.box_nms(det, valid, "3d", t)
    with pytest.raises(RuntimeError):
        ops.box_nms(torch.zeros(1, 4, 13), valid, "3d", 0.5)
    with pytest.raises(TypeError):
        ops.box_nms(det, valid.long(), "3d", 0.5)


# ---- the kernel's per-image function, compiled for the host ------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def nms_shim(tmp_path_factory):
    so = str(tmp_path_factory.mktemp("shim") / "libbox_nms_shim.so")
    r = subprocess.run(["g++", "-O2", "-std=c++17", "-ffp-contract=off", "-shared", "-fPIC", "-o", so,
                        os.path.join(ROOT, "tests", "shim", "box_nms_host.cpp")], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    lib = ctypes.CDLL(so)
    lib.shim_box_nms.argtypes = [ctypes.c_void_p, ctypes.c_void_p] + [ctypes.c_int] * 3 + [ctypes.c_float, ctypes.c_int, ctypes.c_int, ctypes.c_void_p]
    lib.shim_box_nms.restype = None
    lib.shim_box_nms_pair.argtypes = [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_int, ctypes.c_void_p]
    lib.shim_box_nms_pair.restype = None
    lib.shim_box_nms_iou_2d.argtypes = [ctypes.c_void_p, ctypes.c_void_p]
    lib.shim_box_nms_iou_2d.restype = ctypes.c_float
    return lib


def _run_shim(lib, det, valid, kind, thresh, agnostic, early_out=1, alias=False):
    det, valid = np.ascontiguousarray(det, dtype=np.float32), np.ascontiguousarray(valid, dtype=np.int32)
    out = valid.copy() if alias else np.full(valid.shape, -7, dtype=np.int32)
    lib.shim_box_nms(det.ctypes.data, out.ctypes.data if alias else valid.ctypes.data, det.shape[0], det.shape[1], KIND_ID[kind], thresh,
                     int(agnostic), early_out, out.ctypes.data)
    return out


@pytest.mark.parametrize("name,kind,agnostic,thresh", N.table())
def test_kernel_function_on_the_host(nms_shim, name, kind, agnostic, thresh):
    c, want = N.expected(name, kind, agnostic, thresh)
    got = _run_shim(nms_shim, c["det"], c["valid"], kind, thresh, agnostic)
    assert np.array_equal(got, want), (np.argwhere(got != want).tolist())
    # the conservative early-out changes nothing, and neither does writing the result over the input mask
    assert np.array_equal(_run_shim(nms_shim, c["det"], c["valid"], kind, thresh, agnostic, early_out=0), want)
    assert np.array_equal(_run_shim(nms_shim, c["det"], c["valid"], kind, thresh, agnostic, alias=True), want)


def test_pair_arithmetic_on_the_host(nms_shim):
    """The rotated IoU with caller-owned clip rings is bit for bit biou::iou_rows (at stride 1 and at a table stride), within the operator's
    bound of float64, and exactly 0 wherever the early-out declares a pair far apart -- on every pair of the clustered cases and on random
    pairs around the early-out's boundary.  The 2D IoU is _box_iou in float32, NaN included."""
    from monoflex_amd.model.head.detector_infer import _box_iou
    out = np.zeros(3, dtype=np.float32)
    far = near = 0
    pairs = []
    for name in ("clusters", "k128"):
        c = N.case(name)
        for b in range(c["det"].shape[0]):
            rows = np.nonzero(c["valid"][b])[0]
            pairs += [(c["det"][b, i], c["det"][b, j], c["iou"]["3d"][b][i, j]) for n, i in enumerate(rows) for j in rows[n + 1:]]
    rng = np.random.default_rng(9)
    base = N.case("clusters")["det"][0]
    for _ in range(3000):                                            # a second box at 0.6 .. 1.4 of the circles' touching distance, any bearing
        a = base[rng.integers(0, 50)].copy()
        b = base[rng.integers(0, 50)].copy()
        touch = 0.5 * (math.hypot(a[8], a[7]) + math.hypot(b[8], b[7]))
        d, phi = touch * rng.uniform(0.6, 1.4), rng.uniform(0, 2 * math.pi)
        b[9], b[10], b[11] = a[9] + d * math.cos(phi), a[10] + rng.uniform(-0.3, 0.3), a[11] + d * math.sin(phi)
        pairs.append((a, b, None))
    for a, b, ref in pairs:
        a, b = np.ascontiguousarray(a, dtype=np.float32), np.ascontiguousarray(b, dtype=np.float32)
        nms_shim.shim_box_nms_pair(a.ctypes.data, b.ctypes.data, 1, out.ctypes.data)
        got, rows_form, is_far = float(out[0]), float(out[1]), bool(out[2])
        nms_shim.shim_box_nms_pair(a.ctypes.data, b.ctypes.data, 8, out.ctypes.data)
        assert got == rows_form == float(out[0])
        ref = N.pair_iou("3d", a, b) if ref is None else ref
        assert abs(got - ref) <= N.MARGIN_3D
        if is_far:
            far += 1
            assert got == 0.0 and ref == 0.0
        else:
            near += 1
        f32 = nms_shim.shim_box_nms_iou_2d(a[2:6].ctypes.data, b[2:6].ctypes.data)
        want = np.float32(_box_iou(a[2:6], b[2:6]))
        assert (math.isnan(f32) and math.isnan(want)) or f32 == want
    assert far > 1000 and near > 1000
    z = np.ascontiguousarray(N.case("degenerate_2d")["det"][0, 0])
    assert math.isnan(nms_shim.shim_box_nms_iou_2d(z[2:6].ctypes.data, z[2:6].ctypes.data))
