"""GPU tests of the duplicate suppression (TEST.USE_NMS '2d' / '3d'; C ABI mfx_box_nms, ops.box_nms, PostProcessor).

Reference: tests/box_nms_ref.py, the float64 loop-form restatement of the semantics (the reference declares the keys and reads them nowhere).
Expected: the mask EXACTLY, on the case table tests/test_box_nms_cpu.py also runs: every pair IoU of it lies at least a margin away from
every threshold -- 3D: 1e-4, the absolute bound tests/test_gpu_box3d_iou.py holds mfx_box3d_iou_pairs to; 2D: four times the largest
float32-float64 difference of _box_iou over the case's own boxes -- so that rounding cannot flip a comparison.  No case is skipped."""
import ctypes
import os
import sys

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "tests")):
    if p not in sys.path:
        sys.path.insert(0, p)

import box_nms_ref as N                                             # noqa: E402

pytestmark = pytest.mark.gpu
DEV = "cuda"
YAML_FILE = os.path.join(ROOT, "runs", "monoflex.yaml")
KIND_ID = {"2d": 1, "3d": 2}


def _counter():
    from monoflex_amd import lib as L
    return int(L.load().mfx_get_counter(b"box_nms"))


def _entry(det, valid_in, valid_out, K, kind, thresh, agnostic, B=None):
    from monoflex_amd import lib as L
    from monoflex_amd.ops import _ptr, _stream
    return L.load().mfx_box_nms(_ptr(det), _ptr(valid_in), det.shape[0] if B is None else B, K, kind, ctypes.c_float(thresh), int(agnostic),
                                _ptr(valid_out), _stream())


# ---- the case table ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name,kind,agnostic,thresh", N.table())
def test_mask_is_exactly_the_reference(name, kind, agnostic, thresh):
    """ops.box_nms on CUDA tensors; and the C entry with valid_out aliasing valid_in gives the same mask."""
    from monoflex_amd import ops
    c, want = N.expected(name, kind, agnostic, thresh)
    assert c["gap"][kind] >= c["margin"][kind]
    det, valid = torch.from_numpy(c["det"]).to(DEV), torch.from_numpy(c["valid"]).to(DEV)
    before, count = det.clone(), _counter()
    got = ops.box_nms(det, valid, kind, thresh, class_agnostic=agnostic)
    alias = valid.clone()
    assert _entry(det, alias, alias, det.shape[1], KIND_ID[kind], thresh, agnostic) == 0
    torch.cuda.synchronize()
    assert _counter() == count + 2                                   # one launch per call, whatever B
    assert got.dtype == torch.int32 and got.is_cuda and torch.equal(det, before) and torch.equal(valid.cpu(), torch.from_numpy(c["valid"]))
    have = got.cpu().numpy()
    print("%s %s agnostic %d thresh %.1f: %d of %d valid rows kept; closest IoU to a threshold %.3g (margin %.3g)"
          % (name, kind, agnostic, thresh, have.sum(), c["valid"].sum(), c["gap"][kind], c["margin"][kind]))
    assert np.array_equal(have, want), np.argwhere(have != want).tolist()
    assert np.array_equal(alias.cpu().numpy(), want)


def test_more_than_128_rows_is_refused_without_a_launch():
    from monoflex_amd import lib as L, ops
    det, valid = torch.zeros(2, 129, 14, device=DEV), torch.ones(2, 129, dtype=torch.int32, device=DEV)
    out = torch.full((2, 129), -7, dtype=torch.int32, device=DEV)
    count = _counter()
    assert _entry(det, valid, out, 129, 2, 0.5, 0) == -2 and b"128" in L.load().mfx_last_error()
    with pytest.raises(RuntimeError, match="128"):
        ops.box_nms(det, valid, "3d", 0.5)
    torch.cuda.synchronize()
    assert _counter() == count and bool((out == -7).all())


def test_entry_checks_its_arguments_before_any_device_work():
    from monoflex_amd import lib as L
    lib = L.load()
    det, valid = torch.zeros(1, 4, 14, device=DEV), torch.ones(1, 4, dtype=torch.int32, device=DEV)
    out = torch.full((1, 4), -7, dtype=torch.int32, device=DEV)
    count = _counter()
    assert _entry(det, valid, out, 4, 0, 0.5, 0) == -1 and b"kind" in lib.mfx_last_error()
    assert _entry(det, valid, out, 4, 3, 0.5, 0) == -1
    for t in (-0.1, 1.0, 1.5, float("nan")):
        assert _entry(det, valid, out, 4, 2, t, 0) == -1 and b"thresh" in lib.mfx_last_error()
    assert _entry(det, valid, out, -1, 2, 0.5, 0) == -1
    assert _entry(det, None, out, 4, 2, 0.5, 0) == -1 and b"null" in lib.mfx_last_error()
    assert _entry(det, valid, out, 0, 2, 0.5, 0) == 0 and _entry(det, valid, out, 4, 2, 0.5, 0, B=0) == 0      # no rows: a successful no-op
    torch.cuda.synchronize()
    assert _counter() == count and bool((out == -7).all())
    assert _entry(det, valid, out, 4, 2, 0.0, 0) == 0               # thresh 0 is inside [0, 1)
    torch.cuda.synchronize()
    assert out.cpu().tolist() == [[1, 1, 1, 1]]                      # four all-zero rows: their IoU is 0 (2D: NaN), not > 0


# ---- through the post-processor ---------------------------------------------------------------------------------------------------------------
MAP_H, MAP_W = 6, 10            # K = 50 rows need H * W >= 50 (mfx_decode_topk: K <= H * W): the smallest map the decode accepts, with a spare row
FRAME = (40, 24)
P = np.array([[45.0, 0, 20.0, 0], [0, 45.0, 12.0, 0], [0, 0, 1, 0]])
# (image, class, (y, x) of the first peak, (dy, dx) to the second, score of the first, of the second); the third entry of an image stands alone
PEAKS = {0: ((0, 0, (2, 2), (0, 2), 0.8, 0.6), (0, 1, (4, 6), (0, 2), 0.5, 0.7), (0, 2, (1, 8), None, 0.55, None),
             (1, 2, (1, 1), (2, 0), 0.9, 0.45), (1, 0, (4, 5), (0, 2), 0.65, 0.6), (1, 1, (1, 7), None, 0.75, None)),
         1: ((0, 1, (3, 3), (0, 2), 0.6, 0.85), (0, 2, (1, 6), None, 0.7, None),
             (1, 0, (2, 6), (2, 0), 0.5, 0.8), (1, 0, (1, 2), None, 0.3, None), (1, 2, (4, 1), (0, 2), 0.9, 0.35))}


def head_map(variant):
    """fp32 (2, 6, 10, 64) head map: background class logits, and pairs of peaks 2 px apart in one class plane -- the 3x3 pool keeps both --
    whose regression rows point at the same projected centre (3d_offset +1 / -1 px) and the same 2D box, with depth, dimensions and
    orientation a touch apart: two detections of nearly the same box.  Every other pixel carries the same plain row."""
    from decode_ref import R_2D, R_DEPTH, R_DEPTH_UNC, R_DIM3D, R_OFF3D, R_ORI_CLS, R_ORI_OFF
    from monoflex_amd.model.head.detector_predictor import HM_LD, REG_OFF
    hm = np.zeros((2, MAP_H, MAP_W, HM_LD), dtype=np.float32)
    hm[..., 0:3] = -12.0
    row = np.zeros(50, dtype=np.float32)
    row[R_2D:R_2D + 4] = (1.0, 0.8, 1.0, 0.8)
    row[R_DEPTH], row[R_DEPTH_UNC] = -3.0, -3.0                      # inv_sigmoid: 1 / sigmoid(-3) - 1 = 20.1 m
    row[R_ORI_CLS:R_ORI_CLS + 8] = (0, 2, 0, -2, 0, -2, 0, -2)       # bin 0 wins
    row[R_ORI_OFF:R_ORI_OFF + 8:2], row[R_ORI_OFF + 1:R_ORI_OFF + 8:2] = 0.5, 0.8
    hm[..., REG_OFF:REG_OFF + 50] = row
    logit = lambda s: float(np.log(s / (1 - s)))
    for b, cls, (y, x), step, s0, s1 in PEAKS[variant]:
        hm[b, y, x, cls] = logit(s0)
        if step is None:
            continue
        dy, dx = step
        hm[b, y + dy, x + dx, cls] = logit(s1)
        first, second = hm[b, y, x, REG_OFF:REG_OFF + 50], hm[b, y + dy, x + dx, REG_OFF:REG_OFF + 50]
        first[R_OFF3D:R_OFF3D + 2] = (dx / 2, dy / 2)
        second[R_OFF3D:R_OFF3D + 2] = (-dx / 2, -dy / 2)
        # extents (left, top, right, bottom) in cells: the same box seen from either peak
        first[R_2D:R_2D + 4] = (1.0, 0.8, 1.0 + dx, 0.8 + dy)
        second[R_2D:R_2D + 4] = (1.0 + dx, 0.8 + dy, 1.0, 0.8)
        second[R_DEPTH] = -3.004
        second[R_DIM3D:R_DIM3D + 3] = (0.01, -0.01, 0.02)
        second[R_ORI_OFF] = 0.52
    return hm


def _targets():
    from monoflex_amd.structures.params_3d import Calibration, ParamsList
    out = []
    for _ in range(2):
        t = ParamsList(image_size=FRAME, is_train=False)
        t.add_field("pad_size", torch.tensor([0, 0]))
        t.add_field("calib", Calibration(P))
        out.append(t)
    return out


def _post(use_nms):
    from monoflex_amd.config import get_cfg
    from monoflex_amd.model.head.detector_infer import make_post_processor
    cfg = get_cfg(YAML_FILE, ["TEST.USE_NMS", use_nms, "TEST.NMS_THRESH", 0.5, "MODEL.HEAD.OUTPUT_DEPTH", "direct"])
    assert cfg.TEST.DETECTIONS_PER_IMG == 50
    return make_post_processor(cfg)


@pytest.fixture(scope="module")
def three_runs():
    """decode_device on head_map(0) under 'none', '2d' and '3d' -> {mode: (det, topk, valid, launches counted)} as numpy, and the inputs."""
    hm = torch.from_numpy(head_map(0)).to(DEV)
    runs = {}
    for mode in ("none", "2d", "3d"):
        post = _post(mode)
        tg = post.prepare_targets(_targets(), DEV)
        count = _counter()
        det, topk, valid = post.decode_device(hm, *tg)
        torch.cuda.synchronize()
        runs[mode] = (det.cpu().numpy(), topk.cpu().numpy(), valid.cpu().numpy(), _counter() - count)
    return hm, runs


def test_post_processor_decode_device(three_runs):
    from monoflex_amd import ops
    from monoflex_amd.model.head.detector_predictor import REG_OFF
    hm, runs = three_runs
    det, topk, valid, launches = runs["none"]
    assert launches == 0
    post = _post("none")
    pad, calib, size = post.prepare_targets(_targets(), DEV)
    scores, index = ops.decode_topk(hm, 0, 3, 50)
    d0, t0, v0 = ops.decode_boxes(hm, REG_OFF, scores, index, calib, pad, size, 0.2, depth_mode="direct", cfg=post.decode_cfg, heads=post.head_layout)
    torch.cuda.synchronize()
    assert np.array_equal(v0.cpu().numpy(), valid) and np.array_equal(d0.cpu().numpy(), det) and np.array_equal(t0.cpu().numpy(), topk)
    # the input does what it is for: every planted peak is a valid detection (the pool kept both of a pair) ...
    assert valid.sum(axis=1).tolist() == [5, 5]
    for mode in ("2d", "3d"):
        d, t, v, launches = runs[mode]
        assert launches == 1                                         # per call, not per image
        assert d.tobytes() == det.tobytes() and t.tobytes() == topk.tobytes()
        mats = N.iou_matrices(det, valid, mode)
        margin = N.MARGIN_3D if mode == "3d" else 4 * N.box_iou_f32_error(det, valid)
        assert N.gap_to_thresholds(mats, (0.5,)) >= margin
        want = N.nms(det, valid, mode, 0.5, False, iou=mats)
        print("%s: valid %s -> %s" % (mode, valid.sum(axis=1).tolist(), v.sum(axis=1).tolist()))
        assert np.array_equal(v, want)
        assert want.sum(axis=1).tolist() == [3, 3]                   # ... and each pair decodes to nearly one box: its lower-scoring peak goes


@pytest.mark.parametrize("mode", ["none", "2d", "3d"])
def test_post_processor_forward(three_runs, mode):
    """The result lists, vis_scores and the uncertainty lists follow the mask after the suppression; valid_pre_nms is the decode's own."""
    hm, runs = three_runs
    det, topk, valid, _ = runs[mode]
    post = _post(mode)
    assert post.uncertainty_as_conf
    results, utils, _ = post({"hm_nhwc": hm, "cls": None}, _targets())
    torch.cuda.synchronize()
    assert np.array_equal(utils["valid"].cpu().numpy(), valid) and np.array_equal(utils["det_all"].cpu().numpy(), det)
    if mode == "none":
        assert utils["valid_pre_nms"] is None
    else:
        assert np.array_equal(utils["valid_pre_nms"].cpu().numpy(), runs["none"][2]) and valid.sum() < runs["none"][2].sum()
    for b in range(2):
        keep = valid[b].astype(bool)
        assert np.array_equal(results[b].cpu().numpy(), det[b][keep])
        assert np.array_equal(utils["vis_scores"][b].cpu().numpy(), topk[b][keep, 0])
        assert len(utils["uncertainty_conf"][b]) == len(utils["estimated_depth_error"][b]) == int(keep.sum())
        assert np.array_equal(results[b].cpu().numpy()[:, 13], topk[b][keep, 0] * utils["uncertainty_conf"][b].cpu().numpy())


def test_decode_device_with_3d_nms_replays_from_a_captured_graph():
    """One stream, no parallel branches: the captured decode + suppression, replayed after the head map was overwritten in place, gives the
    eager result on the new map."""
    post = _post("3d")
    tg = post.prepare_targets(_targets(), DEV)
    first, second = torch.from_numpy(head_map(0)).to(DEV), torch.from_numpy(head_map(1)).to(DEV)
    hm = first.clone()
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        eager = {n: [t.clone() for t in post.decode_device(m, *tg)] for n, m in (("first", first), ("second", second))}
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        held = post.decode_device(hm, *tg)
    graph.replay()
    torch.cuda.synchronize()
    assert all(torch.equal(a, b) for a, b in zip(held, eager["first"]))
    hm.copy_(second)
    graph.replay()
    torch.cuda.synchronize()
    assert all(torch.equal(a, b) for a, b in zip(held, eager["second"]))
    assert not torch.equal(eager["first"][2], eager["second"][2])     # the two maps are different problems
    none = _post("none").decode_device(second, *tg)
    torch.cuda.synchronize()
    assert int(none[2].sum()) > int(held[2].sum())                   # and the suppression acted in the replay
