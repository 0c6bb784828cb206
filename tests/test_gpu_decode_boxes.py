"""Device tests of the box decode (decode.hip `decode_boxes_kernel` through ops.decode_boxes) against its float64 restatement
(tests/decode_ref.py) on the structured inputs of tests/decode_cases.py: head maps whose rows reach every branch of the decode (the CPU
census of tests/test_decode_ref_cpu.py asserts the shares), three images with their own pad, size and calibration, score lists with ties
across classes, shared pixels and scores at the threshold.

Compared: all K rows of every image (valid or not), all 14 columns, error = |got - want| / max(1, |want|) per column.  `topk` and `valid`
must be EQUAL to the restatement.  Rows whose float64 margin on an arg-max is below 1e-5 (relative) are not compared in alpha / ry (bin
arg-max) or in the depth and what it enters (`hard` arg-max); alpha / ry within 1e-5 of +-pi before the wrap are compared modulo 2 pi; such
rows are capped at 2 % of a case (asserted on the CPU; the committed seeds have none).

Bound: 4x the per-column error of the float32 reference arithmetic (the reference's PostProcessor rows and oracle.decode_image against the
same restatement, decode_ref.YARDSTICK, measured by tests/test_decode_ref_cpu.py).  The kernel does the same float32 arithmetic with the
device's expf / atan2f and its own summation grouping.

column   float32 reference   bound (4x)   kernel, worst of all 38 cases of this module (first MI355X run)
cls      0                   0            0
alpha    4.45e-07            1.78e-06     4.45e-07
x1       9.54e-07            3.82e-06     9.54e-07
y1       4.77e-07            1.91e-06     4.77e-07
x2       9.54e-07            3.82e-06     9.54e-07
y2       4.77e-07            1.91e-06     4.77e-07
h        1.26e-07            5.04e-07     1.15e-07
w        1.49e-07            5.96e-07     1.47e-07
l        1.22e-07            4.88e-07     1.12e-07
X        2.91e-06            1.16e-05     1.86e-06
Y        1.26e-06            5.04e-06     8.26e-07
Z        2.97e-07            1.19e-06     2.58e-07
ry       6.90e-07            2.76e-06     6.53e-07
score    1.40e-07            5.60e-07     1.26e-07
The kernel stays within 1x the float32 reference's own error in every column.  (With the yardstick taken from the anchor maps alone, x1 had
a bound of 7.04e-07 and case k100 missed it with 9.54e-07 = 2^-20: the rounding of (px - e) * 4 - pad itself, which the float32 reference
shows on the same map -- see tests/test_decode_ref_cpu.py.)
"""
import functools
import os

import numpy as np
import pytest
import torch

from tests import decode_cases as C
from tests import decode_ref as D

pytestmark = pytest.mark.gpu
DEV = "cuda"


@functools.lru_cache(maxsize=None)
def _case(name, kind):
    d = C.case_inputs(name, kind)
    for a in d.values():
        if isinstance(a, np.ndarray):
            a.setflags(write=False)
    return d


@functools.lru_cache(maxsize=None)
def _ref(name, kind, mode):
    return C.run_ref(_case(name, kind), mode)


def _device_inputs(d):
    t = lambda a, dt: torch.from_numpy(np.array(a)).to(DEV, dt)
    return (t(d["hmap"], torch.float32), d["reg_off"], t(d["scores"], torch.float32), t(d["index"], torch.int32), t(d["calib"], torch.float32),
            t(d["pad"], torch.int32), t(d["img_size"], torch.int32), float(d["threshold"]))


def _run(d, mode):
    from monoflex_amd import ops
    det, topk, valid = ops.decode_boxes(*_device_inputs(d), depth_mode=mode)
    torch.cuda.synchronize()
    return det.cpu().numpy(), topk.cpu().numpy(), valid.cpu().numpy()


def _compare(what, got, ref, mode):
    det, topk, valid = got
    assert np.isfinite(det).all(), what
    assert np.array_equal(topk.astype(np.float64), ref["topk"]), what + ": topk differs from the restatement"
    assert np.array_equal(valid, ref["valid"]), what + ": valid differs from the restatement"
    assert float(D.near_rows(ref, mode).mean()) <= D.NEAR_CAP, what
    err = D.column_errors(det, ref, mode)
    print("%-40s %s" % (what, D.format_errors(err)))
    bound = D.bounds()
    assert (err <= bound).all(), "%s: column(s) %s past 4x the float32 reference's error: %s" % (
        what, [D.COLUMNS[i] for i in np.nonzero(err > bound)[0]], D.format_errors(err))


def _check_case(name, kind, mode):
    _compare("%s %s %s" % (name, kind, mode), _run(_case(name, kind), mode), _ref(name, kind, mode), mode)


@pytest.mark.parametrize("mode", D.MODES)
def test_every_depth_mode(mode):
    """B = 3, K = 50, ld 64, reg_off 8: three images with their own pad, size and calibration."""
    _check_case("b3_k50", "distinct", mode)


@pytest.mark.parametrize("mode", ["soft", "hard"])
@pytest.mark.parametrize("name", ["k1", "k7", "k100", "k256"])
def test_k_from_1_to_256(name, mode):
    _check_case(name, "distinct", mode)


@pytest.mark.parametrize("mode", ["soft", "hard"])
@pytest.mark.parametrize("name", ["ld50", "b3_k50", "ld72"])
def test_row_layouts(name, mode):
    """(ld, reg_off) = (50, 0), (64, 8), (72, 13); the channels outside the 50 regression values hold noise."""
    c = C.CASES[name]
    assert (c["ld"], c["reg_off"]) == {"ld50": (50, 0), "b3_k50": (64, 8), "ld72": (72, 13)}[name]
    _check_case(name, "distinct", mode)


@pytest.mark.parametrize("mode", ["soft", "hard"])
@pytest.mark.parametrize("name", ["b1_k100", "b3_permuted"])
def test_batch_1_and_permuted_images(name, mode):
    """B = 1; and B = 3 in the order (2, 0, 1): image 0 is then the smallest frame, and ITS size clamps the boxes of all three images."""
    d = _case(name, "distinct")
    if name == "b3_permuted":
        assert tuple(d["img_size"]) == tuple(d["sizes"][0]) and (d["sizes"][0] < d["sizes"][1:]).all()
        own = C.run_ref(d, mode, wrong="clamp_per_image")["det"]
        assert np.abs(own[..., 2:6] - _ref(name, "distinct", mode)["det"][..., 2:6]).max() > 1       # (the inputs can tell the two rules apart)
    _check_case(name, "distinct", mode)


@pytest.mark.parametrize("kind", ["ties", "shared_pixel", "threshold"])
@pytest.mark.parametrize("name", ["k7", "b3_k50", "k256"])
def test_tie_rule_shared_pixels_and_threshold(name, kind):
    """Equal scores across the three classes (many at the heat map's clamp 0.9999) leave stage 2 in position order; one pixel in two classes
    gives two rows; scores at, one ulp below and one ulp above the threshold set `valid`.  topk and valid EQUAL the restatement."""
    d, ref = _case(name, kind), _ref(name, kind, "soft")
    if kind == "ties":
        flat = d["scores"].reshape(d["scores"].shape[0], -1)
        assert all(np.unique(flat[b][D.stage2_merge(d["scores"][b])]).size < d["scores"].shape[2] for b in range(flat.shape[0]))
        assert (ref["topk"][..., 0] == float(C.SCORE_CLAMP)).any() and len(set(ref["topk"][0, ref["topk"][0, :, 0] == float(C.SCORE_CLAMP), 2])) > 1
    _check_case(name, kind, "soft")


def test_graph_replay_is_bitwise_the_eager_call():
    from monoflex_amd import ops
    d = _case("b3_k50", "ties")
    args = _device_inputs(d)
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        eager = [t.clone() for t in ops.decode_boxes(*args, depth_mode="hard")]
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        held = ops.decode_boxes(*args, depth_mode="hard")
    for t in held:
        t.zero_()
    graph.replay()
    torch.cuda.synchronize()
    assert all(torch.equal(a, b) for a, b in zip(held, eager))
    _compare("graph replay b3_k50 ties hard", [t.cpu().numpy() for t in held], _ref("b3_k50", "ties", "hard"), "hard")


def _peak_map():
    """A structured map (B = 3, ld 64, reg_off 8) whose class logits carry isolated peaks: 50 per class, all scores of an image distinct,
    a quarter of each image's best 50 below the threshold."""
    m = C.structured_maps(41, (1, 2, 0))
    scores, index = C.peak_lists(42, 3, 50, [(0.02, 0.26)] * 3)
    hmap = m["hmap"].copy()
    hmap[..., :3] = C.peak_logits(scores, index)
    return dict(m, hmap=hmap, threshold=C.THRESHOLD), scores, index


def _topk_on_device(hm):
    from monoflex_amd import ops
    s, i = ops.decode_topk(hm, 0, 3, 50)
    torch.cuda.synchronize()
    return s, i


def test_topk_then_boxes_on_a_structured_map():
    """ops.decode_topk then ops.decode_boxes: stage 1 must find exactly the planted peaks, and the rows are the restatement's on the scores
    stage 1 produced."""
    from monoflex_amd import ops
    m, scores, index = _peak_map()
    hm = torch.from_numpy(m["hmap"]).to(DEV)
    s, i = _topk_on_device(hm)
    assert np.array_equal(i.cpu().numpy(), np.take_along_axis(index, np.argsort(-scores, axis=2, kind="stable"), axis=2))
    assert np.abs(s.cpu().numpy() - scores).max() <= 2e-7            # sigmoid(logit(s)) in float32: an ulp or two of s < 1
    d = dict(m, scores=s.cpu().numpy(), index=i.cpu().numpy())
    got = ops.decode_boxes(*_device_inputs(d)[:2], s, i, *_device_inputs(d)[4:], depth_mode="soft")
    torch.cuda.synchronize()
    ref = C.run_ref(d, "soft")
    assert 0 < ref["valid"].sum() < ref["valid"].size
    _compare("decode_topk + decode_boxes", [t.cpu().numpy() for t in got], ref, "soft")


def test_post_processor_on_a_structured_map():
    """The same map through make_post_processor(cfg) ('soft', the yaml's): per image the rows that pass the threshold, in order."""
    from monoflex_amd.config import get_cfg
    from monoflex_amd.model.head.detector_infer import make_post_processor
    from monoflex_amd.structures.params_3d import Calibration, ParamsList
    m, scores, index = _peak_map()
    cfg = get_cfg(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "runs", "monoflex.yaml"), [])
    post = make_post_processor(cfg)
    assert post.output_depth == "soft" and post.max_detection == 50 and float(post.det_threshold) == C.THRESHOLD
    targets = []
    for i in m["images"]:
        t = ParamsList(image_size=tuple(C.IMAGES[i]["size"]), is_train=False)
        t.add_field("pad_size", torch.tensor(C.IMAGES[i]["pad"]))
        t.add_field("calib", Calibration(C.image_P(i)))
        targets.append(t)
    hm = torch.from_numpy(m["hmap"]).to(DEV)
    results, utils, _ = post({"hm_nhwc": hm, "cls": None}, targets)
    s, i = _topk_on_device(hm)
    ref = C.run_ref(dict(m, scores=s.cpu().numpy(), index=i.cpu().numpy()), "soft")
    det = utils["det_all"].cpu().numpy()
    _compare("PostProcessor", (det, utils["topk"].cpu().numpy(), utils["valid"].cpu().numpy()), ref, "soft")
    for b in range(3):
        keep = ref["valid"][b].astype(bool)
        assert 0 < keep.sum() < 50 and np.array_equal(results[b].cpu().numpy(), det[b][keep])
