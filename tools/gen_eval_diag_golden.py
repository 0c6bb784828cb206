"""Recorder of tests/golden/eval_diag.npz: the reference's own validation diagnostics, PostProcessor.forward(..., test=False) under
TEST.EVAL_DEPTH / TEST.EVAL_DIS_IOUS (model/head/detector_infer.py:86-89,280-452).

Sibling of tools/gen_decode_cfg_golden.py (same stubs, same structured head maps, one image at a time as the reference evaluates), on the
inputs of tests/eval_diag_cases.py `golden_inputs()`: six images (four cameras with their own pad / calibration), 120 object slots each with holes, one image without
objects, the targets of each image built around another depth estimate.  Stored per image b:
  depth_<mode>_img<b>_<key>   the 13 vectors of evaluate_3D_depths under OUTPUT_DEPTH soft and direct (one value per reg_mask object, slot order)
  boxes_img<b>                (n, 6, 7): the six boxes evaluate_3D_detection builds under OUTPUT_DEPTH direct -- predicted, target, offset, depth,
                              dims, orien -- as the arguments of its five get_iou3d calls
An image without objects stores nothing.  The IoU itself has NO runnable reference: get_iou3d raises NameError (`get_corners` is never imported,
detector_infer.py:477), and under any OUTPUT_DEPTH but 'direct' evaluate_3D_detection raises before it gets there.  The tool therefore replaces
detector_infer.get_iou3d by a recorder that stores its two arguments and returns zeros; the project's IoU is pinned to float64 elsewhere
(tests/test_box3d_iou_cpu.py).  Only data is stored.

Needs the reference checkout that oracle/gen_golden.py names; run from the repository root:
    python tools/gen_eval_diag_golden.py
"""
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import numpy as np
import torch

from monoflex_amd import synthetic as S
from oracle import gen_golden as G
from tests import decode_cases as C
from tests import eval_diag_cases as E
from tests import eval_diag_ref as R

DEPTH_MODES = ("soft", "direct")


def main():
    G.install_stubs()
    sys.path.insert(0, G.REF)
    os.chdir(G.REF)
    from config import cfg
    cfg.merge_from_file(os.path.join(G.REF, "runs", "monoflex.yaml"))
    cfg.MODEL.DEVICE = "cpu"
    cfg.INPUT.WIDTH_TRAIN, cfg.INPUT.HEIGHT_TRAIN = C.W * 4, C.H * 4
    from model.head.detector_infer import make_post_processor
    import model.head.detector_infer as ref_infer
    assert os.path.abspath(ref_infer.__file__).startswith(G.REF + os.sep), ref_infer.__file__
    calls = []

    def recorder(pred_bboxes, target_bboxes):
        calls.append((pred_bboxes.detach().clone().numpy(), target_bboxes.detach().clone().numpy()))
        return pred_bboxes.new_zeros(pred_bboxes.shape[0])
    ref_infer.get_iou3d = recorder

    d = E.golden_inputs()
    gt = d["gt_rows"]
    base = S.synthetic_target(C.W, C.H)
    out = {k: np.array(v) for k, v in E.GOLDEN.items()}
    out["depth_modes"], out["depth_keys"], out["box_names"] = np.array(DEPTH_MODES), np.array(R.DEPTH_KEYS), np.array(R.BOX_NAMES)
    counts = []

    def run(post, b):
        i = d["images"][b]
        tgt = dict(base, P=C.image_P(i), size=tuple(C.IMAGES[i]["size"]), pad_size=torch.tensor(C.IMAGES[i]["pad"], dtype=torch.int64))
        t = G.reference_target(tgt)
        g = torch.from_numpy(gt[b])
        t.add_field("reg_mask", g[:, R.G_MASK].to(torch.uint8))
        t.add_field("cls_ids", g[:, R.G_CLS].long())
        # (an empty slot of the cases holds noise, which mfx_eval_diagnostics must not read; the reference gathers every slot before it
        # masks, so its empty slots get the centre (0, 0) a label encoder leaves there)
        t.add_field("target_centers", (g[:, R.G_CX:R.G_CY + 1] * g[:, R.G_MASK:R.G_MASK + 1]).long())
        t.add_field("offset_3D", g[:, R.G_OFFX:R.G_OFFY + 1].clone())
        t.add_field("locations", g[:, R.G_X:R.G_Z + 1].clone())
        t.add_field("dimensions", g[:, R.G_L:R.G_W + 1].clone())
        t.add_field("rotys", g[:, R.G_RY].clone())
        cls = torch.full((1, 3, C.H, C.W), 1e-4)                        # no peak: the decode half of forward returns at once
        reg = torch.from_numpy(d["hmap"][b, :, :, d["reg_off"]:d["reg_off"] + 50]).permute(2, 0, 1)[None].contiguous()
        _, utils, _ = post({"cls": cls, "reg": reg}, [t], test=False)
        return utils

    for mode in DEPTH_MODES:
        cfg.MODEL.HEAD.OUTPUT_DEPTH = mode
        cfg.TEST.EVAL_DEPTH, cfg.TEST.EVAL_DIS_IOUS = True, False
        post = make_post_processor(cfg)
        assert post.eval_depth and not post.eval_dis_iou and post.output_depth == mode
        for b in range(gt.shape[0]):
            n = int((gt[b, :, R.G_MASK] != 0).sum())
            if n == 0:
                continue
            errs = run(post, b)["depth_errors"]
            assert tuple(errs.keys()) == R.DEPTH_KEYS, tuple(errs.keys())
            for k, v in errs.items():
                assert v.shape == (n,), (k, v.shape, n)
                out["depth_%s_img%d_%s" % (mode, b, k)] = v.numpy()
    cfg.MODEL.HEAD.OUTPUT_DEPTH = "direct"
    cfg.TEST.EVAL_DEPTH, cfg.TEST.EVAL_DIS_IOUS = False, True
    post = make_post_processor(cfg)
    for b in range(gt.shape[0]):
        n = int((gt[b, :, R.G_MASK] != 0).sum())
        counts.append(n)
        if n == 0:
            continue
        del calls[:]
        ious = run(post, b)["dis_ious"]
        assert tuple(ious.keys()) == R.IOU_KEYS and len(calls) == 5
        assert all(np.array_equal(c[1], calls[0][1]) for c in calls)    # the five calls share the target box
        boxes = np.stack([calls[0][0], calls[0][1]] + [c[0] for c in calls[1:]], axis=1)
        assert boxes.shape == (n, 6, 7)
        out["boxes_img%d" % b] = boxes
    print("eval_diag: objects per image", counts)
    out["meta"] = np.array(repr(dict(
        case="eval_diag", torch=torch.__version__, inputs="tests/eval_diag_cases.py golden_inputs()",
        iou="no runnable reference: detector_infer.get_iou3d raises NameError (get_corners is not imported, :477) and evaluate_3D_detection "
            "raises under every OUTPUT_DEPTH but 'direct'; get_iou3d was replaced by a recorder of its arguments that returns zeros, and the "
            "six boxes it received are stored instead")))
    np.savez_compressed(os.path.join(G.GOLD, "eval_diag.npz"), **out)
    print("eval_diag.npz: %d bytes" % os.path.getsize(os.path.join(G.GOLD, "eval_diag.npz")))


if __name__ == "__main__":
    main()
