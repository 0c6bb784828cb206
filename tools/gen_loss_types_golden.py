"""Recorder of tests/golden/loss_types.npz: the reference's own Loss_Computation under its other MODEL.HEAD.LOSS_TYPE settings.

Sibling of tools/gen_head_sets_golden.py.  The reference reads LOSS_TYPE[1] as "L1, or else F.smooth_l1_loss" (the regular regression
loss: offset, dimensions, corners, keypoint depths, the combined depth) and LOSS_TYPE[3] as the direct-depth loss: L1, log, inv_sig
(model/head/detector_loss.py:45-53, model/head/depth_losses.py).  For each setting of tests/loss_types_cases.py GOLDEN -- on the
runs/monoflex.yaml base smooth_l1+L1, L1+log, smooth_l1+log, smooth_l1+inv_sig; smooth_l1+log with the `defaults` switches of
tests/test_object_loss_configs_cpu.py; L1+log on head set s000 (no depth uncertainty) -- this script runs, on the CPU and through
oracle/gen_golden.py's stubs, the reference's Loss_Computation forward and backward on the inputs GOLDEN_INPUTS (`kd_interior` and
`b3_mixed` of tests/test_object_loss_configs_cpu.py, and `branches`: kd_interior with the length / width channels scaled and three target
depths moved next to a predicted depth, tests/loss_types_cases.py make_branches).

Stored per (setting, input): the names and values of the loss dict and of the log dict, and the gradient of the summed loss at the valid
objects' centre pixels.  The inputs are seeded: the test regenerates them.

Asserted from the reference's own intermediates (prepare_predictions): every term that takes the regular regression loss sees both of
its branches, |d| < 1 and |d| > 1, in at least one recorded input of every smooth_l1 setting that has the term; the branch counts are
stored beside the values.

One stub beyond oracle/gen_golden.py's: Loss_Computation calls its depth loss as `self.depth_loss(pred, target, reduction='none')`
(detector_loss.py:299), and Log_L1_Loss.forward / Inverse_Sigmoid_Loss.forward take (prediction, target, weight=None) -- as written the call
raises TypeError.  Both classes compute the unreduced loss, which is what reduction='none' asks for, so the recorder lets their forward accept
that keyword (asserting its value) and changes nothing else: the recorded numbers are the classes' own arithmetic inside the reference's own
Loss_Computation.  (Berhu_Loss is not recorded: its forward opens a debugger.)

Data only.  Needs the reference checkout that oracle/gen_golden.py names; run from the repository root:
    python tools/gen_loss_types_golden.py
"""
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

import numpy as np
import torch

from oracle import gen_golden as G
from tests import decode_cases as C
from tests import loss_types_cases as LT

REG_TERMS = ("offset", "dims", "corners", "keypoint_depth_valid", "keypoint_depth_invalid", "weighted_avg_depth")


def regression_differences(ev, reg, targets):
    """The differences d = prediction - target that self.reg_loss_fnc sees in ev.__call__ (detector_loss.py:309, 330, 339, 356-360, 423), from
    the reference's own prepare_targets / prepare_predictions."""
    with torch.no_grad():
        _, tv = ev.prepare_targets(targets)
        T, P, _, _ = ev.prepare_predictions(tv, {"reg": reg})
        d = {"offset": P['offset_3D'] - T['offset_3D'], "dims": P['dims_3D'] - T['dims_3D'], "corners": P['corners_3D'] - T['corners_3D']}
        if ev.compute_keypoint_corner and ev.compute_keypoint_depth_loss:
            m = T['keypoints_depth_mask'].bool()
            kd = P['keypoints_depths'] - T['depth_3D'].unsqueeze(-1)
            d["keypoint_depth_valid"], d["keypoint_depth_invalid"] = kd[m], kd[~m]
        if ev.corner_with_uncertainty and ev.compute_weighted_depth_loss:
            unc = torch.cat((P['depth_uncertainty'].unsqueeze(1), P['corner_offset_uncertainty']), dim=1).exp()
            dep = torch.cat((P['depth_3D'].unsqueeze(1), P['keypoints_depths']), dim=1)
            w = 1 / unc
            d["weighted_avg_depth"] = torch.sum(dep * (w / w.sum(dim=1, keepdim=True)), dim=1) - T['depth_3D']
    return {k: v.reshape(-1).numpy() for k, v in d.items()}


def accept_reduction_none(klass):
    """Let klass.forward take the `reduction='none'` that Loss_Computation passes (module docstring); the arithmetic stays the class's own."""
    fwd = klass.forward

    def forward(self, prediction, target, weight=None, reduction='none'):
        assert reduction == 'none'
        return fwd(self, prediction, target, weight)
    klass.forward = forward


def run_loss(dl, cfg, name, iname, out):
    tg, cls, reg, plan = LT.golden_input(name, iname)
    ev = dl.Loss_Computation(cfg)
    targets = [G.reference_train_target(t) for t in tg]
    cover = LT.branch_coverage(regression_differences(ev, reg, targets))
    cls, reg = cls.clone().requires_grad_(), reg.clone().requires_grad_()
    loss_dict, log_dict = ev({"cls": cls, "reg": reg}, targets)
    sum(loss_dict.values()).backward()
    tag = "%s/%s" % (name, iname)
    out[tag + "/loss_keys"], out[tag + "/log_keys"] = np.array(list(loss_dict)), np.array(list(log_dict))
    out[tag + "/loss_values"] = np.array([v.item() for v in loss_dict.values()], dtype=np.float64)
    out[tag + "/log_values"] = np.array([float(v) for v in log_dict.values()], dtype=np.float64)
    b, s = (np.array(x) for x in zip(*plan["objects"]))
    cen = np.stack([np.asarray(tg[i]["target_centers"])[j] for i, j in plan["objects"]])
    gr = reg.grad.permute(0, 2, 3, 1)
    out[tag + "/grad_reg_at_objects"] = gr[torch.as_tensor(b), torch.as_tensor(cen[:, 1]), torch.as_tensor(cen[:, 0])].numpy()   # (8, R)
    out[tag + "/grad_reg_abssum"] = np.float64(reg.grad.abs().double().sum())
    out[tag + "/branches"] = np.array([cover.get(k, (False, False)) for k in REG_TERMS], dtype=np.int8)      # (6, 2): saw |d| < 1, saw |d| > 1
    print("loss", tag, {k: round(v.item(), 4) for k, v in loss_dict.items()})
    print("      branches (|d|<1, |d|>1):", {k: cover[k] for k in REG_TERMS if k in cover})
    return cover


def main():
    G.install_stubs()
    sys.path.insert(0, G.REF)
    os.chdir(G.REF)
    from config import cfg
    cfg.merge_from_file(os.path.join(G.REF, "runs", "monoflex.yaml"))
    cfg.MODEL.DEVICE = "cpu"
    cfg.INPUT.WIDTH_TRAIN, cfg.INPUT.HEIGHT_TRAIN = C.W * 4, C.H * 4
    import model.head.detector_loss as dl
    assert os.path.abspath(dl.__file__).startswith(G.REF + os.sep), dl.__file__
    dl.get_iou_3d = lambda a, b: a.new_zeros(a.shape[0])            # shapely is absent; log-only (detector_loss.py:333)
    for klass in (dl.Log_L1_Loss, dl.Inverse_Sigmoid_Loss):
        accept_reduction_none(klass)
    out = {}
    for name, (_, _, reg_kind, _) in LT.GOLDEN.items():
        c = cfg.clone()
        c.merge_from_list(LT.golden_overrides(name))
        seen = {}
        for iname in LT.GOLDEN_INPUTS:
            for k, (lo, hi) in run_loss(dl, c, name, iname, out).items():
                seen[k] = (seen.get(k, (False, False))[0] or lo, seen.get(k, (False, False))[1] or hi)
        if reg_kind != "L1":                                          # both branches of smooth L1, per term, somewhere in the recorded inputs
            assert seen and all(lo and hi for lo, hi in seen.values()), (name, seen)
    out["settings"], out["inputs"], out["reg_terms"] = np.array(list(LT.GOLDEN)), np.array(list(LT.GOLDEN_INPUTS)), np.array(list(REG_TERMS))
    out["meta"] = np.array("reference Loss_Computation (forward + backward of the summed loss) under the LOSS_TYPE settings of tests/loss_types_cases.py "
                           "GOLDEN on its GOLDEN_INPUTS (tests/test_object_loss_configs_cpu.py make_input); get_iou_3d -> zeros (shapely absent); torch %s"
                           % torch.__version__)
    np.savez_compressed(os.path.join(G.GOLD, "loss_types.npz"), **out)


if __name__ == "__main__":
    main()
