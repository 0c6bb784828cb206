"""Recorder of tests/golden/head_sets.npz: the reference's own Loss_Computation and PostProcessor under its REDUCED head sets.

Sibling of tools/gen_right_view_golden.py.  The reference accepts a family of MODEL.HEAD.REGRESSION_HEADS (its ablation ladder:
depth_uncertainty, corner_offset and corner_uncertainty are optional); tests/head_sets_ref.py names the six sets, four of them in
a channel order that differs from runs/monoflex.yaml.  For each of the five new sets this script runs, on the CPU and through
oracle/gen_golden.py's stubs,

  loss    model/head/detector_loss.py Loss_Computation, forward and backward, under every CORNER_LOSS_DEPTH the set can serve, on
          input `kd_interior` of tests/test_object_loss_configs_cpu.py (case b3 of oracle/gen_golden.py loss_case_inputs with truncated
          objects, invalid keypoint-depth groups and keypoint depths inside DEPTH_RANGE), its 50 canonical channels sliced and
          permuted into the set's layout (tests/head_sets_ref.py `take`); s010 also with MODIFY_INVALID_KEYPOINT_DEPTH False and
          every set once with a reduced LOSS_NAMES list.  Stored: the names and values of the loss dict and of the log dict, and
          the gradient of the summed loss at the valid objects' centre pixels.  The inputs are seeded: the test regenerates them.
  decode  model/head/detector_infer.py PostProcessor.forward under every OUTPUT_DEPTH the set can serve x UNCERTAINTY_AS_CONFIDENCE,
          on image 1 of tests/decode_cases.py's structured maps with isolated peaks (as oracle/gen_golden.py run_decode_structured).
          Stored per set: columns 0-8 of the result rows (the same under every mode), and per mode, in the order of
          tests/head_sets_ref.py output_depths, columns 9-13 with the confidence scaling on, the score column with it off,
          estimated_depth_error and uncertainty_conf (NaN where the reference reports None), and whether it reported None.
          The set with corner_uncertainty (s011) also under 'oracle', with the ground-truth boxes / classes / depths it read beside
          the rows (as tests/golden/decode_only.npz has them for the full set).
  raises  one combination of each kind the reference cannot run, stored as the name of the exception it raised.

Data only.  Needs the reference checkout that oracle/gen_golden.py names; run from the repository root:
    python tools/gen_head_sets_golden.py
"""
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

import numpy as np
import torch

from monoflex_amd import synthetic as S
from oracle import gen_golden as G
from tests import decode_cases as C
from tests import head_sets_ref as HS

DECODE = dict(map_seed=31, list_seed=32, K=50, images=(1,), score_ranges=[(0.05, 0.23)])
LOSS_INPUT = "kd_interior"
# LOSS_NAMES subsets recorded once per set (under CORNER_LOSS_DEPTH direct): what the reference's dicts then hold
NAME_SUBSETS = {"s000": ('corner_loss', 'trunc_offset_loss'), "s100": ('trunc_offset_loss',), "s010": ('keypoint_depth_loss',),
                "s110": ('corner_loss', 'keypoint_depth_loss'), "s011": ('weighted_avg_depth_loss',)}
HEAD = "MODEL.HEAD."
# (kind, set, overrides) the reference must raise on
REFUSED = (
    ("loss", "corner_keypoint_mean_without_kp", "s000", [HEAD + "CORNER_LOSS_DEPTH", "keypoint_mean"]),
    ("loss", "corner_soft_without_du", "s011", [HEAD + "CORNER_LOSS_DEPTH", "soft_combine"]),
    ("loss", "corner_hard_without_cu", "s110", [HEAD + "CORNER_LOSS_DEPTH", "hard_combine"]),
    ("loss", "keypoint_depth_loss_without_kp", "s100", "+keypoint_depth_loss"),
    ("loss", "weighted_avg_depth_loss_without_cu", "s010", "+weighted_avg_depth_loss"),
    ("loss", "kp_without_keypoint_loss", "s110", "-keypoint_loss"),
    ("decode", "output_keypoints_without_kp", "s100", [HEAD + "OUTPUT_DEPTH", "keypoints_avg"]),
    ("decode", "output_soft_without_cu", "s110", [HEAD + "OUTPUT_DEPTH", "soft"]),
    ("decode", "output_hard_without_kp", "s000", [HEAD + "OUTPUT_DEPTH", "hard"]),
)


def set_cfg(base, name, extra=(), names=None):
    c = base.clone()
    nm, w = HS.loss_names(name) if names is None else names
    c.merge_from_list([HEAD + "REGRESSION_HEADS", HS.SETS[name], HEAD + "REGRESSION_CHANNELS", HS.channels(name),
                       HEAD + "LOSS_NAMES", list(nm), HEAD + "INIT_LOSS_WEIGHT", list(w), HEAD + "CORNER_LOSS_DEPTH", "direct"] + list(extra))
    return c


def loss_inputs(name):
    import test_object_loss_configs_cpu as T
    tg, reg, cls, plan = T.make_input(LOSS_INPUT)
    return tg, cls, HS.take(reg, name, 1), plan


def run_loss(dl, cfg, name, out, tag):
    tg, cls, reg, plan = loss_inputs(name)
    ev = dl.Loss_Computation(cfg)
    cls, reg = cls.clone().requires_grad_(), reg.clone().requires_grad_()
    loss_dict, log_dict = ev({"cls": cls, "reg": reg}, [G.reference_train_target(t) for t in tg])
    sum(loss_dict.values()).backward()
    out[tag + "/loss_keys"], out[tag + "/log_keys"] = np.array(list(loss_dict)), np.array(list(log_dict))      # the dicts' names, in their order ...
    out[tag + "/loss_values"] = np.array([v.item() for v in loss_dict.values()], dtype=np.float64)                # ... and their values
    out[tag + "/log_values"] = np.array([float(v) for v in log_dict.values()], dtype=np.float64)
    b, s = (np.array(x) for x in zip(*plan["objects"]))
    cen = np.stack([np.asarray(tg[i]["target_centers"])[j] for i, j in plan["objects"]])
    gr = reg.grad.permute(0, 2, 3, 1)
    out[tag + "/grad_reg_at_objects"] = gr[torch.as_tensor(b), torch.as_tensor(cen[:, 1]), torch.as_tensor(cen[:, 0])].numpy()   # (8, R)
    out[tag + "/grad_reg_abssum"] = np.float64(reg.grad.abs().double().sum())
    print("loss", tag, {k: round(v.item(), 4) for k, v in loss_dict.items()})


def decode_inputs():
    maps = C.structured_maps(DECODE["map_seed"], DECODE["images"])
    scores, index = C.peak_lists(DECODE["list_seed"], len(DECODE["images"]), DECODE["K"], DECODE["score_ranges"])
    return maps, scores, index


def run_decode(make_post, cfg, name, out):
    maps, scores, index = decode_inputs()
    base = S.synthetic_target(C.W, C.H)
    reg_set = HS.take(maps["hmap"][..., maps["reg_off"]:maps["reg_off"] + 50], name, 3)
    for b, i in enumerate(DECODE["images"]):
        tgt = dict(base, P=C.image_P(i), size=tuple(C.IMAGES[i]["size"]), pad_size=torch.tensor(C.IMAGES[i]["pad"], dtype=torch.int64))
        cls = torch.from_numpy(C.peak_heat(scores, index, b))[None]
        reg = torch.from_numpy(reg_set[b]).permute(2, 0, 1)[None].contiguous()
        first, modes = None, HS.output_depths(name)
        cols, raw_score, err, none = [], [], [], np.zeros((2, len(modes)), dtype=np.int8)
        for uac in (1, 0):
            for m, mode in enumerate(modes):
                c = cfg.clone()
                c.merge_from_list([HEAD + "OUTPUT_DEPTH", mode, "TEST.UNCERTAINTY_AS_CONFIDENCE", bool(uac)])
                post = make_post(c)
                r, ev, _ = post({"cls": cls.clone(), "reg": reg.clone()}, [G.reference_target(tgt)], test=True)
                r = r.numpy()
                if first is None:
                    first = r[:, :9]
                assert np.array_equal(r[:, :9], first)                         # the depth enters a row through columns 9-13 only
                none[uac, m] = ev['estimated_depth_error'] is None
                assert bool(none[uac, m]) == (ev['uncertainty_conf'] is None) and (uac or none[uac, m])
                if uac:
                    cols.append(r[:, 9:])
                    err.append(np.full((r.shape[0], 2), np.nan, dtype=np.float32) if none[uac, m] else
                               np.stack((ev['estimated_depth_error'].numpy(), ev['uncertainty_conf'].numpy()), axis=1))
                else:
                    assert np.array_equal(r[:, 9:13], cols[m][:, :4])          # without the scaling only the score column changes
                    raw_score.append(r[:, 13])
        tag = "%s/decode" % name
        out[tag + "/cols0_9"], out[tag + "/cols9_14"], out[tag + "/raw_score"] = first, np.stack(cols), np.stack(raw_score)
        out[tag + "/error"], out[tag + "/error_is_none"], out[tag + "/modes"] = np.stack(err), none, np.array(list(modes))
        print("decode", name, "image", i, "rows", first.shape[0], "modes", modes, "None:", none[1].tolist())
        if 'mean' not in modes:
            continue
        # 'oracle' (get_oracle_depths, detector_infer.py:238-277) reads ground truth, as oracle/gen_golden.py run_decode_cases builds it: every
        # third 'mean' detection becomes an object whose box is the detection's shifted by (0.5, -0.25) px at 0.93 x its mean depth, plus two
        # objects no detection meets.  Without depth_uncertainty the choice is among the THREE keypoint depths.
        mean_rows = torch.from_numpy(np.concatenate((first, cols[modes.index('mean')]), axis=1))[::3]
        gt_boxes = torch.cat((mean_rows[:, 2:6] + torch.tensor([0.5, -0.25, 0.5, -0.25]), torch.tensor([[2., 2., 9., 12.], [120., 60., 140., 80.]])))
        gt_cls = torch.cat((mean_rows[:, 0], torch.tensor([0., 1.]))).long()
        gt_depth = torch.cat((mean_rows[:, 11] * 0.93, torch.tensor([20., 35.])))
        n_gt = gt_boxes.shape[0]
        pad_rows = lambda t: torch.cat((t, t.new_zeros((3,) + tuple(t.shape[1:]))))
        t_o = G.reference_target(tgt)
        reg_mask = torch.zeros(n_gt + 3, dtype=torch.uint8)
        reg_mask[:n_gt] = 1
        t_o.add_field("reg_mask", reg_mask)
        t_o.add_field("cls_ids", pad_rows(gt_cls))
        t_o.add_field("gt_bboxes", pad_rows(gt_boxes))
        t_o.add_field("locations", pad_rows(torch.stack((torch.zeros(n_gt), torch.zeros(n_gt), gt_depth), dim=1)))
        for uac in (1, 0):
            c = cfg.clone()
            c.merge_from_list([HEAD + "OUTPUT_DEPTH", "oracle", "TEST.UNCERTAINTY_AS_CONFIDENCE", bool(uac)])
            r, ev, _ = make_post(c)({"cls": cls.clone(), "reg": reg.clone()}, [t_o], test=True)
            r = r.numpy()
            assert np.array_equal(r[:, :9], first) and (ev['estimated_depth_error'] is None) == (not uac)
            out[tag + "/oracle/uac%d_cols9_14" % uac] = r[:, 9:]
            if uac:
                out[tag + "/oracle/error"] = np.stack((ev['estimated_depth_error'].numpy(), ev['uncertainty_conf'].numpy()), axis=1)
        out[tag + "/oracle/gt_boxes"], out[tag + "/oracle/gt_cls"], out[tag + "/oracle/gt_depth"] = gt_boxes.numpy(), gt_cls.numpy(), gt_depth.numpy()
        z = out[tag + "/oracle/uac1_cols9_14"][:, 2]
        single = [cols[modes.index(m)][:, 2] for m in ('keypoints_center', 'keypoints_02', 'keypoints_13')]
        took = [int((z == col).sum()) for col in single]
        left = float((z != cols[modes.index('mean')][:, 2]).mean())
        print("decode", name, "oracle: rows that left the mean %.2f, rows equal to centre / 02 / 13: %s" % (left, took))
        assert 0.1 < left < 0.9 and sum(t > 0 for t in took) >= 2


def names_with(name, spec):
    nm, w = HS.loss_names(name)
    if spec[0] == "+":
        return nm + [spec[1:]], w + [HS.LOSS_WEIGHTS[spec[1:]]]
    i = nm.index(spec[1:])
    return nm[:i] + nm[i + 1:], w[:i] + w[i + 1:]


def main():
    G.install_stubs()
    sys.path.insert(0, G.REF)
    os.chdir(G.REF)
    from config import cfg
    cfg.merge_from_file(os.path.join(G.REF, "runs", "monoflex.yaml"))
    cfg.MODEL.DEVICE = "cpu"
    cfg.INPUT.WIDTH_TRAIN, cfg.INPUT.HEIGHT_TRAIN = C.W * 4, C.H * 4
    import model.head.detector_loss as dl
    import model.head.detector_infer as di
    for m in (dl, di):
        assert os.path.abspath(m.__file__).startswith(G.REF + os.sep), m.__file__
    dl.get_iou_3d = lambda a, b: a.new_zeros(a.shape[0])            # shapely is absent; log-only (detector_loss.py:333)
    out = {}
    for name in HS.NEW_SETS:
        for mode in HS.corner_depths(name):
            run_loss(dl, set_cfg(cfg, name, [HEAD + "CORNER_LOSS_DEPTH", mode]), name, out, "%s/%s" % (name, mode))
        drop = NAME_SUBSETS[name]
        run_loss(dl, set_cfg(cfg, name, names=HS.loss_names(name, drop)), name, out, "%s/names" % name)
        out[name + "/names/dropped"] = np.array(list(drop))
        run_decode(di.make_post_processor, set_cfg(cfg, name), name, out)
    run_loss(dl, set_cfg(cfg, "s010", [HEAD + "MODIFY_INVALID_KEYPOINT_DEPTH", False]), "s010", out, "s010/direct_no_modify")
    raised = []
    for kind, label, name, spec in REFUSED:
        c = set_cfg(cfg, name, names=names_with(name, spec)) if isinstance(spec, str) else set_cfg(cfg, name, spec)
        try:
            if kind == "loss":
                tg, cls, reg, _ = loss_inputs(name)
                dl.Loss_Computation(c)({"cls": cls, "reg": reg}, [G.reference_train_target(t) for t in tg])
            else:
                maps, scores, index = decode_inputs()
                i0 = DECODE["images"][0]
                tgt = dict(S.synthetic_target(C.W, C.H), P=C.image_P(i0), size=tuple(C.IMAGES[i0]["size"]),
                           pad_size=torch.tensor(C.IMAGES[i0]["pad"], dtype=torch.int64))
                reg = torch.from_numpy(HS.take(maps["hmap"][0, :, :, 8:58], name, 2)).permute(2, 0, 1)[None].contiguous()
                di.make_post_processor(c)({"cls": torch.from_numpy(C.peak_heat(scores, index, 0))[None], "reg": reg}, [G.reference_target(tgt)], test=True)
            what = "ran"
        except Exception as e:                                          # the reference itself fails on this combination
            what = type(e).__name__
        out["raises/%s/%s" % (kind, label)] = np.array(what)
        raised.append((label, what))
    out["raises/labels"] = np.array(["%s/%s" % (k, l) for k, l, _, _ in REFUSED])
    for k, v in DECODE.items():
        out["decode_inputs/" + k] = np.array(v)
    out["meta"] = np.array("reference Loss_Computation (forward + backward of the summed loss) and PostProcessor.forward under the head sets of "
                           "tests/head_sets_ref.py SETS; loss input %r of tests/test_object_loss_configs_cpu.py make_input, decode inputs "
                           "tests/decode_cases.py structured_maps / peak_lists; get_iou_3d -> zeros (shapely absent); torch %s"
                           % (LOSS_INPUT, torch.__version__))
    np.savez_compressed(os.path.join(G.GOLD, "head_sets.npz"), **out)
    print("refused by the reference:", raised)
    assert all(w != "ran" for _, w in raised), raised


if __name__ == "__main__":
    main()
