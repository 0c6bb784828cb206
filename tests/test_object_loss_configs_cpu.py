"""The per-object loss arithmetic (csrc/object_loss_math.h, host build tests/shim/object_loss_host.cpp) in EVERY configuration
that Loss_Computation.object_loss_cfg() hands to the kernel, and on the clamps / ties / guards of its inputs.

Reference: the tensor-op form of Loss_Computation (fused_object_loss = False) on the CPU with the regression map in float64 and
gradients from torch autograd -- the restatement of the reference project's detector_loss.py that tests/golden/loss.npz pins in
the runs/monoflex.yaml configuration.  Neither the shim nor the kernel is ever its own reference.  tests/test_gpu_object_loss_
configs.py imports the configuration set, the inputs and the reference from here and runs the device kernels against them.

Configurations (CONFIGS, 37): two baselines -- runs/monoflex.yaml as it is, and the config.py defaults of the switches (exp depth,
direct corner depth, linear dimensions, L1 truncation loss, no invalid-keypoint-depth term) -- every switch set to each of its
other values one at a time around both, the full depth_mode x corner_depth_mode grid, LOSS_NAMES without trunc_offset_loss under
both TRUNCATION_OFFSET_LOSS values, DIMENSION_REG in its four forms, UNCERTAINTY_RANGE [-1, 1], non-uniform weights.  Each
evaluator is built with get_cfg(runs/monoflex.yaml, [KEY, VALUE, ...]); test_configuration_set_is_the_documented_one asserts
the list, test_config_* assert that the setting reached the kernel configuration.

Inputs (INPUTS): `b3` is case b3_empty_middle_mixed_calib of tests/test_loss_golden.py (B=3, the middle image empty, three
calibrations; eight valid objects).  That case has no truncated object and no invalid keypoint-depth group, so `b3_mixed` is
the same case with two objects marked truncated and four objects with invalid groups (one with all three): without it
separate_trunc / trunc_log / modify_invalid would be compared on zeros.  With reg = randn*0.6 the keypoint height differences
are far below a pixel, so every keypoint depth fh / (relu(dh)*down_ratio + eps) of `b3` and `b3_mixed` sits on DEPTH_RANGE[1]
(a constant with zero gradient: keypoint_mean, soft_combine and hard_combine would mix three constants).  `kd_interior` is
`b3_mixed` with the keypoint y channels of six objects set so that the depth of every group lies strictly inside the range, for
exp and linear dimensions alike; check_input asserts that from the reference, and that keypoint_depth_loss and corner_loss
have a nonzero gradient through those channels.  Every configuration runs on all three.  The edge inputs (EDGES) overwrite
channels at object centres (or target fields) to sit ON an edge; every test asserts from the float64 reference's intermediates
that the edge is hit.

Bounds (from tests/test_loss_golden.py): terms 2e-5*max(1,|ref|), logged means 1e-4*max(1,|ref|), per-term gradient
1e-5*max(1,max|ref|) (2e-5 on the device).  No bound here is derived from the shim's or the kernel's output.

    Measured on the CPU against the float64 reference, worst over the 37 configurations x the three inputs and the 25 edge cases,
    in units of the bound.  The yardstick is the float32 tensor-op form (no code under test); it is computed and held under a
    quarter of each bound by test_float32_tensor_ops_stay_under_a_quarter_of_each_bound (every configuration on kd_interior, both
    baselines on every other input and edge), so four times its error fits the project's bounds and those are kept as they are:
      quantity          float32 tensor ops    4x that    host build of the kernel math    bound kept
      terms             0.007                 0.03       0.008                            2e-5*max(1,|ref|)
      logged means      0.002                 0.008      0.002                            1e-4*max(1,|ref|)
      gradients         0.018                 0.07       0.019                            1e-5*max(1,max|ref|)
    (exp depth near the top of its range, -log(iou) and the fh/eps branch included: none of them needs a wider bound.)

Rows a gradient comparison may leave out: only rows whose float64 margin at a selection (orientation arg-max, arg-min of the
four uncertainties, an untied min/max of the GIoU) is below 1e-5 relative; planted exact ties are compared.  The cap of 5% of
the valid rows is asserted; for the seeds used here no row is dropped in any configuration.

Which side was wrong: neither -- these tests found no divergence between object_loss_math.h and the tensor-op form.  One-line
mutations of object_loss_math.h tried on a scratch copy (tests/test_loss_golden.py still passing unless noted): keypoint_mean
and hard_combine swapped -> 17 tests here fail (test_config_kernel_math_vs_float64[*corner_depth_mode=keypoint_mean*|*hard_combine*]);
dim_use_std ignored -> the six [*dim_use_std=1*] cases; modify_invalid ignored -> every [defaults*-b3_mixed] case and
[defaults-counts_none]; l1 where trunc_log asks log(l1+1) -> [defaults-trunc_log=1-b3_mixed], [*-counts_all] (the yaml goldens
catch this one too); a clamp that blocks the gradient ON its bound -> the three [*unc_clamp] edge cases; kd[2] from one keypoint
pair instead of the mean of two -> all 37 [*-kd_interior] cases; a detached fh -> all 37 [*-kd_interior] cases and the linear-
dimension ones on b3; |dh| in place of relu(dh) -> both [*-keypoint_heights] edges and 49 configuration cases (the goldens of
b2 and b1_many catch that one too).
"""
import functools
import os
import sys

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

from test_loss_golden import LOG_NAMES, TERM_NAMES, case_inputs, object_loss_shim, run_object_shim  # noqa: E402,F401 (fixture)

YAML = os.path.join(ROOT, "runs", "monoflex.yaml")
HEAD = "MODEL.HEAD."
YAML_NAMES = ['hm_loss', 'bbox_loss', 'depth_loss', 'offset_loss', 'orien_loss', 'dims_loss', 'corner_loss', 'keypoint_loss',
              'keypoint_depth_loss', 'trunc_offset_loss', 'weighted_avg_depth_loss']
YAML_WEIGHTS = [1, 1, 1, 0.5, 1, 1, 0.2, 1.0, 0.2, 0.1, 0.2]
ODD_WEIGHTS = [1, 0.7, 1.3, 0.5, 0.9, 1.1, 0.2, 0.6, 0.25, 0.3, 0.4]
ODD_DIM_WEIGHT = [0.5, 1.0, 2.0]
SWITCHES = {"depth_mode": ('exp', 'linear', 'inv_sigmoid'), "iou_type": ('giou', 'iou', 'linear_iou'),
            "corner_depth_mode": ('direct', 'keypoint_mean', 'soft_combine', 'hard_combine'), "dim_exp": (0, 1), "dim_use_std": (0, 1),
            "separate_trunc": (0, 1), "trunc_log": (0, 1), "modify_invalid": (0, 1)}
BASE_YAML = dict(depth_mode='inv_sigmoid', iou_type='giou', corner_depth_mode='soft_combine', dim_exp=1, dim_use_std=0, separate_trunc=1,
                 trunc_log=1, modify_invalid=1, unc_range=(-10, 10), weights=None)
BASE_DEFAULTS = dict(BASE_YAML, depth_mode='exp', corner_depth_mode='direct', dim_exp=0, trunc_log=0, modify_invalid=0)   # monoflex_amd/config.py


def _config_set():
    out = {"yaml": BASE_YAML, "defaults": BASE_DEFAULTS}
    for bname, base in (("yaml", BASE_YAML), ("defaults", BASE_DEFAULTS)):
        for key, values in SWITCHES.items():
            for v in values:
                if v != base[key]:
                    out["%s-%s=%s" % (bname, key, v)] = dict(base, **{key: v})
    for d in SWITCHES["depth_mode"]:                                     # the corner depth is built from the decoded depths
        for cd in SWITCHES["corner_depth_mode"]:
            s = dict(BASE_YAML, depth_mode=d, corner_depth_mode=cd)
            if s not in out.values():
                out["grid-%s-%s" % (d, cd)] = s
    for extra in (dict(BASE_YAML, separate_trunc=0, trunc_log=0), dict(BASE_YAML, separate_trunc=0, trunc_log=1),
                  dict(BASE_YAML, dim_exp=0, dim_use_std=1)):
        if extra not in out.values():
            out["extra-" + "-".join("%s=%s" % (k, extra[k]) for k in ("separate_trunc", "trunc_log", "dim_exp", "dim_use_std"))] = extra
    out["unc_range_1"] = dict(BASE_YAML, unc_range=(-1, 1))
    out["weights"] = dict(BASE_YAML, weights=(ODD_WEIGHTS, ODD_DIM_WEIGHT))
    out["defaults-weights"] = dict(BASE_DEFAULTS, weights=(ODD_WEIGHTS, ODD_DIM_WEIGHT))
    return out


CONFIGS = _config_set()
EDGE_CONFIGS = ("yaml", "defaults")


def overrides(s):
    """The KEY VALUE list that turns runs/monoflex.yaml into switch set `s`; keys the yaml already sets that way are left to it."""
    o = []
    if s["depth_mode"] != BASE_YAML["depth_mode"]:
        o += [HEAD + "DEPTH_MODE", s["depth_mode"]]
    if s["iou_type"] != BASE_YAML["iou_type"]:
        o += [HEAD + "LOSS_TYPE", ["Penalty_Reduced_FocalLoss", "L1", s["iou_type"], "L1"]]
    if s["corner_depth_mode"] != BASE_YAML["corner_depth_mode"]:
        o += [HEAD + "CORNER_LOSS_DEPTH", s["corner_depth_mode"]]
    if (s["dim_exp"], s["dim_use_std"]) != (BASE_YAML["dim_exp"], BASE_YAML["dim_use_std"]):
        o += [HEAD + "DIMENSION_REG", ['exp' if s["dim_exp"] else 'linear', True, bool(s["dim_use_std"])]]
    if s["trunc_log"] != BASE_YAML["trunc_log"]:
        o += [HEAD + "TRUNCATION_OFFSET_LOSS", 'log' if s["trunc_log"] else 'L1']
    if s["modify_invalid"] != BASE_YAML["modify_invalid"]:
        o += [HEAD + "MODIFY_INVALID_KEYPOINT_DEPTH", bool(s["modify_invalid"])]
    if tuple(s["unc_range"]) != BASE_YAML["unc_range"]:
        o += [HEAD + "UNCERTAINTY_RANGE", list(s["unc_range"])]
    names, weights = list(YAML_NAMES), list(s["weights"][0] if s["weights"] else YAML_WEIGHTS)
    if not s["separate_trunc"]:
        i = names.index('trunc_offset_loss')
        del names[i], weights[i]
    if not s["separate_trunc"] or s["weights"]:
        o += [HEAD + "LOSS_NAMES", names, HEAD + "INIT_LOSS_WEIGHT", weights]
    if s["weights"]:
        o += [HEAD + "DIMENSION_WEIGHT", list(s["weights"][1])]
    return o


def make_evaluator(cname):
    from monoflex_amd.config import get_cfg
    from monoflex_amd.model.head.detector_loss import Loss_Computation
    return Loss_Computation(get_cfg(YAML, overrides(CONFIGS[cname])))


def check_kernel_cfg(cname, ev):
    """The setting must have reached the kernel configuration: the fused path is taken and carries the expected values."""
    s, c = CONFIGS[cname], ev.object_loss_cfg()
    assert c is not None, cname
    for key, values in SWITCHES.items():
        want = values.index(s[key]) if isinstance(values[0], str) else s[key]
        assert getattr(c, key) == want, (cname, key, getattr(c, key), want)
    assert (c.unc_lo, c.unc_hi) == (float(s["unc_range"][0]), float(s["unc_range"][1])) and c.has_depth_range == 1
    w = dict(zip(YAML_NAMES, s["weights"][0] if s["weights"] else YAML_WEIGHTS))
    if not s["separate_trunc"]:
        w['trunc_offset_loss'] = 0.0
    assert list(c.w) == [float(np.float32(w[k])) for k in TERM_NAMES], cname
    assert list(c.dim_weight) == [float(np.float32(x)) for x in (s["weights"][1] if s["weights"] else (1, 1, 1))], cname
    return c


# ---- inputs -----------------------------------------------------------------------------------------------------------------------
CH = {'2d_dim': 0, '3d_offset': 4, 'corner_offset': 6, 'corner_uncertainty': 26, '3d_dim': 29, 'ori_cls': 32, 'ori_offset': 40, 'depth': 48,
      'depth_uncertainty': 49}                                            # REGRESSION_HEADS / REGRESSION_CHANNELS of runs/monoflex.yaml
DEPTH_OFFSETS = {'exp': (-5.0, 6.0), 'linear': (-3.0, 6.0), 'inv_sigmoid': (5.0, -6.0)}       # decoded below 0.1 / above 100
INPUTS = ("b3", "b3_mixed", "kd_interior")
KD_PAIRS = {0: ((8, 9),), 1: ((0, 4), (2, 6)), 2: ((1, 5), (3, 7))}        # keypoint pairs whose height difference gives each group's depth
KD_DH = {0: (10.0,), 1: (9.0, 14.0), 2: (11.0, 8.0)}                       # fh / (4 dh) inside (0.1, 100) for every dimension decode
EDGES = ("depth_clamp", "unc_clamp", "box_edges", "keypoint_heights", "counts_none", "counts_all", "shared_centre")


def _objects(tg):
    return [(b, int(s)) for b, t in enumerate(tg) for s in np.nonzero(t["reg_mask"])[0]]


def _put(reg, tg, obj, ch, values):
    b, s = obj
    cx, cy = (int(x) for x in tg[b]["target_centers"][s])
    reg[b, ch:ch + len(values), cy, cx] = torch.tensor(values, dtype=torch.float32)


def make_input(name, depth_mode='inv_sigmoid'):
    """(target dicts, reg (3,50,96,320) float32, cls, plan): case b3 with the named edit; plan names the planted objects."""
    tg, cls, reg = case_inputs("b3_empty_middle_mixed_calib")
    tg = [{k: (v.copy() if isinstance(v, np.ndarray) else v) for k, v in t.items()} for t in tg]
    reg = reg.clone()
    o = _objects(tg)
    assert len(o) == 8 and [b for b, _ in o] == [0] * 4 + [2] * 4
    assert len({(b,) + tuple(tg[b]["target_centers"][s]) for b, s in o}) == 8          # the base case shares no centre pixel
    plan = {"objects": o}
    if name == "b3":
        pass
    elif name in ("b3_mixed", "kd_interior"):
        for b, s in (o[0], o[5]):
            tg[b]["trunc_mask"][s] = 1
        for (b, s), m in ((o[1], (0, 1, 1)), (o[2], (0, 0, 0)), (o[5], (1, 0, 1)), (o[6], (1, 1, 0))):
            tg[b]["keypoints_depth_mask"][s] = m
        if name == "kd_interior":
            # randn*0.6 keypoints give height differences well under a pixel: every keypoint depth sits on DEPTH_RANGE[1].  Here the
            # y channels of six objects are set so that each group's depth fh / (dh*down_ratio + eps) lies strictly inside the range
            # (3d_dim h channel 0.5: a positive height in all four DIMENSION_REG forms); objects 3 and 7 stay saturated.
            ky = lambda j: CH['corner_offset'] + 2 * j + 1
            kd = []
            for i, groups in ((0, (0, 1, 2)), (1, (0, 1, 2)), (4, (0, 1, 2)), (5, (0, 1, 2)), (2, (0, 1)), (6, (0, 1))):
                _put(reg, tg, o[i], CH['3d_dim'] + 1, [0.5])
                for g in groups:
                    for (a, c), dh in zip(KD_PAIRS[g], KD_DH[g]):
                        _put(reg, tg, o[i], ky(a), [0.25 + dh + 0.25 * i]); _put(reg, tg, o[i], ky(c), [0.25])
                    kd.append((o[i], g))
            for i in (0, 4):                                               # hard_combine must pick a keypoint depth somewhere: group (0,2)
                _put(reg, tg, o[i], CH['corner_uncertainty'] + 1, [-2.5])
            plan.update(kd=kd, hard=[o[0], o[4]])
    elif name == "depth_clamp":
        lo, hi = DEPTH_OFFSETS[depth_mode]
        for i, v in ((0, lo), (4, lo), (1, hi), (5, hi)):
            _put(reg, tg, o[i], CH['depth'], [v])
        plan.update(low=[o[0], o[4]], high=[o[1], o[5]])
    elif name == "unc_clamp":
        for i, v in ((0, -12.5), (4, -10.000001), (1, 11.0), (5, 10.000001), (2, -10.0), (6, -10.0), (3, 10.0), (7, 10.0)):
            _put(reg, tg, o[i], CH['depth_uncertainty'], [v])
            _put(reg, tg, o[i], CH['corner_uncertainty'], [v, v, v])
        plan.update(below=[o[0], o[4]], above=[o[1], o[5]], on_lo=[o[2], o[6]], on_hi=[o[3], o[7]])
    elif name == "box_edges":
        for i in (0, 4):
            _put(reg, tg, o[i], CH['2d_dim'], [-0.5, -1.0, -2.0, -1e-3])
        for i, vals in ((1, [2.0, 0.0, 3.0, 1.5]), (5, [0.0, 2.5, 1.0, 4.0])):
            _put(reg, tg, o[i], CH['2d_dim'], vals)
        for i in (2, 6):                                                   # left side distance exactly the target's: 3.0 in both precisions
            b, s = o[i]
            cx, cy = (float(x) for x in tg[b]["target_centers"][s])
            tg[b]["2d_bboxes"][s] = (cx - 3.0, cy - 2.5, cx + 4.0, cy + 1.5)
            _put(reg, tg, o[i], CH['2d_dim'], [3.0, 1.25, 5.0, 0.75])
        for i in (3, 7):
            b, s = o[i]
            tg[b]["2d_bboxes"][s][2] = tg[b]["2d_bboxes"][s][0]           # zero width: no bbox term for this object
        plan.update(negative=[o[0], o[4]], zero=[(o[1], 1), (o[5], 0)], tie=[o[2], o[6]], zero_area=[o[3], o[7]])
    elif name == "keypoint_heights":
        ky = lambda j: CH['corner_offset'] + 2 * j + 1
        # differences of exactly 0, slightly below 0, and so far below 0 that |dh| would give a depth INSIDE the range: relu, not abs
        for i, d in ((0, 0.0), (4, -10.0)):                                # centre group: ky[8] - ky[9]
            _put(reg, tg, o[i], ky(8), [1.0 + d]); _put(reg, tg, o[i], ky(9), [1.0])
        for i, (a, c), ds in ((1, (0, 2), (-10.0, -12.0)), (5, (0, 2), (0.0, -0.5)), (2, (1, 3), (-10.0, -12.0)), (6, (1, 3), (0.0, -0.5))):
            for j, d in zip((a, c), ds):                                   # groups (0,2)-(4,6) and (1,3)-(5,7)
                _put(reg, tg, o[i], ky(j), [0.25 + d]); _put(reg, tg, o[i], ky(j + 4), [0.25])
        for i in (0, 4, 1, 5, 2, 6):                                       # a positive height under linear dimensions too: fh > 0
            _put(reg, tg, o[i], CH['3d_dim'] + 1, [0.5])
        plan.update(groups=[(o[0], 0), (o[4], 0), (o[1], 1), (o[5], 1), (o[2], 2), (o[6], 2)])
    elif name == "counts_none":                       # no truncated object, every keypoint-depth group invalid, no visible keypoint
        for b, s in o:
            tg[b]["trunc_mask"][s] = 0
            tg[b]["keypoints_depth_mask"][s] = 0
            tg[b]["keypoints"][s, :, 2] = 0
    elif name == "counts_all":                                             # every object truncated, every group valid
        for b, s in o:
            tg[b]["trunc_mask"][s] = 1
            tg[b]["keypoints_depth_mask"][s] = 1
    elif name == "shared_centre":                                          # two rows of image 0 and three rows of image 2 on one pixel
        tg[0]["target_centers"][o[1][1]] = tg[0]["target_centers"][o[0][1]]
        tg[2]["target_centers"][o[5][1]] = tg[2]["target_centers"][o[4][1]]
        tg[2]["target_centers"][o[6][1]] = tg[2]["target_centers"][o[4][1]]
        plan.update(shared=[[o[0], o[1]], [o[4], o[5], o[6]]])
    else:
        raise KeyError(name)
    return tg, reg, cls, plan


class Reference:
    """The float64 tensor-op loss of one (configuration, input): terms, logged means, each term's gradient at the valid rows'
    centre pixels (10, R, 50), and the decoded intermediates of prepare_predictions (rows n = image*MAX_OBJECTS + slot)."""


@functools.lru_cache(maxsize=None)
def reference(cname, iname, dtype=torch.float64):
    from monoflex_amd.structures.params_3d import make_train_target
    ev = make_evaluator(cname)
    ev.fused_object_loss, ev.log_as_float = False, False
    tg, reg, cls, plan = make_input(iname, CONFIGS[cname]["depth_mode"])
    targets = [make_train_target(t) for t in tg]
    heat, tv = ev.prepare_targets(targets)
    r = reg.to(dtype).requires_grad_()
    loss_dict, logs = ev({"cls": cls.to(dtype), "reg": r}, (heat, tv))
    R = Reference()
    R.plan, R.n = plan, [b * ev.max_objs + s for b, s in plan["objects"]]
    R.pix = [(b,) + tuple(int(x) for x in tg[b]["target_centers"][s]) for b, s in plan["objects"]]           # (image, cx, cy)
    bi, cx, cy = (torch.tensor(x) for x in zip(*R.pix))
    R.terms = {k: float(loss_dict[k].detach()) if k in loss_dict else 0.0 for k in TERM_NAMES}
    R.logs = {k: float(v) for k, v in logs.items()}
    R.grads = torch.zeros(len(TERM_NAMES), len(R.n), 50, dtype=torch.float64)
    for i, k in enumerate(TERM_NAMES):
        if k in loss_dict:
            g, = torch.autograd.grad(loss_dict[k], r, retain_graph=True, allow_unused=True)
            if g is not None:
                R.grads[i] = g.permute(0, 2, 3, 1)[bi, cy, cx].double()
                off = g.permute(0, 2, 3, 1).clone()
                off[bi, cy, cx] = 0
                assert float(off.abs().max()) == 0.0                                                          # nothing off the centres
    with torch.no_grad():
        R.T, R.P, R.sel, _ = ev.prepare_predictions(tv, {"reg": r.detach()})
        R.poi = r.detach().permute(0, 2, 3, 1)[bi, cy, cx]                                                   # (R, 50) raw channels
    R.reg, R.targets, R.rows = reg, targets, tv["object_rows"]
    R.drop = _near_selection_rows(ev, R)
    assert R.drop.sum() <= 0.05 * len(R.n), (cname, iname, R.drop)
    return R


def _near_selection_rows(ev, R):
    """Valid rows whose float64 margin between the two candidates of a selection is below 1e-5 relative (exact ties are planted
    on purpose and stay in the comparison)."""
    n = torch.tensor(R.n)
    drop = torch.zeros(len(R.n), dtype=torch.bool)
    conf = torch.softmax(R.P['orien_3D'][n][:, :8].reshape(-1, 4, 2), dim=2)[..., 1].sort(dim=1, descending=True)[0]
    drop |= (conf[:, 0] - conf[:, 1]) < 1e-5 * conf[:, 0]
    unc = torch.cat((R.P['depth_uncertainty'][n].unsqueeze(1), R.P['corner_offset_uncertainty'][n]), dim=1).exp().sort(dim=1)[0]
    drop |= ((unc[:, 1] - unc[:, 0]) < 1e-5 * unc[:, 1]) & (unc[:, 1] != unc[:, 0])
    p, t = R.P['reg_2D'][n], R.T['reg_2D'][n]
    drop |= (((p - t).abs() < 1e-5 * t.abs().clamp(min=1e-30)) & (p != t)).any(dim=1) & R.sel['reg_2D'][n]
    return drop


def compare(R, terms, logged, grads, gtol, what):
    """terms[10], logged[14], grads (10, R, 50) (each term's gradient summed per centre pixel) against the float64 reference.
    Every figure is printed (in units of its bound) before the assertions."""
    worst = {"terms": 0.0, "logs": 0.0, "grads": 0.0}
    bad = []
    for i, k in enumerate(TERM_NAMES):
        ref = R.terms[k]
        e = abs(float(terms[i]) - ref) / (2e-5 * max(1.0, abs(ref)))
        worst["terms"] = max(worst["terms"], e)
        if not e <= 1.0:
            bad.append((k, float(terms[i]), ref))
    have = dict(zip(LOG_NAMES + ('3D_IoU',), [float(x) for x in logged[:12]]))
    for k, v in have.items():
        ref = R.logs[k]
        e = abs(v - ref) / (1e-4 * max(1.0, abs(ref)))
        worst["logs"] = max(worst["logs"], e)
        if not e <= 1.0:
            bad.append(("log " + k, v, ref))
    keep = ~R.drop
    for i, k in enumerate(TERM_NAMES):
        want = R.grads[i][keep]
        e = float((grads[i][keep].double() - want).abs().max()) / (gtol * max(1.0, float(want.abs().max())))
        worst["grads"] = max(worst["grads"], e)
        if not e <= 1.0:
            bad.append(("grad " + k, e))
    print("%s: error/bound terms %.3f logs %.3f grads %.3f (dropped rows %d)" % (what, worst["terms"], worst["logs"], worst["grads"],
                                                                                 int(R.drop.sum())))
    assert not bad, (what, bad)
    return worst


def shim_run(shim, cname, R):
    """The host build of the kernel math on the reference's inputs: terms, logged, per-term gradient at the centres, G, cfg."""
    ev = make_evaluator(cname)
    check_kernel_cfg(cname, ev)
    terms, logged, dreg, G, rows = run_object_shim(shim, ev, R.reg, R.targets)
    assert float(G[rows[:, 0] == 0].abs().max()) == 0.0 and float(G[..., 50:].abs().max()) == 0.0
    B, _, H, W = R.reg.shape
    bi, cx, cy = (torch.tensor(x) for x in zip(*R.pix))
    grads = torch.zeros(len(TERM_NAMES), len(R.n), 50)
    for i in range(len(TERM_NAMES)):
        dense = torch.zeros(B, H, W, 50)
        for n in R.n:
            dense[int(rows[n, 57]), int(rows[n, 3]), int(rows[n, 2])] += G[n, i, :50]
        grads[i] = dense[bi, cy, cx]
    return terms, logged, grads, G


def rows_of(R, objs):
    """Positions (in R.n / R.pix / R.poi order) and table rows n of the planted objects."""
    pos = [R.plan["objects"].index(o) for o in objs]
    return pos, [R.n[p] for p in pos]


# ---- the edge checks, shared with the device tests: assert from the float64 reference that the edge is hit, then what the edge demands
def check_edge(R, cname, ename, grads):
    """`grads` (10, R, 50): each term's gradient at the centres, from the host build or from the device."""
    s, plan, P, T = CONFIGS[cname], R.plan, R.P, R.T
    depth_range = (0.1, 100.0)
    if ename == "depth_clamp":
        for objs, bound, beyond in ((plan["low"], depth_range[0], lambda d: d < 0.1), (plan["high"], depth_range[1], lambda d: d > 100.0)):
            pos, n = rows_of(R, objs)
            off = R.poi[pos, CH['depth']]
            raw = {'exp': off.exp(), 'linear': off * 16.05988 + 26.494627, 'inv_sigmoid': 1 / torch.sigmoid(off) - 1}[s["depth_mode"]]
            assert len(n) >= 2 and bool(beyond(raw).all()) and bool((P['depth_3D'][n] == bound).all())
            assert float(R.grads[:, pos, CH['depth']].abs().max()) == 0.0
            assert float(grads[:, pos, CH['depth']].abs().max()) == 0.0                     # exactly 0 through the clamp
    elif ename == "unc_clamp":
        chans = [CH['depth_uncertainty']] + [CH['corner_uncertainty'] + g for g in range(3)]
        for key, bound in (("below", -10.0), ("above", 10.0)):
            pos, n = rows_of(R, plan[key])
            raw = R.poi[pos][:, chans]
            assert len(n) >= 2 and bool(((raw < -10.0) if bound < 0 else (raw > 10.0)).all())
            assert bool((P['depth_uncertainty'][n] == bound).all()) and bool((P['corner_offset_uncertainty'][n] == bound).all())
            assert float(R.grads[:, pos][:, :, chans].abs().max()) == 0.0 and float(grads[:, pos][:, :, chans].abs().max()) == 0.0
        for key, bound in (("on_lo", -10.0), ("on_hi", 10.0)):
            pos, n = rows_of(R, plan[key])
            assert len(n) >= 2 and bool((R.poi[pos][:, chans] == bound).all())
            g = R.grads[:, pos][:, :, chans].abs().sum(0)
            assert bool((g > 0).all()) and bool((grads[:, pos][:, :, chans].abs().sum(0) > 0).all())       # the gradient passes ON the bound
    elif ename == "box_edges":
        c2 = slice(CH['2d_dim'], CH['2d_dim'] + 4)
        pos, n = rows_of(R, plan["negative"])
        assert len(n) >= 2 and bool((R.poi[pos, c2] < 0).all()) and float(P['reg_2D'][n].abs().max()) == 0.0 and bool(R.sel['reg_2D'][n].all())
        assert float(grads[:, pos, c2].abs().max()) == 0.0                                   # relu: p_area = 0 and no gradient
        for o, k in plan["zero"]:
            pos, n = rows_of(R, [o])
            assert float(R.poi[pos[0], CH['2d_dim'] + k]) == 0.0 and bool(R.sel['reg_2D'][n[0]])
            assert float(grads[:, pos[0], CH['2d_dim'] + k].abs().max()) == 0.0              # relu'(0) = 0 as torch
        pos, n = rows_of(R, plan["tie"])
        assert len(n) >= 2 and bool((P['reg_2D'][n][:, 0] == T['reg_2D'][n][:, 0]).all()) and bool((T['reg_2D'][n][:, 0] == 3.0).all())
        assert bool((R.grads[0, pos, CH['2d_dim']] != 0).all())
        pos, n = rows_of(R, plan["zero_area"])
        assert len(n) >= 2 and not bool(R.sel['reg_2D'][n].any()) and bool(R.sel['valid'][n].all())
        assert float(R.grads[0, pos].abs().max()) == 0.0 and float(R.grads[1:, pos].abs().max()) > 0   # bbox skipped, the rest kept
        assert float(grads[0, pos].abs().max()) == 0.0 and float(grads[1:, pos].abs().max()) > 0
    elif ename == "keypoint_heights":
        for o, g in plan["groups"]:
            pos, n = rows_of(R, [o])
            ky = R.poi[pos[0], CH['corner_offset'] + 1:CH['corner_offset'] + 20:2]
            dh = {0: ky[8:9] - ky[9:10], 1: ky[0:3:2] - ky[4:7:2], 2: ky[1:4:2] - ky[5:8:2]}[g]
            assert bool((dh <= 0).all()) and float(P['keypoints_depths'][n[0], g]) == depth_range[1]          # fh / eps, then the clamp
            fh = float(P['dims_3D'][n[0], 1]) * float(R.rows[n[0], 66])
            if bool((dh <= -10).all()):                                    # |dh| in place of relu(dh) would land inside the range
                assert 0.1 < float((fh / (dh.abs() * 4 + 1e-3)).mean()) < 100.0
        assert len(plan["groups"]) >= 6 and sum(bool((R.poi[rows_of(R, [o])[0][0]] <= -9).any()) for o, _ in plan["groups"]) >= 3
    elif ename in ("counts_none", "counts_all"):
        # What these two inputs can show: the reference's `max(count, 1)` guards turn an empty selection into a 0 term, and the
        # kernel must give that 0 (not 0/0).  In the kernel itself only the visible-keypoint count's guard is reachable this way:
        # cnt(N_TRUNC), cnt(N_V_INSIDE), cnt(N_KD_VALID) and cnt(N_KD_INVALID) are each read only inside the branch that counted the
        # row, so they are >= 1 wherever they are used and their guards cannot be observed through the kernel's output.
        n = R.n
        km = T['keypoints_depth_mask'][n]
        trunc = T['trunc_mask_3D'][n]
        if ename == "counts_none":
            assert not bool(km.any()) and not bool(trunc.any()) and R.terms['trunc_offset_loss'] == 0.0
            assert float(T['keypoints_mask'][n].abs().max()) == 0.0 and R.terms['keypoint_loss'] == 0.0
            assert float(grads[TERM_NAMES.index('keypoint_loss')].abs().max()) == 0.0
        else:
            assert bool(km.all()) and bool(trunc.all())
            assert R.terms['offset_loss'] == 0.0 or not s["separate_trunc"]
    elif ename == "shared_centre":
        for group in plan["shared"]:
            pos, n = rows_of(R, group)
            assert len({R.pix[p] for p in pos}) == 1 and len(set(n)) == len(group)
            assert float((R.grads[:, pos] - R.grads[:, pos[:1]]).abs().max()) == 0.0        # one pixel: the summed gradient
        assert sorted(len(g) for g in plan["shared"]) == [2, 3]


def check_input(R, cname, iname, grads):
    """What an input of INPUTS is there for, asserted from the float64 reference (and, for gradients, from `grads` as well)."""
    s, n = CONFIGS[cname], R.n
    if iname in ("b3_mixed", "kd_interior"):
        assert 0 < int(R.T['trunc_mask_3D'][n].sum()) < len(n) and not bool(R.T['keypoints_depth_mask'][n].all())
        assert bool((~R.T['keypoints_depth_mask'][n]).all(dim=1).any())          # an object with every group invalid
    if cname == "unc_range_1":
        raw = R.poi[:, [CH['depth_uncertainty']] + [CH['corner_uncertainty'] + g for g in range(3)]]
        assert bool((raw.abs() > 1).any()) and float(R.P['corner_offset_uncertainty'][n].abs().max()) <= 1.0      # the clamp is active
    kd_all = R.P['keypoints_depths'][n]
    if iname != "kd_interior":
        return
    T_KD, T_CORNER = TERM_NAMES.index('keypoint_depth_loss'), TERM_NAMES.index('corner_loss')
    per_group = {0: 0, 1: 0, 2: 0}
    for o, g in R.plan["kd"]:
        pos, rn = rows_of(R, [o])
        chans = [CH['corner_offset'] + 2 * j + 1 for pair in KD_PAIRS[g] for j in pair]
        assert 0.1 < float(R.P['keypoints_depths'][rn[0], g]) < 100.0                                  # strictly inside DEPTH_RANGE
        per_group[g] += 1
        if bool(R.T['keypoints_depth_mask'][rn[0], g]):                                                # (an invalid group is detached)
            assert bool((R.grads[T_KD, pos[0], chans] != 0).all()) and bool((grads[T_KD, pos[0], chans] != 0).all())
        if s["corner_depth_mode"] in ("keypoint_mean", "soft_combine"):
            assert bool((R.grads[T_CORNER, pos[0], chans] != 0).all()) and bool((grads[T_CORNER, pos[0], chans] != 0).all())
        elif s["corner_depth_mode"] == "direct":
            assert float(grads[T_CORNER, pos[0], chans].abs().max()) == 0.0
    assert min(per_group.values()) >= 2 and int(((kd_all > 0.1) & (kd_all < 100.0)).sum()) >= 16
    if s["corner_depth_mode"] == "hard_combine":                             # the arg-min lands on the (0,2) group's depth for two objects
        pos, rn = rows_of(R, R.plan["hard"])
        unc = torch.cat((R.P['depth_uncertainty'][rn].unsqueeze(1), R.P['corner_offset_uncertainty'][rn]), dim=1)
        chans = [CH['corner_offset'] + 2 * j + 1 for pair in KD_PAIRS[1] for j in pair]
        assert bool((unc.argmin(dim=1) == 2).all())
        assert bool((R.grads[T_CORNER, pos][:, chans] != 0).all()) and bool((grads[T_CORNER, pos][:, chans] != 0).all())


# ---- tests ------------------------------------------------------------------------------------------------------------------------
def test_configuration_set_is_the_documented_one():
    names = sorted(CONFIGS)
    print("object-loss configurations covered (%d): %s" % (len(names), ", ".join(names)))
    assert len(names) == 37 and len({tuple(sorted((k, str(v)) for k, v in s.items())) for s in CONFIGS.values()}) == 37
    sw = lambda s: tuple(s[k] for k in SWITCHES)
    have = {sw(s) for s in CONFIGS.values()}
    for base in (BASE_YAML, BASE_DEFAULTS):                                  # one switch at a time around both baselines
        assert sw(base) in have
        for key, values in SWITCHES.items():
            for v in values:
                assert sw(dict(base, **{key: v})) in have, (key, v)
    grid = {(s["depth_mode"], s["corner_depth_mode"]) for s in CONFIGS.values()}
    assert len(grid) == 12
    assert {(s["separate_trunc"], s["trunc_log"]) for s in CONFIGS.values()} == {(0, 0), (0, 1), (1, 0), (1, 1)}
    assert {(s["dim_exp"], s["dim_use_std"]) for s in CONFIGS.values()} == {(0, 0), (0, 1), (1, 0), (1, 1)}
    assert any(s["unc_range"] == (-1, 1) for s in CONFIGS.values()) and any(s["weights"] for s in CONFIGS.values())
    assert overrides(BASE_YAML) == []                                        # the yaml baseline is the file itself


def test_defaults_baseline_is_config_py():
    """The second baseline's switch values are what monoflex_amd/config.py gives when a yaml does not set them."""
    from monoflex_amd.config import get_cfg
    H = get_cfg().MODEL.HEAD
    s = BASE_DEFAULTS
    assert H.DEPTH_MODE == s["depth_mode"] and H.CORNER_LOSS_DEPTH == s["corner_depth_mode"] and H.LOSS_TYPE[2] == s["iou_type"]
    assert (H.DIMENSION_REG[0] == 'exp', bool(H.DIMENSION_REG[2])) == (bool(s["dim_exp"]), bool(s["dim_use_std"]))
    assert (H.TRUNCATION_OFFSET_LOSS != 'L1') == bool(s["trunc_log"]) and bool(H.MODIFY_INVALID_KEYPOINT_DEPTH) == bool(s["modify_invalid"])
    assert tuple(H.UNCERTAINTY_RANGE) == s["unc_range"] and list(H.DIMENSION_WEIGHT) == [1, 1, 1]


@pytest.mark.parametrize("iname", INPUTS)
@pytest.mark.parametrize("cname", sorted(CONFIGS))
def test_config_kernel_math_vs_float64(cname, iname, object_loss_shim):
    """Ten terms, logged means and each term's own gradient row, per configuration, against the float64 tensor-op form."""
    R = reference(cname, iname)
    terms, logged, grads, _ = shim_run(object_loss_shim, cname, R)
    check_input(R, cname, iname, grads)
    compare(R, terms, logged, grads, 1e-5, "%s/%s shim" % (cname, iname))


def edge_cases():
    out = []
    for e in EDGES:
        cn = list(EDGE_CONFIGS)
        if e == "depth_clamp":
            cn += ["yaml-depth_mode=exp", "yaml-depth_mode=linear"]
        if e == "box_edges":
            cn += ["yaml-iou_type=iou", "yaml-iou_type=linear_iou"]
        if e in ("counts_none", "counts_all"):
            cn += ["yaml-separate_trunc=0", "defaults-trunc_log=1", "defaults-modify_invalid=1"]
        if e == "unc_clamp":
            cn += ["yaml-corner_depth_mode=hard_combine"]
        out += [(c, e) for c in cn]
    return out


@pytest.mark.parametrize("cname,ename", edge_cases())
def test_edge_kernel_math_vs_float64(cname, ename, object_loss_shim):
    """Inputs ON a clamp, a relu zero, a min/max tie, a count guard or a shared centre pixel (module docstring)."""
    R = reference(cname, ename)
    terms, logged, grads, G = shim_run(object_loss_shim, cname, R)
    check_edge(R, cname, ename, grads)
    compare(R, terms, logged, grads, 1e-5, "%s/%s shim" % (cname, ename))


YARDSTICK_CASES = [(c, "kd_interior") for c in sorted(CONFIGS)] + [(c, i) for c in EDGE_CONFIGS for i in ("b3", "b3_mixed")] \
    + [(c, e) for c, e in edge_cases() if c in EDGE_CONFIGS]


@pytest.mark.parametrize("cname,iname", YARDSTICK_CASES)
def test_float32_tensor_ops_stay_under_a_quarter_of_each_bound(cname, iname):
    """The yardstick of the module docstring's table: the float32 tensor-op form (no code under test) against the float64 form on
    the same inputs.  Four times its error must fit every bound used here -- otherwise that bound would ask more of the kernel
    than float32 arithmetic can give, and would have to come from this measurement instead."""
    R, R32 = reference(cname, iname), reference(cname, iname, torch.float32)
    terms = [R32.terms[k] for k in TERM_NAMES]
    logged = [R32.logs[k] for k in LOG_NAMES + ('3D_IoU',)]
    worst = compare(R, terms, logged, R32.grads, 1e-5, "%s/%s float32 tensor ops" % (cname, iname))
    assert max(worst.values()) <= 0.25, worst
