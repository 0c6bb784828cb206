"""Configurations, seeded inputs and shared helpers of the head-set tests (tests/test_head_sets_*.py, tests/test_gpu_head_sets*.py): how a set of
tests/head_sets_ref.py becomes a config of this project, the loss input the goldens were recorded on, and the small loss inputs of the
device tests.  The float64 restatement itself (tests/head_sets_ref.py) imports nothing from here or from the project."""
import functools
import os

import numpy as np
import torch

from tests import head_sets_ref as HS

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
YAML = os.path.join(ROOT, "runs", "monoflex.yaml")
HEAD = "MODEL.HEAD."
TERM_NAMES = ('bbox_loss', 'depth_loss', 'offset_loss', 'trunc_offset_loss', 'orien_loss', 'dims_loss', 'corner_loss', 'keypoint_loss',
              'keypoint_depth_loss', 'weighted_avg_depth_loss')                      # mfx_object_loss's term order
LOG_SLOTS = ('2D_IoU', 'depth_loss', 'keypoint_depth_loss', 'depth_MAE', 'center_MAE', '02_MAE', '13_MAE', 'lower_MAE', 'hard_MAE', 'soft_MAE',
             'mean_MAE')                                                             # mfx_object_loss's logged values 0..10
SET_MODES = [(n, m) for n in HS.SETS for m in HS.corner_depths(n)]                   # every set x the corner depths it serves (15)


def overrides(name, corner="direct", names=None, modify=True, extra=()):
    nm, w = HS.loss_names(name) if names is None else names
    return [HEAD + "REGRESSION_HEADS", HS.SETS[name], HEAD + "REGRESSION_CHANNELS", HS.channels(name), HEAD + "LOSS_NAMES", list(nm),
            HEAD + "INIT_LOSS_WEIGHT", list(w), HEAD + "CORNER_LOSS_DEPTH", corner, HEAD + "MODIFY_INVALID_KEYPOINT_DEPTH", bool(modify)] + list(extra)


def cfg_for(name, **kw):
    from monoflex_amd.config import get_cfg
    return get_cfg(YAML, overrides(name, **kw))


def model_cfg(name, extra=()):
    """A whole-model config of a set: runs/monoflex.yaml with the set's heads and loss names, CORNER_LOSS_DEPTH direct, and the yaml's
    OUTPUT_DEPTH soft where the set can serve it (corner_uncertainty), direct otherwise."""
    return cfg_for(name, extra=[HEAD + "OUTPUT_DEPTH", "soft" if HS.flags(name)[2] else "direct"] + list(extra))


def settings(corner="direct", modify=True, **kw):
    return HS.yaml_settings(corner_depth=corner, modify_invalid=modify, **kw)


@functools.lru_cache(maxsize=None)
def golden_input():
    """Input `kd_interior` of tests/test_object_loss_configs_cpu.py in the canonical 50 channels: (target dicts, cls, reg (3,50,96,320), objects)."""
    import tests.test_object_loss_configs_cpu as T
    tg, reg, cls, plan = T.make_input("kd_interior")
    return tg, cls, reg, plan["objects"]


def golden():
    return np.load(os.path.join(ROOT, "tests", "golden", "head_sets.npz"), allow_pickle=False)


# ---- the small loss input of the device tests: B = 3, 24 x 80 map, MAX_OBJECTS 40 --------------------------------------------------------
SMALL = dict(out_w=80, out_h=24, B=3, max_objs=40)
SMALL_SEED = 1                       # chosen on the CPU: no valid row of any set sits near a selection (tests/test_head_sets_cpu.py asserts the 5 % cap)


def small_input(seed, modify=True):
    """(target dicts, reg (3, 50, 24, 80) float32 canonical channels, plan): image 1 has no object; truncated objects; invalid keypoint
    groups (one object with all three); keypoint depths inside DEPTH_RANGE for most objects; uncertainties below, on and above both clamps;
    a 2D box of zero area.  Everything is planted, so the properties hold for every seed; `plan` names the planted objects."""
    from monoflex_amd import synthetic as S
    rs = np.random.RandomState(seed)
    tg = []
    for b, n_obj in enumerate((6, 0, 7)):
        P = np.array(S.KITTI_P2, dtype=np.float64).reshape(3, 4).copy()
        P[0, 0] *= (1.0, 1.1, 1.2)[b]
        P[1, 1] *= (1.0, 1.1, 1.2)[b]
        tg.append(S.synthetic_train_target(seed * 10 + b, out_w=SMALL["out_w"], out_h=SMALL["out_h"], n_obj=n_obj, max_objs=SMALL["max_objs"], P=P))
    objs = [(b, int(s)) for b, t in enumerate(tg) for s in np.nonzero(t["reg_mask"])[0]]
    assert len(objs) >= 8 and not tg[1]["reg_mask"].any() and {b for b, _ in objs} == {0, 2}
    g = torch.Generator().manual_seed(1000 + seed)
    reg = torch.randn(SMALL["B"], 50, SMALL["out_h"], SMALL["out_w"], generator=g) * 0.6
    put = lambda o, ch, vals: reg.__setitem__((o[0], slice(ch, ch + len(vals)), int(tg[o[0]]["target_centers"][o[1]][1]),
                                               int(tg[o[0]]["target_centers"][o[1]][0])), torch.tensor(vals, dtype=torch.float32))
    C = HS.CANON
    for o in (objs[0], objs[-1]):
        tg[o[0]]["trunc_mask"][o[1]] = 1
    for o in objs[1:-1]:
        tg[o[0]]["trunc_mask"][o[1]] = 0
    for o, m in ((objs[1], (0, 1, 1)), (objs[2], (0, 0, 0)), (objs[-2], (1, 0, 1)), (objs[-3], (1, 1, 0)), (objs[0], (1, 1, 1)), (objs[3], (1, 1, 1))):
        tg[o[0]]["keypoints_depth_mask"][o[1]] = m
    # keypoint spans of several cells: every group's depth f h / (4 dh) strictly inside (0.1, 100) for all but the last object
    ky = lambda j: C['corner_offset'] + 2 * j + 1
    for i, o in enumerate(objs[:-1]):
        put(o, C['3d_dim'] + 1, [0.3])
        for (a, c), dh in (((8, 9), 10.0), ((0, 4), 9.0), ((2, 6), 14.0), ((1, 5), 11.0), ((3, 7), 8.0)):
            put(o, ky(a), [0.25 + dh + 0.5 * i]); put(o, ky(c), [0.25])
    # uncertainties: below / on / above the clamps of UNCERTAINTY_RANGE [-10, 10], the rest inside
    for o, v in ((objs[0], -12.5), (objs[1], 11.0), (objs[2], -10.0), (objs[3], 10.0)):
        put(o, C['depth_uncertainty'], [v]); put(o, C['corner_uncertainty'], [v, v + (0.0 if abs(v) == 10 else 0.25), v])
    for o in objs[4:]:
        put(o, C['depth_uncertainty'], [float(rs.uniform(-2, 1))]); put(o, C['corner_uncertainty'], list(rs.uniform(-2.5, 1, 3)))
    zb, zs = objs[4]
    tg[zb]["2d_bboxes"][zs][2] = tg[zb]["2d_bboxes"][zs][0]                          # zero width: no bbox term for this object
    plan = dict(objects=objs, trunc=[objs[0], objs[-1]], invalid_all=objs[2], unc_below=objs[0], unc_above=objs[1], unc_on=[objs[2], objs[3]],
                zero_area=objs[4])
    return tg, reg, plan


# ---- helpers shared by the CPU and the device tests --------------------------------------------------------------------------------------
def evaluator(name, **kw):
    from monoflex_amd.model.head.detector_loss import Loss_Computation
    return Loss_Computation(cfg_for(name, **kw))


def compare_with_restatement(what, name, ref, grads_ref, terms, logged, grads, gtol, drop=None):
    """terms[10], logged[>= 11], grads (10, n, R) against the restatement; absent terms and logged values must be exactly 0.  Prints every
    figure in units of its bound before asserting."""
    worst = {"terms": 0.0, "logs": 0.0, "grads": 0.0}
    bad = []
    for i, k in enumerate(TERM_NAMES):
        want = float(ref.terms[k].detach()) if k in ref.terms else 0.0
        if k not in ref.terms:
            if float(terms[i]) != 0.0 or float(grads[i].abs().max()) != 0.0:
                bad.append((k, "absent term is not exactly 0", float(terms[i])))
            continue
        e = abs(float(terms[i]) - want) / (2e-5 * max(1.0, abs(want)))
        worst["terms"] = max(worst["terms"], e)
        if not e <= 1:
            bad.append((k, float(terms[i]), want))
    for i, k in enumerate(LOG_SLOTS):
        if k == 'keypoint_depth_loss' and HS.flags(name)[1] and k not in ref.logs:
            continue                                                 # (the kernel reports the value even when the loss name is left out)
        if k not in ref.logs:
            if float(logged[i]) != 0.0:
                bad.append(("log " + k, "absent value is not exactly 0", float(logged[i])))
            continue
        e = abs(float(logged[i]) - ref.logs[k]) / (1e-4 * max(1.0, abs(ref.logs[k])))
        worst["logs"] = max(worst["logs"], e)
        if not e <= 1:
            bad.append(("log " + k, float(logged[i]), ref.logs[k]))
    keep = torch.ones(ref.n, dtype=torch.bool) if drop is None else ~drop
    for i, k in enumerate(TERM_NAMES):
        want = grads_ref[i][keep]
        e = float((grads[i][keep].double() - want).abs().max()) / (gtol * max(1.0, float(want.abs().max())))
        worst["grads"] = max(worst["grads"], e)
        if not e <= 1:
            bad.append(("grad " + k, e))
    print("%s: error/bound terms %.3f logs %.3f grads %.3f (dropped rows %d)" % (what, worst["terms"], worst["logs"], worst["grads"], int((~keep).sum())))
    assert not bad, (what, bad)
    return worst


def small_case(name, corner, modify, seed=SMALL_SEED):
    """The device tests' small input (B = 3, 24 x 80, MAX_OBJECTS 40) in the set's layout with its float64 restatement:
    (evaluator, target dicts, reg_set (3, R, 24, 80) float32, ref, per-term gradients (10, n, R), near-selection rows, plan)."""
    tg, reg, plan = small_input(seed)
    reg_set = HS.take(reg, name, 1)
    ev = evaluator(name, corner=corner, modify=modify)
    r = reg_set.double().requires_grad_()
    ref = HS.loss_ref(name, r, tg, settings(corner, modify), *HS.loss_names(name))
    return ev, tg, reg_set, ref, HS.term_gradients(ref, r, TERM_NAMES), HS.near_selection_rows(ref), plan
