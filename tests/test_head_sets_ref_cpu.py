"""Anchors of the float64 restatement of the reduced head sets (tests/head_sets_ref.py) -- no code of the project is under test here
except where stated.

1. loss_ref reproduces what the reference's own Loss_Computation gave under each of the five new sets, every CORNER_LOSS_DEPTH the set can
   serve, one reduced LOSS_NAMES list per set and MODIFY_INVALID_KEYPOINT_DEPTH False (tests/golden/head_sets.npz): the names of the loss
   and log dicts, their values, the gradient of the summed loss at the objects' centres.  Bounds of tests/test_loss_golden.py /
   tests/test_object_loss_configs_cpu.py: terms 2e-5 max(1,|ref|), logged 1e-4 max(1,|ref|), gradient 1e-5 max(1,max|ref|).
2. decode_ref reproduces the recorded PostProcessor rows and estimated_depth_error / uncertainty_conf (or None) under every OUTPUT_DEPTH
   the set can serve, with and without UNCERTAINTY_AS_CONFIDENCE, within 4x the float32 yardstick of tests/decode_cfg_ref.py (the bound
   tests/test_decode_cfg_ref_cpu.py anchors with).
3. For the full set both EQUAL the restatements the suite already pins (tests/decode_cfg_ref.py; the float64 tensor-op loss of
   tests/test_object_loss_configs_cpu.py within float64 rounding).
   (Point 3's decode comparison is between two test-side restatements and touches no project code: unlike every other new test it also
   passes without the feature.  It is kept as the anchor that ties the new restatement to the one the suite already pins.)
4. The acceptance matrix of the restatement refuses exactly what the reference raised on.
"""
import numpy as np
import pytest
import torch

from tests import decode_cases as C
from tests import decode_cfg_ref as DC
from tests import decode_ref as D
from tests import head_sets_cases as HC
from tests import head_sets_ref as HS

LOSS_TAGS = [(n, m, m, True, ()) for n in HS.NEW_SETS for m in HS.corner_depths(n)] + \
    [(n, "names", "direct", True, None) for n in HS.NEW_SETS] + [("s010", "direct_no_modify", "direct", False, ())]


def _ref_loss(name, corner, modify, drop):
    tg, cls, reg, objs = HC.golden_input()
    r = HS.take(reg, name, 1).double().requires_grad_()
    names, weights = HS.loss_names(name, drop)
    return HS.loss_ref(name, r, tg, HC.settings(corner, modify), names, weights), r, names


@pytest.mark.parametrize("name,tag,corner,modify,drop", LOSS_TAGS, ids=["%s-%s" % t[:2] for t in LOSS_TAGS])
def test_loss_restatement_reproduces_the_reference(name, tag, corner, modify, drop):
    g = HC.golden()
    key = "%s/%s" % (name, tag)
    if drop is None:
        drop = tuple(str(x) for x in g[name + "/names/dropped"])
        assert len(drop) >= 1
    ref, r, names = _ref_loss(name, corner, modify, drop)
    loss_keys, log_keys = [str(k) for k in g[key + "/loss_keys"]], [str(k) for k in g[key + "/log_keys"]]
    assert set(loss_keys) == set(ref.terms) | {'hm_loss'} == HS.expected_loss_keys(name, names)
    assert set(log_keys) == set(ref.logs) | {'hm_loss', '3D_IoU'} == HS.expected_log_keys(name, names)
    worst = {"terms": 0.0, "logs": 0.0}
    for k, v in zip(loss_keys, g[key + "/loss_values"]):
        if k != 'hm_loss':
            worst["terms"] = max(worst["terms"], abs(float(ref.terms[k].detach()) - v) / (2e-5 * max(1.0, abs(v))))
    for k, v in zip(log_keys, g[key + "/log_values"]):
        if k not in ('hm_loss', '3D_IoU'):
            worst["logs"] = max(worst["logs"], abs(ref.logs[k] - v) / (1e-4 * max(1.0, abs(v))))
    sum(ref.terms.values()).backward()
    want = g[key + "/grad_reg_at_objects"]
    got = r.grad.permute(0, 2, 3, 1)[ref.bi, ref.cen[:, 1], ref.cen[:, 0]].numpy()
    ge = np.abs(got - want).max() / (1e-5 * max(1.0, np.abs(want).max()))
    # (hm_loss does not read the regression map: the whole gradient of the recorded summed loss is the regression terms')
    ae = abs(float(r.grad.abs().sum()) - float(g[key + "/grad_reg_abssum"])) / (1e-4 * float(g[key + "/grad_reg_abssum"]))
    print("%s: error/bound terms %.3f logs %.3f gradient %.3f |gradient| sum %.3f" % (key, worst["terms"], worst["logs"], ge, ae))
    assert worst["terms"] <= 1 and worst["logs"] <= 1 and ge <= 1 and ae <= 1 and want.shape == (8, HS.WIDTHS[name])


def test_loss_restatement_inputs_exercise_the_absent_head_branches():
    """The recorded input has truncated objects, invalid keypoint groups whose detached term is not zero, and keypoint depths inside the
    range: the arithmetic that changes with an absent head is not compared on zeros."""
    g = HC.golden()
    v = lambda key, k: float(g[key + "/loss_values"][[str(x) for x in g[key + "/loss_keys"]].index(k)])
    assert v("s010/direct", 'keypoint_depth_loss') > v("s010/direct_no_modify", 'keypoint_depth_loss') > 0      # the detached invalid term has a value
    assert v("s011/direct", 'keypoint_depth_loss') != v("s010/direct", 'keypoint_depth_loss')                   # exp(-u) and + w u change it
    assert v("s100/direct", 'depth_loss') != v("s000/direct", 'depth_loss') and v("s000/direct", 'trunc_offset_loss') > 0
    assert v("s010/keypoint_mean", 'corner_loss') != v("s010/direct", 'corner_loss')
    ref, _, _ = _ref_loss("s011", "direct", True, ())
    assert int(((ref.kd > 0.1) & (ref.kd < 100.0)).sum()) >= 12 and not bool(ref.kdm.all()) and bool((~ref.kdm).all(dim=1).any())


def _decode_golden_inputs():
    g = HC.golden()
    images = tuple(int(i) for i in np.atleast_1d(g["decode_inputs/images"]))
    maps = C.structured_maps(int(g["decode_inputs/map_seed"]), images)
    scores, index = C.peak_lists(int(g["decode_inputs/list_seed"]), len(images), int(g["decode_inputs/K"]),
                                 [tuple(r) for r in np.atleast_2d(g["decode_inputs/score_ranges"])])
    return g, maps, scores, index


@pytest.mark.parametrize("name", HS.NEW_SETS)
def test_decode_restatement_reproduces_the_reference(name):
    g, maps, scores, index = _decode_golden_inputs()
    hm = HS.take(maps["hmap"][..., maps["reg_off"]:maps["reg_off"] + 50], name, 3)
    modes = [str(m) for m in g[name + "/decode/modes"]]
    assert tuple(modes) == HS.output_depths(name)
    bound = DC.bounds("yaml")
    rows_total = 0
    for uac in (1, 0):
        for m, mode in enumerate(modes):
            ref = HS.decode_ref(name, hm, 0, scores, index, maps["calib"], maps["pad"], maps["sizes"][0], C.THRESHOLD, mode,
                                HC.settings(uncertainty_as_conf=bool(uac)))
            keep = ref["valid"].astype(bool)
            rows = np.concatenate((g[name + "/decode/cols0_9"], g[name + "/decode/cols9_14"][m]), axis=1).astype(np.float64)
            if not uac:
                rows[:, 13] = g[name + "/decode/raw_score"][m]
            assert rows.shape == (int(keep.sum()), 14) and 0 < rows.shape[0] < 50
            full = ref["det"].copy()
            full[keep] = rows
            err = D.column_errors(full, ref, mode, rows=keep)
            none = bool(g[name + "/decode/error_is_none"][uac, m])
            assert none == (not (uac and HS.has_depth_error(name, mode))), (name, mode, uac)
            if none:
                assert (ref["unc"] == 0).all() and np.array_equal(rows[:, 13], ref["topk"][keep][:, 0])          # the raw score
            else:
                want = ref["unc"][keep]
                ue = (np.abs(g[name + "/decode/error"][m] - want) / np.maximum(1, np.abs(want))).max()
                assert ue <= bound[13], (name, mode, ue)
            print("%s %s uac %d: %s" % (name, mode, uac, D.format_errors(err)))
            assert (err <= bound).all(), (name, mode, uac, D.format_errors(err))
            assert float(D.near_rows(ref, mode).mean()) <= D.NEAR_CAP
            rows_total += rows.shape[0]
    assert rows_total >= 2 * len(modes) * 20


@pytest.mark.parametrize("mode", D.MODES)
def test_decode_restatement_of_the_full_set_equals_decode_cfg_ref(mode):
    d = C.case_inputs("b3_k50")
    old = DC.run_ref(d, mode, DC.YAML)
    new = HS.decode_ref("s111", d["hmap"], d["reg_off"], d["scores"], d["index"], d["calib"], d["pad"], d["img_size"], d["threshold"], mode,
                        HC.settings())
    for k in ("topk", "valid"):
        assert np.array_equal(new[k], old[k]), k
    for k in ("det", "unc"):                                            # the same formulas; sums may associate differently
        assert np.abs(new[k] - old[k]).max() <= 1e-12 * max(1.0, np.abs(old[k]).max()), k
    for k in ("bin_margin", "alpha_wrap_dist", "ry_wrap_dist"):
        assert np.allclose(new[k], old[k], rtol=1e-9, atol=1e-12), k


@pytest.mark.parametrize("cname", ["yaml", "yaml-corner_depth_mode=direct", "yaml-corner_depth_mode=keypoint_mean", "yaml-corner_depth_mode=hard_combine"])
def test_loss_restatement_of_the_full_set_equals_the_pinned_float64_form(cname):
    """The full set against the float64 tensor-op reference of tests/test_object_loss_configs_cpu.py (itself pinned to tests/golden/loss.npz),
    on input kd_interior: terms, logged values and per-term gradients agree to 1e-6 relative -- both are float64 arithmetic, but that form
    holds DIMENSION_MEAN and the weights as float32 tensors (6e-8 relative each) where this restatement takes the config's Python floats."""
    import tests.test_object_loss_configs_cpu as T
    R = T.reference(cname, "kd_interior")
    tg, cls, reg, objs = HC.golden_input()
    r = reg.double().requires_grad_()
    corner = T.CONFIGS[cname]["corner_depth_mode"]
    ref = HS.loss_ref("s111", r, tg, HC.settings(corner), *HS.loss_names("s111"))
    for k in HC.TERM_NAMES:
        assert abs(float(ref.terms[k].detach()) - R.terms[k]) <= 1e-6 * max(1.0, abs(R.terms[k])), k
    for k, v in ref.logs.items():
        assert abs(v - R.logs[k]) <= 1e-6 * max(1.0, abs(R.logs[k])), k
    grads = HS.term_gradients(ref, r, HC.TERM_NAMES)
    assert float((grads - R.grads).abs().max()) <= 1e-6 * max(1.0, float(R.grads.abs().max()))


def test_acceptance_matrix_refuses_what_the_reference_raised_on():
    g = HC.golden()
    labels = [str(x) for x in g["raises/labels"]]
    assert len(labels) == 9
    for lab in labels:
        assert str(g["raises/" + lab]) in ("KeyError", "UnboundLocalError"), lab
    assert 'keypoint_mean' not in HS.corner_depths("s000") and 'soft_combine' not in HS.corner_depths("s011")
    assert 'hard_combine' not in HS.corner_depths("s110") and 'keypoints_avg' not in HS.output_depths("s100")
    assert 'soft' not in HS.output_depths("s110") and 'hard' not in HS.output_depths("s000")
    table = {"s000": (26, 1, 1), "s100": (27, 1, 1), "s010": (46, 2, 5), "s110": (47, 2, 5), "s011": (49, 2, 8), "s111": (50, 4, 8)}
    for name, (R, nc, no) in table.items():
        assert (HS.layout(name)[1], len(HS.corner_depths(name)), len(HS.output_depths(name))) == (R, nc, no)
    assert sum(HS.layout(n)[0] != {k: v for k, v in HS.CANON.items() if k in HS.layout(n)[0]} for n in HS.NEW_SETS) >= 1    # a permuted order
