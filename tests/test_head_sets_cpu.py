"""The reduced head sets of the reference's ablation ladder through every layer that needs no GPU.

Reference: the float64 restatement tests/head_sets_ref.py (anchored to the reference's own outputs by tests/test_head_sets_ref_cpu.py)
and the recorded reference outputs themselves (tests/golden/head_sets.npz).

* lib.HeadSet gives the channel table and R of every set, and what the set can serve.
* Host build of csrc/object_loss_math.h (tests/shim/head_sets_host.cpp) against the restatement for every set x corner depth mode: the
  ten terms, the logged means, each term's own gradient row (through the dual numbers); R channels inside a 64-wide row whose other
  entries hold junk that must not be read.  Project bounds: terms 2e-5 max(1,|ref|), logged 1e-4 max(1,|ref|), gradients
  1e-5 max(1,max|ref|).
* The argument check of mfx_object_loss (head_set_error): absent required key, key past R, cu without kp, unserviceable corner mode.
* Refusal matrix: every (set, CORNER_LOSS_DEPTH) and (set, OUTPUT_DEPTH) outside the table raises NotImplementedError at construction,
  as do the LOSS_NAMES the reference raises on, corner_uncertainty without corner_offset, a missing required key and an unknown key.
* LOSS_NAMES subsets give exactly the reference's dict keys; the tensor-op form (fused_object_loss False, CPU maps) reproduces the
  recorded reference values and gradients under every set x corner depth mode.
* A reduced-set model's state dict round-trips through utils/check_point.py.
"""
import ctypes
import os
import subprocess

import numpy as np
import pytest
import torch

from tests import head_sets_cases as HC
from tests import head_sets_ref as HS
from tests.head_sets_cases import compare_with_restatement, evaluator, small_case

ROOT = HC.ROOT


@pytest.fixture(scope="module")
def shim(tmp_path_factory):
    from monoflex_amd import lib as L
    so = str(tmp_path_factory.mktemp("shim") / "libhead_sets_shim.so")
    r = subprocess.run(["g++", "-O2", "-std=c++17", "-ffp-contract=off", "-shared", "-fPIC", "-o", so,
                        os.path.join(ROOT, "tests", "shim", "head_sets_host.cpp")], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    lib = ctypes.CDLL(so)
    lib.shim_object_loss_heads.argtypes = [ctypes.c_void_p] + [ctypes.c_int] * 5 + [ctypes.c_void_p, ctypes.c_int, ctypes.POINTER(L.ObjectLossCfg),
                                                                                    ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p]
    lib.shim_object_loss_heads.restype = ctypes.c_int
    lib.shim_head_set_error.argtypes = [ctypes.POINTER(L.ObjectLossCfg), ctypes.c_char_p]
    lib.shim_head_set_error.restype = ctypes.c_int
    return lib


# ---- the table ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", list(HS.SETS))
def test_head_set_table(name):
    from monoflex_amd import lib as L
    hs = L.HeadSet(HS.SETS[name], HS.channels(name))
    assert [hs.ch(k) for k in L.HEAD_KEYS] == HS.ch_table(name) and tuple(L.HEAD_KEYS) == HS.KEYS and hs.R == HS.WIDTHS[name]
    assert (hs.du, hs.kp, hs.cu) == HS.flags(name)
    assert set(hs.corner_depths()) == set(HS.corner_depths(name))
    assert set(hs.output_depths()) - {'oracle'} == set(HS.output_depths(name)) and ('oracle' in hs.output_depths()) == hs.cu
    for m in HS.output_depths(name):
        assert hs.has_depth_error(m) == HS.has_depth_error(name, m)
    lay = hs.layout()
    assert list(lay.ch) == HS.ch_table(name) and lay.reg_width == hs.R
    c = evaluator(name).object_loss_cfg()
    assert list(c.ch) == HS.ch_table(name) and c.reg_width == hs.R


# ---- kernel arithmetic, host build ---------------------------------------------------------------------------------------------------------
def run_shim(shim, ev, reg_set, tg, ld=64, ch_off=8, junk_seed=5):
    """reg_set (B, R, H, W) float32 in the set's layout -> (terms[10], logged[14], G (N,10,64), rows, touched[65]).  The R channels sit at
    [ch_off, ch_off + R) of an ld-wide row; everything else holds large junk."""
    from monoflex_amd import lib as L
    from monoflex_amd.structures.params_3d import make_train_target
    _, tv = ev.prepare_targets([make_train_target(t) for t in tg])
    rows = tv["object_rows"].contiguous()
    B, R, H, W = reg_set.shape
    reg = torch.randn(B, H, W, ld, generator=torch.Generator().manual_seed(junk_seed)) * 1e3 + 777.0
    reg[..., ch_off:ch_off + R] = reg_set.permute(0, 2, 3, 1)
    reg = reg.contiguous()
    N = rows.shape[0]
    vals, G = torch.zeros(L.OBJ_VALUES), torch.zeros(N, L.OBJ_TERMS, 64)
    touched = np.zeros(65, dtype=np.uint8)
    cfg = ev.object_loss_cfg()
    rc = shim.shim_object_loss_heads(reg.data_ptr(), B, H, W, ld, ch_off, rows.data_ptr(), N, ctypes.byref(cfg), vals.data_ptr(), G.data_ptr(),
                                     touched.ctypes.data)
    assert rc == 0
    return vals[:L.OBJ_TERMS], vals[L.OBJ_TERMS:], G, rows, touched


def gradients_at_objects(G, rows, ref, R, B, H, W):
    """G (N, 10, 64) -> each term's gradient summed per centre pixel, at the valid rows in the restatement's order: (10, n, R)."""
    dense = torch.zeros(G.shape[1], B, H, W, R)
    for n in torch.nonzero(rows[:, 0] != 0).flatten().tolist():
        dense[:, int(rows[n, 57]), int(rows[n, 3]), int(rows[n, 2])] += G[n, :, :R]
    return dense[:, ref.bi, ref.cen[:, 1], ref.cen[:, 0]]


@pytest.mark.parametrize("modify", [True, False])
@pytest.mark.parametrize("name,corner", HC.SET_MODES)
def test_kernel_math_vs_restatement(name, corner, modify, shim):
    tg, cls, reg, objs = HC.golden_input()
    reg_set = HS.take(reg, name, 1)
    ev = evaluator(name, corner=corner, modify=modify)
    terms, logged, G, rows, touched = run_shim(shim, ev, reg_set, tg)
    r = reg_set.double().requires_grad_()
    ref = HS.loss_ref(name, r, tg, HC.settings(corner, modify), *HS.loss_names(name))
    drop = HS.near_selection_rows(ref)
    assert int(drop.sum()) <= 0.05 * ref.n
    R = HS.WIDTHS[name]
    B, _, H, W = reg_set.shape
    grads = gradients_at_objects(G, rows, ref, R, B, H, W)
    compare_with_restatement("%s/%s/modify=%d shim" % (name, corner, modify), name, ref, HS.term_gradients(ref, r, HC.TERM_NAMES), terms, logged,
                             grads, 1e-5, drop)
    # lanes >= R carry nothing, empty rows carry nothing, and no channel outside the R of this set was read
    assert float(G[..., R:].abs().max()) == 0.0 and float(G[rows[:, 0] == 0].abs().max()) == 0.0
    assert not touched[R:].any() and touched[:R].all(), (name, np.nonzero(touched)[0])


def check_small_input(name, ref, plan, reg_set, tg):
    """What the small input is there for, asserted from the restatement and the inputs alone."""
    du, kp, cu = HS.flags(name)
    starts, R = HS.layout(name)
    objs = plan["objects"]
    pos = lambda o: objs.index(o)
    assert ref.n == len(objs) >= 8 and not np.asarray(tg[1]["reg_mask"]).any()                       # an image with no object
    assert all(bool(tg[b]["trunc_mask"][s]) for b, s in plan["trunc"]) and 0 < sum(int(t["trunc_mask"].sum()) for t in tg) < ref.n
    assert not bool(ref.m2d[pos(plan["zero_area"])]) and int(ref.m2d.sum()) == ref.n - 1             # a 2D box of zero area
    lo, hi = -10.0, 10.0
    raw = lambda key, o: ref.poi[pos(o), starts[key]:starts[key] + HS.WIDTH[key]].detach()
    for key in (['depth_uncertainty'] if du else []) + (['corner_uncertainty'] if cu else []):
        assert bool((raw(key, plan["unc_below"]) < lo).all()) and bool((raw(key, plan["unc_above"]) > hi).all())    # past both clamps
        assert bool((raw(key, plan["unc_on"][0]) == lo).all()) and bool((raw(key, plan["unc_on"][1]) == hi).all())  # and on them
    if kp:
        assert bool((~ref.kdm[pos(plan["invalid_all"])]).all()) and 0 < int(ref.kdm.sum()) < ref.kdm.numel()        # invalid keypoint groups
        assert int(((ref.kd > 0.1) & (ref.kd < 100.0)).sum()) >= 3 * (ref.n - 2)                                   # depths inside the range


@pytest.mark.parametrize("name,corner", HC.SET_MODES)
def test_small_device_input_on_the_host(name, corner, shim):
    """The input of tests/test_gpu_head_sets.py through the host build: it reaches the branches it is there for, at most 5 % of its valid rows
    sit near a selection (the seed is chosen here, on the CPU, from the restatement alone), and the kernel arithmetic meets the project's
    bounds on it before a GPU sees it."""
    for modify in (True, False):
        ev, tg, reg_set, ref, grads_ref, drop, plan = small_case(name, corner, modify)
        assert int(drop.sum()) <= 0.05 * ref.n, (name, corner, drop)
        check_small_input(name, ref, plan, reg_set, tg)
        terms, logged, G, rows, touched = run_shim(shim, ev, reg_set, tg)
        B, R, H, W = reg_set.shape
        compare_with_restatement("%s/%s/modify=%d small input, shim" % (name, corner, modify), name, ref, grads_ref, terms, logged,
                                 gradients_at_objects(G, rows, ref, R, B, H, W), 1e-5, drop)
        assert not touched[R:].any()


def test_kernel_math_without_objects(shim):
    from monoflex_amd import synthetic as S
    tg = [S.synthetic_train_target(9, n_obj=0)]
    reg = torch.randn(1, 50, 96, 320, generator=torch.Generator().manual_seed(1))
    for name in ("s000", "s011"):
        terms, logged, G, rows, _ = run_shim(shim, evaluator(name), HS.take(reg, name, 1), tg)
        assert float(terms.abs().max()) == 0 and float(logged.abs().max()) == 0 and float(G.abs().max()) == 0


def test_argument_check_of_the_kernel_entry(shim):
    """head_set_error (what mfx_object_loss returns MFX_ERR_ARG on), on the host."""
    from monoflex_amd import lib as L
    why = ctypes.create_string_buffer(160)

    def err(name, corner="direct", **edit):
        c = L.ObjectLossCfg.from_buffer_copy(evaluator(name, corner=corner if corner in HS.corner_depths(name) else "direct").object_loss_cfg())
        c.corner_depth_mode = HS.CORNER_DEPTHS.index(corner)
        for k, v in edit.items():
            if k.startswith("ch"):
                c.ch[int(k[2:])] = v
            else:
                setattr(c, k, v)
        return shim.shim_head_set_error(ctypes.byref(c), why), why.value.decode()

    for name in HS.SETS:
        for corner in HS.CORNER_DEPTHS:
            rc, msg = err(name, corner)
            assert rc == (0 if corner in HS.corner_depths(name) else 1), (name, corner, msg)
    for i in (0, 1, 4, 5, 6, 7):                                       # an absent required key
        rc, msg = err("s111", **{"ch%d" % i: -1})
        assert rc == 1 and "required" in msg, (i, msg)
    assert err("s111", ch8=-2)[0] == 1                                  # only -1 marks an absent key
    assert err("s111", reg_width=0)[0] == 0 and err("s111", reg_width=49)[0] == 1 and err("s111", reg_width=51)[0] == 1
    assert err("s000", ch7=26)[0] == 1 and err("s000", ch0=23)[0] == 1 and err("s000", ch0=22)[0] == 0      # ch >= R; the key's last channel past R
    assert err("s011", ch2=-1)[0] == 1                                  # corner_uncertainty without corner_offset
    assert err("s111", corner_depth_mode=4)[0] == 1


# ---- refusals ----------------------------------------------------------------------------------------------------------------------------
def test_refusal_matrix_of_the_loss_evaluator():
    refused = 0
    for name in HS.SETS:
        for corner in HS.CORNER_DEPTHS:
            if corner in HS.corner_depths(name):
                evaluator(name, corner=corner)
            else:
                with pytest.raises(NotImplementedError, match=corner):
                    evaluator(name, corner=corner)
                refused += 1
    assert refused == 3 + 3 + 2 + 2 + 2


def test_refusal_matrix_of_the_post_processor():
    from monoflex_amd.model.head.detector_infer import make_post_processor
    refused = 0
    for name in HS.SETS:
        for mode in HS.OUTPUT_DEPTHS + ('oracle',):
            ok = mode in HS.output_depths(name) or (mode == 'oracle' and HS.flags(name)[2])
            cfg = HC.cfg_for(name, extra=[HC.HEAD + "OUTPUT_DEPTH", mode])
            if ok:
                pp = make_post_processor(cfg)
                assert pp.reg_width == HS.WIDTHS[name] and list(pp.head_layout.ch) == HS.ch_table(name)
            else:
                with pytest.raises(NotImplementedError, match=mode):
                    make_post_processor(cfg)
                refused += 1
    assert refused == 8 + 8 + 4 + 4


def _with(name, add=(), remove=()):
    nm, w = HS.loss_names(name)
    nm, w = list(nm) + list(add), list(w) + [HS.LOSS_WEIGHTS[a] for a in add]
    keep = [i for i, n in enumerate(nm) if n not in remove]
    return [nm[i] for i in keep], [w[i] for i in keep]


@pytest.mark.parametrize("name,add,remove,word", [
    ("s100", ('keypoint_depth_loss',), (), "keypoint_depth_loss"), ("s000", ('keypoint_loss',), (), "keypoint_loss"),
    ("s010", ('weighted_avg_depth_loss',), (), "weighted_avg_depth_loss"), ("s110", (), ('keypoint_loss',), "keypoint_loss"),
    ("s111", (), ('keypoint_loss',), "keypoint_loss"), ("s000", (), ('depth_loss',), "depth_loss"), ("s011", (), ('dims_loss',), "dims_loss")])
def test_refused_loss_names(name, add, remove, word):
    with pytest.raises(NotImplementedError, match=word):
        evaluator(name, names=_with(name, add, remove))


def test_refused_head_lists():
    from monoflex_amd import lib as L
    for heads, chans, word in (([['2d_dim'], ['3d_offset'], ['3d_dim'], ['ori_cls', 'ori_offset']], [[4], [2], [3], [8, 8]], "depth"),
                               ([['depth'], ['corner_uncertainty'], ['2d_dim'], ['3d_offset'], ['3d_dim'], ['ori_cls', 'ori_offset']],
                                [[1], [3], [4], [2], [3], [8, 8]], "corner_uncertainty without corner_offset"),
                               (HS.SETS["s000"] + [['3d_yaw']], HS.channels("s000") + [[1]], "3d_yaw"),
                               (HS.SETS["s000"], [[1], [4], [2], [3], [8, 4]], "ori_offset"),
                               (HS.SETS["s000"] + [['depth']], HS.channels("s000") + [[1]], "repeated")):
        with pytest.raises(NotImplementedError, match=word):
            L.HeadSet(heads, chans)


def test_refusals_cover_what_the_reference_raised_on():
    """Each recorded combination the reference itself raises on is refused here at construction."""
    from monoflex_amd.model.head.detector_infer import make_post_processor
    g = HC.golden()
    assert len(g["raises/labels"]) == 9
    for build in (lambda: evaluator("s000", corner="keypoint_mean"), lambda: evaluator("s011", corner="soft_combine"),
                  lambda: evaluator("s110", corner="hard_combine"), lambda: evaluator("s100", names=_with("s100", ('keypoint_depth_loss',))),
                  lambda: evaluator("s010", names=_with("s010", ('weighted_avg_depth_loss',))), lambda: evaluator("s110", names=_with("s110", (), ('keypoint_loss',))),
                  lambda: make_post_processor(HC.cfg_for("s100", extra=[HC.HEAD + "OUTPUT_DEPTH", "keypoints_avg"])),
                  lambda: make_post_processor(HC.cfg_for("s110", extra=[HC.HEAD + "OUTPUT_DEPTH", "soft"])),
                  lambda: make_post_processor(HC.cfg_for("s000", extra=[HC.HEAD + "OUTPUT_DEPTH", "hard"]))):
        with pytest.raises(NotImplementedError):
            build()


# ---- the tensor-op form against the recorded reference -------------------------------------------------------------------------------------
LOSS_TAGS = [(n, m, m, True) for n in HS.NEW_SETS for m in HS.corner_depths(n)] + [(n, "names", "direct", True) for n in HS.NEW_SETS] + \
    [("s010", "direct_no_modify", "direct", False)]


@pytest.mark.parametrize("name,tag,corner,modify", LOSS_TAGS, ids=["%s-%s" % t[:2] for t in LOSS_TAGS])
def test_tensor_op_form_reproduces_the_reference(name, tag, corner, modify):
    """Loss_Computation with fused_object_loss False on CPU maps: the dict keys ARE the reference's (an absent name is absent, not zero),
    values and the gradient of the summed loss within the bounds of tests/test_loss_golden.py."""
    from monoflex_amd.structures.params_3d import make_train_target
    g = HC.golden()
    key = "%s/%s" % (name, tag)
    drop = tuple(str(x) for x in g[name + "/names/dropped"]) if tag == "names" else ()
    ev = evaluator(name, corner=corner, modify=modify, names=HS.loss_names(name, drop))
    ev.fused_object_loss = False
    tg, cls, reg, objs = HC.golden_input()
    r = HS.take(reg, name, 1).clone().requires_grad_()
    loss_dict, logs = ev({"cls": cls.clone(), "reg": r}, [make_train_target(t) for t in tg])
    loss_keys, log_keys = [str(k) for k in g[key + "/loss_keys"]], [str(k) for k in g[key + "/log_keys"]]
    assert list(loss_dict) == loss_keys, (list(loss_dict), loss_keys)                 # the reference's names in the reference's order
    assert set(logs) == set(log_keys) and all(isinstance(v, float) for v in logs.values())
    for k, v in zip(loss_keys, g[key + "/loss_values"]):
        assert abs(float(loss_dict[k].detach()) - v) <= 2e-5 * max(1.0, abs(v)), (k, float(loss_dict[k].detach()), v)
    for k, v in zip(log_keys, g[key + "/log_values"]):
        if k != '3D_IoU':                                                             # (recorded as 0: shapely is absent in the recorder)
            assert abs(logs[k] - v) <= 1e-4 * max(1.0, abs(v)), (k, logs[k], v)
    sum(loss_dict.values()).backward()
    want = g[key + "/grad_reg_at_objects"]
    b = torch.tensor([o[0] for o in objs])
    cen = torch.stack([torch.as_tensor(tg[i]["target_centers"][j]) for i, j in objs]).long()
    got = r.grad.permute(0, 2, 3, 1)[b, cen[:, 1], cen[:, 0]].numpy()
    assert np.abs(got - want).max() <= 1e-5 * max(1.0, np.abs(want).max())
    assert abs(float(r.grad.abs().double().sum()) - float(g[key + "/grad_reg_abssum"])) <= 1e-4 * float(g[key + "/grad_reg_abssum"])


def test_full_set_dict_keys_are_unchanged():
    from monoflex_amd.structures.params_3d import make_train_target
    ev = evaluator("s111", corner="soft_combine")
    ev.fused_object_loss = False
    tg, cls, reg, _ = HC.golden_input()
    loss_dict, logs = ev({"cls": cls, "reg": reg}, [make_train_target(t) for t in tg])
    assert set(loss_dict) == set(HS.LOSS_NAMES) and set(logs) == HS.expected_log_keys("s111", HS.LOSS_NAMES)


# ---- the model -----------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["s000", "s011"])
def test_reduced_set_model_builds_and_round_trips_its_state(name, tmp_path):
    """KeypointDetector with a reduced head set: the predictor's modules follow the configured branches, and utils/check_point.py saves and
    loads them by those names."""
    from monoflex_amd.model.detector import KeypointDetector
    from monoflex_amd.utils.check_point import DetectronCheckpointer
    cfg = HC.model_cfg(name)
    torch.manual_seed(3)
    model = KeypointDetector(cfg)
    pr = model.heads.predictor
    assert pr.reg_width == HS.WIDTHS[name] and len(pr.reg_heads) == len(HS.SETS[name])
    assert [[h.weight.shape[0] for h in heads] for heads in pr.reg_heads] == HS.channels(name)
    ck = DetectronCheckpointer(cfg, model, save_dir=str(tmp_path))
    ck.save("head_set")
    torch.manual_seed(4)
    other = KeypointDetector(cfg)
    assert any(not torch.equal(a, b) for a, b in zip(model.state_dict().values(), other.state_dict().values()))
    DetectronCheckpointer(cfg, other, save_dir=str(tmp_path)).load(os.path.join(str(tmp_path), "head_set.pth"), use_latest=False)
    for (k, a), (k2, b) in zip(model.state_dict().items(), other.state_dict().items()):
        assert k == k2 and torch.equal(a, b), k
