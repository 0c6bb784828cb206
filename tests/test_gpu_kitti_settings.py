"""GPU parity of the target encoder's other settings (mfx_kitti_encode_targets_cfg, mfx_kitti_preprocess_u8_bgr through the C ABI;
DATASETS.CONSIDER_OUTSIDE_OBJS, INPUT.ADJUST_BOUNDARY_HEATMAP, INPUT.KEYPOINT_VISIBLE_MODIFY, INPUT.HEATMAP_CENTER, INPUT.TO_BGR through
EncodeParams, the dataset and the loader) against the reference's goldens under each setting and the restatement of
tests/kitti_settings_common.py (itself pinned to those goldens on the CPU).  Rules of tests/kitti_common.py: integer / mask / index fields
identical, float fields to float32 round-off; frames exactly.  The loss comparison uses the bounds stated in
tests/test_gpu_object_loss_configs.py: terms 2e-5*max(1,|ref|), logged means 1e-4*max(1,|ref|), gradients 2e-5*max(1,max|ref|)."""
import ctypes
import os
import random

import numpy as np
import pytest
import torch

from monoflex_amd import lib as L
from monoflex_amd import synthetic as S
from monoflex_amd.data import encode as E
from monoflex_amd.data.datasets import kitti_utils as KU
from oracle import kitti_encode_ref as K
from tests import kitti_right_common as R
from tests import kitti_settings_common as C
from tests.kitti_common import NAMES, compare_fields, fuzz_sample, golden_sample

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SETTING_NAMES = list(C.SETTINGS)


def golden_batch():
    return [golden_sample(n)[:4] for n in NAMES]


def device_encode(samples, params, check=True, rights=None, Ps=None):
    out = E.encode_targets([KU.read_label_records(l, C.CLASSES) for l, _, _, _ in samples], Ps or [S.KITTI_P2] * len(samples),
                           [(w, h) for _, w, h, _ in samples], [f for _, _, _, f in samples], params, "cuda", check=check, rights=rights)
    return {k: v.cpu().numpy() for k, v in out.items()}


def entry_encode(samples, cfg, rights=None, Ps=None):
    """mfx_kitti_encode_targets_cfg called directly (cfg: None = NULL, or a KittiEncodeCfg) on a batch prepared with the yaml parameters."""
    recs = [KU.read_label_records(l, C.CLASSES) for l, _, _, _ in samples]
    p = E.PreparedEncode(recs, Ps or [S.KITTI_P2] * len(samples), [(w, h) for _, w, h, _ in samples], [f for _, _, _, f in samples],
                         E.EncodeParams(), torch.device("cuda"), rights)
    stream = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
    L.check(p.lib.mfx_kitti_encode_targets_cfg(ctypes.byref(p.desc), None if p.right is None else p.right.data_ptr(),
                                               None if cfg is None else ctypes.byref(cfg), stream), "mfx_kitti_encode_targets_cfg")
    return {k: v.cpu().numpy() for k, v in p.out.items()}


@pytest.mark.parametrize("setting", SETTING_NAMES)
def test_targets_match_the_reference_goldens(setting):
    out = device_encode(golden_batch(), C.params_of(setting))
    assert (out["status"] == 0).all()
    for b, n in enumerate(NAMES):
        compare_fields({k: v[b] for k, v in out.items()}, C.golden_fields(setting, n), "%s %s" % (setting, n))
    assert out["reg_mask"].sum(axis=1).tolist() == C.KEPT[setting] and out["trunc_mask"].sum(axis=1).tolist() == C.TRUNC[setting]


@pytest.mark.parametrize("setting", SETTING_NAMES)
def test_targets_match_the_restatement_on_fuzzed_labels(setting):
    samples = [fuzz_sample(s) for s in C.FUZZ_SEEDS]
    refs = [C.restated(setting, *s) for s in samples]
    out = device_encode(samples, C.params_of(setting), check=False)
    compared = 0
    for b, ref in enumerate(refs):
        if ref is None:
            assert out["status"][b] != 0, b
            continue
        assert out["status"][b] == 0, b
        compare_fields({k: v[b] for k, v in out.items()}, ref, "%s fuzz%d" % (setting, C.FUZZ_SEEDS[b]))
        compared += 1
    assert 2 * compared >= len(samples)
    if setting in C.KEEPS_TRUNCATED:
        assert sum(int(r["trunc_mask"].sum()) for r in refs if r is not None) >= 1


def test_null_and_yaml_cfg_are_byte_identical_to_the_plain_entry():
    samples = golden_batch() + [fuzz_sample(s) for s in C.FUZZ_SEEDS[:12]]
    plain = device_encode(samples, E.EncodeParams(), check=False)
    for cfg in (None, L.KittiEncodeCfg(1, 1, 1, 0)):
        got = entry_encode(samples, cfg)
        for k, v in plain.items():
            assert got[k].tobytes() == v.tobytes(), (k, cfg is None)
    assert plain["reg_mask"].sum() > 100 and plain["trunc_mask"].sum() > 10


def test_refused_setting_at_the_c_entry_flags_where_the_reference_asserts():
    with pytest.raises(NotImplementedError):
        E.EncodeParams(heatmap_center="2D")
    out = entry_encode(golden_batch(), L.KittiEncodeCfg(1, 1, 1, 1))
    raised = 0
    for b, n in enumerate(NAMES):
        if C.golden_raised(C.REFUSED, n):
            assert out["status"][b] & 8, n
            raised += 1
        else:
            assert out["status"][b] == 0, n
            compare_fields({k: v[b] for k, v in out.items()}, C.golden_fields(C.REFUSED, n), n)
    assert raised == 8


def test_mixed_views_without_outside_objects():
    """Left and right samples in one batch under CONSIDER_OUTSIDE_OBJS False: a row the yaml run keeps untruncated is the same bytes,
    a row the yaml run marks truncated is all zero."""
    samples = [golden_sample(n)[:4] for n in NAMES] + [R.golden_right_sample(n)[:4] for n in R.KEPT]
    rights = [0] * len(NAMES) + [1] * len(R.KEPT)
    order = np.random.RandomState(0).permutation(len(samples))
    samples, rights = [samples[i] for i in order], [rights[i] for i in order]
    Ps = R.view_matrices(rights, len(samples))
    yaml = device_encode(samples, E.EncodeParams(), rights=rights, Ps=Ps)
    got = device_encode(samples, C.params_of("no_outside"), rights=rights, Ps=Ps)
    assert (got["status"] == 0).all()
    trunc = yaml["trunc_mask"] == 1
    assert trunc[[b for b, r in enumerate(rights) if r]].sum() > 0 and trunc[[b for b, r in enumerate(rights) if not r]].sum() > 0
    for k in E.TARGET_FIELDS:
        if yaml[k].ndim < 2 or yaml[k].shape[1] != 40 or k == "heat_radius":
            continue                                                   # per-image fields; heat_radius is compared through hm below
        assert got[k][~trunc].tobytes() == yaml[k][~trunc].tobytes(), k
        assert not got[k][trunc].any(), k
    for k in ("pad_size", "edge_indices", "edge_len", "P"):
        assert got[k].tobytes() == yaml[k].tobytes(), k
    assert np.array_equal(got["heat_radius"][~trunc], yaml["heat_radius"][~trunc]) and not got["heat_radius"][trunc].any()
    for b in range(len(samples)):                                      # heat maps: identical where nothing was truncated, never larger
        if not trunc[b].any():
            assert got["hm"][b].tobytes() == yaml["hm"][b].tobytes(), b
        assert (got["hm"][b] <= yaml["hm"][b]).all()


def test_bgr_frames_are_the_permuted_reference_frames():
    names = [str(n) for n in C.GOLD_S["bgr_cases"]]
    frames, flips = zip(*(C.golden_frame(n) for n in names))
    bgr = E.preprocess_images(list(frames), list(flips), E.EncodeParams(to_bgr=True), "cuda").cpu().numpy()
    rgb = E.preprocess_images(list(frames), list(flips), E.EncodeParams(), "cuda").cpu().numpy()
    for b, n in enumerate(names):
        assert np.array_equal(bgr[b], K.transform_image(frames[b], do_flip=flips[b])[[2, 1, 0]]), n
        assert np.array_equal(rgb[b], K.transform_image(frames[b], do_flip=flips[b])), n
        C.assert_bgr_frame_is_the_recorded_one(bgr[b], n)


def test_raw_keypoint_visibility_targets_through_the_fused_loss():
    """The `no_modify` golden batch (raw per-keypoint visibility, depth masks from it) with fixed random predictions: the fused object loss,
    its logged means and its gradient against the tensor-op form in float64 on the CPU."""
    from monoflex_amd.config import get_cfg
    from monoflex_amd.data.datasets.kitti_utils import Calibration
    from monoflex_amd.engine.trainer import prepare_targets
    from monoflex_amd.model.head.detector_loss import make_loss_evaluator
    from monoflex_amd.structures.params_3d import ParamsList
    samples = golden_batch()
    recs = [KU.read_label_records(l, C.CLASSES) for l, _, _, _ in samples]
    fields = E.encode_targets(recs, [S.KITTI_P2] * len(samples), [(w, h) for _, w, h, _ in samples], [f for _, _, _, f in samples],
                              C.params_of("no_modify"), "cuda")
    yaml = device_encode(samples, E.EncodeParams())
    kp, dm = fields["keypoints"].cpu().numpy(), fields["keypoints_depth_mask"].cpu().numpy()
    assert (kp[..., 2] != yaml["keypoints"][..., 2]).sum() > 0 and (dm != yaml["keypoints_depth_mask"]).sum() > 0
    targets = []
    for _, w, h, flip in samples:
        t = ParamsList(image_size=(1280, 384), is_train=True)
        c = Calibration.from_matrix(S.KITTI_P2)
        t.add_field("calib", c.flipped(w) if flip else c)
        targets.append(t)

    def evaluator(fused):
        class _M:
            pass
        m = _M(); m.heads = _M()
        m.heads.loss_evaluator = make_loss_evaluator(get_cfg(os.path.join(ROOT, "runs", "monoflex.yaml")))
        m.heads.loss_evaluator.fused_object_loss, m.heads.loss_evaluator.log_as_float = fused, False
        return m
    B = len(samples)
    g = torch.Generator().manual_seed(0)
    cls = torch.rand(B, 3, 96, 320, generator=g).clamp(1e-4, 1 - 1e-4)
    reg = torch.randn(B, 50, 96, 320, generator=g) * 0.1
    m = evaluator(True)
    assert m.heads.loss_evaluator.fused_object_loss
    reg_d = reg.cuda().requires_grad_()
    got, got_logs = m.heads.loss_evaluator({"cls": cls.cuda(), "reg": reg_d}, prepare_targets(m, targets, "cuda", fields=fields))
    object_terms = [k for k in got if k != "hm_loss"]                  # the heat-map term is another kernel and reads no keypoint field
    sum(got[k] for k in object_terms).backward()
    m64 = evaluator(False)
    reg_r = reg.double().requires_grad_()
    ref, ref_logs = m64.heads.loss_evaluator({"cls": cls.double(), "reg": reg_r},
                                             prepare_targets(m64, targets, "cpu", fields={k: v.cpu() for k, v in fields.items()}))
    assert set(ref) == set(got) and "keypoint_loss" in object_terms and len(object_terms) >= 9
    sum(ref[k] for k in object_terms).backward()
    for k in object_terms:
        r, v = float(ref[k].detach()), float(got[k].detach())
        e = abs(v - r) / (2e-5 * max(1.0, abs(r)))
        print("term %-20s %.6f ref %.6f error/bound %.3f" % (k, v, r, e))
        assert e <= 1.0, k
    shared = [k for k in ref_logs if k in got_logs and k not in ("hm_loss",)]
    assert {"depth_MAE", "center_MAE", "02_MAE", "13_MAE"} <= set(shared)
    for k in shared:
        r = float(ref_logs[k])
        e = abs(float(got_logs[k]) - r) / (1e-4 * max(1.0, abs(r)))
        print("log  %-20s %.6f ref %.6f error/bound %.3f" % (k, float(got_logs[k]), r, e))
        assert e <= 1.0, k
    want = reg_r.grad
    err = float((reg_d.grad.cpu().double() - want).abs().max())
    print("gradient: max |ref| %.4f error/bound %.3f" % (float(want.abs().max()), err / (2e-5 * max(1.0, float(want.abs().max())))))
    assert float(want.abs().max()) > 0 and err <= 2e-5 * max(1.0, float(want.abs().max()))


def test_dataset_loader_and_a_training_step_under_the_default_data_settings(tmp_path):
    from monoflex_amd.data import DeviceLoader, KITTIDataset
    from monoflex_amd.model.detector import KeypointDetector
    sizes = [(1242, 375), (1224, 370), (1238, 374)]
    cases = [(S.synthetic_kitti_labels(60 + i, w, h, 9), w, h) for i, (w, h) in enumerate(sizes)]
    root = R.make_kitti_dir(tmp_path / "kitti", cases, right_images=False)
    cfg = C.defaults_cfg()
    cfg.MODEL.PRETRAIN = False
    ds = KITTIDataset(cfg, root, is_train=True)                         # flip coin live: p = 0.5
    assert len(ds) == 3 and not ds.params.is_yaml()
    random.seed(1)
    batches = list(DeviceLoader(ds, batch_size=3, sampler=[1, 2, 0]))
    assert len(batches) == 1 and batches[0]["img_ids"] == ("000001", "000002", "000000")
    batch = batches[0]
    differs = 0
    for b, name in enumerate(batch["img_ids"]):
        i = int(name)
        w, h = sizes[i]
        flipped = bool(batch["fields"]["P"][b][0, 3] < 0)               # P2[0, 3] > 0; the flip negates it
        frame = R.frame_pixels(R.left_frame_seed(i), w, h)
        assert np.array_equal(batch["images"].tensors[b].cpu().numpy(), K.transform_image(frame, do_flip=flipped)), name
        ref = C.restated("defaults", cases[i][0], w, h, flipped)
        compare_fields({k: batch["targets"][b].get_field(k).cpu().numpy() for k in R.GOLD_FIELDS}, ref, name)
        yaml = K.encode_sample(cases[i][0], S.KITTI_P2, w, h, do_flip=flipped)
        differs += int(not np.array_equal(yaml["keypoints"], ref["keypoints"]) or not np.array_equal(yaml["reg_mask"], ref["reg_mask"]))
    assert differs > 0
    torch.manual_seed(0)
    model = KeypointDetector(cfg).cuda().train()
    loss_dict, _ = model(batch["images"], list(batch["targets"]))
    total = sum(loss_dict.values())
    assert torch.isfinite(total) and float(total.detach()) > 0
    total.backward()
    g = model.backbone.base.base_layer[0].weight.grad
    assert g is not None and torch.isfinite(g).all() and float(g.abs().sum()) > 0
