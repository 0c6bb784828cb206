"""CPU checks of the target encoder's other settings (DATASETS.CONSIDER_OUTSIDE_OBJS, INPUT.ADJUST_BOUNDARY_HEATMAP,
INPUT.KEYPOINT_VISIBLE_MODIFY, INPUT.HEATMAP_CENTER, INPUT.TO_BGR): the restatement of tests/kitti_settings_common.py against
the reference's goldens, then the host build of monoflex_amd/csrc/kitti_encode_math.h with the settings against both, the
configuration mapping and its refusals, the layout of mfx_kitti_encode_cfg, and the dataset / loader front under the
config/defaults.py data settings with host encoders standing in for the two GPU launches.  No GPU work."""
import ctypes
import os
import random

import numpy as np
import pytest
import torch

from monoflex_amd import lib as L
from monoflex_amd import synthetic as S
from monoflex_amd.data import encode as E
from oracle import kitti_encode_ref as K
from tests import kitti_settings_common as C
from tests.kitti_common import NAMES, compare_fields, fuzz_sample, golden_sample

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
YAML = os.path.join(ROOT, "runs", "monoflex.yaml")
SETTING_NAMES = list(C.SETTINGS)
# a truncated object (centre left of the image) whose label box centre is outside the image as well: status 2 under the yaml
OUTSIDE_BOX_LINE = "Car 0.50 0 1.50 -300.00 150.00 -100.00 250.00 1.50 1.60 3.90 -12.00 1.65 8.00 0.10"


@pytest.fixture(scope="module")
def shim(tmp_path_factory):
    return C.build_cfg_shim(tmp_path_factory.mktemp("cfg_shim"))


@pytest.fixture(scope="module")
def plain_shim(tmp_path_factory):
    """The host build without settings (tests/shim/kitti_encode_host.cpp), which relies on encode_object's defaults."""
    import subprocess
    so = str(tmp_path_factory.mktemp("plain_shim") / "libkitti_shim.so")
    r = subprocess.run(["g++", "-O2", "-std=c++17", "-ffp-contract=off", "-shared", "-fPIC", "-o", so,
                        os.path.join(ROOT, "tests", "shim", "kitti_encode_host.cpp")], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    lib = ctypes.CDLL(so)
    lib.shim_kitti_encode.argtypes = [ctypes.POINTER(L.KittiDesc)]
    lib.shim_kitti_encode.restype = None
    return lib


def golden_batch():
    return [golden_sample(n)[:4] for n in NAMES]


# ---- the restatement is pinned to the reference first -----------------------------------------------------------------------
@pytest.mark.parametrize("setting", SETTING_NAMES)
def test_restatement_matches_the_reference_goldens(setting):
    kept, trunc = [], []
    for n in NAMES:
        assert not C.golden_raised(setting, n)
        lines, w, h, flip, _ = golden_sample(n)
        ref = C.golden_fields(setting, n)
        got = C.restated(setting, lines, w, h, flip)
        assert got is not None, n
        compare_fields(got, ref, "%s %s" % (setting, n))
        assert int(ref["reg_mask"].sum()) == int(got["reg_mask"].sum()) and int(ref["trunc_mask"].sum()) == int(got["trunc_mask"].sum())
        kept.append(int(ref["reg_mask"].sum())); trunc.append(int(ref["trunc_mask"].sum()))
    assert kept == C.KEPT[setting] and trunc == C.TRUNC[setting]


def test_restatement_fails_where_the_reference_does_under_the_refused_setting():
    raised = [n for n in NAMES if C.golden_raised(C.REFUSED, n)]
    assert len(raised) == 8 and all(str(C.GOLD_S["%s_%s_error" % (C.REFUSED, n)]).startswith("AssertionError") for n in raised)
    for n in NAMES:
        lines, w, h, flip, _ = golden_sample(n)
        if n in raised:
            with pytest.raises(AssertionError):
                C.encode_sample_cfg(lines, S.KITTI_P2, w, h, do_flip=flip, heatmap_center="2D")
        else:
            compare_fields(C.encode_sample_cfg(lines, S.KITTI_P2, w, h, do_flip=flip, heatmap_center="2D"), C.golden_fields(C.REFUSED, n), n)


def test_every_setting_changes_a_field_of_the_yaml_goldens():
    from tests.kitti_common import GOLD
    for setting in SETTING_NAMES:
        changed = {k for n in NAMES for k, v in C.golden_fields(setting, n).items() if not np.array_equal(v, GOLD[n + "_" + k])}
        assert changed, setting
        if setting == "circular":
            assert changed == {"hm"}
        if setting == "no_modify":
            assert changed == {"keypoints", "keypoints_depth_mask"}


def test_the_2d_centre_moves_targets_on_the_fuzz_seeds():
    """The fuzz comparison below can tell the '2D' centre from the '3D' one.  (That the centre is rounded in the dtype of the box
    is asserted inside encode_sample_cfg, and target_centers are compared exactly with the fixture above.)"""
    found = 0
    for seed in C.FUZZ_SEEDS:
        lines, w, h, flip = fuzz_sample(seed)
        a = C.restated("center2d_circular", lines, w, h, flip)
        b = C.restated("circular", lines, w, h, flip)
        if a is None or b is None:
            continue
        found += int((a["target_centers"] != b["target_centers"]).any())
    assert found > 0                                                 # the '2D' centre moves targets on these seeds at all


# ---- host build of the device functions -------------------------------------------------------------------------------------
@pytest.mark.parametrize("setting", SETTING_NAMES)
def test_shim_matches_the_reference_goldens(shim, setting):
    out = C.run_cfg_shim(shim, golden_batch(), C.params_of(setting))
    assert (out["status"] == 0).all()
    for b, n in enumerate(NAMES):
        compare_fields({k: v[b] for k, v in out.items()}, C.golden_fields(setting, n), "%s %s" % (setting, n))
    assert out["reg_mask"].sum(axis=1).tolist() == C.KEPT[setting] and out["trunc_mask"].sum(axis=1).tolist() == C.TRUNC[setting]


@pytest.mark.parametrize("setting", SETTING_NAMES)
def test_shim_matches_the_restatement_on_fuzzed_labels(shim, setting):
    samples = [fuzz_sample(s) for s in C.FUZZ_SEEDS]
    refs = [C.restated(setting, *s) for s in samples]
    out = C.run_cfg_shim(shim, samples, C.params_of(setting))
    compared = 0
    for b, ref in enumerate(refs):
        if ref is None:
            assert out["status"][b] != 0, b
            continue
        assert out["status"][b] == 0, b
        compare_fields({k: v[b] for k, v in out.items()}, ref, "%s fuzz%d" % (setting, C.FUZZ_SEEDS[b]))
        compared += 1
    assert 2 * compared >= len(samples)
    truncated = sum(int(r["trunc_mask"].sum()) for r in refs if r is not None)
    if setting in C.KEEPS_TRUNCATED:
        assert truncated >= 1
    else:
        assert truncated == 0 and compared == len(samples)           # nothing can raise once outside objects are skipped


def test_yaml_settings_through_the_new_path_are_byte_identical(shim, plain_shim):
    from tests.test_kitti_encode_host_shim import run_shim
    samples = golden_batch() + [fuzz_sample(s) for s in C.FUZZ_SEEDS[:12]]
    plain = run_shim(plain_shim, samples)
    for cfg in (None, E.EncodeParams().encode_cfg(), L.KittiEncodeCfg(1, 1, 1, 0)):
        got = C.run_cfg_shim(shim, samples, E.EncodeParams(), cfg=cfg)
        for k, v in plain.items():
            assert got[k].tobytes() == v.tobytes(), k
    assert E.EncodeParams().is_yaml() and not any(C.params_of(s).is_yaml() for s in SETTING_NAMES)


def test_status_bits_keep_their_meaning(shim):
    from tests.kitti_common import oracle_fields
    assert oracle_fields([OUTSIDE_BOX_LINE], 1242, 375, False) is None
    samples = [([OUTSIDE_BOX_LINE], 1242, 375, False), (golden_sample("s00")[0], 1242, 375, False)]
    yaml = C.run_cfg_shim(shim, samples, E.EncodeParams())
    assert yaml["status"].tolist() == [2, 0]
    skipped = C.run_cfg_shim(shim, samples, C.params_of("no_outside"))
    assert skipped["status"].tolist() == [0, 0] and skipped["reg_mask"][0].sum() == 0 and skipped["hm"][0].max() == 0
    moved = C.run_cfg_shim(shim, samples, C.params_of("center2d_circular"))
    assert moved["status"].tolist() == [2, 0] and moved["reg_mask"][0].sum() == 0
    # the refused combination, which only the C entry accepts: bit 8 exactly where the reference asserts
    out = C.run_cfg_shim(shim, golden_batch(), E.EncodeParams(), cfg=L.KittiEncodeCfg(1, 1, 1, 1))
    for b, n in enumerate(NAMES):
        if C.golden_raised(C.REFUSED, n):
            assert out["status"][b] == 8, n
        else:
            assert out["status"][b] == 0, n
            compare_fields({k: v[b] for k, v in out.items()}, C.golden_fields(C.REFUSED, n), n)
    off = C.run_cfg_shim(shim, golden_batch(), C.params_of("circular"))
    assert (off["status"] == 0).all() and (off["heat_radius"][..., 2][off["heat_radius"][..., 3] == 1] == 1).all()


def test_encode_cfg_layout_matches_the_c_struct(shim):
    assert ctypes.sizeof(L.KittiEncodeCfg) == shim.shim_sizeof_encode_cfg() == 16
    c = L.KittiEncodeCfg()
    shim.shim_fill_encode_cfg(ctypes.byref(c))
    assert (c.consider_outside_objs, c.adjust_boundary_heatmap, c.keypoint_visible_modify, c.heatmap_center_2d) == (1, 2, 3, 4)
    assert [n for n, _ in L.KittiEncodeCfg._fields_] == ["consider_outside_objs", "adjust_boundary_heatmap", "keypoint_visible_modify",
                                                         "heatmap_center_2d"]
    e = E.EncodeParams(consider_outside_objs=False, heatmap_center="2D").encode_cfg()
    assert (e.consider_outside_objs, e.adjust_boundary_heatmap, e.keypoint_visible_modify, e.heatmap_center_2d) == (0, 1, 1, 1)


# ---- configuration ------------------------------------------------------------------------------------------------------
def _params_tuple(p):
    return (p.consider_outside_objs, p.adjust_boundary_heatmap, p.keypoint_visible_modify, p.heatmap_center, p.to_bgr,
            p.filter_trunc, p.filter_size, p.edge_ratio, p.in_w, p.in_h, p.down, p.max_objs, p.num_classes)


def test_from_cfg_maps_the_settings():
    from monoflex_amd.config import get_cfg
    assert _params_tuple(E.EncodeParams.from_cfg(get_cfg(YAML))) == _params_tuple(E.EncodeParams())
    assert _params_tuple(E.EncodeParams())[:5] == (True, True, True, "3D", False)
    for setting in SETTING_NAMES:
        cfg = get_cfg(YAML)
        cfg.merge_from_list([str(v) for v in C.GOLD_S[setting + "_opts"]])      # the overrides the fixture was recorded with
        assert _params_tuple(E.EncodeParams.from_cfg(cfg)) == _params_tuple(C.params_of(setting)), setting
    cfg = get_cfg(YAML)
    cfg.merge_from_list(["INPUT.TO_BGR", "True"])
    assert E.EncodeParams.from_cfg(cfg).to_bgr is True and E.EncodeParams.from_cfg(cfg).is_yaml()
    # the project's defaults (= config/defaults.py of the reference) build once the orientation code is the multi-bin one
    cfg = get_cfg()
    cfg.merge_from_list(["INPUT.ORIENTATION", "multi-bin"])
    p = E.EncodeParams.from_cfg(cfg)
    assert (p.consider_outside_objs, p.adjust_boundary_heatmap, p.keypoint_visible_modify, p.heatmap_center) == (False, False, False, "3D")
    assert p.filter_trunc == -1.0


def test_from_cfg_refuses_what_the_reference_cannot_run():
    from monoflex_amd.config import get_cfg

    def refused(*opts):
        cfg = get_cfg(YAML)
        cfg.merge_from_list(list(opts))
        with pytest.raises(NotImplementedError) as e:
            E.EncodeParams.from_cfg(cfg)
        return str(e.value)
    msg = refused("INPUT.HEATMAP_CENTER", "2D")
    assert "HEATMAP_CENTER '2D'" in msg and "CONSIDER_OUTSIDE_OBJS" in msg and "ADJUST_BOUNDARY_HEATMAP" in msg and "assertion" in msg
    with pytest.raises(NotImplementedError):
        E.EncodeParams(heatmap_center="2D")
    msg = refused("INPUT.APPROX_3D_CENTER", "nearest")
    assert "APPROX_3D_CENTER" in msg and "the reference raises NotImplementedError" in msg
    msg = refused("INPUT.ORIENTATION", "head-axis")
    assert "head-axis" in msg and "three-wide" in msg
    msg = refused("INPUT.ORIENTATION_BIN_SIZE", "2")
    assert "ORIENTATION_BIN_SIZE != 4" in msg
    with pytest.raises(NotImplementedError):
        E.EncodeParams.from_cfg(get_cfg())                            # defaults as they are: 'head-axis'


# ---- frames ---------------------------------------------------------------------------------------------------------------
def test_shim_bgr_frames(shim):
    frames, flips = zip(*(C.golden_frame(n) for n in C.GOLD_S["bgr_cases"]))
    bgr = C.shim_frames(shim, frames, flips, True)
    rgb = C.shim_frames(shim, frames, flips, False)
    for b, n in enumerate(C.GOLD_S["bgr_cases"]):
        assert np.array_equal(bgr[b], C.bgr_frame(frames[b], flips[b])) and np.array_equal(rgb[b], K.transform_image(frames[b], do_flip=flips[b]))
        C.assert_bgr_frame_is_the_recorded_one(bgr[b], str(n))
        cs = C.GOLD_S["bgr_%s_img_sum" % n]
        x = bgr[b].astype(np.float64)
        np.testing.assert_allclose([x.sum(), np.abs(x).sum(), (x * x).sum()], cs, rtol=1e-9)


# ---- dataset and loader front under the defaults.py data settings ---------------------------------------------------------------
@pytest.fixture
def cpu_encoders(shim, monkeypatch):
    """Host stand-ins for the two GPU launches, called with the argument lists the dataset uses; both read their settings from `params`."""
    import monoflex_amd.data.datasets.kitti as DK

    def encode(records, Ps, sizes, flips, params, device, check=True):
        out = C.shim_encode_records(shim, records, Ps, sizes, flips, params)
        return {k: torch.from_numpy(v) for k, v in out.items()}

    def frames(fr, flips, params, device, mean, std):
        return torch.from_numpy(C.shim_frames(shim, fr, flips, params.to_bgr, params.in_w, params.in_h, mean, std))
    monkeypatch.setattr(DK, "encode_targets", encode)
    monkeypatch.setattr(DK, "preprocess_images", frames)


def test_dataset_and_loader_under_the_default_data_settings(tmp_path, cpu_encoders):
    from monoflex_amd.data import DeviceLoader, KITTIDataset
    from tests.kitti_right_common import GOLD_FIELDS, frame_pixels, left_frame_seed, make_kitti_dir
    sizes = [(1242, 375), (1224, 370), (1238, 374)]
    cases = [(S.synthetic_kitti_labels(60 + i, w, h, 9), w, h) for i, (w, h) in enumerate(sizes)]
    root = make_kitti_dir(tmp_path / "kitti", cases, right_images=False)
    cfg = C.defaults_cfg()
    cfg.merge_from_list(["INPUT.TO_BGR", "True"])
    ds = KITTIDataset(cfg, root, is_train=True, device="cpu")
    assert not ds.params.is_yaml() and ds.params.to_bgr and ds.params.filter_trunc == -1.0
    random.seed(2)
    batches = list(DeviceLoader(ds, batch_size=2, sampler=[2, 0, 1]))
    assert [b["img_ids"] for b in batches] == [("000002", "000000"), ("000001",)]
    flips, differs = set(), 0
    for batch in batches:
        for b, name in enumerate(batch["img_ids"]):
            i = int(name)
            w, h = sizes[i]
            flipped = bool(batch["fields"]["P"][b][0, 3] < 0)             # P2[0, 3] > 0; the flip negates it
            flips.add(flipped)
            ref = C.restated("defaults", cases[i][0], w, h, flipped)
            compare_fields({k: batch["targets"][b].get_field(k).numpy() for k in GOLD_FIELDS}, ref, name)
            yaml = K.encode_sample(cases[i][0], S.KITTI_P2, w, h, do_flip=flipped)
            differs += int(not np.array_equal(yaml["keypoints"], ref["keypoints"]) or not np.array_equal(yaml["reg_mask"], ref["reg_mask"]))
            assert np.array_equal(batch["images"].tensors[b].numpy(), C.bgr_frame(frame_pixels(left_frame_seed(i), w, h), flipped)), name
    assert differs > 0                                                  # these frames tell the default settings from the yaml's
    img, tgt, idx = KITTIDataset(cfg, root, is_train=True, augment=False, device="cpu")[1]
    assert idx == "000001" and np.array_equal(img.numpy(), C.bgr_frame(frame_pixels(left_frame_seed(1), *sizes[1]), False))
    compare_fields({k: tgt.get_field(k).numpy() for k in GOLD_FIELDS}, C.restated("defaults", cases[1][0], *sizes[1], False), "item")
