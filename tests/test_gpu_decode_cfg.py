"""Device tests of the configurable box decode (decode.hip `decode_boxes_kernel` with a `mfx_decode_cfg`, through ops.decode_boxes(cfg=...),
PostProcessor and KeypointDetector) against its float64 restatement (tests/decode_cfg_ref.py) on the structured inputs of
tests/decode_cases.py, under the seven head settings of decode_cfg_ref.SETTINGS: the config defaults (exp depth, linear dimensions, raw
score) and the same with DIMENSION_STD, linear depth, exp dimensions with std, linear dimensions, one class and two classes with custom
statistics and DEPTH_RANGE [1, 60].

Compared: all K rows of every image, all 14 columns, error = |got - want| / max(1, |want|) per column; `topk` and `valid` EQUAL the
restatement; `unc` = [sigma, 1 - clamp(sigma, 0.01, 1)] within the score column's bound, and exactly zero -- with the score column exactly
topk's score -- where the confidence scaling is off.  Near-decision rows as in tests/test_gpu_decode_boxes.py.

Bound: 4x the per-column error of the float32 reference arithmetic under the same setting (decode_cfg_ref.YARDSTICK, measured by
tests/test_decode_cfg_ref_cpu.py from the reference's recorded PostProcessor rows and a float32 torch evaluation on every pixel of these maps).

Per column, over the settings (every case of this module; first MI355X run):
column   float32 reference (worst setting)   bound of the tightest setting   kernel, worst of all cases
cls      0.00e+00                            0.00e+00                        0.00e+00
alpha    5.12e-07                            1.78e-06                        4.45e-07
x1       9.54e-07                            3.82e-06                        6.45e-07
y1       4.77e-07                            1.91e-06                        2.68e-07
x2       9.54e-07                            3.82e-06                        9.54e-07
y2       4.77e-07                            1.91e-06                        4.77e-07
h        1.26e-07                            2.97e-07                        1.15e-07
w        1.49e-07                            2.73e-07                        1.22e-07
l        1.26e-07                            3.01e-07                        1.12e-07
X        2.91e-06                            5.08e-06                        2.18e-06
Y        1.26e-06                            2.92e-06                        1.06e-06
Z        2.00e-06                            1.10e-06                        1.15e-06
ry       1.74e-06                            2.74e-06                        9.95e-07
score    1.41e-07                            0.00e+00                        1.07e-07
(The columns mix settings: Z's 1.15e-06 is the linear depth of b_linear_depth, whose own bound is 8.00e-06; the score column's bound of 0 belongs
to the settings without confidence scaling, where the kernel's score error is 0.)  Per setting, the kernel's worst against that setting's own
yardstick (decode_cfg_ref.YARDSTICK; the bound is 4x it):
setting          alpha     x1        y1        x2        y2        h         w         l         X         Y         Z         ry        score
a_defaults       4.45e-07  6.45e-07  2.68e-07  9.54e-07  4.77e-07  8.09e-08  7.25e-08  6.79e-08  2.18e-06  1.01e-06  2.60e-07  5.81e-07  0
a_linear_std     4.45e-07  6.45e-07  2.68e-07  9.54e-07  4.77e-07  6.86e-08  5.96e-08  7.48e-08  1.37e-06  9.15e-07  2.37e-07  6.67e-07  0
b_linear_depth   4.45e-07  6.45e-07  2.68e-07  9.54e-07  4.77e-07  1.15e-07  1.22e-07  1.12e-07  1.37e-06  8.80e-07  1.15e-06  9.95e-07  1.07e-07
c_exp_dims_std   4.45e-07  6.45e-07  2.68e-07  9.54e-07  4.77e-07  8.58e-08  1.04e-07  7.64e-08  1.71e-06  1.04e-06  2.52e-07  6.85e-07  1.07e-07
d_linear_dims    4.45e-07  6.45e-07  2.68e-07  9.54e-07  4.77e-07  8.00e-08  7.25e-08  6.79e-08  1.71e-06  1.06e-06  2.89e-07  5.58e-07  1.07e-07
e_car            4.40e-07  6.30e-07  2.68e-07  9.54e-07  4.77e-07  7.72e-08  8.32e-08  8.10e-08  1.12e-06  6.03e-07  9.92e-07  5.89e-07  7.84e-08
e_two_classes    4.40e-07  6.45e-07  2.68e-07  9.54e-07  4.77e-07  8.82e-08  8.80e-08  9.74e-08  1.01e-06  7.83e-07  2.44e-07  5.35e-07  0
yaml             4.45e-07  4.49e-07  2.38e-07  3.88e-07  4.77e-07  9.70e-08  1.09e-07  9.77e-08  1.24e-06  5.40e-07  2.38e-07  6.49e-07  7.96e-08
The kernel stays within about 1x the float32 reference's own error in every column of every setting (worst ratio 1.05, X of a_defaults).
"""
import ctypes
import functools
import os

import numpy as np
import pytest
import torch

from tests import decode_cases as C
from tests import decode_cfg_ref as DC
from tests import decode_ref as D

pytestmark = pytest.mark.gpu
DEV = "cuda"
SETTINGS = list(DC.SETTINGS)
WORST = {}                                                  # setting -> worst per-column error of the cases run so far (printed by the last test)


def _lib_cfg(s, mode="soft"):
    """lib.DecodeCfg of a decode_cfg_ref setting, built the way PostProcessor builds its own (lib.decode_cfg)."""
    from monoflex_amd import lib as L
    head = dict(depth_mode=s["depth_mode"], depth_range=tuple(s["depth_range"]), depth_ref=tuple(s["depth_ref"]), dim_mean=s["dim_mean"],
                dim_std=s["dim_std"], dim_modes=["exp" if s["dim_exp"] else "linear", True, bool(s["dim_use_std"])], down_ratio=4, eps=1e-3)
    return L.decode_cfg(head, s["uncertainty_as_conf"], mode)


@functools.lru_cache(maxsize=None)
def _case(name, setting, kind="distinct"):
    d = DC.case_inputs(name, setting, kind)
    for a in d.values():
        if isinstance(a, np.ndarray):
            a.setflags(write=False)
    return d


@functools.lru_cache(maxsize=None)
def _ref(name, setting, mode, kind="distinct"):
    return DC.run_ref(_case(name, setting, kind), mode, setting)


def _device_inputs(d):
    t = lambda a, dt: torch.from_numpy(np.array(a)).to(DEV, dt)
    return (t(d["hmap"], torch.float32), d["reg_off"], t(d["scores"], torch.float32), t(d["index"], torch.int32), t(d["calib"], torch.float32),
            t(d["pad"], torch.int32), t(d["img_size"], torch.int32), float(d["threshold"]))


def _run(d, mode, s):
    from monoflex_amd import ops
    out = ops.decode_boxes(*_device_inputs(d), depth_mode=mode, cfg=_lib_cfg(s), return_unc=True)
    torch.cuda.synchronize()
    return [t.cpu().numpy() for t in out]


def _compare(what, got, ref, mode, setting, s=None):
    s = DC.SETTINGS[setting] if s is None else s
    det, topk, valid, unc = got
    assert np.isfinite(det).all() and np.isfinite(unc).all(), what
    assert np.array_equal(topk.astype(np.float64), ref["topk"]), what + ": topk differs from the restatement"
    assert np.array_equal(valid, ref["valid"]), what + ": valid differs from the restatement"
    assert float(D.near_rows(ref, mode).mean()) <= D.NEAR_CAP, what
    err = D.column_errors(det, ref, mode)
    uerr = DC.unc_errors(unc, ref)
    print("%-44s %s  sigma %.2e  conf %.2e" % (what, D.format_errors(err), uerr[0], uerr[1]))
    WORST[setting] = np.maximum(WORST.get(setting, np.zeros(14)), err)
    bound = DC.bounds(setting)
    assert (err <= bound).all(), "%s: column(s) %s past 4x the float32 reference's error: %s" % (
        what, [D.COLUMNS[i] for i in np.nonzero(err > bound)[0]], D.format_errors(err))
    if s["uncertainty_as_conf"]:
        assert (uerr <= bound[13]).all(), "%s: unc [sigma, conf] errors %s past the score column's bound %.2e" % (what, uerr, bound[13])
    else:
        assert (unc == 0).all() and np.array_equal(det[..., 13], topk[..., 0]), what + ": confidence scaling is off"


def _check_case(name, setting, mode, kind="distinct"):
    _compare("%s %s %s %s" % (setting, name, kind, mode), _run(_case(name, setting, kind), mode, DC.SETTINGS[setting]), _ref(name, setting, mode, kind),
             mode, setting)


@pytest.mark.parametrize("mode", DC.GOLDEN_MODES)
@pytest.mark.parametrize("setting", SETTINGS)
def test_settings_and_depth_modes(setting, mode):
    """B = 3, K = 50, ld 64, reg_off 8: three images with their own pad, size and calibration; 3, 1 and 2 classes."""
    _check_case("b3_k50", setting, mode)


@pytest.mark.parametrize("name", ["k1", "k7", "k256"])
@pytest.mark.parametrize("setting", SETTINGS)
def test_k_from_1_to_256(setting, name):
    _check_case(name, setting, "soft")
    _check_case(name, setting, "direct")


@pytest.mark.parametrize("name", ["ld50", "ld72"])
@pytest.mark.parametrize("setting", SETTINGS)
def test_row_layouts(setting, name):
    """(ld, reg_off) = (50, 0) and (72, 13) ((64, 8) is b3_k50); the channels outside the 50 regression values hold noise."""
    c = C.CASES[name]
    assert (c["ld"], c["reg_off"]) == {"ld50": (50, 0), "ld72": (72, 13)}[name]
    _check_case(name, setting, "hard")


@pytest.mark.parametrize("setting", ["a_defaults", "e_car", "e_two_classes"])
def test_ties_and_threshold(setting):
    """Equal scores across the classes, and scores at / one ulp around the threshold: topk and valid EQUAL the restatement with 1, 2 and 3 classes."""
    for kind in ("ties", "threshold"):
        _check_case("b3_k50", setting, "soft", kind)


@pytest.mark.parametrize("mode", D.MODES)
def test_default_cfg_is_bitwise_the_built_in_decode(mode):
    """mfx_decode_boxes_cfg with the runs/monoflex.yaml values IS mfx_decode_boxes_mode, for all eight output_depth modes."""
    from monoflex_amd import ops
    d = C.case_inputs("b3_k50", "ties")
    args = _device_inputs(d)
    old = ops.decode_boxes(*args, depth_mode=mode)
    new = ops.decode_boxes(*args, depth_mode=mode, cfg=_lib_cfg(DC.YAML), return_unc=True)
    torch.cuda.synchronize()
    assert all(torch.equal(a, b) for a, b in zip(old, new[:3]))
    ref = DC.run_ref(d, mode, DC.YAML)
    _compare("yaml cfg b3_k50 ties %s" % mode, [t.cpu().numpy() for t in new], ref, mode, "yaml", s=DC.YAML)


def test_argument_validation():
    """Every MFX_ERR_ARG case returns -1 with its message and launches nothing."""
    from monoflex_amd import lib as L
    lib = L.load()
    d = _case("k7", "a_defaults")
    hm, reg_off, sc, ix, calib, pad, size, thr = _device_inputs(d)
    B, H, W, ld = hm.shape
    K = sc.shape[2]
    det, topk = torch.zeros(B, K, 14, device=DEV), torch.zeros(B, K, 5, device=DEV)
    valid = torch.zeros(B, K, dtype=torch.int32, device=DEV)
    p = lambda t: ctypes.c_void_p(t.data_ptr())

    def call(cfg, ncls=3, K=K):
        ref = ctypes.byref(cfg) if cfg is not None else None
        return lib.mfx_decode_boxes_cfg(p(hm), ld, reg_off, p(sc), p(ix), ncls, B, H, W, K, p(calib), p(pad), p(size), ctypes.c_float(thr), ref,
                                        p(det), p(topk), p(valid), None, None)

    def cfg(**kw):
        c = _lib_cfg(DC.SETTINGS["a_defaults"])
        for k, v in kw.items():
            if isinstance(v, tuple):
                getattr(c, k)[0], getattr(c, k)[1] = v
            else:
                setattr(c, k, v)
        return c
    cases = [(dict(cfg=None), b"null cfg"), (dict(cfg=cfg(depth_decode=3)), b"depth_decode"), (dict(cfg=cfg(depth_decode=-1)), b"depth_decode"),
             (dict(cfg=cfg(output_depth=8)), b"output_depth"), (dict(cfg=cfg(output_depth=-1)), b"output_depth"),
             (dict(cfg=cfg(depth_range=(2.0, 1.0))), b"depth_range"), (dict(cfg=cfg(depth_range=(0.1, float("inf")))), b"depth_range"),
             (dict(cfg=cfg(depth_range=(float("nan"), 100.0))), b"depth_range"),
             (dict(cfg=cfg(), ncls=4), b"ncls"), (dict(cfg=cfg(), ncls=0), b"ncls"), (dict(cfg=cfg(), K=257), b"K <= 256")]
    for kw, msg in cases:
        assert call(**kw) == -1 and msg in lib.mfx_last_error(), (kw, lib.mfx_last_error())
    torch.cuda.synchronize()
    assert not det.any() and not topk.any() and not valid.any()
    assert call(cfg()) == 0
    torch.cuda.synchronize()
    assert valid.any()


def test_graph_replay_is_bitwise_the_eager_call():
    from monoflex_amd import ops
    setting, mode = "e_two_classes", "hard"
    args = _device_inputs(_case("b3_k50", setting, "ties"))
    cfg = _lib_cfg(DC.SETTINGS[setting])
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        eager = [t.clone() for t in ops.decode_boxes(*args, depth_mode=mode, cfg=cfg, return_unc=True)]
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        held = ops.decode_boxes(*args, depth_mode=mode, cfg=cfg, return_unc=True)
    cfg.depth_decode = 2                                      # the launch holds a copy: the caller's struct may change or go away
    for t in held:
        t.zero_()
    graph.replay()
    torch.cuda.synchronize()
    assert all(torch.equal(a, b) for a, b in zip(held, eager))
    _compare("graph replay %s b3_k50 ties %s" % (setting, mode), [t.cpu().numpy() for t in held], _ref("b3_k50", setting, mode, "ties"), mode, setting)


# ---- through the configuration --------------------------------------------------------------------------------------------------------------
YAML_FILE = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "runs", "monoflex.yaml")


def _defaults_cfg():
    """monoflex_amd/config.py's defaults WITHOUT the yaml; only what the decode kernel's layout needs is set: the nine regression heads and
    multi-bin orientation (the defaults' five heads and head-axis orientation stay refused).  DEPTH_MODE exp, DIMENSION_REG
    ['linear', True, False], UNCERTAINTY_AS_CONFIDENCE False, OUTPUT_DEPTH direct and threshold 0.1 are the defaults' own."""
    from monoflex_amd.config import get_cfg
    cfg = get_cfg(None, [])
    cfg.MODEL.HEAD.REGRESSION_HEADS = [['2d_dim'], ['3d_offset'], ['corner_offset'], ['corner_uncertainty'], ['3d_dim'], ['ori_cls', 'ori_offset'],
                                       ['depth'], ['depth_uncertainty']]
    cfg.MODEL.HEAD.REGRESSION_CHANNELS = [[4], [2], [20], [3], [3], [8, 8], [1], [1]]
    cfg.INPUT.ORIENTATION = 'multi-bin'
    return cfg


def _car_cfg():
    from monoflex_amd.config import get_cfg
    cfg = get_cfg(YAML_FILE, [])
    cfg.DATASETS.DETECT_CLASSES = ("Car",)
    return cfg


def _setting_of(cfg):
    """The decode_cfg_ref setting a configuration asks for, read from the configuration itself (not from the post-processor under test)."""
    H = cfg.MODEL.HEAD
    return dict(depth_mode=H.DEPTH_MODE, depth_ref=tuple(H.DEPTH_REFERENCE), depth_range=tuple(H.DEPTH_RANGE), dim_exp=H.DIMENSION_REG[0] == 'exp',
                dim_use_std=bool(H.DIMENSION_REG[2]), uncertainty_as_conf=bool(cfg.TEST.UNCERTAINTY_AS_CONFIDENCE), dim_mean=H.DIMENSION_MEAN,
                dim_std=H.DIMENSION_STD, ncls=len(cfg.DATASETS.DETECT_CLASSES))


def _peak_map(ncls, lo_hi):
    """A structured map (B = 3, ld 64, reg_off 8) whose first ncls channels carry isolated class peaks, 50 per class, all scores of an image
    distinct, part of each image's best 50 below the threshold; the channels up to the regression rows hold noise."""
    m = C.structured_maps(61, (1, 2, 0))
    scores, index = C.peak_lists(62, 3, 50, [lo_hi] * 3)
    hmap = m["hmap"].copy()
    hmap[..., :ncls] = C.peak_logits(scores, index)[..., :ncls]
    return dict(m, hmap=hmap), scores[:, :ncls], index[:, :ncls]


@pytest.mark.parametrize("which", ["defaults", "car"])
def test_post_processor_under_other_settings(which):
    """make_post_processor(cfg) built from the config defaults without the yaml, and with DETECT_CLASSES ("Car",): per image the rows that
    pass the threshold, in order, and the eval_utils fields of the reference's dict."""
    from monoflex_amd import ops
    from monoflex_amd.model.head.detector_infer import make_post_processor
    from monoflex_amd.structures.params_3d import Calibration, ParamsList
    cfg = _defaults_cfg() if which == "defaults" else _car_cfg()
    s = _setting_of(cfg)
    assert (s["depth_mode"], s["dim_exp"], s["dim_use_std"], s["uncertainty_as_conf"], s["ncls"]) == \
        {"defaults": ("exp", False, False, False, 3), "car": ("inv_sigmoid", True, False, True, 1)}[which]
    post = make_post_processor(cfg)
    mode, thr = cfg.MODEL.HEAD.OUTPUT_DEPTH, float(cfg.TEST.DETECTIONS_THRESHOLD)
    assert mode == {"defaults": "direct", "car": "soft"}[which] and thr == {"defaults": 0.1, "car": 0.2}[which] and post.max_detection == 50
    m, scores, index = _peak_map(s["ncls"], (0.02, thr * 1.3))
    targets = []
    for i in m["images"]:
        t = ParamsList(image_size=tuple(C.IMAGES[i]["size"]), is_train=False)
        t.add_field("pad_size", torch.tensor(C.IMAGES[i]["pad"]))
        t.add_field("calib", Calibration(C.image_P(i)))
        targets.append(t)
    hm = torch.from_numpy(m["hmap"]).to(DEV)
    results, utils, _ = post({"hm_nhwc": hm, "cls": None}, targets)
    sc, ix = ops.decode_topk(hm, 0, s["ncls"], 50)
    torch.cuda.synchronize()
    assert np.array_equal(ix.cpu().numpy(), np.take_along_axis(index, np.argsort(-scores, axis=2, kind="stable"), axis=2))
    ref = DC.decode_boxes(m["hmap"], m["reg_off"], sc.cpu().numpy(), ix.cpu().numpy(), m["calib"], m["pad"], m["img_size"], thr, mode, s)
    det, topk, valid = (utils[k].cpu().numpy() for k in ("det_all", "topk", "valid"))
    # (the uncertainty the dict reports covers the valid rows only: the full table is compared through decode_device below)
    unc = post.decode_device(hm, *post.prepare_targets(targets, DEV), return_unc=True)[3].cpu().numpy()
    setting = {"defaults": "a_defaults", "car": "yaml"}[which]                 # the yardstick of the same arithmetic (car: the yaml's rules, one class)
    _compare("PostProcessor %s" % which, (det, topk, valid, unc), ref, mode, setting, s=s)
    for b in range(3):
        keep = ref["valid"][b].astype(bool)
        assert 0 < keep.sum() < 50 and np.array_equal(results[b].cpu().numpy(), det[b][keep])
        assert np.array_equal(utils["vis_scores"][b].cpu().numpy(), topk[b][keep, 0])
        if which == "defaults":
            assert utils["uncertainty_conf"] is None and utils["estimated_depth_error"] is None
        else:
            assert np.array_equal(utils["estimated_depth_error"][b].cpu().numpy(), unc[b][keep, 0])
            assert np.array_equal(utils["uncertainty_conf"][b].cpu().numpy(), unc[b][keep, 1])
            assert np.array_equal(results[b].cpu().numpy()[:, 13], topk[b][keep, 0] * unc[b][keep, 1])


def test_detector_forward_under_the_config_defaults():
    """An eval-mode KeypointDetector whose decode settings are the config defaults (the yaml keeps the network as it is): the rows of the
    device pipeline, eager and replayed from a graph, are bitwise post.decode_device on the head map it produced -- and differ from the
    built-in decode's."""
    from monoflex_amd import ops, synthetic as S
    from monoflex_amd.config import get_cfg
    from monoflex_amd.model.detector import KeypointDetector
    from monoflex_amd.model.head.detector_predictor import REG_OFF
    from monoflex_amd.structures.params_3d import make_test_target
    ow, oh = 48, 24
    cfg = get_cfg(YAML_FILE, [])
    d = _defaults_cfg()
    cfg.MODEL.HEAD.DEPTH_MODE, cfg.MODEL.HEAD.DIMENSION_REG = d.MODEL.HEAD.DEPTH_MODE, list(d.MODEL.HEAD.DIMENSION_REG)
    cfg.MODEL.HEAD.OUTPUT_DEPTH, cfg.TEST.UNCERTAINTY_AS_CONFIDENCE = d.MODEL.HEAD.OUTPUT_DEPTH, d.TEST.UNCERTAINTY_AS_CONFIDENCE
    cfg.MODEL.PRETRAIN, cfg.DATASETS.TEST_SPLIT = False, "test"
    cfg.INPUT.WIDTH_TRAIN, cfg.INPUT.HEIGHT_TRAIN = ow * 4, oh * 4
    m = KeypointDetector(cfg).eval()
    m.load_state_dict(S.synthetic_state_dict(m.state_dict(), seed=0, cls_bias=-1.0))
    m.to(DEV)
    post = m.heads.post_processor
    assert (post.decode_cfg.depth_decode, post.decode_cfg.dim_exp, post.decode_cfg.uncertainty_as_conf, post.output_depth) == (0, 0, 0, "direct")
    imgs = S.synthetic_images(2, oh * 4, ow * 4, seed=1000).to(DEV)
    tg = m.device_targets([make_test_target(S.synthetic_target(ow, oh))] * 2, DEV)
    with torch.no_grad():
        side = torch.cuda.Stream()
        side.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(side):
            eager = [t.clone() for t in m.detect_device(imgs, *tg)]
        torch.cuda.current_stream().wait_stream(side)
        torch.cuda.synchronize()
        graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(graph):
            held = m.detect_device(imgs, *tg)
        graph.replay()
        torch.cuda.synchronize()
        for det, topk, valid, hm in (eager, held):
            again = post.decode_device(hm, tg[2], tg[3], tg[4], None)
            assert all(torch.equal(a, b) for a, b in zip((det, topk, valid), again))
            assert torch.equal(det[..., 13], topk[..., 0]) and int(valid.sum()) > 0
            built_in = ops.decode_boxes(hm, REG_OFF, *ops.decode_topk(hm, 0, 3, post.max_detection), tg[3], tg[2], tg[4], float(post.det_threshold),
                                        depth_mode="direct")
            assert not torch.equal(built_in[0][..., 6:9], det[..., 6:9])
    assert all(torch.equal(a, b) for a, b in zip(eager[:3], held[:3]))


def test_zz_worst_error_table():
    """Prints the per-column worst error of the cases above next to the yardstick (the table of the module docstring)."""
    if not WORST:                                             # (run alone: nothing to print)
        return
    worst = np.max(np.stack(list(WORST.values())), axis=0)
    yard = np.array([DC.YARDSTICK[s] for s in WORST])
    print("column   float32 reference (worst setting)   bound of the tightest setting   kernel, worst of all cases")
    for i, c in enumerate(D.COLUMNS):
        print("%-8s %-35.2e %-31.2e %.2e" % (c, yard[:, i].max(), 4 * yard[:, i].min(), worst[i]))
    for s in WORST:
        print("%-16s %s" % (s, D.format_errors(WORST[s])))
