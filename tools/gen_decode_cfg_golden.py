"""Recorder of tests/golden/decode_cfg.npz: the reference's own PostProcessor.forward under head settings other than runs/monoflex.yaml's.

Sibling of oracle/gen_golden.py `decode_structured` (same structured head maps of tests/decode_cases.py, isolated class peaks with distinct
scores, four images with their own pad / size / calibration, one image at a time), with the configuration changed per setting of
tests/decode_cfg_ref.py SETTINGS:
  a_defaults      DEPTH_MODE exp, DIMENSION_REG [linear, True, False], TEST.UNCERTAINTY_AS_CONFIDENCE False (the config defaults)
  a_linear_std    the same with DIMENSION_REG [linear, True, True] (DIMENSION_STD in use)
  b_linear_depth  DEPTH_MODE linear (DEPTH_REFERENCE)
  c_exp_dims_std  DIMENSION_REG [exp, True, True]
  d_linear_dims   DIMENSION_REG [linear, True, False]
  e_car           DETECT_CLASSES ("Car",), custom DIMENSION_MEAN / DIMENSION_STD, DEPTH_RANGE [1, 60]
  e_two_classes   DETECT_CLASSES ("Car", "Pedestrian"), custom DIMENSION_MEAN / DIMENSION_STD, DEPTH_RANGE [1, 60]
each under OUTPUT_DEPTH soft, hard and direct.  Stored: the seeds, and per (setting, mode, image) the result rows and, where the reference
reports them, `uncertainty_conf` and `estimated_depth_error`.

Needs the reference checkout that oracle/gen_golden.py names; run from the repository root:
    python tools/gen_decode_cfg_golden.py
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
from tests import decode_cfg_ref as DC

SEEDS = dict(map_seed=51, list_seed=52, K=50, score_ranges=[(0.02, 0.245), (0.05, 0.23), (0.02, 0.22), (0.02, 0.235)])
IMAGES = (0, 1, 2, 3)
CLASSES = ("Car", "Pedestrian", "Cyclist")


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
    maps = C.structured_maps(SEEDS["map_seed"], IMAGES)
    scores, index = C.peak_lists(SEEDS["list_seed"], len(IMAGES), SEEDS["K"], SEEDS["score_ranges"])
    base = S.synthetic_target(C.W, C.H)
    out = {k: np.array(v) for k, v in SEEDS.items()}
    out["images"], out["settings"], out["modes"] = np.array(IMAGES), np.array(list(DC.SETTINGS)), np.array(DC.GOLDEN_MODES)
    for name, s in DC.SETTINGS.items():
        H = cfg.MODEL.HEAD
        H.DEPTH_MODE, H.DEPTH_RANGE, H.DEPTH_REFERENCE = s["depth_mode"], list(s["depth_range"]), tuple(s["depth_ref"])
        H.DIMENSION_REG = ["exp" if s["dim_exp"] else "linear", True, bool(s["dim_use_std"])]
        H.DIMENSION_MEAN, H.DIMENSION_STD = tuple(tuple(r) for r in s["dim_mean"]), tuple(tuple(r) for r in s["dim_std"])
        cfg.TEST.UNCERTAINTY_AS_CONFIDENCE = bool(s["uncertainty_as_conf"])
        cfg.DATASETS.DETECT_CLASSES = CLASSES[:s["ncls"]]
        for mode in DC.GOLDEN_MODES:
            H.OUTPUT_DEPTH = mode
            post = make_post_processor(cfg)
            assert post.max_detection == SEEDS["K"] and post.det_threshold == C.THRESHOLD and post.uncertainty_as_conf == s["uncertainty_as_conf"]
            assert post.anno_encoder.depth_mode == s["depth_mode"] and list(post.anno_encoder.dim_modes) == H.DIMENSION_REG
            n_rows = []
            for b, i in enumerate(IMAGES):
                tgt = dict(base, P=C.image_P(i), size=tuple(C.IMAGES[i]["size"]), pad_size=torch.tensor(C.IMAGES[i]["pad"], dtype=torch.int64))
                cls = torch.from_numpy(C.peak_heat(scores, index, b)[:s["ncls"]])[None]
                reg = torch.from_numpy(maps["hmap"][b, :, :, maps["reg_off"]:maps["reg_off"] + 50]).permute(2, 0, 1)[None].contiguous()
                r, utils, _ = post({"cls": cls.clone(), "reg": reg.clone()}, [G.reference_target(tgt)], test=True)
                key = "%s_%s_img%d" % (name, mode, b)
                out[key + "_result"] = r.numpy()
                assert (utils["uncertainty_conf"] is None) == (utils["estimated_depth_error"] is None) == (not s["uncertainty_as_conf"])
                if utils["uncertainty_conf"] is not None:
                    out[key + "_uncertainty_conf"] = utils["uncertainty_conf"].numpy()
                    out[key + "_estimated_depth_error"] = utils["estimated_depth_error"].numpy()
                n_rows.append(r.shape[0])
            print("decode_cfg %-16s %-6s rows per image" % (name, mode), n_rows)
    out["meta"] = np.array(repr(dict(case="decode_cfg", torch=torch.__version__, inputs="tests/decode_cases.py structured_maps / peak_lists (the first "
                                     "ncls class planes)", settings="tests/decode_cfg_ref.py SETTINGS")))
    np.savez_compressed(os.path.join(G.GOLD, "decode_cfg.npz"), **out)
    print("decode_cfg.npz: %d bytes" % os.path.getsize(os.path.join(G.GOLD, "decode_cfg.npz")))


if __name__ == "__main__":
    main()
