"""Recorder of tests/golden/edge_fusion_settings.npz: the reference's own predictor under the edge fusion's other settings.

Sibling of tools/gen_head_act_golden.py: the reference's `make_predictor` on the CPU under oracle/gen_golden.py's stand-ins, runs/monoflex.yaml with
MODEL.INPLACE_ABN False (torch's own BatchNorm2d + ReLU trunks, no third-party module in the recording), B = 2 on a 24 x 40 map, once per setting
(MODEL.HEAD.EDGE_FUSION_KERNEL_SIZE, EDGE_FUSION_NORM, EDGE_FUSION_RELU) of tests/edge_fusion_ref.py SETTINGS:

    k = 1 BN, k = 5 BN, k = 7 BN + ReLU, k = 3 no norm, k = 5 no norm + ReLU

The inputs are the seeded ones of tests/head_act_ref.py (state, feature map, two edge sequences of different edge_len).  Per setting, in eval mode and
in train mode (batch statistics; forward only, no gradients: the tests take those from float64 autograd of tests/edge_fusion_ref.py), the file holds
`cls` (sigmoid_hm of the logits) and the two `3d_offset` channels of `reg` at the edge_len listed border pixels of each image -- pixels off the border do
not depend on these settings, tests/golden/head_act.npz covers them --, the reference's state-dict key list and, in train mode, the updated running
statistics of the two BatchNorm1d.

Needs the reference checkout that oracle/gen_golden.py names; run from the repository root:
    python tools/gen_edge_fusion_golden.py
"""
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

import numpy as np
import torch

from oracle import gen_golden as G
from tests import edge_fusion_ref as EF
from tests import head_act_ref as HA

FUSIONS = ("trunc_heatmap_conv", "trunc_offset_conv")


def border(t, ei, el):
    """(B, C, H, W) -> per image (C, edge_len[b]) at the listed border pixels, concatenated along the second axis"""
    return np.concatenate([t[b][:, ei[b, :el[b], 1], ei[b, :el[b], 0]].numpy() for b in range(t.shape[0])], axis=1)


def main():
    G.install_stubs()
    sys.path.insert(0, G.REF)
    os.chdir(G.REF)
    from config import cfg
    cfg.merge_from_file(os.path.join(G.REF, "runs", "monoflex.yaml"))
    cfg.MODEL.DEVICE = "cpu"
    cfg.MODEL.INPLACE_ABN = False
    cfg.INPUT.WIDTH_TRAIN, cfg.INPUT.HEIGHT_TRAIN = HA.W * 4, HA.H * 4
    import data                                                        # noqa: F401  (first: structures.params_3d and data.datasets import each other)
    from model.head.detector_predictor import make_predictor
    import model.head.detector_predictor as ref_pred
    assert os.path.abspath(ref_pred.__file__).startswith(G.REF + os.sep), ref_pred.__file__
    x = HA.features()
    tg, ei, el = HA.edge_targets()
    targets = [G.reference_target(t) for t in tg]
    out = {k: np.array(v) for k, v in HA.SEEDS.items()}
    out["beta_shift"], out["orig_sizes"] = np.array(HA.BETA_SHIFT), np.array(HA.ORIG_SIZES)
    out["settings"] = np.array([EF.setting_name(*s) for s in EF.SETTINGS])
    out["edge_len"] = el.numpy()
    for k, norm, relu in EF.SETTINGS:
        name = EF.setting_name(k, norm, relu)
        cfg.MODEL.HEAD.EDGE_FUSION_KERNEL_SIZE, cfg.MODEL.HEAD.EDGE_FUSION_NORM, cfg.MODEL.HEAD.EDGE_FUSION_RELU = k, norm, relu
        torch.manual_seed(0)
        model = make_predictor(cfg, 64)
        assert model.trunc_heatmap_conv[0].kernel_size == (k,) and isinstance(model.trunc_heatmap_conv[1], torch.nn.BatchNorm1d) == (norm == "BN")
        assert isinstance(model.trunc_heatmap_conv[2], torch.nn.ReLU) == relu
        out[name + "/keys"] = np.array(list(model.state_dict().keys()))
        model.load_state_dict(HA.synthetic_state(model.state_dict()))
        oi, oj = model.offset_index
        lo = sum(sum(c) for c in cfg.MODEL.HEAD.REGRESSION_CHANNELS[:oi]) + sum(cfg.MODEL.HEAD.REGRESSION_CHANNELS[oi][:oj])
        for mode in ("eval", "train"):
            model.train(mode == "train")
            with torch.no_grad():
                r = model(x.clone(), targets)
            out["%s/%s_cls" % (name, mode)] = border(r["cls"], ei, el)
            out["%s/%s_off" % (name, mode)] = border(r["reg"][:, lo:lo + 2], ei, el)
        if norm == "BN":
            sd = model.state_dict()
            for f in FUSIONS:
                for s in ("running_mean", "running_var"):
                    out["%s/train_%s.1.%s" % (name, f, s)] = sd["%s.1.%s" % (f, s)].numpy().copy()
        print("%-14s %3d keys, eval |cls| max %.4f |3d_offset| max %.3f" % (name, len(out[name + "/keys"]), float(np.abs(out[name + "/eval_cls"]).max()),
                                                                          float(np.abs(out[name + "/eval_off"]).max())))
    out["meta"] = np.array(repr(dict(case="edge_fusion_settings", torch=torch.__version__,
                                     config="runs/monoflex.yaml + MODEL.INPLACE_ABN False + the setting's three MODEL.HEAD.EDGE_FUSION_* keys",
                                     inputs="tests/head_act_ref.py synthetic_state / features / edge_targets")))
    path = os.path.join(G.GOLD, "edge_fusion_settings.npz")
    np.savez_compressed(path, **out)
    print("edge_fusion_settings.npz: %d bytes" % os.path.getsize(path))


if __name__ == "__main__":
    main()
