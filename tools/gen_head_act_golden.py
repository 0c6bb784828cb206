"""Recorder of tests/golden/head_act.npz: the reference's own predictor with MODEL.INPLACE_ABN False (conv3x3 -> BatchNorm2d -> ReLU trunks).

Sibling of tools/gen_decode_cfg_golden.py: the reference's `make_predictor` on the CPU under oracle/gen_golden.py's stand-ins, runs/monoflex.yaml
with INPLACE_ABN False, B = 2 on a 24 x 40 map.  The inputs are the seeded ones of tests/head_act_ref.py (state, feature map, edge sequences,
loss weights); the file stores the seeds, the reference's state-dict key list and its results:
  eval   `cls` (sigmoid_hm of the logits) and `reg`
  train  one step under the linear loss sum(cls * g_cls) + sum(reg * g_reg): `cls`, `reg` and `d features` (the latter two at every third
         pixel), the updated running statistics of two trunks, and per parameter the sum and the absolute sum of its gradient.

Needs the reference checkout that oracle/gen_golden.py names; run from the repository root:
    python tools/gen_head_act_golden.py
"""
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import numpy as np
import torch

from oracle import gen_golden as G
from tests import head_act_ref as HA


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
    torch.manual_seed(0)
    model = make_predictor(cfg, 64)
    assert isinstance(model.class_head[1], torch.nn.BatchNorm2d) and isinstance(model.class_head[2], torch.nn.ReLU)
    keys = list(model.state_dict().keys())
    model.load_state_dict(HA.synthetic_state(model.state_dict()))
    x = HA.features()
    tg, _, _ = HA.edge_targets()
    targets = [G.reference_target(t) for t in tg]
    out = {k: np.array(v) for k, v in HA.SEEDS.items()}
    out["beta_shift"], out["orig_sizes"], out["subset"] = np.array(HA.BETA_SHIFT), np.array(HA.ORIG_SIZES), np.array(HA.SUBSET)
    out["keys"] = np.array(keys)
    out["stat_trunks"] = np.array(HA.STAT_TRUNKS)

    model.eval()
    with torch.no_grad():
        r = model(x.clone(), targets)
    out["eval_cls"], out["eval_reg"] = r["cls"].numpy(), r["reg"].numpy()

    model.train()
    xt = x.clone().requires_grad_()
    r = model(xt, targets)
    g_cls, g_reg = HA.loss_weights(r["cls"].shape[1], r["reg"].shape[1])
    ((r["cls"] * g_cls).sum() + (r["reg"] * g_reg).sum()).backward()
    sub = HA.pixel_subset().numpy()
    out["train_cls"] = r["cls"].detach().numpy()
    out["train_reg_subset"] = r["reg"].detach().flatten(2).numpy()[:, :, sub]
    out["train_dx_subset"] = xt.grad.flatten(2).numpy()[:, :, sub]
    out["train_dx_sums"] = np.array([float(xt.grad.double().sum()), float(xt.grad.double().abs().sum())])
    sd = model.state_dict()
    for n in HA.STAT_TRUNKS:
        out["train_" + n + ".running_mean"] = sd[n + ".running_mean"].numpy().copy()
        out["train_" + n + ".running_var"] = sd[n + ".running_var"].numpy().copy()
    names = [n for n, p in model.named_parameters() if p.grad is not None]
    assert names == [n for n, _ in model.named_parameters()], "a parameter without a gradient"
    out["grad_names"] = np.array(names)
    out["grad_sums"] = np.array([[float(p.grad.double().sum()), float(p.grad.double().abs().sum())] for _, p in model.named_parameters()])
    out["meta"] = np.array(repr(dict(case="head_act", torch=torch.__version__, config="runs/monoflex.yaml + MODEL.INPLACE_ABN False",
                                     inputs="tests/head_act_ref.py synthetic_state / features / edge_targets / loss_weights")))
    path = os.path.join(G.GOLD, "head_act.npz")
    np.savez_compressed(path, **out)
    print("head_act.npz: %d bytes, %d keys, eval |cls| max %.3f |reg| max %.3f" % (os.path.getsize(path), len(keys), float(np.abs(out["eval_cls"]).max()),
                                                                                 float(np.abs(out["eval_reg"]).max())))


if __name__ == "__main__":
    main()
