"""Recorder of tests/golden/kitti_encode_settings.npz: the reference's own KITTIDataset under the target-encoder settings other
than those of runs/monoflex.yaml.

Sibling of tools/gen_right_view_golden.py and of oracle/gen_golden.py `kitti`: the same twelve label sets, sizes, flips, image
seeds and `random.seed(i)`, the same stand-ins, runs/monoflex.yaml plus the overrides of one entry of SETTINGS at a time.
Recorded per setting and case: every target field that a setting can touch -- or, where the reference itself raises, that it
did and with what.  `hm` is stored as its difference from the yaml heat map of the same case (flat indices + values; the yaml
run is repeated here and checked against tests/golden/kitti_encode.npz, which holds the labels and sizes as well), the other
fields whole.  `edge_indices`, `edge_len` and `pad_size` depend on no setting and are not stored.  INPUT.TO_BGR True is recorded
as frame checksums of three cases.

Needs the reference checkout that oracle/gen_golden.py names; run from the repository root:
    python tools/gen_encode_settings_golden.py
"""
import os
import random
import shutil
import sys
import tempfile
import types

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import numpy as np
import torch

from monoflex_amd import synthetic as S
from oracle import gen_golden as G

# name -> overrides of runs/monoflex.yaml, as command-line `opts` pairs
SETTINGS = {
    "no_outside": ["DATASETS.CONSIDER_OUTSIDE_OBJS", "False"],
    "circular": ["INPUT.ADJUST_BOUNDARY_HEATMAP", "False"],
    "no_modify": ["INPUT.KEYPOINT_VISIBLE_MODIFY", "False"],
    "center2d_circular": ["INPUT.HEATMAP_CENTER", "2D", "INPUT.ADJUST_BOUNDARY_HEATMAP", "False"],
    "center2d_no_outside": ["INPUT.HEATMAP_CENTER", "2D", "DATASETS.CONSIDER_OUTSIDE_OBJS", "False"],
    "center2d_edge": ["INPUT.HEATMAP_CENTER", "2D"],                                   # the reference asserts on most samples
    "defaults": ["DATASETS.CONSIDER_OUTSIDE_OBJS", "False", "INPUT.ADJUST_BOUNDARY_HEATMAP", "False",
                 "INPUT.KEYPOINT_VISIBLE_MODIFY", "False", "DATASETS.FILTER_ANNO_ENABLE", "False"],
}
FIELDS = [k for k in G.KITTI_FIELDS if k not in ("edge_indices", "edge_len", "pad_size", "hm")]
BGR_CASES = ("s00", "s01", "s06")


def main():
    from PIL import Image
    G.install_stubs()
    sys.path.insert(0, G.REF)
    os.chdir(G.REF)
    np.int = int                                                        # kitti.py:434,436 under numpy >= 1.24
    from config import cfg as base_cfg
    base_cfg.merge_from_file(os.path.join(G.REF, "runs", "monoflex.yaml"))
    import data.transforms.transforms as T
    T.F = types.SimpleNamespace(
        to_tensor=lambda img: torch.from_numpy(np.asarray(img, dtype=np.uint8).copy()).permute(2, 0, 1).float().div(255),
        normalize=lambda t, mean, std: (t - torch.tensor(mean).view(3, 1, 1)) / torch.tensor(std).view(3, 1, 1))
    from data.transforms import build_transforms
    from data.datasets.kitti import KITTIDataset
    import data.datasets.kitti as ref_kitti
    assert os.path.abspath(ref_kitti.__file__).startswith(G.REF + os.sep), ref_kitti.__file__
    from data.augmentations.augmentations import Compose, RandomHorizontallyFlip
    root = tempfile.mkdtemp(prefix="kitti_fake_settings_")
    for d in ("image_2", "label_2", "calib", "ImageSets"):
        os.makedirs(os.path.join(root, d))
    cases = G.kitti_cases()
    P = np.asarray(S.KITTI_P2, dtype=np.float64).reshape(-1)
    yaml_gold = np.load(os.path.join(G.GOLD, "kitti_encode.npz"))
    for i, (name, w, h, n, flip, lseed, iseed) in enumerate(cases):
        Image.fromarray(np.random.RandomState(iseed).randint(0, 256, (h, w, 3)).astype(np.uint8)).save(os.path.join(root, "image_2", "%06d.png" % i))
        lines = S.synthetic_kitti_labels(lseed, w, h, n)
        assert "\n".join(lines) == str(yaml_gold[name + "_labels"]) and [w, h, int(flip), iseed] == list(yaml_gold[name + "_meta"])
        with open(os.path.join(root, "label_2", "%06d.txt" % i), "w") as f:
            f.write("".join(l + "\n" for l in lines))
        with open(os.path.join(root, "calib", "%06d.txt" % i), "w") as f:
            f.write("P2: " + " ".join("%.12e" % v for v in P) + "\n")
            f.write("P3: " + " ".join("%.12e" % v for v in P) + "\n")
            f.write("R0_rect: 1 0 0 0 1 0 0 0 1\nTr_velo_to_cam: 1 0 0 0 0 1 0 0 0 0 1 0\n")
    with open(os.path.join(root, "ImageSets", "train.txt"), "w") as f:
        f.write("".join("%06d\n" % i for i in range(len(cases))))

    def sample(ds, i, flip):
        ds.augmentation = Compose([RandomHorizontallyFlip(1.0 if flip else 0.0)])
        random.seed(i)
        img, target, idx = ds[i]
        assert idx == "%06d" % i and tuple(img.shape) == (3, 384, 1280)
        return img, target

    def dataset(opts):
        cfg = base_cfg.clone()
        cfg.merge_from_list(opts)
        return KITTIDataset(cfg, root, is_train=True, transforms=build_transforms(cfg, True), augment=True)

    out = dict(names=np.array([c[0] for c in cases]), settings=np.array(list(SETTINGS)), fields=np.array(FIELDS),
               bgr_cases=np.array(BGR_CASES))
    ds = dataset([])                                                    # the yaml run: the base of the stored heat-map differences
    yaml_hm = {}
    for i, (name, w, h, n, flip, lseed, iseed) in enumerate(cases):
        _, target = sample(ds, i, flip)
        yaml_hm[name] = np.asarray(target.get_field("hm"))
        assert np.array_equal(yaml_hm[name], yaml_gold[name + "_hm"]), name
    report = {}
    for setting, opts in SETTINGS.items():
        out[setting + "_opts"] = np.array(opts)
        ds = dataset(opts)
        kept = []
        for i, (name, w, h, n, flip, lseed, iseed) in enumerate(cases):
            key = "%s_%s_" % (setting, name)
            try:
                _, target = sample(ds, i, flip)
            except Exception as e:                                       # the reference itself fails on this sample
                out[key + "raised"] = np.array(1)
                out[key + "error"] = np.array("%s: %s" % (type(e).__name__, e))
                kept.append(None)
                continue
            out[key + "raised"] = np.array(0)
            for k in FIELDS:
                out[key + k] = np.asarray(target.get_field(k))
            hm = np.asarray(target.get_field("hm"))
            idx = np.flatnonzero(hm.ravel() != yaml_hm[name].ravel())
            out[key + "hm_idx"], out[key + "hm_val"] = idx.astype(np.int32), hm.ravel()[idx]
            kept.append((int(target.get_field("reg_mask").sum()), int(target.get_field("trunc_mask").sum())))
        report[setting] = kept
    ds = dataset(["INPUT.TO_BGR", "True"])
    for i, (name, w, h, n, flip, lseed, iseed) in enumerate(cases):
        if name in BGR_CASES:
            img, _ = sample(ds, i, flip)
            cs = G.checksum(img)
            out["bgr_%s_img_sum" % name] = np.array([cs["sum"], cs["abssum"], cs["sq"]])
            out["bgr_%s_img_idx" % name], out["bgr_%s_img_samples" % name] = cs["idx"], cs["samples"]
    out["meta"] = np.array("reference KITTIDataset.__getitem__ (data/datasets/kitti.py) + RandomHorizontallyFlip + ToTensor/Normalize "
                           "stand-in under runs/monoflex.yaml + <setting>_opts; numpy %s; P2 = monoflex_amd.synthetic.KITTI_P2; labels, "
                           "sizes, flips and the yaml heat maps that <setting>_<case>_hm_idx/_hm_val patch: kitti_encode.npz" % np.__version__)
    path = os.path.join(G.GOLD, "kitti_encode_settings.npz")
    np.savez_compressed(path, **out)
    shutil.rmtree(root)
    with open(os.path.join(G.GOLD, "kitti_encode_settings.md"), "w") as f:
        f.write("# kitti_encode_settings.npz\n\n"
                "Written by `tools/gen_encode_settings_golden.py`: the reference's own `KITTIDataset.__getitem__` on the twelve label sets of\n"
                "`kitti_encode.npz` (same sizes, flips, seeds) under `runs/monoflex.yaml` plus the overrides below, one setting at a time.\n\n"
                "Keys: `<setting>_opts`; per case `<setting>_<case>_raised`, then either `_error` or every field of `fields` plus\n"
                "`_hm_idx` / `_hm_val`, the flat positions and values at which the heat map differs from `<case>_hm` of `kitti_encode.npz`.\n"
                "`edge_indices`, `edge_len` and `pad_size` depend on no setting and are not stored. `bgr_<case>_img_*`: checksums of the\n"
                "network input under `INPUT.TO_BGR True` for the cases of `bgr_cases`.\n\n"
                "| setting | overrides | kept objects s00..s11 | truncated s00..s11 |\n|---|---|---|---|\n")
        for setting, kept in report.items():
            f.write("| `%s` | `%s` | %s | %s |\n" % (setting, " ".join(SETTINGS[setting]),
                                                  " ".join("raised" if k is None else str(k[0]) for k in kept),
                                                  " ".join("-" if k is None else str(k[1]) for k in kept)))
        f.write("\n`raised`: the reference fails there (`AssertionError` at its edge heat map, both radii positive); `center2d_edge` is the\n"
                "combination the Python front refuses.\n")
    print("kitti_encode_settings.npz: %d bytes; (kept, truncated) objects per sample (None: the reference raised)" % os.path.getsize(path))
    for setting, kept in report.items():
        print("  %-20s %s" % (setting, kept))
        for name in out["names"]:
            if int(out["%s_%s_raised" % (setting, name)]):
                print("      %s raised %s" % (name, out["%s_%s_error" % (setting, name)]))


if __name__ == "__main__":
    main()
