"""Recorder of tests/golden/kitti_encode_right.npz: the reference's own KITTIDataset with DATASETS.USE_RIGHT_IMAGE True.

Sibling of oracle/gen_golden.py `kitti` (same twelve label sets, sizes, flips and `random.seed(i)`), with three differences:
the generated folder also has image_3/ (frames drawn from another seed than image_2/, so that reading the wrong directory
shows), the calib files carry a real right-camera matrix (monoflex_amd.synthetic.KITTI_P3: P2 with KITTI's usual P3 offsets
in the last column) and the configuration switches the right view on.  Recorded per case: `ds[N + i]`, i.e. frame i seen by
the right camera -- every target field, the target's calib.P, the frame checksum -- or, where the reference itself raises,
that it did and with what.

Needs the reference checkout that oracle/gen_golden.py names; run from the repository root:
    python tools/gen_right_view_golden.py
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

RIGHT_IMAGE_SEED = 1900                                   # image_3/ frame i: RandomState(RIGHT_IMAGE_SEED + i); image_2/ uses 900 + i


def main():
    from PIL import Image
    G.install_stubs()
    sys.path.insert(0, G.REF)
    os.chdir(G.REF)
    np.int = int                                                        # kitti.py:434,436 under numpy >= 1.24
    from config import cfg
    cfg.merge_from_file(os.path.join(G.REF, "runs", "monoflex.yaml"))
    cfg.DATASETS.USE_RIGHT_IMAGE = True
    import data.transforms.transforms as T
    T.F = types.SimpleNamespace(
        to_tensor=lambda img: torch.from_numpy(np.asarray(img, dtype=np.uint8).copy()).permute(2, 0, 1).float().div(255),
        normalize=lambda t, mean, std: (t - torch.tensor(mean).view(3, 1, 1)) / torch.tensor(std).view(3, 1, 1))
    from data.transforms import build_transforms
    from data.datasets.kitti import KITTIDataset
    import data.datasets.kitti as ref_kitti
    assert os.path.abspath(ref_kitti.__file__).startswith(G.REF + os.sep), ref_kitti.__file__
    from data.augmentations.augmentations import Compose, RandomHorizontallyFlip
    root = tempfile.mkdtemp(prefix="kitti_fake_right_")
    for d in ("image_2", "image_3", "label_2", "calib", "ImageSets"):
        os.makedirs(os.path.join(root, d))
    cases = G.kitti_cases()
    N = len(cases)
    P2, P3 = np.asarray(S.KITTI_P2, dtype=np.float64).reshape(-1), np.asarray(S.KITTI_P3, dtype=np.float64).reshape(-1)
    out = dict(names=np.array([c[0] for c in cases]))
    for i, (name, w, h, n, flip, lseed, iseed) in enumerate(cases):
        for folder, seed in (("image_2", iseed), ("image_3", RIGHT_IMAGE_SEED + i)):
            img = np.random.RandomState(seed).randint(0, 256, (h, w, 3)).astype(np.uint8)
            Image.fromarray(img).save(os.path.join(root, folder, "%06d.png" % i))
        lines = S.synthetic_kitti_labels(lseed, w, h, n)
        with open(os.path.join(root, "label_2", "%06d.txt" % i), "w") as f:
            f.write("".join(l + "\n" for l in lines))
        with open(os.path.join(root, "calib", "%06d.txt" % i), "w") as f:
            f.write("P2: " + " ".join("%.12e" % v for v in P2) + "\n")
            f.write("P3: " + " ".join("%.12e" % v for v in P3) + "\n")
            f.write("R0_rect: 1 0 0 0 1 0 0 0 1\nTr_velo_to_cam: 1 0 0 0 0 1 0 0 0 0 1 0\n")
        out[name + "_labels"] = np.array("\n".join(lines))
        out[name + "_meta"] = np.array([w, h, int(flip), RIGHT_IMAGE_SEED + i])
    with open(os.path.join(root, "ImageSets", "train.txt"), "w") as f:
        f.write("".join("%06d\n" % i for i in range(N)))
    ds = KITTIDataset(cfg, root, is_train=True, transforms=build_transforms(cfg, True), augment=True)
    out["len"] = np.array(len(ds))
    kept = []
    for i, (name, w, h, n, flip, lseed, iseed) in enumerate(cases):
        ds.augmentation = Compose([RandomHorizontallyFlip(1.0 if flip else 0.0)])
        random.seed(i)
        try:
            img, target, idx = ds[N + i]
        except Exception as e:                                           # the reference itself fails on this sample
            out[name + "_raised"] = np.array(1)
            out[name + "_error"] = np.array("%s: %s" % (type(e).__name__, e))
            kept.append(None)
            continue
        out[name + "_raised"] = np.array(0)
        assert idx == "%06d" % i and tuple(img.shape) == (3, 384, 1280)
        for k in G.KITTI_FIELDS:
            out[name + "_" + k] = np.asarray(target.get_field(k))
        out[name + "_P"] = np.asarray(target.get_field("calib").P, dtype=np.float64)
        cs = G.checksum(img)
        out[name + "_img_sum"] = np.array([cs["sum"], cs["abssum"], cs["sq"]])
        out[name + "_img_idx"], out[name + "_img_samples"] = cs["idx"], cs["samples"]
        kept.append(int(target.get_field("reg_mask").sum()))
    out["P3"] = np.asarray(S.KITTI_P3, dtype=np.float64).reshape(3, 4)
    out["meta"] = np.array("reference KITTIDataset.__getitem__(N + i) with DATASETS.USE_RIGHT_IMAGE True (data/datasets/kitti.py) + "
                           "RandomHorizontallyFlip + ToTensor/Normalize stand-in; numpy %s; P3 = monoflex_amd.synthetic.KITTI_P2 with "
                           "the last column %r (monoflex_amd.synthetic.KITTI_P3); image_3 frame i = RandomState(%d + i)"
                           % (np.__version__, tuple(float(v) for v in S.KITTI_P3[:, 3]), RIGHT_IMAGE_SEED))
    np.savez_compressed(os.path.join(G.GOLD, "kitti_encode_right.npz"), **out)
    shutil.rmtree(root)
    print("kitti_encode_right.npz: len(ds) = %d, objects kept per sample (None: the reference raised)" % len(ds), kept)
    for name in out["names"]:
        if int(out[str(name) + "_raised"]):
            print("  %s raised %s" % (name, out[str(name) + "_error"]))


if __name__ == "__main__":
    main()
