"""The loops around the network with and without the resident split (DATALOADER.RESIDENT): one JSON line.

On a generated validation directory (default 48 frames of 1242x375, 8 objects each, random pixels: incompressible PNGs, the
worst case for the decoder) it reports
  - the store build: seconds and bytes;
  - one pass of DeviceLoader with num_workers 0 and 4 and one pass of ResidentLoader: img/s, batches only, no model;
  - inference() end to end both ways (bf16, batch 8, synthetic weights; result files and the AP evaluation included);
  - the resident kernels from device events: the frame entry (one launch) and the target entry (object + heat-map launches).
Each variant runs in processes of its own, alternated over --rounds; a process makes one warm-up pass and --passes timed ones
of every loop. Means and the spread (min, max over all timed passes of all rounds) are printed; compare two means only where
they differ by more than the spread.
--child VARIANT runs one variant ("device" or "resident") in this process on --root and prints its raw passes (what the rounds
are made of; the "device" child needs nothing of the resident path)."""
import argparse
import json
import os
import subprocess
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def generate(root, frames, objects):
    import numpy as np
    from PIL import Image
    from monoflex_amd import synthetic as S
    for d in ("image_2", "label_2", "calib", "ImageSets"):
        os.makedirs(os.path.join(root, d))
    P = " ".join("%.12e" % v for v in np.asarray(S.KITTI_P2).reshape(-1))
    for i in range(frames):
        Image.fromarray(np.random.RandomState(i).randint(0, 256, (375, 1242, 3)).astype(np.uint8)).save(os.path.join(root, "image_2", "%06d.png" % i))
        with open(os.path.join(root, "label_2", "%06d.txt" % i), "w") as f:
            f.write("\n".join(S.synthetic_kitti_labels(70 + i, 1242, 375, objects, z_range=(5, 38), occl_max=1)))
        with open(os.path.join(root, "calib", "%06d.txt" % i), "w") as f:
            f.write("P2: " + P + "\nP3: " + P + "\n")
    with open(os.path.join(root, "ImageSets", "val.txt"), "w") as f:
        f.write("".join("%06d\n" % i for i in range(frames)))


def child(a):
    import torch
    from monoflex_amd import synthetic as S
    from monoflex_amd.config import get_cfg
    from monoflex_amd.data import DeviceLoader, InferenceSampler, KITTIDataset
    from monoflex_amd.engine.inference import inference
    from monoflex_amd.model.detector import KeypointDetector
    cfg = get_cfg(os.path.join(ROOT, "runs", "monoflex.yaml"), ["MODEL.COMPUTE_DTYPE", "bf16"])
    cfg.MODEL.PRETRAIN = False
    ds = KITTIDataset(cfg, a.root, is_train=False)
    n, out = len(ds), {"variant": a.child, "frames": len(ds), "batch": a.batch}

    def rate(fn):
        """One warm-up call, then a.passes timed ones -> img/s each (host clock around work that ends in a synchronise)."""
        fn()
        rates = []
        for _ in range(a.passes):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            fn()
            torch.cuda.synchronize()
            rates.append(n / (time.perf_counter() - t0))
        return rates

    def batches(loader):
        return lambda: [None for _ in loader]

    torch.manual_seed(0)
    model = KeypointDetector(cfg).cuda()
    model.load_state_dict(S.synthetic_state_dict(model.state_dict(), seed=0, cls_bias=-1.0))
    folder = tempfile.mkdtemp(prefix="resident_bench_out_")

    def infer(loader):
        return lambda: inference(model, loader, "kitti_val", output_folder=folder)

    if a.child == "device":
        for w in (0, 4):
            loader = DeviceLoader(ds, batch_size=a.batch, sampler=InferenceSampler(n), num_workers=w)
            out["loader_w%d_img_s" % w] = rate(batches(loader))
            out["inference_w%d_img_s" % w] = rate(infer(loader))
    else:
        from monoflex_amd.data import ResidentLoader, ResidentStore
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        store = ResidentStore.build(ds, list(InferenceSampler(n)), num_workers=4)
        out["store_build_s"], out["store_bytes"] = time.perf_counter() - t0, store.nbytes
        loader = ResidentLoader(ds, store=store, batch_size=a.batch, sampler=InferenceSampler(n))
        out["loader_resident_img_s"] = rate(batches(loader))
        out["inference_resident_img_s"] = rate(infer(loader))
        _, _, frames, targets = loader.prepare(list(range(min(a.batch, n))), [b % 2 for b in range(min(a.batch, n))])
        for name, fn in (("frames_entry_us", frames), ("targets_entry_us", targets)):
            for _ in range(5):
                fn()
            ev = [torch.cuda.Event(enable_timing=True) for _ in range(2)]
            ev[0].record()
            for _ in range(a.iters):
                fn()
            ev[1].record()
            torch.cuda.synchronize()
            out[name] = ev[0].elapsed_time(ev[1]) / a.iters * 1e3
    print(json.dumps(out))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", type=int, default=48)
    ap.add_argument("--objects", type=int, default=8)
    ap.add_argument("--batch", type=int, default=8)
    ap.add_argument("--passes", type=int, default=3)
    ap.add_argument("--rounds", type=int, default=2)
    ap.add_argument("--iters", type=int, default=50)
    ap.add_argument("--root", default=None, help="an existing generated directory (default: a fresh temporary one)")
    ap.add_argument("--child", choices=("device", "resident"), default=None)
    a = ap.parse_args()
    if a.child:
        return child(a)
    root = a.root
    if root is None:
        root = os.path.join(tempfile.mkdtemp(prefix="resident_bench_"), "kitti")
        generate(root, a.frames, a.objects)
    raw = {}
    for _ in range(a.rounds):
        for variant in ("device", "resident"):          # a fresh process each: the GPU is opened by one process at a time
            r = subprocess.run([sys.executable, os.path.abspath(__file__), "--child", variant, "--root", root, "--batch", str(a.batch),
                                "--passes", str(a.passes), "--iters", str(a.iters)], capture_output=True, text=True)
            if r.returncode != 0:
                sys.stderr.write(r.stderr)
                raise SystemExit("the %s child failed with exit status %d" % (variant, r.returncode))
            for k, v in json.loads(r.stdout.strip().splitlines()[-1]).items():
                if k not in ("variant", "frames", "batch"):
                    raw.setdefault(k, []).extend(v if isinstance(v, list) else [v])
    result = {"tool": "resident_loader_bench", "frames": a.frames, "batch": a.batch, "rounds": a.rounds, "passes": a.passes}
    for k, v in raw.items():
        result[k] = {"mean": sum(v) / len(v), "min": min(v), "max": max(v), "n": len(v)}
    print(json.dumps(result))


if __name__ == "__main__":
    main()
