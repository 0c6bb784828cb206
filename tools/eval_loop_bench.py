"""The evaluation loop with result files and on the device (TEST.EVAL_ON_DEVICE), leg by leg: one JSON line.

On the generated validation directory of tools/resident_loader_bench.py (default 48 frames of 1242x375, 8 objects each), with a
ResidentLoader, bf16, batch 8 and synthetic weights, it reports in milliseconds per pass over the split
  files : pass_ms        compute_on_dataset as inference() runs it: network, rows to pinned memory, one result file per image
          pass_nowrite_ms the same with the file writer switched off: network + rows
          write_ms       generate_kitti_3d_detection for every image, from rows that are already on the host
          read_ms        read_label_folder of the result folder and of the label folder (what evaluate_python does per metric)
          eval_ms        get_official_eval_result from the parsed records: packing, upload, the evaluator launches, the report
  device: loader_ms      the ResidentLoader alone: the batches of one pass, no model
          pass_ms        compute_on_dataset with a results buffer: network + rows filed on the device, then one synchronise
          pass_host_ms   of that, the host time between taking a batch and having queued all its work (nothing waits for the device there)
          eval_ms / eval2_ms   DeviceResults.evaluate with one / two metrics: pack kernels, ONE PR table, the report(s)
  both  : inference_img_s / inference2_img_s   inference() end to end with one / two metrics, images per second
          all_depths_img_s                     inference_all_depths end to end
Each variant runs in processes of its own, alternated over --rounds; a process makes one warm-up call and --passes timed ones of
every leg.  --parent TREE adds a third variant: the `files` legs of inference() run from another checkout (the parent commit,
built), alternated with the others in the same session -- the yardstick of the device path.  Means and the spread (min, max over
all timed passes of all rounds) are printed; compare two means only where they differ by more than the larger spread.
--child VARIANT runs one variant in this process on --root and prints its raw passes."""
import argparse
import json
import os
import subprocess
import sys
import tempfile
import time

HERE = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def child(a):
    tree = os.path.abspath(a.tree or HERE)
    sys.path.insert(0, tree)
    import torch
    from monoflex_amd import synthetic as S
    from monoflex_amd.config import get_cfg
    from monoflex_amd.data import InferenceSampler, KITTIDataset, ResidentLoader, ResidentStore
    from monoflex_amd.data import evaluation as EV
    from monoflex_amd.engine import inference as I
    from monoflex_amd.model.detector import KeypointDetector
    cfg = get_cfg(os.path.join(tree, "runs", "monoflex.yaml"), ["MODEL.COMPUTE_DTYPE", "bf16"])
    cfg.MODEL.PRETRAIN = False
    ds = KITTIDataset(cfg, a.root, is_train=False)
    n, out = len(ds), {"variant": a.child, "frames": len(ds), "batch": a.batch}
    torch.manual_seed(0)
    model = KeypointDetector(cfg).cuda()
    model.load_state_dict(S.synthetic_state_dict(model.state_dict(), seed=0, cls_bias=-1.0))
    store = ResidentStore.build(ds, list(InferenceSampler(n)), num_workers=4)
    loader = ResidentLoader(ds, store=store, batch_size=a.batch, sampler=InferenceSampler(n))
    folder = tempfile.mkdtemp(prefix="eval_loop_bench_out_")
    dev = torch.device("cuda")

    def timed(fn):
        """One warm-up call, then a.passes timed ones -> seconds each (host clock around work that ends in a synchronise)."""
        fn()
        secs = []
        for _ in range(a.passes):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            fn()
            torch.cuda.synchronize()
            secs.append(time.perf_counter() - t0)
        return secs

    ms = lambda secs: [s * 1e3 for s in secs]
    rate = lambda secs: [n / s for s in secs]
    on_device = a.child == "device"
    kw = dict(eval_on_device=True) if on_device else {}
    if a.child != "parent":
        if on_device:
            table = EV.LabelTable.of(ds)
            K = int(model.heads.post_processor.max_detection)
            state = {}

            host = []

            def one_pass():
                timer = {}
                state["results"] = EV.DeviceResults(table, 1, K, dev)
                I.compute_on_dataset(model, loader, dev, None, timer, results=state["results"])
                host.append(timer["inference_seconds"])
            out["loader_ms"] = ms(timed(lambda: [None for _ in loader]))
            out["pass_ms"] = ms(timed(one_pass))
            out["pass_host_ms"] = ms(host[-a.passes:])
            out["eval_ms"] = ms(timed(lambda: state["results"].evaluate(ds.classes, ("R40",))))
            out["eval2_ms"] = ms(timed(lambda: state["results"].evaluate(ds.classes, ("R40", "R11"))))
        else:
            data = os.path.join(folder, "data")
            os.makedirs(data, exist_ok=True)
            out["pass_ms"] = ms(timed(lambda: I.compute_on_dataset(model, loader, dev, data)))
            writer = I.generate_kitti_3d_detection
            I.generate_kitti_3d_detection = lambda rows, path: None
            try:
                out["pass_nowrite_ms"] = ms(timed(lambda: I.compute_on_dataset(model, loader, dev, data)))
            finally:
                I.generate_kitti_3d_detection = writer
            with open(ds.imageset_txt) as f:
                ids = [int(line) for line in f.readlines()]
            rows = [torch.from_numpy(r[:, [0, 3, 4, 5, 6, 7, 9, 10, 8, 11, 12, 13, 14, 15]].astype("float32")) for r in EV.read_label_folder(data)]
            out["write_ms"] = ms(timed(lambda: [writer(r, os.path.join(data, "%06d.txt" % i)) for r, i in zip(rows, sorted(ids))]))
            recs = {}

            def read():
                recs["dt"], recs["gt"] = EV.read_label_folder(data), EV.read_label_folder(ds.label_dir, ids)
            out["read_ms"] = ms(timed(read))
            out["eval_ms"] = ms(timed(lambda: EV.get_official_eval_result(recs["gt"], recs["dt"], ds.classes, metric="R40", device="cuda")))
    out["inference_img_s"] = rate(timed(lambda: I.inference(model, loader, "kitti_val", output_folder=folder, metrics=("R40",), **kw)))
    out["inference2_img_s"] = rate(timed(lambda: I.inference(model, loader, "kitti_val", output_folder=folder, metrics=("R40", "R11"), **kw)))
    if a.child != "parent":
        out["all_depths_img_s"] = rate(timed(lambda: I.inference_all_depths(model, loader, "kitti_val", output_folder=folder, **kw)))
    print(json.dumps(out))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", type=int, default=48)
    ap.add_argument("--objects", type=int, default=8)
    ap.add_argument("--batch", type=int, default=8)
    ap.add_argument("--passes", type=int, default=3)
    ap.add_argument("--rounds", type=int, default=2)
    ap.add_argument("--root", default=None, help="an existing generated directory (default: a fresh temporary one)")
    ap.add_argument("--parent", default=None, help="another built checkout whose inference() is timed alternately (variant 'parent')")
    ap.add_argument("--child-timeout", type=float, default=300.0, help="seconds a child process may take")
    ap.add_argument("--child", choices=("files", "device", "parent"), default=None)
    ap.add_argument("--tree", default=None, help="(with --child) the checkout the child imports the package from")
    a = ap.parse_args()
    if a.child:
        return child(a)
    sys.path.insert(0, HERE)
    from tools.resident_loader_bench import generate
    root = a.root
    if root is None:
        root = os.path.join(tempfile.mkdtemp(prefix="eval_loop_bench_"), "kitti")
        generate(root, a.frames, a.objects)
    variants = [("parent", a.parent)] * bool(a.parent) + [("files", HERE), ("device", HERE)]
    raw = {}
    for _ in range(a.rounds):
        for variant, tree in variants:              # a fresh process each: the GPU is opened by one process at a time
            r = subprocess.run([sys.executable, os.path.abspath(__file__), "--child", variant, "--tree", tree, "--root", root, "--batch", str(a.batch),
                                "--passes", str(a.passes)], capture_output=True, text=True, timeout=a.child_timeout)
            if r.returncode != 0:
                sys.stderr.write(r.stderr)
                raise SystemExit("the %s child failed with exit status %d" % (variant, r.returncode))
            for k, v in json.loads(r.stdout.strip().splitlines()[-1]).items():
                if k not in ("variant", "frames", "batch"):
                    raw.setdefault(variant + "." + k, []).extend(v)
    result = {"tool": "eval_loop_bench", "frames": a.frames, "batch": a.batch, "rounds": a.rounds, "passes": a.passes}
    for k, v in raw.items():
        result[k] = {"mean": sum(v) / len(v), "min": min(v), "max": max(v), "n": len(v)}
    print(json.dumps(result))


if __name__ == "__main__":
    main()
