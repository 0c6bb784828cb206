"""Evaluation loop (reference engine/inference.py:17-126): run the detector over a loader, write one KITTI result file per
image, score them.  Batches of any size are accepted (the reference is batch-1 only); the per-image (N,14) rows come back
from the device once per batch.  TEST.EVAL_DIS_IOUS / TEST.EVAL_DEPTH (the reference's disentangled 3D IoUs, engine/inference.py:45-63,92-93,
and per-object depth errors) are computed on the device at the labelled centres and averaged here; the score-versus-IoU plots of
`--eval_score_iou` and `--vis` are not produced."""
import logging
import os
import time

import torch

from .. import ops
from ..data.evaluation import DeviceResults, LabelTable, evaluate_python, generate_kitti_3d_detection
from ..parallel import barrier


class _DiagnosticSums:
    """Host-side sums of the per-object diagnostics over a pass -> the means `compute_on_dataset(diagnostics=...)` reports."""

    def __init__(self):
        self.sums = {"depth_errors": None, "dis_ious": None}
        self.objects = 0

    def add(self, depth_err, iou, mask):
        """Fixed-shape host tables (B,M,13) / (B,M,5) (None when not computed) and reg_mask (B,M); float64 sums."""
        keep = mask.reshape(-1) != 0
        self.objects += int(keep.sum())
        for name, t in (("depth_errors", depth_err), ("dis_ious", iou)):
            if t is not None:
                part = t.reshape(-1, t.shape[-1])[keep].double().sum(dim=0)
                self.sums[name] = part if self.sums[name] is None else self.sums[name] + part

    def write(self, out):
        n = self.objects
        for name, keys in (("dis_ious", ops.EVAL_IOU_KEYS), ("depth_errors", ops.EVAL_DEPTH_KEYS)):
            s = self.sums[name]
            out[name] = {} if s is None else {k: (float(s[i]) / n if n else float("nan")) for i, k in enumerate(keys)}
        out["objects"] = n


def compute_on_dataset(model, data_loader, device, predict_folder, timer=None, overlap=True, diagnostics=None, methods=None, folders=None,
                       results=None):
    """Returns the number of images processed; `timer`, if given, is a dict that receives the seconds spent in the model (launches + waits).
    `overlap` (default, CUDA only): ONE batch stays in flight -- the fixed-size (B,50,14) rows and validity flags of batch k are copied to
    pinned memory behind an event, batch k+1 is launched, and only then does the host wait for batch k's event and write its files
    (the reference's loop, engine/inference.py:26-56, waits for every batch before it touches the next: 21 % of the time at B = 8, bench.py
    `pipeline` leg).  Same rows, same files: the per-image selection `det[b][valid[b]]` is the one PostProcessor.forward makes.
    OUTPUT_DEPTH 'oracle' keeps the overlap: its ground-truth table (ops.oracle_gt_rows, from the loader's stacked `fields` or the targets)
    goes to the device with the batch and the match runs there; targets without labels raise ValueError.
    `methods` + `folders` (equally long; `predict_folder` is then not used): ONE walk of the loader writes the result files of every depth
    method of `methods` into its folder of `folders` -- one network pass and one (B,NM,50,14) copy per batch (KeypointDetector.detect_all_device),
    the files being those of a walk per method with `post_processor.output_depth` set to it.  This form needs the device path (a CUDA device)
    and computes no diagnostics.
    `results` (a data.evaluation.DeviceResults; `predict_folder` / `folders` are then not used): the rows stay on the device -- each batch's
    det / valid are filed into the buffer by row (index_copy_, the row indices going up as one small pinned copy) and NOTHING comes back:
    no pinned result copies, no event wait, no per-image Python, no files.  (The diagnostics keep their route: with them on, their tables
    still travel behind an event per batch.)  Needs the device path as well."""
    model.eval()
    n, busy = 0, 0.0
    dev = torch.device(device)
    overlap = bool(overlap) and dev.type == "cuda" and hasattr(model, "detect_device")
    pending = None
    post = getattr(getattr(model, "heads", None), "post_processor", None)
    want = int(getattr(post, "diagnostics_wanted", 0))
    sums = _DiagnosticSums()
    multi = methods is not None
    if multi:
        methods, folders = list(methods), list(folders if folders is not None else ())
        if (results is None and len(methods) != len(folders)) or not methods:
            raise ValueError("compute_on_dataset: `methods` and `folders` pair up (one result folder per depth method)")
        if not (dev.type == "cuda" and hasattr(model, "detect_all_device")):
            raise RuntimeError("compute_on_dataset: the one-pass form over several depth methods runs on the device path (CUDA)")
        overlap, want = bool(overlap), 0
    elif results is not None and not overlap:
        raise RuntimeError("compute_on_dataset: a results buffer is filled on the device path (CUDA, a model with detect_device)")
    oracle = 'oracle' in methods if multi else getattr(post, "output_depth", None) == "oracle"

    def pinned(t):
        h = torch.empty(t.shape, dtype=t.dtype, pin_memory=True)
        h.copy_(t, non_blocking=True)
        return h

    def labelled_source(batch, targets):
        """What the ground-truth tables are stacked from: the loader's batch-stacked `fields` when the targets carry labels, else the targets
        (the test split's carry none: ValueError from the table builders, as forward)."""
        fields = batch.get("fields")
        labelled = fields is not None and all(t.has_field("reg_mask") for t in targets)
        return fields if labelled else targets

    def finish(p):
        ev, rows_h, valid_h, ids, diag_h = p
        ev.synchronize()
        for b, image_id in enumerate(ids if rows_h is not None else ()):
            if multi:
                for i, folder in enumerate(folders):
                    generate_kitti_3d_detection(rows_h[b, i][valid_h[b, i].bool()], os.path.join(folder, image_id + ".txt"))
            else:
                generate_kitti_3d_detection(rows_h[b][valid_h[b].bool()], os.path.join(predict_folder, image_id + ".txt"))
        if diag_h is not None:
            sums.add(*diag_h)
        return len(ids)

    with torch.no_grad():
        for batch in data_loader:
            images, targets, image_ids = batch["images"], batch["targets"], batch["img_ids"]
            images = images.to(device)
            targets = [t.to(device) for t in targets]
            t0 = time.perf_counter()
            if overlap or multi:
                tensors = images.tensors if hasattr(images, "tensors") else images
                dt = model.device_targets(targets, dev)
                gt = ops.oracle_gt_rows(labelled_source(batch, targets), dev) if oracle else None
                if multi:
                    det, _, valid, hm = model.detect_all_device(tensors, *dt, methods=methods, gt_rows=gt)
                else:
                    det, _, valid, hm = model.detect_device(tensors, *dt, gt_rows=gt)
                if results is not None:
                    results.scatter(image_ids, det, valid)
                    if not want:
                        busy += time.perf_counter() - t0
                        n += len(image_ids)
                        continue
                    rows_h = valid_h = None
                else:
                    rows_h = torch.empty(det.shape, dtype=det.dtype, pin_memory=True)
                    valid_h = torch.empty(valid.shape, dtype=valid.dtype, pin_memory=True)
                    rows_h.copy_(det, non_blocking=True)
                    valid_h.copy_(valid, non_blocking=True)
                diag_h = None
                if want:        # the diagnostics kernel, the ~16 small torch launches that stack its (B,M,16) table (a fill, casts, slice copies) and up to
                                # three more fixed-shape copies to pinned memory, all behind the same event: no synchronisation is added
                    gt_rows = ops.eval_diag_rows(labelled_source(batch, targets), dev)
                    depth_err, iou = model.diagnose_device(hm, gt_rows, dt[2], dt[3])
                    diag_h = (None if depth_err is None else pinned(depth_err), None if iou is None else pinned(iou),
                              pinned(gt_rows[..., 0].contiguous()))
                ev = torch.cuda.Event()
                ev.record()
                busy += time.perf_counter() - t0
                if pending is not None:
                    n += finish(pending)
                pending = (ev, rows_h, valid_h, list(image_ids), diag_h)
                if not overlap:                                        # (the one-pass form without the overlap: wait for this batch now)
                    t0 = time.perf_counter()
                    ev.synchronize()
                    busy += time.perf_counter() - t0
                    n += finish(pending)
                    pending = None
                continue
            output, eval_utils, _ = model(images, targets)
            outputs = [output] if torch.is_tensor(output) else list(output)
            outputs = [o.cpu() for o in outputs]                       # the host copy synchronises
            busy += time.perf_counter() - t0
            for image_id, rows in zip(image_ids, outputs):
                generate_kitti_3d_detection(rows, os.path.join(predict_folder, image_id + ".txt"))
            n += len(outputs)
            if want:                                                   # the valid objects' values, (image, slot) order (PostProcessor.forward)
                de, di = eval_utils["depth_errors"], eval_utils["dis_ious"]
                stack = lambda d, keys: None if d is None else torch.stack([d[k] for k in keys], dim=1).cpu()
                de, di = stack(de, ops.EVAL_DEPTH_KEYS), stack(di, ops.EVAL_IOU_KEYS)
                count = (de if de is not None else di).shape[0]
                sums.add(de, di, torch.ones(count))
        if pending is not None:
            t0 = time.perf_counter()
            pending[0].synchronize()
            busy += time.perf_counter() - t0
            n += finish(pending)
    if timer is not None:
        timer["inference_seconds"] = timer.get("inference_seconds", 0.0) + busy
    if diagnostics is not None:
        sums.write(diagnostics)
    return n


def _on_one_rank(logger, what):
    """True when this process is the whole job.  Gathering the shards of several ranks on the device is not built: they use the files."""
    import torch.distributed as dist
    if dist.is_available() and dist.is_initialized() and dist.get_world_size() > 1:
        if not _on_one_rank.told:
            logger.info("%s: TEST.EVAL_ON_DEVICE serves one rank; with %d ranks the result files are written and read back", what, dist.get_world_size())
            _on_one_rank.told = True
        return False
    return True


_on_one_rank.told = False


def _wanted_on_device(eval_on_device, data_loader):
    """The argument, or the mark data.build.build_test_loader leaves on its loaders for TEST.EVAL_ON_DEVICE (run_test passes no config on)."""
    return bool(eval_on_device) or bool(getattr(data_loader, "eval_on_device", False))


def inference(model, data_loader, dataset_name, eval_types=("detections",), device="cuda", output_folder=None, metrics=("R40",),
              eval_on_device=False):
    """-> (ret_dicts, result text of the last metric, dis_ious) on rank 0, (None, None, None) elsewhere
    (engine/inference.py:66-126). Every rank writes the result files of its shard into `<output_folder>/data`.
    dis_ious: {key: mean 3D IoU} of the five disentangled IoUs under TEST.EVAL_DIS_IOUS, {} without it; logged as the reference's
    "<key>, MEAN IOU = ..." lines, and the depth errors of TEST.EVAL_DEPTH as one line per key.  The means are rank-local, like the
    reference's: each rank averages (and rank 0 returns) the objects of its own shard; they are not reduced across ranks.
    `eval_on_device` (TEST.EVAL_ON_DEVICE): no result folder -- the rows of the pass stay on the device (compute_on_dataset's `results`
    form), one kernel pair turns them into the evaluator's records and ONE PR table serves every metric; same log lines, same return value.
    A split without labels is a ValueError before the pass starts; with more than one rank the file path is used.  A loader of
    build_test_loader under TEST.EVAL_ON_DEVICE True switches it on as well: that is how the key reaches this call through `run_test`."""
    import torch.distributed as dist
    logger = logging.getLogger("monoflex.inference")
    dataset = data_loader.dataset
    eval_on_device = _wanted_on_device(eval_on_device, data_loader) and _on_one_rank(logger, dataset_name)
    results = None
    if eval_on_device:
        table = LabelTable.of(dataset)                                 # (the test split has no labels: ValueError before the pass starts)
        results = DeviceResults(table, 1, int(model.heads.post_processor.max_detection), torch.device(device))
        predict_folder = None
    else:
        predict_folder = os.path.join(output_folder, "data")
        os.makedirs(predict_folder, exist_ok=True)
    timer = {}
    t0 = time.perf_counter()
    diagnostics = {}
    n = compute_on_dataset(model, data_loader, torch.device(device), predict_folder, timer, diagnostics=diagnostics, results=results)
    barrier()
    for key, value in diagnostics["dis_ious"].items():
        logger.info("%s, MEAN IOU = %.4f", key, value)
    for key, value in diagnostics["depth_errors"].items():
        logger.info("depth %s, MEAN = %.4f", key, value)
    logger.info("%s: %d images in %.2f s (%.4f s / img in the model)", dataset_name, n, time.perf_counter() - t0,
                timer["inference_seconds"] / max(n, 1))
    if dist.is_available() and dist.is_initialized() and dist.get_rank() != 0:
        return None, None, None
    ret_dicts, result = [], None
    if eval_on_device:
        for metric, (result, ret_dict) in zip(metrics, results.evaluate(dataset.classes, metrics)):
            logger.info("metric = %s\n%s", metric, result)
            ret_dicts.append(ret_dict)
        return ret_dicts, result, diagnostics["dis_ious"]
    for metric in metrics:
        result, ret_dict = evaluate_python(label_path=dataset.label_dir, result_path=predict_folder,
                                           label_split_file=dataset.imageset_txt, current_class=dataset.classes, metric=metric,
                                           device=device)
        logger.info("metric = %s\n%s", metric, result)
        ret_dicts.append(ret_dict)
    return ret_dicts, result, diagnostics["dis_ious"]


EVAL_DEPTH_METHODS = ("oracle", "hard", "soft", "mean", "direct", "keypoints_center", "keypoints_02", "keypoints_13")   # engine/inference.py:154


def inference_all_depths(model, data_loader, dataset_name, eval_types=("detections",), device="cuda", output_folder=None, metrics=("R40",),
                         single_pass=True, eval_on_device=False):
    """`--eval_all_depths` (engine/inference.py:131-198): the evaluation under every depth-solving method, each into
    `<output_folder>/eval_all_depths/<method>` ('oracle' needs the ground-truth fields of a validation split).  Logs the Car AP@0.70 bev/3d
    line per method and the ranking by 3D moderate.  A reduced head set walks the methods it can serve.
    `single_pass` (default): ONE walk of the loader -- every image is read and runs through the network once, and one decode launch emits the
    rows of all the methods (compute_on_dataset's `methods` form; the method enters a row through the location, roty, the score and nothing
    else).  False: the reference's loop, one whole pass per method, by re-assigning `post_processor.output_depth` between passes.  Same
    folders, byte-identical files, same log lines, same return value.
    `eval_on_device` (TEST.EVAL_ON_DEVICE; single_pass only): no folders -- the (N, NM, K, 14) rows of the one walk stay on the device and
    each method is evaluated from its slice of them.  Same log lines, same return value; with more than one rank the file path is used.
    -> {method: ret_dict} on rank 0 (the reference returns (None, None, None); the log lines are its product), the attribute restored."""
    import numpy as np
    import torch.distributed as dist
    logger = logging.getLogger("monoflex.inference")
    dataset = data_loader.dataset
    post = model.heads.post_processor
    before = post.output_depth
    root = os.path.join(output_folder, "eval_all_depths")
    rank0 = not (dist.is_available() and dist.is_initialized() and dist.get_rank() != 0)
    ret = {}
    eval_on_device = _wanted_on_device(eval_on_device, data_loader) and _on_one_rank(logger, dataset_name)
    if eval_on_device and not single_pass:
        raise ValueError("inference_all_depths: eval_on_device evaluates the one-pass form (single_pass=True); a pass per method writes files")
    table = LabelTable.of(dataset) if eval_on_device else None

    def prepare(method):
        logger.info("evaluation with depth method: %s", method)
        folder = os.path.join(root, method)
        os.makedirs(folder, exist_ok=True)
        if rank0:
            for f in os.listdir(folder):                               # stale predictions of an earlier run (:162-164)
                os.remove(os.path.join(folder, f))
        return folder

    def evaluate(method, folder):
        _, ret[method] = evaluate_python(label_path=dataset.label_dir, result_path=folder, label_split_file=dataset.imageset_txt,
                                         current_class=dataset.classes, metric="R40", device=device)

    try:
        # (a reduced head set serves a subset: lib.HeadSet.output_depths -- the others would raise in the reference, and are refused here)
        methods = [m for m in EVAL_DEPTH_METHODS if m in post.head_set.output_depths()]
        if eval_on_device:
            results = DeviceResults(table, len(methods), int(post.max_detection), torch.device(device))
            for method in methods:
                logger.info("evaluation with depth method: %s", method)
            compute_on_dataset(model, data_loader, torch.device(device), None, methods=methods, results=results)
            results.check_complete()
            for i, method in enumerate(methods):
                _, ret[method] = results.evaluate(dataset.classes, ("R40",), method=i)[0]
        elif single_pass:
            folders = [prepare(m) for m in methods]
            barrier()
            compute_on_dataset(model, data_loader, torch.device(device), None, methods=methods, folders=folders)
            barrier()
            if rank0:
                for method, folder in zip(methods, folders):
                    evaluate(method, folder)
        else:
            for method in methods:
                folder = prepare(method)
                barrier()
                post.output_depth = method
                compute_on_dataset(model, data_loader, torch.device(device), folder)
                barrier()
                if rank0:
                    evaluate(method, folder)
    finally:
        post.output_depth = before
    if not rank0:
        return None
    cls, thresh = "Car", 0.7
    logger.info("%s AP@%.2f, %.2f:", cls, thresh, thresh)
    key = lambda kind, level: "%s_%s_%.2f/%s" % (cls, kind, thresh, level)
    for method in methods:
        d = ret[method]
        logger.info("bev/3d AP, method %s:", method)
        logger.info("%.4f/%.4f, %.4f/%.4f, %.4f/%.4f", d[key("bev", "easy")], d[key("3d", "easy")], d[key("bev", "moderate")],
                    d[key("3d", "moderate")], d[key("bev", "hard")], d[key("3d", "hard")])
    order = np.argsort(-np.array([ret[m][key("3d", "moderate")] for m in methods]))
    logger.info("Cls %s, Thresh %s, Sort: %s", cls, thresh, " > ".join(methods[i] for i in order))
    return ret
