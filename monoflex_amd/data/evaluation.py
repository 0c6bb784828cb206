"""KITTI result files and AP evaluation (reference data/datasets/evaluation/__init__.py:7-34,
kitti_object_eval_python/{evaluate,eval,rotate_iou,kitti_common}.py).

Same entry points as the reference -- `generate_kitti_3d_detection(prediction, predict_txt)` and
`evaluate_python(label_path, result_path, label_split_file, current_class, metric) -> (report text, result dict)` -- with
the work split differently: the host parses text and formats the report; the overlap matrices (2D, rotated BEV, 3D), the
per-class / per-difficulty ignore rules, the greedy matching at every one of the <= 41 score thresholds and the PR
accumulation run on the GPU (C ABI group 5, csrc/kitti_eval.hip), all images and all 54 (class, difficulty, metric, overlap
set) combinations at once.  The reference does this with numba CPU loops plus a numba.cuda kernel for the rotated IoU.

A second, opt-in path (TEST.EVAL_ON_DEVICE) skips the text: `DeviceResults` keeps the decode rows of a whole pass on the device,
mfx_kitti_eval_pack_* (csrc/kitti_eval_pack.hip) turn them into the record table the result files would have parsed to, bit for bit,
and `results_from_device` evaluates them against a `LabelTable` that was read once: the same report text and result dict, no files."""
import ctypes
import os
import re

import numpy as np
import torch

from .. import lib as L
from .encode import _upload

ID_TYPE_CONVERSION = {0: "Car", 1: "Pedestrian", 2: "Cyclist"}                             # evaluate.py:36-40
NAME_CODES = {"car": 0, "pedestrian": 1, "cyclist": 2, "van": 3, "person_sitting": 4, "truck": 5}
CLASS_TO_NAME = {0: "Car", 1: "Pedestrian", 2: "Cyclist", 3: "Van", 4: "Person_sitting", 5: "Truck"}
CODE_DONTCARE, CODE_OTHER, REC, PTS, MAX_DET = 6, 7, 16, 41, 64
LEVELS = ("easy", "moderate", "hard")


# ---- text ------------------------------------------------------------------------------------------------------------------
def generate_kitti_3d_detection(prediction, predict_txt):
    """(N,14) rows [cls, alpha, x1, y1, x2, y2, h, w, l, x, y, z, ry, score] -> one KITTI result file: `Type 0 0 alpha ...`,
    values rounded to 4 decimals in float32 and written as the resulting python floats; an empty prediction gives one empty
    line (evaluate.py:34-52)."""
    rows = prediction.detach().cpu().numpy() if isinstance(prediction, torch.Tensor) else np.asarray(prediction)
    lines = []
    for p in rows.reshape(-1, 14) if len(rows) else []:
        p = p.round(4)
        lines.append(" ".join([ID_TYPE_CONVERSION[int(p[0])], "0", "0"] + [repr(v) for v in p[1:].tolist()]))
    with open(predict_txt, "w", newline="") as f:
        f.write("\n".join(lines) + "\n")


def parse_label_text(text):
    """One label / result file -> (n,16) records [code, truncated, occluded, alpha, bbox(4), l, h, w, x, y, z, ry, score]
    (kitti_common.py:294-332: a file whose first line is shorter than 15 characters is empty; scores are read when the first
    line has 16 fields). Name codes follow the evaluator's lower-cased comparisons; `DontCare` is matched exactly."""
    lines = text.splitlines(keepends=True)
    if len(lines) == 0 or len(lines[0]) < 15:
        return np.zeros((0, REC), dtype=np.float64)
    rows = [l.strip().split(" ") for l in lines]
    has_score = len(rows[0]) == 16
    out = np.zeros((len(rows), REC), dtype=np.float64)
    for i, r in enumerate(rows):
        code = CODE_DONTCARE if r[0] == "DontCare" else NAME_CODES.get(r[0].lower(), CODE_OTHER)
        v = [float(x) for x in r[1:15]]
        h, w, l = v[7], v[8], v[9]
        out[i] = [code, v[0], int(r[2]), v[2], v[3], v[4], v[5], v[6], l, h, w, v[10], v[11], v[12], v[13],
                  float(r[15]) if has_score else 0.0]
    return out


def read_label_folder(folder, image_ids=None):
    """kitti_common.py:334-349: records of `<folder>/%06d.txt` for the given ids (default: every six-digit file, sorted)."""
    if image_ids is None:
        image_ids = sorted(int(f[:-4]) for f in os.listdir(folder) if re.match(r"^\d{6}.txt$", f))
    out = []
    for idx in image_ids:
        with open(os.path.join(folder, "%06d.txt" % idx)) as f:
            out.append(parse_label_text(f.read()))
    return out


# ---- device evaluation -------------------------------------------------------------------------------------------------------
def pack_eval_inputs(gts, dts, classes, min_overlaps):
    """Ragged record lists -> the flat input arrays of mfx_kitti_eval_desc, their sizes, and the orientation flag."""
    if len(gts) != len(dts):
        raise ValueError("need one detection record array per ground-truth image")
    ng = np.array([len(g) for g in gts], dtype=np.int64)
    nd = np.array([len(d) for d in dts], dtype=np.int64)
    if nd.max(initial=0) > MAX_DET:
        raise ValueError("at most %d detections per image (got %d)" % (MAX_DET, nd.max()))
    aos = False
    for d in dts:                                                   # eval.py:676-681: alpha == -10 marks "no orientation"
        if len(d):
            aos = bool(d[0, 3] != -10)
            break
    arrays = dict(gt=np.concatenate(list(gts) + [np.zeros((0, REC))]), dt=np.concatenate(list(dts) + [np.zeros((0, REC))]),
                  gt_off=np.concatenate([[0], np.cumsum(ng)]).astype(np.int32), dt_off=np.concatenate([[0], np.cumsum(nd)]).astype(np.int32),
                  pair_off=np.concatenate([[0], np.cumsum(ng * nd)]).astype(np.int64), classes=np.asarray(classes, dtype=np.int32),
                  min_overlaps=np.ascontiguousarray(min_overlaps, dtype=np.float64))
    sizes = dict(B=len(gts), n_gt=int(ng.sum()), n_dt=int(nd.sum()), n_pairs=int((ng * nd).sum()), num_classes=len(classes),
                 num_k=int(arrays["min_overlaps"].shape[0]))
    return arrays, sizes, aos


def _launch_pr(dev, sz, aos, device):
    """The four evaluator launches on inputs that are already on the device: `dev` holds gt, dt, gt_off, dt_off, pair_off, classes and
    min_overlaps as tensors (gt / dt may be absent or empty when there is no record), `sz` the sizes of pack_eval_inputs.
    -> (pr (n_comb,41,4), num_thresholds (n_comb), overlaps (3, max(n_pairs,1))) device tensors; nothing here waits for the device."""
    B, n_gt, n_dt, n_pairs, nc, nk = sz["B"], sz["n_gt"], sz["n_dt"], sz["n_pairs"], sz["num_classes"], sz["num_k"]
    n_comb = nc * 9 * nk
    lib = L.load()
    f64 = dict(dtype=torch.float64, device=device)
    overlaps = torch.empty((3, max(n_pairs, 1)), **f64)
    tp_scores = torch.empty((n_comb, max(n_gt, 1)), **f64)
    thresholds = torch.empty((n_comb, PTS), **f64)
    pr = torch.empty((n_comb, PTS, 4), **f64)
    num_valid = torch.empty((nc, 3), dtype=torch.int32, device=device)
    num_th = torch.empty(n_comb, dtype=torch.int32, device=device)
    d = L.KittiEvalDesc()
    for k in ("gt", "dt", "gt_off", "dt_off", "pair_off", "classes", "min_overlaps"):
        setattr(d, k, dev[k].data_ptr() if k in dev and dev[k].numel() else None)
    d.overlaps, d.tp_scores, d.thresholds, d.pr = overlaps.data_ptr(), tp_scores.data_ptr(), thresholds.data_ptr(), pr.data_ptr()
    d.num_valid_gt, d.num_thresholds = num_valid.data_ptr(), num_th.data_ptr()
    d.B, d.n_gt, d.n_dt, d.num_classes, d.num_k, d.compute_aos, d.n_pairs = B, n_gt, n_dt, nc, nk, int(aos), n_pairs
    with torch.cuda.device(device):
        st = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
        L.check(lib.mfx_kitti_eval_overlaps(ctypes.byref(d), st), "mfx_kitti_eval_overlaps")
        L.check(lib.mfx_kitti_eval_match_pass1(ctypes.byref(d), st), "mfx_kitti_eval_match_pass1")
        ordered = torch.sort(tp_scores, dim=1, descending=True).values.contiguous()
        L.check(lib.mfx_kitti_eval_thresholds(ctypes.byref(d), ordered.data_ptr(), st), "mfx_kitti_eval_thresholds")
        L.check(lib.mfx_kitti_eval_match_pass2(ctypes.byref(d), st), "mfx_kitti_eval_match_pass2")
    return pr, num_th, overlaps


def pr_table(gts, dts, classes, min_overlaps, device="cuda"):
    """[ (n_i,16) ] ground truths and detections, class codes, min_overlaps (num_k, 3, num_classes) ->
    (pr (nc,3,3,nk,41,4) float64, num_thresholds (nc,3,3,nk), overlaps (3,n_pairs), pair offsets, compute_aos)."""
    if torch.device(device).type != "cuda":
        raise RuntimeError("the KITTI evaluator runs on the GPU (HIP kernels); there is no CPU fallback")
    arrays, sz, aos = pack_eval_inputs(gts, dts, classes, min_overlaps)
    dev = _upload({k: v for k, v in arrays.items() if v.size}, device)
    pr, num_th, overlaps = _launch_pr(dev, sz, aos, device)
    shape = (sz["num_classes"], 3, 3, sz["num_k"])
    return (pr.cpu().numpy().reshape(shape + (PTS, 4)), num_th.cpu().numpy().reshape(shape), overlaps[:, :sz["n_pairs"]].cpu().numpy(),
            arrays["pair_off"], aos)


def _curves(pr, num_th):
    """tp/fp/fn/similarity table -> precision, orientation curves with the right-to-left running maximum (eval.py:551-565)."""
    prec, ori = np.zeros(pr.shape[:-1]), np.zeros(pr.shape[:-1])
    with np.errstate(divide="ignore", invalid="ignore"):
        for idx in np.ndindex(*num_th.shape):
            n = int(num_th[idx])
            p = pr[idx][:n]
            prec[idx][:n] = p[:, 0] / (p[:, 0] + p[:, 1])
            ori[idx][:n] = p[:, 3] / (p[:, 0] + p[:, 1])
            for t in range(n):                                      # maximum over the whole tail, zeros past n included
                prec[idx][t] = np.max(prec[idx][t:])
                ori[idx][t] = np.max(ori[idx][t:])
    return prec, ori


def _ap(curve, metric):
    idx = range(1, PTS) if metric == "R40" else range(0, PTS, 4)     # eval.py:585-597
    total = 0
    for i in idx:
        total = total + curve[..., i]
    return total / (40 if metric == "R40" else 11) * 100


def _class_overlaps(current_classes):
    """Class names or codes -> (codes, min_overlaps (2, 3, num_classes)): the strict and the loose overlap set (eval.py:650-660)."""
    name_to_class = {v: k for k, v in CLASS_TO_NAME.items()}
    if not isinstance(current_classes, (list, tuple)):
        current_classes = [current_classes]
    classes = [name_to_class[c] if isinstance(c, str) else int(c) for c in current_classes]
    strict = np.array([[0.7, 0.5, 0.5, 0.7, 0.5, 0.7]] * 3)
    loose = np.array([[0.7, 0.5, 0.5, 0.7, 0.5, 0.5], [0.5, 0.25, 0.25, 0.5, 0.25, 0.5], [0.5, 0.25, 0.25, 0.5, 0.25, 0.5]])
    return classes, np.stack([strict, loose], axis=0)[:, :, classes]


def _report(pr, num_th, aos, classes, mo, metric):
    """PR table -> (report text, result dict) under one metric (eval.py:662-741).  The table does not depend on the metric: 'R40' and
    'R11' sample the same curves at different recall positions."""
    if metric not in ("R40", "R11"):
        raise ValueError(metric)
    prec, ori = _curves(pr, num_th)
    ap = _ap(prec, metric)                                          # [class, level, metric, k]
    ap_aos = _ap(ori[:, :, 0], metric) if aos else None
    text, ret = "", {}
    for j, c in enumerate(classes):
        n = CLASS_TO_NAME[c]
        for i in range(mo.shape[0]):
            text += "{} AP@{:.2f}, {:.2f}, {:.2f}:\n".format(n, *mo[i, :, j])
            for tag, m in (("bbox", 0), ("bev ", 1), ("3d  ", 2)):
                text += "{} AP:{:.4f}, {:.4f}, {:.4f}\n".format(tag, *ap[j, :, m, i])
            if aos:
                text += "aos  AP:{:.2f}, {:.2f}, {:.2f}\n".format(*ap_aos[j, :, i])
                if i == 0:
                    for l, lv in enumerate(LEVELS):
                        ret["%s_aos/%s" % (n, lv)] = ap_aos[j, l, 0]
            for l, lv in enumerate(LEVELS):                         # key naming as in the reference (eval.py:727-737)
                ret["{}_3d_{:.2f}/{}".format(n, mo[i, 1, j], lv)] = ap[j, l, 2, i]
                ret["{}_bev_{:.2f}/{}".format(n, mo[i, 2, j], lv)] = ap[j, l, 1, i]
                ret["{}_image/{}".format(n, lv)] = ap[j, l, 0, 0]
    return text, ret


def get_official_eval_result(gts, dts, current_classes, metric="R40", device="cuda"):
    """eval.py:648-741: (report text, {'Car_3d_0.70/moderate': AP, ...}) from record lists."""
    classes, mo = _class_overlaps(current_classes)
    if metric not in ("R40", "R11"):
        raise ValueError(metric)
    pr, num_th, _, _, aos = pr_table(gts, dts, classes, mo, device)
    return _report(pr, num_th, aos, classes, mo, metric)


def evaluate_python(label_path, result_path, label_split_file, current_class, metric="R40", score_thresh=-1, device="cuda"):
    """data/datasets/evaluation/__init__.py:31-34 -> evaluate.py:17-32. `score_thresh` > 0 drops detections scoring below it
    before the evaluation (kitti_common.py:191-202)."""
    with open(label_split_file) as f:
        ids = [int(line) for line in f.readlines()]
    dts = read_label_folder(result_path)
    if score_thresh > 0:
        dts = [d[d[:, 15] >= score_thresh] for d in dts]
    gts = read_label_folder(label_path, ids)
    return get_official_eval_result(gts, dts, current_class, metric=metric, device=device)


# ---- evaluation of a pass that stayed on the device (TEST.EVAL_ON_DEVICE) -------------------------------------------------------------
class LabelTable:
    """The ground truths of a split as the evaluator reads them: `gt` (n_gt,16) = read_label_folder(label_dir, ids) concatenated and
    `gt_off` (N+1), ids in split-file order as evaluate_python reads them.  Built once per dataset (LabelTable.of caches it there) and
    uploaded once per device.  `row_of(image_id)`: the result folder is read back SORTED (read_label_folder) and paired with the ground
    truths by position, so the detections of an image belong in the row that is the rank of its id among the split's ids."""

    def __init__(self, label_dir, imageset_txt):
        with open(imageset_txt) as f:
            self.ids = [int(line) for line in f.readlines()]
        gts = read_label_folder(label_dir, self.ids)
        self.gt = np.concatenate(list(gts) + [np.zeros((0, REC))])
        self.gt_off = np.concatenate([[0], np.cumsum([len(g) for g in gts])]).astype(np.int32)
        self._rank = {idx: r for r, idx in enumerate(sorted(set(self.ids)))}
        self._dev = {}

    def __len__(self):
        return len(self.ids)

    @classmethod
    def of(cls, dataset):
        """The table of a dataset's split; the test split has no label files, which is a ValueError."""
        if getattr(dataset, "split", None) == "test":
            raise ValueError("the evaluation on the device reads the labels of the split, and the test split has none "
                             "(TEST.EVAL_ON_DEVICE needs a validation split)")
        table = getattr(dataset, "_label_table", None)
        if table is None:
            table = dataset._label_table = cls(dataset.label_dir, dataset.imageset_txt)
        return table

    def row_of(self, image_id):
        try:
            return self._rank[int(image_id)]
        except KeyError:
            raise ValueError("need one detection record array per ground-truth image (image %s is not in the split)" % (image_id,)) from None

    def on(self, device):
        """{gt, gt_off} on `device`, uploaded at the first call."""
        device = torch.device(device)
        if device.type == "cuda" and device.index is None:
            device = torch.device("cuda", torch.cuda.current_device())
        if device not in self._dev:
            self._dev[device] = dict(gt=torch.from_numpy(self.gt).to(device), gt_off=torch.from_numpy(self.gt_off).to(device))
        return self._dev[device]


def _check_slots(K):
    if K > MAX_DET:
        raise ValueError("at most %d detections per image (got %d)" % (MAX_DET, K))


class DeviceResults:
    """The detections of one pass, kept on the device: det (N, NM, K, 14) float32 and valid (N, NM, K) int32, row = LabelTable.row_of(id).
    `scatter` files a batch by row (an image delivered twice overwrites its row, as its result file would be overwritten); `evaluate`
    refuses a pass that left an image of the split out with the ValueError the file path raises on the count mismatch."""

    def __init__(self, label_table, num_methods=1, K=50, device="cuda"):
        _check_slots(K)
        self.table, N = label_table, len(label_table)
        self.det = torch.empty((N, num_methods, K, 14), dtype=torch.float32, device=device)
        self.valid = torch.zeros((N, num_methods, K), dtype=torch.int32, device=device)
        self.seen = np.zeros(N, dtype=bool)

    def scatter(self, image_ids, det, valid):
        """det (B,[NM,]K,14), valid (B,[NM,]K) of the images `image_ids` -> their rows; the row indices go up as one small pinned copy."""
        rows = np.asarray([self.table.row_of(i) for i in image_ids], dtype=np.int64)
        if tuple(det.shape[-2:]) != tuple(self.det.shape[-2:]) or det.numel() != len(rows) * self.det[0].numel() or valid.numel() != len(rows) * self.valid[0].numel():
            raise ValueError("a batch of %d images brings det %s / valid %s, the buffer holds %s per image"
                             % (len(rows), tuple(det.shape), tuple(valid.shape), tuple(self.det.shape[1:])))
        index = _upload(dict(rows=rows), self.det.device)["rows"] if self.det.device.type == "cuda" else torch.from_numpy(rows)
        self.det.index_copy_(0, index, det.reshape((len(rows),) + tuple(self.det.shape[1:])))
        self.valid.index_copy_(0, index, valid.reshape((len(rows),) + tuple(self.valid.shape[1:])))
        self.seen[rows] = True

    def check_complete(self):
        if not self.seen.all():
            raise ValueError("need one detection record array per ground-truth image (%d of the split's %d images were not delivered)"
                             % (int((~self.seen).sum()), len(self.seen)))

    def evaluate(self, classes, metrics=("R40",), method=0):
        self.check_complete()
        return results_from_device(self.table, self.det, self.valid, classes, metrics, method)


def pack_detections(gt_off, det, valid, method=0):
    """det (N,NM,K,14) float32, valid (N,NM,K) int32 and the ground-truth offsets (N+1) int32, all on the device -> the evaluator's detection
    inputs for depth method `method`: (dt (N*K,16) float64 of which the first n_dt rows are records, dt_off (N+1) int32, pair_off (N+1) int64,
    n_dt, n_pairs, compute_aos).  Two launches (mfx_kitti_eval_pack_count / _rows) with two cumsums between them; n_dt, n_pairs and the first
    record's alpha (eval.py:676-681: alpha == -10 marks "no orientation") come to the host in one small copy, the only wait."""
    N, NM, K = (int(v) for v in valid.shape)
    _check_slots(K)
    if det.device.type != "cuda":
        raise RuntimeError("the KITTI evaluator runs on the GPU (HIP kernels); there is no CPU fallback")
    if tuple(det.shape) != (N, NM, K, 14) or det.dtype != torch.float32 or valid.dtype != torch.int32 or not (det.is_contiguous() and valid.is_contiguous()):
        raise ValueError("pack_detections: det (N,NM,K,14) float32 and valid (N,NM,K) int32, contiguous; got %s %s / %s %s"
                         % (tuple(det.shape), det.dtype, tuple(valid.shape), valid.dtype))
    if tuple(gt_off.shape) != (N + 1,) or gt_off.dtype != torch.int32 or not 0 <= method < NM:
        raise ValueError("pack_detections: gt_off (N+1) int32 and a method index below NM")
    device, lib = det.device, L.load()
    n_det = torch.empty(N, dtype=torch.int32, device=device)
    n_pair = torch.empty(N, dtype=torch.int64, device=device)
    dt_off = torch.zeros(N + 1, dtype=torch.int32, device=device)
    pair_off = torch.zeros(N + 1, dtype=torch.int64, device=device)
    dt = torch.empty((N * K, REC), dtype=torch.float64, device=device)
    with torch.cuda.device(device):
        st = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
        L.check(lib.mfx_kitti_eval_pack_count(valid.data_ptr(), N, NM, K, method, gt_off.data_ptr(), n_det.data_ptr(), n_pair.data_ptr(), st),
                "mfx_kitti_eval_pack_count")
        torch.cumsum(n_det, 0, dtype=torch.int32, out=dt_off[1:])
        torch.cumsum(n_pair, 0, out=pair_off[1:])
        L.check(lib.mfx_kitti_eval_pack_rows(det.data_ptr(), valid.data_ptr(), N, NM, K, method, dt_off.data_ptr(), dt.data_ptr(), st),
                "mfx_kitti_eval_pack_rows")
        head = torch.stack([dt_off[N].double(), pair_off[N].double(), dt[0, 3]]).cpu()
    n_dt, n_pairs = int(head[0]), int(head[1])
    return dt, dt_off, pair_off, n_dt, n_pairs, bool(n_dt > 0 and float(head[2]) != -10)


def results_from_device(label_table, det, valid, classes, metrics=("R40",), method=0):
    """[(report text, result dict) per metric] of the detections det / valid (pack_detections' layout, rows in LabelTable.row_of order)
    against the split's labels: what evaluate_python returns for the result files of the same rows.  ONE PR table serves every metric."""
    metrics = list(metrics)
    for metric in metrics:
        if metric not in ("R40", "R11"):
            raise ValueError(metric)
    if valid.shape[0] != len(label_table):
        raise ValueError("need one detection record array per ground-truth image")
    codes, mo = _class_overlaps(classes)
    device = det.device
    gt = label_table.on(device)
    dt, dt_off, pair_off, n_dt, n_pairs, aos = pack_detections(gt["gt_off"], det, valid, method)
    dev = _upload(dict(classes=np.asarray(codes, dtype=np.int32), min_overlaps=np.ascontiguousarray(mo, dtype=np.float64)), device)
    dev.update(gt=gt["gt"], gt_off=gt["gt_off"], dt=dt, dt_off=dt_off, pair_off=pair_off)
    sz = dict(B=len(label_table), n_gt=int(label_table.gt_off[-1]), n_dt=n_dt, n_pairs=n_pairs, num_classes=len(codes), num_k=int(mo.shape[0]))
    pr, num_th, _ = _launch_pr(dev, sz, aos, device)
    shape = (len(codes), 3, 3, int(mo.shape[0]))
    pr, num_th = pr.cpu().numpy().reshape(shape + (PTS, 4)), num_th.cpu().numpy().reshape(shape)
    return [_report(pr, num_th, aos, codes, mo, metric) for metric in metrics]
