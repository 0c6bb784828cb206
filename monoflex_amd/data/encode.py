"""Device-side sample encoding: the ctypes front of mfx_kitti_encode_targets[_views|_cfg] / mfx_kitti_preprocess_u8[_bgr].

Replaces the numeric half of the reference's KITTIDataset.__getitem__ (data/datasets/kitti.py:231-525), its flip
augmentation (data/augmentations/augmentations.py:33-78) and ToTensor+Normalize (data/transforms/transforms.py:15-31):
one launch pair encodes the targets of a whole batch, one launch converts its frames.  Inputs travel as a single pinned
host buffer per call; nothing is synchronised unless the caller asks for the status check."""
import ctypes

import numpy as np
import torch

from .. import lib as L
from .datasets.kitti_utils import RECORD_WIDTH

# target field -> (descriptor member, trailing shape (M = max_objs, C/H/W = heat map, E = edge slots), dtype)
TARGET_FIELDS = {
    "hm": ("hm", ("C", "H", "W"), torch.float32),
    "cls_ids": ("cls_ids", ("M",), torch.int32),
    "target_centers": ("target_centers", ("M", 2), torch.int32),
    "keypoints": ("keypoints", ("M", 10, 3), torch.float32),
    "keypoints_depth_mask": ("keypoints_depth_mask", ("M", 3), torch.float32),
    "dimensions": ("dimensions", ("M", 3), torch.float32),
    "locations": ("locations", ("M", 3), torch.float32),
    "reg_mask": ("reg_mask", ("M",), torch.uint8),
    "reg_weight": ("reg_weight", ("M",), torch.float32),
    "offset_3D": ("offset_3D", ("M", 2), torch.float32),
    "2d_bboxes": ("bboxes", ("M", 4), torch.float32),
    "gt_bboxes": ("gt_bboxes", ("M", 4), torch.float32),
    "rotys": ("rotys", ("M",), torch.float32),
    "trunc_mask": ("trunc_mask", ("M",), torch.uint8),
    "alphas": ("alphas", ("M",), torch.float32),
    "orientations": ("orientations", ("M", 8), torch.float32),
    "occlusions": ("occlusions", ("M",), torch.float64),
    "truncations": ("truncations", ("M",), torch.float64),
    "pad_size": ("pad_size", (2,), torch.int64),
    "edge_indices": ("edge_indices", ("E", 2), torch.int64),
    "edge_len": ("edge_len", (), torch.int64),
    "P": ("P_out", (3, 4), torch.float64),
    "heat_radius": ("heat_radius", ("M", 4), torch.int32),
    "status": ("status", (), torch.int32),
}
STATUS_MESSAGES = {1: "more objects of the detect classes than DATASETS.MAX_OBJECTS",
                   2: "truncated object whose 2D box centre lies outside the image (the reference fails on it)",
                   4: "truncated object: the centre line meets no image border",
                   8: "boundary heat map with both radii > 0",
                   16: "store row outside the resident store (mfx_kitti_encode_targets_indexed)"}


class EncodeParams:
    """The dataset settings the encoder depends on (reference KITTIDataset.__init__, kitti.py:60-98). The defaults are the
    runs/monoflex.yaml values. consider_outside_objs / adjust_boundary_heatmap / keypoint_visible_modify / heatmap_center are
    DATASETS.CONSIDER_OUTSIDE_OBJS, INPUT.ADJUST_BOUNDARY_HEATMAP, INPUT.KEYPOINT_VISIBLE_MODIFY, INPUT.HEATMAP_CENTER;
    to_bgr is INPUT.TO_BGR and concerns the frames only."""

    def __init__(self, in_w=1280, in_h=384, down=4, max_objs=40, num_classes=3, filter_annos=(0.9, 20.0), filter_enable=True,
                 edge_ratio=0.5, consider_outside_objs=True, adjust_boundary_heatmap=True, keypoint_visible_modify=True,
                 heatmap_center="3D", to_bgr=False):
        self.in_w, self.in_h, self.down, self.max_objs, self.num_classes = in_w, in_h, down, max_objs, num_classes
        self.filter_trunc = float(filter_annos[0]) if filter_enable else -1.0
        self.filter_size = float(filter_annos[1])
        self.edge_ratio = float(edge_ratio)
        if heatmap_center not in ("3D", "2D"):
            raise ValueError("INPUT.HEATMAP_CENTER is '3D' or '2D', got %r" % (heatmap_center,))
        self.consider_outside_objs, self.adjust_boundary_heatmap = bool(consider_outside_objs), bool(adjust_boundary_heatmap)
        self.keypoint_visible_modify, self.heatmap_center, self.to_bgr = bool(keypoint_visible_modify), heatmap_center, bool(to_bgr)
        if heatmap_center == "2D" and self.consider_outside_objs and self.adjust_boundary_heatmap:
            raise NotImplementedError(
                "INPUT.HEATMAP_CENTER '2D' with DATASETS.CONSIDER_OUTSIDE_OBJS and INPUT.ADJUST_BOUNDARY_HEATMAP both on: the "
                "reference draws the edge heat map around a centre in the middle of the box, where both radii are positive, and "
                "fails its assertion on all but the smallest truncated objects; switch one of the two off")

    def is_yaml(self):
        """True when the four encoder switches have their runs/monoflex.yaml values (the plain entries serve those)."""
        return (self.consider_outside_objs and self.adjust_boundary_heatmap and self.keypoint_visible_modify
                and self.heatmap_center == "3D")

    def encode_cfg(self):
        return L.KittiEncodeCfg(int(self.consider_outside_objs), int(self.adjust_boundary_heatmap),
                                int(self.keypoint_visible_modify), int(self.heatmap_center == "2D"))

    @classmethod
    def from_cfg(cls, cfg):
        """Refuses, with the reason, what the reference itself cannot run (it raises while encoding) and the one orientation
        code that is not built; the '2D'-centre edge heat map is refused by the constructor."""
        unsupported = []
        if cfg.INPUT.APPROX_3D_CENTER != "intersect":
            unsupported.append("INPUT.APPROX_3D_CENTER != 'intersect' (the reference raises NotImplementedError for any other mode)")
        if cfg.INPUT.ORIENTATION == "head-axis":
            unsupported.append("INPUT.ORIENTATION 'head-axis' (the reference writes eight values into a three-wide row and fails on "
                               "the first kept object)")
        elif cfg.INPUT.ORIENTATION != "multi-bin":
            unsupported.append("INPUT.ORIENTATION %r (only 'multi-bin' is encoded)" % (cfg.INPUT.ORIENTATION,))
        if cfg.INPUT.ORIENTATION_BIN_SIZE != 4:
            unsupported.append("INPUT.ORIENTATION_BIN_SIZE != 4 (the encoder and the heads are built for four bins)")
        if unsupported:
            raise NotImplementedError("the device target encoder does not serve: " + "; ".join(unsupported))
        return cls(cfg.INPUT.WIDTH_TRAIN, cfg.INPUT.HEIGHT_TRAIN, cfg.MODEL.BACKBONE.DOWN_RATIO, cfg.DATASETS.MAX_OBJECTS,
                   len(cfg.DATASETS.DETECT_CLASSES), tuple(cfg.DATASETS.FILTER_ANNOS), bool(cfg.DATASETS.FILTER_ANNO_ENABLE),
                   cfg.INPUT.HEATMAP_RATIO, bool(cfg.DATASETS.CONSIDER_OUTSIDE_OBJS), bool(cfg.INPUT.ADJUST_BOUNDARY_HEATMAP),
                   bool(cfg.INPUT.KEYPOINT_VISIBLE_MODIFY), cfg.INPUT.HEATMAP_CENTER, bool(cfg.INPUT.TO_BGR))

    def dims(self):
        out_w, out_h = self.in_w // self.down, self.in_h // self.down
        return {"M": self.max_objs, "C": self.num_classes, "H": out_h, "W": out_w, "E": 2 * (out_w + out_h)}


def pack_inputs(records, Ps, sizes, flips, params):
    """Host-side packing of one batch: list of (n_i,14) record arrays, (3,4) matrices, (w,h) sizes, flip flags ->
    dict of numpy arrays in the descriptor's input layout. Raises when a sample has more objects than MAX_OBJECTS
    (the reference overruns its fixed-size arrays there)."""
    B, M = len(records), params.max_objs
    rec = np.zeros((B, M, RECORD_WIDTH), dtype=np.float64)
    n_obj = np.zeros(B, dtype=np.int32)
    for b, r in enumerate(records):
        r = np.asarray(r, dtype=np.float64).reshape(-1, RECORD_WIDTH)
        if r.shape[0] > M:
            raise IndexError("sample %d has %d objects of the detect classes, DATASETS.MAX_OBJECTS is %d" % (b, r.shape[0], M))
        rec[b, :r.shape[0]] = r
        n_obj[b] = r.shape[0]
    return dict(records=rec, n_obj=n_obj, P=np.asarray(Ps, dtype=np.float64).reshape(B, 3, 4).copy(),
                img_wh=np.asarray(sizes, dtype=np.int32).reshape(B, 2).copy(), flip=np.asarray(flips, dtype=np.int32).reshape(B).copy())


def _align16(n):
    return (n + 15) // 16 * 16


def _upload(arrays, device):
    """Several small numpy arrays -> one pinned buffer -> one async copy; returns device views in the original dtypes."""
    total = sum(_align16(a.nbytes) for a in arrays.values())
    host = torch.empty(total, dtype=torch.uint8, pin_memory=True)
    hn, views, off = host.numpy(), {}, 0
    for k, a in arrays.items():
        hn[off:off + a.nbytes] = np.ascontiguousarray(a).view(np.uint8).reshape(-1)
        views[k] = (off, a.shape, a.dtype)
        off += _align16(a.nbytes)
    dev = host.to(device, non_blocking=True)
    return {k: _view(dev, o, shape, getattr(torch, np.dtype(dt).name)) for k, (o, shape, dt) in views.items()}


def _view(buf, offset, shape, dtype):
    n = int(np.prod(shape, dtype=np.int64)) * torch.empty((), dtype=dtype).element_size()
    return buf[offset:offset + n].view(dtype).view(*shape)


def _alloc_outputs(B, dims, device):
    """All output fields as views of one device allocation (one allocator call per batch instead of 24)."""
    specs, total = {}, 0
    for name, (_, shape, dt) in TARGET_FIELDS.items():
        full = (B,) + tuple(dims.get(s, s) for s in shape)
        specs[name] = (total, full, dt)
        total += _align16(int(np.prod(full, dtype=np.int64)) * torch.empty((), dtype=dt).element_size())
    buf = torch.empty(total, dtype=torch.uint8, device=device)
    return {name: _view(buf, o, full, dt) for name, (o, full, dt) in specs.items()}


class PreparedEncode:
    """One batch ready to launch: inputs uploaded, outputs allocated, descriptor filled. `launch()` enqueues the two encoder
    kernels on the current stream and may be repeated (the timing tools do); `out` is {field: (B, ...) device tensor}.
    With every switch of `params` at its yaml value the plain entries are called; otherwise mfx_kitti_encode_targets_cfg."""

    def __init__(self, records, Ps, sizes, flips, params, device, rights=None):
        self.lib, self.device = L.load(), device
        arrays = pack_inputs(records, Ps, sizes, flips, params)
        B, dims = len(records), params.dims()
        if rights is not None:
            arrays["right"] = np.asarray(rights, dtype=np.int32).reshape(B).copy()      # rides in the same pinned upload as `flip`
        self.inp = _upload(arrays, device)
        self.right = self.inp.pop("right", None)
        self.out = _alloc_outputs(B, dims, device)
        d = self.desc = L.KittiDesc()
        for k, t in self.inp.items():
            setattr(d, k, t.data_ptr())
        for name, (member, _, _) in TARGET_FIELDS.items():
            setattr(d, member, self.out[name].data_ptr())
        d.B, d.max_objs, d.in_w, d.in_h, d.down, d.num_classes = B, params.max_objs, params.in_w, params.in_h, params.down, params.num_classes
        d.filter_trunc, d.filter_size, d.edge_ratio = params.filter_trunc, params.filter_size, params.edge_ratio
        self.cfg = None if params.is_yaml() else params.encode_cfg()

    def launch(self):
        with torch.cuda.device(self.device):
            stream = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
            if self.cfg is not None:
                L.check(self.lib.mfx_kitti_encode_targets_cfg(ctypes.byref(self.desc), None if self.right is None else self.right.data_ptr(),
                                                              ctypes.byref(self.cfg), stream), "mfx_kitti_encode_targets_cfg")
            elif self.right is None:
                L.check(self.lib.mfx_kitti_encode_targets(ctypes.byref(self.desc), stream), "mfx_kitti_encode_targets")
            else:
                L.check(self.lib.mfx_kitti_encode_targets_views(ctypes.byref(self.desc), self.right.data_ptr(), stream),
                        "mfx_kitti_encode_targets_views")


def encode_targets(records, Ps, sizes, flips, params, device, check=True, rights=None):
    """Batch of raw labels -> {field: (B, ...) device tensor} with every field of the reference's training target
    (kitti.py:496-523; "calib" is left to the caller, "P" is the camera matrix after the flip).
    rights: per-sample flags, 1 = right-camera view (DATASETS.USE_RIGHT_IMAGE, kitti.py:232-252): `Ps` holds P3 for that
    sample and its 2D boxes are regenerated from the 3D corners (mfx_kitti_encode_targets_views). None = all left views.
    check=True synchronises once to turn a non-zero status into the exception the reference would have raised."""
    if torch.device(device).type != "cuda":
        raise RuntimeError("encode_targets runs on the GPU (HIP kernels); there is no CPU fallback")
    prepared = PreparedEncode(records, Ps, sizes, flips, params, device, rights)
    prepared.launch()
    if check:
        check_status(prepared.out["status"])
    return prepared.out


def check_status(status, ids=None):
    """ids: the sample ids of the batch, named in the message when given."""
    bad = torch.nonzero(status).flatten().tolist()
    if bad:
        code = int(status[bad[0]])
        msgs = [m for bit, m in STATUS_MESSAGES.items() if code & bit]
        who = "" if ids is None else " (id %s)" % (ids[bad[0]],)
        raise ValueError("target encoding failed for sample %d of the batch%s: %s" % (bad[0], who, "; ".join(msgs)))


def preprocess_images(frames, flips, params, device, mean=(0.485, 0.456, 0.406), std=(0.229, 0.224, 0.225)):
    """List of (h_i, w_i, 3) uint8 RGB frames (numpy) -> (B, 3, in_h, in_w) float32 device tensor: flip, centre zero padding,
    /255, (x - mean) / std (kitti.py:218-228, transforms.py:15-31). params.to_bgr (INPUT.TO_BGR): the normalised channels
    are then stored in B, G, R order (mfx_kitti_preprocess_u8_bgr); mean / std stay in RGB order."""
    if torch.device(device).type != "cuda":
        raise RuntimeError("preprocess_images runs on the GPU (HIP kernel); there is no CPU fallback")
    lib = L.load()
    B = len(frames)
    sizes = np.zeros((B, 2), dtype=np.int32)
    offsets = np.zeros(B, dtype=np.int64)
    total = 0
    for b, f in enumerate(frames):
        if f.dtype != np.uint8 or f.ndim != 3 or f.shape[2] != 3:
            raise ValueError("frame %d: expected (h, w, 3) uint8, got %s %s" % (b, f.shape, f.dtype))
        if f.shape[0] > params.in_h or f.shape[1] > params.in_w:
            raise ValueError("frame %d (%dx%d) is larger than the network input %dx%d"
                             % (b, f.shape[1], f.shape[0], params.in_w, params.in_h))
        sizes[b] = (f.shape[1], f.shape[0])
        offsets[b] = total
        total += _align16(f.size)
    host = torch.empty(total, dtype=torch.uint8, pin_memory=True)
    hn = host.numpy()
    for b, f in enumerate(frames):
        hn[offsets[b]:offsets[b] + f.size] = f.reshape(-1)
    pixels = host.to(device, non_blocking=True)
    meta = _upload(dict(offsets=offsets, img_wh=sizes, flip=np.asarray(flips, dtype=np.int32).reshape(B).copy()), device)
    out = torch.empty((B, 3, params.in_h, params.in_w), dtype=torch.float32, device=device)
    m3, s3 = (ctypes.c_float * 3)(*mean), (ctypes.c_float * 3)(*std)
    with torch.cuda.device(device):
        stream = torch.cuda.current_stream().cuda_stream
        name = "mfx_kitti_preprocess_u8_bgr" if params.to_bgr else "mfx_kitti_preprocess_u8"
        L.check(getattr(lib, name)(pixels.data_ptr(), meta["offsets"].data_ptr(), meta["img_wh"].data_ptr(),
                                   meta["flip"].data_ptr(), out.data_ptr(), B, params.in_w, params.in_h, m3, s3,
                                   ctypes.c_void_p(stream)), name)
    return out
