"""Shared by the CPU and GPU tests of the target encoder's other settings (DATASETS.CONSIDER_OUTSIDE_OBJS,
INPUT.ADJUST_BOUNDARY_HEATMAP, INPUT.KEYPOINT_VISIBLE_MODIFY, INPUT.HEATMAP_CENTER, INPUT.TO_BGR): the reference's goldens
under each setting (tests/golden/kitti_encode_settings.npz, recorded by tools/gen_encode_settings_golden.py), a numpy
restatement of the encoder with the settings on top of oracle/kitti_encode_ref.py, and the host build of the device functions
with the settings.  Comparison rules are those of tests/kitti_common.py; nothing here adds a tolerance.  The restatement is
pinned to the fixture in tests/test_kitti_encode_settings_cpu.py before anything else relies on it."""
import ctypes
import os
import subprocess

import numpy as np
import torch

from monoflex_amd import lib as L
from monoflex_amd import synthetic as S
from monoflex_amd.data import encode as E
from monoflex_amd.data.datasets import kitti_utils as KU
from oracle import kitti_encode_ref as K
from tests.kitti_common import GOLD, NAMES, golden_sample

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLD_S = np.load(os.path.join(ROOT, "tests", "golden", "kitti_encode_settings.npz"))
CLASSES = ("Car", "Pedestrian", "Cyclist")
NP_DTYPES = {torch.float32: np.float32, torch.float64: np.float64, torch.int32: np.int32, torch.int64: np.int64, torch.uint8: np.uint8}
ORACLE_ERRORS = (TypeError, ValueError, AssertionError, IndexError)

# servable settings: fixture name -> EncodeParams keywords (everything else as runs/monoflex.yaml)
SETTINGS = {
    "no_outside": dict(consider_outside_objs=False),
    "circular": dict(adjust_boundary_heatmap=False),
    "no_modify": dict(keypoint_visible_modify=False),
    "center2d_circular": dict(heatmap_center="2D", adjust_boundary_heatmap=False),
    "center2d_no_outside": dict(heatmap_center="2D", consider_outside_objs=False),
    "defaults": dict(consider_outside_objs=False, adjust_boundary_heatmap=False, keypoint_visible_modify=False, filter_enable=False),
}
REFUSED = "center2d_edge"                       # '2D' centre with the edge heat map: the reference asserts; Python refuses it
# kept / truncated objects of s00..s11 as the reference gives them (run of its KITTIDataset, one override at a time)
YAML_KEPT, YAML_TRUNC = [4, 0, 9, 13, 7, 0, 25, 8, 3, 14, 6, 12], [0, 0, 2, 1, 1, 0, 4, 1, 1, 1, 1, 2]
NO_OUTSIDE_KEPT = [4, 0, 7, 12, 6, 0, 21, 7, 2, 13, 5, 10]
KEPT = {"no_outside": NO_OUTSIDE_KEPT, "circular": YAML_KEPT, "no_modify": YAML_KEPT, "center2d_circular": YAML_KEPT,
        "center2d_no_outside": NO_OUTSIDE_KEPT, "defaults": [4, 0, 7, 13, 6, 0, 21, 7, 2, 13, 5, 10]}
TRUNC = {"no_outside": [0] * 12, "circular": YAML_TRUNC, "no_modify": YAML_TRUNC, "center2d_circular": YAML_TRUNC,
         "center2d_no_outside": [0] * 12, "defaults": [0] * 12}
KEEPS_TRUNCATED = [s for s, kw in SETTINGS.items() if kw.get("consider_outside_objs", True)]
FUZZ_SEEDS = range(21000, 21036)                # fresh range (7000.. and 1000..1299 are used by the yaml and right-view tests)


def params_of(setting):
    return E.EncodeParams(**SETTINGS[setting])


def golden_raised(setting, name):
    return bool(int(GOLD_S["%s_%s_raised" % (setting, name)]))


def golden_fields(setting, name):
    """{field: array} of one recorded case under one setting; `hm` is rebuilt from the yaml heat map and the stored difference,
    the three fields no setting touches come from the yaml fixture."""
    key = "%s_%s_" % (setting, name)
    f = {str(k): GOLD_S[key + str(k)] for k in GOLD_S["fields"]}
    hm = GOLD[name + "_hm"].copy()
    hm.reshape(-1)[GOLD_S[key + "hm_idx"]] = GOLD_S[key + "hm_val"]
    f["hm"] = hm
    for k in ("pad_size", "edge_len", "edge_indices"):
        f[k] = GOLD[name + "_" + k]
    return f


def encode_sample_cfg(lines, P, img_w, img_h, do_flip=False, consider_outside_objs=True, adjust_boundary_heatmap=True,
                      keypoint_visible_modify=True, heatmap_center="3D", filter_enable=True, in_w=1280, in_h=384, down=4,
                      max_objs=40, filter_annos=(0.9, 20), edge_ratio=0.5):
    """oracle.kitti_encode_ref.encode_sample with the four switches and FILTER_ANNO_ENABLE (reference kitti.py:335-489).
    The box keeps its dtype (float32 label box / float64 projected box) through the '2D' centre's round()."""
    P = np.asarray(P, dtype=np.float64).reshape(3, 4)
    objs = K.read_objects(lines)
    if do_flip:
        P = K.flip(objs, P, img_w)
    pad = K.pad_size(img_w, img_h, in_w, in_h)
    out_w, out_h = in_w // down, in_h // down
    x_min, y_min = int(np.ceil(pad[0] / down)), int(np.ceil(pad[1] / down))
    x_max, y_max = (pad[0] + img_w - 1) // down, (pad[1] + img_h - 1) // down
    ei, el = K.edge_indices(img_w, img_h, pad, down, (out_w + out_h) * 2)
    f = dict(hm=np.zeros((3, out_h, out_w), np.float32), cls_ids=np.zeros(max_objs, np.int32),
             target_centers=np.zeros((max_objs, 2), np.int32), gt_bboxes=np.zeros((max_objs, 4), np.float32),
             keypoints=np.zeros((max_objs, 10, 3), np.float32), keypoints_depth_mask=np.zeros((max_objs, 3), np.float32),
             dimensions=np.zeros((max_objs, 3), np.float32), locations=np.zeros((max_objs, 3), np.float32),
             rotys=np.zeros(max_objs, np.float32), alphas=np.zeros(max_objs, np.float32),
             offset_3D=np.zeros((max_objs, 2), np.float32), occlusions=np.zeros(max_objs), truncations=np.zeros(max_objs),
             orientations=np.zeros((max_objs, 8), np.float32), reg_mask=np.zeros(max_objs, np.uint8),
             trunc_mask=np.zeros(max_objs, np.uint8), reg_weight=np.zeros(max_objs, np.float32))
    f["2d_bboxes"] = np.zeros((max_objs, 4), np.float32)
    if len(objs) > max_objs:
        raise IndexError("more than MAX_OBJECTS=%d objects of the detect classes" % max_objs)
    for i, o in enumerate(objs):
        cls_id = K.TYPE_ID[o.type]
        locs = o.t.copy()
        locs[1] = locs[1] - o.h / 2
        if locs[-1] <= 0:
            continue
        c3 = K.corners3d(o)
        c2, _ = K.project(P, c3)
        pbox = np.array([c2[:, 0].min(), c2[:, 1].min(), c2[:, 0].max(), c2[:, 1].max()])
        if pbox[0] >= 0 and pbox[1] >= 0 and pbox[2] <= img_w - 1 and pbox[3] <= img_h - 1:
            box = pbox.copy()                                        # float64
        else:
            box = o.box2d.copy()                                     # float32
        if filter_enable and o.truncation >= filter_annos[0] and (box[2:] - box[:2]).min() <= filter_annos[1]:
            continue
        pc, _ = K.project(P, locs.reshape(-1, 3))
        pc = pc[0]
        inside = (0 <= pc[0] <= img_w - 1) and (0 <= pc[1] <= img_h - 1)
        approx = False
        if not inside:
            if not consider_outside_objs:
                continue                                             # kitti.py:393-394, before approx_proj_center
            approx = True
            tpc = K.intersect_center(pc, (box[:2] + box[2:]) / 2, img_w, img_h)
            if tpc is None:
                raise TypeError("truncated object whose 2D box centre is outside the image")
        else:
            tpc = pc.copy()
        k3 = np.concatenate((c3, np.stack((c3[:4].mean(axis=0), c3[4:].mean(axis=0)))), axis=0)
        k2, _ = K.project(P, k3)
        vis = (k2[:, 0] >= 0) & (k2[:, 0] <= img_w - 1) & (k2[:, 1] >= 0) & (k2[:, 1] <= img_h - 1) & (k3[:, -1] > 0)
        if keypoint_visible_modify:
            vis = np.append(np.tile(vis[:4] | vis[4:8], 2), np.tile(vis[8] | vis[9], 2))
        dvalid = np.stack((vis[[8, 9]].all(), vis[[0, 2, 4, 6]].all(), vis[[1, 3, 5, 7]].all()))
        k2 = (k2 + pad.reshape(1, 2)) / down
        tpc = (tpc + pad) / down
        pc = (pc + pad) / down
        box[0::2] += pad[0]
        box[1::2] += pad[1]
        box /= down
        bcenter = (box[:2] + box[2:]) / 2                            # dtype of the box
        assert bcenter.dtype == box.dtype
        bdim = box[2:] - box[:2]
        tc = (bcenter.round() if heatmap_center == "2D" else tpc.round()).astype(int)
        tc[0] = np.clip(tc[0], x_min, x_max)
        tc[1] = np.clip(tc[1], y_min, y_max)
        pred_2d = tc[0] >= box[0] and tc[1] >= box[1] and tc[0] <= box[2] and tc[1] <= box[3]
        if (bdim > 0).all() and 0 <= tc[0] <= out_w - 1 and 0 <= tc[1] <= out_h - 1:
            if adjust_boundary_heatmap and approx:
                bw = min(tc[0] - box[0], box[2] - tc[0])
                bh = min(tc[1] - box[1], box[3] - tc[1])
                rx, ry = max(0, int(bw * edge_ratio)), max(0, int(bh * edge_ratio))
                assert min(rx, ry) == 0
                K.draw_gaussian(f["hm"][cls_id], int(tc[0]), int(tc[1]), rx, ry, circular=False)
            else:
                r = max(0, int(K.gaussian_radius(bdim[1], bdim[0])))
                K.draw_gaussian(f["hm"][cls_id], int(tc[0]), int(tc[1]), r, r, circular=True)
            f["cls_ids"][i] = cls_id
            f["target_centers"][i] = tc
            f["offset_3D"][i] = pc - tc
            f["gt_bboxes"][i] = o.box2d
            if pred_2d:
                f["2d_bboxes"][i] = box
            f["keypoints"][i] = np.concatenate((k2 - tc.reshape(1, -1), vis[:, None].astype(np.float32)), axis=1)
            f["keypoints_depth_mask"][i] = dvalid
            f["dimensions"][i] = (o.l, o.h, o.w)
            f["locations"][i] = locs
            f["rotys"][i], f["alphas"][i] = o.ry, o.alpha
            f["orientations"][i] = K.multibin(o.alpha)
            f["reg_mask"][i], f["reg_weight"][i], f["trunc_mask"][i] = 1, 1, int(approx)
            f["occlusions"][i], f["truncations"][i] = float(o.occlusion), o.truncation
    f.update(pad_size=pad, edge_indices=ei, edge_len=el, P=P, size=np.array([in_w, in_h]))
    return f


def restated(setting, lines, w, h, flip, P=S.KITTI_P2):
    """Restatement under a setting of SETTINGS, or None where the reference itself fails."""
    try:
        return encode_sample_cfg(lines, P, w, h, do_flip=flip, **SETTINGS[setting])
    except ORACLE_ERRORS:
        return None


def build_cfg_shim(directory):
    """Compiles tests/shim/kitti_encode_cfg_host.cpp (-ffp-contract=off, like the device build) -> ctypes library."""
    so = os.path.join(str(directory), "libkitti_cfg_shim.so")
    cmd = ["g++", "-O2", "-std=c++17", "-ffp-contract=off", "-shared", "-fPIC", "-o", so,
           os.path.join(ROOT, "tests", "shim", "kitti_encode_cfg_host.cpp")]
    r = subprocess.run(cmd, capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    lib = ctypes.CDLL(so)
    lib.shim_kitti_encode_cfg.argtypes = [ctypes.POINTER(L.KittiDesc), ctypes.c_void_p, ctypes.POINTER(L.KittiEncodeCfg)]
    lib.shim_kitti_encode_cfg.restype = None
    lib.shim_kitti_preprocess_bgr.argtypes = [ctypes.c_void_p] * 5 + [ctypes.c_int] * 3 + [ctypes.c_void_p] * 2 + [ctypes.c_int]
    lib.shim_kitti_preprocess_bgr.restype = None
    lib.shim_sizeof_encode_cfg.restype = ctypes.c_int
    lib.shim_fill_encode_cfg.argtypes = [ctypes.POINTER(L.KittiEncodeCfg)]
    lib.shim_fill_encode_cfg.restype = None
    return lib


def shim_encode_records(shim, records, Ps, sizes, flips, params, rights=None, cfg="params"):
    """Host twin of monoflex_amd.data.encode.encode_targets: same packing, same descriptor, the device functions compiled for
    the CPU.  cfg: "params" = the switches of `params`, None = a NULL pointer, or a KittiEncodeCfg."""
    inp = E.pack_inputs(records, Ps, sizes, flips, params)
    dims, B = params.dims(), len(records)
    out = {name: np.full((B,) + tuple(dims.get(s, s) for s in shape), 77, dtype=NP_DTYPES[dt])      # poison: every element must be written
           for name, (_, shape, dt) in E.TARGET_FIELDS.items()}
    d = L.KittiDesc()
    for k, a in inp.items():
        setattr(d, k, a.ctypes.data)
    for name, (member, _, _) in E.TARGET_FIELDS.items():
        setattr(d, member, out[name].ctypes.data)
    d.B, d.max_objs, d.in_w, d.in_h, d.down, d.num_classes = B, params.max_objs, params.in_w, params.in_h, params.down, params.num_classes
    d.filter_trunc, d.filter_size, d.edge_ratio = params.filter_trunc, params.filter_size, params.edge_ratio
    right = None if rights is None else np.asarray(rights, dtype=np.int32).reshape(B).copy()
    c = params.encode_cfg() if isinstance(cfg, str) else cfg
    shim.shim_kitti_encode_cfg(ctypes.byref(d), None if right is None else right.ctypes.data, None if c is None else ctypes.byref(c))
    return out


def run_cfg_shim(shim, samples, params, cfg="params"):
    """samples: [(lines, w, h, flip)] -> {field: (B, ...) numpy}, all left views through KITTI_P2."""
    recs = [KU.read_label_records(lines, CLASSES) for lines, _, _, _ in samples]
    return shim_encode_records(shim, recs, [S.KITTI_P2] * len(samples), [(w, h) for _, w, h, _ in samples],
                               [f for _, _, _, f in samples], params, cfg=cfg)


def shim_frames(shim, frames, flips, to_bgr, in_w=1280, in_h=384, mean=K.PIXEL_MEAN, std=K.PIXEL_STD):
    """preprocess_pixel of kitti_encode_math.h over a list of (h, w, 3) uint8 frames -> (B, 3, in_h, in_w) float32."""
    offsets = np.cumsum([0] + [f.size for f in frames[:-1]]).astype(np.int64)
    pixels = np.concatenate([np.ascontiguousarray(f).reshape(-1) for f in frames])
    wh = np.array([(f.shape[1], f.shape[0]) for f in frames], dtype=np.int32)
    fl = np.asarray([int(bool(v)) for v in flips], dtype=np.int32)
    out = np.full((len(frames), 3, in_h, in_w), 77, dtype=np.float32)
    m3 = np.asarray(mean, dtype=np.float32)
    s3 = np.asarray(std, dtype=np.float32)
    shim.shim_kitti_preprocess_bgr(pixels.ctypes.data, offsets.ctypes.data, wh.ctypes.data, fl.ctypes.data, out.ctypes.data,
                                   len(frames), in_w, in_h, m3.ctypes.data, s3.ctypes.data, int(to_bgr))
    return out


def bgr_frame(frame, flip):
    """The reference's TO_BGR frame: normalised in RGB order, then channels [2, 1, 0] (transforms.py:24-30)."""
    return K.transform_image(frame, do_flip=bool(flip))[[2, 1, 0]]


def assert_bgr_frame_is_the_recorded_one(image, name):
    flat = np.asarray(image, dtype=np.float64).ravel()
    np.testing.assert_allclose(flat[GOLD_S["bgr_%s_img_idx" % name]], GOLD_S["bgr_%s_img_samples" % name], rtol=0, atol=1e-6, err_msg=name)


def golden_frame(name):
    _, w, h, flip, iseed = golden_sample(name)
    return np.random.RandomState(iseed).randint(0, 256, (h, w, 3)).astype(np.uint8), flip


def defaults_cfg():
    """runs/monoflex.yaml model settings with the data settings of config/defaults.py (the three switches off, no annotation filter)."""
    from monoflex_amd.config import get_cfg
    cfg = get_cfg(os.path.join(ROOT, "runs", "monoflex.yaml"))
    cfg.merge_from_list([str(v) for v in GOLD_S["defaults_opts"]])
    return cfg
