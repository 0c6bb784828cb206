"""Seeded inputs of mfx_eval_diagnostics at small shapes (helper module, not a test file): the structured head maps of
tests/decode_cases.py (24 x 40 grid, four cameras with their own pad / calib, regression rows that reach every branch of the decode) and a
ground-truth table whose objects sit on pixels of those maps.  Plain numpy; needs only the CPU.  Read by tests/test_eval_diag_cpu.py,
tests/test_gpu_eval_diag.py and tools/gen_eval_diag_golden.py.

The target of an object is the float64 decode of the object's OWN row (under its class and the case's `mode`), perturbed: a per-object scale
s in [0, 1] times a shift of up to 0.6 of the box's footprint along x and z, 0.4 of its height along y, 40 % in each dimension and 0.5 rad of
yaw -- so that each of the five disentangled IoUs spreads over (0, 1) -- with a stated share of objects far from their prediction (IoU 0)
and a stated share identical to it.  A target is self-consistent, as a label is: its location is the projection of its own centre offset at
its own depth.  `shares` counts all this from the float64 restatement alone; the CPU tests assert it.
"""
import functools
import os

import numpy as np

from tests import decode_cases as C
from tests import decode_ref as D
from tests import eval_diag_ref as R

H, W = C.H, C.W
FAR_SHARE, SAME_SHARE = 0.10, 0.10

# images: indices into decode_cases.IMAGES; M: object slots per image; mode: the output_depth the targets are built around
CASES = {
    "b1_m1": dict(seed=31, images=(3,), M=1, ld=64, reg_off=8, mode="direct"),
    "b3_m40": dict(seed=32, images=(0, 1, 2), M=40, ld=64, reg_off=8, mode="direct"),
    "b4_m70": dict(seed=33, images=(0, 1, 2, 3), M=70, ld=64, reg_off=8, mode="soft"),
    "b4_m70_direct": dict(seed=34, images=(2, 3, 0, 1), M=70, ld=64, reg_off=8, mode="direct"),
    "b3_m70_ld50": dict(seed=35, images=(1, 2, 3), M=70, ld=50, reg_off=0, mode="hard"),
    "b4_m40_ld72": dict(seed=36, images=(3, 2, 1, 0), M=40, ld=72, reg_off=13, mode="keypoints_avg"),
    "b1_m70": dict(seed=37, images=(1,), M=70, ld=64, reg_off=8, mode="mean"),
}
SHARE_MIN_ROWS = C.CENSUS_MIN_ROWS       # the shares are asserted for every case with at least this many valid objects
# what tools/gen_eval_diag_golden.py records: six images, the targets of each built around another depth (`target_modes`), so that every
# estimate is close to its target's depth in a part of the objects -- where |estimate - Z| is small, the error of the estimate itself shows
GOLDEN = dict(seed=41, images=(0, 1, 2, 3, 0, 2), M=120, ld=64, reg_off=8, mode="direct",
              target_modes=("direct", "direct", "hard", "soft", "mean", "keypoints_avg"))


def build(c):
    """-> dict(hmap (B,H,W,ld), reg_off, calib (B,6), pad (B,2) int32, gt_rows (B,M,16) float32, mode, kind (B,M): 0 empty, 1 perturbed,
    2 far, 3 identical)."""
    m = C.structured_maps(c["seed"], c["images"], c["ld"], c["reg_off"])
    rng = np.random.default_rng(c["seed"] + 5000)
    B, M = len(c["images"]), c["M"]
    hmap, reg_off = m["hmap"], c["reg_off"]
    gt = np.zeros((B, M, R.GT_ROW), dtype=np.float64)
    kind = np.zeros((B, M), dtype=np.int64)
    for b in range(B):
        mask = rng.uniform(size=M) < 0.8                              # holes
        if M > 1:
            mask[0] = b % 2 == 1                                       # the first valid slot is not always slot 0
            mask[M - 1] = True                                         # the tail of the last workgroup is used
        else:
            mask[:] = True
        if B >= 3 and b == 1:
            mask[:] = False                                            # an image with no object
        cx, cy = rng.integers(0, W, M), rng.integers(0, H, M)
        if M >= 7:
            mask[5] = mask[6] = not (B >= 3 and b == 1)
            cx[6], cy[6] = cx[5], cy[5]                                # two objects share a centre pixel
        cls = rng.integers(0, 3, M)
        if M >= 7:
            cls[6] = (cls[5] + 1) % 3
        cam, pad = m["calib"][b].astype(np.float64), m["pad"][b].astype(np.float64)
        r = hmap[b].reshape(H * W, -1)[cy * W + cx, reg_off:reg_off + D.R_TOTAL].astype(np.float64)
        dec = R.decode_rows(r, cls, cam[0])
        depth = R.output_depth(dec, c["target_modes"][b] if "target_modes" in c else c["mode"])
        dims = dec["dims"]
        loc = R._location(cx.astype(np.float64), cy.astype(np.float64), r[:, D.R_OFF3D], r[:, D.R_OFF3D + 1], depth, cam, pad)
        ry = R._wrap(dec["alpha_raw"] + np.arctan2(loc[:, 0], loc[:, 2]))
        what = rng.uniform(size=M)
        k = np.where(what < FAR_SHARE, 2, np.where(what < FAR_SHARE + SAME_SHARE, 3, 1))
        s = rng.uniform(0, 1, M) * (k == 1) + 6.0 * (k == 2)           # far: six footprints away
        un = lambda: rng.uniform(-1, 1, M)
        foot = np.minimum(dims[:, 0], dims[:, 2])
        far_sign = np.where(un() < 0, -1.0, 1.0)
        jitter = lambda: np.where(k == 2, far_sign, un())
        t_depth = np.maximum(depth + s * jitter() * 0.6 * foot, 0.05)
        # a shift of the projected centre by dx metres at the target's depth is dx f / (Z down_ratio) cells
        t_offx = r[:, D.R_OFF3D] + s * jitter() * 0.6 * foot * cam[0] / (t_depth * 4.0)
        t_offy = r[:, D.R_OFF3D + 1] + np.minimum(s, 1.0) * un() * 0.4 * dims[:, 1] * cam[1] / (t_depth * 4.0)
        t_dims = dims * (1 + 0.4 * np.minimum(s, 1.0)[:, None] * rng.uniform(-1, 1, (M, 3)))
        t_ry = ry + 0.5 * np.minimum(s, 1.0) * un()
        # the values a label file holds are float32: round the independent quantities, then derive the location from them
        t_offx, t_offy, t_depth = (v.astype(np.float32).astype(np.float64) for v in (t_offx, t_offy, t_depth))
        t_loc = R._location(cx.astype(np.float64), cy.astype(np.float64), t_offx, t_offy, t_depth, cam, pad)
        rows = np.concatenate((mask[:, None].astype(np.float64), cls[:, None].astype(np.float64), cx[:, None].astype(np.float64),
                               cy[:, None].astype(np.float64), t_offx[:, None], t_offy[:, None], t_loc, t_dims, t_ry[:, None], np.zeros((M, 3))), axis=1)
        rows[~mask, 1:] = rng.normal(0, 5, (int((~mask).sum()), R.GT_ROW - 1))      # an empty slot holds noise: it must not be read
        gt[b] = rows
        kind[b] = np.where(mask, k, 0)
    gt32 = gt.astype(np.float32)
    return dict(hmap=hmap, reg_off=reg_off, ld=c["ld"], calib=m["calib"], pad=m["pad"], gt_rows=np.ascontiguousarray(gt32), mode=c["mode"],
                kind=kind, images=tuple(c["images"]))


def case_inputs(name):
    return build(CASES[name])


def golden_inputs():
    return build(GOLDEN)


def run_ref(d, mode=None, with_iou=True):
    return R.evaluate(d["hmap"], d["reg_off"], d["gt_rows"], d["calib"], d["pad"], mode or d["mode"], with_iou=with_iou)


def shares(d, ref):
    """Of the valid objects of a case under its own mode -> {name: share}: per IoU key the share inside (0.05, 0.95), the share with
    pred_IoU exactly 0 and the share with pred_IoU above 0.95 among the identical ones."""
    v = ref["valid"]
    iou = ref["iou"][v]
    out = {"%s in (0.05, 0.95)" % k: float(np.mean((iou[:, i] > 0.05) & (iou[:, i] < 0.95))) for i, k in enumerate(R.IOU_KEYS)}
    out["pred_IoU == 0"] = float(np.mean(iou[:, 0] == 0.0))
    out["offset_IoU == 0"] = float(np.mean(iou[:, 1] == 0.0))
    out["depth_IoU == 0"] = float(np.mean(iou[:, 2] == 0.0))
    same = d["kind"][v] == 3
    out["identical objects"] = float(np.mean(same))
    out["identical objects with every IoU > 0.999"] = float(np.mean((iou[same] > 0.999).all(axis=1))) if same.any() else 0.0
    return out


def census_lists(d, ncls=3):
    """Per-class lists (B, 3, M) for tests/decode_ref.py / ops.decode_boxes whose merged top-M of image b is exactly (slot 0's pixel under slot
    0's class, slot 1's ..., ...): slot m's pixel carries the score 0.9 - m / 1000 in the list of its class and a score below 0.05 in the two
    others.  An empty slot stands in with pixel 0, class 0.  Row j of the decode is then slot j, decoded at that pixel under that class."""
    gt = d["gt_rows"]
    B, M = gt.shape[:2]
    valid = gt[..., R.G_MASK] != 0
    cls = np.where(valid, gt[..., R.G_CLS], 0).astype(np.int64) % ncls          # (ncls < 3: the classes are folded, as the caller folds them)
    pix = np.where(valid, gt[..., R.G_CY] * W + gt[..., R.G_CX], 0).astype(np.int32)
    scores = np.zeros((B, ncls, M), dtype=np.float32)
    for c in range(ncls):
        low = 0.04 - (np.arange(M) * 3 + c) * 1e-4
        scores[:, c] = np.where(cls == c, 0.9 - np.arange(M)[None, :] * 1e-3, low[None, :])
    index = np.ascontiguousarray(np.broadcast_to(pix[:, None, :], (B, ncls, M)))
    return np.ascontiguousarray(scores), index


# ---- helpers shared by tests/test_eval_diag_cpu.py and tests/test_gpu_eval_diag.py ----------------------------------------------------------
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@functools.lru_cache(maxsize=None)
def golden():
    return np.load(os.path.join(ROOT, "tests", "golden", "eval_diag.npz"), allow_pickle=False)


def yaml_cfg(mode):
    """mfx_decode_cfg of runs/monoflex.yaml with output_depth `mode`."""
    from monoflex_amd import lib as L
    from tests import head_sets_cases as HC
    return L.decode_cfg(L.head_decode_settings(HC.cfg_for("s111")), True, mode)


def full_layout():
    from monoflex_amd import lib as L
    from tests import head_sets_ref as HS
    return L.HeadSet(HS.SETS["s111"], HS.channels("s111")).layout()


def golden_tables(mode):
    """The golden's per-image vectors scattered into fixed-shape tables -> (depth_err (B, M, 13), boxes (B, M, 6, 7) or None)."""
    d = golden_inputs()
    valid = d["gt_rows"][..., 0] != 0
    B, M = valid.shape
    de, bx = np.zeros((B, M, 13)), np.zeros((B, M, 6, 7))
    for b in range(B):
        if not valid[b].any():
            assert "boxes_img%d" % b not in golden().files
            continue
        de[b, valid[b]] = np.stack([golden()["depth_%s_img%d_%s" % (mode, b, k)] for k in R.DEPTH_KEYS], axis=1)
        if mode == "direct":
            bx[b, valid[b]] = golden()["boxes_img%d" % b]
    return d, de, (bx if mode == "direct" else None)


def check_against(de, iou, bx, ref, mode, what):
    """The three tables against a restatement result at the bounds; every element written, empty slots exactly zero."""
    empty = ~ref["valid"]
    for name, t in (("depth_err", de), ("iou", iou), ("boxes", bx)):
        if t is not None:
            assert np.isfinite(t).all() and (np.abs(t) < 1e8).all(), (what, name, "an element was not written")
            assert (t[empty] == 0).all(), (what, name, "an empty slot is not zero")
    if de is not None:
        e = R.depth_errors_err(de, ref, mode)
        assert (e <= R.depth_bounds()).all(), (what, R.format_depth(e))
    if bx is not None:
        e = R.boxes_err(bx, ref, mode)
        assert (e <= R.box_bounds()).all(), (what, R.format_box(e))
        want_iou = R.iou_of_boxes(bx)                                  # float64 IoU of the boxes this arithmetic produced
        assert (np.abs(iou - want_iou) <= R.IOU_TOL * np.maximum(1.0, np.abs(want_iou))).all(), (what, np.abs(iou - want_iou).max())
