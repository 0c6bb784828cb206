"""float64, loop-form restatement of the duplicate suppression (TEST.USE_NMS '2d' / '3d'; helper module of the box_nms tests, not a test
file), and the case table the CPU and GPU tests share.

The reference declares TEST.USE_NMS / NMS_THRESH / NMS_CLASS_AGNOSTIC and reads them nowhere, so there is no recorded golden: the
semantics are the ones INTEGRATION.md states, written here as plainly as they read --
  * rows: cls, alpha, x1, y1, x2, y2, h, w, l, x, y (bottom centre), z, ry, score (generate_kitti_3d_detection's columns);
  * valid rows ranked by score descending, ties to the lower slot;
  * a row is kept unless an already kept row overlaps it with IoU > thresh (strict); a suppressed row suppresses nothing;
  * unless class-agnostic only rows of equal class id meet;
  * '2d': _box_iou of columns 2:6 (no +1, 0 / 0 = NaN, which is not > thresh); '3d': the rotated IoU of (x, y - h / 2, z, l, h, w, ry),
    by the float64 restatement tests/box3d_iou_ref.py that ops.box3d_iou is held to;
  * invalid rows take no part; the output is valid & kept.
Nothing here calls monoflex_amd.ops."""
import functools
import math

import numpy as np

import box3d_iou_ref as R3

THRESHOLDS = (0.1, 0.5, 0.9)
KINDS = ("2d", "3d")
MARGIN_3D = 1e-4            # the absolute bound tests/test_gpu_box3d_iou.py holds mfx_box3d_iou_pairs to (TOL * max(1, |ref|), IoU <= 1)


# ---- the restatement ------------------------------------------------------------------------------------------------------------------
def iou_2d(a, b):
    """_box_iou (model/head/detector_infer.py) of two (x1, y1, x2, y2) in python floats; 0 / 0 -> NaN."""
    a, b = [float(v) for v in a], [float(v) for v in b]
    inter = max(min(a[2], b[2]) - max(a[0], b[0]), 0.0) * max(min(a[3], b[3]) - max(a[1], b[1]), 0.0)
    den = (a[2] - a[0]) * (a[3] - a[1]) + (b[2] - b[0]) * (b[3] - b[1]) - inter
    if den == 0.0:
        return math.nan if inter == 0.0 else math.copysign(math.inf, inter)
    return inter / den


def box7(row):
    """det row -> (x, y, z, l, h, w, ry) with y the box centre."""
    r = [float(v) for v in row]
    return (r[9], r[10] - r[6] / 2.0, r[11], r[8], r[6], r[7], r[12])


def pair_iou(kind, ra, rb):
    return iou_2d(ra[2:6], rb[2:6]) if kind == "2d" else R3.iou_boxes(box7(ra), box7(rb))


def iou_matrix(det, valid, kind):
    """(K, 14), (K,) -> (K, K) float64, symmetric; NaN on the diagonal and wherever a row is invalid (such pairs are never asked for)."""
    K = det.shape[0]
    m = np.full((K, K), np.nan, dtype=np.float64)
    rows = [i for i in range(K) if valid[i]]
    for n, i in enumerate(rows):
        for j in rows[n + 1:]:
            m[i, j] = m[j, i] = pair_iou(kind, det[i], det[j])
    return m


def nms_image(det, valid, iou, thresh, class_agnostic, tie_to_higher_slot=False):
    """One image -> kept & valid as a bool array.  `tie_to_higher_slot` is NOT the semantics: the tests use it to find out whether a tie
    was decided by slot order."""
    K = det.shape[0]
    rows = [i for i in range(K) if valid[i]]
    rows.sort(key=lambda i: (-float(det[i, 13]), -i if tie_to_higher_slot else i))
    kept = []
    for c in rows:
        suppressed = False
        for k in kept:
            if not class_agnostic and float(det[k, 0]) != float(det[c, 0]):
                continue
            if iou[k, c] > thresh:
                suppressed = True
                break
        if not suppressed:
            kept.append(c)
    out = np.zeros(K, dtype=bool)
    out[kept] = True
    return out


def nms(det, valid, kind, thresh, class_agnostic, iou=None, tie_to_higher_slot=False):
    """(B, K, 14), (B, K) -> (B, K) int32.  iou: the list of per-image matrices when the caller holds them (iou_matrices)."""
    det, valid = np.asarray(det, dtype=np.float64), np.asarray(valid)
    out = np.zeros(valid.shape, dtype=np.int32)
    for b in range(det.shape[0]):
        m = iou[b] if iou is not None else iou_matrix(det[b], valid[b], kind)
        out[b] = nms_image(det[b], valid[b], m, thresh, class_agnostic, tie_to_higher_slot)
    return out


def iou_matrices(det, valid, kind):
    det = np.asarray(det, dtype=np.float64)
    return [iou_matrix(det[b], valid[b], kind) for b in range(det.shape[0])]


def gap_to_thresholds(mats, thresholds=THRESHOLDS):
    """Smallest |IoU - t| over every pair of valid rows and every threshold (NaN pairs, which no rounding turns into a number, aside)."""
    v = np.concatenate([m[np.isfinite(m)] for m in mats]) if mats else np.zeros(0)
    return min((float(np.abs(v - t).min()) for t in thresholds), default=math.inf) if v.size else math.inf


def box_iou_f32_error(det, valid):
    """Largest |float32 - float64| of _box_iou over every pair of valid rows of every image: the 2D margin is 4 times this."""
    from monoflex_amd.model.head.detector_infer import _box_iou
    worst = 0.0
    for b in range(det.shape[0]):
        rows = [i for i in range(det.shape[1]) if valid[b, i]]
        for n, i in enumerate(rows):
            for j in rows[n + 1:]:
                f32 = float(_box_iou(det[b, i, 2:6].astype(np.float32), det[b, j, 2:6].astype(np.float32)))
                f64 = iou_2d(det[b, i, 2:6], det[b, j, 2:6])
                if math.isfinite(f32) and math.isfinite(f64):
                    worst = max(worst, abs(f32 - f64))
    return worst


# ---- the case table ---------------------------------------------------------------------------------------------------------------------
def _row(cls, box2d, hwl, xyz, ry, score):
    r = np.zeros(14, dtype=np.float64)
    r[0], r[1] = cls, 0.0
    r[2:6], r[6:9], r[9:12], r[12], r[13] = box2d, hwl, xyz, ry, score
    return r


def _wrap(a):
    return (a + math.pi) % (2 * math.pi) - math.pi


def _cluster_image(rng, K):
    """Base boxes with 2-5 jittered near-copies each (shift, size and ry, the ry jitter across +-pi), some copies of another class, some
    scores equal; the rest of the K slots are isolated boxes.  Slots shuffled, a fifth of the rows invalid."""
    rows = []
    n_base = int(rng.integers(8, 11)) if K >= 50 else max(1, K // 5)
    for _ in range(n_base):
        if len(rows) >= K:
            break
        cls = int(rng.integers(0, 3))
        hwl = np.array([rng.uniform(1.4, 1.8), rng.uniform(1.5, 1.9), rng.uniform(3.2, 4.6)])
        xyz = np.array([rng.uniform(-25, 25), rng.uniform(1.0, 2.2), rng.uniform(8, 60)])
        ry = rng.uniform(-math.pi, math.pi) if rng.random() < 0.7 else math.copysign(math.pi - rng.uniform(0, 0.05), rng.normal())
        x1, y1 = rng.uniform(0, 1000), rng.uniform(100, 250)
        box = np.array([x1, y1, x1 + rng.uniform(30, 200), y1 + rng.uniform(25, 120)])
        score = rng.uniform(0.2, 0.95)
        rows.append(_row(cls, box, hwl, xyz, ry, score))
        for _ in range(int(rng.integers(2, 6))):
            if len(rows) >= K:
                break
            size = box[2:] - box[:2]
            amount = float(rng.choice([0.1, 0.5, 1.0]))                # from a near-exact copy (IoU above 0.9) to a loose one
            jbox = box + amount * np.concatenate((rng.normal(0, 0.06, 2) * size, rng.normal(0, 0.06, 2) * size))
            jry = _wrap(ry + amount * rng.uniform(-0.15, 0.15) + rng.choice([0.0, math.pi, -math.pi]))
            jcls = cls if rng.random() < 0.8 else (cls + 1) % 3
            jscore = score if rng.random() < 0.25 else rng.uniform(0.2, 0.95)
            rows.append(_row(jcls, jbox, hwl * (1 + amount * rng.uniform(-0.1, 0.1, 3)), xyz + amount * rng.normal(0, 0.15, 3) * [1, 0.3, 1], jry, jscore))
    while len(rows) < K:
        x1, y1 = rng.uniform(0, 1000), rng.uniform(100, 250)
        rows.append(_row(int(rng.integers(0, 3)), [x1, y1, x1 + rng.uniform(30, 200), y1 + rng.uniform(25, 120)],
                         [rng.uniform(1.4, 1.8), rng.uniform(0.6, 1.9), rng.uniform(0.8, 4.6)],
                         [rng.uniform(-25, 25), rng.uniform(1.0, 2.2), rng.uniform(8, 60)], rng.uniform(-math.pi, math.pi), rng.uniform(0.2, 0.95)))
    det = np.stack(rows)[rng.permutation(K)]
    valid = (rng.random(K) >= 0.2).astype(np.int32)
    return det, valid


def clusters(seed, B, K):
    rng = np.random.default_rng(seed)
    imgs = [_cluster_image(rng, K) for _ in range(B)]
    return np.stack([d for d, _ in imgs]).astype(np.float32), np.stack([v for _, v in imgs])


def chain(thresh):
    """A > B > C by score, equal boxes shifted along x by r and 2 r of their length: IoU(A, B) = IoU(B, C) = (1 - r) / (1 + r) > thresh,
    IoU(A, C) = (1 - 2 r) / (1 + 2 r) (0 from r = 1 / 2) < thresh, in 2D and in 3D (ry = 0: the length lies along x).  C must be kept.
    Slots C, A, B; a second image holds the same chain in class-mixed form (B of another class: nothing meets unless agnostic)."""
    r = 0.75 * (1 - thresh) / (1 + thresh)
    out = []
    for other in (0, 1):
        rows = []
        for n, score in ((2, 0.5), (0, 0.9), (1, 0.7)):
            cls = 1 if (other and n == 1) else 0
            rows.append(_row(cls, [100 + 80 * r * n, 50, 180 + 80 * r * n, 110], [1.5, 1.6, 4.0], [2.0 + 4.0 * r * n, 1.7, 20.0], 0.0, score))
        out.append(np.stack(rows))
    return np.stack(out).astype(np.float32), np.ones((2, 3), dtype=np.int32)


def identical(K, equal_scores):
    """K identical valid boxes: with distinct scores the top-scoring one survives (slot 17 here), with equal scores slot 0."""
    base = _row(0, [300, 120, 420, 200], [1.5, 1.6, 3.9], [3.0, 1.6, 25.0], 0.4, 0.5)
    det = np.tile(base, (1, K, 1))
    if not equal_scores:
        perm = np.random.default_rng(5).permutation(K)
        top = int(np.argmax(perm))
        perm[top], perm[17 % K] = perm[17 % K], perm[top]
        det[0, :, 13] = 0.3 + 0.5 * perm / K                      # distinct, the largest at slot 17 % K
    return det.astype(np.float32), np.ones((1, K), dtype=np.int32)


def class_pair():
    """Two coincident boxes of different classes: both kept unless class-agnostic."""
    a = _row(0, [300, 120, 420, 200], [1.5, 1.6, 3.9], [3.0, 1.6, 25.0], -2.0, 0.8)
    b = a.copy()
    b[0], b[13] = 2, 0.6
    return np.stack([a, b])[None].astype(np.float32), np.ones((1, 2), dtype=np.int32)


def degenerate_2d():
    """A zero-area 2D box (x1 = x2) and a copy of itself: 0 / 0 = NaN under '2d', so neither is suppressed.  (The 3D boxes coincide.)"""
    a = _row(1, [250, 120, 250, 200], [1.7, 0.7, 0.9], [-4.0, 1.8, 14.0], 1.0, 0.8)
    b = a.copy()
    b[13] = 0.6
    return np.stack([a, b])[None].astype(np.float32), np.ones((1, 2), dtype=np.int32)


def with_empty_image(seed):
    det, valid = clusters(seed, 3, 50)
    valid[1] = 0
    return det, valid


SEEDS = tuple(range(100, 140))                                      # tried in order until no pair IoU lies within the margins of a threshold


@functools.lru_cache(maxsize=None)
def case(name, thresh=None):
    """-> dict(det float32 (B, K, 14), valid int32 (B, K), iou {kind: per-image float64 matrices}, margin {kind: value}, gap {kind: value},
    seed).  Seeded cases re-draw their jitter (next seed of SEEDS) until every pair IoU is at least the kind's margin away from every
    threshold; the fixed cases are asserted to be."""
    makers = {"clusters": lambda s: clusters(s, 4, 50), "empty_image": with_empty_image, "k1": lambda s: clusters(s, 2, 1),
              "k64": lambda s: clusters(s, 2, 64), "k65": lambda s: clusters(s, 2, 65), "k128": lambda s: clusters(s, 2, 128)}
    fixed = {"chain": lambda: chain(thresh), "identical": lambda: identical(50, False), "identical_equal": lambda: identical(50, True),
             "class_pair": class_pair, "degenerate_2d": degenerate_2d}
    for seed in (SEEDS if name in makers else (None,)):
        det, valid = makers[name](seed) if name in makers else fixed[name]()
        iou = {k: iou_matrices(det, valid, k) for k in KINDS}
        margin = {"2d": 4 * box_iou_f32_error(det, valid), "3d": MARGIN_3D}
        gap = {k: gap_to_thresholds(iou[k]) for k in KINDS}
        if all(gap[k] >= margin[k] for k in KINDS):
            return dict(det=det, valid=valid, iou=iou, margin=margin, gap=gap, seed=seed)
        assert name in makers, "fixed case %s has a pair IoU within the margin of a threshold: %r < %r" % (name, gap, margin)
    raise AssertionError("no seed of SEEDS keeps case %s clear of the thresholds" % name)


CASES = ("clusters", "chain", "identical", "identical_equal", "class_pair", "degenerate_2d", "empty_image", "k1", "k64", "k65", "k128")
CLUSTERED = ("clusters", "k64", "k65", "k128")                      # every image of these must see a suppression and a survivor


def table():
    """Every (case name, kind, class_agnostic, thresh) of the table."""
    return [(n, k, a, t) for n in CASES for k in KINDS for a in (False, True) for t in THRESHOLDS]


def expected(name, kind, agnostic, thresh, tie_to_higher_slot=False):
    c = case(name, thresh if name == "chain" else None)
    return c, nms(c["det"], c["valid"], kind, thresh, agnostic, iou=c["iou"][kind], tie_to_higher_slot=tie_to_higher_slot)
