"""float64 reference of the rotated 3D box IoU (helper module of the box3d_iou tests, not a test file).

Written from the definition the reference's get_iou_3d (model/layers/iou_loss.py:99-136) states in terms of shapely:
`Polygon(a).intersection(Polygon(b)).area` of the two bottom rectangles, times the overlap of the two height intervals, over
`area_a * h_a + area_b * h_b - overlap`.  The intersection of two convex polygons is the set of points of one that lie in every edge
half-plane of the other, so it is computed by Sutherland-Hodgman clipping (subject polygon cut by one half-plane after another) and its
area by the shoelace formula.  Everything is python floats (float64); the inputs are taken as exact.  tests/test_box3d_iou_cpu.py pins
this module itself to closed forms before anything is compared against it."""
import math

import numpy as np

SX = (-1.0, -1.0, 1.0, 1.0, -1.0, -1.0, 1.0, 1.0)                   # encode_box3d's corner order (anno_encoder.py:88-122)
SY = (1.0, 1.0, 1.0, 1.0, -1.0, -1.0, -1.0, -1.0)
SZ = (-1.0, 1.0, 1.0, -1.0, -1.0, 1.0, 1.0, -1.0)


def polygon_area(p):
    """Unsigned shoelace area of a ring of (x, y) points."""
    s = 0.0
    for i in range(len(p)):
        (x0, y0), (x1, y1) = p[i], p[(i + 1) % len(p)]
        s += x0 * y1 - x1 * y0
    return abs(s) / 2.0


def _signed_area(p):
    return sum(p[i][0] * p[(i + 1) % len(p)][1] - p[(i + 1) % len(p)][0] * p[i][1] for i in range(len(p))) / 2.0


def clip_convex(subject, clip):
    """Sutherland-Hodgman: the part of convex polygon `subject` inside convex polygon `clip` (lists of (x, y)), as a ring."""
    clip = list(clip)
    if _signed_area(clip) < 0:
        clip.reverse()                                               # counter-clockwise: inside is to the left of every edge
    ring = list(subject)
    for i in range(len(clip)):
        if not ring:
            break
        (ax, ay), (bx, by) = clip[i], clip[(i + 1) % len(clip)]

        def left(p):
            return (bx - ax) * (p[1] - ay) - (by - ay) * (p[0] - ax)
        nxt = []
        for j in range(len(ring)):
            cur, prev = ring[j], ring[j - 1]
            dc, dp = left(cur), left(prev)
            if dc >= 0:
                if dp < 0:
                    t = dp / (dp - dc)
                    nxt.append((prev[0] + t * (cur[0] - prev[0]), prev[1] + t * (cur[1] - prev[1])))
                nxt.append(cur)
            elif dp >= 0:
                t = dp / (dp - dc)
                nxt.append((prev[0] + t * (cur[0] - prev[0]), prev[1] + t * (cur[1] - prev[1])))
        ring = nxt
    return ring


def intersection_area(a, b):
    ring = clip_convex([tuple(map(float, p)) for p in a], [tuple(map(float, p)) for p in b])
    return polygon_area(ring) if len(ring) >= 3 else 0.0


def corners_of(box):
    """(x, y, z, l, h, w, ry), y = centre -> (8, 3) float64 corners in encode_box3d order."""
    x, y, z, l, h, w, ry = (float(v) for v in box)
    c, s = math.cos(ry), math.sin(ry)
    out = np.zeros((8, 3), dtype=np.float64)
    for k in range(8):
        px, py, pz = 0.5 * l * SX[k], 0.5 * h * SY[k], 0.5 * w * SZ[k]
        out[k] = (c * px + s * pz + x, py + y, -s * px + c * pz + z)
    return out


def iou_corners(A, B):
    """One pair of (8, 3) corner tables -> IoU (python float); 0 when the union is not positive and finite."""
    A, B = np.asarray(A, dtype=np.float64), np.asarray(B, dtype=np.float64)
    lo_a, hi_a = -float(A[0:4, 1].sum()) / 4.0, -float(A[4:8, 1].sum()) / 4.0
    lo_b, hi_b = -float(B[0:4, 1].sum()) / 4.0, -float(B[4:8, 1].sum()) / 4.0
    h_ov = max(0.0, min(hi_a, hi_b) - max(lo_a, lo_b))
    qa, qb = [(A[k, 0], A[k, 2]) for k in range(4)], [(B[k, 0], B[k, 2]) for k in range(4)]
    ov = intersection_area(qa, qb) * h_ov
    union = polygon_area(qa) * (hi_a - lo_a) + polygon_area(qb) * (hi_b - lo_b) - ov
    if not (union > 0.0) or not math.isfinite(union) or not math.isfinite(ov):
        return 0.0
    return ov / union


def iou_boxes(a, b):
    return iou_corners(corners_of(a), corners_of(b))


def iou_pairs(A, B):
    """(N, 7) rows or (N, 8, 3) corner tables -> (N,) float64."""
    A, B = np.asarray(A), np.asarray(B)
    f = iou_boxes if A.ndim == 2 else iou_corners
    return np.array([f(A[i], B[i]) for i in range(A.shape[0])], dtype=np.float64)


# ---- inputs shared by the CPU and the GPU test files ------------------------------------------------------------------------------
def random_pairs(n, seed):
    """KITTI-like matched pairs as float32 (n, 7) rows: dimensions 0.5-5 m, the second centre within +-3 m of the first in x and z
    (+-1.5 m in y), 5-70 m deep, any yaw."""
    rng = np.random.default_rng(seed)
    a = np.zeros((n, 7), dtype=np.float64)
    a[:, 0], a[:, 1], a[:, 2] = rng.uniform(-30, 30, n), rng.uniform(-1, 3, n), rng.uniform(5, 70, n)
    a[:, 3:6] = rng.uniform(0.5, 5.0, (n, 3))
    a[:, 6] = rng.uniform(-math.pi, math.pi, n)
    b = a.copy()
    b[:, 0] += rng.uniform(-3, 3, n)
    b[:, 1] += rng.uniform(-1.5, 1.5, n)
    b[:, 2] += rng.uniform(-3, 3, n)
    b[:, 3:6] = rng.uniform(0.5, 5.0, (n, 3))
    b[:, 6] = rng.uniform(-math.pi, math.pi, n)
    return a.astype(np.float32), b.astype(np.float32)


def near_identical_pairs(n, seed, delta=1e-3):
    """Pairs that differ by `delta` in ONE of the seven parameters (pair i: parameter i % 7): coincident and nearly collinear edges."""
    a, _ = random_pairs(n, seed)
    b = a.copy()
    for i in range(n):
        b[i, i % 7] += np.float32(delta)
    return a, b


def corner_tables(rows):
    """float32 (n, 7) rows -> float32 (n, 8, 3) corner tables (built in float64, rounded once)."""
    return np.stack([corners_of(r) for r in rows]).astype(np.float32)


def overlapping_loss_case(ev, name="b1_many", seed=0):
    """A loss case whose predicted boxes DO overlap their targets (the seeded golden cases decode random maps: their IoU is 0): the inputs
    of golden case `name`, with every object's target offset, depth, dimensions and yaw replaced by the decoded prediction plus a seeded
    perturbation of up to 0.4 px / 0.6 m / 15 % / 0.3 rad.  Returns (cls, reg, heat, tv): `ev(preds, (heat, tv))` evaluates it.  ev: a
    Loss_Computation."""
    import torch
    from test_loss_golden import case_inputs
    from monoflex_amd.structures.params_3d import make_train_target
    tg, cls, reg = case_inputs(name)
    heat, tv = ev.prepare_targets([make_train_target(t) for t in tg])
    with torch.no_grad():
        _, P, _, _ = ev.prepare_predictions(tv, {"reg": reg})
    B, M = tv["reg_mask"].shape[:2]
    g = torch.Generator().manual_seed(seed)
    u = lambda *shape: torch.rand(*shape, generator=g) * 2 - 1
    scale = torch.rand(B * M, 1, generator=g)                        # per object: from a near-perfect to a loose prediction
    cat = P["cat_3D"].detach()
    tv["offset_3D"] = (P["offset_3D"].detach() + 0.4 * scale * u(B * M, 2)).reshape(B, M, 2).to(tv["offset_3D"].dtype)
    loc = tv["locations"].clone()
    loc[..., 2] = (cat[:, 2] + 0.6 * scale[:, 0] * u(B * M)).reshape(B, M).to(loc.dtype)
    tv["locations"] = loc
    tv["dimensions"] = (cat[:, 3:6] * (1 + 0.15 * scale * u(B * M, 3))).reshape(B, M, 3).to(tv["dimensions"].dtype)
    tv["rotys"] = (cat[:, 6] + 0.3 * scale[:, 0] * u(B * M)).reshape(B, M).to(tv["rotys"].dtype)
    tv["object_rows"] = ev.pack_objects(tv)
    return cls, reg, heat, tv


def mean_iou_of_case(ev, reg, tv):
    """float64 mean IoU over the valid rows of the boxes the tensor-op form decodes (its `cat_3D` rows: centre, dims, yaw)."""
    import torch
    with torch.no_grad():
        T, P, sel, _ = ev.prepare_predictions(tv, {"reg": reg})
    valid = sel["valid"].numpy()
    if not valid.any():
        return 0.0
    return float(iou_pairs(P["cat_3D"].double().numpy()[valid], T["cat_3D"].double().numpy()[valid]).mean())
