"""`get_iou_3d` of the reference's model/layers/iou_loss.py:99-136: the rotated 3D box IoU behind the logged `3D_IoU`.

The reference builds one shapely Polygon per object on the host.  Here CUDA tensors go to the device operator (ops.box3d_iou ->
mfx_box3d_iou_pairs: one launch on the current stream, no synchronisation, capturable); CPU tensors -- the tensor-op form of the loss
run on the host -- take a small float64 restatement of the same definition below.  `IOULoss` lives in the loss itself
(detector_loss.py `_iou`, csrc/object_loss_math.h) and `get_corners` has no caller: neither is provided."""
import numpy as np
import torch


def _clip_area(a, b):
    """Area of the intersection of two convex polygons (k, 2) / (m, 2), ring order, either orientation: `a` cut by the half-plane of
    every edge of `b` in turn, then the shoelace sum."""
    def area2(p):
        x, y = p[:, 0], p[:, 1]
        return float(np.dot(x, np.roll(y, -1)) - np.dot(np.roll(x, -1), y))
    if area2(b) < 0:
        b = b[::-1]
    poly = [tuple(p) for p in a]
    for i in range(len(b)):
        (ex, ey), (fx, fy) = b[i], b[(i + 1) % len(b)]
        side = [(fx - ex) * (y - ey) - (fy - ey) * (x - ex) for x, y in poly]
        out = []
        for j in range(len(poly)):
            (px, py), (qx, qy), dp, dq = poly[j - 1], poly[j], side[j - 1], side[j]
            if (dp >= 0) != (dq >= 0):
                t = dp / (dp - dq)
                out.append((px + t * (qx - px), py + t * (qy - py)))
            if dq >= 0:
                out.append((qx, qy))
        poly = out
        if not poly:
            return 0.0
    return 0.5 * abs(area2(np.asarray(poly))) if len(poly) >= 3 else 0.0


def _iou_3d_host(A, B):
    A, B = np.asarray(A, dtype=np.float64), np.asarray(B, dtype=np.float64)
    out = np.zeros(A.shape[0], dtype=np.float64)
    lo_a, hi_a = -A[:, 0:4, 1].mean(axis=1), -A[:, 4:8, 1].mean(axis=1)      # y points down: heights on the negated axis
    lo_b, hi_b = -B[:, 0:4, 1].mean(axis=1), -B[:, 4:8, 1].mean(axis=1)
    h_ov = np.maximum(0.0, np.minimum(hi_a, hi_b) - np.maximum(lo_a, lo_b))
    for i in range(A.shape[0]):
        qa, qb = A[i, 0:4][:, [0, 2]], B[i, 0:4][:, [0, 2]]
        ov = _clip_area(qa, qb) * h_ov[i] if h_ov[i] > 0 else 0.0
        union = _clip_area(qa, qa) * (hi_a[i] - lo_a[i]) + _clip_area(qb, qb) * (hi_b[i] - lo_b[i]) - ov
        if union > 0 and np.isfinite(union) and np.isfinite(ov):
            out[i] = ov / union
    return out


def get_iou_3d(pred_corners, target_corners):
    """(N, 8, 3) corner tables in rect coordinates (encode_box3d order) -> (N,) float IoU of box i of one with box i of the other:
    overlap of the bottom rectangles (corners 0..3, x-z) times the overlap in height, over the union of the two volumes.  A pair
    without a positive finite union gives 0."""
    if pred_corners.shape != target_corners.shape or pred_corners.dim() != 3 or tuple(pred_corners.shape[1:]) != (8, 3):
        raise ValueError("get_iou_3d: two (N, 8, 3) corner tables, got %s and %s" % (tuple(pred_corners.shape), tuple(target_corners.shape)))
    if pred_corners.is_cuda:
        from ... import ops
        return ops.box3d_iou(pred_corners, target_corners)
    iou = _iou_3d_host(pred_corners.detach().double().numpy(), target_corners.detach().double().numpy())
    return torch.from_numpy(iou).float()
