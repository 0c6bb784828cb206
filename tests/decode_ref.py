"""float64 restatement of mfx_decode_boxes_mode (monoflex_amd/csrc/decode.hip `decode_boxes_kernel`), plain numpy.

Inputs are the kernel's own: the NHWC head map with its row length `ld` and the offset `reg_off` of the 50 regression channels, the per-class
top-K lists `scores` / `index` (B, ncls, K), `calib` (B, 6) = [f_u, f_v, c_u, c_v, b_x, b_y], `pad` (B, 2), `img_size` (2,) of image 0,
`threshold` and the `output_depth` mode.  Every float32 input is taken as the exact real number it holds; all arithmetic is float64.
Written from the reference's formulas (model/layers/utils.py:61-100, model/anno_encoder.py:69-295, model/head/detector_infer.py:77-237) and
independent of oracle/monoflex_ref.py (float32, one image at a time), whose constants it reads.

Besides `det` (B, K, 14), `topk` (B, K, 5) and `valid` (B, K) it returns, per row, the margin of every discontinuous decision of the decode
(a row below such a margin may legitimately land on either side in float32) and the intermediate values the census of tests/decode_cases.py
reads.

`wrong=` names deliberately wrong variants of the decode.  They exist for the sensitivity tests of tests/test_decode_ref_cpu.py only: a test
input on which a wrong variant gives the same rows as the correct decode cannot tell the two apart.
"""
import math

import numpy as np

from oracle.monoflex_ref import DEPTH_RANGE, DIM_MEAN, DOWN_RATIO, EPS_KPT

MODES = ("soft", "hard", "mean", "direct", "keypoints_avg", "keypoints_center", "keypoints_02", "keypoints_13")
# key2channel offsets of runs/monoflex.yaml: 2d_dim 4, 3d_offset 2, corner_offset 20, corner_uncertainty 3, 3d_dim 3, ori_cls 8, ori_offset 8,
# depth 1, depth_uncertainty 1
R_2D, R_OFF3D, R_KPT, R_KPT_UNC, R_DIM3D, R_ORI_CLS, R_ORI_OFF, R_DEPTH, R_DEPTH_UNC, R_TOTAL = 0, 4, 6, 26, 29, 32, 40, 48, 49, 50
COLUMNS = ("cls", "alpha", "x1", "y1", "x2", "y2", "h", "w", "l", "X", "Y", "Z", "ry", "score")
WRONG = ("d3_from_d2_pairs", "d2_one_pair", "calib_of_image0", "pad_of_image0", "clamp_per_image", "no_half_height", "dims_not_rolled")

NEAR_MARGIN = 1e-5            # relative margin of an arg-max, absolute distance (rad) of an un-wrapped angle from +-pi, below which float32 may differ
NEAR_CAP = 0.02               # such rows may be at most this share of the rows of any case

# Per-column yardstick: the worst error, as |a - b| / max(1, |b|), of the float32 reference arithmetic against this restatement on the same
# inputs -- the reference's own PostProcessor rows (tests/golden/decode_structured.npz, decode_only.npz) and oracle.decode_image, the
# latter also on every pixel of the very maps the device cases read -- measured by tests/test_decode_ref_cpu.py (which prints the figures
# and asserts they stay below 4x these).  The device kernel gets the same 4x.
# (The box columns' 9.54e-07 = 2^-20 is the float32 formula itself: (px - e) in [4, 8) carries half an ulp, 2.4e-7, times the down ratio 4,
# and the pad then cancels the result down to below 1.)
YARDSTICK = dict(zip(COLUMNS, (0.0, 4.45e-07, 9.54e-07, 4.77e-07, 9.54e-07, 4.77e-07, 1.26e-07, 1.49e-07, 1.22e-07, 2.91e-06, 1.26e-06, 2.97e-07, 6.90e-07, 1.40e-07)))
BOUND_FACTOR = 4.0


def stage2_merge(scores):
    """select_topk stage 2 (utils.py:88-91): the K best of the concatenated (ncls * K) list of one image under the kernel's total order,
    value descending, position ascending.  -> positions (K,)"""
    flat = np.asarray(scores, dtype=np.float64).reshape(-1)
    K = np.asarray(scores).shape[-1]
    order = np.lexsort((np.arange(flat.size), -flat))          # last key is the primary one
    return order[:K]


def _rel_margin(values):
    """(best - second) / |best| along the last axis."""
    s = np.sort(values, axis=-1)
    return (s[..., -1] - s[..., -2]) / np.maximum(np.abs(s[..., -1]), 1e-300)


def decode_boxes(hmap, reg_off, scores, index, calib, pad, img_size, threshold, mode="soft", wrong=(), img_sizes=None):
    """-> dict(det (B,K,14), topk (B,K,5), valid (B,K) int32, margins..., census intermediates...), all float64.
    `img_sizes` (B, 2) is read by the wrong variant 'clamp_per_image' only."""
    assert mode in MODES, mode
    wrong = (wrong,) if isinstance(wrong, str) else tuple(wrong)
    assert all(w in WRONG for w in wrong), wrong
    hmap = np.asarray(hmap)
    B, H, W, ld = hmap.shape
    scores, index = np.asarray(scores), np.asarray(index)
    ncls, K = scores.shape[1], scores.shape[2]
    assert scores.shape == index.shape == (B, ncls, K) and ncls == 3
    assert np.isfinite(scores).all() and (index >= 0).all() and (index < H * W).all()
    calib = np.asarray(calib, dtype=np.float64).reshape(B, 6)
    pad = np.asarray(pad, dtype=np.float64).reshape(B, 2)
    img_size = np.asarray(img_size, dtype=np.float64).reshape(2)
    thr = float(np.float32(threshold))                           # the kernel compares float32 with float32
    dmin, dmax = float(DEPTH_RANGE[0]), float(DEPTH_RANGE[1])
    mean = np.asarray(DIM_MEAN, dtype=np.float64)
    pi = math.pi

    out = {k: np.zeros((B, K)) for k in ("bin_margin", "hard_margin", "alpha_wrap_dist", "ry_wrap_dist", "alpha_raw", "ry_raw", "sigma",
                                         "d_direct_raw", "d1_raw", "d2_raw", "d3_raw")}
    out["best_bin"] = np.zeros((B, K), dtype=np.int64)
    out["hard_choice"] = np.zeros((B, K), dtype=np.int64)
    out["kpt_terms"] = np.zeros((B, K, 5))                       # f_u h / (relu(dy) 4 + eps): centre, pair 0-4, 2-6, 1-5, 3-7
    out["kpt_dy"] = np.zeros((B, K, 5))
    out["box_raw"] = np.zeros((B, K, 4))                         # the 2D box before its clamp
    out["box_max"] = np.zeros((B, 2))
    det, topk, valid = np.zeros((B, K, 14)), np.zeros((B, K, 5)), np.zeros((B, K), dtype=np.int32)
    for b in range(B):
        pos = stage2_merge(scores[b])
        cls = pos // K                                           # utils.py:91
        sc = scores[b].reshape(-1).astype(np.float64)[pos]
        idx = index[b].reshape(-1).astype(np.int64)[pos]
        ys, xs = idx // W, idx % W
        r = hmap[b].reshape(H * W, ld)[idx, reg_off:reg_off + R_TOTAL].astype(np.float64)
        fu, fv, cu, cv, bx, by = calib[0 if "calib_of_image0" in wrong else b]
        padx, pady = pad[0 if "pad_of_image0" in wrong else b]
        px, py = xs.astype(np.float64), ys.astype(np.float64)

        # decode_box2d_fcos (anno_encoder.py:69-86); the clamp uses image 0's size
        size = np.asarray(img_sizes, dtype=np.float64)[b] if "clamp_per_image" in wrong else img_size
        wmax, hmax = size[0] - 1, size[1] - 1
        raw = np.stack(((px - np.maximum(r[:, R_2D + 0], 0)) * DOWN_RATIO - padx, (py - np.maximum(r[:, R_2D + 1], 0)) * DOWN_RATIO - pady,
                        (px + np.maximum(r[:, R_2D + 2], 0)) * DOWN_RATIO - padx, (py + np.maximum(r[:, R_2D + 3], 0)) * DOWN_RATIO - pady), axis=1)
        box = raw.copy()
        box[:, 0::2] = np.clip(box[:, 0::2], 0, wmax)
        box[:, 1::2] = np.clip(box[:, 1::2], 0, hmax)

        # decode_dimension (anno_encoder.py:221-243): exp(offset) * mean[cls], (l, h, w)
        dims = np.exp(r[:, R_DIM3D:R_DIM3D + 3]) * mean[cls]
        dl, dh, dw = dims[:, 0], dims[:, 1], dims[:, 2]

        # decode_depth, inv_sigmoid (anno_encoder.py:124-140): 1 / sigmoid(x) - 1 = exp(-x)
        d0_raw = np.exp(-r[:, R_DEPTH])
        d0 = np.clip(d0_raw, dmin, dmax)
        u0 = np.exp(r[:, R_DEPTH_UNC])

        # decode_depth_from_keypoints_batch (anno_encoder.py:187-219); keypoint k = (r[6 + 2k], r[7 + 2k])
        ky = lambda k: r[:, R_KPT + 2 * k + 1]
        kdepth = lambda dy: fu * dh / (np.maximum(dy, 0) * DOWN_RATIO + EPS_KPT)
        dy = np.stack((ky(8) - ky(9), ky(0) - ky(4), ky(2) - ky(6), ky(1) - ky(5), ky(3) - ky(7)), axis=1)
        t = np.stack([kdepth(dy[:, i]) for i in range(5)], axis=1)
        d1_raw = t[:, 0]
        d2_raw = t[:, 1] if "d2_one_pair" in wrong else (t[:, 1] + t[:, 2]) / 2
        d3_raw = (t[:, 1] + t[:, 2]) / 2 if "d3_from_d2_pairs" in wrong else (t[:, 3] + t[:, 4]) / 2
        d1, d2, d3 = (np.clip(v, dmin, dmax) for v in (d1_raw, d2_raw, d3_raw))
        u1, u2, u3 = (np.exp(r[:, R_KPT_UNC + i]) for i in range(3))

        # which depth leaves the four estimates (detector_infer.py:149-198)
        d_all, u_all = np.stack((d0, d1, d2, d3), axis=1), np.stack((u0, u1, u2, u3), axis=1)
        w_all = 1.0 / u_all
        hard = np.argmax(w_all, axis=1)                          # first of equals
        if mode == "soft":
            wn = w_all / w_all.sum(axis=1, keepdims=True)
            depth, sigma = (d_all * wn).sum(axis=1), (wn * u_all).sum(axis=1)
        elif mode == "hard":
            depth, sigma = d_all[np.arange(K), hard], u_all.min(axis=1)
        elif mode == "mean":
            depth, sigma = d_all.mean(axis=1), u_all.mean(axis=1)
        elif mode == "keypoints_avg":
            depth, sigma = d_all[:, 1:].mean(axis=1), u_all[:, 1:].mean(axis=1)
        else:
            c = {"direct": 0, "keypoints_center": 1, "keypoints_02": 2, "keypoints_13": 3}[mode]
            depth, sigma = d_all[:, c], u_all[:, c]

        # decode_location_flatten (anno_encoder.py:142-155) + project_image_to_rect (kitti_utils.py:350-369)
        u = (px + r[:, R_OFF3D + 0]) * DOWN_RATIO - padx
        v = (py + r[:, R_OFF3D + 1]) * DOWN_RATIO - pady
        X = (u - cu) * depth / fu + bx
        Y = (v - cv) * depth / fv + by
        Z = depth

        # decode_axes_orientation, multi-bin (anno_encoder.py:245-295): softmax over each bin's pair, arg-max of the second entry
        a, c = r[:, R_ORI_CLS:R_ORI_CLS + 8:2], r[:, R_ORI_CLS + 1:R_ORI_CLS + 8:2]
        m = np.maximum(a, c)
        p1 = np.exp(c - m) / (np.exp(a - m) + np.exp(c - m))
        best = np.argmax(p1, axis=1)
        centers = np.array([0.0, pi / 2, pi, -pi / 2])
        off = r[:, R_ORI_OFF:R_ORI_OFF + 8].reshape(K, 4, 2)[np.arange(K), best]
        alpha_raw = np.arctan2(off[:, 0], off[:, 1]) + centers[best]
        ry_raw = alpha_raw + np.arctan2(X, Z)
        wrap = lambda x: np.where(x > pi, x - 2 * pi, np.where(x < -pi, x + 2 * pi, x))
        alpha, ry = wrap(alpha_raw), wrap(ry_raw)

        if "no_half_height" not in wrong:
            Y = Y + dh / 2                                       # detector_infer.py:215
        final = sc * (1 - np.clip(sigma, 0.01, 1))               # :225-227
        hwl = (dl, dh, dw) if "dims_not_rolled" in wrong else (dh, dw, dl)       # roll(-1): (l, h, w) -> (h, w, l)
        det[b] = np.stack((cls.astype(np.float64), alpha, box[:, 0], box[:, 1], box[:, 2], box[:, 3], hwl[0], hwl[1], hwl[2], X, Y, Z, ry, final), axis=1)
        topk[b] = np.stack((sc, idx.astype(np.float64), cls.astype(np.float64), py, px), axis=1)
        valid[b] = (sc >= thr).astype(np.int32)

        out["bin_margin"][b], out["best_bin"][b] = _rel_margin(p1), best
        out["hard_margin"][b], out["hard_choice"][b] = _rel_margin(w_all), hard
        out["alpha_wrap_dist"][b] = np.minimum(np.abs(alpha_raw - pi), np.abs(alpha_raw + pi))
        out["ry_wrap_dist"][b] = np.minimum(np.abs(ry_raw - pi), np.abs(ry_raw + pi))
        out["alpha_raw"][b], out["ry_raw"][b], out["sigma"][b] = alpha_raw, ry_raw, sigma
        out["d_direct_raw"][b], out["d1_raw"][b], out["d2_raw"][b], out["d3_raw"][b] = d0_raw, d1_raw, d2_raw, d3_raw
        out["kpt_terms"][b], out["kpt_dy"][b], out["box_raw"][b], out["box_max"][b] = t, dy, raw, (wmax, hmax)
    out.update(det=det, topk=topk, valid=valid)
    return out


def near_rows(ref, mode):
    """Rows whose orientation-bin arg-max (or, in 'hard' mode, the arg-max over the four weights) is decided by less than NEAR_MARGIN:
    alpha, ry and the depth of such a row are not compared (column_errors)."""
    near = ref["bin_margin"] < NEAR_MARGIN
    if mode == "hard":
        near = near | (ref["hard_margin"] < NEAR_MARGIN)
    return near


def column_errors(got, ref, mode, rows=None):
    """Worst |got - want| / max(1, |want|) per column -> (14,) over the rows selected by the boolean mask `rows` (default: all).
    Near-decision rows: a bin arg-max below the margin takes alpha and ry out; a `hard` arg-max below it takes the depth out, that is Z and
    the columns the depth enters (X, Y, ry) -- the score does not depend on the choice (sigma = min u).  alpha / ry within NEAR_MARGIN of
    +-pi before the wrap are compared modulo 2 pi.  Everything else is compared."""
    want = ref["det"]
    got = np.asarray(got, dtype=np.float64)
    assert got.shape == want.shape, (got.shape, want.shape)
    err = np.abs(got - want) / np.maximum(1.0, np.abs(want))
    for col, dist in ((1, ref["alpha_wrap_dist"]), (12, ref["ry_wrap_dist"])):
        d = np.abs(got[..., col] - want[..., col])
        mod = np.minimum(d, np.abs(d - 2 * math.pi)) / np.maximum(1.0, np.abs(want[..., col]))
        err[..., col] = np.where(dist < NEAR_MARGIN, mod, err[..., col])
    use = np.ones(want.shape, dtype=bool) if rows is None else np.broadcast_to(np.asarray(rows, dtype=bool)[..., None], want.shape).copy()
    near_bin = ref["bin_margin"] < NEAR_MARGIN
    use[..., 1] &= ~near_bin
    use[..., 12] &= ~near_bin
    if mode == "hard":
        near_hard = ref["hard_margin"] < NEAR_MARGIN
        for col in (9, 10, 11, 12):
            use[..., col] &= ~near_hard
    err = np.where(use, err, 0.0)
    return err.reshape(-1, 14).max(axis=0) if err.size else np.zeros(14)


def bounds():
    return np.array([BOUND_FACTOR * YARDSTICK[c] for c in COLUMNS])


def format_errors(err):
    return "  ".join("%s %.2e" % (c, e) for c, e in zip(COLUMNS, err))
