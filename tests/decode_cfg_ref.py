"""float64 restatement of mfx_decode_boxes_cfg (monoflex_amd/csrc/decode.hip `decode_boxes_kernel` with a `mfx_decode_cfg`), plain numpy.

The configurable form of tests/decode_ref.py (which stays the restatement of the runs/monoflex.yaml decode): the head settings a model is
trained with decide how its maps are decoded --
  DEPTH_MODE 'exp' / 'linear' (with DEPTH_REFERENCE) / 'inv_sigmoid', then the DEPTH_RANGE clamp          (model/anno_encoder.py:124-140)
  DIMENSION_REG[0] 'exp' / 'linear' and DIMENSION_REG[2]: off * std + mean, or off * mean                    (model/anno_encoder.py:221-243)
  DIMENSION_MEAN / DIMENSION_STD, one (l, h, w) row per class, 1 to 3 classes
  TEST.UNCERTAINTY_AS_CONFIDENCE: score * (1 - clamp(sigma, 0.01, 1)), or the raw score                     (model/head/detector_infer.py:223-229)
Inputs, conventions and outputs are decode_ref's (every float32 input is the exact real number it holds, all arithmetic float64; the
configuration values are taken as the Python floats the config holds); `unc` (B, K, 2) = [estimated_depth_error, uncertainty_conf] is new:
sigma and 1 - clamp(sigma, 0.01, 1), both zero when the confidence scaling is off (the reference reports None there).

`decode_rows_f32` evaluates the same formulas in float32 torch operations, in the reference's operation order, on the rows the restatement
selected: with the recorded rows of the reference's own PostProcessor (tests/golden/decode_cfg.npz) it is the float32 arithmetic whose
distance from this restatement is the yardstick below.

`wrong=` names deliberately wrong variants, for the sensitivity tests of tests/test_decode_cfg_ref_cpu.py only.
"""
import math

import numpy as np

from tests import decode_ref as D
from tests.decode_ref import (BOUND_FACTOR, COLUMNS, MODES, NEAR_CAP, NEAR_MARGIN, R_2D, R_DEPTH, R_DEPTH_UNC, R_DIM3D, R_KPT, R_KPT_UNC,  # noqa: F401
                              R_OFF3D, R_ORI_CLS, R_ORI_OFF, R_TOTAL, column_errors, format_errors, near_rows, stage2_merge)

DOWN_RATIO, EPS_KPT = 4, 1e-3
DEPTH_DECODE = ("exp", "linear", "inv_sigmoid")               # mfx_decode_cfg.depth_decode = mfx_object_loss_cfg.depth_mode's numbering
WRONG = ("std_ignored", "mean_of_class0", "depth_ref_swapped", "no_depth_clamp_direct", "conf_always_applied", "exp_dims_when_linear")

KITTI_MEAN = ((3.8840, 1.5261, 1.6286), (0.8423, 1.7607, 0.6602), (1.7635, 1.7372, 0.5968))
KITTI_STD = ((0.4259, 0.1367, 0.1022), (0.2349, 0.1133, 0.1427), (0.1766, 0.0948, 0.1242))
DEPTH_REFERENCE = (26.494627, 16.05988)
# (custom statistics, two to three times KITTI's spread; off * std + mean stays clear of zero for the offsets of tests/decode_cases.py, |off| <= 1.5:
# a linear dimension that crosses zero is ill-conditioned in float32 -- h = 1e-5 with an error of 1e-7 moves a keypoint depth by a percent -- and
# would widen the yardstick of the depth columns a thousandfold.  Negative linear dimensions are reached through off * mean, which does not cancel.)
CUSTOM_MEAN = ((4.1, 1.6, 1.7), (0.9, 1.7, 0.7), (1.8, 1.75, 0.6))
CUSTOM_STD = ((0.9, 0.3, 0.25), (0.3, 0.25, 0.2), (0.4, 0.2, 0.2))


def _setting(**kw):
    s = dict(depth_mode="inv_sigmoid", depth_ref=DEPTH_REFERENCE, depth_range=(0.1, 100.0), dim_exp=True, dim_use_std=False,
             uncertainty_as_conf=True, dim_mean=KITTI_MEAN, dim_std=KITTI_STD, ncls=3)
    s.update(kw)
    return s


YAML = _setting()                                               # runs/monoflex.yaml: what mfx_decode_boxes_mode has built in
# the settings the tests and the recorded reference rows (tools/gen_decode_cfg_golden.py) run
SETTINGS = {
    # monoflex_amd/config.py's own defaults: DEPTH_MODE exp, DIMENSION_REG ['linear', True, False] (its third entry is the std switch: off),
    # no confidence scaling -- and the same with the std switch on, the fourth form of decode_dimension
    "a_defaults": _setting(depth_mode="exp", dim_exp=False, dim_use_std=False, uncertainty_as_conf=False),
    "a_linear_std": _setting(depth_mode="exp", dim_exp=False, dim_use_std=True, uncertainty_as_conf=False),
    "b_linear_depth": _setting(depth_mode="linear"),
    "c_exp_dims_std": _setting(dim_use_std=True),
    "d_linear_dims": _setting(dim_exp=False),
    "e_car": _setting(ncls=1, depth_mode="linear", dim_exp=False, dim_use_std=True, depth_range=(1.0, 60.0), dim_mean=CUSTOM_MEAN[:1],
                      dim_std=CUSTOM_STD[:1]),
    "e_two_classes": _setting(ncls=2, depth_mode="exp", dim_use_std=True, uncertainty_as_conf=False, depth_range=(1.0, 60.0),
                              dim_mean=CUSTOM_MEAN, dim_std=CUSTOM_STD),
}
GOLDEN_MODES = ("soft", "hard", "direct")

# Per-column yardstick of each setting: the worst error, as |a - b| / max(1, |b|), of the float32 reference arithmetic against this
# restatement on the same inputs -- the reference's own PostProcessor rows (tests/golden/decode_cfg.npz) and decode_rows_f32 on every pixel
# of the maps the device cases read -- measured by tests/test_decode_cfg_ref_cpu.py, which prints the figures and asserts that they stay
# below 4x these.  The device kernel gets the same 4x.  Never taken from the kernel.
YARDSTICK = {   # cls, alpha, x1, y1, x2, y2, h, w, l, X, Y, Z, ry, score
    "a_defaults": (0.0, 5.12e-07, 9.54e-07, 4.77e-07, 9.54e-07, 4.77e-07, 8.43e-08, 7.27e-08, 7.53e-08, 2.08e-06, 1.12e-06, 2.85e-07, 7.77e-07, 0.0),
    "a_linear_std": (0.0, 5.12e-07, 9.54e-07, 4.77e-07, 9.54e-07, 4.77e-07, 7.43e-08, 6.82e-08, 8.08e-08, 2.10e-06, 1.14e-06, 2.75e-07, 7.77e-07, 0.0),
    "b_linear_depth": (0.0, 5.12e-07, 9.54e-07, 4.77e-07, 9.54e-07, 4.77e-07, 1.18e-07, 1.42e-07, 1.26e-07, 2.10e-06, 1.17e-06, 2.00e-06, 1.74e-06, 1.29e-07),
    "c_exp_dims_std": (0.0, 5.12e-07, 9.54e-07, 4.77e-07, 9.54e-07, 4.77e-07, 1.13e-07, 1.24e-07, 9.47e-08, 2.10e-06, 1.18e-06, 2.87e-07, 6.85e-07, 1.29e-07),
    "d_linear_dims": (0.0, 5.12e-07, 9.54e-07, 4.77e-07, 9.54e-07, 4.77e-07, 8.43e-08, 7.27e-08, 7.53e-08, 2.08e-06, 1.09e-06, 3.22e-07, 7.09e-07, 1.29e-07),
    "e_car": (0.0, 5.12e-07, 9.54e-07, 4.77e-07, 9.54e-07, 4.77e-07, 8.33e-08, 8.34e-08, 8.66e-08, 1.28e-06, 7.29e-07, 1.84e-06, 7.45e-07, 1.41e-07),
    "e_two_classes": (0.0, 5.12e-07, 9.54e-07, 4.77e-07, 9.54e-07, 4.77e-07, 1.08e-07, 9.04e-08, 1.22e-07, 1.27e-06, 8.00e-07, 2.92e-07, 6.98e-07, 0.0),
}
YARDSTICK["yaml"] = tuple(D.YARDSTICK[c] for c in COLUMNS)      # the runs/monoflex.yaml rules: decode_ref's own yardstick, measured there
# (Where the confidence scaling is off the score column is a copy of the top-K score: its yardstick and bound are 0.  The linear depth
# x * 16.06 + 26.49 cancels near zero: Z of b_linear_depth and e_car carries the rounding of a value near 26, 2e-6.)


def bounds(setting):
    return np.array([BOUND_FACTOR * v for v in YARDSTICK[setting]])


def decode_boxes(hmap, reg_off, scores, index, calib, pad, img_size, threshold, mode="soft", cfg=YAML, wrong=()):
    """-> dict(det (B,K,14), topk (B,K,5), valid (B,K) int32, unc (B,K,2), margins..., census intermediates...), all float64.
    The class count is scores.shape[1] (1 to 3); `cfg` is one of SETTINGS' dicts (its `ncls` is not read)."""
    assert mode in MODES, mode
    wrong = (wrong,) if isinstance(wrong, str) else tuple(wrong)
    assert all(w in WRONG for w in wrong), wrong
    hmap = np.asarray(hmap)
    B, H, W, ld = hmap.shape
    scores, index = np.asarray(scores), np.asarray(index)
    ncls, K = scores.shape[1], scores.shape[2]
    assert scores.shape == index.shape == (B, ncls, K) and 1 <= ncls <= 3
    assert np.isfinite(scores).all() and (index >= 0).all() and (index < H * W).all()
    calib = np.asarray(calib, dtype=np.float64).reshape(B, 6)
    pad = np.asarray(pad, dtype=np.float64).reshape(B, 2)
    img_size = np.asarray(img_size, dtype=np.float64).reshape(2)
    thr = float(np.float32(threshold))                           # the kernel compares float32 with float32
    dmin, dmax = float(cfg["depth_range"][0]), float(cfg["depth_range"][1])
    mean = np.asarray(cfg["dim_mean"], dtype=np.float64)
    std = np.asarray(cfg["dim_std"], dtype=np.float64)
    assert mean.shape[0] >= ncls and std.shape[0] >= ncls and cfg["depth_mode"] in DEPTH_DECODE
    ref0, ref1 = (float(v) for v in cfg["depth_ref"])
    if "depth_ref_swapped" in wrong:
        ref0, ref1 = ref1, ref0
    dim_exp = bool(cfg["dim_exp"]) or "exp_dims_when_linear" in wrong
    use_std = bool(cfg["dim_use_std"]) and "std_ignored" not in wrong
    as_conf = bool(cfg["uncertainty_as_conf"]) or "conf_always_applied" in wrong
    pi = math.pi

    out = {k: np.zeros((B, K)) for k in ("bin_margin", "hard_margin", "alpha_wrap_dist", "ry_wrap_dist", "alpha_raw", "ry_raw", "sigma",
                                         "d_direct_raw", "d1_raw", "d2_raw", "d3_raw")}
    out["best_bin"] = np.zeros((B, K), dtype=np.int64)
    out["hard_choice"] = np.zeros((B, K), dtype=np.int64)
    out["kpt_terms"] = np.zeros((B, K, 5))                       # f_u h / (relu(dy) 4 + eps): centre, pair 0-4, 2-6, 1-5, 3-7
    out["kpt_dy"] = np.zeros((B, K, 5))
    out["box_raw"] = np.zeros((B, K, 4))                         # the 2D box before its clamp
    out["box_max"] = np.zeros((B, 2))
    out["dims"] = np.zeros((B, K, 3))                            # (l, h, w) as decoded
    det, topk, valid, unc = np.zeros((B, K, 14)), np.zeros((B, K, 5)), np.zeros((B, K), dtype=np.int32), np.zeros((B, K, 2))
    for b in range(B):
        pos = stage2_merge(scores[b])
        cls = pos // K                                           # utils.py:91
        sc = scores[b].reshape(-1).astype(np.float64)[pos]
        idx = index[b].reshape(-1).astype(np.int64)[pos]
        ys, xs = idx // W, idx % W
        r = hmap[b].reshape(H * W, ld)[idx, reg_off:reg_off + R_TOTAL].astype(np.float64)
        fu, fv, cu, cv, bx, by = calib[b]
        padx, pady = pad[b]
        px, py = xs.astype(np.float64), ys.astype(np.float64)

        # decode_box2d_fcos (anno_encoder.py:69-86); the clamp uses image 0's size
        wmax, hmax = img_size[0] - 1, img_size[1] - 1
        raw = np.stack(((px - np.maximum(r[:, R_2D + 0], 0)) * DOWN_RATIO - padx, (py - np.maximum(r[:, R_2D + 1], 0)) * DOWN_RATIO - pady,
                        (px + np.maximum(r[:, R_2D + 2], 0)) * DOWN_RATIO - padx, (py + np.maximum(r[:, R_2D + 3], 0)) * DOWN_RATIO - pady), axis=1)
        box = raw.copy()
        box[:, 0::2] = np.clip(box[:, 0::2], 0, wmax)
        box[:, 1::2] = np.clip(box[:, 1::2], 0, hmax)

        # decode_dimension (anno_encoder.py:221-243), (l, h, w): exp(off) or off, then * std + mean or * mean
        row = np.zeros_like(cls) if "mean_of_class0" in wrong else cls
        off = r[:, R_DIM3D:R_DIM3D + 3]
        off = np.exp(off) if dim_exp else off
        dims = off * std[row] + mean[row] if use_std else off * mean[row]
        dl, dh, dw = dims[:, 0], dims[:, 1], dims[:, 2]

        # decode_depth (anno_encoder.py:124-140)
        x = r[:, R_DEPTH]
        if cfg["depth_mode"] == "exp":
            d0_raw = np.exp(x)
        elif cfg["depth_mode"] == "linear":
            d0_raw = x * ref1 + ref0
        else:
            d0_raw = np.exp(-x)                                  # 1 / sigmoid(x) - 1
        d0 = d0_raw if "no_depth_clamp_direct" in wrong else np.clip(d0_raw, dmin, dmax)
        u0 = np.exp(r[:, R_DEPTH_UNC])

        # decode_depth_from_keypoints_batch (anno_encoder.py:187-219); keypoint k = (r[6 + 2k], r[7 + 2k])
        ky = lambda k: r[:, R_KPT + 2 * k + 1]
        kdepth = lambda dy: fu * dh / (np.maximum(dy, 0) * DOWN_RATIO + EPS_KPT)
        dy = np.stack((ky(8) - ky(9), ky(0) - ky(4), ky(2) - ky(6), ky(1) - ky(5), ky(3) - ky(7)), axis=1)
        t = np.stack([kdepth(dy[:, i]) for i in range(5)], axis=1)
        d1_raw, d2_raw, d3_raw = t[:, 0], (t[:, 1] + t[:, 2]) / 2, (t[:, 3] + t[:, 4]) / 2
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
        ori = r[:, R_ORI_OFF:R_ORI_OFF + 8].reshape(K, 4, 2)[np.arange(K), best]
        alpha_raw = np.arctan2(ori[:, 0], ori[:, 1]) + centers[best]
        ry_raw = alpha_raw + np.arctan2(X, Z)
        wrap = lambda x: np.where(x > pi, x - 2 * pi, np.where(x < -pi, x + 2 * pi, x))
        alpha, ry = wrap(alpha_raw), wrap(ry_raw)

        Y = Y + dh / 2                                           # detector_infer.py:215
        conf = 1 - np.clip(sigma, 0.01, 1)                       # :223-229
        final = sc * conf if as_conf else sc
        unc[b] = np.stack((sigma, conf), axis=1) if as_conf else 0.0
        det[b] = np.stack((cls.astype(np.float64), alpha, box[:, 0], box[:, 1], box[:, 2], box[:, 3], dh, dw, dl, X, Y, Z, ry, final), axis=1)
        topk[b] = np.stack((sc, idx.astype(np.float64), cls.astype(np.float64), py, px), axis=1)
        valid[b] = (sc >= thr).astype(np.int32)

        out["bin_margin"][b], out["best_bin"][b] = D._rel_margin(p1), best
        out["hard_margin"][b], out["hard_choice"][b] = D._rel_margin(w_all), hard
        out["alpha_wrap_dist"][b] = np.minimum(np.abs(alpha_raw - pi), np.abs(alpha_raw + pi))
        out["ry_wrap_dist"][b] = np.minimum(np.abs(ry_raw - pi), np.abs(ry_raw + pi))
        out["alpha_raw"][b], out["ry_raw"][b], out["sigma"][b] = alpha_raw, ry_raw, sigma
        out["d_direct_raw"][b], out["d1_raw"][b], out["d2_raw"][b], out["d3_raw"][b] = d0_raw, d1_raw, d2_raw, d3_raw
        out["kpt_terms"][b], out["kpt_dy"][b], out["box_raw"][b], out["box_max"][b], out["dims"][b] = t, dy, raw, (wmax, hmax), dims
    out.update(det=det, topk=topk, valid=valid, unc=unc)
    return out


def decode_rows_f32(hmap, reg_off, scores, index, calib, pad, img_size, mode, cfg):
    """The same decode in float32 torch operations, in the reference's operation order (anno_encoder.py, detector_infer.py:121-232), on the
    rows stage 2 selects -> det (B, K, 14), unc (B, K, 2), float32 numpy.  Not a restatement to test against: the float32 arithmetic whose
    distance from decode_boxes above is measured as the yardstick."""
    import torch
    import torch.nn.functional as F
    hmap, scores, index = np.asarray(hmap), np.asarray(scores), np.asarray(index)
    B, H, W, ld = hmap.shape
    ncls, K = scores.shape[1], scores.shape[2]
    f32 = lambda a: torch.as_tensor(np.asarray(a, dtype=np.float32))
    mean, std = f32(cfg["dim_mean"]), f32(cfg["dim_std"])
    ref = f32(cfg["depth_ref"])
    dmin, dmax = cfg["depth_range"]
    det, unc = np.zeros((B, K, 14), dtype=np.float32), np.zeros((B, K, 2), dtype=np.float32)
    for b in range(B):
        pos = stage2_merge(scores[b])
        cls = torch.as_tensor(pos // K)
        sc = f32(scores[b].reshape(-1)[pos])
        idx = index[b].reshape(-1).astype(np.int64)[pos]
        pts = torch.stack((f32(idx % W), f32(idx // W)), dim=1)
        r = f32(hmap[b].reshape(H * W, ld)[idx, reg_off:reg_off + R_TOTAL])
        fu, fv, cu, cv, bx, by = (float(v) for v in np.asarray(calib, dtype=np.float32).reshape(B, 6)[b])
        padt = f32(np.asarray(pad).reshape(B, 2)[b]).view(1, 2)
        reg2d = F.relu(r[:, R_2D:R_2D + 4])
        box = torch.cat((pts - reg2d[:, :2], pts + reg2d[:, 2:]), dim=1) * DOWN_RATIO - padt.repeat(1, 2)
        box[:, 0::2] = box[:, 0::2].clamp(min=0, max=float(img_size[0]) - 1)
        box[:, 1::2] = box[:, 1::2].clamp(min=0, max=float(img_size[1]) - 1)
        off = r[:, R_DIM3D:R_DIM3D + 3]
        if cfg["dim_exp"]:
            off = off.exp()
        dims = off * std[cls] + mean[cls] if cfg["dim_use_std"] else off * mean[cls]
        x = r[:, R_DEPTH]
        if cfg["depth_mode"] == "exp":
            d0 = x.exp()
        elif cfg["depth_mode"] == "linear":
            d0 = x * ref[1] + ref[0]
        else:
            d0 = 1 / torch.sigmoid(x) - 1
        d0 = torch.clamp(d0, min=dmin, max=dmax)
        u0 = r[:, R_DEPTH_UNC:R_DEPTH_UNC + 1].exp()
        kp = r[:, R_KPT:R_KPT + 20].view(-1, 10, 2)
        h3d = dims[:, 1].clone()
        dc = kp[:, 8, 1] - kp[:, 9, 1]
        d02 = kp[:, [0, 2], 1] - kp[:, [4, 6], 1]
        d13 = kp[:, [1, 3], 1] - kp[:, [5, 7], 1]
        zc = fu * h3d / (F.relu(dc) * DOWN_RATIO + EPS_KPT)
        z02 = (fu * h3d.unsqueeze(-1) / (F.relu(d02) * DOWN_RATIO + EPS_KPT)).mean(dim=1)
        z13 = (fu * h3d.unsqueeze(-1) / (F.relu(d13) * DOWN_RATIO + EPS_KPT)).mean(dim=1)
        d_kpt = torch.stack([t.clamp(min=dmin, max=dmax) for t in (zc, z02, z13)], dim=1)
        u_kpt = r[:, R_KPT_UNC:R_KPT_UNC + 3].exp()
        d_all, u_all = torch.cat((d0.unsqueeze(1), d_kpt), dim=1), torch.cat((u0, u_kpt), dim=1)
        wts = 1 / u_all
        single = {"direct": 0, "keypoints_center": 1, "keypoints_02": 2, "keypoints_13": 3}
        if mode == "soft":
            wts = wts / wts.sum(dim=1, keepdim=True)
            depth, sigma = torch.sum(d_all * wts, dim=1), torch.sum(wts * u_all, dim=1)
        elif mode == "hard":
            depth, sigma = d_all[torch.arange(K), wts.argmax(dim=1)], u_all.min(dim=1).values
        elif mode == "mean":
            depth, sigma = d_all.mean(dim=1), u_all.mean(dim=1)
        elif mode == "keypoints_avg":
            depth, sigma = d_kpt.mean(dim=1), u_kpt.mean(dim=1)
        else:
            depth, sigma = d_all[:, single[mode]], u_all[:, single[mode]]
        uv = (pts + r[:, R_OFF3D:R_OFF3D + 2]) * DOWN_RATIO - padt
        X = ((uv[:, 0] - cu) * depth) / fu + bx
        Y = ((uv[:, 1] - cv) * depth) / fv + by
        bins = torch.softmax(r[:, R_ORI_CLS:R_ORI_CLS + 8].view(-1, 4, 2), dim=2)[..., 1]
        best = bins.argmax(dim=1)
        centers = torch.tensor([0, math.pi / 2, math.pi, -math.pi / 2], dtype=torch.float32)
        ori = r[:, R_ORI_OFF:R_ORI_OFF + 8].view(-1, 4, 2)[torch.arange(K), best]
        alphas = torch.atan2(ori[:, 0], ori[:, 1]) + centers[best]
        rotys = alphas + torch.atan2(X, depth)
        rotys = torch.where(rotys > math.pi, rotys - 2 * math.pi, rotys)
        rotys = torch.where(rotys < -math.pi, rotys + 2 * math.pi, rotys)
        alphas = torch.where(alphas > math.pi, alphas - 2 * math.pi, alphas)
        alphas = torch.where(alphas < -math.pi, alphas + 2 * math.pi, alphas)
        Y = Y + dims[:, 1] / 2
        conf = 1 - torch.clamp(sigma, min=0.01, max=1)
        final = sc * conf if cfg["uncertainty_as_conf"] else sc
        hwl = dims.roll(shifts=-1, dims=1)
        det[b] = torch.cat([cls.float().view(-1, 1), alphas.view(-1, 1), box, hwl, X.view(-1, 1), Y.view(-1, 1), depth.view(-1, 1),
                            rotys.view(-1, 1), final.view(-1, 1)], dim=1).numpy()
        if cfg["uncertainty_as_conf"]:
            unc[b] = torch.stack((sigma, conf), dim=1).numpy()
    return det, unc


def unc_errors(got, ref):
    """Worst |got - want| / max(1, |want|) of the two `unc` columns -> (2,)."""
    want = ref["unc"]
    err = np.abs(np.asarray(got, dtype=np.float64) - want) / np.maximum(1.0, np.abs(want))
    return err.reshape(-1, 2).max(axis=0)


# ---- the inputs the tests run: tests/decode_cases.py's maps and lists, with the first `ncls` class lists of a setting -----------------------
DEVICE_CASES = ("b3_k50", "k1", "k7", "k256", "ld50", "ld72")     # B = 3 with own pad / size / calib; K 1, 7, 256; (ld, reg_off) (50, 0), (64, 8), (72, 13)


def case_inputs(name, setting, kind="distinct"):
    from tests import decode_cases as C
    d = C.case_inputs(name, kind)
    n = SETTINGS[setting]["ncls"]
    return dict(d, scores=np.ascontiguousarray(d["scores"][:, :n]), index=np.ascontiguousarray(d["index"][:, :n]))


def run_ref(d, mode, setting, **kw):
    return decode_boxes(d["hmap"], d["reg_off"], d["scores"], d["index"], d["calib"], d["pad"], d["img_size"], d["threshold"], mode,
                        SETTINGS[setting] if isinstance(setting, str) else setting, **kw)


def census(ref, cfg):
    """Share of the rows that take each branch the configurable decode adds -> {name: share}; counted from the restatement alone."""
    n = ref["det"].shape[0] * ref["det"].shape[1]
    dmin, dmax = cfg["depth_range"]
    d0, sigma = ref["d_direct_raw"].reshape(n), ref["sigma"].reshape(n)
    neg_h = ref["dims"].reshape(n, 3)[:, 1] < 0
    kpt_raw = np.stack([ref[k].reshape(n) for k in ("d1_raw", "d2_raw", "d3_raw")], axis=1)
    c = {
        "direct depth below the range": d0 < dmin, "direct depth above the range": d0 > dmax, "direct depth inside the range": (d0 >= dmin) & (d0 <= dmax),
        "a decoded dimension negative": (ref["dims"].reshape(n, 3) < 0).any(axis=1),
        "height negative: all keypoint depths at the lower clamp": neg_h & (kpt_raw < dmin).all(axis=1),
        "height negative, a keypoint depth NOT at the lower clamp": neg_h & ~(kpt_raw < dmin).all(axis=1),
        "a keypoint span with relu(dy) == 0": (ref["kpt_dy"].reshape(n, 5) <= 0).any(axis=1),
        "sigma below 0.01": sigma < 0.01, "sigma inside [0.01, 1]": (sigma >= 0.01) & (sigma <= 1), "sigma above 1": sigma > 1,
    }
    return {k: float(np.mean(v)) for k, v in c.items()}
