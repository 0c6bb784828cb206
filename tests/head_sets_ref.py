"""float64 restatement of the training loss and of the box decode for the reference's REDUCED head sets (its ablation ladder).

The reference's loss (model/head/detector_loss.py:116-493) and post-processor (model/head/detector_infer.py:121-235) accept a family of
MODEL.HEAD.REGRESSION_HEADS: six keys are required (2d_dim, 3d_offset, 3d_dim, ori_cls, ori_offset, depth), three are optional --
depth_uncertainty (du), corner_offset (kp) and corner_uncertainty (cu, only with kp) -- in any grouping and order.  This module restates
both for any such set, independently of monoflex_amd: `loss_ref` in float64 torch (the reference's own compaction by boolean masks,
gradients from autograd), `decode_ref` in float64 numpy.  tests/test_head_sets_ref_cpu.py anchors them to tests/golden/head_sets.npz
(recorded from the reference itself by tools/gen_head_sets_golden.py) and, for the full set, to the restatements the suite already pins
(tests/decode_cfg_ref.py, the float64 tensor-op loss of tests/test_object_loss_configs_cpu.py); the shim, kernel and Python tests then
compare the code under test with these two functions.  Nothing here imports the code under test.

SETS: the six sets of the ladder.  Four of them use a channel order that differs from runs/monoflex.yaml (the depth branch first, the
uncertainties ahead of the keypoints ...), so that a hard-wired channel offset cannot pass.  `take` slices and permutes a canonical
50-channel map (the runs/monoflex.yaml order every seeded input of the suite is drawn in) into a set's layout.
"""
import math

import numpy as np
import torch

WIDTH = {'2d_dim': 4, '3d_offset': 2, 'corner_offset': 20, 'corner_uncertainty': 3, '3d_dim': 3, 'ori_cls': 8, 'ori_offset': 8, 'depth': 1,
         'depth_uncertainty': 1}
KEYS = tuple(WIDTH)                                              # the order of mfx_object_loss_cfg.ch[] / mfx_head_layout.ch[]
# channel starts of runs/monoflex.yaml: the canonical order of the seeded inputs
CANON = {'2d_dim': 0, '3d_offset': 4, 'corner_offset': 6, 'corner_uncertainty': 26, '3d_dim': 29, 'ori_cls': 32, 'ori_offset': 40, 'depth': 48,
         'depth_uncertainty': 49}

SETS = {   # name = du kp cu
    "s000": [['depth'], ['2d_dim'], ['3d_offset'], ['3d_dim'], ['ori_cls', 'ori_offset']],                                    # the depth branch first
    "s100": [['2d_dim'], ['3d_offset'], ['3d_dim'], ['ori_cls', 'ori_offset'], ['depth'], ['depth_uncertainty']],
    "s010": [['2d_dim'], ['3d_offset'], ['corner_offset'], ['3d_dim'], ['ori_cls', 'ori_offset'], ['depth']],
    "s110": [['corner_offset'], ['depth', 'depth_uncertainty'], ['2d_dim'], ['3d_offset'], ['ori_cls', 'ori_offset'], ['3d_dim']],
    "s011": [['depth'], ['corner_uncertainty'], ['2d_dim'], ['3d_offset'], ['corner_offset'], ['3d_dim'], ['ori_cls', 'ori_offset']],
    "s111": [['2d_dim'], ['3d_offset'], ['corner_offset'], ['corner_uncertainty'], ['3d_dim'], ['ori_cls', 'ori_offset'], ['depth'],
             ['depth_uncertainty']],                                                                                         # runs/monoflex.yaml
}
NEW_SETS = ("s000", "s100", "s010", "s110", "s011")
WIDTHS = {"s000": 26, "s100": 27, "s010": 46, "s110": 47, "s011": 49, "s111": 50}

CORNER_DEPTHS = ('direct', 'keypoint_mean', 'soft_combine', 'hard_combine')
OUTPUT_DEPTHS = ('soft', 'hard', 'mean', 'direct', 'keypoints_avg', 'keypoints_center', 'keypoints_02', 'keypoints_13')       # MFX_DEPTH_* order
LOSS_NAMES = ('hm_loss', 'bbox_loss', 'depth_loss', 'offset_loss', 'orien_loss', 'dims_loss', 'corner_loss', 'keypoint_loss',
              'keypoint_depth_loss', 'trunc_offset_loss', 'weighted_avg_depth_loss')                                          # runs/monoflex.yaml order
LOSS_WEIGHTS = dict(zip(LOSS_NAMES, (1, 1, 1, 0.5, 1, 1, 0.2, 1.0, 0.2, 0.1, 0.2)))


def channels(name):
    return [[WIDTH[k] for k in group] for group in SETS[name]]


def flags(name):
    """(du, kp, cu) of a set."""
    keys = [k for g in SETS[name] for k in g]
    return 'depth_uncertainty' in keys, 'corner_offset' in keys, 'corner_uncertainty' in keys


def layout(name):
    """-> ({key: first channel}, R)."""
    starts, s = {}, 0
    for g in SETS[name]:
        for k in g:
            starts[k] = s
            s += WIDTH[k]
    assert s == WIDTHS[name]
    return starts, s


def ch_table(name):
    """The nine channel starts in KEYS order, -1 for an absent key (what mfx_object_loss_cfg.ch / mfx_head_layout.ch must hold)."""
    starts, _ = layout(name)
    return [starts.get(k, -1) for k in KEYS]


# ---- the ladder's acceptance matrix (the issue's table: what the reference itself runs without raising) -----------------------------------
def corner_depths(name):
    du, kp, cu = flags(name)
    return ('direct',) + (('keypoint_mean',) if kp else ()) + (('soft_combine', 'hard_combine') if du and kp and cu else ())


def output_depths(name):
    du, kp, cu = flags(name)
    return ('direct',) + (('keypoints_avg', 'keypoints_center', 'keypoints_02', 'keypoints_13') if kp else ()) + (('soft', 'hard', 'mean') if cu else ())


def has_depth_error(name, mode):
    """Whether the reference's estimated_depth_error is not None under OUTPUT_DEPTH `mode`."""
    du, kp, cu = flags(name)
    return du if mode == 'direct' else cu


def loss_names(name, drop=()):
    """The runs/monoflex.yaml LOSS_NAMES a set can serve (and their weights), without those in `drop`."""
    du, kp, cu = flags(name)
    out = [n for n in LOSS_NAMES if n not in drop and (kp or n not in ('keypoint_loss', 'keypoint_depth_loss')) and (cu or n != 'weighted_avg_depth_loss')]
    return out, [LOSS_WEIGHTS[n] for n in out]


def expected_loss_keys(name, names):
    return set(names)


def expected_log_keys(name, names):
    du, kp, cu = flags(name)
    keys = {'2D_IoU', '3D_IoU', 'depth_loss', 'depth_MAE'} | set(names)
    if kp:
        keys |= {'center_MAE', '02_MAE', '13_MAE'}
    if cu:
        keys |= {'lower_MAE', 'hard_MAE', 'soft_MAE', 'mean_MAE'}
    return keys


def take(canon, name, axis, ld=None, off=0, junk=None):
    """Slice and permute the canonical 50 channels along `axis` of a numpy array / tensor into a set's layout; with `ld` the R channels sit
    at [off, off + R) of an ld-wide axis whose other entries are `junk` (same type, ld wide) -- values that must never be read."""
    starts, R = layout(name)
    is_t = torch.is_tensor(canon)
    idx = [0] * R
    for k, s in starts.items():
        for i in range(WIDTH[k]):
            idx[s + i] = CANON[k] + i
    sel = canon.index_select(axis, torch.tensor(idx)) if is_t else np.take(canon, idx, axis=axis)
    if ld is None:
        return sel.contiguous() if is_t else np.ascontiguousarray(sel)
    assert off + R <= ld and junk is not None and junk.shape[axis] == ld
    out = junk.clone() if is_t else junk.copy()
    sl = [slice(None)] * out.ndim
    sl[axis] = slice(off, off + R)
    out[tuple(sl)] = sel
    return out


# ---- loss --------------------------------------------------------------------------------------------------------------------------------
KITTI_MEAN = ((3.8840, 1.5261, 1.6286), (0.8423, 1.7607, 0.6602), (1.7635, 1.7372, 0.5968))
KITTI_STD = ((0.4259, 0.1367, 0.1022), (0.2349, 0.1133, 0.1427), (0.1766, 0.0948, 0.1242))


def yaml_settings(**kw):
    """The loss / decode settings of runs/monoflex.yaml as plain values."""
    s = dict(depth_mode='inv_sigmoid', depth_ref=(26.494627, 16.05988), depth_range=(0.1, 100.0), dim_exp=True, dim_use_std=False,
             dim_mean=KITTI_MEAN, dim_std=KITTI_STD, unc_range=(-10.0, 10.0), down_ratio=4.0, eps=1e-3, iou='giou', trunc_log=True,
             modify_invalid=True, dim_weight=(1.0, 1.0, 1.0), corner_depth='direct', uncertainty_as_conf=True)
    s.update(kw)
    return s


def _calib(t):
    """[f_u, f_v, c_u, c_v, b_x, b_y] as the float32 values the kernels read (data/datasets/kitti_utils.py:213-218), in float64."""
    P = np.asarray(t["P"], dtype=np.float64).reshape(3, 4)
    c = np.array([P[0, 0], P[1, 1], P[0, 2], P[1, 2], P[0, 3] / -P[0, 0], P[1, 3] / -P[1, 1]])
    return c.astype(np.float32).astype(np.float64)


def _decode_depth(x, S):
    if S["depth_mode"] == 'exp':
        d = x.exp()
    elif S["depth_mode"] == 'linear':
        d = x * S["depth_ref"][1] + S["depth_ref"][0]
    else:
        d = 1 / torch.sigmoid(x) - 1
    return d.clamp(min=S["depth_range"][0], max=S["depth_range"][1])


def _locations(pts, off, depth, cal, pad, S):
    uv = (pts + off) * S["down_ratio"] - pad
    return torch.stack(((uv[:, 0] - cal[:, 2]) * depth / cal[:, 0] + cal[:, 4], (uv[:, 1] - cal[:, 3]) * depth / cal[:, 1] + cal[:, 5], depth), dim=1)


def _corners(ry, dims, loc):
    c, s = ry.cos(), ry.sin()
    sx = torch.tensor([-1., -1, 1, 1, -1, -1, 1, 1], dtype=dims.dtype)
    sy = torch.tensor([1., 1, 1, 1, -1, -1, -1, -1], dtype=dims.dtype)
    sz = torch.tensor([-1., 1, 1, -1, -1, 1, 1, -1], dtype=dims.dtype)
    x, y, z = dims[:, 0:1] * 0.5 * sx, dims[:, 1:2] * 0.5 * sy, dims[:, 2:3] * 0.5 * sz
    return torch.stack((c[:, None] * x + s[:, None] * z + loc[:, 0:1], y + loc[:, 1:2], -s[:, None] * x + c[:, None] * z + loc[:, 2:3]), dim=2)


def _f(t):
    return float(t.detach()) if torch.is_tensor(t) else float(t)


class LossRef:
    """Result of loss_ref: terms {name: 0-d float64 tensor on the graph of `reg`}, logs {name: float}, the gathered rows and intermediates."""


def loss_ref(name, reg, tg, S, names, weights):
    """The regression terms of the reference's Loss_Computation for head set `name` (hm_loss is left out: it does not read the regression map).
    reg (B, R, H, W) float64 tensor in the set's layout (requires_grad for gradients); tg: the per-image target dicts of
    monoflex_amd.synthetic.synthetic_train_target; `names` / `weights`: LOSS_NAMES / INIT_LOSS_WEIGHT.  The 3D_IoU log is not restated."""
    du, kp, cu = flags(name)
    starts, R = layout(name)
    W = dict(zip(names, (_f(w) for w in weights)))
    assert reg.dtype == torch.float64 and reg.shape[1] == R
    f64 = lambda k: torch.stack([torch.as_tensor(np.asarray(t[k])) for t in tg]).double()
    mask = torch.stack([torch.as_tensor(np.asarray(t["reg_mask"])) for t in tg]).bool()
    B, M = mask.shape
    bi = torch.arange(B).view(B, 1).expand(B, M)[mask]
    cen = torch.stack([torch.as_tensor(np.asarray(t["target_centers"])) for t in tg]).long()[mask]
    n = int(mask.sum())
    poi = reg.permute(0, 2, 3, 1)[bi, cen[:, 1], cen[:, 0]]                       # (n, R)
    key = lambda k: poi[:, starts[k]:starts[k] + WIDTH[k]]
    cal_all = torch.tensor(np.stack([_calib(t) for t in tg]))
    cal = cal_all[bi]
    pad = f64("pad_size")[bi]
    pts = cen.double()
    box = f64("2d_bboxes")[mask]
    m2d = ((box[:, 3] - box[:, 1]) > 0) & ((box[:, 2] - box[:, 0]) > 0)
    t_depth = f64("locations")[mask][:, 2]
    t_off, t_dims, t_ry, t_ori = f64("offset_3D")[mask], f64("dimensions")[mask], f64("rotys")[mask], f64("orientations")[mask]
    cls = torch.stack([torch.as_tensor(np.asarray(t["cls_ids"])) for t in tg]).long()[mask]
    trunc = torch.stack([torch.as_tensor(np.asarray(t["trunc_mask"])) for t in tg]).bool()[mask]
    t_loc = _locations(pts, t_off, t_depth, cal, pad, S)
    t_cor = _corners(t_ry, t_dims, t_loc)

    out = LossRef()
    out.n, out.bi, out.cen, out.poi, out.m2d = n, bi, cen, poi, m2d
    terms, logs = {}, {}
    lo, hi = S["unc_range"]
    # 2D box
    p2 = torch.relu(key('2d_dim'))[m2d]
    t2 = torch.cat((pts - box[:, :2], box[:, 2:] - pts), dim=1)[m2d]
    out.p2, out.t2 = p2, t2
    pl, pt, pr, pb = p2.unbind(1)
    tl, tt, tr, tb = t2.unbind(1)
    t_area, p_area = (tl + tr) * (tt + tb), (pl + pr) * (pt + pb)
    w_i, h_i = torch.min(pl, tl) + torch.min(pr, tr), torch.min(pb, tb) + torch.min(pt, tt)
    g_w, g_h = torch.max(pl, tl) + torch.max(pr, tr), torch.max(pb, tb) + torch.max(pt, tt)
    ac, inter = g_w * g_h + 1e-7, w_i * h_i
    union = t_area + p_area - inter
    iou = (inter + 1.0) / (union + 1.0)
    l2 = {'iou': -torch.log(iou), 'linear_iou': 1 - iou, 'giou': 1 - (iou - (ac - union) / ac)}[S["iou"]]
    if int(m2d.sum()) > 0:
        terms['bbox_loss'] = W['bbox_loss'] * l2.mean()
        logs['2D_IoU'] = _f(iou.mean())
    else:
        terms['bbox_loss'], logs['2D_IoU'] = reg.sum() * 0, 0.0
    # decoded predictions
    off = key('3d_dim')
    off = off.exp() if S["dim_exp"] else off
    mean, std = torch.tensor(S["dim_mean"], dtype=torch.float64)[cls], torch.tensor(S["dim_std"], dtype=torch.float64)[cls]
    p_dims = off * std + mean if S["dim_use_std"] else off * mean
    p_depth = _decode_depth(key('depth')[:, 0], S)
    out.p_depth = p_depth
    if du:
        d_unc = key('depth_uncertainty')[:, 0].clamp(min=lo, max=hi)
    if kp:
        kpt = key('corner_offset').reshape(n, 10, 2)
        # the focal length is the one of the image's RANK among those that own an object (anno_encoder.py:198-199)
        present = sorted(set(bi.tolist()))
        fu = torch.tensor([float(cal_all[present.index(int(b)), 0]) for b in bi.tolist()], dtype=torch.float64)
        solve = lambda dh: fu * p_dims[:, 1] / (torch.relu(dh) * S["down_ratio"] + S["eps"])
        ky = kpt[:, :, 1]
        kd = torch.stack((solve(ky[:, 8] - ky[:, 9]), (solve(ky[:, 0] - ky[:, 4]) + solve(ky[:, 2] - ky[:, 6])) / 2,
                          (solve(ky[:, 1] - ky[:, 5]) + solve(ky[:, 3] - ky[:, 7])) / 2), dim=1)
        kd = kd.clamp(min=S["depth_range"][0], max=S["depth_range"][1])
        out.kd = kd
    if cu:
        c_unc = key('corner_uncertainty').clamp(min=lo, max=hi)
    if cu and du:
        comb_d, comb_u = torch.cat((p_depth[:, None], kd), dim=1), torch.cat((d_unc[:, None], c_unc), dim=1).exp()
    elif cu:
        comb_d, comb_u = kd, c_unc.exp()
    if cu:
        wts = 1 / comb_u
        wts = wts / wts.sum(dim=1, keepdim=True)
        soft = (comb_d * wts).sum(dim=1)
        out.comb_u = comb_u
    mode = S["corner_depth"]
    assert mode in corner_depths(name), (name, mode)
    if mode == 'direct':
        c_depth = p_depth
    elif mode == 'keypoint_mean':
        c_depth = kd.mean(dim=1)
    elif mode == 'soft_combine':
        c_depth = soft
    else:
        c_depth = comb_d[torch.arange(n), comb_u.argmin(dim=1)]
    p_loc = _locations(pts, key('3d_offset'), c_depth, cal, pad, S)
    ori_cls, ori_off = key('ori_cls'), key('ori_offset')
    conf = torch.softmax(ori_cls.reshape(n, 4, 2), dim=2)[..., 1]
    out.bin_conf = conf
    best = conf.argmax(dim=1)
    centers = torch.tensor([0, math.pi / 2, math.pi, -math.pi / 2], dtype=torch.float64)
    oo = ori_off.reshape(n, 4, 2)[torch.arange(n), best]
    ry = torch.atan2(oo[:, 0], oo[:, 1]) + centers[best] + torch.atan2(p_loc[:, 0], p_loc[:, 2])
    ry = torch.where(ry > math.pi, ry - 2 * math.pi, ry)
    ry = torch.where(ry < -math.pi, ry + 2 * math.pi, ry)
    p_cor = _corners(ry, p_dims, p_loc)
    # depth
    d_l1 = W['depth_loss'] * (p_depth - t_depth).abs()
    logs['depth_loss'] = _f(d_l1.mean())
    terms['depth_loss'] = (d_l1 * torch.exp(-d_unc) + d_unc * W['depth_loss']).mean() if du else d_l1.mean()
    # offset
    o_l1 = (key('3d_offset') - t_off).abs().sum(dim=1)
    if 'trunc_offset_loss' in W:
        tl1 = torch.log(1 + o_l1[trunc]) if S["trunc_log"] else o_l1[trunc]
        terms['trunc_offset_loss'] = W['trunc_offset_loss'] * tl1.sum() / max(int(trunc.sum()), 1)
        terms['offset_loss'] = W['offset_loss'] * (o_l1[~trunc].mean() if int((~trunc).sum()) else o_l1.sum() * 0)
    else:
        terms['offset_loss'] = W['offset_loss'] * o_l1.mean()
    # orientation (Real_MultiBin_loss)
    cls_l, reg_l, reg_n = 0, 0, 0
    for i in range(4):
        cls_l = cls_l + torch.nn.functional.cross_entropy(ori_cls[:, 2 * i:2 * i + 2], t_ori[:, i].long(), reduction='mean')
        sel = t_ori[:, i] == 1
        if int(sel.sum()):
            o = torch.nn.functional.normalize(ori_off[sel][:, 2 * i:2 * i + 2])
            reg_l = reg_l + ((o[:, 0] - torch.sin(t_ori[sel, 4 + i])).abs() + (o[:, 1] - torch.cos(t_ori[sel, 4 + i])).abs()).sum()
            reg_n += int(sel.sum())
    terms['orien_loss'] = W['orien_loss'] * (cls_l / 4 + reg_l / max(reg_n, 1))
    terms['dims_loss'] = W['dims_loss'] * ((p_dims - t_dims).abs() * torch.tensor(S["dim_weight"], dtype=torch.float64)).sum(dim=1).mean()
    if 'corner_loss' in W:
        terms['corner_loss'] = W['corner_loss'] * (p_cor - t_cor).abs().sum(dim=2).mean()
    depth_mae = (p_depth - t_depth).abs() / t_depth
    logs['depth_MAE'] = _f(depth_mae.mean())
    if kp:
        tk = f64("keypoints")[mask]
        kmask = tk[..., 2]
        kl = W['keypoint_loss'] * (kpt - tk[..., :2]).abs().sum(dim=2) * kmask
        terms['keypoint_loss'] = kl.sum() / kmask.sum().clamp(min=1)
        kdm = f64("keypoints_depth_mask")[mask].bool()
        out.kdm = kdm
        if 'keypoint_depth_loss' in W:
            wk = W['keypoint_depth_loss']
            t_kd = t_depth[:, None].repeat(1, 3)
            valid_l = wk * (kd[kdm] - t_kd[kdm]).abs()
            invalid_l = wk * (kd[~kdm].detach() - t_kd[~kdm]).abs()
            logs['keypoint_depth_loss'] = _f(valid_l.mean()) if int(kdm.sum()) else 0.0
            if cu:
                valid_l = valid_l * torch.exp(-c_unc[kdm]) + wk * c_unc[kdm]
                invalid_l = invalid_l * torch.exp(-c_unc[~kdm])
            valid_l = valid_l.sum() / max(int(kdm.sum()), 1)
            invalid_l = invalid_l.sum() / max(int((~kdm).sum()), 1)
            terms['keypoint_depth_loss'] = valid_l + invalid_l if S["modify_invalid"] else valid_l
        k_mae = (kd - t_depth[:, None]).abs() / t_depth[:, None]
        logs.update({'center_MAE': _f(k_mae[:, 0].mean()), '02_MAE': _f(k_mae[:, 1].mean()), '13_MAE': _f(k_mae[:, 2].mean())})
    if cu:
        c_mae = torch.cat((depth_mae[:, None], k_mae), dim=1) if du else k_mae
        logs.update({'lower_MAE': _f(c_mae.min(dim=1)[0].mean()), 'hard_MAE': _f(c_mae[torch.arange(n), comb_u.argmin(dim=1)].mean()),
                     'soft_MAE': _f(((soft - t_depth).abs() / t_depth).mean()),
                     'mean_MAE': _f(((comb_d.mean(dim=1) - t_depth).abs() / t_depth).mean())})
        if 'weighted_avg_depth_loss' in W:
            terms['weighted_avg_depth_loss'] = W['weighted_avg_depth_loss'] * (soft - t_depth).abs().mean()
    for k in list(terms):
        if k not in W:
            del terms[k]
    for k, v in terms.items():
        logs.setdefault(k, _f(v))
    out.terms, out.logs = terms, logs
    return out


def near_selection_rows(ref, rel=1e-5):
    """Valid rows whose float64 margin at a selection (orientation arg-max, arg-min of the combined uncertainties, an untied min / max of the
    GIoU) is below `rel` relative: the float32 code may legitimately select the other candidate there.  (n,) bool."""
    drop = torch.zeros(ref.n, dtype=torch.bool)
    conf = ref.bin_conf.detach().sort(dim=1, descending=True)[0]
    drop |= (conf[:, 0] - conf[:, 1]) < rel * conf[:, 0]
    if hasattr(ref, "comb_u"):
        u = ref.comb_u.detach().sort(dim=1)[0]
        drop |= ((u[:, 1] - u[:, 0]) < rel * u[:, 1]) & (u[:, 1] != u[:, 0])
    p, t = ref.p2.detach(), ref.t2
    near = (((p - t).abs() < rel * t.abs().clamp(min=1e-30)) & (p != t)).any(dim=1)
    rows = torch.nonzero(ref.m2d).flatten()
    drop[rows[near]] = True
    return drop


def term_gradients(ref, reg, term_names):
    """Each term's gradient at the valid rows' centre pixels, summed per pixel as a scatter would: (len(term_names), n, R) float64; a term
    the set does not have gives zeros.  Asserts that nothing off the centres receives a gradient."""
    g = torch.zeros(len(term_names), ref.n, reg.shape[1], dtype=torch.float64)
    for i, k in enumerate(term_names):
        if k in ref.terms and ref.terms[k].requires_grad:
            d, = torch.autograd.grad(ref.terms[k], reg, retain_graph=True, allow_unused=True)
            if d is not None:
                d = d.permute(0, 2, 3, 1)
                g[i] = d[ref.bi, ref.cen[:, 1], ref.cen[:, 0]]
                rest = d.clone()
                rest[ref.bi, ref.cen[:, 1], ref.cen[:, 0]] = 0
                assert float(rest.abs().max()) == 0.0
    return g


# ---- decode ------------------------------------------------------------------------------------------------------------------------------
def decode_ref(name, hmap, reg_off, scores, index, calib, pad, img_size, threshold, mode, S):
    """The box decode (mfx_decode_boxes_heads) for head set `name` -> dict(det (B,K,14), topk (B,K,5), valid (B,K), unc (B,K,2)) float64.
    Conventions of tests/decode_cfg_ref.py: every float32 input is the exact real number it holds; `unc` is 0 where the reference's
    estimated_depth_error is None (no confidence scaling asked, or no uncertainty head for the chosen depth); the score is then raw."""
    from tests.decode_ref import stage2_merge
    du, kp, cu = flags(name)
    assert mode in output_depths(name), (name, mode)
    starts, R = layout(name)
    hmap, scores, index = np.asarray(hmap), np.asarray(scores), np.asarray(index)
    B, H, W, ld = hmap.shape
    ncls, K = scores.shape[1], scores.shape[2]
    calib = np.asarray(calib, dtype=np.float64).reshape(B, 6)
    pad = np.asarray(pad, dtype=np.float64).reshape(B, 2)
    img_size = np.asarray(img_size, dtype=np.float64).reshape(2)
    thr = float(np.float32(threshold))
    dmin, dmax = S["depth_range"]
    mean, std = np.asarray(S["dim_mean"], dtype=np.float64), np.asarray(S["dim_std"], dtype=np.float64)
    down, eps, pi = S["down_ratio"], S["eps"], math.pi
    as_conf = bool(S["uncertainty_as_conf"]) and has_depth_error(name, mode)
    det, topk, valid, unc = np.zeros((B, K, 14)), np.zeros((B, K, 5)), np.zeros((B, K), dtype=np.int32), np.zeros((B, K, 2))
    # the margins of the discontinuous decisions, as tests/decode_ref.py reports them (read by its near_rows / column_errors)
    margins = {k: np.full((B, K), np.inf) for k in ("bin_margin", "hard_margin", "alpha_wrap_dist", "ry_wrap_dist")}
    rel_margin = lambda v: (np.sort(v, axis=-1)[..., -1] - np.sort(v, axis=-1)[..., -2]) / np.maximum(np.abs(np.sort(v, axis=-1)[..., -1]), 1e-300)
    for b in range(B):
        pos = stage2_merge(scores[b])
        cls = pos // K
        sc = scores[b].reshape(-1).astype(np.float64)[pos]
        idx = index[b].reshape(-1).astype(np.int64)[pos]
        ys, xs = idx // W, idx % W
        r = hmap[b].reshape(H * W, ld)[idx, reg_off:reg_off + R].astype(np.float64)
        key = lambda k: r[:, starts[k]:starts[k] + WIDTH[k]]
        fu, fv, cu_, cv, bx, by = calib[b]
        px, py = xs.astype(np.float64), ys.astype(np.float64)
        e = np.maximum(key('2d_dim'), 0)
        box = np.stack(((px - e[:, 0]) * down - pad[b, 0], (py - e[:, 1]) * down - pad[b, 1], (px + e[:, 2]) * down - pad[b, 0],
                        (py + e[:, 3]) * down - pad[b, 1]), axis=1)
        box[:, 0::2] = np.clip(box[:, 0::2], 0, img_size[0] - 1)
        box[:, 1::2] = np.clip(box[:, 1::2], 0, img_size[1] - 1)
        off = np.exp(key('3d_dim')) if S["dim_exp"] else key('3d_dim')
        dims = off * std[cls] + mean[cls] if S["dim_use_std"] else off * mean[cls]
        x = key('depth')[:, 0]
        d0 = {'exp': lambda: np.exp(x), 'linear': lambda: x * S["depth_ref"][1] + S["depth_ref"][0], 'inv_sigmoid': lambda: np.exp(-x)}[S["depth_mode"]]()
        d0 = np.clip(d0, dmin, dmax)
        cols_d, cols_u = [], []
        if du:
            u0 = np.exp(key('depth_uncertainty')[:, 0])
        if kp:
            ky = key('corner_offset')[:, 1::2]
            kdepth = lambda dy: fu * dims[:, 1] / (np.maximum(dy, 0) * down + eps)
            kd = np.stack((kdepth(ky[:, 8] - ky[:, 9]), (kdepth(ky[:, 0] - ky[:, 4]) + kdepth(ky[:, 2] - ky[:, 6])) / 2,
                           (kdepth(ky[:, 1] - ky[:, 5]) + kdepth(ky[:, 3] - ky[:, 7])) / 2), axis=1)
            kd = np.clip(kd, dmin, dmax)
        if cu:
            ku = np.exp(key('corner_uncertainty'))
        sigma = np.zeros(K)
        if mode == 'direct':
            depth = d0
            if du:
                sigma = u0
        elif mode.startswith('keypoints'):
            c = {'keypoints_center': 0, 'keypoints_02': 1, 'keypoints_13': 2}.get(mode)
            depth = kd.mean(axis=1) if c is None else kd[:, c]
            if cu:
                sigma = ku.mean(axis=1) if c is None else ku[:, c]
        else:
            d_all, u_all = (np.concatenate((d0[:, None], kd), axis=1), np.concatenate((u0[:, None], ku), axis=1)) if du else (kd, ku)
            w_all = 1 / u_all
            margins["hard_margin"][b] = rel_margin(w_all)
            if mode == 'hard':
                depth, sigma = d_all[np.arange(K), np.argmax(w_all, axis=1)], u_all.min(axis=1)
            elif mode == 'soft':
                wn = w_all / w_all.sum(axis=1, keepdims=True)
                depth, sigma = (d_all * wn).sum(axis=1), (wn * u_all).sum(axis=1)
            else:
                depth, sigma = d_all.mean(axis=1), u_all.mean(axis=1)
        o3 = key('3d_offset')
        u, v = (px + o3[:, 0]) * down - pad[b, 0], (py + o3[:, 1]) * down - pad[b, 1]
        X, Y, Z = (u - cu_) * depth / fu + bx, (v - cv) * depth / fv + by, depth
        oc = key('ori_cls')
        a, c = oc[:, 0::2], oc[:, 1::2]
        m = np.maximum(a, c)
        p1 = np.exp(c - m) / (np.exp(a - m) + np.exp(c - m))
        best = np.argmax(p1, axis=1)
        ori = key('ori_offset').reshape(K, 4, 2)[np.arange(K), best]
        alpha = np.arctan2(ori[:, 0], ori[:, 1]) + np.array([0.0, pi / 2, pi, -pi / 2])[best]
        ry = alpha + np.arctan2(X, Z)
        wrap = lambda t: np.where(t > pi, t - 2 * pi, np.where(t < -pi, t + 2 * pi, t))
        margins["bin_margin"][b] = rel_margin(p1)
        margins["alpha_wrap_dist"][b] = np.minimum(np.abs(alpha - pi), np.abs(alpha + pi))
        margins["ry_wrap_dist"][b] = np.minimum(np.abs(ry - pi), np.abs(ry + pi))
        alpha, ry = wrap(alpha), wrap(ry)
        Y = Y + dims[:, 1] / 2
        conf = 1 - np.clip(sigma, 0.01, 1)
        final = sc * conf if as_conf else sc
        if as_conf:
            unc[b] = np.stack((sigma, conf), axis=1)
        det[b] = np.stack((cls.astype(np.float64), alpha, box[:, 0], box[:, 1], box[:, 2], box[:, 3], dims[:, 1], dims[:, 2], dims[:, 0],
                           X, Y, Z, ry, final), axis=1)
        topk[b] = np.stack((sc, idx.astype(np.float64), cls.astype(np.float64), py, px), axis=1)
        valid[b] = (sc >= thr).astype(np.int32)
    return dict(margins, det=det, topk=topk, valid=valid, unc=unc)
