"""PostProcessor (reference model/head/detector_infer.py:20-237) on the gfx950 decode kernels.

The reference decode is batch-1 only; here every image of the batch is decoded by
its own workgroup with the batch-1 semantics (its own calib / pad_size; the 2D-box clamp uses image
0's padded size exactly like `out_size = out_size[0]`, anno_encoder.py:79).  The device always
produces K=50 rows + a validity mask (static shapes, hipGraph-capturable); the `score >= threshold`
compaction of detector_infer.py:102-119 happens when the result is handed to the host.
"""
import numpy as np
import torch
from torch import nn

from ... import lib as L
from ... import ops
from ..layers.utils import Converter_key2channel
from .detector_predictor import HM_LD, REG_OFF


def make_post_processor(cfg):
    key2channel = Converter_key2channel(keys=cfg.MODEL.HEAD.REGRESSION_HEADS, channels=cfg.MODEL.HEAD.REGRESSION_CHANNELS)
    return PostProcessor(cfg=cfg, key2channel=key2channel)


class PostProcessor(nn.Module):
    def __init__(self, cfg, key2channel, anno_encoder=None):
        super().__init__()
        self.key2channel = key2channel
        self.det_threshold = cfg.TEST.DETECTIONS_THRESHOLD
        self.max_detection = cfg.TEST.DETECTIONS_PER_IMG
        self.output_width = cfg.INPUT.WIDTH_TRAIN // cfg.MODEL.BACKBONE.DOWN_RATIO
        self.output_height = cfg.INPUT.HEIGHT_TRAIN // cfg.MODEL.BACKBONE.DOWN_RATIO
        self.output_depth = cfg.MODEL.HEAD.OUTPUT_DEPTH
        self.uncertainty_as_conf = cfg.TEST.UNCERTAINTY_AS_CONFIDENCE
        self.num_classes = len(cfg.DATASETS.DETECT_CLASSES)
        # What the decode kernel cannot do is refused; every head setting the loss evaluator accepts (DEPTH_MODE, DEPTH_REFERENCE,
        # DEPTH_RANGE, DIMENSION_REG, DIMENSION_MEAN / _STD) and TEST.UNCERTAINTY_AS_CONFIDENCE reach it through mfx_decode_cfg.
        # The head set (lib.HeadSet, the loss evaluator's reading too) decides which OUTPUT_DEPTH can be served: what the reference raises on
        # is refused here.
        hs = self.head_set = L.HeadSet([key2channel.keys], [key2channel.channels])
        s = self.decode_settings = L.head_decode_settings(cfg)      # the same reading of the config as Loss_Computation's
        refused = []
        if self.output_depth not in L.DEPTH_MODES and self.output_depth != 'oracle':
            refused.append("OUTPUT_DEPTH %r" % (self.output_depth,))
        else:
            hs.check_output_depth(self.output_depth)
        if cfg.INPUT.ORIENTATION != 'multi-bin' or cfg.INPUT.ORIENTATION_BIN_SIZE != 4:
            refused.append("an orientation other than multi-bin with 4 bins")
        if s["down_ratio"] != 4:
            refused.append("DOWN_RATIO != 4")
        if s["depth_range"] is None:
            refused.append("DEPTH_RANGE None (the keypoint depths are clamped to it)")
        if s["depth_mode"] not in L.DEPTH_DECODES:
            refused.append("DEPTH_MODE %r" % (s["depth_mode"],))
        if not 1 <= self.num_classes <= 3:
            refused.append("%d classes (1 to 3)" % self.num_classes)
        if len(s["dim_mean"]) < self.num_classes or len(s["dim_std"]) < self.num_classes or len(s["dim_mean"]) > 3 or len(s["dim_std"]) > 3:
            refused.append("DIMENSION_MEAN / DIMENSION_STD with fewer rows than classes (or more than three)")
        if refused:
            raise NotImplementedError("the HIP decode kernel does not implement: " + "; ".join(refused))
        self.decode_cfg = L.decode_cfg(s, self.uncertainty_as_conf)
        self.head_layout = hs.layout()
        self.reg_width = hs.R
        # TEST.EVAL_DEPTH / TEST.EVAL_DIS_IOUS (detector_infer.py:37-38,86-89): the ground-truth diagnostics of a validation pass, evaluated on
        # the device at the labelled centres (ops.eval_diagnostics).  What the head set cannot serve is refused here, as above.
        self.eval_depth, self.eval_dis_iou = bool(cfg.TEST.EVAL_DEPTH), bool(cfg.TEST.EVAL_DIS_IOUS)
        if self.eval_depth and not hs.full:
            raise NotImplementedError("TEST.EVAL_DEPTH with the %s: the depth errors read depth_uncertainty, corner_offset and corner_uncertainty "
                                      "(detector_infer.py:296-300)" % hs.describe())
        if self.eval_dis_iou and self.output_depth == 'oracle':
            raise NotImplementedError("TEST.EVAL_DIS_IOUS with OUTPUT_DEPTH 'oracle': the disentangled boxes take the depth of one decode mode "
                                      "(%s)" % ", ".join(L.DEPTH_MODES))
        # TEST.USE_NMS / NMS_THRESH / NMS_CLASS_AGNOSTIC: declared by the reference (config/defaults.py) and read by none of its files.  Here
        # '2d' / '3d' suppress duplicate detections on the device after the decode (ops.box_nms; the semantics are in INTEGRATION.md);
        # 'none', the default, launches nothing.  A user who turns it on without a usable threshold is told.
        self.use_nms, self.nms_thresh = cfg.TEST.USE_NMS, float(cfg.TEST.NMS_THRESH)
        self.nms_class_agnostic = bool(cfg.TEST.NMS_CLASS_AGNOSTIC)
        if self.use_nms != 'none' and self.use_nms not in L.NMS_KINDS:
            raise ValueError("TEST.USE_NMS %r is not one of 'none', %s" % (self.use_nms, ", ".join(repr(k) for k in L.NMS_KINDS)))
        if self.use_nms != 'none':
            if not 0.0 <= self.nms_thresh < 1.0:
                raise ValueError("TEST.NMS_THRESH %r with TEST.USE_NMS %r: the IoU threshold must be in [0, 1) (the default -1 means "
                                 "\"not set\")" % (cfg.TEST.NMS_THRESH, self.use_nms))
            if self.max_detection > L.NMS_MAX_ROWS:
                raise NotImplementedError("TEST.USE_NMS %r with TEST.DETECTIONS_PER_IMG %d: the suppression kernel keeps one image's pair matrix "
                                          "and ranking in one workgroup's LDS, at most %d rows" % (self.use_nms, self.max_detection, L.NMS_MAX_ROWS))

    @staticmethod
    def prepare_targets(targets, device):
        """pad_size (B,2) int32, calib (B,6) fp32 [f_u,f_v,c_u,c_v,b_x,b_y], size (2,) int32 of image 0."""
        pad = torch.stack([torch.as_tensor(t.get_field("pad_size")) for t in targets]).to(device=device, dtype=torch.int32)
        calib = torch.from_numpy(np.stack([t.get_field("calib").as_f32() if hasattr(t.get_field("calib"), "as_f32")
                                           else _calib_f32(t.get_field("calib")) for t in targets])).to(device)
        size = torch.tensor(list(targets[0].size), dtype=torch.int32, device=device)
        return pad.contiguous(), calib.contiguous(), size

    def decode_device(self, hm, pad, calib, size, cls_planar=None, return_unc=False, gt_rows=None):
        """hm fp32 (B,H,W,64) -> det (B,K,14), topk (B,K,5) [score, flat index, cls, y, x], valid (B,K) int32
        [, unc (B,K,2) = estimated_depth_error, uncertainty_conf].  Under TEST.USE_NMS '2d' / '3d' valid is the mask after the suppression
        (one more launch, ops.box_nms); det and topk are what they are without it.  `gt_rows` (B,M,8) (ops.oracle_gt_rows): the ground truth
        output_depth 'oracle' matches against on the device (one ops.decode_boxes_multi launch); 'oracle' without it is refused."""
        if self.output_depth == 'oracle':
            if gt_rows is None:
                raise ValueError("output_depth = 'oracle' reads the ground truth of each image: pass gt_rows (ops.oracle_gt_rows), or call the "
                                 "module (forward) with the dataset's targets")
            out = self._decode_oracle_device(hm, pad, calib, size, cls_planar, gt_rows)
            out = out if return_unc else out[:3]
        else:
            out = self._decode(hm, pad, calib, size, cls_planar, return_unc)
        if self.use_nms == 'none':
            return out
        return tuple(out[:2]) + (self.suppress(out[0], out[2]),) + tuple(out[3:])

    def _decode_oracle_device(self, hm, pad, calib, size, cls_planar, gt_rows):
        """`output_depth = 'oracle'` on the device: (det, topk, valid, unc), what decode_oracle assembles on the host."""
        self.head_set.check_output_depth('oracle')
        scores, index = ops.decode_topk(hm, 0, self.num_classes, self.max_detection, planar=cls_planar)
        det, topk, valid, unc, _ = ops.decode_boxes_multi(hm, REG_OFF, scores, index, calib, pad, size, float(self.det_threshold), ('oracle',),
                                                          self.decode_cfg, heads=self.head_layout, gt_rows=gt_rows, return_unc=True)
        return det[:, 0], topk, valid, unc[:, 0]

    def decode_all_device(self, hm, pad, calib, size, cls_planar, methods, gt_rows=None, return_unc=False):
        """The rows of every depth method of `methods` (names of head_set.output_depths(), 'oracle' with `gt_rows`) from one top-K and one
        ops.decode_boxes_multi launch: det (B,NM,K,14), topk (B,K,5), valid (B,NM,K) int32, unc (B,NM,K,2) or None; slice i is what
        decode_device gives under output_depth = methods[i].  Under TEST.USE_NMS valid is the mask after ONE ops.box_nms launch on the
        (B * NM, K, 14) view; without it the decode's mask repeated."""
        methods = list(methods)
        for m in methods:
            self.head_set.check_output_depth(m)
        if 'oracle' in methods and gt_rows is None:
            raise ValueError("output_depth = 'oracle' reads the ground truth of each image: pass gt_rows (ops.oracle_gt_rows)")
        scores, index = ops.decode_topk(hm, 0, self.num_classes, self.max_detection, planar=cls_planar)
        det, topk, valid, unc, _ = ops.decode_boxes_multi(hm, REG_OFF, scores, index, calib, pad, size, float(self.det_threshold), methods,
                                                          self.decode_cfg, heads=self.head_layout, gt_rows=gt_rows, return_unc=return_unc)
        B, NM, K = det.shape[:3]
        valid = valid[:, None, :].expand(B, NM, K).contiguous()
        if self.use_nms != 'none':
            valid = self.suppress(det.reshape(B * NM, K, 14), valid.reshape(B * NM, K)).reshape(B, NM, K)
        return det, topk, valid, unc

    def suppress(self, det, valid):
        """valid (B,K) after TEST.USE_NMS '2d' / '3d' on the rows det (B,K,14): ops.box_nms, one launch, no host synchronisation."""
        return ops.box_nms(det, valid, self.use_nms, self.nms_thresh, self.nms_class_agnostic)

    def _decode(self, hm, pad, calib, size, cls_planar, return_unc):
        """The decode alone: top-K and box rows, valid = score >= threshold."""
        scores, index = ops.decode_topk(hm, 0, self.num_classes, self.max_detection, planar=cls_planar)
        # (`output_depth` is read at every call: engine/inference.py:166 re-assigns it between the passes of `eval_all_depths`)
        self.head_set.check_output_depth(self.output_depth)
        return ops.decode_boxes(hm, REG_OFF, scores, index, calib, pad, size, float(self.det_threshold), depth_mode=self.output_depth,
                                cfg=self.decode_cfg, return_unc=return_unc, heads=self.head_layout)

    @property
    def diagnostics_wanted(self):
        """mfx_eval_diagnostics' `want`: bit 0 = TEST.EVAL_DEPTH, bit 1 = TEST.EVAL_DIS_IOUS."""
        return (1 if self.eval_depth else 0) | (2 if self.eval_dis_iou else 0)

    def diagnose_device(self, hm, gt_rows, pad, calib):
        """hm fp32 (B,H,W,64), gt_rows (B,M,16) (ops.eval_diag_rows) -> (depth_err (B,M,13) or None, iou (B,M,5) or None): the fixed-shape
        tables of the flags that are on, zeros in the empty slots; one launch, no host synchronisation."""
        want = self.diagnostics_wanted
        if not want:
            return None, None
        # (`output_depth` is read at every call, as decode_device does)
        if want & 2:
            if self.output_depth == 'oracle':
                raise NotImplementedError("TEST.EVAL_DIS_IOUS with output_depth 'oracle'")
            self.head_set.check_output_depth(self.output_depth)
        c = L.DecodeCfg.from_buffer_copy(self.decode_cfg)
        c.output_depth = L.DEPTH_MODES[self.output_depth] if want & 2 else L.DEPTH_MODES['direct']
        return ops.eval_diagnostics(hm, REG_OFF, gt_rows, calib, pad, c, self.head_layout, want=want)

    @staticmethod
    def diagnostics_tables(depth_err, iou, mask):
        """The fixed-shape tables -> the reference's dicts {key: 1-D tensor over the valid objects in (image, slot) order}
        (detector_infer.py:341-357,450); None for a table that was not computed."""
        keep = mask.reshape(-1).bool()
        rows = lambda t, keys: None if t is None else {k: t.reshape(-1, len(keys))[keep, i] for i, k in enumerate(keys)}
        return rows(depth_err, ops.EVAL_DEPTH_KEYS), rows(iou, ops.EVAL_IOU_KEYS)

    def forward(self, predictions, targets, features=None, test=False, refine_module=None):
        hm = predictions['hm_nhwc']
        pad, calib, size = self.prepare_targets(targets, hm.device)
        depth_errors = dis_ious = None
        if self.diagnostics_wanted:
            gt_rows = ops.eval_diag_rows(targets, hm.device)            # ValueError on targets without labels (the `test` split)
            depth_errors, dis_ious = self.diagnostics_tables(*self.diagnose_device(hm, gt_rows, pad, calib), gt_rows[..., 0])
        if self.output_depth == 'oracle':                                    # matched on the device; decode_oracle below is the host form of the rule
            self.head_set.check_output_depth('oracle')
            det, topk, valid, unc = self._decode_oracle_device(hm, pad, calib, size, predictions.get('cls_planar'),
                                                               ops.oracle_gt_rows(targets, hm.device))
        else:
            det, topk, valid, unc = self._decode(hm, pad, calib, size, predictions.get('cls_planar'), True)
        # TEST.USE_NMS: on the rows the decode (under 'oracle': the per-detection choice of row) produced; everything below follows the mask
        # after it, and 'valid_pre_nms' carries the decode's own
        valid_pre = None
        if self.use_nms != 'none':
            valid_pre, valid = valid, self.suppress(det, valid)
        keep = valid.bool()
        results = [det[b][keep[b]] for b in range(det.shape[0])]          # host sync, as detector_infer.py:106
        vis_scores = [topk[b][keep[b], 0] for b in range(det.shape[0])]
        one = lambda rows: rows[0] if len(results) == 1 else rows
        # detector_infer.py:223-229,234-235: the valid rows' values under UNCERTAINTY_AS_CONFIDENCE, None without it -- and None where the head
        # set has no uncertainty head for the chosen depth (estimated_depth_error is None there: the score stays raw)
        report = self.uncertainty_as_conf and self.head_set.has_depth_error(self.output_depth)
        depth_error = one([unc[b][keep[b], 0] for b in range(det.shape[0])]) if report else None
        unc_conf = one([unc[b][keep[b], 1] for b in range(det.shape[0])]) if report else None
        eval_utils = {'dis_ious': dis_ious, 'depth_errors': depth_errors, 'vis_scores': one(vis_scores), 'uncertainty_conf': unc_conf,
                      'estimated_depth_error': depth_error, 'topk': topk, 'valid': valid, 'det_all': det, 'valid_pre_nms': valid_pre}
        visualize_preds = {'heat_map': predictions['cls']}
        result = results[0] if len(results) == 1 else results
        return result, eval_utils, visualize_preds

    def decode_oracle(self, hm, pad, calib, size, cls_planar, targets):
        """`output_depth = 'oracle'` (detector_infer.py:199-202, get_oracle_depths :238-277; the first method engine/inference.py:154 evaluates):
        every detection takes, of its four (three without depth_uncertainty) depth estimates, the one closest to the depth of the ground-truth object it overlaps (nearest box centre
        of its class, 2D IoU >= 0.5), and the mean of the four when it overlaps none.  The depth only enters a row through location, rotation and
        the uncertainty-scaled score, so the row of a detection under 'oracle' IS its row from the decode of the chosen single estimate (or of
        'mean'): five launches of the box kernel on one top-K, and a per-detection choice of row on the host, where the ground truth is.
        (The reference reads targets[0] only -- it evaluates at batch 1; here image b reads targets[b].)"""
        scores, index = ops.decode_topk(hm, 0, self.num_classes, self.max_detection, planar=cls_planar)
        # the single-estimate decodes whose rows are chosen among, in the column order of the reference's pred_combined_depths
        # (detector_infer.py:173-182): direct, then the three keypoint groups -- the three alone for a head set without depth_uncertainty
        self.head_set.check_output_depth('oracle')
        columns = self.head_set.oracle_columns()
        dec = {m: ops.decode_boxes(hm, REG_OFF, scores, index, calib, pad, size, float(self.det_threshold), depth_mode=m, cfg=self.decode_cfg,
                                   return_unc=True, heads=self.head_layout)
               for m in ('mean',) + columns}
        det, topk, valid, _ = dec['mean']
        rows = {m: d[0].cpu() for m, d in dec.items()}
        uncs = {m: d[3].cpu() for m, d in dec.items()}
        valid_h = valid.cpu().bool()
        out, out_unc = rows['mean'].clone(), uncs['mean'].clone()
        for b, t in enumerate(targets):
            mask = torch.as_tensor(t.get_field('reg_mask')).bool().cpu()
            gt_cls = torch.as_tensor(t.get_field('cls_ids')).cpu()[mask]
            gt_box = torch.as_tensor(t.get_field('gt_bboxes')).cpu()[mask].float()
            gt_depth = torch.as_tensor(t.get_field('locations')).cpu()[mask][:, -1].float()
            if gt_box.shape[0] == 0:
                continue
            gt_centre = (gt_box[:, :2] + gt_box[:, 2:]) / 2
            for i in torch.nonzero(valid_h[b]).flatten().tolist():
                box = rows['mean'][b, i, 2:6]
                dis = torch.sum((((box[:2] + box[2:]) / 2).reshape(1, 2) - gt_centre) ** 2, dim=1)
                dis[gt_cls != int(rows['mean'][b, i, 0])] = 9999
                near = int(torch.argmin(dis))
                if _box_iou(box.numpy(), gt_box[near].numpy()) < 0.5:            # (a 0 / 0 overlap is not "< 0.5": such a pair counts as met, :268-270)
                    continue
                est = torch.stack([rows[m][b, i, 11] for m in columns])     # row[11] = location z = the depth that decode used
                chosen = columns[int(torch.argmin(torch.abs(est - gt_depth[near])))]
                out[b, i], out_unc[b, i] = rows[chosen][b, i], uncs[chosen][b, i]
        return out.to(det.device), topk, valid, out_unc.to(det.device)


def _box_iou(a, b):
    """engine/visualize_infer.py:23-27, in the float32 scalars the reference computes it in."""
    with np.errstate(invalid='ignore', divide='ignore'):
        inter = max(min(a[2], b[2]) - max(a[0], b[0]), 0) * max(min(a[3], b[3]) - max(a[1], b[1]), 0)
        return inter / ((a[2] - a[0]) * (a[3] - a[1]) + (b[2] - b[0]) * (b[3] - b[1]) - inter)


def _calib_f32(c):
    return np.array([c.f_u, c.f_v, c.c_u, c.c_v, c.b_x, c.b_y], dtype=np.float32)
