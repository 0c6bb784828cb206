"""Device tests of the several-modes-and-oracle box decode (csrc/decode_multi.hip, mfx_decode_boxes_multi) and of what stands on it:
PostProcessor.decode_device / forward under OUTPUT_DEPTH 'oracle', decode_all_device, KeypointDetector.detect_device(gt_rows=...) inside a
hipGraph, and the one-pass form of `--eval_all_depths`.

Expected everywhere: EQUALITY (torch.equal / byte-identical files).  Every slice of a launch is bit for bit the row the single-mode launch
(mfx_decode_boxes_heads) writes; an oracle row is bit for bit the row of the mode it chose, and the choice is the one the host form
(PostProcessor.decode_oracle, pinned to the reference's recorded rows by tests/test_gpu_ops.py) and the float32 restatement of
tests/test_decode_oracle_cpu.py make.  Shapes: the 24 x 40 maps of tests/decode_cases.py at B = 3 / 1 and K = 50 / 7; the 96 x 320 map only
for the reference's two recorded cases."""
import ctypes
import functools
import os

import numpy as np
import pytest
import torch

from tests import decode_cases as C
from tests import head_sets_cases as HC
from tests import head_sets_ref as HS
from tests.test_decode_oracle_cpu import restate

pytestmark = pytest.mark.gpu
DEV = "cuda"
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LD, CH_OFF = 64, 8
P = lambda t: None if t is None else ctypes.c_void_p(t.data_ptr())                     # noqa: E731
MODES8 = HS.OUTPUT_DEPTHS                                            # MFX_DEPTH_* order
COLUMN_MODES = ("direct", "keypoints_center", "keypoints_02", "keypoints_13")


@pytest.fixture(scope="module", autouse=True)
def _release_cached_inputs():
    """The cases below are cached on the device across tests: drop them, and the allocator's blocks, when the module is done."""
    yield
    _inputs.cache_clear()
    _built.cache_clear()
    torch.cuda.synchronize()
    torch.cuda.empty_cache()


def _L():
    from monoflex_amd import lib as L
    from monoflex_amd import ops
    return ops, L


def _decode_cfg(uac):
    from monoflex_amd import lib as L
    s = HC.settings()
    head = dict(depth_mode=s["depth_mode"], depth_range=tuple(s["depth_range"]), depth_ref=tuple(s["depth_ref"]), dim_mean=s["dim_mean"],
                dim_std=s["dim_std"], dim_modes=["exp", True, False], down_ratio=4, eps=1e-3)
    return L.decode_cfg(head, uac)


def _layout(name):
    from monoflex_amd import lib as L
    return L.HeadSet(HS.SETS[name], HS.channels(name)).layout()


@functools.lru_cache(maxsize=None)
def _inputs(case, name, B, ncls):
    """(hmap, reg_off, scores, index, calib, pad, img_size, threshold) on the device: a case of tests/decode_cases.py, its 50 channels in the
    set's layout, the first B images, the first ncls classes' lists."""
    d = C.case_inputs(case)
    hm = HS.take(d["hmap"][..., CH_OFF:CH_OFF + 50], name, 3, ld=LD, off=CH_OFF, junk=d["hmap"])
    t = lambda a, dt: torch.from_numpy(np.ascontiguousarray(a)).to(DEV, dt)
    return (t(hm[:B], torch.float32), CH_OFF, t(d["scores"][:B, :ncls], torch.float32), t(d["index"][:B, :ncls], torch.int32),
            t(d["calib"][:B], torch.float32), t(d["pad"][:B], torch.int32), t(d["img_size"], torch.int32), float(d["threshold"]))


def _gt_from_rows(rows, valid, columns, M, every=1, cls_of=None, shift=0.125):
    """One image's table (M, 8) built on the host from its decoded rows: an object per `every`-th valid detection -- its 2D box shifted by
    multiples of 1/8 px, its class (or cls_of), a depth next to the estimate of one column (the columns taken in turn)."""
    t = np.zeros((M, 8), dtype=np.float32)
    n = 0
    for i in np.nonzero(valid)[0][::every]:
        if n == M:
            break
        col = columns[n % len(columns)]
        t[n, 0] = 1
        t[n, 1] = rows["mean"][i, 0] if cls_of is None else cls_of
        t[n, 2:6] = rows["mean"][i, 2:6] + np.float32(shift * (n % 3))
        t[n, 6] = rows[col][i, 11] + np.float32(0.015625)
        n += 1
    return t


# ---- 1: every mode against the single-mode launch --------------------------------------------------------------------------------------------
@pytest.mark.parametrize("ncls", [3, 1])
@pytest.mark.parametrize("uac", [True, False])
@pytest.mark.parametrize("case,B", [("b3_k50", 3), ("k7", 3), ("b3_k50", 1)])
@pytest.mark.parametrize("name", ["s111", "s011"])
def test_every_slice_is_the_single_mode_launch(name, case, B, uac, ncls):
    ops, L = _L()
    args = _inputs(case, name, B, ncls)
    modes = [m for m in MODES8 if m in HS.output_depths(name)]
    assert len(modes) == 8                                               # (s011 serves all eight: soft / hard / mean on its three keypoint depths)
    cfg, lay = _decode_cfg(uac), _layout(name)
    det, topk, valid, unc, choice = ops.decode_boxes_multi(*args, modes, cfg, heads=lay, return_unc=True)
    assert choice is None and tuple(det.shape) == (B, len(modes), args[2].shape[2], 14) and tuple(unc.shape) == tuple(det.shape[:3]) + (2,)
    # the order asked for is the order returned, whatever the bit order
    back = ops.decode_boxes_multi(*args, modes[::-1], cfg, heads=lay, return_unc=True)
    torch.cuda.synchronize()
    differ = 0
    for i, m in enumerate(modes):
        one = ops.decode_boxes(*args, depth_mode=m, cfg=cfg, return_unc=True, heads=lay)
        what = "%s %s %s B=%d uac=%d ncls=%d" % (name, case, m, B, uac, ncls)
        assert torch.equal(det[:, i], one[0]) and torch.equal(topk, one[1]) and torch.equal(valid, one[2]) and torch.equal(unc[:, i], one[3]), what
        assert torch.equal(back[0][:, len(modes) - 1 - i], one[0]) and torch.equal(back[3][:, len(modes) - 1 - i], one[3]), what
        differ += int(not torch.equal(det[:, i], det[:, 0]))
    assert differ >= len(modes) - 2                                     # (the slices are different rows: not one mode written eight times)
    if name == "s111":                                                   # the nine-key layout is the default
        d2 = ops.decode_boxes_multi(*args, modes, cfg, return_unc=False)
        assert d2[3] is None and torch.equal(d2[0], det)


# ---- 2: the device oracle against the host form -----------------------------------------------------------------------------------------------
def _target(size, pad, Pmat, fields=None):
    from monoflex_amd.structures.params_3d import Calibration, ParamsList
    t = ParamsList(image_size=tuple(size), is_train=False)
    t.add_field("pad_size", torch.as_tensor(pad, dtype=torch.int64))
    t.add_field("calib", Calibration(Pmat))
    for k, v in (fields or {}).items():
        t.add_field(k, v)
    return t


def _fields(table):
    """The dataset's fields of one image from its (M, 8) table."""
    t = torch.from_numpy(table)
    loc = torch.zeros(table.shape[0], 3)
    loc[:, 2] = t[:, 6]
    return dict(reg_mask=t[:, 0].to(torch.uint8), cls_ids=t[:, 1].to(torch.int64), gt_bboxes=t[:, 2:6].clone(), locations=loc)


def _compare_with_host(post, hm, targets, want_unc=True):
    """decode_device(gt_rows=...) and forward against decode_oracle -> (host det, valid, unc, topk, gt_rows)."""
    ops, L = _L()
    pad, calib, size = post.prepare_targets(targets, DEV)
    assert post.output_depth == "oracle"
    h_det, h_topk, h_valid, h_unc = post.decode_oracle(hm, pad, calib, size, None, targets)
    gt_rows = ops.oracle_gt_rows(targets, DEV)
    assert gt_rows.dtype == torch.float32 and gt_rows.shape[0] == len(targets) and gt_rows.shape[2] == 8
    det, topk, valid, unc = post.decode_device(hm, pad, calib, size, gt_rows=gt_rows, return_unc=True)
    assert torch.equal(det, h_det) and torch.equal(valid, h_valid) and torch.equal(unc, h_unc) and torch.equal(topk, h_topk)
    assert len(post.decode_device(hm, pad, calib, size, gt_rows=gt_rows)) == 3
    res, ev, _ = post({"hm_nhwc": hm, "cls": None}, targets)
    res = [res] if torch.is_tensor(res) else res
    for b in range(len(targets)):
        assert torch.equal(res[b], h_det[b][h_valid[b].bool()])
    assert torch.equal(ev["det_all"], h_det) and torch.equal(ev["valid"], h_valid)
    return h_det, h_valid, h_unc, h_topk, gt_rows


@pytest.mark.parametrize("n", [0, 1])
def test_device_oracle_on_the_reference_cases(golden_dir, n):
    from monoflex_amd import synthetic as S
    from monoflex_amd.config import get_cfg
    from monoflex_amd.model.head.detector_infer import make_post_processor
    g = np.load(os.path.join(golden_dir, "decode_only.npz"))
    tgt = S.synthetic_target(320, 96)
    post = make_post_processor(get_cfg(os.path.join(ROOT, "runs", "monoflex.yaml"), [HC.HEAD + "OUTPUT_DEPTH", "oracle"]))
    gen = torch.Generator().manual_seed(int(g["case%d_seed" % n]))
    logits = torch.randn(1, 3, 96, 320, generator=gen) * 0.8 - 2.0 + float(g["case%d_shift" % n])
    reg = torch.randn(1, 50, 96, 320, generator=gen) * 0.7
    hm = torch.zeros(1, 96, 320, 64)
    hm[..., :3] = logits.permute(0, 2, 3, 1)
    hm[..., 8:58] = reg.permute(0, 2, 3, 1)
    G = g["case%d_gt_boxes" % n].shape[0]
    table = np.zeros((G + 2, 8), dtype=np.float32)
    table[:G, 0], table[:G, 1], table[:G, 2:6], table[:G, 6] = 1, g["case%d_gt_cls" % n], g["case%d_gt_boxes" % n], g["case%d_gt_depth" % n]
    t = _target(tgt["size"], tgt["pad_size"], tgt["P"], _fields(table))
    h_det, h_valid, _, _, gt_rows = _compare_with_host(post, hm.to(DEV), [t])
    assert torch.equal(gt_rows[0].cpu(), torch.from_numpy(table))
    want = g["case%d_result_oracle" % n]
    got = h_det[0][h_valid[0].bool()].cpu().numpy()
    assert got.shape == want.shape and np.allclose(got, want, rtol=1e-4, atol=2e-3)


@functools.lru_cache(maxsize=None)
def _built(name):
    """The built case on the 24 x 40 maps: B = 3, K = 50; image 0 has an object next to every valid detection (depths next to each column in
    turn), image 1 has no object, image 2 has objects of a class no detection has (the first of them on a detection's box).
    -> (post, hm, targets, tables, single-mode rows per image)."""
    from monoflex_amd.model.head.detector_infer import make_post_processor
    ops, L = _L()
    images = (0, 1, 2)
    scores, index = C.peak_lists(21, 3, 50, [(0.3, 0.98), (0.02, 0.23), (0.02, 0.23)])
    maps = C.structured_maps(31, images)
    hm = HS.take(maps["hmap"][..., CH_OFF:CH_OFF + 50], name, 3, ld=LD, off=CH_OFF, junk=maps["hmap"])
    hm[..., :3] = C.peak_logits(scores, index)
    hm = torch.from_numpy(hm).to(DEV)
    post = make_post_processor(HC.cfg_for(name, extra=[HC.HEAD + "OUTPUT_DEPTH", "oracle", "INPUT.WIDTH_TRAIN", C.W * 4, "INPUT.HEIGHT_TRAIN", C.H * 4]))
    columns = post.head_set.oracle_columns()
    bare = [_target(C.IMAGES[i]["size"], C.IMAGES[i]["pad"], C.image_P(i)) for i in images]
    pad, calib, size = post.prepare_targets(bare, DEV)
    rows = {}
    for m in ("mean",) + columns:                                      # the 'mean' and single-estimate decodes first
        post.output_depth = m
        d = post._decode(hm, pad, calib, size, None, True)
        rows[m], valid = d[0].cpu().numpy(), d[2].cpu().numpy()
    post.output_depth = "oracle"
    M = 64
    per = lambda b: {m: r[b] for m, r in rows.items()}
    tables = [_gt_from_rows(per(0), valid[0], columns, M), np.zeros((M, 8), dtype=np.float32),
              _gt_from_rows(per(2), valid[2], columns, M, every=3, cls_of=5)]
    targets = [_target(C.IMAGES[i]["size"], C.IMAGES[i]["pad"], C.image_P(i), _fields(tables[b])) for b, i in enumerate(images)]
    return post, hm, targets, tables, rows, valid


def _host_choice(has_direct, tables, rows, topk, threshold):
    """The restatement's choice per detection (B, K) from the single-mode rows (the callers check that the rows it picks are the host form's)."""
    B, K = rows["mean"].shape[:2]
    d = np.stack([rows[m][..., 11] if m in rows else np.zeros((B, K), np.float32) for m in COLUMN_MODES], axis=2)
    return np.stack([restate(rows["mean"][b, :, 2:6], rows["mean"][b, :, 0].astype(np.int32), topk[b, :, 0], np.float32(threshold), d[b],
                             has_direct, tables[b]) for b in range(B)])


@pytest.mark.parametrize("name", ["s111", "s011"])
def test_device_oracle_on_the_built_case(name):
    post, hm, targets, tables, rows, valid = _built(name)
    h_det, h_valid, h_unc, h_topk, gt_rows = _compare_with_host(post, hm, targets)
    assert all(torch.equal(gt_rows[b].cpu(), torch.from_numpy(tables[b])) for b in range(3))
    # what the host form answered: every choice occurs, a third of the valid detections are matched, the special images behave
    choice = _host_choice(post.head_set.du, tables, rows, h_topk.cpu().numpy(), post.det_threshold)
    picked = np.stack([np.stack([rows["mean" if c < 0 else COLUMN_MODES[c]][b, i] for i, c in enumerate(choice[b])]) for b in range(3)])
    assert np.array_equal(picked, h_det.cpu().numpy())                   # the restatement's choice IS the host form's
    v = h_valid.cpu().numpy().astype(bool)
    assert np.array_equal(v, valid.astype(bool)) and (choice[~v] == -1).all()
    assert set(choice[v].tolist()) == ({-1, 0, 1, 2, 3} if name == "s111" else {-1, 1, 2, 3})
    print("%s built case: valid %s, matched %s" % (name, v.sum(axis=1).tolist(), (choice >= 0).sum(axis=1).tolist()))
    assert (choice >= 0).sum() * 3 >= v.sum() and v[1].sum() > 5 and v[2].sum() > 5
    assert (choice[1] == -1).all() and 1 <= (choice[2] >= 0).sum() < v[2].sum()


# ---- 3: the oracle in a combined launch, its choice, and under NMS --------------------------------------------------------------------------------
@pytest.mark.parametrize("name,K,B", [("s111", 50, 3), ("s111", 7, 3), ("s011", 50, 1)])
def test_oracle_in_a_combined_launch(name, K, B):
    ops, L = _L()
    args = _inputs("b3_k50" if K == 50 else "k7", name, B, 3)
    cfg, lay = _decode_cfg(True), _layout(name)
    modes = [m for m in MODES8 if m in HS.output_depths(name)]
    columns = [m for m in COLUMN_MODES if m in modes and (m != "direct" or name == "s111")]
    single = {m: ops.decode_boxes(*args, depth_mode=m, cfg=cfg, return_unc=True, heads=lay) for m in modes}
    rows = {m: single[m][0].cpu().numpy() for m in modes}
    valid = single["mean"][2].cpu().numpy()
    M = 40
    tables = [_gt_from_rows({m: r[b] for m, r in rows.items()}, valid[b], columns, M, every=1 + b) for b in range(B)]
    gt_rows = torch.from_numpy(np.stack(tables)).to(DEV)
    alone = ops.decode_boxes_multi(*args, ["oracle"], cfg, heads=lay, gt_rows=gt_rows, return_unc=True)
    both = ops.decode_boxes_multi(*args, ["soft", "oracle"] + [m for m in modes if m != "soft"], cfg, heads=lay, gt_rows=gt_rows, return_unc=True)
    torch.cuda.synchronize()
    assert tuple(both[0].shape) == (B, len(modes) + 1, K, 14)
    assert torch.equal(both[0][:, 1], alone[0][:, 0]) and torch.equal(both[3][:, 1], alone[3][:, 0]) and torch.equal(both[4], alone[4])
    assert torch.equal(both[0][:, 0], single["soft"][0]) and torch.equal(both[0][:, 2], single[[m for m in modes if m != "soft"][0]][0])
    # the choice is the restatement's (the host form's: test_device_oracle_on_the_built_case), and each row is the row of its choice
    want = _host_choice(name == "s111", tables, rows, single["mean"][1].cpu().numpy(), args[7])
    choice = alone[4].cpu().numpy()
    assert np.array_equal(choice, want)
    assert (want >= 0).sum() >= max(2, valid.sum() // 4) and (want == -1).sum() >= 1
    uncs = {m: single[m][3].cpu().numpy() for m in modes}
    for b in range(B):
        for i, c in enumerate(choice[b]):
            m = "mean" if c < 0 else COLUMN_MODES[c]
            assert np.array_equal(alone[0][b, 0, i].cpu().numpy(), rows[m][b, i]) and np.array_equal(alone[3][b, 0, i].cpu().numpy(), uncs[m][b, i])


def test_oracle_under_nms_and_all_methods():
    """TEST.USE_NMS '2d': decode_device's mask is ops.box_nms on the host form's rows; decode_all_device gives every method's rows and one
    suppression launch over the (B * NM, K, 14) view."""
    from monoflex_amd.model.head.detector_infer import make_post_processor
    ops, L = _L()
    post, hm, targets, tables, rows, valid = _built("s111")
    nms = make_post_processor(HC.cfg_for("s111", extra=[HC.HEAD + "OUTPUT_DEPTH", "oracle", "INPUT.WIDTH_TRAIN", C.W * 4, "INPUT.HEIGHT_TRAIN", C.H * 4,
                                                        "TEST.USE_NMS", "2d", "TEST.NMS_THRESH", 0.3]))
    pad, calib, size = post.prepare_targets(targets, DEV)
    gt_rows = ops.oracle_gt_rows(targets, DEV)
    h_det, _, h_valid, _ = post.decode_oracle(hm, pad, calib, size, None, targets)
    det, _, mask = nms.decode_device(hm, pad, calib, size, gt_rows=gt_rows)
    want = ops.box_nms(h_det, h_valid, "2d", 0.3, False)
    assert torch.equal(det, h_det) and torch.equal(mask, want) and int(want.sum()) < int(h_valid.sum())
    methods = ["oracle", "hard", "soft", "mean", "direct", "keypoints_center", "keypoints_02", "keypoints_13"]
    lib = L.load()
    n0, m0 = lib.mfx_get_counter(b"box_nms"), lib.mfx_get_counter(b"decode_multi")
    a_det, a_topk, a_valid, a_unc = nms.decode_all_device(hm, pad, calib, size, None, methods, gt_rows=gt_rows, return_unc=True)
    assert lib.mfx_get_counter(b"box_nms") == n0 + 1 and lib.mfx_get_counter(b"decode_multi") == m0 + 1
    p_det, _, p_valid, _ = post.decode_all_device(hm, pad, calib, size, None, methods, gt_rows=gt_rows)
    assert tuple(a_det.shape) == (3, 8, 50, 14) and tuple(a_valid.shape) == (3, 8, 50) and torch.equal(a_det, p_det)
    for i, m in enumerate(methods):
        nms.output_depth = post.output_depth = m
        one = nms.decode_device(hm, pad, calib, size, return_unc=True, gt_rows=gt_rows)
        assert torch.equal(a_det[:, i], one[0]) and torch.equal(a_valid[:, i], one[2]) and torch.equal(a_unc[:, i], one[3]), m
        assert torch.equal(p_valid[:, i], post.decode_device(hm, pad, calib, size, gt_rows=gt_rows)[2])
    post.output_depth = "oracle"
    with pytest.raises(ValueError):
        post.decode_all_device(hm, pad, calib, size, None, methods)          # 'oracle' without its table
    with pytest.raises(ValueError):
        post.decode_device(hm, pad, calib, size)
    with pytest.raises(NotImplementedError):
        make_post_processor(HC.cfg_for("s010", extra=[HC.HEAD + "OUTPUT_DEPTH", "direct"])).decode_all_device(hm, pad, calib, size, None, ["soft"])


# ---- 4 and 7: the model ----------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def small_model():
    from tests.test_gpu_e2e import _hip_model
    return _hip_model(-1.0, "bf16", 48, 24)


def _model_inputs(m, B=2):
    from monoflex_amd import synthetic as S
    from monoflex_amd.structures.params_3d import make_test_target
    imgs = S.synthetic_images(B, 96, 192, seed=5).to(DEV)
    tg = m.device_targets([make_test_target(S.synthetic_target(48, 24)) for _ in range(B)], DEV)
    return imgs, tg


def test_default_detect_device_does_not_take_the_multi_kernel(small_model):
    ops, L = _L()
    lib = L.load()
    before = lib.mfx_get_counter(b"decode_multi")
    assert before >= 0
    imgs, tg = _model_inputs(small_model)
    assert small_model.heads.post_processor.output_depth == "soft"
    with torch.no_grad():
        small_model.detect_device(imgs, *tg)
    torch.cuda.synchronize()
    assert lib.mfx_get_counter(b"decode_multi") - before == 0             # (process-wide counter: other tests of this file launch the kernel)


def test_detect_device_oracle_inside_a_hipgraph(small_model):
    m = small_model
    post = m.heads.post_processor
    imgs, tg = _model_inputs(m)
    try:
        with torch.no_grad():
            post.output_depth = "mean"
            mean = m.detect_device(imgs, *tg)
            post.output_depth = "direct"
            direct = m.detect_device(imgs, *tg)
            torch.cuda.synchronize()
            valid = mean[2].cpu().numpy()
            gt = np.zeros((2, 40, 8), dtype=np.float32)
            for b in range(2):
                rows = {"mean": mean[0][b].cpu().numpy(), "direct": direct[0][b].cpu().numpy()}
                gt[b] = _gt_from_rows(rows, np.ones_like(valid[b]), ["direct"], 40, every=2)
            gt_rows = torch.from_numpy(gt).to(DEV)
            post.output_depth = "oracle"
            with pytest.raises(ValueError):
                m.detect_device(imgs, *tg)
            eager = [t.clone() for t in m.detect_device(imgs, *tg, gt_rows=gt_rows)]
            side = torch.cuda.Stream()
            side.wait_stream(torch.cuda.current_stream())
            with torch.cuda.stream(side):
                m.detect_device(imgs, *tg, gt_rows=gt_rows)
            torch.cuda.current_stream().wait_stream(side)
            torch.cuda.synchronize()
            graph = torch.cuda.CUDAGraph()
            with torch.cuda.graph(graph):
                out = m.detect_device(imgs, *tg, gt_rows=gt_rows)
            graph.replay(); graph.replay()
        torch.cuda.synchronize()
        for a, b in zip(out[:3], eager[:3]):
            assert torch.equal(a, b)
        for sl in (slice(0, 3), slice(8, 58)):                              # (the map's other channels are padding nobody writes)
            assert torch.equal(out[3][..., sl], eager[3][..., sl])
        assert torch.equal(eager[1], mean[1]) and not torch.equal(eager[0], mean[0])          # the table moved rows off the mean
        all_det, _, all_valid, _ = m.detect_all_device(imgs, *tg, methods=["mean", "oracle", "direct"], gt_rows=gt_rows)
        assert torch.equal(all_det[:, 0], mean[0]) and torch.equal(all_det[:, 1], eager[0]) and torch.equal(all_det[:, 2], direct[0])
        assert torch.equal(all_valid[:, 1], eager[2])
    finally:
        post.output_depth = "soft"


# ---- 5: one pass against eight ----------------------------------------------------------------------------------------------------------------
def test_single_pass_equals_eight_passes(tmp_path):
    from PIL import Image
    from monoflex_amd import synthetic as S
    from monoflex_amd.config import get_cfg
    from monoflex_amd.data import DeviceLoader, InferenceSampler, KITTIDataset
    from monoflex_amd.engine.inference import EVAL_DEPTH_METHODS, compute_on_dataset, inference_all_depths
    from monoflex_amd.model.detector import KeypointDetector
    for d in ("image_2", "label_2", "calib", "ImageSets"):
        (tmp_path / d).mkdir()
    Pm = np.asarray(S.KITTI_P2).reshape(-1)
    n = 3
    for i in range(n):
        Image.fromarray(np.random.RandomState(i).randint(0, 256, (375, 1242, 3)).astype(np.uint8)).save(tmp_path / "image_2" / ("%06d.png" % i))
        (tmp_path / "label_2" / ("%06d.txt" % i)).write_text("\n".join(S.synthetic_kitti_labels(70 + i, 1242, 375, 8, z_range=(5, 38), occl_max=1)))
        (tmp_path / "calib" / ("%06d.txt" % i)).write_text("P2: " + " ".join("%.12e" % v for v in Pm) + "\nP3: " + " ".join("%.12e" % v for v in Pm) + "\n")
    (tmp_path / "ImageSets" / "val.txt").write_text("".join("%06d\n" % i for i in range(n)))
    cfg = get_cfg(os.path.join(ROOT, "runs", "monoflex.yaml"), ["MODEL.COMPUTE_DTYPE", "bf16"])
    cfg.MODEL.PRETRAIN = False
    ds = KITTIDataset(cfg, str(tmp_path), is_train=False)
    torch.manual_seed(0)
    model = KeypointDetector(cfg).cuda()
    model.load_state_dict(S.synthetic_state_dict(model.state_dict(), seed=0, cls_bias=-1.0))
    loader = DeviceLoader(ds, batch_size=2, sampler=InferenceSampler(len(ds)))
    names = ["%06d.txt" % i for i in range(n)]

    def folder_bytes(root):
        out = {}
        for m in EVAL_DEPTH_METHODS:
            folder = root / "eval_all_depths" / m
            assert sorted(os.listdir(folder)) == names
            out[m] = [(folder / f).read_bytes() for f in names]
        return out

    one_root, eight_root = tmp_path / "one", tmp_path / "eight"
    stale = one_root / "eval_all_depths" / "hard"
    stale.mkdir(parents=True)
    (stale / "999999.txt").write_text("stale\n")                        # removed, as by the eight passes
    one = inference_all_depths(model, loader, "kitti_val", output_folder=str(one_root))
    assert model.heads.post_processor.output_depth == "soft"
    eight = inference_all_depths(model, loader, "kitti_val", output_folder=str(eight_root), single_pass=False)
    assert tuple(one) == tuple(eight) == EVAL_DEPTH_METHODS
    for m in EVAL_DEPTH_METHODS:
        assert sorted(one[m]) == sorted(eight[m]) and "Car_3d_0.70/moderate" in one[m]
        assert all(one[m][k] == eight[m][k] or (np.isnan(one[m][k]) and np.isnan(eight[m][k])) for k in one[m]), m
    b1, b8 = folder_bytes(one_root), folder_bytes(eight_root)
    assert b1 == b8
    assert len({b"".join(v) for v in b1.values()}) >= 4
    # 'oracle' alone: one batch in flight or not, the same files
    post = model.heads.post_processor
    post.output_depth = "oracle"
    try:
        for sub, overlap in (("ov", True), ("seq", False)):
            (tmp_path / sub).mkdir()
            assert compute_on_dataset(model, loader, "cuda", str(tmp_path / sub), overlap=overlap) == n
        for i, f in enumerate(names):
            assert (tmp_path / "ov" / f).read_bytes() == (tmp_path / "seq" / f).read_bytes() == b1["oracle"][i]
    finally:
        post.output_depth = "soft"


# ---- 6: refusals ------------------------------------------------------------------------------------------------------------------------------
def test_refusals_launch_nothing():
    ops, L = _L()
    lib = L.load()
    hm, reg_off, sc, ix, calib, pad, size, thr = _inputs("b3_k50", "s111", 3, 3)
    B, H, W, ld = hm.shape
    K = sc.shape[2]
    det = torch.full((B, 9, K, 14), float("nan"), device=DEV)
    topk, valid = torch.zeros(B, K, 5, device=DEV), torch.zeros(B, K, dtype=torch.int32, device=DEV)
    gt = torch.zeros(B, 129, 8, device=DEV)
    cfg = _decode_cfg(True)

    def call(modes, gt_rows=None, M=0, name="s111", cfg_=cfg, hm_=hm):
        lay = _layout(name)
        return lib.mfx_decode_boxes_multi(P(hm_), ld, reg_off, P(sc), P(ix), 3, B, H, W, K, P(calib), P(pad), P(size), ctypes.c_float(thr),
                                          ctypes.byref(cfg_) if cfg_ is not None else None, ctypes.byref(lay), modes, P(gt_rows), M, P(det),
                                          P(topk), P(valid), None, None, None)

    before = lib.mfx_get_counter(b"decode_multi")
    s011 = _inputs("b3_k50", "s011", 3, 3)[0]
    s010 = torch.from_numpy(np.ascontiguousarray(HS.take(C.case_inputs("b3_k50")["hmap"][..., CH_OFF:CH_OFF + 50], "s010", 3, ld=LD, off=CH_OFF,
                                                         junk=C.case_inputs("b3_k50")["hmap"]))).to(DEV)
    for what, refused, word in (("oracle bit without gt_rows", lambda: call(1 << 8), "gt_rows"),
                                ("M = 129", lambda: call(1 << 8, gt, 129), "128"),
                                ("M = 0", lambda: call(1 << 8, gt, 0), "128"),
                                ("modes = 0", lambda: call(0), "modes is 0"),
                                ("a bit above 8", lambda: call(1 << 9), "above 8"),
                                ("soft without corner_uncertainty", lambda: call(0b1001, name="s010", hm_=s010), "corner_uncertainty"),
                                ("oracle without corner_uncertainty", lambda: call((1 << 8) | 8, gt, 40, name="s010", hm_=s010), "corner_uncertainty"),
                                ("keypoints_02 without corner_offset", lambda: call(1 << 6, name="s000", hm_=s010), "corner_offset"),
                                ("null cfg", lambda: call(1, cfg_=None), "cfg")):
        assert refused() == -1, what
        assert word in lib.mfx_last_error().decode(), (what, lib.mfx_last_error().decode())
    assert call(0b11111110, name="s011", hm_=s011) == 0                     # (the modes s011 serves, direct included: accepted)
    torch.cuda.synchronize()
    assert lib.mfx_get_counter(b"decode_multi") == before + 1
    det.fill_(float("nan"))
    assert call(1 << 8) == -1
    torch.cuda.synchronize()
    assert bool(torch.isnan(det).all()) and lib.mfx_get_counter(b"decode_multi") == before + 1
    with pytest.raises(RuntimeError, match="gt_rows"):
        ops.decode_boxes_multi(hm, reg_off, sc, ix, calib, pad, size, thr, ["oracle"], cfg)
    with pytest.raises(ValueError):
        ops.decode_boxes_multi(hm, reg_off, sc, ix, calib, pad, size, thr, ["soft", "combine"], cfg)
    with pytest.raises(ValueError):
        ops.decode_boxes_multi(hm, reg_off, sc, ix, calib, pad, size, thr, ["soft", "soft"], cfg)
    with pytest.raises(ValueError, match="reg_mask"):
        ops.oracle_gt_rows([_target((136, 80), (12, 8), C.image_P(0))], DEV)
