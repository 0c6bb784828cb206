"""Validation diagnostics on the device (mfx_eval_diagnostics; TEST.EVAL_DEPTH / TEST.EVAL_DIS_IOUS): the kernel on every case of
tests/eval_diag_cases.py against the float64 restatement and the reference's recording, its agreement with the box decode and the IoU
operator it restates, hipGraph capture, and the evaluation loop end to end.

Bounds as in tests/test_eval_diag_cpu.py: BOUND_FACTOR x the reference's own float32 error (eval_diag_ref.YARDSTICK_*); the IoU columns against
the float64 IoU of the device's own boxes at the IoU operator's 1e-4 * max(1, |ref|)."""
import ctypes
import functools
import os

import numpy as np
import pytest
import torch

from monoflex_amd import lib as L
from monoflex_amd import ops
from monoflex_amd import synthetic as S
from tests import decode_cases as C
from tests import decode_ref as D
from tests import eval_diag_cases as E
from tests import eval_diag_ref as R

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
POISON = 7.75e8


@functools.lru_cache(maxsize=None)
def inputs(name):
    """One case's numpy inputs and their device copies (built once, shared, never written)."""
    d = E.golden_inputs() if name == "golden" else E.case_inputs(name)
    dev = {k: torch.from_numpy(np.ascontiguousarray(d[k])).cuda() for k in ("hmap", "gt_rows", "calib", "pad")}
    return d, dev


def run(d, dev, mode, want=3, gt_rows=None):
    de, iou, bx = ops.eval_diagnostics(dev["hmap"], d["reg_off"], dev["gt_rows"] if gt_rows is None else gt_rows, dev["calib"], dev["pad"],
                                       E.yaml_cfg(mode), E.full_layout(), want=want, return_boxes=True)
    return de.cpu().numpy(), iou.cpu().numpy(), bx.cpu().numpy()


@pytest.mark.parametrize("name", list(E.CASES))
def test_kernel_against_restatement(name):
    d, dev = inputs(name)
    for mode in D.MODES:
        de, iou, bx = run(d, dev, mode)
        ref = E.run_ref(d, mode, with_iou=False)
        print("%s %-16s depth %s\n    boxes %s" % (name, mode, R.format_depth(R.depth_errors_err(de, ref, mode)), R.format_box(R.boxes_err(bx, ref, mode))))
        E.check_against(de, iou, bx, ref, mode, "%s %s" % (name, mode))


def test_kernel_against_golden():
    d, dev = inputs("golden")
    for mode in ("soft", "direct"):
        _, gde, gbx = E.golden_tables(mode)
        de, iou, bx = run(d, dev, mode)
        ref = dict(E.run_ref(d, mode, with_iou=False), depth_err=gde)
        if gbx is not None:
            ref["boxes"] = gbx
        E.check_against(de, iou if gbx is not None else None, bx if gbx is not None else None, ref, mode, "golden " + mode)


def test_every_element_written_and_want_bits():
    """Outputs pre-filled with a poison value: every element is overwritten, empty slots with zeros; an output that is not wanted is left
    alone; empty slots' rows are not read (NaN there changes nothing)."""
    d, dev = inputs("b4_m70")
    lib = L.load()
    B, H, W, ld = dev["hmap"].shape
    M = dev["gt_rows"].shape[1]
    cfg, heads = E.yaml_cfg("soft"), E.full_layout()
    gt = dev["gt_rows"].clone()
    empty = gt[..., 0] == 0
    gt[..., 1:][empty] = float("nan")
    gt[..., 13:] = float("nan")
    out = {}
    for want in (3, 1, 2):
        de, iou, bx = (torch.full(s, POISON, device="cuda") for s in ((B, M, 13), (B, M, 5), (B, M, 6, 7)))
        L.check(lib.mfx_eval_diagnostics(ops._ptr(dev["hmap"]), ld, d["reg_off"], ops._ptr(gt), B, M, H, W, ops._ptr(dev["calib"]), ops._ptr(dev["pad"]),
                                         ctypes.byref(cfg), ctypes.byref(heads), want, ops._ptr(de), ops._ptr(iou), ops._ptr(bx) if want & 2 else None, ops._stream()), "eval_diagnostics")
        out[want] = (de.cpu(), iou.cpu(), bx.cpu())
    de, iou, bx = out[3]
    e = empty.cpu()
    for t in (de, iou, bx):
        assert torch.isfinite(t).all() and (t.abs() < 1e8).all() and (t[e] == 0).all()
    ref = run(d, dev, "soft")
    assert np.array_equal(de.numpy(), ref[0]) and np.array_equal(iou.numpy(), ref[1]) and np.array_equal(bx.numpy(), ref[2])
    assert torch.equal(out[1][0], de) and (out[1][1] == POISON).all() and (out[1][2] == POISON).all()
    assert torch.equal(out[2][1], iou) and torch.equal(out[2][2], bx) and (out[2][0] == POISON).all()
    # argument errors come back through mfx_fail
    with pytest.raises(RuntimeError, match="want must be"):
        ops.eval_diagnostics(dev["hmap"], d["reg_off"], dev["gt_rows"], dev["calib"], dev["pad"], cfg, heads, want=0)
    with pytest.raises(RuntimeError, match="inside a row"):
        ops.eval_diagnostics(dev["hmap"], 20, dev["gt_rows"], dev["calib"], dev["pad"], cfg, heads, want=3)


ULP = 2.0 ** -23                                  # float32 spacing relative to a value in [1, 2)
SOFT_ULPS = 8                                     # see test_pred_box_is_the_decode_kernels_row


@pytest.mark.parametrize("name", ["b4_m70", "b3_m70_ld50", "b4_m40_ld72"])
def test_pred_box_is_the_decode_kernels_row(name):
    """Box 0 EQUALS the row ops.decode_boxes gives for the same pixel listed under the object's class: X, Z, l, h, w and ry bit for bit in the
    seven modes that pick or average estimates, and the dimensions in every mode.  Under `soft` the two kernels run the same function
    (csrc/box_decode_math.h bdec::combine: ((d0 w0 + d1 w1) + d2 w2) + d3 w3 with w_i = (1 / u_i) / sum), but the compiler contracts its
    multiply-adds differently in the two contexts (decode_boxes_kernel also forms sigma from the same weights): the depth then differs in its
    last bits in ~9 % of the rows (measured: 419 of 455, 510 of 560, 788 of 865 values identical; worst 2.00 ulps).  A fused against an unfused product-sum of four terms differs by at
    most 4 roundings of the depth, and X, Y and ry inherit that relative difference through one product and one sum each: SOFT_ULPS = 8
    float32 ulps of max(1, |value|) bounds it; the worst figure seen is printed.  A restated formula that sums in another order or drops a
    term is off by far more than ulps on these inputs (the four estimates of a row differ by metres).
    Y: the decode stores fl(Y + h / 2), box 0 stores Y; half an ulp of |Y| + |h| / 2 apart at most, asserted at 2 ulps."""
    d, dev = inputs(name)
    scores, index = E.census_lists(d)
    size = torch.tensor([160, 96], dtype=torch.int32, device="cuda")
    v = d["gt_rows"][..., 0] != 0
    for mode in D.MODES:
        _, _, bx = run(d, dev, mode)
        det, _, _ = ops.decode_boxes(dev["hmap"], d["reg_off"], torch.from_numpy(scores).cuda(), torch.from_numpy(index).cuda(), dev["calib"], dev["pad"],
                                     size, C.THRESHOLD, depth_mode=mode, cfg=E.yaml_cfg(mode))
        det = det.cpu().numpy()
        assert (det[..., 0][v] == d["gt_rows"][..., 1][v]).all()                                          # row j is slot j under its class
        worst = 0.0
        for mine, theirs in ((3, 8), (4, 6), (5, 7), (0, 9), (2, 11), (6, 12)):
            got, want = bx[..., 0, mine][v].astype(np.float64), det[..., theirs][v].astype(np.float64)
            if mode != "soft" or theirs in (6, 7, 8):
                assert np.array_equal(got, want), (mode, D.COLUMNS[theirs], int((got != want).sum()), np.abs(got - want).max())
            else:
                diff = np.abs(got - want)
                if theirs == 12:
                    diff = np.minimum(diff, np.abs(diff - 2 * np.pi))                                    # a wrap decided either way is the same angle
                ulps = diff / (ULP * np.maximum(1.0, np.abs(want)))
                worst = max(worst, float(ulps.max()))
                assert (ulps <= SOFT_ULPS).all(), (mode, D.COLUMNS[theirs], float(ulps.max()))
        y = det[..., 10][v].astype(np.float64) - det[..., 6][v].astype(np.float64) / 2
        scale = np.maximum(1.0, np.abs(det[..., 10][v]) + np.abs(det[..., 6][v]))
        yulps = np.abs(bx[..., 0, 1][v] - y) / (ULP * scale)
        assert (yulps <= (2 if mode != "soft" else 2 + SOFT_ULPS)).all(), (mode, float(yulps.max()))
        print("%s %s: bit-identical%s; Y within %.2f ulp" % (name, mode, "" if mode != "soft" else " dims, X / Z / ry within %.2f ulp" % worst, yulps.max()))


IOU_ULPS = 8                                      # see test_pred_iou_is_the_iou_operator


def test_pred_iou_is_the_iou_operator():
    """Every IoU column EQUALS ops.box3d_iou of the kernel's own box rows, up to how the compiler contracts the multiply-adds of the one
    function (biou::iou_rows) in two kernels: 86-100 % of the values are bit-identical and the worst difference measured is 2.4e-07, two
    float32 ulps of an IoU near 1.  Asserted at IOU_ULPS = 8 ulps of 1 (9.5e-07), a hundred times below the operator's own 1e-4 bound to
    float64 -- a second copy of the clip that drifts from the operator's is seen here long before it is seen there."""
    d, dev = inputs("b4_m70_direct")
    for mode in ("direct", "soft"):
        _, iou, bx = run(d, dev, mode)
        t = torch.from_numpy(bx).cuda()
        for k, which in enumerate(R.IOU_OF_BOX):
            got = ops.box3d_iou(t[:, :, which].reshape(-1, 7).contiguous(), t[:, :, 1].reshape(-1, 7).contiguous()).cpu().numpy().astype(np.float64)
            diff = np.abs(got - iou[..., k].reshape(-1))
            print("%s %s: worst difference to ops.box3d_iou %.2e, %d of %d bit-identical" % (mode, R.IOU_KEYS[k], diff.max(), int((diff == 0).sum()), diff.size))
            assert (diff <= IOU_ULPS * ULP).all(), (mode, R.IOU_KEYS[k], diff.max())


def test_graph_capture_replays_the_tables():
    d, dev = inputs("b3_m40")
    cfg, heads = E.yaml_cfg("soft"), E.full_layout()
    eager = ops.eval_diagnostics(dev["hmap"], d["reg_off"], dev["gt_rows"], dev["calib"], dev["pad"], cfg, heads, want=3, return_boxes=True)
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        out = ops.eval_diagnostics(dev["hmap"], d["reg_off"], dev["gt_rows"], dev["calib"], dev["pad"], cfg, heads, want=3, return_boxes=True)
    for t in out:
        t.fill_(POISON)
    g.replay()
    torch.cuda.synchronize()
    for a, b in zip(eager, out):
        assert torch.equal(a, b)


def test_inference_loop_with_diagnostics(tmp_path):
    """Generated three-image validation directory, both flags on: five finite IoU means as inference()'s third value, result files
    byte-identical to a flags-off run, and the overlapped and the sequential loop report identical diagnostics."""
    from PIL import Image
    from monoflex_amd.config import get_cfg
    from monoflex_amd.data import DeviceLoader, InferenceSampler, KITTIDataset
    from monoflex_amd.engine.inference import compute_on_dataset, inference
    from monoflex_amd.model.detector import KeypointDetector
    for sub in ("image_2", "label_2", "calib", "ImageSets"):
        (tmp_path / sub).mkdir()
    P = np.asarray(S.KITTI_P2).reshape(-1)
    n = 3
    for i in range(n):
        Image.fromarray(np.random.RandomState(i).randint(0, 256, (375, 1242, 3)).astype(np.uint8)).save(tmp_path / "image_2" / ("%06d.png" % i))
        (tmp_path / "label_2" / ("%06d.txt" % i)).write_text("\n".join(S.synthetic_kitti_labels(70 + i, 1242, 375, 8, z_range=(5, 38), occl_max=1)))
        (tmp_path / "calib" / ("%06d.txt" % i)).write_text("P2: " + " ".join("%.12e" % v for v in P) + "\nP3: " + " ".join("%.12e" % v for v in P) + "\n")
    (tmp_path / "ImageSets" / "val.txt").write_text("".join("%06d\n" % i for i in range(n)))
    yaml = os.path.join(ROOT, "runs", "monoflex.yaml")
    cfg_on = get_cfg(yaml, ["MODEL.COMPUTE_DTYPE", "bf16", "TEST.EVAL_DEPTH", True, "TEST.EVAL_DIS_IOUS", True])
    cfg_off = get_cfg(yaml, ["MODEL.COMPUTE_DTYPE", "bf16"])
    models = {}
    for key, cfg in (("on", cfg_on), ("off", cfg_off)):
        cfg.MODEL.PRETRAIN = False
        torch.manual_seed(0)
        models[key] = KeypointDetector(cfg).cuda()
        models[key].load_state_dict(S.synthetic_state_dict(models[key].state_dict(), seed=0, cls_bias=-1.0))
    ds = KITTIDataset(cfg_on, str(tmp_path), is_train=False)
    loader = DeviceLoader(ds, batch_size=2, sampler=InferenceSampler(len(ds)))
    assert models["on"].heads.post_processor.diagnostics_wanted == 3 and models["off"].heads.post_processor.diagnostics_wanted == 0
    _, _, ious = inference(models["on"], loader, "kitti_val", output_folder=str(tmp_path / "on"))
    _, _, none = inference(models["off"], loader, "kitti_val", output_folder=str(tmp_path / "off"))
    assert none == {} and tuple(ious) == R.IOU_KEYS and all(np.isfinite(v) and 0.0 <= v <= 1.0 for v in ious.values()), ious
    files = sorted(os.listdir(tmp_path / "on" / "data"))
    assert files == ["%06d.txt" % i for i in range(n)]
    for f in files:
        assert (tmp_path / "on" / "data" / f).read_bytes() == (tmp_path / "off" / "data" / f).read_bytes(), f
    diag = {}
    for overlap in (True, False):
        folder = tmp_path / ("loop%d" % overlap)
        folder.mkdir()
        diag[overlap] = {}
        assert compute_on_dataset(models["on"], loader, "cuda", str(folder), overlap=overlap, diagnostics=diag[overlap]) == n
        for f in files:
            assert (folder / f).read_bytes() == (tmp_path / "off" / "data" / f).read_bytes(), f
    assert diag[True] == diag[False] and diag[True]["dis_ious"] == ious
    assert diag[True]["objects"] > 0 and tuple(diag[True]["depth_errors"]) == R.DEPTH_KEYS
    assert all(np.isfinite(v) for v in diag[True]["depth_errors"].values())
    # the forward path's per-object dicts: one value per labelled object of the batch
    batch = next(iter(loader))
    _, utils, _ = models["on"](batch["images"].to("cuda"), [t.to("cuda") for t in batch["targets"]])
    count = sum(int(torch.count_nonzero(t.get_field("reg_mask"))) for t in batch["targets"])
    assert tuple(utils["depth_errors"]) == R.DEPTH_KEYS and all(v.shape == (count,) for v in utils["depth_errors"].values())
    assert tuple(utils["dis_ious"]) == R.IOU_KEYS and all(v.shape == (count,) for v in utils["dis_ious"].values())
    _, utils, _ = models["off"](batch["images"].to("cuda"), [t.to("cuda") for t in batch["targets"]])
    assert utils["depth_errors"] is None and utils["dis_ious"] is None
