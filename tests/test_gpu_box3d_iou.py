"""GPU tests of the rotated 3D box IoU (reference get_iou_3d, model/layers/iou_loss.py:99-136; the logged `3D_IoU` of
model/head/detector_loss.py:333,436): the stand-alone operator mfx_box3d_iou_pairs, value slot 21 of the fused per-object loss, and the
log entry of Loss_Computation / KeypointDetector.

Reference: tests/box3d_iou_ref.py in float64 (pinned to closed forms by tests/test_box3d_iou_cpu.py).  Bound: 1e-4 * max(1, |ref|) on every
pair and every mean; nothing is skipped or filtered."""
import ctypes
import os
import sys

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "tests")):
    if p not in sys.path:
        sys.path.insert(0, p)

import box3d_iou_ref as R                                           # noqa: E402

pytestmark = pytest.mark.gpu
DEV = "cuda"
TOL = 1e-4
SIZES = (0, 1, 63, 64, 65, 400)


def close(have, ref):
    have, ref = np.asarray(have, dtype=np.float64), np.asarray(ref, dtype=np.float64)
    return np.abs(have - ref) <= TOL * np.maximum(1.0, np.abs(ref))


def _dev(a):
    return torch.from_numpy(np.ascontiguousarray(a, dtype=np.float32)).to(DEV)


def pair_set(seed=11):
    """400 pairs: 300 KITTI-like random ones and 100 that differ in one parameter by 1e-3, interleaved so that every prefix holds both."""
    a, b = R.random_pairs(300, seed)
    na, nb = R.near_identical_pairs(100, seed + 1)
    order = np.random.default_rng(seed + 2).permutation(400)
    return np.concatenate((a, na))[order], np.concatenate((b, nb))[order]


@pytest.fixture(scope="module")
def pairs():
    a, b = pair_set()
    ca, cb = R.corner_tables(a), R.corner_tables(b)
    return {0: (a, b, R.iou_pairs(a.astype(np.float64), b.astype(np.float64))),
            1: (ca, cb, R.iou_pairs(ca.astype(np.float64), cb.astype(np.float64)))}


@pytest.mark.parametrize("n", SIZES)
@pytest.mark.parametrize("form", [0, 1])
def test_pairs_entry_vs_float64(pairs, form, n):
    """The C entry on caller-owned buffers: results against the reference, and nothing written past the N-th result."""
    from monoflex_amd import lib as L
    from monoflex_amd.ops import _ptr, _stream
    a, b, ref = pairs[form]
    x, y = _dev(a[:n]), _dev(b[:n])
    out = torch.full((n + 64,), -7.0, device=DEV)
    L.check(L.load().mfx_box3d_iou_pairs(_ptr(x), _ptr(y), n, form, _ptr(out), _stream()), "mfx_box3d_iou_pairs")
    torch.cuda.synchronize()
    have = out.cpu().numpy()
    assert (have[n:] == -7.0).all()
    err = np.abs(have[:n] - ref[:n])
    print("form %d, N %d: max |err| %.3g" % (form, n, err.max() if n else 0.0))
    assert np.isfinite(have[:n]).all() and close(have[:n], ref[:n]).all(), (int(err.argmax()), float(err.max()))


def test_entry_rejects_bad_arguments():
    from monoflex_amd import lib as L
    lib = L.load()
    x = torch.zeros(4, 7, device=DEV)
    out = torch.zeros(4, device=DEV)
    p = lambda t: ctypes.c_void_p(t.data_ptr())
    assert lib.mfx_box3d_iou_pairs(p(x), p(x), 4, 2, p(out), None) == -1 and b"form" in lib.mfx_last_error()
    assert lib.mfx_box3d_iou_pairs(p(x), p(x), -1, 0, p(out), None) == -1
    assert lib.mfx_box3d_iou_pairs(p(x), None, 4, 0, p(out), None) == -1 and b"null" in lib.mfx_last_error()
    assert lib.mfx_box3d_iou_pairs(None, None, 0, 0, None, None) == 0          # N = 0: a successful no-op


def test_op_and_get_iou_3d_on_cuda_tensors(pairs):
    from monoflex_amd import ops
    from model.layers.iou_loss import get_iou_3d
    for form in (0, 1):
        a, b, ref = pairs[form]
        out = ops.box3d_iou(_dev(a), _dev(b))
        assert out.shape == (400,) and out.dtype == torch.float32 and out.is_cuda
        assert close(out.cpu().numpy(), ref).all()
    ca, cb, ref = pairs[1]
    out = get_iou_3d(_dev(ca), _dev(cb))
    assert out.is_cuda and close(out.cpu().numpy(), ref).all()
    assert close(get_iou_3d(_dev(cb), _dev(ca)).cpu().numpy(), ref).all()          # symmetric
    assert ops.box3d_iou(torch.zeros(0, 7, device=DEV), torch.zeros(0, 7, device=DEV)).shape == (0,)
    with pytest.raises(RuntimeError):
        ops.box3d_iou(torch.zeros(3, 6, device=DEV), torch.zeros(3, 6, device=DEV))


def test_pairs_entry_replays_from_a_captured_graph(pairs):
    """One kernel node: replayed after the input buffers were overwritten, the output follows the new inputs."""
    from monoflex_amd import ops
    a, b, ref = pairs[1]
    x, y = _dev(a[:200]), _dev(b[:200])
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        eager = ops.box3d_iou(x, y).clone()
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        held = ops.box3d_iou(x, y)
    graph.replay()
    torch.cuda.synchronize()
    assert torch.equal(held, eager) and close(held.cpu().numpy(), ref[:200]).all()
    x.copy_(_dev(a[200:400])); y.copy_(_dev(b[200:400]))
    graph.replay()
    torch.cuda.synchronize()
    assert close(held.cpu().numpy(), ref[200:400]).all()
    assert not close(held.cpu().numpy(), ref[:200]).all()            # the two halves are different problems


# ---- value slot 21 of the fused per-object loss -----------------------------------------------------------------------------------------
def _fused_logged(ev, reg, tv):
    from monoflex_amd import autograd as AG
    nhwc = reg.to(DEV).permute(0, 2, 3, 1).contiguous().requires_grad_()
    terms, logged = AG.ObjectLossFn.apply(nhwc, tv["object_rows"].to(DEV), ev.object_loss_cfg(), 0)
    terms.sum().backward()
    torch.cuda.synchronize()
    return terms.detach().cpu(), logged.detach().cpu(), nhwc.grad.detach().cpu()


@pytest.mark.parametrize("name", ["b2", "b3_empty_middle_mixed_calib", "b1_many"])
def test_fused_object_loss_slot_on_golden_cases(name):
    from test_loss_golden import case_inputs, evaluator
    from monoflex_amd.structures.params_3d import make_train_target
    tg, cls, reg = case_inputs(name)
    ev = evaluator()
    _, tv = ev.prepare_targets([make_train_target(t) for t in tg])
    ref = R.mean_iou_of_case(ev, reg, tv)
    terms, logged, grad = _fused_logged(ev, reg, tv)
    print("%s: logged[11] %.6g, float64 mean IoU %.6g" % (name, float(logged[11]), ref))
    assert close(float(logged[11]), ref) and float(logged[12:].abs().max()) == 0.0


@pytest.mark.parametrize("name", ["b2", "b3_empty_middle_mixed_calib", "b1_many"])
def test_fused_object_loss_slot_on_overlapping_boxes(name):
    """Targets moved onto the decoded predictions (the golden cases' boxes miss their targets): the kernel's slot, the fused and the
    tensor-op form of Loss_Computation all against the float64 mean; and the slot is values only -- terms and gradient are those of the
    tensor-op form."""
    from test_loss_golden import evaluator, TERM_NAMES
    ev = evaluator()
    cls, reg, heat, tv = R.overlapping_loss_case(ev, name)
    ref = R.mean_iou_of_case(ev, reg, tv)
    assert ref > 0.2
    terms, logged, grad = _fused_logged(ev, reg, tv)
    print("%s: logged[11] %.6g, float64 mean IoU %.6g" % (name, float(logged[11]), ref))
    assert close(float(logged[11]), ref)
    tvd = {k: (v.to(DEV) if torch.is_tensor(v) else v) for k, v in tv.items()}
    assert ev.fused_object_loss
    _, logs_f = ev({"cls": cls.to(DEV), "reg": reg.to(DEV)}, (heat.to(DEV), tvd))
    ev.fused_object_loss = False
    reg_d = reg.to(DEV).requires_grad_()
    loss_dict, logs_t = ev({"cls": cls.to(DEV), "reg": reg_d}, (heat.to(DEV), tvd))
    assert list(logs_f) == list(logs_t) and list(logs_f)[:2] == ["2D_IoU", "3D_IoU"]
    print("%s: 3D_IoU fused %.6g, tensor-op %.6g" % (name, logs_f["3D_IoU"], logs_t["3D_IoU"]))
    assert logs_f["3D_IoU"] > 0.2 and close(logs_f["3D_IoU"], ref) and close(logs_t["3D_IoU"], ref)
    assert close(logs_f["3D_IoU"], logs_t["3D_IoU"])
    sum(loss_dict[k] for k in TERM_NAMES).backward()
    for i, k in enumerate(TERM_NAMES):
        assert abs(float(terms[i]) - float(loss_dict[k])) <= 2e-5 * max(1.0, abs(float(loss_dict[k]))), k
    want = reg_d.grad.permute(0, 2, 3, 1).cpu()
    assert float((grad - want).abs().max()) <= 2e-5 * max(1.0, float(want.abs().max()))


def test_fused_object_loss_slot_without_objects():
    from test_loss_golden import evaluator
    from monoflex_amd import synthetic as S
    from monoflex_amd.structures.params_3d import make_train_target
    ev = evaluator()
    reg = torch.randn(1, 50, 96, 320, generator=torch.Generator().manual_seed(1))
    _, tv = ev.prepare_targets([make_train_target(S.synthetic_train_target(9, n_obj=0))])
    terms, logged, grad = _fused_logged(ev, reg, tv)
    assert float(logged[11]) == 0.0 and float(logged.abs().max()) == 0.0


def test_fused_loss_with_the_slot_replays_from_a_captured_graph():
    """The slot comes out of the launch that was already there: the captured fused loss replays with a new regression map."""
    from test_loss_golden import evaluator
    from monoflex_amd import autograd as AG
    ev = evaluator()
    cls, reg, heat, tv = R.overlapping_loss_case(ev, "b1_many")
    ref = R.mean_iou_of_case(ev, reg, tv)
    rows, cfg = tv["object_rows"].to(DEV), ev.object_loss_cfg()
    x = reg.to(DEV).permute(0, 2, 3, 1).contiguous()
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side), torch.no_grad():
        AG.ObjectLossFn.apply(x, rows, cfg, 0)
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph), torch.no_grad():
        terms, logged = AG.ObjectLossFn.apply(x, rows, cfg, 0)
    graph.replay()
    torch.cuda.synchronize()
    assert close(float(logged[11]), ref)
    x.copy_(torch.randn(x.shape, generator=torch.Generator().manual_seed(5)).to(DEV) * 0.6)      # random map: the boxes miss again
    graph.replay()
    torch.cuda.synchronize()
    reg2 = x.permute(0, 3, 1, 2).cpu()
    assert close(float(logged[11]), R.mean_iou_of_case(ev, reg2, tv))


def test_detector_in_training_mode_logs_the_3d_iou():
    """KeypointDetector.forward in training mode: `3D_IoU` is in log_loss_dict at the reference's position, a float in [0, 1], and the
    fused and the tensor-op loss forms log the same value for the same step."""
    from monoflex_amd import synthetic as S
    from monoflex_amd.config import get_cfg
    from monoflex_amd.model.detector import KeypointDetector
    from monoflex_amd.structures.params_3d import make_train_target
    out_w, out_h = 96, 32
    cfg = get_cfg(os.path.join(ROOT, "runs", "monoflex.yaml"))
    cfg.MODEL.PRETRAIN = False
    cfg.MODEL.COMPUTE_DTYPE = "fp32"
    cfg.INPUT.WIDTH_TRAIN, cfg.INPUT.HEIGHT_TRAIN = out_w * 4, out_h * 4
    m = KeypointDetector(cfg)
    m.load_state_dict(S.synthetic_state_dict(m.state_dict(), seed=3, cls_bias=-1.0))
    m = m.to(DEV).train()
    tg = [S.synthetic_train_target(20 + i, out_w=out_w, out_h=out_h, n_obj=3 + i) for i in range(2)]
    imgs = S.synthetic_images(2, out_h * 4, out_w * 4, seed=20).to(DEV)
    targets = [make_train_target(t).to(DEV) for t in tg]
    loss_dict, logs = m(imgs, targets)
    assert list(logs)[:2] == ["2D_IoU", "3D_IoU"] and isinstance(logs["3D_IoU"], float)
    assert 0.0 <= logs["3D_IoU"] <= 1.0 + TOL
    m.heads.loss_evaluator.fused_object_loss = False
    _, logs_t = m(imgs, targets)
    print("detector 3D_IoU: fused %.6g, tensor-op %.6g" % (logs["3D_IoU"], logs_t["3D_IoU"]))
    assert close(logs["3D_IoU"], logs_t["3D_IoU"])
