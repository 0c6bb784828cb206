"""The one-launch optimizer's other recipes (csrc/adamw.hip mfx_optim_multi / mfx_grad_norm_multi, monoflex_amd/solver.MultiTensorAdam and the clipped
`step(max_norm)`): SOLVER.OPTIMIZER 'adam' (reference solver/__init__.py:33-34: optim.Adam with L2 weight decay) against torch's own fused capturable
Adam, and SOLVER.GRAD_NORM_CLIP (reference engine/trainer.py:119) against torch.nn.utils.clip_grad_norm_ followed by torch's fused step.
Tensor shapes: tests/test_gpu_optim.py `_params` (ragged sizes, more than one chunk, a storage that is not 16-byte aligned).

Bounds.  Parameters and moments: that file's 2e-6 (max |difference| / max |value|).  total_norm against the float64 norm of the same fp32
gradients, 2e-6 relative: each chunk partial is at most 16 serial additions, one squaring and 8 tree levels in fp32 over non-negative terms,
<= 25 * 2^-24 relative on the sum of squares; the square root halves that; the sum of the partials and the root are taken in double.
coef against torch's rule evaluated in fp32 on the kernel's own total_norm: one addition and one division, 2 * 2^-24 relative."""
import copy

import pytest
import torch

from test_gpu_optim import DEV, _params

pytestmark = pytest.mark.gpu


def _lr(v):
    return torch.tensor(v, dtype=torch.float32, device=DEV)


def _opt(ps, kind="adam"):
    groups = [{"params": ps[::2], "lr": _lr(3e-3)}, {"params": ps[1::2], "lr": _lr(6e-3)}]
    cls = torch.optim.Adam if kind == "adam" else torch.optim.AdamW
    return cls(groups, lr=_lr(3e-3), weight_decay=1e-2, betas=(0.9, 0.99), fused=True, capturable=True)


def _counters():
    from monoflex_amd import lib as L
    return {k: L.load().mfx_get_counter(k.encode()) for k in ("adamw_multi", "optim_multi", "grad_norm_multi")}


def _rel(x, y):
    return float((x.detach() - y.detach()).abs().max() / x.detach().abs().max().clamp(min=1e-30))


def test_multi_tensor_adam_follows_torch_fused_adam():
    from monoflex_amd.solver import MultiTensorAdam, MultiTensorAdamW, multi_tensor_driver, optimizer_step
    a, b = _params(1), _params(1)
    oa, ob = _opt(a), _opt(b)
    assert MultiTensorAdam.eligible(ob) and not MultiTensorAdamW.eligible(ob) and not MultiTensorAdam.eligible(_opt(_params(1), "adamw"))
    assert type(multi_tensor_driver(ob)) is MultiTensorAdam
    found = torch.zeros((), dtype=torch.float32, device=DEV)
    oa.found_inf = ob.found_inf = found
    oa.grad_scale = None
    g = torch.Generator().manual_seed(9)
    c0 = _counters()
    for it in range(6):
        skip = it == 3                                                      # a skipped step: nothing may move, counters included
        found.fill_(1.0 if skip else 0.0)
        before = [p.detach().clone() for p in b]
        for pa, pb in zip(a, b):
            gr = torch.randn(pa.shape, generator=g).to(DEV) * (10.0 ** (it - 3))
            pa.grad, pb.grad = gr.clone(), gr.clone()
        if it == 4:
            for o in (oa, ob):
                o.param_groups[1]["lr"].fill_(1e-3)                         # a scheduler writes the device scalar between steps
        oa.step()
        optimizer_step(ob)
        torch.cuda.synchronize()
        for i, (pa, pb) in enumerate(zip(a, b)):
            sa, sb = oa.state[pa], ob.state[pb]
            assert float(sa["step"]) == float(sb["step"]) == (it + 1 - (1 if it >= 3 else 0)), (it, i)
            for x, y, name in ((pa, pb, "param"), (sa["exp_avg"], sb["exp_avg"], "exp_avg"), (sa["exp_avg_sq"], sb["exp_avg_sq"], "exp_avg_sq")):
                assert _rel(x, y) < 2e-6, (it, i, name, _rel(x, y))
            if skip:
                assert torch.equal(pb, before[i])
    c1 = _counters()
    assert c1["optim_multi"] == c0["optim_multi"] + 6 and c1["adamw_multi"] == c0["adamw_multi"] and c1["grad_norm_multi"] == c0["grad_norm_multi"]
    # L2 decay is not decoupled decay: the same gradients through the AdamW rule land elsewhere
    w, ow = _params(1), None
    ow = _opt(w, "adamw")
    for pw, pb in zip(w, b):
        pw.grad = pb.grad.clone()
    optimizer_step(ow)
    assert _counters()["adamw_multi"] == c1["adamw_multi"] + 1
    # the state is torch's own: it loads into a plain torch Adam
    oc = torch.optim.Adam([{"params": (pc := _params(1))[::2]}, {"params": pc[1::2]}], lr=1e-3)
    oc.load_state_dict(copy.deepcopy(ob.state_dict()))
    assert all(torch.equal(oc.state[x]["exp_avg"], ob.state[y]["exp_avg"]) and torch.equal(oc.state[x]["exp_avg_sq"], ob.state[y]["exp_avg_sq"])
               for go, gb in zip(oc.param_groups, ob.param_groups) for x, y in zip(go["params"], gb["params"]))


@pytest.mark.parametrize("clip", [-1.0, 10.0])
def test_multi_tensor_adam_replays_from_a_graph(clip):
    from monoflex_amd.solver import finish_capture, optimizer_step
    a, b = _params(2), _params(2)
    oa, ob = _opt(a), _opt(b)
    g = torch.Generator().manual_seed(3)
    for pa, pb in zip(a, b):
        gr = torch.randn(pa.shape, generator=g).to(DEV)
        pa.grad, pb.grad = gr.clone(), gr.clone()
    optimizer_step(ob, clip)                                                 # eager first step: state and tables exist
    optimizer_step(oa, clip)
    graph = torch.cuda.CUDAGraph()
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        with torch.cuda.graph(graph, capture_error_mode="thread_local"):
            optimizer_step(ob, clip)
    finish_capture(ob)
    for it in range(3):
        for pa, pb in zip(a, b):
            gr = torch.randn(pa.shape, generator=g).to(DEV) * (1e-3 if it == 1 else 1.0)
            pa.grad.copy_(gr)
            pb.grad.copy_(gr)
        optimizer_step(oa, clip)
        graph.replay()
        torch.cuda.synchronize()
        for pa, pb in zip(a, b):
            assert torch.equal(pa, pb) and float(oa.state[pa]["step"]) == float(ob.state[pb]["step"]) == it + 2
            assert torch.equal(oa.state[pa]["exp_avg_sq"], ob.state[pb]["exp_avg_sq"])
        if clip > 0:
            assert torch.equal(oa._mfx_multi.grad_norm, ob._mfx_multi.grad_norm)
            assert (float(ob._mfx_multi.grad_norm[1]) == 1.0) == (it == 1)


def _set_grads(ps, seed, scale):
    g = torch.Generator().manual_seed(seed)
    for p in ps:
        p.grad = (torch.randn(p.shape, generator=g) * scale).to(DEV)


# (gradient scale, max_norm): the norm of the unit-scale gradients is ~ sqrt(180 644 elements) = 425
CLIP_CASES = {"below": (1.0, 1e4), "above": (1.0, 10.0), "scaled_1e-3": (1e-3, 0.1), "scaled_1e3": (1e3, 10.0)}


@pytest.mark.parametrize("kind", ["adam", "adamw"])
@pytest.mark.parametrize("case", sorted(CLIP_CASES))
def test_clipped_step_follows_clip_grad_norm_then_torch_fused_step(case, kind):
    from monoflex_amd.solver import optimizer_step
    scale, max_norm = CLIP_CASES[case]
    a, b, b2, u = _params(5), _params(5), _params(5), _params(5)
    oa, ob, ob2, ou = (_opt(p, kind) for p in (a, b, b2, u))
    for ps in (a, b, b2, u):
        _set_grads(ps, 6, scale)
    grads = [p.grad.clone() for p in b]
    want_norm = float(torch.sqrt(sum((gr.double() ** 2).sum() for gr in grads)))
    c0 = _counters()
    optimizer_step(ob, max_norm)
    optimizer_step(ob2, max_norm)
    optimizer_step(ou)                                                       # the unclipped one-launch step
    tn = torch.nn.utils.clip_grad_norm_(a, max_norm, foreach=True)
    oa.step()
    torch.cuda.synchronize()
    c1 = _counters()
    assert c1["grad_norm_multi"] == c0["grad_norm_multi"] + 2 and c1["optim_multi"] == c0["optim_multi"] + 2 + (kind == "adam")
    assert c1["adamw_multi"] == c0["adamw_multi"] + (kind == "adamw")
    total, coef = (float(x) for x in ob._mfx_multi.grad_norm)
    print("%s %s: total_norm %.9g (float64 %.9g, rel %.2e; torch %.9g) coef %.9g" % (case, kind, total, want_norm, abs(total - want_norm) / want_norm, float(tn), coef))
    assert abs(total - want_norm) <= 2e-6 * want_norm
    t32 = torch.tensor(total, dtype=torch.float32)
    want_coef = float(torch.clamp(max_norm / (t32 + 1e-6), max=1.0))         # torch's rule on the kernel's own norm
    assert abs(coef - want_coef) <= 2 * 2.0 ** -24 * want_coef
    assert (coef == 1.0) == (case in ("below",)), (case, coef)
    for i, (pa, pb, pb2, pu) in enumerate(zip(a, b, b2, u)):
        assert torch.equal(pb.grad, grads[i])                                # p.grad keeps the unclipped values
        assert torch.equal(pb, pb2) and torch.equal(ob.state[pb]["exp_avg"], ob2.state[pb2]["exp_avg"])       # two runs: the same bits
        for x, y, name in ((pa, pb, "param"), (oa.state[pa]["exp_avg"], ob.state[pb]["exp_avg"], "exp_avg"),
                           (oa.state[pa]["exp_avg_sq"], ob.state[pb]["exp_avg_sq"], "exp_avg_sq")):
            assert _rel(x, y) < 2e-6, (case, i, name, _rel(x, y))
        if coef == 1.0:                                                      # bit-equal to the unclipped step
            assert torch.equal(pb, pu) and torch.equal(ob.state[pb]["exp_avg_sq"], ou.state[pu]["exp_avg_sq"])
    assert torch.equal(ob._mfx_multi.grad_norm, ob2._mfx_multi.grad_norm)


def test_clipped_step_under_found_inf_moves_nothing_and_leaves_coef_at_one():
    from monoflex_amd.solver import optimizer_step
    b = _params(7)
    ob = _opt(b)
    ob.found_inf = torch.ones((), dtype=torch.float32, device=DEV)
    _set_grads(b, 8, 1.0)
    b[2].grad[17] = float("inf")
    before = [p.detach().clone() for p in b]
    optimizer_step(ob, 10.0)
    torch.cuda.synchronize()
    assert float(ob._mfx_multi.grad_norm[1]) == 1.0
    assert all(torch.equal(p, q) for p, q in zip(b, before)) and all(float(ob.state[p]["step"]) == 0.0 for p in b)


def test_entries_refuse_bad_arguments():
    from monoflex_amd import lib as L
    lib = L.load()
    x = torch.zeros(64, device=DEV)
    p = lambda t: L.ctypes.c_void_p(t.data_ptr())                            # noqa: E731
    assert lib.mfx_optim_multi(p(x), p(x), 1, 1, p(x), 2, None, None, None) == -1 and b"rule" in lib.mfx_last_error()
    assert lib.mfx_grad_norm_multi(p(x), p(x), 1, 4, 10.0, p(x), 8, p(x), None, None) == -1 and b"workspace" in lib.mfx_last_error()
    assert lib.mfx_grad_norm_multi(p(x), p(x), 1, 4, 0.0, p(x), 64, p(x), None, None) == -1
    assert lib.mfx_grad_norm_workspace_bytes(5) == 20
