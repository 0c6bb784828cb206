"""mfx_object_loss_types (csrc/loss_kernels.hip: the per-object loss kernel with the loss kinds of MODEL.HEAD.LOSS_TYPE entries 1 and 3)
on the device through autograd.ObjectLossFn, in every configuration and on the planted edges of tests/test_loss_types_cpu.py, against
the float64 tensor-op reference of tests/loss_types_cases.py (computed on the CPU inside the test).  Both addressing forms: the dense
map with the 50 channels inside a wider pixel (ld 64, ch_off 8) and the gathered [N][ld] table.  Harness and device bounds are those
of tests/test_gpu_object_loss_configs.py: terms 2e-5*max(1,|ref|), logged means 1e-4*max(1,|ref|), gradients 2e-5*max(1,max|ref|)."""
import os
import sys

import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

import loss_types_cases as LT                                                       # noqa: E402
import test_object_loss_configs_cpu as T                                            # noqa: E402
from test_gpu_object_loss_configs import CH_OFF, LD, NT, _pixel_sums                # noqa: E402
from test_loss_types_cpu import check_edge                                          # noqa: E402

pytestmark = pytest.mark.gpu
DEV = "cuda"


def device_run(cname, R, form, explicit_kinds=True):
    """test_gpu_object_loss_configs.device_run with the evaluator's loss kinds: ObjectLossFn forward + eleven backwards -> terms, logged,
    per-term gradient at the centres (10, R, 50), the weighted gradient (R, 50), the raw vals and the full weighted gradient tensor."""
    from monoflex_amd import autograd as AG
    ev = LT.make_evaluator(cname)
    cfg = LT.check_kernel_cfg(cname, ev)
    rows = R.rows.to(DEV)
    nhwc = R.reg.permute(0, 2, 3, 1)
    B, H, W, _ = nhwc.shape
    gen = torch.Generator().manual_seed(7)
    bi, cx, cy = (torch.tensor(x, device=DEV) for x in zip(*R.pix))
    if form == "dense":
        x = torch.randn(B, H, W, LD, generator=gen)
        x[..., CH_OFF:CH_OFF + 50] = nhwc
    else:
        x = torch.randn(rows.shape[0], LD, generator=gen)
        x[:, CH_OFF:CH_OFF + 50] = nhwc[R.rows[:, 57].long(), R.rows[:, 3].long(), R.rows[:, 2].long()]
    x = x.to(DEV).requires_grad_()
    kinds = ev.object_loss_kinds() if explicit_kinds else ()                          # () = the kinds the configuration object carries
    terms, logged = AG.ObjectLossFn.apply(x, rows, cfg, CH_OFF, *kinds)

    def grad_at_centres(gout):
        g, = torch.autograd.grad(terms, x, grad_outputs=gout.to(DEV), retain_graph=True)
        assert float(g[..., :CH_OFF].abs().max()) == 0.0 and float(g[..., CH_OFF + 50:].abs().max()) == 0.0
        inner = g[..., CH_OFF:CH_OFF + 50]
        if form == "dense":
            at = inner[bi, cy, cx]
            off = inner.clone()
            off[bi, cy, cx] = 0
        else:
            at = _pixel_sums(R, inner)
            off = inner.clone()
            off[R.n] = 0
        assert float(off.abs().max()) == 0.0
        return at.cpu(), g

    grads = torch.stack([grad_at_centres(torch.eye(NT)[i])[0] for i in range(NT)])
    weighted, full = grad_at_centres(torch.linspace(0.5, 1.5, NT))
    return terms.detach().cpu(), logged.detach().cpu(), grads, weighted, torch.cat((terms, logged)).detach().cpu(), full.cpu()


def check_device(cname, iname, form, ename=None):
    R = LT.reference(cname, iname)
    terms, logged, grads, weighted, _, _ = device_run(cname, R, form)
    if ename is not None:
        check_edge(R, cname, ename, grads)
    else:
        T.check_input(R, LT.CONFIGS[cname][0], iname, grads)
    T.compare(R, terms, logged, grads, 2e-5, "%s/%s %s" % (cname, iname, form))
    gout = torch.linspace(0.5, 1.5, NT).double()
    want = (R.grads * gout.view(NT, 1, 1)).sum(0)[~R.drop]
    err = float((weighted[~R.drop].double() - want).abs().max())
    print("weighted backward: error/bound %.3f" % (err / (2e-5 * max(1.0, float(want.abs().max())))))
    assert err <= 2e-5 * max(1.0, float(want.abs().max())), (cname, iname, form, err)


@pytest.mark.parametrize("form", ["dense", "gathered"])
@pytest.mark.parametrize("iname", LT.INPUTS)
@pytest.mark.parametrize("cname", sorted(LT.CONFIGS))
def test_config_kernel_vs_float64(cname, iname, form):
    check_device(cname, iname, form)


@pytest.mark.parametrize("form", ["dense", "gathered"])
@pytest.mark.parametrize("ename", LT.EDGES)
@pytest.mark.parametrize("cname", LT.EDGE_CONFIGS)
def test_edge_kernel_vs_float64(cname, ename, form):
    check_device(cname, ename, form, ename)


def test_kinds_carried_by_the_configuration_equal_explicit_kinds_and_differ_from_l1():
    """ObjectLossFn without explicit kinds takes them from the evaluator's configuration object; (0, 0) is another function."""
    from monoflex_amd import autograd as AG
    from monoflex_amd import lib as L
    R = LT.reference("yaml-smooth_l1-log", "kd_interior")
    L.check(L.load().mfx_set_option(b"deterministic", 1), "opt")        # (the default mode adds the objects' values in any order)
    try:
        a = device_run("yaml-smooth_l1-log", R, "dense")
        b = device_run("yaml-smooth_l1-log", R, "dense", explicit_kinds=False)
    finally:
        L.check(L.load().mfx_set_option(b"deterministic", 0), "opt")
    assert torch.equal(a[0], b[0]) and torch.equal(a[2], b[2])
    ev = LT.make_evaluator("yaml-smooth_l1-log")
    x = R.reg.permute(0, 2, 3, 1).contiguous().to(DEV)
    l1, _ = AG.ObjectLossFn.apply(x, R.rows.to(DEV), ev.object_loss_cfg(), 0, 0, 0)
    i_dep, i_dim = LT.TERM_NAMES.index('depth_loss'), LT.TERM_NAMES.index('dims_loss')
    assert abs(float(l1[i_dep]) - float(a[0][i_dep])) > 1e-2 and abs(float(l1[i_dim]) - float(a[0][i_dim])) > 1e-2
    with pytest.raises(RuntimeError, match="reg_loss"):
        AG.ObjectLossFn.apply(x, R.rows.to(DEV), ev.object_loss_cfg(), 0, 2, 0)


@pytest.mark.parametrize("cname,iname", [("yaml-smooth_l1-log", "kd_interior"), ("defaults-smooth_l1-inv_sig", "b3_mixed")])
@pytest.mark.parametrize("form", ["dense", "gathered"])
def test_deterministic_option_is_bit_identical_and_agrees(cname, iname, form):
    """Option `deterministic` covers the new entry: two runs give the same bits in vals and dreg and agree with the reference."""
    from monoflex_amd import lib as L
    R = LT.reference(cname, iname)
    lib_ = L.load()
    L.check(lib_.mfx_set_option(b"deterministic", 1), "opt")
    try:
        a = device_run(cname, R, form)
        b = device_run(cname, R, form)
    finally:
        L.check(lib_.mfx_set_option(b"deterministic", 0), "opt")
    assert torch.equal(a[4], b[4]) and torch.equal(a[5], b[5]) and torch.equal(a[2], b[2])
    T.compare(R, a[0], a[1], a[2], 2e-5, "%s/%s %s deterministic" % (cname, iname, form))
