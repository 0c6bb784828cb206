"""mfx_object_loss / mfx_object_loss_backward (csrc/loss_kernels.hip) on the device, in every configuration and on every edge
input of tests/test_object_loss_configs_cpu.py, against that module's float64 tensor-op reference (computed on the CPU inside
the test: no shim, no compiler here) -- the `kd_interior` input, whose keypoint depths lie inside DEPTH_RANGE, included.  Both addressing forms: the dense map with the 50 channels inside a wider pixel (ld 64,
ch_off 8) and the gathered [N][ld] table (B = 0).  Each term's own gradient row comes from a backward with a one-hot incoming
gradient; a backward with torch.linspace(0.5, 1.5, 10) must give their weighted sum.

Bounds: terms 2e-5*max(1,|ref|), logged means 1e-4*max(1,|ref|), gradients 2e-5*max(1,max|ref|) (tests/test_gpu_train.py: the
device's expf/logf differ from the host's).  No configuration needed a wider one (the CPU module's docstring has the figures).
"""
import os
import sys

import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

from test_object_loss_configs_cpu import (CONFIGS, INPUTS, TERM_NAMES, check_edge, check_input, check_kernel_cfg, compare,  # noqa: E402
                                          edge_cases, make_evaluator, reference)

pytestmark = pytest.mark.gpu
DEV = "cuda"
LD, CH_OFF = 64, 8
NT = len(TERM_NAMES)


def _pixel_sums(R, per_row):
    """(.., N, 50) per table row -> (.., R, 50): rows that share a centre pixel summed, as the map's gradient shows them."""
    out = []
    for p in range(len(R.n)):
        same = [R.n[q] for q in range(len(R.n)) if R.pix[q] == R.pix[p]]
        out.append(per_row[..., same, :].sum(dim=-2))
    return torch.stack(out, dim=-2)


def device_run(cname, R, form):
    """ObjectLossFn forward + eleven backwards (one-hot per term, then the linspace weights) -> terms, logged, per-term gradient at
    the centres (10, R, 50), the weighted gradient (R, 50), the raw vals and the full weighted gradient tensor."""
    from monoflex_amd import autograd as AG
    ev = make_evaluator(cname)
    cfg = check_kernel_cfg(cname, ev)
    rows = R.rows.to(DEV)
    nhwc = R.reg.permute(0, 2, 3, 1)
    B, H, W, _ = nhwc.shape
    gen = torch.Generator().manual_seed(7)
    bi, cx, cy = (torch.tensor(x, device=DEV) for x in zip(*R.pix))
    if form == "dense":
        x = torch.randn(B, H, W, LD, generator=gen)
        x[..., CH_OFF:CH_OFF + 50] = nhwc
    else:                                                    # the [N][ld] table: the map indexed at the rows' pixels
        x = torch.randn(rows.shape[0], LD, generator=gen)
        x[:, CH_OFF:CH_OFF + 50] = nhwc[R.rows[:, 57].long(), R.rows[:, 3].long(), R.rows[:, 2].long()]
    x = x.to(DEV).requires_grad_()
    terms, logged = AG.ObjectLossFn.apply(x, rows, cfg, CH_OFF)

    def grad_at_centres(gout):
        g, = torch.autograd.grad(terms, x, grad_outputs=gout.to(DEV), retain_graph=True)
        assert float(g[..., :CH_OFF].abs().max()) == 0.0 and float(g[..., CH_OFF + 50:].abs().max()) == 0.0     # the 14 foreign channels
        inner = g[..., CH_OFF:CH_OFF + 50]                                      # (checked on the device: only the centres travel)
        if form == "dense":
            at = inner[bi, cy, cx]
            off = inner.clone()
            off[bi, cy, cx] = 0
        else:
            at = _pixel_sums(R, inner)
            off = inner.clone()
            off[R.n] = 0
        assert float(off.abs().max()) == 0.0                                 # nothing outside the valid rows' pixels
        return at.cpu(), g

    grads = torch.stack([grad_at_centres(torch.eye(NT)[i])[0] for i in range(NT)])
    gout = torch.linspace(0.5, 1.5, NT)
    weighted, full = grad_at_centres(gout)
    return terms.detach().cpu(), logged.detach().cpu(), grads, weighted, torch.cat((terms, logged)).detach().cpu(), full.cpu()


def check_device(cname, iname, form, ename=None):
    R = reference(cname, iname)
    terms, logged, grads, weighted, _, _ = device_run(cname, R, form)
    if ename is not None:
        check_edge(R, cname, ename, grads)
    else:
        check_input(R, cname, iname, grads)
    compare(R, terms, logged, grads, 2e-5, "%s/%s %s" % (cname, iname, form))
    gout = torch.linspace(0.5, 1.5, NT).double()
    want = (R.grads * gout.view(NT, 1, 1)).sum(0)[~R.drop]
    err = float((weighted[~R.drop].double() - want).abs().max())
    print("weighted backward: error/bound %.3f" % (err / (2e-5 * max(1.0, float(want.abs().max())))))
    assert err <= 2e-5 * max(1.0, float(want.abs().max())), (cname, iname, form, err)


@pytest.mark.parametrize("form", ["dense", "gathered"])
@pytest.mark.parametrize("iname", INPUTS)
@pytest.mark.parametrize("cname", sorted(CONFIGS))
def test_config_kernel_vs_float64(cname, iname, form):
    check_device(cname, iname, form)


@pytest.mark.parametrize("form", ["dense", "gathered"])
@pytest.mark.parametrize("cname,ename", edge_cases())
def test_edge_kernel_vs_float64(cname, ename, form):
    check_device(cname, ename, form, ename)


def test_shared_centre_rows_show_the_summed_gradient():
    """Two and three object rows on one pixel: the dense map's gradient at that pixel is the sum of the rows' own gradients (the
    gathered form gives them one by one), and both equal the float64 reference's gradient there."""
    R = reference("yaml", "shared_centre")
    _, _, dense, _, _, _ = device_run("yaml", R, "dense")
    _, _, gathered, _, _, _ = device_run("yaml", R, "gathered")
    for group in R.plan["shared"]:
        pos = [R.plan["objects"].index(o) for o in group]
        for i in range(NT):
            want = R.grads[i, pos[0]]
            tol = 2e-5 * max(1.0, float(R.grads[i].abs().max()))
            assert float((dense[i, pos[0]].double() - want).abs().max()) <= tol and float((gathered[i, pos[0]].double() - want).abs().max()) <= tol
            for p in pos[1:]:
                assert torch.equal(dense[i, p], dense[i, pos[0]])
    assert float(R.grads[:, [R.plan["objects"].index(g[0]) for g in R.plan["shared"]]].abs().max()) > 0


@pytest.mark.parametrize("cname,iname", [("yaml", "shared_centre"), ("defaults", "b3_mixed"), ("yaml-corner_depth_mode=hard_combine", "unc_clamp")])
@pytest.mark.parametrize("form", ["dense", "gathered"])
def test_deterministic_option_is_bit_identical_and_agrees(cname, iname, form):
    """Option `deterministic` (one wave walks the rows in order): two runs give the same bits in vals and dreg, agree with the
    reference, and agree with the default mode within the terms / gradient bounds."""
    from monoflex_amd import lib as L
    R = reference(cname, iname)
    base = device_run(cname, R, form)
    lib_ = L.load()
    L.check(lib_.mfx_set_option(b"deterministic", 1), "opt")
    try:
        a = device_run(cname, R, form)
        b = device_run(cname, R, form)
    finally:
        L.check(lib_.mfx_set_option(b"deterministic", 0), "opt")
    assert torch.equal(a[4], b[4]) and torch.equal(a[5], b[5]) and torch.equal(a[2], b[2])
    compare(R, a[0], a[1], a[2], 2e-5, "%s/%s %s deterministic" % (cname, iname, form))
    for i in range(NT):
        assert abs(float(a[0][i]) - float(base[0][i])) <= 2e-5 * max(1.0, abs(R.terms[TERM_NAMES[i]])), TERM_NAMES[i]
        assert float((a[2][i] - base[2][i]).abs().max()) <= 2e-5 * max(1.0, float(R.grads[i].abs().max())), TERM_NAMES[i]
    assert float((a[5] - base[5]).abs().max()) <= 2e-5 * max(1.0, float((R.grads * torch.linspace(0.5, 1.5, NT).view(NT, 1, 1)).sum(0).abs().max()))
