"""The heads' fused training nodes on the device against float64: autograd.FanOutConvFn, HeadConvGatherFn and EdgeScatterAddFn, each run once per
training step (detector_predictor.forward_train) and until now seen on the GPU only through whole-step comparisons at 16-bit tolerances.

References, case builders and the error model: tests/head_nodes_ref.py (checked without a GPU by tests/test_head_nodes_ref_cpu.py, teeth
included).  Every bound is derived -- exact 16-bit products, n 2^-24 sum|terms| per fp32 accumulation of n terms, one u_out |value| per store,
times 1 + 2^-6 -- and none carries a measured constant.  Maps are small, channel counts are the production ones (64 -> 256 3x3 trunks, 256-channel
head inputs): the kernel instantiations depend on them.

  FanOutConvFn      y_i, dx (the chain of data-gradient convs through the `res` epilogue: one rounding per link) and dW_i against float64, and
                    against n separate Conv2dFn nodes (same packs and kernels: y and dW bitwise under set_deterministic, within the two fp32-sum
                    bounds where dW goes through atomics; dx within the sum of both formulations' bounds).  Variants: an unused output (its dy is
                    None: no launches, dW None), x without a gradient, a frozen weight.  Output channels that do not fill whole chunks raise.
  HeadConvGatherFn  y[..., :Cout] (fp32 out), y[..., Cout:] == 0, e bitwise the gathered rows; df, dW, db.  The loss reads the slice
                    y[..., :Cout] as forward_train does, so dy arrives zero-padded.  df's bound allows two roundings of the output type per pixel
                    however many rows land on it; the case carries quarter-ulp addends on pixel (0, 0) of the edge_len = 0 image (96 + 2 halo rows),
                    which a rounding per row loses entirely.  Again under set_deterministic: two runs bitwise equal, same bounds.
                    (`dy.shape[-1] < emin` in _conv_backward cannot be reached through this node: its cpad is at least one chunk.)
  EdgeScatterAddFn  exact: out == (base + add) rounded once to fp32 (unique border points: one fp32 add per element), dbase == g, do == the gathered,
                    masked rows; base contiguous and a slice of a wider map; o in fp32 / bf16 / fp16; base unchanged.

Worst error / bound on MI355X, fp32 | bf16 | fp16: fan-out y 0.005 | 0.94 | 0.76, dx 0.001 | 0.69 | 0.25, dW 0.013 | 0.002 | 0.002; gather y 0.015 |
0.004 | 0.005, dW 0.028 | 0.008 | 0.009, db 0.010 | 0 | 0.001, df 0.53 | 0.98 | 0.98 (0.39 | 0.90 | 0.96 at the teeth pixel); the scatter is exact.
With the row gradients added row by row into the 16-bit map (`index_add_`, as the node did before) df missed by up to 7.8 | 183 | 56.

The worst error-to-bound ratio per case and quantity goes to head_nodes_<mode>.json under $MFX_REPORT_DIR (default: the git-ignored artifacts/) and
is printed, with the conv / weight-gradient dispatch counter deltas of the case (information, not asserted)."""
import functools
import json
import os

import pytest
import torch

import head_nodes_ref as R

pytestmark = pytest.mark.gpu
DEV = "cuda"
D64 = torch.float64
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
REPORT_DIR = os.environ.get("MFX_REPORT_DIR") or os.path.join(ROOT, "artifacts")
MODES = ("fp32", "bf16", "fp16")
COUNTERS = ("conv_cw", "conv_halo", "conv_igemm", "conv_splitk", "wgrad_patch", "wgrad_tr", "wgrad_mfma", "wgrad_valu", "wgrad_reduce")
REPORT = {}


def _mods():
    from monoflex_amd import autograd as AG, lib as L
    return L.load(), L, AG


def _counters(lib):
    return {n: int(lib.mfx_get_counter(n.encode())) for n in COUNTERS}


def _record(mode, case, ratios, before=None):
    """Keep the worst ratio per (case, quantity), rewrite the mode's report file, print."""
    slot = REPORT.setdefault(mode, {}).setdefault(case, {})
    for k, v in ratios.items():
        slot[k] = max(slot.get(k, 0.0), float(v))
    moved = {}
    if before is not None:
        after = _counters(_mods()[0])
        moved = {n: after[n] - before[n] for n in COUNTERS if after[n] != before[n]}
        slot["counters"] = moved
    os.makedirs(REPORT_DIR, exist_ok=True)
    with open(os.path.join(REPORT_DIR, "head_nodes_%s.json" % mode), "w") as f:
        json.dump(dict(mode=mode, cases=REPORT[mode]), f, indent=1, sort_keys=True)
    print("head_nodes %s %s: %s %s" % (mode, case, " ".join("%s %.3g" % kv for kv in sorted(ratios.items())), moved))


def _check(ratios, what):
    bad = {k: v for k, v in ratios.items() if not v <= 1.0}
    assert not bad, "%s: error / bound above 1: %s" % (what, bad)


def _dev(t, mode):
    """float64 CPU tensor holding numbers of the mode's type -> device tensor of that type (exact)."""
    return t.to(R.DTYPES[mode]).contiguous().to(DEV)


# ---- FanOutConvFn ---------------------------------------------------------------------------------------------------------------------------------

@functools.lru_cache(maxsize=None)
def _fanout(case, mode, unused=None):
    c = R.fanout_case(*case, mode)
    dys = [None if i == unused else d for i, d in enumerate(c["dy"])]
    return c, R.fanout_ref(c["x"], c["w"], 1, dys)


def _fanout_bounds(case, r, mode):
    B, H, W, _ = case
    return dict(y=[R.bound_out(9 * R.FANOUT_CIN, M, y, mode) for M, y in zip(r["M"], r["y"])],
                dw=[None if m is None else R.bound_sum(B * H * W, m) for m in r["dw_mag"]],
                dx=R.bound_chain(9 * R.FANOUT_COUT, r["dgrad_mag"], r["S"], mode) if r["S"] else None)


def _run_fanout(AG, c, mode, unused=None, x_grad=True, frozen=None):
    n = len(c["w32"])
    xd = _dev(c["x"], mode).requires_grad_(x_grad)
    ws = [torch.nn.Parameter(w.to(DEV), requires_grad=i != frozen) for i, w in enumerate(c["w32"])]
    ys = AG.fanout_conv(xd, ws, 1)
    used = [i for i in range(n) if i != unused]
    torch.autograd.backward([ys[i] for i in used], [_dev(c["dy"][i], mode) for i in used])
    torch.cuda.synchronize()
    return [y.detach().cpu() for y in ys], (xd.grad.cpu() if xd.grad is not None else None), [w.grad.cpu() if w.grad is not None else None for w in ws]


def _fanout_ratios(got, r, bd):
    ys, dx, dws = got
    out = {"y": max(R.ratio(y, ry, b) for y, ry, b in zip(ys, r["y"], bd["y"]))}
    dwr = [R.ratio(g, rw, b) for g, rw, b in zip(dws, r["dw"], bd["dw"]) if g is not None]
    if dwr:
        out["dw"] = max(dwr)
    if dx is not None:
        out["dx"] = R.ratio(dx, r["S"][-1], bd["dx"])
    return out


@pytest.mark.parametrize("det", [False, True], ids=["atomics", "deterministic"])
@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("case", R.FANOUT_CASES, ids=lambda c: "x".join(map(str, c)))
def test_fanout_conv_node(case, mode, det):
    lib, L, AG = _mods()
    B, H, W, n = case
    td = R.DTYPES[mode]
    c, r = _fanout(case, mode)
    bd = _fanout_bounds(case, r, mode)
    before = _counters(lib)
    try:
        L.set_deterministic(det)
        got = _run_fanout(AG, c, mode)
        ys, dx, dws = got
        assert all(y.dtype == td and tuple(y.shape) == (B, H, W, R.FANOUT_COUT) for y in ys) and dx.dtype == td
        assert all(g is not None and g.dtype == torch.float32 for g in dws)
        ratios = _fanout_ratios(got, r, bd)
        # n separate Conv2dFn nodes on the same inputs: autograd adds their n input gradients in the activation type
        x2 = _dev(c["x"], mode).requires_grad_()
        w2 = [torch.nn.Parameter(w.to(DEV)) for w in c["w32"]]
        y2 = [AG.conv2d(x2, w, None, 1, 1) for w in w2]
        torch.autograd.backward(y2, [_dev(d, mode) for d in c["dy"]])
        torch.cuda.synchronize()
    finally:
        L.set_deterministic(False)
    for i in range(n):
        assert torch.equal(y2[i].detach().cpu(), ys[i]), "y%d differs from the separate node" % i
        g2 = w2[i].grad.cpu()
        if det:
            assert torch.equal(g2, dws[i]), "dW%d differs from the separate node" % i
        else:
            assert R.ratio(g2, dws[i].to(D64), 2 * bd["dw"][i]) <= 1.0
    # the separate formulation: every dgrad stored once, then n - 1 adds of autograd, each rounding the running sum once
    sep = torch.zeros_like(r["S"][0])
    for j in range(len(r["S"])):
        sep = sep + R.bound_out(9 * R.FANOUT_COUT, r["dgrad_mag"][j], r["dgrad"][j], mode) + (R.bound_out(0, 0.0, r["S"][j], mode) if j else 0.0)
    ratios["dx_vs_separate"] = R.ratio(x2.grad.cpu(), dx.to(D64), bd["dx"] + sep)
    _record(mode, "fanout_%dx%dx%dx%d%s" % (B, H, W, n, "_det" if det else ""), ratios, before)
    _check(ratios, "fan-out %s %s" % (case, mode))


@pytest.mark.parametrize("variant", ["unused_output", "x_without_grad", "frozen_weight"])
@pytest.mark.parametrize("mode", MODES)
def test_fanout_conv_node_variants(mode, variant):
    lib, L, AG = _mods()
    case = R.FANOUT_CASES[1]
    n = case[3]
    unused = 0 if variant == "unused_output" else None
    c, r = _fanout(case, mode, unused)
    bd = _fanout_bounds(case, r, mode)
    before = _counters(lib)
    got = _run_fanout(AG, c, mode, unused=unused, x_grad=variant != "x_without_grad", frozen=1 if variant == "frozen_weight" else None)
    ys, dx, dws = got
    if variant == "unused_output":
        assert dws[0] is None and dws[1] is not None and r["links"] == [1]       # dy is None: no gradient work for that branch
    elif variant == "x_without_grad":
        assert dx is None and all(g is not None for g in dws)                    # no dx: the chain is not built
    else:
        assert dws[1] is None and dws[0] is not None and dx is not None and len(r["S"]) == n      # the frozen weight's branch still feeds dx
    ratios = _fanout_ratios(got, r, bd)
    _record(mode, "fanout_%s" % variant, ratios, before)
    _check(ratios, "fan-out %s %s" % (variant, mode))


@pytest.mark.parametrize("mode", MODES)
def test_fanout_conv_node_rejects_partial_chunks(mode):
    _, _, AG = _mods()
    x = torch.zeros(1, 4, 4, R.FANOUT_CIN, dtype=R.DTYPES[mode], device=DEV)
    w = torch.nn.Parameter(torch.zeros(20, R.FANOUT_CIN, 3, 3, device=DEV))
    with pytest.raises(ValueError, match="whole 16-byte chunks"):
        AG.fanout_conv(x, [w], 1)


# ---- HeadConvGatherFn -----------------------------------------------------------------------------------------------------------------------------

@functools.lru_cache(maxsize=None)
def _gather(cout, bias, halo, mode):
    c = R.gather_case(cout, bias, halo, mode)
    return c, R.head_conv_gather_ref(c["f"], c["w"], c["b"], c["edges"]["rowmap"], c["dy"], c["de"])


def _run_gather(AG, c, mode):
    cout = c["w32"].shape[0]
    fd = _dev(c["f"], mode).requires_grad_()
    wd = torch.nn.Parameter(c["w32"].to(DEV))
    bd = torch.nn.Parameter(c["b32"].to(DEV)) if c["b32"] is not None else None
    y, e = AG.HeadConvGatherFn.apply(fd, wd, bd, c["edges"]["rowmap"].to(DEV))
    # upstream: fp32 on the 16-bit grid for the fp32 head map (sliced as forward_train slices it), the activation type for the rows
    torch.autograd.backward([y[..., :cout], e], [c["ry"].float().to(DEV), _dev(c["de"], mode)])
    torch.cuda.synchronize()
    return dict(y=y.detach().cpu(), e=e.detach().cpu(), df=fd.grad.cpu(), dw=wd.grad.cpu(), db=bd.grad.cpu() if bd is not None else None)


def _gather_ratios(g, c, r, mode):
    B, H, W = R.GATHER_MAP
    C, cout, cpad, td = R.GATHER_C, c["w32"].shape[0], r["cpad"], R.DTYPES[mode]
    assert g["y"].dtype == torch.float32 and tuple(g["y"].shape) == (B, H, W, cpad)
    assert float(g["y"][..., cout:].abs().max()) == 0 if cpad > cout else True                  # the padded channels are exactly zero
    assert g["e"].dtype == td and torch.equal(g["e"].to(D64), r["e"])                           # the rows are copies
    assert g["df"].dtype == td and g["dw"].dtype == torch.float32 and tuple(g["dw"].shape) == (cout, C, 1, 1)
    df_bound = R.bound_gather_df(r, mode)
    df = g["df"].reshape(-1, C)
    out = {"y": R.ratio(g["y"], r["y"], R.bound_out(C, r["y_mag"], r["y"], mode, u_out=R.U32)),
           "df": R.ratio(df, r["df_total"], df_bound),
           "df_pixel00": R.ratio(df[R.TEETH_PIXEL], r["df_total"][R.TEETH_PIXEL], df_bound[R.TEETH_PIXEL]),
           "dw": R.ratio(g["dw"], r["dw"], R.bound_sum(B * H * W, r["dw_mag"]))}
    if r["db"] is not None:
        assert g["db"].dtype == torch.float32 and tuple(g["db"].shape) == (cout,)
        out["db"] = R.ratio(g["db"], r["db"], R.bound_sum(B * H * W, r["db_mag"]))
    else:
        assert g["db"] is None
    return out


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("halo", R.GATHER_HALOS)
@pytest.mark.parametrize("cout,bias", R.GATHER_HEADS, ids=lambda v: str(v))
def test_head_conv_gather_node(cout, bias, halo, mode):
    lib, L, AG = _mods()
    c, r = _gather(cout, bias, halo, mode)
    case = "gather_cout%d_%s_halo%d" % (cout, "bias" if bias else "nobias", halo)
    before = _counters(lib)
    ratios = _gather_ratios(_run_gather(AG, c, mode), c, r, mode)
    _record(mode, case, ratios, before)
    try:
        L.set_deterministic(True)
        g1, g2 = _run_gather(AG, c, mode), _run_gather(AG, c, mode)
    finally:
        L.set_deterministic(False)
    for k in g1:
        assert (g1[k] is None and g2[k] is None) or torch.equal(g1[k], g2[k]), "deterministic mode: %s differs between two runs" % k
    det = _gather_ratios(g1, c, r, mode)
    _record(mode, case + "_det", det)
    _check(ratios, "%s %s" % (case, mode))
    _check(det, "%s %s deterministic" % (case, mode))


# ---- EdgeScatterAddFn -----------------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("odt", MODES)
@pytest.mark.parametrize("sliced", [False, True], ids=["contiguous", "sliced"])
@pytest.mark.parametrize("lo,co,cb", R.SCATTER_CFGS)
def test_edge_scatter_add_node(lo, co, cb, sliced, odt):
    _, _, AG = _mods()
    c = R.scatter_case(lo, co, cb)
    ed = c["edges"]
    wide = c["wide"].to(DEV).requires_grad_()
    base = wide[..., :cb] if sliced else wide.detach()[..., :cb].contiguous().requires_grad_()
    assert base.is_contiguous() != sliced
    keep = wide.detach().clone()
    o = _dev(c["o"], odt).requires_grad_()
    g = c["g"].float().to(DEV)
    out = AG.EdgeScatterAddFn.apply(base, o, ed["ei"].to(DEV), ed["el"].to(DEV), lo, ed["rows_center"].to(DEV), ed["valid_l"].float().to(DEV))
    gb, go = torch.autograd.grad(out, (base, o), g)
    torch.cuda.synchronize()
    want, dbase, do = R.edge_scatter_ref(c["base"], c["o"], ed["ei"], ed["el"], lo, ed["rows_center"], ed["valid_l"], c["g"])
    assert out.dtype == torch.float32 and out.is_contiguous()
    wrong = dict(out=int((out.detach().cpu() != want.float()).sum()), dbase=int((gb.cpu() != dbase.float()).sum()),
                 do=int((go.cpu().to(D64) != do).sum()), base=int((wide.detach() != keep).sum()))
    _record(odt, "scatter_lo%d_co%d_cb%d_%s" % (lo, co, cb, "sliced" if sliced else "contiguous"), wrong)
    assert go.dtype == o.dtype and wrong == dict(out=0, dbase=0, do=0, base=0), wrong
    assert 0 < int((want != c["base"]).sum()) <= 35 * co                                        # 28 + 7 border rows were added, none elsewhere
