"""tests/head_nodes_ref.py is right, and its bounds have teeth (no GPU).

  * every restatement against torch autograd in float64, on the dense formulation the nodes replace: n separate F.conv2d with their input gradients
    summed; a 1x1 conv plus the advanced-index gather at the replicate-padded sequence positions; index_put(accumulate=True).  1e-12 relative;
  * the multiplicity bound of the gather's df (head_nodes_ref.bound_gather_df) against the value a per-row-rounding implementation
    (`dx.index_add_(0, rowmap, de.to(dx.dtype))` on a 16-bit dx) produces at pixel (0, 0) of the edge_len = 0 image, computed here on the CPU: it
    must miss by at least 4x in bf16 and fp16.  Obtained on the 30 (Cout, bias, halo, type) cases of the GPU test: 11.4 .. 13.8x on the least
    affected channel of the teeth chunk, up to 24.8x on the most affected one (n_p = 96 + 2 halo addends of a quarter ulp each, all lost, against
    a bound of one to two ulp).  The form that sums the rows in fp32 and rounds once more stays inside the bound on every channel of the pixel;
  * a fan-out reference that leaves one branch out of the summed input gradient misses the chain bound by far more than 2x.
"""
import pytest
import torch
import torch.nn.functional as F

import head_nodes_ref as R

D64 = torch.float64


def _close(a, b, what):
    scale = float(b.abs().max())
    assert float((a - b).abs().max()) <= 1e-12 * max(scale, 1.0), what


@pytest.mark.parametrize("unused", [None, 1])
def test_fanout_ref_matches_autograd(unused):
    gen = torch.Generator().manual_seed(1)
    B, H, W, C, Co, n = 2, 5, 7, 8, 16, 3
    x = torch.randn(B, H, W, C, generator=gen, dtype=D64).requires_grad_()
    ws = [torch.randn(Co, C, 3, 3, generator=gen, dtype=D64).requires_grad_() for _ in range(n)]
    dys = [torch.randn(B, H, W, Co, generator=gen, dtype=D64) for _ in range(n)]
    if unused is not None:
        dys[unused] = None
    ys = [F.conv2d(x.permute(0, 3, 1, 2), w, padding=1).permute(0, 2, 3, 1) for w in ws]
    loss = sum((y * dy).sum() for y, dy in zip(ys, dys) if dy is not None)
    grads = torch.autograd.grad(loss, [x] + ws, allow_unused=True)
    r = R.fanout_ref(x.detach(), [w.detach() for w in ws], 1, dys)
    assert r["links"] == [i for i in range(n) if dys[i] is not None] and len(r["S"]) == len(r["links"])
    for i in range(n):
        _close(r["y"][i], ys[i].detach(), "y%d" % i)
        assert bool((r["M"][i] >= r["y"][i].abs() - 1e-12).all())
        if dys[i] is None:
            assert r["dw"][i] is None and grads[1 + i] is None
        else:
            _close(r["dw"][i], grads[1 + i], "dw%d" % i)
            assert bool((r["dw_mag"][i] >= r["dw"][i].abs() - 1e-12).all())
    _close(r["S"][-1], grads[0], "dx")
    _close(sum(r["dgrad"]), r["S"][-1], "partial sums")
    for d, m in zip(r["dgrad"], r["dgrad_mag"]):
        assert bool((m >= d.abs() - 1e-12).all())


@pytest.mark.parametrize("halo", [0, 1, 2, 3])
@pytest.mark.parametrize("bias", [True, False])
def test_head_conv_gather_ref_matches_autograd(halo, bias):
    gen = torch.Generator().manual_seed(2 + halo)
    B, H, W, C, Cout, cpad, Lmax = 3, 5, 8, 16, 3, 8, 30
    ed = R.edge_case(B, H, W, Lmax, [0, 22, 5], halo)
    Lp = ed["Lp"]
    f = torch.randn(B, H, W, C, generator=gen, dtype=D64).requires_grad_()
    w = torch.randn(Cout, C, 1, 1, generator=gen, dtype=D64).requires_grad_()
    b = torch.randn(Cout, generator=gen, dtype=D64).requires_grad_() if bias else None
    ry = torch.randn(B, H, W, Cout, generator=gen, dtype=D64)
    de = torch.randn(B * Lp, C, generator=gen, dtype=D64)
    # the dense two-node formulation (detector_predictor.forward_train without the fused nodes)
    pos = torch.arange(-halo, Lmax + halo).clamp(0, Lmax - 1)
    xy = ed["ei"][:, pos].long()
    bidx = torch.arange(B).view(B, 1).expand(B, Lp)
    y0 = f @ w.view(Cout, C).t() + (b if bias else 0.0)
    e0 = f[bidx, xy[..., 1], xy[..., 0]]
    want = torch.autograd.grad((y0 * ry).sum() + (e0 * de.view(B, Lp, C)).sum(), [f, w] + ([b] if bias else []))
    r = R.head_conv_gather_ref(f.detach(), w.detach(), b.detach() if bias else None, ed["rowmap"], F.pad(ry, (0, cpad - Cout)), de)
    _close(r["y"][..., :Cout], y0.detach(), "y")
    assert r["y"].shape[-1] == cpad and float(r["y"][..., Cout:].abs().max()) == 0
    assert torch.equal(r["e"].view(B, Lp, C), e0.detach())
    _close(r["df_total"].view(B, H, W, C), want[0], "df")
    _close(r["dw"], want[1], "dw")
    if bias:
        _close(r["db"], want[2], "db")
    else:
        assert r["db"] is None
    # multiplicity: every position of the edge_len = 0 image lands on its pixel (0, 0); a pixel no position names receives nothing
    assert int(r["n_p"][0]) == Lp and float(r["n_p"].sum()) == B * Lp
    assert torch.equal(r["df_total"][r["n_p"] == 0], r["df_conv"][r["n_p"] == 0])
    assert bool((r["sum_abs_de"] >= (r["df_total"] - r["df_conv"]).abs() - 1e-12).all())


@pytest.mark.parametrize("lo,co,cb", R.SCATTER_CFGS)
def test_edge_scatter_ref_matches_autograd(lo, co, cb):
    c = R.scatter_case(lo, co, cb)
    ed = c["edges"]
    B, L = c["o"].shape[:2]
    base, o = c["base"].clone().requires_grad_(), c["o"].clone().requires_grad_()
    bl = torch.arange(B).view(B, 1).expand(B, L)
    add = torch.zeros(*base.shape[:3], co, dtype=D64).index_put((bl, ed["ei"][..., 1].long(), ed["ei"][..., 0].long()), o * ed["valid_l"],
                                                                 accumulate=True)
    want = base + F.pad(add, (lo, cb - lo - co))
    gb, go = torch.autograd.grad((want * c["g"]).sum(), (base, o))
    out, dbase, do = R.edge_scatter_ref(c["base"], c["o"], ed["ei"], ed["el"], lo, ed["rows_center"], ed["valid_l"], c["g"])
    _close(out, want.detach(), "out")
    _close(dbase, gb, "dbase")
    _close(do, go, "do")
    assert float(do[0].abs().max()) == 0 and float(do[2, 7:].abs().max()) == 0            # padding rows receive no gradient


def test_edge_case_builder():
    """Explicit edge_len, Lmax beyond the border, the plan tensors of halo 0 .. 3 as the predictor's edge_plan builds them."""
    B, H, W = R.GATHER_MAP
    assert len(R.border_points(H, W)) == 28 == len(set(R.border_points(H, W)))
    for halo in range(4):
        ed = R.edge_case(B, H, W, R.GATHER_LMAX, R.GATHER_EDGE_LEN, halo)
        Lp = R.GATHER_LMAX + 2 * halo
        rm = ed["rowmap"].view(B, Lp)
        assert ed["rows_center"].numel() == B * R.GATHER_LMAX and torch.equal(ed["rows_center"].view(B, -1), rm[:, halo:Lp - halo])
        assert bool((rm[0] == 0).all())                                                   # edge_len 0: pixel (0, 0) of image 0, every position
        assert len(set(rm[1, halo:halo + 28].tolist())) == 28                             # the whole border, every pixel once
        assert bool((rm[1, halo + 28:] == H * W).all()) and bool((rm[2, halo + 7:] == 2 * H * W).all())
        assert ed["valid_l"].sum(1).flatten().tolist() == [0.0, 28.0, 7.0]


@pytest.mark.parametrize("mode", ["bf16", "fp16"])
@pytest.mark.parametrize("halo", R.GATHER_HALOS)
@pytest.mark.parametrize("cout,bias", R.GATHER_HEADS)
def test_multiplicity_bound_has_teeth(cout, bias, halo, mode):
    c = R.gather_case(cout, bias, halo, mode)
    r = R.head_conv_gather_ref(c["f"], c["w"], c["b"], c["edges"]["rowmap"], c["dy"], c["de"])
    p, ch = R.TEETH_PIXEL, slice(c["chunk"], c["chunk"] + 8)
    bound = R.bound_gather_df(r, mode)[p]
    assert int(r["n_p"][p]) == R.GATHER_LMAX + 2 * halo
    assert torch.equal(R.on_grid(r["df_conv"][p], mode), c["v"])
    # addends of a quarter ulp: all of one sign per channel of the chunk
    rows = c["de"][c["edges"]["rowmap"] == p][:, ch]
    assert bool((rows == rows[0]).all()) and torch.equal(rows[0].abs() * 4, R.ulp(c["v"][ch], mode))
    bad = R.per_row_rounding(c, r, mode)
    assert torch.equal(bad[ch], c["v"][ch])                                               # every addend was lost
    miss = ((bad - r["df_total"][p]).abs() / bound)[ch]
    print("per-row rounding misses the bound by %.1f .. %.1fx on the teeth chunk (%s, Cout %d, halo %d)" % (float(miss.min()), float(miss.max()),
                                                                                                        mode, cout, halo))
    assert float(miss.min()) >= 4.0, float(miss.min())
    good = R.summed_then_rounded(c, r, mode)
    assert float(((good - r["df_total"][p]).abs() / bound).max()) <= 1.0


def test_fanout_bound_has_teeth():
    B, H, W, n = R.FANOUT_CASES[1]
    for mode in ("bf16", "fp16", "fp32"):
        c = R.fanout_case(B, H, W, n, mode)
        r = R.fanout_ref(c["x"], c["w"], 1, c["dy"])
        bound = R.bound_chain(9 * R.FANOUT_COUT, r["dgrad_mag"], r["S"], mode)
        for j in range(n):
            wrong = r["S"][-1] - r["dgrad"][j]
            assert R.ratio(wrong, r["S"][-1], bound) >= 2.0
        assert R.ratio(r["S"][-1], r["S"][-1], bound) == 0.0
