"""Host logic of the training path's edge-fusion nodes (autograd.HeadConvGatherFn / EdgeScatterAddFn), on CPU: the device operators
they call (conv, data/weight gradient, border scatter) are replaced by plain torch stand-ins, so what is checked here is the index
arithmetic and the gradient routing of the nodes against the reference formulation (detector_predictor.py:125-147: gather of the
trunk at the edge points, '+=' of the edge outputs at the border pixels) differentiated by torch autograd."""
import types

import pytest
import torch
import torch.nn.functional as F

from monoflex_amd import autograd as AG, ops
from monoflex_amd.model.head.detector_predictor import make_edge_rowmap


def _edges(B, H, W, L, gen):
    """Unique border points per image (first edge_len entries), zero padding after, like the reference's edge_indices."""
    ei = torch.zeros(B, L, 2, dtype=torch.int32)
    el = torch.zeros(B, dtype=torch.int32)
    border = [(x, 0) for x in range(W)] + [(W - 1, y) for y in range(1, H)] + [(x, H - 1) for x in range(W - 1)] + [(0, y) for y in range(1, H - 1)]
    for b in range(B):
        n = int(torch.randint(3, min(L, len(border)) + 1, (1,), generator=gen))
        start = int(torch.randint(0, len(border), (1,), generator=gen))
        pts = [border[(start + i) % len(border)] for i in range(n)]
        ei[b, :n] = torch.tensor(pts, dtype=torch.int32)
        el[b] = n
    return ei, el


@pytest.fixture
def cpu_ops(monkeypatch):
    def scatter(out, ch_off, C, v, edge_xy, edge_len, planar=None):
        for b in range(out.shape[0]):
            for j in range(int(edge_len[b])):
                x, y = int(edge_xy[b, j, 0]), int(edge_xy[b, j, 1])
                out[b, y, x, ch_off:ch_off + C] += v[b, j, :C]
    monkeypatch.setattr(ops, "edge_scatter_add", scatter)

    def pack_weight(weight, dtype, mode, rows, ck, stride, pad_h, pad_w, shift=None):
        return types.SimpleNamespace(weight=weight.detach(), shift=shift, rows=rows)

    def conv2d(x, p, out_dtype=None, **kw):                      # 1x1 NHWC conv with padded output channels
        w = p.weight.reshape(p.weight.shape[0], -1).float()
        y = x.float() @ w.t()
        if p.rows > y.shape[-1]:
            y = F.pad(y, (0, p.rows - y.shape[-1]))
        if p.shift is not None:
            y = y + p.shift[:y.shape[-1]]
        return y.to(out_dtype or x.dtype)

    def conv_backward(x, weight, dy, stride, pad, has_bias, Cout, needs, res=None):
        w = weight.reshape(weight.shape[0], -1).float()
        g = dy[..., :Cout].float()
        dx = (g @ w).to(x.dtype)
        dw = (g.reshape(-1, Cout).t() @ x.reshape(-1, x.shape[-1]).float()).view_as(weight)
        return dx, dw, (g.reshape(-1, Cout).sum(0) if has_bias else None)

    monkeypatch.setattr(AG, "_pack_weight", pack_weight)
    monkeypatch.setattr(ops, "conv2d", conv2d)
    monkeypatch.setattr(AG, "_conv_backward", conv_backward)
    monkeypatch.setattr(ops, "cout_pad", lambda n: n)


@pytest.mark.parametrize("lo,co,cb", [(0, 3, 3), (4, 2, 7)])
def test_edge_scatter_add_node_matches_reference_formulation(cpu_ops, lo, co, cb):
    gen = torch.Generator().manual_seed(5)
    B, H, W, L = 3, 6, 9, 20
    ei, el = _edges(B, H, W, L, gen)
    base = torch.randn(B, H, W, cb, generator=gen).requires_grad_()
    o = torch.randn(B, L, co, generator=gen).requires_grad_()
    r = torch.randn(B, H, W, cb, generator=gen)
    # reference formulation (static shapes, as the predictor's torch path)
    valid = (torch.arange(L).view(1, L) < el.view(B, 1).long()).float()
    bl = torch.arange(B).view(B, 1).expand(B, L)
    add = torch.zeros(B, H, W, co).index_put((bl, ei[..., 1].long(), ei[..., 0].long()), o * valid.unsqueeze(-1), accumulate=True)
    want = base + F.pad(add, (lo, cb - lo - co))
    gb, go = torch.autograd.grad((want * r).sum(), (base, o))
    # the node
    rm = make_edge_rowmap(ei, H, W).long()
    rows = rm.view(B, L + 2)[:, 1:-1].reshape(-1)
    got = AG.EdgeScatterAddFn.apply(base, o, ei, el, lo, rows, valid.unsqueeze(-1))
    hb, ho = torch.autograd.grad((got * r).sum(), (base, o))
    assert torch.allclose(got, want, atol=1e-6) and torch.allclose(hb, gb) and torch.allclose(ho, go, atol=1e-6)
    # a non-contiguous base (the sliced padded conv output) takes the same path
    wide = torch.randn(B, H, W, cb + 1, generator=gen)
    got2 = AG.EdgeScatterAddFn.apply(wide[..., :cb], o, ei, el, lo, rows, valid.unsqueeze(-1))
    assert torch.allclose(got2 - wide[..., :cb], want.detach() - base.detach(), atol=1e-6)


def test_head_conv_gather_node_matches_two_nodes(cpu_ops):
    gen = torch.Generator().manual_seed(6)
    B, H, W, L, C, Cout = 2, 5, 8, 14, 16, 3
    ei, el = _edges(B, H, W, L, gen)
    f = torch.randn(B, H, W, C, generator=gen).requires_grad_()
    w = torch.randn(Cout, C, 1, 1, generator=gen).requires_grad_()
    b = torch.randn(Cout, generator=gen).requires_grad_()
    ry = torch.randn(B, H, W, Cout, generator=gen)
    re = torch.randn(B, L + 2, C, generator=gen)
    # two nodes: 1x1 conv, and the gather at positions -1 .. L with replicate padding (k = 3 Conv1d)
    pos = torch.arange(-1, L + 1).clamp(0, L - 1)
    xy = ei[:, pos].long()
    bidx = torch.arange(B).view(B, 1).expand(B, L + 2)
    y_ref = f @ w.view(Cout, C).t() + b
    e_ref = f[bidx, xy[..., 1], xy[..., 0]]
    want = torch.autograd.grad((y_ref * ry).sum() + (e_ref * re).sum(), (f, w, b))
    rm = make_edge_rowmap(ei, H, W).long()
    y, e = AG.HeadConvGatherFn.apply(f, w, b, rm)
    assert y.shape[-1] >= Cout and torch.allclose(y[..., :Cout], y_ref, atol=1e-5)
    assert torch.equal(e.view(B, L + 2, C), e_ref)
    got = torch.autograd.grad((y[..., :Cout] * ry).sum() + (e.view(B, L + 2, C) * re).sum(), (f, w, b))
    for g, h in zip(got, want):
        assert torch.allclose(g, h, atol=1e-4), float((g - h).abs().max())


@pytest.mark.parametrize("halo", [0, 1, 3])
def test_edge_first_rows_matches_a_python_loop(halo):
    """autograd.edge_first_rows (where HeadConvGatherFn sums the row gradients of one pixel): the smallest position naming the same pixel, for
    images without edge points, with the whole border and with a few points; int32 and int64 row maps alike."""
    B, H, W, L = 3, 6, 10, 40
    border = [(x, 0) for x in range(W)] + [(W - 1, y) for y in range(1, H)] + [(x, H - 1) for x in range(W - 1)] + [(0, y) for y in range(1, H - 1)]
    ei = torch.zeros(B, L, 2, dtype=torch.int32)
    ei[1, :len(border)] = torch.tensor(border, dtype=torch.int32)
    ei[2, :7] = torch.tensor(border[5:12], dtype=torch.int32)
    rm = make_edge_rowmap(ei, H, W, halo)
    seen, want = {}, []
    for j, p in enumerate(rm.tolist()):
        want.append(seen.setdefault(p, j))
    for r in (rm, rm.long()):
        first = AG.edge_first_rows(r, B)
        assert first.dtype == torch.int64 and first.tolist() == want
    assert want[:L + 2 * halo] == [0] * (L + 2 * halo) and len(set(want)) == 1 + (28 + 1 - 1) + (7 + 1)


def test_padded_bias_registry_follows_the_parameter():
    """autograd._padded_bias: persistent zero-padded copy of a bias parameter -- same buffer every step, refreshed when the
    parameter's version moves (on demand) or by pack_all_weights() (one _foreach_copy_), dropped with the parameter."""
    import gc
    reg = AG._PADS
    n0 = len(reg.entries)
    b = torch.nn.Parameter(torch.arange(1., 28.))                      # the 27-channel offset/mask conv bias
    p1 = AG._padded_bias(b, 32)
    assert p1.shape == (32,) and torch.equal(p1[:27], b.detach()) and float(p1[27:].abs().sum()) == 0
    assert AG._padded_bias(b, 32) is p1                                # handed out again, nothing copied
    with torch.no_grad():
        b.mul_(2.0)                                                    # an optimizer step: version moves
    assert torch.equal(AG._padded_bias(b, 32)[:27], b.detach()) and AG._padded_bias(b, 32) is p1
    with torch.no_grad():
        b.add_(1.0)
    reg.refresh_all()                                                  # what pack_all_weights() runs at the top of a step
    assert torch.equal(p1[:27], b.detach()) and float(p1[27:].abs().sum()) == 0
    # exact size: the parameter itself; a temporary (stacked head biases): padded on the spot
    c = torch.nn.Parameter(torch.ones(16))
    assert AG._padded_bias(c, 16).data_ptr() == c.data_ptr()
    t = torch.cat([torch.ones(3), torch.zeros(2)])
    assert torch.equal(AG._padded_bias(t, 8), torch.nn.functional.pad(t, (0, 3))) and len(reg.entries) == n0 + 1
    del b, p1
    gc.collect()
    assert len(reg.entries) == n0


def test_edge_position_of_rows_matches_a_python_loop():
    """detector_predictor.edge_position_of_rows (the 3d_offset branch in the sparse set: an object whose centre is a border pixel receives that
    pixel's fused edge output): against a loop over objects and edge positions; padding positions beyond edge_len never match."""
    import torch
    from monoflex_amd.model.head.detector_predictor import edge_position_of_rows, make_edge_rowmap
    g = torch.Generator().manual_seed(9)
    B, H, W, Lmax, N = 3, 8, 12, 2 * (8 + 12), 14
    edge_indices = torch.zeros(B, Lmax, 2, dtype=torch.int32)
    edge_lens = torch.tensor([2 * (H + W) - 4, 17, 0], dtype=torch.int32)
    border = [(x, 0) for x in range(W)] + [(W - 1, y) for y in range(1, H)] + [(x, H - 1) for x in range(W - 2, -1, -1)] + [(0, y) for y in range(H - 2, 0, -1)]
    for b in range(B):
        for l in range(int(edge_lens[b])):
            edge_indices[b, l, 0], edge_indices[b, l, 1] = border[l]
    rm = make_edge_rowmap(edge_indices, H, W).long()
    rows_center = rm.view(B, Lmax + 2)[:, 1:-1].reshape(-1)
    valid_l = (torch.arange(Lmax).view(1, Lmax) < edge_lens.view(B, 1)).float().unsqueeze(-1)
    rows = torch.zeros(N, 72)
    rows[:, 0] = (torch.rand(N, generator=g) > 0.2).float()
    rows[:, 57] = torch.randint(0, B, (N,), generator=g).float()
    rows[:, 2] = torch.randint(0, W, (N,), generator=g).float()
    rows[:, 3] = torch.randint(0, H, (N,), generator=g).float()
    rows[0, :4] = torch.tensor([1.0, 0.0, 0.0, 0.0]); rows[0, 57] = 0                       # corner pixel (0, 0) of image 0: edge position 0
    rows[1, 0], rows[1, 57], rows[1, 2], rows[1, 3] = 1.0, 1.0, float(W - 1), float(H - 1)  # border pixel of image 1 beyond its edge_len
    rows[2, 0], rows[2, 57], rows[2, 2], rows[2, 3] = 1.0, 2.0, 0.0, 0.0                    # image 2 has no edge points: padding must not match
    e_idx, hit = edge_position_of_rows(rows, rows_center, valid_l, B, H, W)
    for r in range(N):
        b, x, y = int(rows[r, 57]), int(rows[r, 2]), int(rows[r, 3])
        want = [b * Lmax + l for l in range(int(edge_lens[b])) if (int(edge_indices[b, l, 0]), int(edge_indices[b, l, 1])) == (x, y)]
        if want and rows[r, 0] > 0:
            assert bool(hit[r]) and int(e_idx[r]) == want[0], r
        else:
            assert not bool(hit[r]), r
    assert bool(hit[0]) and int(e_idx[0]) == 0 and not bool(hit[2])
