"""float64 reference of the edge fusion's conv chain (detector_predictor.py:111-119,136-158), test-only: per fusion branch the 3x3 trunk + folded ABN +
LeakyReLU(0.01) at the border points, the replicate-padded k = 3 Conv1d + folded BN1d (+ ReLU) along the point sequence, and the 1x1 + bias.  No
intermediate is rounded; what the operands are rounded to before they enter is the caller's choice (`chain_operands(..., dtype)`)."""
import torch
import torch.nn.functional as F

D64 = torch.float64


def _fold64(bn, bias=None):
    scale = bn.weight.detach().to(D64) / torch.sqrt(bn.running_var.detach().to(D64) + bn.eps)
    shift = bn.bias.detach().to(D64) - bn.running_mean.detach().to(D64) * scale
    if bias is not None:
        shift = shift + bias.detach().to(D64) * scale
    return scale, shift


def chain_operands(pred, dtype=None):
    """The two fusion branches (class, 3d_offset) of a predictor -- the product's or the oracle's: both name their modules alike -- as float64
    operands: weights rounded to `dtype` first (None: as they are), the folded normalisations exact.  `relu`: whether a ReLU follows the BN1d."""
    rnd = (lambda t: t.detach().to(D64)) if dtype is None else (lambda t: t.detach().to(dtype).to(D64))
    oi = pred.offset_index[0]
    out = []
    for trunk, seq in ((pred.class_head, pred.trunc_heatmap_conv), (pred.reg_features[oi], pred.trunc_offset_conv)):
        s0, t0 = _fold64(trunk[1])
        s1, t1 = _fold64(seq[1], seq[0].bias)
        out.append(dict(w_trunk=rnd(trunk[0].weight), s_trunk=s0, t_trunk=t0, w_conv=rnd(seq[0].weight), s_conv=s1, t_conv=t1,
                        w_out=rnd(seq[3].weight), b_out=seq[3].bias.detach().to(D64), relu=isinstance(seq[2], torch.nn.ReLU)))
    return out


def edge_chain_ref(x, edge_xy, branches, unit_roundoff=None):
    """x (B,64,H,W) float64, edge_xy (B,L,2) integer (x, y), `branches` from chain_operands -> per branch (B, c, L) float64: the Conv1d stack's
    output at EVERY sequence position (the padding rows of edge_xy included, from the pixel they list).

    With `unit_roundoff` u (2^-8 for bfloat16's 8 significant bits, 2^-11 for IEEE half) the result is per branch (output, bound): `bound` is what
    rounding the two intermediates to that type can move each output by at most, to first order in u.  An element t of the trunk moves by <= u |t|,
    which reaches the output through |W_conv|, |s_conv|, a 1-Lipschitz activation and |W_out|; an element z of the Conv1d output moves by
    <= u |z| on top, which reaches the output through |W_out|:  bound = u |W_out| (|z| + |s_conv| (|W_conv| * |t|))."""
    B = x.shape[0]
    bidx = torch.arange(B).view(B, 1)
    xs, ys = edge_xy[..., 0].long(), edge_xy[..., 1].long()
    outs = []
    for p in branches:
        t = F.conv2d(x, p["w_trunk"], None, 1, 1) * p["s_trunk"].view(1, -1, 1, 1) + p["t_trunk"].view(1, -1, 1, 1)
        t = F.leaky_relu(t, 0.01)
        e = t[bidx, :, ys, xs].permute(0, 2, 1)                                     # (B, 256, L)
        z = F.conv1d(F.pad(e, (1, 1), mode="replicate"), p["w_conv"]) * p["s_conv"].view(1, -1, 1) + p["t_conv"].view(1, -1, 1)
        if p["relu"]:
            z = F.relu(z)
        o = F.conv1d(z, p["w_out"], p["b_out"])
        if unit_roundoff is None:
            outs.append(o)
            continue
        moved = F.conv1d(F.pad(e.abs(), (1, 1), mode="replicate"), p["w_conv"].abs()) * p["s_conv"].abs().view(1, -1, 1)
        outs.append((o, unit_roundoff * F.conv1d(z.abs() + moved, p["w_out"].abs())))
    return outs
