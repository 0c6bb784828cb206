"""The edge fusion under its other settings -- MODEL.HEAD.EDGE_FUSION_KERNEL_SIZE k (any odd window), EDGE_FUSION_NORM 'BN' or anything else
(no norm: Conv1d with its bias), EDGE_FUSION_RELU -- stated in plain float64 torch, test-only.  It generalises tests/edge_chain_ref.py (the conv
chain of the eval path with its first-order rounding bound; k = 3, BN) and tests/head_act_ref.py's HeadActRef (the whole predictor, eval and train;
k = 3, BN), neither of which changes.

tests/golden/edge_fusion_settings.npz (tools/gen_edge_fusion_golden.py) holds what the reference's own predictor returns under five settings for the
seeded inputs of tests/head_act_ref.py; tests/test_edge_fusion_settings_cpu.py pins this statement to it, tests/test_gpu_edge_fusion_settings.py
compares the kernels with this statement, gradients being torch autograd of it in float64.

`tap_shift` and `norm` deliberately mis-state it: a window off by one tap, or a BatchNorm where the setting has none (its parameters then come from
`norm_state`), are what the CPU tests show the recording tells apart."""
import torch
import torch.nn.functional as F

from head_act_ref import HeadActRef

D64 = torch.float64
SETTINGS = ((1, "BN", False), (5, "BN", False), (7, "BN", True), (3, "none", False), (5, "none", True))      # (k, EDGE_FUSION_NORM, EDGE_FUSION_RELU): the recorded ones


def setting_name(k, norm, relu):
    return "k%d_%s_%s" % (k, "bn" if norm == "BN" else "none", "relu" if relu else "lin")


def setting_opts(k, norm, relu):
    """The configuration overrides of a setting (yacs list form)."""
    return ["MODEL.HEAD.EDGE_FUSION_KERNEL_SIZE", k, "MODEL.HEAD.EDGE_FUSION_NORM", norm, "MODEL.HEAD.EDGE_FUSION_RELU", bool(relu)]


def pad_window(e, k, shift=0):
    """(B, C, L) -> (B, C, L + k - 1): replicate padding k // 2 on both sides, as Conv1d(padding=k // 2, padding_mode='replicate') of an odd k (several
    taps read the same position where L <= k // 2; F.pad's own replicate mode refuses a padding >= L).  `shift`: the window moved by that many
    positions (a wrong statement, for the tests' counter-example)."""
    h, L = k // 2, e.shape[-1]
    return e[..., torch.arange(-h + shift, L + h + shift).clamp(0, L - 1)]


class EdgeFusionRef(HeadActRef):
    """HeadActRef with the edge fusion's window and norm as the configuration (or the caller) names them."""

    def __init__(self, sd, cfg, slope=0.0, requires_grad=False, tap_shift=0, norm=None, norm_state=None):
        super().__init__(sd, cfg, slope, requires_grad)
        self.window = int(cfg.MODEL.HEAD.EDGE_FUSION_KERNEL_SIZE)
        self.norm = (cfg.MODEL.HEAD.EDGE_FUSION_NORM == "BN") if norm is None else norm
        self.tap_shift = tap_shift
        for k, v in (norm_state or {}).items():
            self.p[k] = v.detach().double().clone()
        assert self.window % 2 == 1
        self.edge_out = {}                  # after forward(): per fusion the (B, c, L) output at every sequence position

    def _edge(self, e, prefix, train):
        """(B, 256, L) -> Conv1d k (replicate padding over the whole padded sequence) -> [BN1d] -> [ReLU] -> Conv1d 1x1."""
        p = self.p
        y = F.conv1d(pad_window(e, self.window, self.tap_shift), p[prefix + ".0.weight"], p[prefix + ".0.bias"])
        if self.norm:
            y = self._bn(y, prefix + ".1", train, (0, 2))
        if self.edge_relu:
            y = y.relu()
        o = F.conv1d(y, p[prefix + ".3.weight"], p[prefix + ".3.bias"])
        self.edge_out[prefix] = o
        return o


def _fold64(bn, bias=None):
    if bn is None or isinstance(bn, torch.nn.Identity):
        b = bias.detach().to(D64)
        return torch.ones_like(b), b
    scale = bn.weight.detach().to(D64) / torch.sqrt(bn.running_var.detach().to(D64) + bn.eps)
    shift = bn.bias.detach().to(D64) - bn.running_mean.detach().to(D64) * scale
    if bias is not None:
        shift = shift + bias.detach().to(D64) * scale
    return scale, shift


def chain_operands(pred, dtype=None):
    """edge_chain_ref.chain_operands for any window and with or without the BN1d (no norm: s_conv = 1, t_conv = the Conv1d's bias); `slope`: the trunk
    activation below zero (0.01 InPlaceABN, 0 BatchNorm2d + ReLU)."""
    rnd = (lambda t: t.detach().to(D64)) if dtype is None else (lambda t: t.detach().to(dtype).to(D64))
    oi = pred.offset_index[0]
    out = []
    for trunk, seq in ((pred.class_head, pred.trunc_heatmap_conv), (pred.reg_features[oi], pred.trunc_offset_conv)):
        s0, t0 = _fold64(trunk[1])
        s1, t1 = _fold64(seq[1], seq[0].bias)
        out.append(dict(w_trunk=rnd(trunk[0].weight), s_trunk=s0, t_trunk=t0, w_conv=rnd(seq[0].weight), s_conv=s1, t_conv=t1,
                        w_out=rnd(seq[3].weight), b_out=seq[3].bias.detach().to(D64), relu=isinstance(seq[2], torch.nn.ReLU),
                        slope=0.0 if isinstance(trunk[1], torch.nn.BatchNorm2d) else 0.01))
    return out


def edge_chain_ref(x, edge_xy, branches, unit_roundoff=None):
    """edge_chain_ref.edge_chain_ref with the window read from w_conv: x (B,64,H,W) float64, edge_xy (B,L,2) integer (x, y) -> per branch (B, c, L)
    float64, the Conv1d stack's output at EVERY sequence position; with `unit_roundoff` u per branch (output, bound),
        bound = u |W_out| (|z| + |s_conv| (|W_conv| * |t|))
    what rounding the trunk t and the Conv1d output z to the activation type can move each output by, to first order in u (derivation there; with no
    norm |s_conv| = 1)."""
    B = x.shape[0]
    bidx = torch.arange(B).view(B, 1)
    xs, ys = edge_xy[..., 0].long(), edge_xy[..., 1].long()
    outs = []
    for p in branches:
        k = p["w_conv"].shape[-1]
        t = F.conv2d(x, p["w_trunk"], None, 1, 1) * p["s_trunk"].view(1, -1, 1, 1) + p["t_trunk"].view(1, -1, 1, 1)
        t = F.leaky_relu(t, p["slope"])
        e = t[bidx, :, ys, xs].permute(0, 2, 1)                                     # (B, 256, L)
        z = F.conv1d(pad_window(e, k), p["w_conv"]) * p["s_conv"].view(1, -1, 1) + p["t_conv"].view(1, -1, 1)
        if p["relu"]:
            z = F.relu(z)
        o = F.conv1d(z, p["w_out"], p["b_out"])
        if unit_roundoff is None:
            outs.append(o)
            continue
        moved = F.conv1d(pad_window(e.abs(), k), p["w_conv"].abs()) * p["s_conv"].abs().view(1, -1, 1)
        outs.append((o, unit_roundoff * F.conv1d(z.abs() + moved, p["w_out"].abs())))
    return outs


def rowmap_loop(edge_indices, H, W, halo):
    """make_edge_rowmap as a plain loop: the flat pixel of the sequence positions -halo .. L - 1 + halo of every image, clamped to 0 .. L - 1."""
    B, Lm = edge_indices.shape[0], edge_indices.shape[1]
    out = []
    for b in range(B):
        for q in range(-halo, Lm + halo):
            x, y = edge_indices[b, min(max(q, 0), Lm - 1)].tolist()
            out.append(b * H * W + y * W + x)
    return out
