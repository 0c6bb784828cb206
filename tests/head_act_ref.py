"""MODEL.INPLACE_ABN False: the predictor whose trunks are conv3x3 -> BatchNorm2d -> ReLU, stated in plain float64 torch.

The reference builds this form by default (config/defaults.py; model/head/detector_predictor.py:53-58,75-77): only its two runs/*.yaml files
switch the third-party InPlaceABN on.  oracle/monoflex_ref.py's Predictor is the leaky (ABN) form; this module is the CPU statement of the
BN + ReLU form, eval and train, with the activation's slope below zero as a parameter (0: ReLU; 0.01: what a build that still computed the
ABN form would give -- tests/test_head_act_cpu.py shows that the two differ by far more than any tolerance a device test grants).

tests/golden/head_act.npz (tools/gen_head_act_golden.py) holds what the reference's own predictor returns for the inputs below, as seeds and
results; tests/test_head_act_cpu.py pins this statement to it, tests/test_gpu_head_act.py compares the kernels with this statement.

Inputs (all seeded, nothing stored): the state is monoflex_amd.synthetic.synthetic_state_dict of the predictor's own state dict, with every
fourth channel of each trunk norm's beta moved to -BETA_SHIFT: those channels are dead under ReLU (so more than a fifth of the trunk
activations are exactly zero) and strongly negative under a leaky ReLU (so the two forms are far apart in every output map).
"""
import os

import torch
import torch.nn.functional as F

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
B, H, W = 2, 24, 40                                  # the shape of tests/test_gpu_ops.py test_heads_fused_vs_torch
SEEDS = dict(state_seed=7, x_seed=9, loss_seed=13)
BETA_SHIFT = 400.0
ORIG_SIZES = ((W * 4 - 4, H * 4 - 2), (W * 4 - 28, H * 4 - 14))      # un-padded frame of each image: two edge sequences of different length
STAT_TRUNKS = ("class_head.1", "reg_features.1.1")                   # the two trunks whose running statistics the golden holds
SUBSET = 3                                                             # the golden's train-mode `reg` and `d features`: every third pixel


def make_cfg(inplace_abn=False, extra=()):
    from monoflex_amd.config import get_cfg
    cfg = get_cfg(os.path.join(ROOT, "runs", "monoflex.yaml"))
    cfg.MODEL.INPLACE_ABN = inplace_abn
    cfg.MODEL.PRETRAIN = False
    cfg.INPUT.WIDTH_TRAIN, cfg.INPUT.HEIGHT_TRAIN = W * 4, H * 4
    if extra:
        cfg.merge_from_list(list(extra))
    return cfg


def trunk_norms(keys):
    """'class_head.1', 'reg_features.0.1', ...: the norm of every trunk, from a state dict's keys."""
    return [k[:-len(".running_mean")] for k in keys if k.endswith(".1.running_mean") and (k.startswith("class_head") or k.startswith("reg_features"))]


def synthetic_state(template, seed=SEEDS["state_seed"]):
    """The state every head_act test uses: synthetic_state_dict + the beta shift described in the module docstring."""
    from monoflex_amd import synthetic as S
    sd = S.synthetic_state_dict(template, seed=seed, cls_bias=-1.0)
    for n in trunk_norms(sd):
        sd[n + ".bias"] = sd[n + ".bias"].clone()
        sd[n + ".bias"][::4] = -BETA_SHIFT
    return sd


def features(batch=B, h=H, w=W, seed=SEEDS["x_seed"]):
    """(batch, 64, h, w) fp32, post-ReLU like the backbone's output."""
    return torch.randn(batch, 64, h, w, generator=torch.Generator().manual_seed(seed)).relu()


def edge_targets(w=W, h=H, orig_sizes=ORIG_SIZES):
    """One test-split target dict per image (monoflex_amd.synthetic.synthetic_target) + stacked (edge_indices int64 (B, L, 2), edge_len int64 (B,))."""
    from monoflex_amd import synthetic as S
    tg = [S.synthetic_target(w, h, orig_size=o) for o in orig_sizes]
    ei = torch.stack([torch.as_tensor(t["edge_indices"]) for t in tg]).long()
    el = torch.tensor([int(t["edge_len"]) for t in tg]).long()
    return tg, ei, el


def loss_weights(ncls, R, batch=B, h=H, w=W, seed=SEEDS["loss_seed"]):
    """The fixed linear loss of the golden's training step: sum(cls * g_cls) + sum(reg * g_reg)."""
    g = torch.Generator().manual_seed(seed)
    return torch.randn(batch, ncls, h, w, generator=g), torch.randn(batch, R, h, w, generator=g)


def pixel_subset(h=H, w=W):
    return torch.arange(0, h * w, SUBSET)


class HeadActRef:
    """float64 statement of the predictor.  `sd`: the predictor's state dict (either form: the last class layer is class_head.3 or .2);
    `slope`: the trunk activation below zero.  forward() returns the class LOGITS and the regression maps after the edge fusion (NCHW); in
    train mode the norms use batch statistics and `self.running` holds the updated running statistics afterwards.  Parameters are leaves
    of `self.p` (requires_grad as asked), so that torch.autograd gives every gradient."""

    def __init__(self, sd, cfg, slope=0.0, requires_grad=False):
        self.p = {}
        for k, v in sd.items():
            t = v.detach().cpu().double().clone()
            if requires_grad and v.is_floating_point() and not k.endswith(("running_mean", "running_var")):
                t.requires_grad_()
            self.p[k] = t
        self.slope = slope
        self.last = 3 if "class_head.3.weight" in sd else 2
        self.heads = [list(h) for h in cfg.MODEL.HEAD.REGRESSION_HEADS]
        self.channels = [list(c) for c in cfg.MODEL.HEAD.REGRESSION_CHANNELS]
        self.offset_index = [(i, j) for i, hs in enumerate(self.heads) for j, k in enumerate(hs) if k == '3d_offset'][0]
        self.edge_fusion = bool(cfg.MODEL.HEAD.ENABLE_EDGE_FUSION)
        self.edge_relu = bool(cfg.MODEL.HEAD.EDGE_FUSION_RELU)
        self.momentum = float(cfg.MODEL.HEAD.BN_MOMENTUM)
        self.eps = 1e-5
        self.running, self.acts, self.pre = {}, {}, {}      # after forward(): updated running statistics, trunk activations, their pre-activations

    def _bn(self, y, name, train, dims):
        p = self.p
        shape = [1, -1] + [1] * (y.dim() - 2)
        if train:
            mean, var = y.mean(dims), y.var(dims, unbiased=False)
            n = y.numel() // y.shape[1]
            with torch.no_grad():
                self.running[name + ".running_mean"] = p[name + ".running_mean"] + self.momentum * (mean - p[name + ".running_mean"])
                self.running[name + ".running_var"] = p[name + ".running_var"] + self.momentum * (var * n / (n - 1) - p[name + ".running_var"])
        else:
            mean, var = p[name + ".running_mean"], p[name + ".running_var"]
        return (y - mean.view(shape)) * torch.rsqrt(var + self.eps).view(shape) * p[name + ".weight"].view(shape) + p[name + ".bias"].view(shape)

    def _trunk(self, x, prefix, train):
        z = self._bn(F.conv2d(x, self.p[prefix + ".0.weight"], None, padding=1), prefix + ".1", train, (0, 2, 3))
        a = F.leaky_relu(z, self.slope)
        self.acts[prefix], self.pre[prefix] = a.detach(), z.detach()
        return a

    def _edge(self, e, prefix, train):
        """(B, 256, L) -> Conv1d k3 (replicate padding over the whole padded sequence) -> BN1d -> [ReLU] -> Conv1d 1x1."""
        p = self.p
        y = F.conv1d(F.pad(e, (1, 1), mode="replicate"), p[prefix + ".0.weight"], p[prefix + ".0.bias"])
        y = self._bn(y, prefix + ".1", train, (0, 2))
        if self.edge_relu:
            y = y.relu()
        return F.conv1d(y, p[prefix + ".3.weight"], p[prefix + ".3.bias"])

    def forward(self, x, edge_indices=None, edge_lens=None, train=False):
        p = self.p
        x = x.double() if x.dtype != torch.float64 else x
        f_cls = self._trunk(x, "class_head", train)
        cls = F.conv2d(f_cls, p["class_head.%d.weight" % self.last], p["class_head.%d.bias" % self.last])
        regs, f_off = [], None
        for i, keys in enumerate(self.heads):
            f = self._trunk(x, "reg_features.%d" % i, train)
            if i == self.offset_index[0]:
                f_off = f
            regs.append([F.conv2d(f, p["reg_heads.%d.%d.weight" % (i, j)], p["reg_heads.%d.%d.bias" % (i, j)]) for j in range(len(keys))])
        if self.edge_fusion:
            oi, oj = self.offset_index
            xs, ys = edge_indices[..., 0].long(), edge_indices[..., 1].long()
            bidx = torch.arange(x.shape[0]).view(-1, 1).expand_as(xs)
            o_cls = self._edge(f_cls[bidx, :, ys, xs].permute(0, 2, 1), "trunc_heatmap_conv", train)      # grid_sample at integer points
            o_off = self._edge(f_off[bidx, :, ys, xs].permute(0, 2, 1), "trunc_offset_conv", train)
            valid = (torch.arange(xs.shape[1]).view(1, -1) < edge_lens.view(-1, 1)).to(x.dtype)           # the valid border pixels are unique
            for o, which in ((o_cls, "cls"), (o_off, "off")):
                add = torch.zeros(x.shape[0], x.shape[2], x.shape[3], o.shape[1], dtype=x.dtype)
                add = add.index_put((bidx, ys, xs), o.permute(0, 2, 1) * valid.unsqueeze(-1), accumulate=True).permute(0, 3, 1, 2)
                if which == "cls":
                    cls = cls + add
                else:
                    regs[oi][oj] = regs[oi][oj] + add
        return cls, torch.cat([r for group in regs for r in group], dim=1)

    @staticmethod
    def sigmoid_hm(logits):
        """The reference's 'cls' output (model/layers/utils.py sigmoid_hm)."""
        return torch.sigmoid(logits).clamp(min=1e-4, max=1 - 1e-4)

    def grads(self):
        return {k: v.grad for k, v in self.p.items() if v.requires_grad and v.grad is not None}


def object_rows(edge_indices, edge_lens, n_per_image, batch=B, h=H, w=W, seed=17):
    """An object table as the loss packs it (fp32 [batch * n_per_image, 72]: column 0 the valid flag, 57 the image, 2 / 3 the centre x / y):
    every third slot empty, two objects on one pixel, and one centre on a valid border pixel of image 0 (it receives the fused edge output)."""
    g = torch.Generator().manual_seed(seed)
    N = batch * n_per_image
    rows = torch.zeros(N, 72)
    rows[:, 57] = torch.arange(N).div(n_per_image, rounding_mode="floor").float()
    rows[:, 2] = torch.randint(1, w - 1, (N,), generator=g).float()
    rows[:, 3] = torch.randint(1, h - 1, (N,), generator=g).float()
    rows[:, 0] = (torch.arange(N) % 3 != 2).float()
    rows[4, 2:4] = rows[1, 2:4]                                           # two objects, one pixel
    k = int(edge_lens[0]) // 2
    rows[0, 2], rows[0, 3] = float(edge_indices[0, k, 0]), float(edge_indices[0, k, 1])
    assert rows[0, 0] == 1 and rows[1, 0] == 1 and rows[4, 0] == 1
    return rows
