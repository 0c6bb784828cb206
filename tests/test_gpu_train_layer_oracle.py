"""Node-by-node oracle walk of the backbone of the benchmarked training step (bench.py --mode train: B = 8 per GPU, 1280x384, bf16 and fp16
under the loss scaler), with its BN buffers, its AdamW step and its dispatch counts.

Setup = bench.run_train's first batch: bench.build_model(train=True) with log_as_float off, seed parallel.shard_seed(1000, 0, 8), synthetic images,
make_train_target(synthetic_train_target(seed + i)) through prepare_targets, build_optimizer(capturable=True), LossScaler.for_model for fp16.  ONE
eager engine.trainer.train_step runs in its production configuration (non-deterministic, RESIDUAL_ALIAS on, Gram heads, fused losses, the one-launch
AdamW) with `apply` of every autograd Function wrapped.  Per call of a checked Function the wrapper keeps the inputs, the outputs, the gradient
that arrived at each output and the gradient each activation input received FROM THIS NODE (activations are re-viewed, as in
test_gpu_train_fullsize.Recorder; parameters are passed unchanged -- a view of a parameter would change how its operand is packed -- and a
parameter's gradient is read from p.grad where exactly one node consumes it, or from the hooked view where a node takes weight.unsqueeze(2)).

Reference: Conv2dFn (plain, statistics and alias forms), BNActFn, CatConv1x1Fn (Root), StemConvFn, MaxPool2x2Fn, UpsampleAddFn and DCNModuleFn are
restated in float64 with plain torch ops on the GPU, teacher-forced on the recorded inputs, from the fp32 parameters (never the library's packs);
the recorded output gradient is back-propagated through the restatement.  Train-mode BN takes the batch statistics.  The DCN samples bilinearly
(zeros outside the map, the arithmetic of tests/test_gpu_layer_oracle._dcn64) at the offsets / mask the kernel used (read from the node), with the
derivative of the float64 offset conv behind them (straight-through); a sample coordinate takes the kernel's fp32 value, because the derivative of
bilinear sampling jumps at integral coordinates.  Conv2dFn covers the prediction heads' plain convs and the edge fusion's 1 x 3 / 1 x 1 convs too.

Error model, per element: |got - ref| <= k * (u_op * M + u_out * |ref|), M = the same expression on absolute values (|x|, |w|, |dy|; BN forward
|gamma| (|x| + |mean|) rstd + |beta| (+ |res|); BN backward |gamma| rstd (|g| + |mean g| + |xhat| |mean(g xhat)|), g = dy times the activation's
derivative; DCN: the sampling of |x| with |w| and |dy|, plus the offset conv's |x|, |w_off| and the float64 |d offset / mask|).  u_op / u_out =
2^-8 / 2^-9 (bf16) and 2^-11 (fp16); fp16 outputs add half a subnormal spacing.  ReLU / leaky masks: elements whose float64 pre-activation lies
within its own bound of zero may take either side in the backward (it recomputes the pre-activation in fp32): their number is counted and bounded
(AMB_FRAC), the element takes the nearer side, and every sum gets exactly the slack such elements can move it by.  Elements whose forward side
differs from float64 must lie within that bound too.  k is ~2x the worst value observed on MI355X (train_layer_oracle_<mode>.json under
$MFX_REPORT_DIR, default: the git-ignored artifacts/).

Whole step: p.grad of every single-consumer parameter of a checked node (the accumulation of autograd, the _SumArena bias sums, the alias
residual), BN running_mean / running_var (unbiased) / num_batches_tracked, AdamW (parameters, exp_avg, exp_avg_sq, step) against a float64
decoupled-weight-decay AdamW from the recorded gradients, the one-pass BN stuck flag, the exact number of calls per Function and the exact per-family
dispatch counter deltas (a GraphedTrainStep on the same state then launches the same families per step).  Teeth: deliberately wrong references
must miss by at least 2x: (a) a DCN input gradient without its far-corner samples, (b) a weight gradient without one image, (c) running_var with
the biased variance, (d) AdamW with L2 instead of decoupled weight decay.

Not restated here, only counted (calls and dispatch families): the heads' fused nodes (FanOutConvFn, HeadConvGatherFn, EdgeScatterAddFn,
GramRegHeadsHipFn) and the fused focal / object losses; so neither is the gradient they hand the backbone's output, nor p.grad of the parameters they
consume.  GramRegHeadsHipFn has its own float64 reference at small shapes: tests/test_gpu_gram_heads_oracle.py (tests/gram_heads_ref.py); so have
FanOutConvFn, HeadConvGatherFn and EdgeScatterAddFn: tests/test_gpu_head_nodes.py (tests/head_nodes_ref.py), with derived bounds at the production
channel counts."""
import json
import os
import time

import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
REPORT_DIR = os.environ.get("MFX_REPORT_DIR") or os.path.join(ROOT, "artifacts")
B = 8
D64 = torch.float64
U = {"bf16": (2.0 ** -8, 2.0 ** -9), "fp16": (2.0 ** -11, 2.0 ** -11)}
ETA = {"bf16": 0.0, "fp16": 2.0 ** -25}     # absolute rounding floor of a 16-bit output: half of fp16's subnormal spacing (bf16's is below 1e-40)
U32 = 2.0 ** -24
COUNTERS = ("wgrad_patch", "wgrad_tr", "wgrad_mfma", "wgrad_valu", "wgrad_reduce", "stem_wgrad", "bn_fwd_onepass", "bn_bwd_onepass", "bn_fwd_two",
            "bn_bwd_two", "conv_bn_stats", "dcn_bt_tile", "dcn_bt_sample", "dcn_bt_far", "dcn_bt_fused", "dcn_bt_fly", "gram", "adamw_multi")
CHECKED = ("Conv2dFn", "BNActFn", "CatConv1x1Fn", "StemConvFn", "MaxPool2x2Fn", "UpsampleAddFn", "DCNModuleFn")
COUNTED = ("DCNFn", "FanOutConvFn", "HeadConvGatherFn", "EdgeScatterAddFn", "SparseRegHeadsFn", "FocalLossFn", "ObjectLossFn")
GRAM = ("GramRegHeadsHipFn", "GramRegHeadsFn")
# per-family dispatch counts of one step (eager and graphed alike), from the dispatch code (conv_wgrad_impl, mfx_bn_train_fwd / _bwd and
# bn_onepass_plan, dcn_backward_v2_impl, mfx_gram_heads phases), cross-checked with profiles/r06_a_train_replay_kernel_timeline.md
STEP_COUNTS = {
    "bf16": {"wgrad_patch": 38, "wgrad_tr": 10, "wgrad_mfma": 37, "wgrad_valu": 0, "wgrad_reduce": 73, "stem_wgrad": 1, "bn_fwd_onepass": 12,
             "bn_bwd_onepass": 42, "bn_fwd_two": 44, "bn_bwd_two": 14, "conv_bn_stats": 14, "dcn_bt_tile": 11, "dcn_bt_sample": 11,
             "dcn_bt_far": 16, "dcn_bt_fused": 5, "dcn_bt_fly": 5, "gram": 8, "adamw_multi": 1},
}
STEP_COUNTS["fp16"] = dict(STEP_COUNTS["bf16"])
# calls per Function in one step: 30 backbone conv + BN pairs (level0 / level1, 24 block convs, 4 projections) and 4 head convs, 6 Roots, 16 DCN
# modules (each with its BN) ... -- every autograd node of the step; a dispatch change has to update this on purpose
CALLS = {"Conv2dFn": 34, "BNActFn": 56, "CatConv1x1Fn": 6, "StemConvFn": 1, "MaxPool2x2Fn": 4, "UpsampleAddFn": 8, "DCNModuleFn": 16,
         "DCNFn": 0, "FanOutConvFn": 1, "HeadConvGatherFn": 1, "EdgeScatterAddFn": 1, "SparseRegHeadsFn": 0, "FocalLossFn": 1,
         "ObjectLossFn": 1, "GramRegHeadsHipFn": 1, "GramRegHeadsFn": 0}
# k per (node family, quantity): the bound on max |err| / (u_op M + u_out |ref| + eta), ~2x the worst value observed on MI355X (rounded up;
# at least 0.02; fp16 conv d weight 0.05: the fp32 sums over the edge fusion's rows, observed 0.023).  Parameter-gradient rows sit far below 1: their operands are exact in the activation type and only fp32 accumulation
# remains.  The conv family includes the heads' convs and the edge fusion's 1 x 3 / 1 x 1 convs.
K = {
    'bf16': {('bn', 'd beta'): 0.02, ('bn', 'd gamma'): 0.02, ('bn', 'd input'): 1.4, ('bn', 'd residual'): 0.02, ('bn', 'forward'): 1.4,
             ('conv', 'd bias'): 0.02, ('conv', 'd input'): 2.2, ('conv', 'd weight'): 0.02, ('conv', 'forward'): 1.4, ('dcn', 'd bias'): 0.02,
             ('dcn', 'd input'): 1.9, ('dcn', 'd offset bias'): 0.14, ('dcn', 'd offset weight'): 0.74, ('dcn', 'd weight'): 0.66,
             ('dcn', 'forward'): 0.79, ('dcn', 'mask'): 0.29, ('dcn', 'offsets'): 0.36, ('root', 'd input0'): 1.9, ('root', 'd input1'): 1.8,
             ('root', 'd input2'): 1.3, ('root', 'd input3'): 1.4, ('root', 'd weight'): 0.02, ('root', 'forward'): 1.3,
             ('stem', 'd weight'): 0.02, ('stem', 'forward'): 1.3, ('up_add', 'd input'): 1.4, ('up_add', 'd skip'): 0.02,
             ('up_add', 'd weight'): 0.02, ('up_add', 'forward'): 1.4},
    'fp16': {('bn', 'd beta'): 0.02, ('bn', 'd gamma'): 0.036, ('bn', 'd input'): 2.0, ('bn', 'd residual'): 0.02, ('bn', 'forward'): 1.0,
             ('conv', 'd bias'): 0.02, ('conv', 'd input'): 1.7, ('conv', 'd weight'): 0.05, ('conv', 'forward'): 1.2, ('dcn', 'd bias'): 0.02,
             ('dcn', 'd input'): 1.7, ('dcn', 'd offset bias'): 0.15, ('dcn', 'd offset weight'): 0.54, ('dcn', 'd weight'): 0.52,
             ('dcn', 'forward'): 1.3, ('dcn', 'mask'): 0.27, ('dcn', 'offsets'): 0.35, ('root', 'd input0'): 1.5, ('root', 'd input1'): 1.4,
             ('root', 'd input2'): 1.2, ('root', 'd input3'): 1.3, ('root', 'd weight'): 0.02, ('root', 'forward'): 1.0,
             ('stem', 'd weight'): 0.02, ('stem', 'forward'): 0.97, ('up_add', 'd input'): 1.0, ('up_add', 'd skip'): 0.02,
             ('up_add', 'd weight'): 0.02, ('up_add', 'forward'): 2.0},
}
K_DEFAULT = 0.0               # (a family / quantity without an entry has no bound yet: it fails until one is measured)
K_RUNNING = 24.0              # running statistics, in units of 2^-24 of their magnitude (observed 6.7 bf16, 10.9 fp16)
K_ADAMW = 40.0                # AdamW, in units of 2^-24 (observed 17.9: exp_avg_sq)
# at most this fraction of a BN's elements may lie within their own bound of zero (either activation side allowed in the backward, with the exact
# slack of that choice in every sum); observed at most 0.95 % (bf16) and 0.08 % (fp16) of a layer
AMB_FRAC = {"bf16": 0.02, "fp16": 0.002}
MASK_FLIP_FRAC = 1e-4         # at most this fraction of a BN's elements may take the other side of the activation (each within its bound)


def _k(mode, fam, q):
    return K[mode].get((fam, q), K_DEFAULT)


def _n64(t):
    """NHWC -> NCHW float64 (4-D); anything else: float64."""
    t = t.detach()
    return t.permute(0, 3, 1, 2).to(D64) if t.dim() == 4 else t.to(D64)


def _param_of(t):
    """The parameter a tensor argument is, or is a view of (None otherwise)."""
    if not torch.is_tensor(t):
        return None
    if isinstance(t, torch.nn.Parameter):
        return t
    return t._base if isinstance(t._base, torch.nn.Parameter) else None


def _leaf(t):
    return t.detach().clone().requires_grad_()


def _grads(outs, ins, gouts):
    gs = torch.autograd.grad(outs, ins, gouts, allow_unused=True)
    return [g if g is not None else torch.zeros_like(i) for g, i in zip(gs, ins)]


def _score(got, ref, mag, uop, uout, eta=0.0, slack=None):
    """Ratios |got - ref| / (u_op M + u_out |ref| + eta) per element and their summary (max, mean, border band of the outer 2 rows / columns,
    worst channel's mean).  `slack`: what elements that may take either side of an activation can move, taken off |got - ref| first."""
    got, ref = got.to(D64), ref.to(D64)
    d = (got - ref).abs()
    if slack is not None:
        d = (d - slack).clamp(min=0)
    den = uop * mag + uout * ref.abs() + eta
    ratio = torch.where(d == 0, torch.zeros_like(d), d / den.clamp(min=1e-300))
    out = dict(max=float(ratio.max()), mean=float(ratio.mean()),
               rel_l2=float(d.norm() / ref.norm().clamp(min=1e-300)))
    if ratio.dim() == 4 and ratio.shape[2] > 4 and ratio.shape[3] > 4:
        band = torch.zeros(ratio.shape[2:], dtype=torch.bool, device=ratio.device)
        band[:2], band[-2:], band[:, :2], band[:, -2:] = True, True, True, True
        out["border_max"] = float(ratio[:, :, band].max())
        out["chan_mean"] = float(ratio.mean(dim=(0, 2, 3)).max())
    elif ratio.dim() >= 2:
        out["chan_mean"] = float(ratio.transpose(0, 1).reshape(ratio.shape[1], -1).mean(1).max()) if ratio.dim() > 1 else out["mean"]
    return out


def _bilinear(x, py, px):
    """Bilinear sample of x (B,C,H,W) at (py, px) (B,H,W), corners outside the map count zero (DCNv2's im2col / col2im; grid_sample's
    zeros padding with align_corners).  Written out instead of grid_sample so that the corner pair a coordinate's derivative takes is the
    floor of the coordinate itself: grid_sample's normalise / unnormalise round trip can move an integral coordinate below its integer."""
    Bn, C, H, W = x.shape
    y0, x0 = torch.floor(py.detach()), torch.floor(px.detach())
    fy, fx = py - y0, px - x0
    xf = x.reshape(Bn, C, H * W)
    out = 0
    for dy, wy in ((0, 1 - fy), (1, fy)):
        for dx, wx in ((0, 1 - fx), (1, fx)):
            yy, xx = y0 + dy, x0 + dx
            ok = ((yy >= 0) & (yy < H) & (xx >= 0) & (xx < W)).to(x.dtype)
            idx = (yy.clamp(0, H - 1) * W + xx.clamp(0, W - 1)).long().view(Bn, 1, -1).expand(Bn, C, -1)
            out = out + torch.gather(xf, 2, idx).view(Bn, C, H, W) * (wy * wx * ok).unsqueeze(1)
    return out


def _dcn64(x, off, msk, w):
    """Modulated deformable 3x3 / stride 1 / pad 1 in float64 (the arithmetic of tests/test_gpu_layer_oracle._dcn64).  The sample coordinates
    take the kernel's value -- (y + i - 1) + offset rounded once to fp32 -- with the float64 derivative: the derivative of bilinear sampling
    jumps at integral coordinates, so a coordinate within an fp32 rounding of an integer must fall on the kernel's side of it."""
    Bn, C, H, W = x.shape
    ys, xs = torch.meshgrid(torch.arange(H, dtype=D64, device=x.device), torch.arange(W, dtype=D64, device=x.device), indexing="ij")
    out = 0
    for k in range(9):
        i, j = divmod(k, 3)
        py = ys + (i - 1) + off[:, 2 * k]
        px = xs + (j - 1) + off[:, 2 * k + 1]
        py = py + (py.detach().float().to(D64) - py.detach())
        px = px + (px.detach().float().to(D64) - px.detach())
        smp = _bilinear(x, py, px) * msk[:, k:k + 1]
        out = out + torch.einsum("oc,bchw->bohw", w[:, :, i, j], smp)
    return out


def _far_taps(off):
    """(B,9,H,W) bool: the samples of which a bilinear corner lies outside the DCN backward's candidate window of the output pixel's tile
    (dcn_bwd_tile.hip: 8 x 16 tiles, a ring of BT_D_VAL = 8 pixels) -- the corners the far-corner kernels add."""
    Bn, _, H, W = off.shape
    dev = off.device
    ys = torch.arange(H, device=dev, dtype=D64).view(1, H, 1)
    xs = torch.arange(W, device=dev, dtype=D64).view(1, 1, W)
    ty0, tx0 = torch.div(ys, 8, rounding_mode="floor") * 8, torch.div(xs, 16, rounding_mode="floor") * 16
    far = []
    for k in range(9):
        i, j = divmod(k, 3)
        y0 = torch.floor(ys + (i - 1) + off[:, 2 * k])
        x0 = torch.floor(xs + (j - 1) + off[:, 2 * k + 1])
        near = (y0 >= ty0 - 8) & (y0 + 1 < ty0 + 16) & (x0 >= tx0 - 8) & (x0 + 1 < tx0 + 24)
        far.append(~near)
    return torch.stack(far, 1)


class _Walk:
    def __init__(self, mode, model, lib, scale):
        self.mode, self.model, self.lib, self.scale = mode, model, lib, scale
        self.uop, self.uout = U[mode]
        self.recs, self.calls, self.rows, self.teeth, self.fail = [], {}, [], [], []
        self.names = {id(p): n for n, p in model.named_parameters()}
        self.param_uses = {}
        self.bn_ref = {}                     # id(running_mean) -> (rm ref, rv ref, magnitudes, M, momentum, biased var) for the buffer check
        self.mask_flips = 0
        self.nonfinite = 0
        self.applied = True
        self.far_samples = 0
        self.amb_count = 0
        self.amb_worst = 0.0
        self.tooth_c_M = None                  # rows of the BN that carries tooth (c): the smallest one (the biased variance differs most there)
        self.adamw_worst = {}                  # (family, quantity) -> (worst ratio, parameter name)
        self.tooth_d = (0.0, "")               # (d): the worst miss of an L2-weight-decay AdamW, and where

    # ---- recording -------------------------------------------------------------------------------------------------------------
    def wrap(self, cls, name):
        orig = cls.apply

        def run(*args):
            self.calls[name] = self.calls.get(name, 0) + 1
            for a in args:
                if isinstance(a, torch.nn.Parameter):
                    self.param_uses[id(a)] = self.param_uses.get(id(a), 0) + 1
            if name not in CHECKED:
                return orig(*args)
            rec = dict(kind=name, gin={}, gout={})
            a2 = list(args)
            for i, a in enumerate(args):
                if torch.is_tensor(a) and a.requires_grad and not isinstance(a, torch.nn.Parameter):
                    v = a.view_as(a)
                    v.register_hook(lambda g, i=i: rec["gin"].__setitem__(i, g.detach().clone()))
                    a2[i] = v
            # the values at this call: parameters and views of parameters (the edge fusion's weight.unsqueeze(2)) are copied -- AdamW changes
            # them in place after the backward --, so is every tensor below 4 M elements (row buffers); the large activation maps are kept
            rec["args"] = [(a.detach().clone() if (_param_of(a) is not None or a.numel() < (1 << 22)) else a.detach())
                           if torch.is_tensor(a) else a for a in args]
            rec["params"] = {i: a for i, a in enumerate(args) if isinstance(a, torch.nn.Parameter)}
            rec["views"] = {i: _param_of(a) for i, a in enumerate(args) if _param_of(a) is not None and not isinstance(a, torch.nn.Parameter)}
            rec["ids"] = [id(a) for a in args]
            out = orig(*a2)
            outs = out if isinstance(out, tuple) else (out,)
            rec["out"] = [o.detach() if torch.is_tensor(o) else o for o in outs]
            for j, o in enumerate(outs):
                if torch.is_tensor(o) and o.requires_grad:
                    o.register_hook(lambda g, j=j: rec["gout"].__setitem__(j, g.detach().clone()))
            if name == "DCNModuleFn":
                rec["om"] = outs[0].grad_fn.saved_tensors[1].detach()       # offsets | sigmoid(mask) the kernel sampled with
            self.recs.append(rec)
            return out
        return run

    # ---- judging ---------------------------------------------------------------------------------------------------------------
    def judge(self, node, fam, q, got, ref, mag, slack=None):
        if not (bool(torch.isfinite(ref).all()) and (mag is None or bool(torch.isfinite(mag).all()))) or \
                not (self.applied or bool(torch.isfinite(got).all())):
            self.nonfinite += 1                                  # (fp16: an overflowed gradient -- the loss scaler skips this step)
            return None
        s = _score(got, ref, mag, self.uop, self.uout, ETA[self.mode], slack)
        k = _k(self.mode, fam, q)
        self.rows.append(dict(node=node, family=fam, quantity=q, bound=k, **s))
        if not s["max"] <= k or not s["max"] == s["max"]:
            self.fail.append((node, q, s["max"], k))
        return s

    def tooth(self, name, fam, q, got, ref, mag):
        """A deliberately wrong reference; per case letter the strongest instance is kept."""
        if not (bool(torch.isfinite(ref).all()) and bool(torch.isfinite(got).all())):
            return
        s = _score(got, ref, mag, self.uop, self.uout, ETA[self.mode])
        old = [t for t in self.teeth if t["case"][:3] == name[:3]]
        if old and old[0]["observed"] >= s["max"]:
            return
        self.teeth = [t for t in self.teeth if t["case"][:3] != name[:3]]
        self.teeth.append(dict(case=name, observed=s["max"], bound=_k(self.mode, fam, q)))

    def param_grad(self, rec, idx):
        """The gradient this node's parameter input received (p.grad in the scaled domain), or None when other nodes feed it too."""
        p = rec["params"].get(idx)
        if p is None or p.grad is None or self.param_uses.get(id(p), 0) != 1:
            return None
        return p.grad.detach().to(D64) * self.scale

    def pname(self, rec, idx):
        p = rec["params"].get(idx)
        return self.names.get(id(p), "?") if p is not None else "?"

    # ---- references ------------------------------------------------------------------------------------------------------------
    def Conv2dFn(self, rec, n):
        from monoflex_amd import lib as L
        a = rec["args"]
        x, w, b, stride, pad = a[0], a[1], a[2], a[3], a[4]
        act = a[6] if len(a) > 6 else L.ACT_NONE
        alias = len(a) > 8 and bool(a[8])
        if act != L.ACT_NONE:
            return "skipped"
        Cout = w.shape[0]
        fam = "conv"
        wp = rec["params"].get(1, rec["views"].get(1))                # (the edge fusion's 1 x 3 / 1 x 1 convs take weight.unsqueeze(2))
        name = "conv[%s]" % (self.names.get(id(wp), "?") if wp is not None else "?")
        y = rec["out"][0][..., :Cout]
        x64, w64 = _leaf(_n64(x)), _leaf(w.to(D64))
        b64 = _leaf(b.to(D64)) if b is not None else None
        ins = [x64, w64] + ([b64] if b64 is not None else [])
        yr = F.conv2d(x64, w64, b64, stride, pad)
        xa, wa = _leaf(x64.abs()), _leaf(w64.abs())
        ba = _leaf(b64.abs()) if b64 is not None else None
        insa = [xa, wa] + ([ba] if ba is not None else [])
        ya = F.conv2d(xa, wa, ba, stride, pad)
        self.judge(name, fam, "forward", _n64(y), yr.detach(), ya.detach())
        if 0 not in rec["gout"]:
            return "no-grad"
        gy = rec["gout"][0][..., :Cout]
        if gy.dtype != x.dtype:                                        # an fp32 output: the backward rounds dy to the operand type first
            gy = gy.to(x.dtype)
        gy = _n64(gy.contiguous())
        gr = _grads(yr, ins, gy)
        ga = _grads(ya, insa, gy.abs())
        if alias and 1 in rec["gout"]:
            gal = _n64(rec["gout"][1])
            gr[0] = gr[0] + gal
            ga[0] = ga[0] + gal.abs()
        if 0 in rec["gin"]:
            self.judge(name, fam, "d input", _n64(rec["gin"][0]), gr[0], ga[0])
        pw = self.param_grad(rec, 1)
        if pw is None and 1 in rec["gin"]:                             # a view of a parameter: the gradient this node gave the view
            pw = rec["gin"][1].detach().to(D64)
        if pw is not None:
            self.judge(name, fam, "d weight", pw, gr[1], ga[1])
            if stride == 1 and w.shape[2] == 3 and gy.shape[0] == B:      # (b) the weight gradient with image 0's pixels left out
                gy0 = gy.clone()
                gy0[0] = 0
                self.tooth("(b) %s d weight without image 0" % name, "conv", "d weight", pw, _grads(F.conv2d(x64, w64, b64, stride, pad), [w64], gy0)[0], ga[1])
        if b64 is not None:
            pb = self.param_grad(rec, 2)
            if pb is not None:
                self.judge(name, fam, "d bias", pb, gr[2], ga[2])
        return "ok"

    def BNActFn(self, rec, n):
        from monoflex_amd import lib as L
        a = rec["args"]
        x, gamma, beta, rm, rv, res, act, mom, eps = a[:9]
        name = "bn[%s]" % self.pname(rec, 1)
        x64 = _leaf(_n64(x))
        g64, b64 = _leaf(gamma.to(D64)), _leaf(beta.to(D64))
        r64 = _leaf(_n64(res)) if res is not None else None
        C = x64.shape[1]
        red = [0] + list(range(2, x64.dim()))
        shp = [1, C] + [1] * (x64.dim() - 2)
        M = x64.numel() // C
        mean = x64.mean(dim=red, keepdim=True)
        var = x64.var(dim=red, unbiased=False, keepdim=True)
        rstd = (var + eps).rsqrt()
        xh = (x64 - mean) * rstd
        z = g64.view(shp) * xh + b64.view(shp)
        if r64 is not None:
            z = z + r64
        mz = (g64.detach().abs().view(shp) * (x64.detach().abs() + mean.detach().abs()) * rstd.detach() + b64.detach().abs().view(shp))
        if r64 is not None:
            mz = mz + r64.detach().abs()
        slope = 0.0 if act == L.ACT_RELU else 0.01 if act == L.ACT_LEAKY else 1.0
        yk = _n64(rec["out"][0])
        zd = z.detach()
        if act in (L.ACT_RELU, L.ACT_LEAKY):
            # the kernel's side: its output's, except that without a residual the backward recomputes the pre-activation from x, so an
            # fp16 output that rounded a tiny positive value to zero still passes the gradient
            pos_k = (yk > 0) | ((yk == 0) & (zd > 0) & (r64 is None))
            flips = pos_k != (zd > 0)
            nflip = int(flips.sum())
            self.mask_flips += nflip
            zb = _k(self.mode, "bn", "forward") * (self.uop * mz + self.uout * zd.abs())
            if nflip and not bool((zd[flips].abs() <= zb[flips]).all()):
                self.fail.append((name, "activation side beyond the bound", nflip))
            if nflip > max(8, MASK_FLIP_FRAC * zd.numel()):
                self.fail.append((name, "activation side flips", nflip))
            dact = torch.where(pos_k, torch.ones_like(zd), torch.full_like(zd, slope))
            yr = torch.where(zd > 0, z, z * slope)
            # elements within their own bound of zero may take either side in the backward (it recomputes the pre-activation in fp32)
            amb = zd.abs() <= zb
            namb = int(amb.sum())
            self.amb_count += namb
            self.amb_worst = max(self.amb_worst, namb / zd.numel())
            if namb > AMB_FRAC[self.mode] * zd.numel():
                self.fail.append((name, "elements within their bound of zero", namb, zd.numel()))
        else:
            dact = torch.ones_like(zd)
            yr = z
            pos_k = amb = torch.zeros_like(zd, dtype=torch.bool)
        self.judge(name, "bn", "forward", yk, yr.detach(), mz)
        # running statistics after the step (checked once the step is over)
        varu = x64.detach().var(dim=red, unbiased=True).view(-1)
        self.bn_ref[rec["ids"][3]] = dict(name=name, mean=mean.detach().view(-1), var_u=varu, var_b=var.detach().view(-1), mom=float(mom), M=M,
                                   absmean=x64.detach().abs().mean(dim=red).view(-1), sq=(x64.detach() ** 2).mean(dim=red).view(-1))
        if 0 not in rec["gout"]:
            return "no-grad"
        gy = _n64(rec["gout"][0])
        gg = gy * dact
        ins = [x64, g64, b64] + ([r64] if r64 is not None else [])
        # the backward of the float64 restatement with the kernel's activation side (teacher-forced mask)
        gr = _grads(z, ins, gg)
        ag = gg.abs()
        xhd = xh.detach()
        mg = gg.mean(dim=red, keepdim=True).abs()
        mgx = (gg * xhd).mean(dim=red, keepdim=True).abs()
        mdx = g64.detach().abs().view(shp) * rstd.detach() * (ag + mg + xhd.abs() * mgx)
        # the other side of an ambiguous element: its own term changes by gamma rstd dy (1 - slope), every sum by dy (1 - slope) (x xhat)
        da_amb = (gy.abs() * amb * (1 - slope))
        s1 = da_amb.sum(dim=red, keepdim=True)
        s2 = (da_amb * xhd.abs()).sum(dim=red, keepdim=True)
        slack_dx = g64.detach().abs().view(shp) * rstd.detach() * (s1 + xhd.abs() * s2) / M
        if 0 in rec["gin"]:
            dxk = _n64(rec["gin"][0])
            alt = gr[0] + torch.where(pos_k, -1.0, 1.0) * g64.detach().view(shp) * rstd.detach() * gy * (1 - slope)
            ref_dx = torch.where(amb & ((dxk - alt).abs() < (dxk - gr[0]).abs()), alt, gr[0])
            self.judge(name, "bn", "d input", dxk, ref_dx, mdx, slack=slack_dx)
        if r64 is not None and 5 in rec["gin"]:
            self.judge(name, "bn", "d residual", _n64(rec["gin"][5]), gr[3], ag)
        pg, pb = self.param_grad(rec, 1), self.param_grad(rec, 2)
        if pg is not None:
            self.judge(name, "bn", "d gamma", pg, gr[1], (ag * xhd.abs()).sum(dim=red), slack=s2.view(-1))
        if pb is not None:
            self.judge(name, "bn", "d beta", pb, gr[2], ag.sum(dim=red), slack=s1.view(-1))
        return "ok"

    def CatConv1x1Fn(self, rec, n):
        a = rec["args"]
        w, xs = a[0], a[1:]
        name = "root[%s]" % self.pname(rec, 0)
        x64 = [_leaf(_n64(t)) for t in xs]
        w64 = _leaf(w.to(D64))
        yr = F.conv2d(torch.cat(x64, 1), w64)
        xa = [_leaf(t.abs()) for t in x64]
        wa = _leaf(w64.abs())
        ya = F.conv2d(torch.cat(xa, 1), wa)
        self.judge(name, "root", "forward", _n64(rec["out"][0]), yr.detach(), ya.detach())
        if 0 not in rec["gout"]:
            return "no-grad"
        gy = _n64(rec["gout"][0])
        gr = _grads(yr, x64 + [w64], gy)
        ga = _grads(ya, xa + [wa], gy.abs())
        for i in range(len(xs)):
            if 1 + i in rec["gin"]:
                self.judge(name, "root", "d input%d" % i, _n64(rec["gin"][1 + i]), gr[i], ga[i])
        pw = self.param_grad(rec, 0)
        if pw is not None:
            self.judge(name, "root", "d weight", pw, gr[-1], ga[-1])
        return "ok"

    def StemConvFn(self, rec, n):
        images, w = rec["args"][0], rec["args"][1]
        name = "stem[%s]" % self.pname(rec, 1)
        i64 = images.detach().to(D64)
        w64 = _leaf(w.to(D64))
        wa = _leaf(w64.abs())
        yr = F.conv2d(i64, w64, None, 1, 3)
        ya = F.conv2d(i64.abs(), wa, None, 1, 3)
        self.judge(name, "stem", "forward", _n64(rec["out"][0]), yr.detach(), ya.detach())
        pw = self.param_grad(rec, 1)
        if 0 in rec["gout"] and pw is not None:
            gy = _n64(rec["gout"][0])
            self.judge(name, "stem", "d weight", pw, _grads(yr, [w64], gy)[0], _grads(ya, [wa], gy.abs())[0])
        return "ok"

    def MaxPool2x2Fn(self, rec, n):
        x = rec["args"][0]
        x64 = _n64(x)
        yr = F.max_pool2d(x64, 2, 2)
        y = _n64(rec["out"][0])
        ok = bool(torch.equal(y, yr))
        bad = 0
        if 0 in rec["gout"] and 0 in rec["gin"]:
            gy, dx = _n64(rec["gout"][0]), _n64(rec["gin"][0])
            H2, W2 = yr.shape[2] * 2, yr.shape[3] * 2
            up = F.interpolate(yr, scale_factor=2, mode="nearest")
            xs, dxs = x64[:, :, :H2, :W2], dx[:, :, :H2, :W2]
            # the gradient goes to one maximum of each window, exactly, and nowhere else (ties: any of them)
            bad += int(((dxs != 0) & (xs != up)).sum()) + int((dx[:, :, H2:] != 0).sum()) + int((dx[:, :, :, W2:] != 0).sum())
            bad += int((F.avg_pool2d(dxs, 2, 2) * 4 != gy).sum())
        self.rows.append(dict(node="maxpool %dx%d" % tuple(x64.shape[2:]), family="maxpool", quantity="forward + d input", 
                              bound=0.0, max=float(bad) + (0.0 if ok else 1.0), mean=0.0, rel_l2=0.0))
        if not ok or bad:
            self.fail.append(("maxpool", bad, ok))
        return "ok"

    def UpsampleAddFn(self, rec, n):
        t, w, skip, f = rec["args"][:4]
        name = "up[%s]" % self.pname(rec, 1)
        t64, s64, w64 = _leaf(_n64(t)), _leaf(_n64(skip)), _leaf(w.to(D64))
        C = t64.shape[1]
        yr = F.conv_transpose2d(t64, w64, None, f, f // 2, groups=C) + s64
        ta, sa, wa = _leaf(t64.abs()), _leaf(s64.abs()), _leaf(w64.abs())
        ya = F.conv_transpose2d(ta, wa, None, f, f // 2, groups=C) + sa
        self.judge(name, "up_add", "forward", _n64(rec["out"][0]), yr.detach(), ya.detach())
        if 0 not in rec["gout"]:
            return "no-grad"
        gy = _n64(rec["gout"][0])
        gr = _grads(yr, [t64, s64, w64], gy)
        ga = _grads(ya, [ta, sa, wa], gy.abs())
        if 0 in rec["gin"]:
            self.judge(name, "up_add", "d input", _n64(rec["gin"][0]), gr[0], ga[0])
        if 2 in rec["gin"]:
            self.judge(name, "up_add", "d skip", _n64(rec["gin"][2]), gr[1], ga[1])
        pw = self.param_grad(rec, 1)
        if pw is not None:
            self.judge(name, "up_add", "d weight", pw, gr[2], ga[2])
        return "ok"

    def DCNModuleFn(self, rec, n):
        x, w_off, b_off, w, bias = rec["args"][:5]
        name = "dcn[%s]" % self.pname(rec, 3)
        om = rec["om"].permute(0, 3, 1, 2).to(D64)
        off_k, msk_k = om[:, :18], om[:, 18:27]
        x64 = _leaf(_n64(x))
        wo, bo, w64, b64 = _leaf(w_off.to(D64)), _leaf(b_off.to(D64)), _leaf(w.to(D64)), _leaf(bias.to(D64))
        raw = F.conv2d(x64, wo, bo, 1, 1)
        raw.retain_grad()
        # (a) the offset / mask conv the kernel ran, against float64 (magnitude: |x| * |w_off| + |b_off|; the mask through the sigmoid, slope <= 1/4)
        with torch.no_grad():
            mraw = F.conv2d(x64.abs(), wo.abs(), bo.abs(), 1, 1)
        self.judge(name, "dcn", "offsets", off_k, raw[:, :18].detach(), mraw[:, :18])
        self.judge(name, "dcn", "mask", msk_k, torch.sigmoid(raw[:, 18:27]).detach(), 0.25 * mraw[:, 18:27])
        off = off_k + (raw[:, :18] - raw[:, :18].detach())
        sm = torch.sigmoid(raw[:, 18:27])
        msk = msk_k + (sm - sm.detach())
        yr = _dcn64(x64, off, msk, w64) + b64.view(1, -1, 1, 1)
        xa, wa, ba = _leaf(x64.detach().abs()), _leaf(w64.detach().abs()), _leaf(b64.detach().abs())
        ya = _dcn64(xa, off_k, msk_k, wa) + ba.view(1, -1, 1, 1)
        self.judge(name, "dcn", "forward", _n64(rec["out"][0]), yr.detach(), ya.detach())
        if 0 not in rec["gout"]:
            return "no-grad"
        gy = _n64(rec["gout"][0])
        yr.backward(gy)
        gr = [t.grad if t.grad is not None else torch.zeros_like(t) for t in (x64, wo, bo, w64, b64)]
        ga = _grads(ya, [xa, wa, ba], gy.abs())
        # magnitudes of the offset conv's gradients: its operands |x|, |w_off| and the float64 gradient of the raw offset / mask map
        adr = raw.grad.detach().abs()
        xd, wod = _leaf(x64.detach().abs()), _leaf(wo.detach().abs())
        mo = _grads(F.conv2d(xd, wod, None, 1, 1), [xd, wod], adr)
        mdx = ga[0] + mo[0]
        if 0 in rec["gin"]:
            dxk = _n64(rec["gin"][0])
            self.judge(name, "dcn", "d input", dxk, gr[0], mdx)
            far = _far_taps(off_k)
            nfar = int(far.sum())
            self.far_samples += nfar
            if nfar:                                                   # (a) the input gradient without the far corners' samples (kept: the layer where it shows most)
                xs_ = _leaf(x64.detach())
                part = _grads(_dcn64(xs_, off_k, msk_k, w64.detach()), [xs_], gy)[0]
                xs2 = _leaf(x64.detach())
                part_far_dropped = _grads(_dcn64(xs2, off_k, msk_k.masked_fill(far, 0.0), w64.detach()), [xs2], gy)[0]
                self.tooth("(a) %s d input without its %d far samples" % (name, nfar), "dcn", "d input", dxk, gr[0] - part + part_far_dropped, mdx)
        for idx, q, g_ref, mag in ((1, "d offset weight", gr[1], mo[1]), (2, "d offset bias", gr[2], adr.sum(dim=(0, 2, 3))),
                                   (3, "d weight", gr[3], ga[1]), (4, "d bias", gr[4], ga[2])):
            pg = self.param_grad(rec, idx)
            if pg is not None:
                self.judge(name, "dcn", q, pg, g_ref, mag)
        return "ok"


def _first_batch(model, device):
    """bench.run_train's batch 0."""
    from monoflex_amd import parallel, synthetic as S
    from monoflex_amd.engine.trainer import _clone_targets, prepare_targets
    from monoflex_amd.structures.params_3d import make_train_target
    seed = parallel.shard_seed(1000, 0, B)
    imgs = S.synthetic_images(B, seed=seed).to(device)
    tg = prepare_targets(model, [make_train_target(S.synthetic_train_target(seed + i)).to(device) for i in range(B)], device)
    return imgs, tg, _clone_targets


def _counters(lib):
    return {n: int(lib.mfx_get_counter(n.encode())) for n in COUNTERS}


@pytest.mark.parametrize("mode", ["bf16", "fp16"])
def test_train_layer_oracle_walk_of_the_benchmarked_step(mode):
    import bench
    from monoflex_amd import autograd as AG, gram_heads as GH, lib as L
    from monoflex_amd.engine.trainer import GraphedTrainStep, LossScaler, train_step
    from monoflex_amd.solver import build_optimizer
    t_start = time.time()
    lib = L.load()
    dev = torch.device("cuda:0")
    assert AG.RESIDUAL_ALIAS[0] and not AG._BN_SEPARATE[0] and not AG._CONV_STATS_OFF[0]
    model, _, cfg = bench.build_model(mode, dev, train=True)
    model.heads.loss_evaluator.log_as_float = False
    assert model.heads.loss_evaluator.fused_object_loss
    imgs, tg, clone_targets = _first_batch(model, dev)
    opt = build_optimizer(model, cfg, capturable=True)
    scaler = LossScaler.for_model(model, dev)
    if scaler is not None:
        scaler.attach(opt)
    s0 = float(scaler.scale) if scaler is not None else 1.0
    with torch.no_grad():
        p_old = {id(p): p.detach().clone() for p in model.parameters()}
        buf_old = {id(b): b.detach().clone() for b in model.buffers()}
    w = _Walk(mode, model, lib, s0)
    classes = [(getattr(AG, n), n) for n in CHECKED + COUNTED] + [(getattr(GH, n), n) for n in GRAM]
    L.bn_onepass_ok(reset=True)
    torch.cuda.synchronize()
    c0 = _counters(lib)
    try:
        for cls, n in classes:
            setattr(cls, "apply", w.wrap(cls, n))
        loss, _, _ = train_step(model, opt, imgs, tg, scaler=scaler)
        torch.cuda.synchronize()
    finally:
        for cls, n in classes:
            if "apply" in cls.__dict__:
                delattr(cls, "apply")
    c1 = _counters(lib)
    eager = {k: c1[k] - c0[k] for k in COUNTERS}
    onepass_ok = L.bn_onepass_ok(reset=True)
    t_step = time.time()
    applied = True
    if scaler is not None:
        applied = float(scaler.found_inf) == 0.0
    w.applied = applied
    # ---- every checked node against its float64 restatement, one at a time
    status = {}
    nrec = len(w.recs)
    print("\n%s: step done in %.0f s, %d recorded nodes" % (mode, t_step - t_start, nrec), flush=True)
    while w.recs:
        if (nrec - len(w.recs)) % 25 == 0:
            print("%s: node %d / %d at %.0f s" % (mode, nrec - len(w.recs), nrec, time.time() - t_start), flush=True)
        rec = w.recs.pop(0)
        try:
            st = getattr(w, rec["kind"])(rec, len(w.recs))
        except Exception as e:                                             # noqa: BLE001  (reported with the node, the walk goes on)
            st = "error"
            w.fail.append((rec["kind"], "reference raised", repr(e)[:300]))
        status[(rec["kind"], st)] = status.get((rec["kind"], st), 0) + 1
        del rec
    torch.cuda.empty_cache()
    # ---- BN running buffers
    bn_of = {id(m.running_mean): m for m in model.modules() if torch.is_tensor(getattr(m, "running_mean", None))}
    assert set(w.bn_ref) <= set(bn_of)
    for key, r in w.bn_ref.items():
        m = bn_of[key]
        if m.num_batches_tracked is not None and int(m.num_batches_tracked) != int(buf_old[id(m.num_batches_tracked)]) + 1:
            w.fail.append(("num_batches_tracked", r["name"]))
        mom = r["mom"]
        rm0, rv0 = buf_old[id(m.running_mean)].to(D64), buf_old[id(m.running_var)].to(D64)
        rm_ref = (1 - mom) * rm0 + mom * r["mean"]
        rv_ref = (1 - mom) * rv0 + mom * r["var_u"]
        mm = (1 - mom) * rm0.abs() + mom * r["absmean"]
        mv = (1 - mom) * rv0.abs() + mom * r["sq"] * r["M"] / max(1, r["M"] - 1)
        for q, got, ref, mag in (("running_mean", m.running_mean, rm_ref, mm), ("running_var", m.running_var, rv_ref, mv)):
            s = _score(got.detach().to(D64), ref, mag, U32, 0.0)
            w.rows.append(dict(node=r["name"], family="bn_buffers", quantity=q, bound=K_RUNNING, **s))
            if not s["max"] <= K_RUNNING:
                w.fail.append((r["name"], q, s["max"]))
        if w.tooth_c_M is None or r["M"] < w.tooth_c_M:
            w.tooth_c_M = r["M"]
            s = _score(m.running_var.detach().to(D64), (1 - mom) * rv0 + mom * r["var_b"], mv, U32, 0.0)
            w.teeth = [t for t in w.teeth if not t["case"].startswith("(c)")]
            w.teeth.append(dict(case="(c) %s running_var with the biased variance (M = %d)" % (r["name"], r["M"]), observed=s["max"], bound=K_RUNNING))
    # ---- AdamW from the recorded (unscaled) gradients, float64
    for g in opt.param_groups:
        lr = float(g["lr"])
        b1, b2 = g["betas"]
        eps, wd = float(g["eps"]), float(g["weight_decay"])
        for p in g["params"]:
            st = opt.state.get(p, {})
            p0 = p_old[id(p)].to(D64)
            if p.grad is None:
                continue
            if not applied:
                if not torch.equal(p.detach(), p_old[id(p)]):
                    w.fail.append(("skipped step moved", w.names.get(id(p))))
                continue
            gr = p.grad.detach().to(D64)
            step = 1
            m1 = (1 - b1) * gr
            v1 = (1 - b2) * gr * gr
            bc1, bc2 = 1 - b1 ** step, 1 - b2 ** step
            upd = (lr / bc1) * m1 / (v1.sqrt() / bc2 ** 0.5 + eps)
            pref = p0 * (1 - lr * wd) - upd
            mag = p0.abs() + upd.abs()
            for q, got, ref, mg in (("param", p, pref, mag), ("exp_avg", st["exp_avg"], m1, m1.abs()), ("exp_avg_sq", st["exp_avg_sq"], v1, v1)):
                s = _score(got.detach().to(D64), ref, mg, U32, 0.0)
                key = ("adamw", q)
                if s["max"] > w.adamw_worst.get(key, (0.0, ""))[0]:
                    w.adamw_worst[key] = (s["max"], w.names.get(id(p), "?"))
                if not s["max"] <= K_ADAMW:
                    w.fail.append(("adamw", q, w.names.get(id(p)), s["max"]))
            if int(float(st["step"])) != step:
                w.fail.append(("adamw step", w.names.get(id(p)), float(st["step"])))
            # (d) L2 instead of decoupled weight decay
            g2 = gr + wd * p0
            m2, v2 = (1 - b1) * g2, (1 - b2) * g2 * g2
            pl2 = p0 - (lr / bc1) * m2 / (v2.sqrt() / bc2 ** 0.5 + eps)
            s = _score(p.detach().to(D64), pl2, mag, U32, 0.0)
            if s["max"] > w.tooth_d[0]:
                w.tooth_d = (s["max"], w.names.get(id(p), "?"))
    for key, (v, pn) in sorted(w.adamw_worst.items()):
        w.rows.append(dict(node="adamw (worst: %s)" % pn, family="adamw", quantity=key[1], bound=K_ADAMW, max=v, mean=0.0, rel_l2=0.0))
    if applied:
        w.teeth.append(dict(case="(d) AdamW with L2 instead of decoupled weight decay (worst: %s)" % w.tooth_d[1], observed=w.tooth_d[0], bound=K_ADAMW))
    t_ref = time.time()
    # ---- the captured step on the same state: the same families per step (3 warm-up steps + the capture)
    tg2 = clone_targets(tg)
    im2 = imgs.clone()
    g0 = _counters(lib)
    step = GraphedTrainStep(model, opt, im2, tg2, scaler=scaler)
    torch.cuda.synchronize()
    g1 = _counters(lib)
    graphed = {k: (g1[k] - g0[k]) / 4.0 for k in COUNTERS}
    step()
    torch.cuda.synchronize()
    assert L.bn_onepass_ok(reset=True)
    del step
    # ---- report
    calls = dict(w.calls)
    os.makedirs(REPORT_DIR, exist_ok=True)
    with open(os.path.join(REPORT_DIR, "train_layer_oracle_%s.json" % mode), "w") as f:
        json.dump(dict(mode=mode, batch=B, loss=float(loss), loss_scale=s0, step_applied=applied, seconds=dict(step=t_step - t_start,
                       reference=t_ref - t_step, total=time.time() - t_start), counters_eager=eager, counters_graphed_per_step=graphed,
                       calls=calls, node_status={"%s:%s" % k: v for k, v in status.items()}, nonfinite=w.nonfinite, mask_flips=w.mask_flips, ambiguous=w.amb_count,
                       ambiguous_worst_fraction=w.amb_worst, far_samples=w.far_samples,
                       rows=w.rows, teeth=w.teeth, failures=[str(x) for x in w.fail]), f, indent=1)
    worst = {}
    for r in w.rows:
        key = (r["family"], r["quantity"])
        if r["max"] >= worst.get(key, {"max": -1})["max"]:
            worst[key] = r
    print("\n%s: %d comparisons, step %.0f s, reference %.0f s; worst per (family, quantity):" % (mode, len(w.rows), t_step - t_start, t_ref - t_step))
    for key in sorted(worst):
        r = worst[key]
        print("  %-10s %-18s max %.3g mean %.3g border %.3g chan %.3g relL2 %.2e bound %.3g  (%s)" % (
            key[0], key[1], r["max"], r["mean"], r.get("border_max", 0.0), r.get("chan_mean", 0.0), r["rel_l2"], r["bound"], r["node"]))
    print("%s counters eager %s" % (mode, eager))
    print("%s counters graphed/step %s" % (mode, graphed))
    print("%s calls %s, mask flips %d, elements within their bound of zero %d (worst BN %.3g %%), far samples %d" % (
        mode, calls, w.mask_flips, w.amb_count, 100 * w.amb_worst, w.far_samples))
    for t in w.teeth:
        print("%s tooth %-80s observed %.3g bound %.3g" % (mode, t["case"], t["observed"], t["bound"]))
    # ---- assertions
    assert onepass_ok, "a one-pass BN launch gave up at its grid barrier during the step"
    assert eager["bn_fwd_onepass"] > 0 and eager["bn_bwd_onepass"] > 0
    assert eager == STEP_COUNTS[mode], {k: (eager[k], STEP_COUNTS[mode][k]) for k in COUNTERS if eager[k] != STEP_COUNTS[mode][k]}
    assert graphed == {k: float(v) for k, v in eager.items()}, (graphed, eager)
    for n, want in CALLS.items():
        if want is not None:
            assert calls.get(n, 0) == want, (n, calls.get(n, 0), want)
    assert not w.fail, w.fail[:20]
    from test_gpu_train_fullsize import BOUND as B2
    fam2 = {"conv": "conv_bn", "bn": "conv_bn", "root": "root", "dcn": "dcn", "up_add": "up_add", "stem": "stem"}
    for r in w.rows:
        f2 = fam2.get(r["family"])
        if f2 is not None and r["quantity"] not in ("offsets", "mask"):
            assert r["rel_l2"] < B2[mode][(f2, "fwd" if r["quantity"] == "forward" else "grad")], r
    assert applied or mode == "fp16"
    assert w.nonfinite == 0 or not applied, w.nonfinite
    cases = {t["case"][:3] for t in w.teeth}
    assert "(c)" in cases and ("(b)" in cases or not applied) and ("(d)" in cases or not applied) and ("(a)" in cases or w.far_samples == 0), cases
    weak = [t for t in w.teeth if not t["observed"] >= 2 * t["bound"]]
    assert not weak, weak
