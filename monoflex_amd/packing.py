"""Every weight layout the kernels read (include/monoflex_hip.h), and nothing else: the packed parameter containers, the
split-precision operand rule, the operand geometry rule and the pack functions.  Packing is torch indexing on whatever device the
weights live on (done once per `prepare`, not on the hot path); the operator wrappers that consume the packs are in ops.py."""
import math
from dataclasses import dataclass
from typing import Optional

import torch

from .lib import ACT_LEAKY, ACT_NONE, ACT_RELU


# Compute tag of the split-precision mode (include/monoflex_hip.h MFX_F16X2): activations are ordinary float32 tensors, the GEMM
# kernels (conv2d / cat_conv1x1 / dcn / heads_fused) multiply fp16 (hi, lo) operand pairs.  The tag travels with the PACKED WEIGHTS
# (`pack_*(…, dtype=F16X2)` -> `.split`), which is what selects the kernel; modules learn it from `compute_tag`.
F16X2 = "f16x2"


def compute_tag(module, dtype):
    """The pack / kernel tag a module uses for activations of `dtype`: F16X2 when the module was switched to the split-precision
    mode (KeypointDetector.set_compute_dtype("fp16x2") marks every sub-module) and the activations are fp32."""
    if dtype == torch.float32 and module.__dict__.get("_mfx_split", False):
        return F16X2
    return dtype


def storage_dtype(dtype):
    return torch.float32 if dtype == F16X2 else dtype


def _elems(dtype):
    return 4 if (dtype == torch.float32 or dtype == F16X2) else 8


def split_halves(w):
    """fp32 -> (hi, lo), two fp16 tensors of the same shape: hi = fp16(w), lo = fp16(w - hi) (csrc/common.h f32s_t).  THE split-precision
    operand rule; the power-of-two scale the weights are multiplied with first is `split_weight_scale`."""
    hi = w.half()
    return hi, (w - hi.float()).half()


def split_chunks(w):
    """fp32 tensor (element count a multiple of 4, chunks of 4 consecutive values) -> the same shape, float32-TYPED, every 16-byte
    chunk holding [4 hi halves | 4 lo halves] of its 4 values (split_halves)."""
    w = w.detach().float().contiguous()
    return torch.cat(split_halves(w.view(-1, 4)), 1).contiguous().view(torch.float32).view(w.shape)


def cast_operand(w, dtype):
    """Weights as the kernels of compute tag `dtype` read them."""
    return split_chunks(w) if dtype == F16X2 else w.to(dtype)


def pair_steps(x, dim):
    """Split-precision fragment-major weights for the kernels that walk K in step PAIRS (csrc/heads.hip): `x` is float32-typed with
    16-byte chunks [hi hi | lo lo] (dwords) in its last axis and the K step on axis `dim`; the result replaces that axis by
    [pair][hi | lo] and every chunk by [its dwords of step 2p | of step 2p+1]: one 8-element fp16 MFMA operand of hi (lo) halves."""
    sh = list(x.shape)
    dim = dim % len(sh)
    assert sh[-1] == 4 and sh[dim] % 2 == 0
    lead, mid = sh[:dim], sh[dim + 1:-1]
    nl, nm = len(lead), len(mid)
    v = x.reshape(*lead, sh[dim] // 2, 2, *mid, 2, 2)                  # [.., pair, step in pair, mid.., hi/lo, dword]
    perm = list(range(nl)) + [nl, nl + 2 + nm] + [nl + 2 + i for i in range(nm)] + [nl + 1, nl + 3 + nm]
    return v.permute(*perm).contiguous().view(*lead, sh[dim] // 2, 2, *mid, 4)


def split_weight_scale(w):
    """Power of two s (python float) that brings max |w| * s into [2^11, 2^12): the lo halves of the scaled weights are then normal
    fp16 numbers down to |w| = 2^-14 of the largest one (unscaled, every lo half of a |w| < 0.25 weight is an fp16 SUBNORMAL, i.e.
    carries a 3e-8 absolute error -- ~1e-6 relative on DLA-34's weights, the largest error term of the split mode).  The kernels'
    epilogues undo it exactly: pack_* fold 1/s into the per-channel `scale` (and remember it: PackedConv.split_scale)."""
    m = float(w.detach().abs().max())
    if not (m > 0.0) or not math.isfinite(m):
        return 1.0
    return 2.0 ** (11 - math.floor(math.log2(m)))


def _pow2(v):
    return v > 0 and (v & (v - 1)) == 0


def _round_up(v, m):
    return (v + m - 1) // m * m


def cout_pad(c):
    """Rows of a packed operand with `c` output channels."""
    return 16 if c <= 16 else 32 if c <= 32 else _round_up(c, 64)


def _pad_channels(n, dtype):
    """Output-channel padding of a training conv: a power of two (>= one 16-byte chunk) so the padded map is a valid conv input."""
    return _round_up(n, 64) if n >= 64 else max(4 if dtype == torch.float32 else 8, 1 << (n - 1).bit_length())


def operand_geometry(kh, kw, ck, rows, stride, pad_h, pad_w, elems):
    """THE geometry of a conv operand [rows][(tap, `ck` channels)] of `elems` elements per 16-byte chunk -> (K_pad, Cout_pad, whether
    it gets a fragment-major copy for the LDS-halo kernels: 3x3, stride 1 or 2, pad 1).  128 bytes of K lets the kernel run 64- or 128-byte
    k-iterations; a K of 64 bytes (the 32 -> 64 1x1 "project" conv of DLA level 2 in 16-bit modes) stays at 64: padded to 128 the generic kernel
    loaded every row twice as wide as it is (19.3 -> 13.4 us at 8 x 96 x 320, tools/pointwise_bench.py)."""
    K = kh * kw * ck
    K_pad = _round_up(K, 8 * elems if K >= 8 * elems else 4 * elems)
    return K_pad, cout_pad(rows), kh == 3 and kw == 3 and stride in (1, 2) and pad_h == 1 and pad_w == 1


@dataclass
class PackedConv:
    w: torch.Tensor                 # [Cout_pad][K_pad]
    scale: Optional[torch.Tensor]   # fp32 [Cout_pad]
    shift: Optional[torch.Tensor]
    kh: int
    kw: int
    stride: int
    pad_h: int
    pad_w: int
    dil_w: int
    Ck: int
    Cout: int
    Cout_pad: int
    K_pad: int
    act: int
    w_frag: Optional[torch.Tensor] = None   # fragment-major copy for the LDS-halo kernel (3x3 / stride 1)
    w_frag_f16: Optional[torch.Tensor] = None   # same, IEEE fp16 (DCN LDS-patch kernel, bf16 mode)
    w_frag_pair: Optional[torch.Tensor] = None  # split precision: w_frag with its K steps paired (pair_steps; mfx_conv_desc.w_frag_pair)
    w_pair_f16: Optional[torch.Tensor] = None   # IEEE fp16, tap-pair K order of the fourth-generation DCN kernel (dcn_pair_fragments; mfx_dcn_desc.w_pair_f16)
    ps: Optional["PackedConv"] = None           # DCN as project-then-sample: the same weights as ONE 1x1 conv C -> 9*Cout (rows (tap, n)); built on first use (dcn_ps_pack)
    split: bool = False                     # split-precision operands (F16X2): fp32 activations, MFX_F16X2 kernels
    split_scale: float = 1.0                # split precision: the power of two `w` holds the weights times (split_weight_scale; `scale` holds the caller's / it)
    transient: bool = False                 # training operand, rebuilt every step: no derived operand is worth packing behind it (ops.dcn_ps_applies)
    entry: Optional[dict] = None            # training operand: its _PackRegistry entry (autograd._pack_weight)
    f1_w160: Optional[torch.Tensor] = None  # [Cout][160] slice of `w`, cached by ops.f1_fused


@dataclass
class PackedCat:
    w: torch.Tensor
    scale: torch.Tensor
    shift: torch.Tensor
    Cseg: int
    Cout: int
    Cout_pad: int
    K_pad: int
    act: int
    split: bool = False


@dataclass
class PackedHeads:
    w1: torch.Tensor
    scale1: torch.Tensor
    shift1: torch.Tensor
    w2: torch.Tensor
    bias2: torch.Tensor
    K_pad: int
    ch_off: list
    c_out: list
    ld_out: int
    split: bool = False
    act: int = ACT_LEAKY                     # the trunks' activation (mfx_heads_fused_act): ACT_LEAKY (InPlaceABN) or ACT_RELU (BatchNorm2d + ReLU)
    w2_scale: Optional[list] = None          # per branch, multiplies the 1x1 sums before the bias (split precision: 1 / the weights' packing scale)
    w1_32: Optional[torch.Tensor] = None     # packs of the v_mfma_f32_32x32x16 form of the kernel (16-bit modes; mfx_heads_desc.w1_32 / w2_32)
    w2_32: Optional[torch.Tensor] = None
    edge_trunk: Optional[PackedConv] = None  # edge fusion (detector_predictor._pack): the class and 3d_offset trunks as one conv at the border points
    edge_branches: Optional[list] = None     # ... and per fusion branch (Conv1d pack (k = 1, 3, 5, 7), Conv1d 1x1 pack, channels, channel offset in the head map)
    edge_chain: Optional["PackedEdgeChain"] = None   # the same five operands for the one-kernel chain (16-bit modes; pack_edge_chain)


@dataclass
class PackedEdgeChain:
    """mfx_edge_chain's / mfx_edge_chain_ks's operands (csrc/edge_chain.hip): fragment-major weights, branch 0 = class, 1 = 3d_offset."""
    w_trunk: torch.Tensor       # [2 x 16][18][4][16][8]
    scale_trunk: torch.Tensor   # fp32 [2 x 256]
    shift_trunk: torch.Tensor
    w_conv: torch.Tensor        # [2][16][8 ksize][4][16][8]
    scale_conv: torch.Tensor    # fp32 [2][256] (no BatchNorm1d: ones, and shift_conv the Conv1d's bias)
    shift_conv: torch.Tensor
    w_out: torch.Tensor         # [2][1][8][4][16][8]
    bias_out: torch.Tensor      # fp32 [2][16]
    relu: bool
    act_trunk: int = ACT_LEAKY  # the trunk's activation (mfx_edge_chain_act), the row-map trunk pack's
    ksize: int = 3              # the Conv1d's window (MODEL.HEAD.EDGE_FUSION_KERNEL_SIZE): 1, 3, 5 or 7


EDGE_CHAIN_KSIZES = (1, 3, 5, 7)    # the windows csrc/edge_chain.hip is instantiated for


def fragment_major(w2d, dtype):
    """[Cout_pad][K_pad] -> [Cout_pad/16][K_pad/(4E)][4 kq][16 n][E]: one MFMA weight fragment (16 rows x 64 bytes of K)
    per contiguous KiB, lane (kq*16 + n) owning 16 bytes."""
    E = _elems(dtype)
    N, K = w2d.shape
    assert N % 16 == 0 and K % (4 * E) == 0
    return w2d.view(N // 16, 16, K // (4 * E), 4, E).permute(0, 2, 3, 1, 4).contiguous()


def pack_edge_chain(trunk: PackedConv, branches):
    """The edge fusion's five conv operands (detector_predictor._pack: the row-map trunk of both branches, per branch the Conv1d and the 1x1
    pack) as the one-kernel chain reads them: the SAME [rows][K] matrices, K = (tap, channel), fragment-major, so that both forms multiply the
    same numbers in the same K order.  16-bit packs of the 64 -> 256 trunk, a Conv1d of k = 1, 3, 5 or 7 and at most 4 output channels; None otherwise."""
    dtype = trunk.w.dtype
    if trunk.split or dtype not in (torch.bfloat16, torch.float16) or len(branches) != 2 or trunk.act not in (ACT_LEAKY, ACT_RELU):
        return None
    if (trunk.kh, trunk.kw, trunk.Ck, trunk.Cout, trunk.K_pad) != (3, 3, 64, 512, 576):
        return None
    k = branches[0][0].kw
    if k not in EDGE_CHAIN_KSIZES:
        return None
    for pk1, pk2, cout, _ in branches:
        if (pk1.kh, pk1.kw, pk1.Ck, pk1.Cout, pk1.K_pad) != (1, k, 256, 256, 256 * k) or pk1.act not in (ACT_NONE, ACT_RELU) or pk1.act != branches[0][0].act:
            return None
        if (pk2.kh, pk2.kw, pk2.Ck, pk2.Cout_pad, pk2.K_pad) != (1, 1, 256, 16, 256) or cout > 4 or pk2.scale is not None or pk2.act != ACT_NONE:
            return None
    return PackedEdgeChain(fragment_major(trunk.w, dtype), trunk.scale, trunk.shift,
                           torch.stack([fragment_major(pk1.w, dtype) for pk1, _, _, _ in branches]).contiguous(),
                           torch.stack([pk1.scale for pk1, _, _, _ in branches]).contiguous(),
                           torch.stack([pk1.shift for pk1, _, _, _ in branches]).contiguous(),
                           torch.stack([fragment_major(pk2.w, dtype) for _, pk2, _, _ in branches]).contiguous(),
                           torch.stack([pk2.shift for _, pk2, _, _ in branches]).contiguous(), branches[0][0].act == ACT_RELU, act_trunk=trunk.act, ksize=k)


def fold_bn(bn, conv_bias=None):
    """Eval-mode BatchNorm as y = x*scale + shift (a preceding conv bias folded in).  No norm (`bn` None or an nn.Identity, the reference's
    stand-in where a norm setting is not 'BN'): scale = 1, shift = the bias -- the kernels' acc * 1 + bias is exact."""
    if bn is None or isinstance(bn, torch.nn.Identity):
        if conv_bias is None:
            raise ValueError("fold_bn: neither a norm nor a bias")
        shift = conv_bias.detach().float()
        return torch.ones_like(shift).contiguous(), shift.contiguous()
    scale = bn.weight.detach().float() / torch.sqrt(bn.running_var.detach().float() + bn.eps)
    shift = bn.bias.detach().float() - bn.running_mean.detach().float() * scale
    if conv_bias is not None:
        shift = shift + conv_bias.detach().float() * scale
    return scale.contiguous(), shift.contiguous()


def _pad_rows_cols(w2d, rows, cols):
    out = w2d.new_zeros(rows, cols)
    out[:w2d.shape[0], :w2d.shape[1]] = w2d
    return out


def pack_conv(weight, dtype, scale=None, shift=None, stride=1, pad=0, act=ACT_NONE, cout=None):
    """weight (Cout,Cin,kh,kw) -> K-contiguous [Cout_pad][K_pad], K = (tap, channel)."""
    Cout, Cin, kh, kw = weight.shape
    if not _pow2(Cin) or Cin < _elems(dtype):
        raise ValueError("pack_conv: Cin must be a power of two >= %d (got %d)" % (_elems(dtype), Cin))
    cout = Cout if cout is None else cout
    K_pad, cp, frag = operand_geometry(kh, kw, Cin, cout, stride, pad, pad, _elems(dtype))
    w2 = weight.detach().float().permute(0, 2, 3, 1).reshape(Cout, kh * kw * Cin)
    ws = 1.0
    if dtype == F16X2:
        ws = split_weight_scale(w2)
        w2 = w2 * ws
        scale = (scale.detach().float() if scale is not None else torch.ones(Cout, device=weight.device)) / ws
    w2 = cast_operand(_pad_rows_cols(w2, cp, K_pad), dtype).contiguous()

    def padv(v, fill):
        if v is None:
            return None
        v = v.detach().float()
        if v.numel() < cp:
            v = torch.cat((v, v.new_full((cp - v.numel(),), fill)))
        return v.contiguous()
    wf = fragment_major(w2, dtype) if frag else None
    pk = PackedConv(w2, padv(scale, 1.0), padv(shift, 0.0), kh, kw, stride, pad, pad, 1, Cin, cout, cp, K_pad, act, wf, split=dtype == F16X2, split_scale=ws)
    if wf is not None and dtype == F16X2 and Cin >= 32:
        pk.w_frag_pair = pair_steps(wf, 1)
    return pk


# stem geometry: zero-padded NHWC4 image, 3 columns left / 5 right, 3 rows top/bottom
STEM_PAD_H, STEM_PAD_WL, STEM_PAD_WR = 3, 3, 5


def pack_stem(weight, dtype, scale, shift, act=ACT_RELU):
    """7x7/s1/p3 conv on 3 channels (dla_dcn.py:268-272) over the padded NHWC4 image.
    bf16: a 16-byte chunk is 2 adjacent pixels x 4 ch -> 7 x 4 'super taps' of 8 elements, dil_w = 2.
    f32 : a chunk is 1 pixel x 4 ch -> 7 x 7 taps of 4 elements."""
    Cout = weight.shape[0]
    w = weight.detach().float()
    w4 = torch.cat((w, w.new_zeros(Cout, 1, 7, 7)), dim=1)              # (Cout,4,7,7)
    dedicated = dtype == F16X2 and Cout == 16      # split precision, dedicated kernel (csrc/stem.hip stem_conv7x7_split_kernel): the fp16 super-tap matrix
    if dedicated or dtype in (torch.bfloat16, torch.float16):
        w8 = torch.cat((w4, w4.new_zeros(Cout, 4, 7, 1)), dim=3)        # kw 7 -> 8
        # [n][th][j][u][c] with kw = 2j+u
        wp = w8.permute(0, 2, 3, 1).reshape(Cout, 7, 4, 2, 4).reshape(Cout, 7 * 4 * 8)
        kh, kw, Ck, dil = 7, 4, 8, 2
    else:
        wp = w4.permute(0, 2, 3, 1).reshape(Cout, 7 * 7 * 4)
        kh, kw, Ck, dil = 7, 7, 4, 1
    K_pad = wp.shape[1] if dedicated else _round_up(wp.shape[1], 8 * _elems(dtype))
    cp = cout_pad(Cout)
    ws = 1.0
    if dtype == F16X2:
        ws = split_weight_scale(wp)
        wp, scale = wp * ws, scale.detach().float() / ws
    if dedicated:
        wp = torch.cat(split_halves(wp), 0)                            # ... twice: hi rows, then lo rows
    else:
        wp = cast_operand(_pad_rows_cols(wp, cp, K_pad), dtype)
    return PackedConv(wp.contiguous(), scale.contiguous(), shift.contiguous(), kh, kw, 1, 0, 0, dil, Ck, Cout, cp, K_pad, act, split=dtype == F16X2, split_scale=ws)


def pack_cat(weight, dtype, scale, shift, src_channels, act=ACT_RELU):
    Cout, Ctot = weight.shape[:2]
    assert sum(src_channels) == Ctot
    Cseg = min(src_channels)
    assert all(c % Cseg == 0 for c in src_channels) and _pow2(Cseg)
    cp = cout_pad(Cout)
    w2 = weight.detach().float().reshape(Cout, Ctot)
    if dtype == F16X2:
        ws = split_weight_scale(w2)
        w2, scale = w2 * ws, scale.detach().float() / ws
    w2 = cast_operand(_pad_rows_cols(w2, cp, Ctot), dtype).contiguous()
    return PackedCat(w2, scale.contiguous(), shift.contiguous(), Cseg, Cout, cp, Ctot, act, split=dtype == F16X2)


def dcn_pair_fragments(weight, cout_pad):
    """(Cout, Cin, 3, 3) -> the fourth-generation DCN kernel's fp16 weights (csrc/dcn_lds.hip, mfx_dcn_desc.w_pair_f16): the input channels in slices
    of 16, five MFMA k-steps (K = 32) per slice, k-step j = taps (2j, 2j + 1) x the slice's 16 channels (the tenth tap is zeros); fragment-major
    [cout_pad / 16][Cin / 16 * 5][4 kq][16 n][8]: lane (kq, n) holds tap 2j + (kq >> 1), channels 16 s + 8 (kq & 1) .. + 7 of output channel 16 nf + n."""
    Cout, Cin, kh, kw = weight.shape
    assert kh == 3 and kw == 3 and Cin % 16 == 0 and cout_pad % 16 == 0
    w = weight.detach().float().permute(0, 2, 3, 1).reshape(Cout, 9, Cin)
    wp = w.new_zeros(cout_pad, 10, Cin)
    wp[:Cout, :9] = w
    wp = wp.view(cout_pad, 5, 2, Cin // 16, 2, 8).permute(0, 3, 1, 2, 4, 5)      # (n, slice, step, tap parity, channel half, 8)
    w2d = wp.reshape(cout_pad, (Cin // 16) * 5 * 32).to(torch.float16).contiguous()
    return fragment_major(w2d, torch.float16)


def add_f16_fragments(p: PackedConv, weight):
    """Attach the fp16 fragment-major weights the DCN LDS-patch kernels multiply with (bf16 / fp16 mode, 3x3/s1/p1; split precision: the (hi, lo) halves
    of the scaled weights as two consecutive arrays each -- csrc/dcn_lds.hip dcn_lds_split_kernel)."""
    def frag16(w):                                              # (Cout, Cin, kh, kw) -> IEEE fp16 [Cout_pad][K_pad], K = (tap, channel), fragment-major
        w2 = _pad_rows_cols(w.permute(0, 2, 3, 1).reshape(w.shape[0], -1), p.Cout_pad, p.K_pad)
        return fragment_major(w2.to(device=p.w.device, dtype=torch.float16).contiguous(), torch.float16)
    if p.split and p.kh == 3 and p.kw == 3 and p.Cout_pad == 64 and weight.shape[1] % 32 == 0 and p.K_pad == 9 * weight.shape[1]:
        halves = split_halves(weight.detach().float().to(p.w.device) * p.split_scale)
        p.w_pair_f16 = torch.cat([dcn_pair_fragments(h.float(), p.Cout_pad).reshape(-1) for h in halves]).contiguous()
        p.w_frag_f16 = torch.cat([frag16(h).reshape(-1) for h in halves]).contiguous()
        return p
    if p.w_frag is not None and p.w.dtype in (torch.float16, torch.bfloat16) and p.kh == 3 and p.kw == 3 and p.Cout_pad == 64 \
            and weight.shape[1] % 16 == 0 and not p.split:
        p.w_pair_f16 = dcn_pair_fragments(weight.to(p.w.device), p.Cout_pad)
    if p.w_frag is not None and p.w.dtype == torch.float16:
        p.w_frag_f16 = p.w_frag                                  # fp16 mode: the fragments already are IEEE fp16
    elif p.w_frag is not None and p.w.dtype == torch.bfloat16:
        p.w_frag_f16 = frag16(weight.detach().float())
    return p


def dcn_ps_pack(p: PackedConv):
    """The DCN weights [Cout][(tap, c)] as a 1x1 conv C -> 9 * Cout whose output row is [(tap, n)] (no scale / shift / activation: those follow the sampling)."""
    if p.ps is None:
        C = p.K_pad // 9
        w = p.w[:p.Cout].view(p.Cout, 9, C).permute(1, 0, 2).reshape(9 * p.Cout, C, 1, 1)
        p.ps = pack_conv(w, p.w.dtype, None, None, stride=1, pad=0, act=ACT_NONE)
    return p.ps


def pack_upsample(weight):
    """(C,1,k,k) depthwise deconv weight -> fp32 [k*k][C]."""
    C, _, k, _ = weight.shape
    return weight.detach().float().reshape(C, k * k).t().contiguous()


def pack_heads(w3x3, folds, w1x1, b1x1, num_classes, ch_off, ld_out, dtype, act=ACT_LEAKY):
    """The fused heads kernel's operands (csrc/heads.hip).  Per branch (the class head first): `w3x3` the trunk's (256, 64, 3, 3) weight, `folds` its
    folded ABN (scale, shift), `w1x1` / `b1x1` the (c, 256[, 1, 1]) weights and (c,) biases of its stacked 1x1 heads (c <= 32; `num_classes` for the
    class head), `ch_off` its first channel in the `ld_out`-wide head map; `dtype` the compute tag; `act` the trunks' activation, ACT_LEAKY (the folded ABN's) or ACT_RELU (BatchNorm2d + ReLU)."""
    if act not in (ACT_LEAKY, ACT_RELU):
        raise NotImplementedError("pack_heads: the trunk activation is ACT_LEAKY or ACT_RELU, got %r" % (act,))
    nb, hc = len(w3x3), w3x3[0].shape[0]
    w1 = [w.detach().float().permute(0, 2, 3, 1).reshape(hc, -1) for w in w3x3]
    sc, sh = [s for s, _ in folds], [b for _, b in folds]
    K = w1[0].shape[1]
    assert K == 576 and hc == 256 and w1x1[0].shape[0] == num_classes
    E = _elems(dtype)
    steps = K // (4 * E)
    dev = w1[0].device
    w2_scale = None
    if dtype == F16X2:                                         # weights times a power of two per branch (split_weight_scale), undone by scale1 / w2_scale
        for i in range(nb):
            ws = split_weight_scale(w1[i])
            w1[i], sc[i] = w1[i] * ws, sc[i] / ws
    # 3x3 weights, fragment-major: [branch][wave wn 4][step][frag j 4][k-group kq 4][row nl 16][E]  (lane = kq*16+nl)
    W1 = cast_operand(torch.stack(w1, 0).view(nb, 4, 4, 16, steps, 4, E).permute(0, 1, 4, 2, 5, 3, 6).contiguous(), dtype)
    if dtype == F16X2:
        W1 = pair_steps(W1, 2)                                  # [branch][wn][step pair][hi | lo][j][kq][nl][4]: heads.hip walks K in step pairs
    w2 = torch.zeros(nb, 32, hc, device=dev)
    b2 = torch.zeros(nb, 32, device=dev)
    c_out = [w.shape[0] for w in w1x1]
    for i, (w, b) in enumerate(zip(w1x1, b1x1)):
        w2[i, :c_out[i]] = w.detach().float().reshape(c_out[i], -1)
        b2[i, :c_out[i]] = b.detach().float()
    if dtype == F16X2:
        w2_scale = []
        for i in range(nb):
            ws = split_weight_scale(w2[i])
            w2[i] *= ws
            w2_scale.append(1.0 / ws)
    # 1x1 weights, fragment-major with the K order the kernel's accumulators arrive in (heads.hip TrunkPack):
    #   bf16: [branch][wn][kb 2][of 2][g 4][o_l 16][half 2][q 4], trunk channel n = 64wn + 32kb + 16half + 4g + q
    #   f32 : [branch][wn][kb 4][of 2][g 4][o_l 16][e 4],          n = 64wn + 16kb + 4g + e
    if dtype in (torch.float32, F16X2):
        W2 = cast_operand(w2.view(nb, 2, 16, 4, 4, 4, 4).permute(0, 3, 4, 1, 5, 2, 6).contiguous(), dtype)
        if dtype == F16X2:
            W2 = pair_steps(W2, 2)                              # [branch][wn][kb pair][hi | lo][of][g][o_l][4]
    else:
        W2 = w2.view(nb, 2, 16, 4, 2, 2, 4, 4).permute(0, 3, 4, 1, 6, 2, 5, 7).contiguous().to(dtype)
    p = PackedHeads(W1, torch.cat(sc).contiguous(), torch.cat(sh).contiguous(), W2, b2.contiguous(), K, list(ch_off), c_out, ld_out, split=dtype == F16X2, act=act, w2_scale=w2_scale)
    if dtype in (torch.bfloat16, torch.float16):
        # the same weights for the v_mfma_f32_32x32x16 form (csrc/heads.hip heads_fused32_kernel; option "heads_mfma32"):
        #   3x3: [branch][wn 4][K-step 36][rb 2][h 2][row 32][8], channel 64 wn + 32 rb + row, k = 16 s + 8 h + e
        #   1x1: [branch][wn 4][rb 2][t 2][h 2][o 32][a 2][q 4], trunk channel n = 64 wn + 32 rb + 16 t + 8 a + 4 h + q (k-slot e = 4 a + q)
        p.w1_32 = torch.stack(w1, 0).view(nb, 4, 2, 32, 36, 2, 8).permute(0, 1, 4, 2, 5, 3, 6).contiguous().to(dtype)
        p.w2_32 = w2.view(nb, 32, 4, 2, 2, 2, 2, 4).permute(0, 2, 3, 4, 6, 1, 5, 7).contiguous().to(dtype)
    return p
