"""Float64 restatement of the Gram regression-heads node (monoflex_amd/gram_heads.py, csrc/gram_heads.hip) as the DENSE layers it replaces
(reference model/head/detector_predictor.py:125-165), its error-model magnitudes, and the inputs of the oracle cases.  Pure torch, any device.

Per branch:  conv3x3(64 -> 256, pad 1, no bias) -> train-mode BN (biased batch variance) -> leaky(0.01) or ReLU -> 1x1 head (optional bias), read
at the object rows, times (rows[:, 0] > 0), zero in the columns no branch owns; the named branch's activation is also read at the `extra` pixels.
Inputs are what the device sees: x and the trunk weights rounded to the 16-bit type, everything else the fp32 values (never the library's packs).
Gradients are autograd's through that restatement.

Error model, per element:  |got - ref| <= k (u_op M + n_acc u_out |ref| + eta).  M (`magnitudes`) is the same expression on absolute values,
written for the algebra the kernel documents (gram_heads.hip:5-18), so that the Gram path's cancellations count in M and not in k:

    M_y = conv(|x|, |W|)                                     (also evaluated on the one-pixel FRAME around the image)
    the sums over pixels the kernel forms as (autocorrelation over the grown image) - (frame part), gram_heads.hip:17: every pixel sum of M
    counts the image once and the frame TWICE (added by the autocorrelation / the 5x5 conv, taken off again by the frame GEMM / gram_ring)
    M_mean = sum M_y / Mpx,   M_var = sum M_y^2 / Mpx + mean^2          (= sum |w| |G| |w| / M + mean^2)
    M_rstd = rstd + 1/2 rstd^3 M_var,  M_sc = |gamma| M_rstd,  M_sh = |beta| + M_mean |sc| + |mean| M_sc,  M_z = M_y |sc| + |y| M_sc + M_sh
    g = d act . act',  |d sh|+ = sum |g|,  |d sc|+ = sum |g y| + |mean| sum |g|,  |d var|+ = 1/2 |gamma| rstd^3 |d sc|+
    |d s1|+ = (|sc| |d sh|+ + 2 |mean| |d var|+) / Mpx,  |d s2|+ = |d var|+ / Mpx
    M_dy(px, c) = |d y at the rows| + |d s1|+ + 2 |d s2|+ M_y(px, c),   M_dx = conv_transpose(M_dy, |W|),
    M_dW = sum_rows |d y| |patch| + |d s1|+ sum_px |patch| + 2 |d s2|+ (|W| |G|)
    fp16 only: the row gradients d y become fp16 operands (hi + lo halves, gram_heads.hip:20) and underflow below 2^-24: an absolute 2^-25 per
    (row, channel), i.e. eta_dx = 2^-25 (1 + sum_rows sum_c |W|), eta_dW = 2^-25 sum_rows |patch|.  This is a WIDER floor than the plain
    eta = 2^-25 of an fp16 output (test_gpu_train_layer_oracle's, kept for act_e): on d x up to a few thousand times 2^-25 inside the windows,
    nothing more outside them; on d W, which is an fp32 output, a floor where there was none.  With the scaled_down inputs the teeth still
    bite by 16 k or more (test_gram_heads_ref_cpu).

Activation side: the backward recomputes z = y sc + sh in fp32.  A (row, channel) with float64 |z| <= 64 2^-24 (|y| |sc| + |sh|) is AMBIGUOUS: it
may take either side; the reference takes its own and `slack` returns, per element of every gradient, exactly what the other side would move.
Channels with sc == sh == 0 (z == 0 exactly everywhere) have a defined side -- the slope -- and are not ambiguous."""
from types import SimpleNamespace

import torch
import torch.nn.functional as F

D64 = torch.float64
DT = {"bf16": torch.bfloat16, "fp16": torch.float16, "fp32": torch.float32}
U = {"bf16": (2.0 ** -8, 2.0 ** -9), "fp16": (2.0 ** -11, 2.0 ** -11), "fp32": (2.0 ** -24, 2.0 ** -24)}     # (u_op, u_out), test_gpu_train_layer_oracle
ETA = {"bf16": 0.0, "fp16": 2.0 ** -25, "fp32": 0.0}
U32 = 2.0 ** -24
AMB_C = 64.0 * U32
AMB_CAP = 1e-3                                   # at most this fraction of a case's (row, channel) pairs may be ambiguous
SIXTEEN = ("dx", "dW", "act_e")                  # 16-bit grade; everything else is fp32 grade
BASE_KS, BASE_OFFS, BASE_LD = (4, 2, 20, 3), (0, 4, 6, 26), 50
EIGHT_KS = (4, 2, 20, 3, 1, 8, 3, 32)
CASES = ("base", "ragged", "single", "empty", "empty_edge", "eight", "offset", "offset_fwd", "relu", "scaled_up", "scaled_down")
FORWARD_ONLY = ("offset_fwd",)                   # forward pass alone: table, edge activations, running statistics (phases 0..2)
ONLY = {"offset": ("bf16",), "offset_fwd": ("bf16",), "scaled_up": ("fp16",), "scaled_down": ("fp16",)}          # cases that run in one type only
NEEDS_INTERIOR = ("base", "offset", "relu", "scaled_up", "scaled_down")                  # >= 100 pixels that the 5x5 conv alone produces


def case_list():
    return [(dt, name) for dt in ("bf16", "fp16") for name in CASES if dt in ONLY.get(name, ("bf16", "fp16"))]


def _border_pixels(B, H, W):
    """Left column and top row of every image (the edge sequence's pixels), as flat indices."""
    return [b * H * W + y * W for b in range(B) for y in range(H)] + [b * H * W + xx for b in range(B) for xx in range(W)]


def _random_rows(g, N, B, H, W, n_empty):
    rows = torch.zeros(N, 72)
    rows[:, 0] = 1.0
    rows[:, 57] = torch.randint(0, B, (N,), generator=g).float()
    rows[:, 2] = torch.randint(0, W, (N,), generator=g).float()
    rows[:, 3] = torch.randint(0, H, (N,), generator=g).float()
    rows[0, 2:4] = torch.tensor([0.0, 0.0])
    rows[1, 2:4] = torch.tensor([W - 1.0, H - 1.0])
    rows[3] = rows[5]                                                          # coincident objects
    if n_empty:
        rows[torch.arange(N - 1, 5, -1)[:n_empty * 2:2], 0] = 0.0              # every other row from the end: empty slots between valid ones
    return rows


def _placed_rows(places):
    rows = torch.zeros(len(places), 72)
    rows[:, 0] = 1.0
    for r, (b, y, xx) in enumerate(places):
        rows[r, 57], rows[r, 3], rows[r, 2] = float(b), float(y), float(xx)
    return rows


def make_case(name, dt, seed=None, C=256, Cin=64):
    """The inputs of one case as CPU tensors: x in the activation type, everything else fp32 (d act_e rounded to the activation type)."""
    dtype = DT[dt]
    kind = "base" if name in ("relu", "scaled_up", "scaled_down") else name
    g = torch.Generator().manual_seed({"base": 131, "ragged": 132, "single": 133, "empty": 134, "empty_edge": 134, "eight": 136,
                                       "offset": 137, "offset_fwd": 137}[kind] if seed is None else seed)
    slope, dscale, degenerate, xoff, woff = 0.01, 1.0, False, 0.0, 0.0
    if kind == "base":
        B, H, W, N = 2, 12, 20, 20
        ks, offs, ld = BASE_KS, BASE_OFFS, BASE_LD
        rows = _random_rows(g, N, B, H, W, 4)
        pix = _border_pixels(B, H, W)
        extra_branch, extra = 1, pix + [H * W - 1, 2 * H * W - 1] + pix[:3] + [pix[-1]]          # 70 rows: repeats, both far corners
        degenerate = name in ("base", "relu")             # (the scaled cases keep every channel regular: with var == 0, rstd = eps^-1/2 = 316
        #                                                    and d y = g sc times 2^12 leaves fp16's range -- an overflow the loss scaler answers, not rounding)
        slope = 0.0 if name == "relu" else 0.01
        dscale = {"scaled_up": 2.0 ** 12, "scaled_down": 2.0 ** -12}.get(name, 1.0)
    elif kind == "ragged":
        B, H, W = 3, 5, 7
        ks, offs, ld = (32,), (0,), 32
        rows = _placed_rows([(0, 0, 0), (0, 0, 6), (0, 4, 0), (0, 4, 6), (1, 0, 3), (1, 4, 3), (1, 2, 0), (1, 2, 6), (2, 2, 3), (2, 2, 3), (2, 2, 3),
                             (2, 2, 4), (2, 3, 3), (2, 3, 4), (0, 2, 2), (1, 1, 1), (2, 1, 5)])
        extra_branch, extra = -1, None
    elif kind == "single":
        B, H, W = 1, 5, 7
        ks, offs, ld = (1,), (0,), 1
        rows = _placed_rows([(0, 0, 0)])
        extra_branch, extra = 0, [H * W - 1]
    elif kind in ("empty", "empty_edge"):
        B, H, W = 2, 5, 7
        ks, offs, ld = (4, 3), (0, 4), 7
        rows = _random_rows(g, 8, B, H, W, 0)
        rows[:, 0] = 0.0
        extra_branch, extra = (0, [0, 6, 17, 40, 69]) if kind == "empty_edge" else (-1, None)
    elif kind == "eight":
        B, H, W, N = 1, 6, 10, 5
        ks = EIGHT_KS
        offs = tuple(sum(ks[:i]) for i in range(len(ks)))
        ld = sum(ks)
        rows = _placed_rows([(0, 0, 0), (0, 5, 9), (0, 2, 4), (0, 2, 5), (0, 3, 7)])
        extra_branch, extra = 7, [0, 9, 31]
    elif kind in ("offset", "offset_fwd"):
        B, H, W, N = 3, 12, 20, 40
        ks, offs, ld = BASE_KS, BASE_OFFS, BASE_LD
        rows = _random_rows(g, N, B, H, W, 0)
        extra_branch, extra = 1, _border_pixels(B, H, W)[:20]
        if kind == "offset_fwd":
            # x + 1.5, W + 0.01: mean^2 / var ~ 26 (median; up to ~40) per channel -- E[y^2] - E[y]^2 from fp32 sums loses five bits.  Forward only:
            # at this ratio M's |d s1|+ and |d s2|+ (which ADD the two cancelling terms of d mean) widen the 16-bit bounds on d x and d W so far
            # that a reference without the statistics path stays inside them (0.008 of the bound on d x); no gradient is compared where no
            # wrong reference can miss
            xoff, woff = 1.5, 0.01
        else:
            # the largest shift at which the teeth (a) and (d) of test_gram_heads_ref_cpu still bite on d x and d W by a factor of two:
            # mean^2 / var ~ 3.4; objects 3, 5, 7, 11, 15 on one pixel and two more coincident pairs
            xoff, woff = 0.1, 0.015
            for r_ in (7, 11, 15):
                rows[r_] = rows[5]
            rows[9], rows[13] = rows[8], rows[12]
    else:
        raise KeyError(name)
    N = rows.shape[0]
    x = (torch.randn(B, H, W, Cin, generator=g) * 0.8 + 0.1 + xoff).to(dtype)
    wt = [torch.randn(C, Cin, 3, 3, generator=g) / 24.0 + woff for _ in ks]
    w2 = [torch.randn(k, C, 1, 1, generator=g) * 0.1 for k in ks]
    b2 = [None if kind == "single" else torch.randn(k, generator=g) * 0.1 for k in ks]
    gam = [torch.rand(C, generator=g) + 0.5 for _ in ks]
    bet = [torch.randn(C, generator=g) * 0.3 for _ in ks]
    rm0 = [torch.randn(C, generator=g) * 0.2 for _ in ks]                     # running statistics before the step
    rv0 = [torch.rand(C, generator=g) + 0.5 for _ in ks]
    if degenerate:
        for i in range(len(ks)):
            wt[i][0] = 0.0                                                     # var == 0: the clamp and the d var branch of gram_stats_bwd
            gam[i][1] = 0.0; bet[i][1] = 0.0                                   # z == 0 exactly on every row
            gam[i][2] = -gam[i][2]
    dout = torch.randn(N, ld, generator=g) * dscale                            # on every row, empty ones included
    extra_t = None if extra is None else torch.tensor(extra, dtype=torch.long)
    dact = None if extra is None else (torch.randn(len(extra), C, generator=g) * dscale).to(dtype)
    return SimpleNamespace(name=name, dt=dt, dtype=dtype, x=x, rows=rows, wt=wt, w2=w2, b2=b2, gam=gam, bet=bet, rm0=rm0, rv0=rv0, ks=tuple(ks),
                           offs=tuple(offs), ld=ld, extra_branch=extra_branch, extra=extra_t, dout=dout, dact=dact, slope=slope, eps=1e-5,
                           momentum=0.1, forward_only=name in FORWARD_ONLY)


def _coords(c):
    """(image, cy, cx) of the object rows as the node reads them (clamped to the map, truncated), and the valid flag."""
    B, H, W, _ = c.x.shape
    r = c.rows.to(D64)
    bi = r[:, 57].clamp(0, B - 1).long()
    cy = r[:, 3].clamp(0, H - 1).long()
    cx = r[:, 2].clamp(0, W - 1).long()
    return bi, cy, cx, c.rows[:, 0] > 0


def _first_of_coincident(bi, cy, cx, valid, HW, W):
    pix = (bi * HW + cy * W + cx).tolist()
    seen, keep = set(), []
    for p, v in zip(pix, valid.tolist()):
        keep.append(v and p not in seen)
        if v:
            seen.add(p)
    return torch.tensor(keep)


def reference(c, flips=(), variant=None):
    """Everything the node returns, in float64.  `flips`: (branch, 'o' | 'e', row, channel) elements that take the other activation side.
    `variant`: a deliberately WRONG reference (the teeth of test_gram_heads_ref_cpu): 'const_stats' (batch statistics as constants),
    'no_edge_dw' (trunk d W without the edge rows), 'dedupe' (coincident objects once), 'replicate' (row patches from a replicate-padded map),
    'relu_out' (ReLU in place of the case's activation), 'biased_running_var' (the momentum step with the biased variance)."""
    dev = c.x.device
    x = c.x.to(D64)
    B, H, W, Cin = x.shape
    Mpx = B * H * W
    bi, cy, cx, valid = _coords(c)
    if variant == "dedupe":
        valid = _first_of_coincident(bi, cy, cx, valid, H * W, W).to(dev)
    vf = valid.to(D64).view(-1, 1)
    slope = 0.0 if variant == "relu_out" else c.slope
    nb = len(c.ks)
    xr = x.permute(0, 3, 1, 2).clone().requires_grad_()
    xrep = F.pad(xr, (1, 1, 1, 1), mode="replicate") if variant == "replicate" else None
    leaf = lambda t: t.detach().to(D64).clone().requires_grad_()                                     # noqa: E731
    Wl = [leaf(w.to(c.dtype)) for w in c.wt]
    gl, bl, w2l = [leaf(t) for t in c.gam], [leaf(t) for t in c.bet], [leaf(w.view(w.shape[0], -1)) for w in c.w2]
    b2l = [None if b is None else leaf(b) for b in c.b2]
    out = torch.zeros(c.rows.shape[0], c.ld, dtype=D64, device=dev)
    act_e, inter, res = None, [], {}
    flip = {}
    for (b, kind, r, ch) in flips:
        flip.setdefault((b, kind), []).append((r, ch))

    def side(z, key):
        pos = z.detach() > 0
        for (r, ch) in flip.get(key, ()):
            pos[r, ch] = ~pos[r, ch]
        return pos

    res["running_mean"], res["running_var"] = [], []
    for i in range(nb):
        y = F.conv2d(xr, Wl[i], None, 1, 1)
        ys = y.detach() if variant == "const_stats" else y
        mean = ys.mean((0, 2, 3))
        var = ((ys - mean.view(1, -1, 1, 1)) ** 2).mean((0, 2, 3))
        rstd = (var + c.eps) ** -0.5
        sc = gl[i] * rstd
        sh = bl[i] - mean * sc
        ysrc = F.conv2d(xrep, Wl[i]) if variant == "replicate" else y
        y_o = ysrc.permute(0, 2, 3, 1)[bi, cy, cx]
        z_o = y_o * sc + sh
        pos_o = side(z_o, (i, "o"))
        a_o = torch.where(pos_o, z_o, slope * z_o)
        o = a_o @ w2l[i].t()
        if b2l[i] is not None:
            o = o + b2l[i]
        out = out.index_add(1, torch.arange(c.offs[i], c.offs[i] + c.ks[i], device=dev), o * vf)
        it = dict(mean=mean.detach(), var=var.detach(), rstd=rstd.detach(), sc=sc.detach(), sh=sh.detach(), y_o=y_o.detach(), z_o=z_o.detach(),
                  pos_o=pos_o)
        if i == c.extra_branch and c.extra is not None:
            ye_src = F.conv2d(xr, Wl[i].detach(), None, 1, 1) if variant == "no_edge_dw" else ysrc
            y_e = ye_src.permute(0, 2, 3, 1).reshape(Mpx, -1)[c.extra]
            z_e = y_e * sc + sh
            pos_e = side(z_e, (i, "e"))
            act_e = torch.where(pos_e, z_e, slope * z_e)
            it.update(y_e=y_e.detach(), z_e=z_e.detach(), pos_e=pos_e)
        inter.append(it)
        unb = var.detach() * (Mpx / max(Mpx - 1, 1))
        if variant == "biased_running_var":
            unb = var.detach()
        res["running_mean"].append(c.rm0[i].to(D64) * (1 - c.momentum) + c.momentum * mean.detach())
        res["running_var"].append(c.rv0[i].to(D64) * (1 - c.momentum) + c.momentum * unb)
    res.update(out=out.detach(), act_e=None if act_e is None else act_e.detach(), nbt=1, inter=inter)
    tot = (out * c.dout.to(D64)).sum()
    if act_e is not None:
        tot = tot + (act_e * c.dact.to(D64)).sum()
    wanted = [xr] + Wl + gl + bl + w2l + [b for b in b2l if b is not None]
    gs = torch.autograd.grad(tot, wanted, allow_unused=True)
    gs = [torch.zeros_like(t) if g is None else g for g, t in zip(gs, wanted)]
    res["dx"] = gs[0].permute(0, 2, 3, 1).contiguous()
    res["dW"], res["dgamma"], res["dbeta"], res["dW2"] = (gs[1 + j * nb:1 + (j + 1) * nb] for j in range(4))
    it_b = iter(gs[1 + 4 * nb:])
    res["db2"] = [None if b is None else next(it_b) for b in b2l]
    return res


GRAD_KEYS = ("dx", "dW", "dgamma", "dbeta", "dW2", "db2")


def _dact_abs(c, i, valid):
    """|d act|+ at the object rows of branch i: |d out| |W2| on the valid rows."""
    d = c.dout.to(D64)[:, c.offs[i]:c.offs[i] + c.ks[i]].abs() * valid.to(D64).view(-1, 1)
    return d, d @ c.w2[i].to(D64).view(c.ks[i], -1).abs()


def ambiguous(c, ref):
    """[(branch, 'o' | 'e', row, channel)] of the elements whose activation side the fp32 recomputation may not reproduce (valid object rows and
    edge rows), and the number of (row, channel) pairs they are counted against."""
    _, _, _, valid = _coords(c)
    amb, total = [], 0
    for i, it in enumerate(ref["inter"]):
        live = ~((it["sc"] == 0) & (it["sh"] == 0))
        for kind in ("o", "e"):
            if "z_" + kind not in it:
                continue
            z, y = it["z_" + kind], it["y_" + kind]
            a = (z.abs() <= AMB_C * (y.abs() * it["sc"].abs() + it["sh"].abs())) & live
            if kind == "o":
                a = a & valid.view(-1, 1)
                total += int(valid.sum()) * z.shape[1]
            else:
                total += z.numel()
            amb += [(i, kind, int(r), int(ch)) for r, ch in a.nonzero().tolist()]
    return amb, total


def slack(c, ref, amb):
    """Per element of every gradient: what the ambiguous elements can move it by (the backward is linear in g = d act . act', so each element's
    other side shifts every sum by a fixed amount; the amounts add up)."""
    out = {k: ([torch.zeros_like(t) if t is not None else None for t in ref[k]] if isinstance(ref[k], list) else torch.zeros_like(ref[k]))
           for k in GRAD_KEYS}
    for a in amb:
        alt = reference(c, flips=(a,))
        for k in GRAD_KEYS:
            if isinstance(ref[k], list):
                for s, p, q in zip(out[k], alt[k], ref[k]):
                    if s is not None:
                        s += (p - q).abs()
            else:
                out[k] += (alt[k] - ref[k]).abs()
    return out


def magnitudes(c, ref):
    """M per quantity (see the module docstring), the fp16 operand-underflow floors, the number of 16-bit accumulations per d x pixel and the
    three disjoint d x regions."""
    dev = c.x.device
    x = c.x.to(D64)
    B, H, W, Cin = x.shape
    Mpx = B * H * W
    bi, cy, cx, valid = _coords(c)
    vf = valid.to(D64)
    nb = len(c.ks)
    xa = x.abs().permute(0, 3, 1, 2).clone().requires_grad_()
    wgt = torch.full((H + 2, W + 2), 2.0, dtype=D64, device=dev)                # the frame counts twice (added, then taken off again)
    wgt[1:-1, 1:-1] = 1.0
    # rows per pixel of the grown grid (valid objects; the edge rows of their branch)
    cnt_o = torch.zeros(B, H + 2, W + 2, dtype=D64, device=dev).index_put_((bi, cy + 1, cx + 1), vf, accumulate=True)
    cnt_e = torch.zeros_like(cnt_o)
    if c.extra is not None:
        eb, ey, ex = c.extra // (H * W), (c.extra // W) % H, c.extra % W
        cnt_e.index_put_((eb, ey + 1, ex + 1), torch.ones(c.extra.numel(), dtype=D64, device=dev), accumulate=True)
    M = dict(out=torch.zeros(c.rows.shape[0], c.ld, dtype=D64, device=dev), act_e=None, running_mean=[], running_var=[], dW=[], dgamma=[],
             dbeta=[], dW2=[], db2=[])
    eta = dict(dW=[])
    m_dx = torch.zeros_like(xa)
    e_dx = torch.zeros_like(xa)
    for i, it in enumerate(ref["inter"]):
        Wa = c.wt[i].to(c.dtype).to(D64).abs().requires_grad_()
        My_p = F.conv2d(xa, Wa, None, 1, 2)                                     # [B][C][H + 2][W + 2]: the image and its one-pixel frame
        Myd = My_p.detach()
        My = Myd[:, :, 1:-1, 1:-1]
        mean, rstd, sc, sh = it["mean"], it["rstd"], it["sc"], it["sh"]
        gam, bet = c.gam[i].to(D64), c.bet[i].to(D64)
        M_mean = (Myd * wgt).sum((0, 2, 3)) / Mpx
        M_var = (Myd * Myd * wgt).sum((0, 2, 3)) / Mpx + mean * mean
        M_rstd = rstd + 0.5 * rstd ** 3 * M_var
        M_sc = gam.abs() * M_rstd
        M_sh = bet.abs() + M_mean * sc.abs() + mean.abs() * M_sc
        My_o = My.permute(0, 2, 3, 1)[bi, cy, cx]
        Mz_o = My_o * sc.abs() + it["y_o"].abs() * M_sc + M_sh
        w2a = c.w2[i].to(D64).view(c.ks[i], -1).abs()
        mo = Mz_o @ w2a.t() + (0.0 if c.b2[i] is None else c.b2[i].to(D64).abs())
        M["out"][:, c.offs[i]:c.offs[i] + c.ks[i]] = mo * vf.view(-1, 1)
        M["running_mean"].append((1 - c.momentum) * c.rm0[i].to(D64).abs() + c.momentum * M_mean)
        M["running_var"].append((1 - c.momentum) * c.rv0[i].to(D64).abs() + c.momentum * M_var * (Mpx / max(Mpx - 1, 1)))
        # backward
        d_abs, da = _dact_abs(c, i, valid)
        der = lambda pos: torch.where(pos, torch.ones((), dtype=D64, device=dev), torch.full((), float(c.slope), dtype=D64, device=dev))   # noqa: E731
        g_o = da * der(it["pos_o"])
        Sg, Sgy = g_o.sum(0), (g_o * it["y_o"].abs()).sum(0)
        gy = torch.zeros_like(Myd)
        gy.permute(0, 2, 3, 1).index_put_((bi, cy + 1, cx + 1), g_o * sc.abs(), accumulate=True)
        if "z_e" in it:
            My_e = My.permute(0, 2, 3, 1).reshape(Mpx, -1)[c.extra]
            M["act_e"] = My_e * sc.abs() + it["y_e"].abs() * M_sc + M_sh
            g_e = c.dact.to(D64).abs() * der(it["pos_e"])
            Sg, Sgy = Sg + g_e.sum(0), Sgy + (g_e * it["y_e"].abs()).sum(0)
            gy.permute(0, 2, 3, 1).index_put_((eb, ey + 1, ex + 1), g_e * sc.abs(), accumulate=True)
        dsh_p = Sg
        dsc_p = Sgy + mean.abs() * Sg
        dvar_p = 0.5 * gam.abs() * rstd ** 3 * dsc_p
        ds1_p = (sc.abs() * dsh_p + 2 * mean.abs() * dvar_p) / Mpx
        ds2_p = dvar_p / Mpx
        M["dbeta"].append(dsh_p)
        M["dgamma"].append(dsc_p * M_rstd)
        M["dW2"].append(d_abs.t() @ Mz_o)
        M["db2"].append(None if c.b2[i] is None else d_abs.sum(0))
        M_dy = gy + wgt * (ds1_p.view(1, -1, 1, 1) + 2 * ds2_p.view(1, -1, 1, 1) * Myd)
        gx, gw = torch.autograd.grad(My_p, [xa, Wa], M_dy, retain_graph=True)    # conv_transpose(M_dy, |W|) and sum_px M_dy |patch| in one call
        m_dx += gx
        M["dW"].append(gw)
        cnt = cnt_o + (cnt_e if "z_e" in it else 0.0)
        ex_, ew = torch.autograd.grad(My_p, [xa, Wa], cnt.view(B, 1, H + 2, W + 2).expand_as(Myd))
        e_dx += ex_
        eta["dW"].append(ew * 2.0 ** -25)
    M["dx"] = m_dx.permute(0, 2, 3, 1).contiguous()
    eta["dx"] = (1.0 + e_dx.permute(0, 2, 3, 1)) * 2.0 ** -25
    cnt = (cnt_o + cnt_e).view(B, 1, H + 2, W + 2)
    win = F.conv2d(cnt, torch.ones(1, 1, 3, 3, dtype=D64, device=dev), None, 1, 1)[:, 0, 1:-1, 1:-1]      # windows that cover each pixel
    ring = torch.zeros(B, H, W, dtype=torch.bool, device=dev)
    ring[:, 0], ring[:, -1], ring[:, :, 0], ring[:, :, -1] = True, True, True, True
    n_acc = 1.0 + ring.to(D64) + win
    regions = dict(window=win > 0, ring=ring & ~(win > 0), interior=~ring & ~(win > 0))
    return dict(M=M, eta=eta, n_acc=n_acc, regions=regions)


def denominator(c, q, ref_t, M_t, n_acc=None, eta_t=None, grade=None):
    """u_op M + n_acc u_out |ref| + eta of one tensor of quantity q (without k)."""
    dt = grade or (c.dt if q in SIXTEEN else "fp32")
    uop, uout = U[dt]
    den = uop * M_t + uout * ref_t.abs() * (1.0 if n_acc is None else n_acc)
    if dt == "fp16" and q in SIXTEEN:
        den = den + (ETA["fp16"] if eta_t is None else eta_t)
    return den


def ratios(c, q, got, ref_t, M_t, n_acc=None, eta_t=None, slack_t=None, grade=None):
    """|got - ref| (less the ambiguity slack) over the denominator, per element; 0 where they agree exactly, inf where the model allows nothing."""
    d = (got.to(D64) - ref_t).abs()
    if slack_t is not None:
        d = (d - slack_t).clamp(min=0)
    den = denominator(c, q, ref_t, M_t, n_acc, eta_t, grade)
    rt = torch.where(d == 0, torch.zeros_like(d), d / den.clamp(min=1e-300))
    return torch.nan_to_num(rt, nan=float("inf"), posinf=float("inf"))                    # a NaN in the result misses every bound


FORWARD_KEYS = ("out", "act_e", "running_mean", "running_var")


def score(c, got, ref, mag, slk=None, grade=None):
    """{quantity: worst ratio}, with d x also per region ('dx/window', 'dx/ring', 'dx/interior'; None for an empty region).  `got` holds the
    node's results under the reference's keys (lists per branch where the reference has lists)."""
    M, eta = mag["M"], mag["eta"]
    res = {}
    for q in FORWARD_KEYS + (() if c.forward_only else GRAD_KEYS):
        if ref[q] is None:
            continue
        rs, gs, ms = (t if isinstance(t, list) else [t] for t in (ref[q], got[q], M[q]))
        es = eta[q] if q == "dW" else [eta.get(q)] * len(rs)
        ss = [None] * len(rs) if (slk is None or q not in slk) else (slk[q] if isinstance(slk[q], list) else [slk[q]])
        worst = 0.0
        for r_, g_, m_, e_, s_ in zip(rs, gs, ms, es, ss):
            if r_ is None:
                continue
            na = mag["n_acc"].unsqueeze(-1) if q == "dx" else None
            rt = ratios(c, q, g_.reshape(r_.shape), r_, m_, na, e_, s_, grade)
            worst = max(worst, float(rt.max()) if rt.numel() else 0.0)
            if q == "dx":
                for name, mask in mag["regions"].items():
                    res["dx/" + name] = float(rt[mask].max()) if bool(mask.any()) else None
        res[q] = worst
    return res
