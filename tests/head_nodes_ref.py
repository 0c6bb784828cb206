"""float64 restatements of the heads' fused training nodes (autograd.FanOutConvFn / HeadConvGatherFn / EdgeScatterAddFn), their error model and
the case builders of tests/test_gpu_head_nodes.py.  Plain torch on the CPU; nothing here imports the library's kernels (the edge case builder
calls detector_predictor.make_edge_rowmap, which is index arithmetic in torch).

Operands are taken as the kernels see them: activations and upstream gradients already lie on the mode's 16-bit grid, weights are rounded with
.to(dtype) in the 16-bit modes (`round_w`) and used as they are in fp32, biases stay fp32.

Error model (every bound is derived, none is measured):
  * the product of two 16-bit operands is exact in fp32; an fp32 product of fp32 operands rounds once, which the n below already counts
    (n - 1 adds and one product per term);
  * an fp32 accumulation of n terms in any order (split-K, atomics, a reduce pass) errs by at most n 2^-24 sum|terms|;
  * every store rounds once: u_out |value|, u_out = 2^-8 (bf16), 2^-11 (fp16), 2^-24 (fp32) -- the unit roundoff 2^-p of a type with p
    significant bits (8, 11, 24); an fp16 store also adds 2^-25 (half of the subnormal spacing).  (2^-9 for bf16 is provably too tight: round
    to nearest errs by up to half an ulp = 2^(e-8) at |value| = 2^e (1 + 2^-8), a relative 2^-8; the CPU simulation of the two-rounding form in
    test_head_nodes_ref_cpu.py reaches 1.58x of a 2^-9 bound.)
  * the total is multiplied by 1 + 2^-6 for the second-order terms (a rounding of a value that already carries an error; the fp32 add of the
    residual before a 16-bit store: 2^-24 against 2^-6 u_out >= 2^-17).
"""
import torch
import torch.nn.functional as F

D64 = torch.float64
DTYPES = {"fp32": torch.float32, "bf16": torch.bfloat16, "fp16": torch.float16}
U32 = 2.0 ** -24
U_OUT = {"fp32": 2.0 ** -24, "bf16": 2.0 ** -8, "fp16": 2.0 ** -11}
ETA = {"fp32": 0.0, "bf16": 0.0, "fp16": 2.0 ** -25}
BITS = {"fp32": 24, "bf16": 8, "fp16": 11}          # significant bits: ulp(v) = 2^(floor(log2 |v|) - BITS + 1)
SECOND = 1.0 + 2.0 ** -6


def on_grid(t, mode):
    """float64 copy of `t` rounded once to the mode's activation type."""
    return t.to(DTYPES[mode]).to(D64)


def round_w(w, mode):
    """A weight as the packed operand holds it: rounded in the 16-bit modes, untouched in fp32."""
    return w.to(D64) if mode == "fp32" else w.to(DTYPES[mode]).to(D64)


def ulp(v, mode):
    """Spacing of the mode's activation type at |v| (float64 tensor, v != 0, normal range)."""
    _, e = torch.frexp(v.abs())                     # |v| = m 2^e, m in [0.5, 1)
    return torch.ldexp(torch.ones_like(v), e - BITS[mode])


# ---- bounds -------------------------------------------------------------------------------------------------------------------------------------

def bound_sum(n, mag):
    """An fp32 sum of n terms with sum|terms| = mag, kept in fp32 (weight and bias gradients)."""
    return SECOND * n * U32 * mag


def bound_out(n, mag, ref, mode, u_out=None):
    """The same sum stored once with unit roundoff u_out (default: the mode's activation type)."""
    u = U_OUT[mode] if u_out is None else u_out
    eta = ETA[mode] if u_out is None else 0.0
    return SECOND * (n * U32 * mag + u * ref.abs() + eta)


def bound_chain(K, mags, sums, mode):
    """dx of the fan-out: one fp32 accumulation of K terms and one store per link, the previous link's value added in fp32 before the store."""
    tot = torch.zeros_like(sums[0])
    for M, S in zip(mags, sums):
        tot = tot + K * U32 * M + U_OUT[mode] * S.abs() + ETA[mode]
    return SECOND * tot


def bound_gather_df(r, mode):
    """df of HeadConvGatherFn: at most TWO roundings of the output type at any pixel (the data-gradient conv's store and one more after the
    arriving rows were summed in fp32), however many rows land on it."""
    return SECOND * (U_OUT[mode] * (r["df_conv"].abs() + r["df_total"].abs()) + 2 * ETA[mode]
                     + U32 * (r["cpad"] * r["M_conv"] + r["n_p"].unsqueeze(-1) * r["sum_abs_de"]))


def ratio(got, ref, bound):
    """Worst |got - ref| / bound over the tensor (0 / 0 counts as 0: an exact zero that came out as zero)."""
    err = (got.to(D64) - ref).abs()
    q = torch.where(err == 0, torch.zeros_like(err), err / bound.expand_as(err).clamp_min(1e-300))
    return float(q.max()) if q.numel() else 0.0


# ---- restatements -------------------------------------------------------------------------------------------------------------------------------

def _nchw(t):
    return t.permute(0, 3, 1, 2)


def _nhwc(t):
    return t.permute(0, 2, 3, 1).contiguous()


def fanout_ref(x, weights, pad, dys):
    """x (B, H, W, C) float64 NHWC, weights OIHW float64 (already rounded), dys NHWC float64 or None per weight.
    -> dict: y[i], M[i] = conv(|x|, |w_i|); dw[i], dw_mag[i] = sum |x| |dy| (None where dy is None); links = the indices whose dy is not None, in
    weight order; dgrad[j], dgrad_mag[j] per link; S[j] = the running sum of the data gradients up to and including link j (the node rounds once
    per link)."""
    xn, xa = _nchw(x), _nchw(x.abs())
    r = dict(y=[], M=[], dw=[], dw_mag=[], links=[], dgrad=[], dgrad_mag=[], S=[])
    run = None
    for i, (w, dy) in enumerate(zip(weights, dys)):
        r["y"].append(_nhwc(F.conv2d(xn, w, padding=pad)))
        r["M"].append(_nhwc(F.conv2d(xa, w.abs(), padding=pad)))
        if dy is None:
            r["dw"].append(None); r["dw_mag"].append(None)
            continue
        g = _nchw(dy)
        r["dw"].append(torch.nn.grad.conv2d_weight(xn, w.shape, g, padding=pad))
        r["dw_mag"].append(torch.nn.grad.conv2d_weight(xa, w.shape, g.abs(), padding=pad))
        d = _nhwc(F.conv_transpose2d(g, w, padding=pad))
        r["links"].append(i)
        r["dgrad"].append(d)
        r["dgrad_mag"].append(_nhwc(F.conv_transpose2d(g.abs(), w.abs(), padding=pad)))
        run = d if run is None else run + d
        r["S"].append(run)
    return r


def head_conv_gather_ref(f, w, b, rowmap, dy, de):
    """f (B, H, W, C), w (Cout, C, 1, 1) rounded, b (Cout,) or None, rowmap long [R], dy (B, H, W, cpad) with zero padded channels, de (R, C);
    all float64.  -> dict: y (cpad channels, the padded ones zero), y_mag, e, df_conv, M_conv, df_total = df_conv + the rows of de added at
    their pixels with multiplicity, n_p (pixels,) rows per pixel, sum_abs_de (pixels, C), dw / dw_mag, db / db_mag, cpad."""
    B, H, W, C = f.shape
    Cout, cpad = w.shape[0], dy.shape[-1]
    w2 = w.reshape(Cout, C)
    f2, g = f.reshape(-1, C), dy.reshape(-1, cpad)[:, :Cout]
    y = f2 @ w2.t() + (b if b is not None else 0.0)
    r = dict(cpad=cpad)
    r["y"] = F.pad(y, (0, cpad - Cout)).view(B, H, W, cpad)
    r["y_mag"] = F.pad(f2.abs() @ w2.abs().t(), (0, cpad - Cout)).view(B, H, W, cpad)
    r["e"] = f2.index_select(0, rowmap)
    r["df_conv"] = g @ w2
    r["M_conv"] = g.abs() @ w2.abs()
    r["df_total"] = r["df_conv"] + torch.zeros_like(f2).index_add_(0, rowmap, de)
    r["n_p"] = torch.bincount(rowmap, minlength=f2.shape[0]).to(D64)
    r["sum_abs_de"] = torch.zeros_like(f2).index_add_(0, rowmap, de.abs())
    r["dw"], r["dw_mag"] = (g.t() @ f2).view_as(w), (g.abs().t() @ f2.abs()).view_as(w)
    r["db"], r["db_mag"] = (g.sum(0), g.abs().sum(0)) if b is not None else (None, None)
    return r


def edge_scatter_ref(base, o, edge_xy, edge_len, lo, rows, valid, g):
    """out = base with o[b, l] added to channels [lo, lo + co) of pixel edge_xy[b, l], l < edge_len[b] (a loop: independent of rows / valid);
    dbase = g; do = the rows of g at `rows`, channels [lo, lo + co), times `valid`.  float64."""
    B, L, co = o.shape
    out = base.clone()
    for b in range(B):
        for l in range(int(edge_len[b])):
            x, y = int(edge_xy[b, l, 0]), int(edge_xy[b, l, 1])
            out[b, y, x, lo:lo + co] += o[b, l]
    do = g.reshape(-1, g.shape[-1]).index_select(0, rows)[:, lo:lo + co].reshape(B, L, co) * valid
    return out, g.clone(), do


# ---- cases --------------------------------------------------------------------------------------------------------------------------------------

def border_points(H, W):
    """The border of an H x W map, clockwise from (0, 0), every pixel once: 2 (H + W) - 4 points (x, y)."""
    return ([(x, 0) for x in range(W)] + [(W - 1, y) for y in range(1, H)] + [(x, H - 1) for x in range(W - 2, -1, -1)]
            + [(0, y) for y in range(H - 2, 0, -1)])


def edge_case(B, H, W, Lmax, edge_len, halo, start=0):
    """Unique border points in the first edge_len[b] positions of image b, zeros after (the reference's padded edge_indices); Lmax may exceed the
    border, so padding rows exist.  -> dict(ei int32 [B, Lmax, 2], el int32 [B], rowmap / rows_center long, valid_l float [B, Lmax, 1])."""
    from monoflex_amd.model.head.detector_predictor import make_edge_rowmap
    border = border_points(H, W)
    assert len(edge_len) == B and max(edge_len) <= min(Lmax, len(border))
    ei = torch.zeros(B, Lmax, 2, dtype=torch.int32)
    for b, n in enumerate(edge_len):
        if n:
            ei[b, :n] = torch.tensor([border[(start + 3 * b + i) % len(border)] for i in range(n)], dtype=torch.int32)
    el = torch.tensor(edge_len, dtype=torch.int32)
    rm = make_edge_rowmap(ei, H, W, halo).long()
    Lp = Lmax + 2 * halo
    return dict(ei=ei, el=el, halo=halo, Lp=Lp, rowmap=rm, rows_center=rm.view(B, Lp)[:, halo:Lmax + halo].reshape(-1).contiguous(),
                valid_l=(torch.arange(Lmax).view(1, Lmax) < el.view(B, 1)).to(D64).unsqueeze(-1))


FANOUT_CIN, FANOUT_COUT = 64, 256
FANOUT_CASES = [(2, 12, 20, 9), (1, 13, 37, 2), (1, 13, 37, 1)]


def fanout_case(B, H, W, n, mode, seed=11):
    """x and the n upstream gradients ~ N(0, 1) on the mode's grid, fp32 weights ~ N(0, 1) / 24 (fan-in 576: unit-scale outputs).  float64 /
    fp32 CPU tensors: dict(x, w32 [fp32 OIHW], w [rounded float64], dy)."""
    gen = torch.Generator().manual_seed(seed + 131 * n + H)
    x = on_grid(torch.randn(B, H, W, FANOUT_CIN, generator=gen), mode)
    w32 = [torch.randn(FANOUT_COUT, FANOUT_CIN, 3, 3, generator=gen) / 24.0 for _ in range(n)]
    dy = [on_grid(torch.randn(B, H, W, FANOUT_COUT, generator=gen), mode) for _ in range(n)]
    return dict(x=x, w32=w32, w=[round_w(w, mode) for w in w32], dy=dy)


GATHER_C = 256
GATHER_MAP = (3, 6, 10)
GATHER_LMAX = 96
GATHER_EDGE_LEN = [0, 28, 7]                  # none, the whole border of a 6 x 10 map, a few
GATHER_HALOS = (0, 1, 3)
GATHER_HEADS = [(3, True), (2, True), (8, True), (20, True), (3, False)]       # (Cout, bias)
TEETH_PIXEL = 0                               # flat pixel (0, 0) of image 0, whose edge_len is 0: every sequence position of that image lands on it


def cpad_of(cout, mode):
    """autograd's output-channel padding of a training conv (packing._pad_channels), restated."""
    e = 4 if mode == "fp32" else 8
    return (cout + 63) // 64 * 64 if cout >= 64 else max(e, 1 << (cout - 1).bit_length())


def gather_case(cout, bias, halo, mode, seed=23):
    """The HeadConvGatherFn case: f ~ N(0, 1), w ~ N(0, 1) / 16 (fan-in 256), b ~ N(0, 1), the gradient of y[..., :Cout] ~ N(0, 1) except +-8 at
    TEETH_PIXEL (so that df_conv there is of unit scale), de ~ N(0, 1) / 4 -- all on the mode's grid.

    The teeth: on the aligned 8-channel chunk of TEETH_PIXEL whose smallest |df_conv| (rounded to the output type: v) is largest, every row that
    lands on the pixel carries sign(v) ulp(v) / 4.  Each such addend is below half an ulp of the running value, so an implementation that rounds
    to the output type after every row loses all n_p of them: n_p / 4 ulp, against a bound of about one ulp.  -> dict with float64 / fp32 CPU
    tensors and `chunk` (first channel of the teeth chunk)."""
    B, H, W = GATHER_MAP
    C = GATHER_C
    gen = torch.Generator().manual_seed(seed + 17 * cout + 3 * halo + int(bias))
    edges = edge_case(B, H, W, GATHER_LMAX, GATHER_EDGE_LEN, halo)
    f = on_grid(torch.randn(B, H, W, C, generator=gen), mode)
    w32 = torch.randn(cout, C, 1, 1, generator=gen) / 16.0
    b32 = torch.randn(cout, generator=gen) if bias else None
    ry = on_grid(torch.randn(B, H, W, cout, generator=gen), mode)
    ry[0, 0, 0] = 8.0 * torch.where(torch.rand(cout, generator=gen) < 0.5, -1.0, 1.0).to(D64)
    de = on_grid(torch.randn(B * edges["Lp"], C, generator=gen) / 4.0, mode)
    w = round_w(w32, mode)
    v = on_grid(ry[0, 0, 0] @ w.reshape(cout, C), mode)                       # df_conv at the pixel as the data-gradient conv stores it
    chunk = 8 * int(v.abs().view(C // 8, 8).min(1).values.argmax())
    vc = v[chunk:chunk + 8]
    assert float(vc.abs().min()) >= 0.25, "teeth chunk: |df_conv| below 1/4 (a quarter ulp would leave fp16's normal range)"
    hit = edges["rowmap"] == TEETH_PIXEL
    assert int(hit.sum()) == edges["Lp"]
    de[hit, chunk:chunk + 8] = (torch.sign(vc) * ulp(vc, mode) / 4.0).expand(int(hit.sum()), 8)
    assert torch.equal(on_grid(de, mode), de)
    dy = F.pad(ry, (0, cpad_of(cout, mode) - cout))
    return dict(edges=edges, f=f, w32=w32, w=w, b32=b32, b=b32.to(D64) if bias else None, ry=ry, dy=dy, de=de, chunk=chunk, v=v)


def per_row_rounding(case, ref, mode, pixel=TEETH_PIXEL):
    """What `dx.index_add_(0, rowmap, de.to(dtype))` on a 16-bit dx produces at `pixel`: the float64 df_conv rounded once, then the rows added one
    at a time in rowmap order with a rounding to the output type after each add."""
    td = DTYPES[mode]
    acc = ref["df_conv"][pixel].to(td)
    for j in (case["edges"]["rowmap"] == pixel).nonzero().flatten().tolist():
        acc = (acc.to(D64) + case["de"][j]).to(td)
    return acc.to(D64)


def summed_then_rounded(case, ref, mode, pixel=TEETH_PIXEL):
    """The two-rounding form at `pixel`: the rows summed in fp32 (here: in rowmap order), added to the stored df_conv in fp32, rounded once."""
    td = DTYPES[mode]
    s = torch.zeros(case["de"].shape[1], dtype=torch.float32)
    for j in (case["edges"]["rowmap"] == pixel).nonzero().flatten().tolist():
        s = s + case["de"][j].float()
    return (ref["df_conv"][pixel].to(td).float() + s).to(td).to(D64)


SCATTER_CFGS = [(0, 3, 3), (0, 2, 2), (4, 2, 7)]               # (lo, co, cb)


def scatter_case(lo, co, cb, seed=31):
    """base (fp32 values), o and g on the grid common to bf16 and fp16 (multiples of 1/8 up to 4), a wider map for the sliced base."""
    B, H, W = GATHER_MAP
    gen = torch.Generator().manual_seed(seed + 7 * lo + co)
    edges = edge_case(B, H, W, GATHER_LMAX, GATHER_EDGE_LEN, 1)
    k8 = lambda *s: torch.randint(-32, 33, s, generator=gen).to(D64) / 8.0                       # noqa: E731
    wide = torch.randn(B, H, W, cb + 1, generator=gen).float()
    return dict(edges=edges, wide=wide, base=wide[..., :cb].contiguous().to(D64), o=k8(B, GATHER_LMAX, co), g=k8(B, H, W, cb))
