"""tests/gram_heads_ref.py without a device: (1) the float64 restatement agrees with GramRegHeadsFn (fp32, CPU, the library launches swapped for
torch as in test_gram_heads_cpu) inside the fp32-grade error model; (2) every GPU case's inputs keep the ambiguous activation sides under the
cap and the regions the case table promises; (3) TEETH -- for the GPU cases' inputs, deliberately wrong references miss the bound of
test_gpu_gram_heads_oracle (its K, the case's widest 16-bit type first) by at least a factor of two:

    (a) d x and d W with the batch statistics as constants: on the pixels outside every window (against K_OUTSIDE, the k of those regions,
        and against K["dx"] too on the cases that must have >= 100 interior pixels), and on d W (whose difference is exactly the
        d s1 (x) m + 2 d s2 W G part)          (b) d W of the extra branch without the edge rows          (c) running_var from the biased variance
    (d) coincident object rows counted once     (e) d x with border patches read from a replicate-padded map
    (f) d gamma without - mean d sh (fp32 grade) (g) `out` with a ReLU where the case asks for leaky (fp32 grade)

Each tooth is asserted on EVERY case that has the feature (TEETH below); on the cases that must have >= 100 interior pixels, (a) is asserted on
the interior pixels specifically -- the ones the 5x5 conv produces alone.  The offset case's shift is chosen so that this holds: at the shift
x + 1.5, W + 0.01 (mean^2 / var ~ 26 .. 40) M's |d s1|+ and |d s2|+, which add the two cancelling terms of d mean, widen the bf16 bounds until
(a) reaches 0.008 of the bound on d x and (d) 0.17 / 0.14 on d x / d W; at mean^2 / var ~ 3.4 with five coincident objects they reach 2.4 k
(interior), 2.2 k (d W), 7.8 k and 4.5 k.  The large shift lives on as the forward-only case offset_fwd, where (c) and (g) bite."""
import functools

import pytest
import torch

import gram_heads_ref as R
from test_gram_heads_cpu import patch_library_launches
from test_gpu_gram_heads_oracle import K, K_OUTSIDE

# reference against the fp32 torch node: twice the worst ratio observed over the three small cases, per quantity (observed beside it)
K_TORCH = {"out": 0.25,            # 0.124 base
           "act_e": 0.53,          # 0.262 base
           "running_mean": 0.62,   # 0.309 single
           "running_var": 0.89,    # 0.442 single
           "dx": 1.6,              # 0.762 single (window; ring 0.164, interior 0.213)
           "dW": 2.2,              # 1.06  single
           "dgamma": 0.39,         # 0.194 single
           "dbeta": 1.6,           # 0.776 base
           "dW2": 1.2,             # 0.579 base
           "db2": 1.5}             # 0.750 base
OUTSIDE = ("dx/ring", "dx/interior")
# tooth -> (variant, {quantity or region group: cases it must bite on})
_ALL = tuple(n for n in R.CASES if n != "empty" and n not in R.FORWARD_ONLY)          # cases with gradients
_EDGE = ("base", "relu", "scaled_up", "scaled_down", "single", "empty_edge", "eight", "offset")
_COINCIDENT = ("base", "relu", "scaled_up", "scaled_down", "ragged", "offset")
_ROWS = tuple(n for n in R.CASES if n not in ("empty", "empty_edge"))                  # cases with valid object rows
TEETH = {
    "a": ("const_stats", {"outside": tuple(n for n in _ALL if n not in R.NEEDS_INTERIOR), "interior": R.NEEDS_INTERIOR,
                          "interior_k_dx": ("base", "relu", "scaled_up", "scaled_down"), "dW": _ALL}),
    "b": ("no_edge_dw", {"dW": _EDGE}),
    "c": ("biased_running_var", {"running_var": R.CASES}),
    "d": ("dedupe", {"dx": _COINCIDENT, "dW": _COINCIDENT}),
    "e": ("replicate", {"dx": _ALL}),
    "f": ("no_mean_dsh", {"dgamma": _ALL}),
    "g": ("relu_out", {"out": tuple(n for n in _ROWS if n != "relu")}),
}


@functools.lru_cache(maxsize=None)
def _case(dt, name):
    c = R.make_case(name, dt)
    ref = R.reference(c)
    return c, ref, R.magnitudes(c, ref)


def _run_torch_node(c):
    from monoflex_amd import gram_heads as GH, lib as L
    from monoflex_amd.model.head.detector_predictor import InPlaceABN
    C = c.wt[0].shape[0]
    abns = []
    for i in range(len(c.ks)):
        h = InPlaceABN(C)
        with torch.no_grad():
            h.weight.copy_(c.gam[i]); h.bias.copy_(c.bet[i]); h.running_mean.copy_(c.rm0[i]); h.running_var.copy_(c.rv0[i])
        abns.append(h)
    xd = c.x.clone().requires_grad_()
    wtd = [w.clone().requires_grad_() for w in c.wt]
    wd = [w.clone().requires_grad_() for w in c.w2]
    bd = [None if b is None else b.clone().requires_grad_() for b in c.b2]
    out, ae = GH.gram_reg_heads(xd, c.rows, abns, c.offs, c.ld, wtd, [h.weight for h in abns], [h.bias for h in abns], wd, bd, sync=False,
                                extra_branch=c.extra_branch, extra_rows=c.extra, act=L.ACT_RELU if c.slope == 0.0 else L.ACT_LEAKY)
    if ae is None:
        torch.autograd.backward([out], [c.dout])
    else:
        torch.autograd.backward([out, ae], [c.dout, c.dact])
    d = lambda t: None if t is None else t.detach().double()          # noqa: E731
    return dict(out=d(out), act_e=d(ae), dx=d(xd.grad), dW=[d(w.grad) for w in wtd], dgamma=[d(h.weight.grad) for h in abns],
                dbeta=[d(h.bias.grad) for h in abns], dW2=[d(w.grad) for w in wd], db2=[None if b is None else d(b.grad) for b in bd],
                running_mean=[d(h.running_mean) for h in abns], running_var=[d(h.running_var) for h in abns]), [int(h.num_batches_tracked) for h in abns]


@pytest.mark.parametrize("name", ["base", "ragged", "single"])
def test_reference_agrees_with_the_fp32_torch_node(monkeypatch, name):
    """Every quantity inside the fp32-grade model (u_op = u_out = 2^-24 on all of them) at a small non-kernel size: Cin 8, C 16."""
    patch_library_launches(monkeypatch)
    c = R.make_case(name, "fp32", C=16, Cin=8)
    ref = R.reference(c)
    mag = R.magnitudes(c, ref)
    amb, _ = R.ambiguous(c, ref)
    got, nbt = _run_torch_node(c)
    sc = R.score(c, got, ref, mag, R.slack(c, ref, amb) if amb else None, grade="fp32")
    print(name, {k: (None if v is None else round(v, 4)) for k, v in sc.items()})
    assert nbt == [1] * len(c.ks)
    bad = {q: (v, K_TORCH.get(q, 0.0)) for q, v in sc.items() if "/" not in q and not v <= K_TORCH.get(q, 0.0)}
    assert not bad, bad


@pytest.mark.parametrize("dt,name", R.case_list())
def test_every_gpu_case_keeps_the_ambiguity_cap_and_its_regions(dt, name):
    c, ref, mag = _case(dt, name)
    amb, total = R.ambiguous(c, ref)
    assert len(amb) <= R.AMB_CAP * max(total, 1), (len(amb), total)
    regions = {k: int(v.sum()) for k, v in mag["regions"].items()}
    assert sum(regions.values()) == c.x.shape[0] * c.x.shape[1] * c.x.shape[2]
    if name in R.NEEDS_INTERIOR:
        assert regions["interior"] >= 100, regions
    if name in ("base", "relu"):                                  # the degenerate channels are what they are meant to be
        for it in ref["inter"]:
            assert float(it["var"][0]) == 0.0 and float(it["sc"][1]) == 0.0 and float(it["sh"][1]) == 0.0 and float(it["sc"][2]) < 0
            assert float(it["z_o"][:, 1].abs().max()) == 0.0
    if name == "offset":
        assert all(float((it["mean"] ** 2 / it["var"]).median()) > 3 for it in ref["inter"])
        assert int((torch.as_tensor(c.rows[:, [57, 3, 2]]) == c.rows[5, [57, 3, 2]]).all(1).sum()) == 5          # five objects on one pixel
    if name == "offset_fwd":
        assert all(float((it["mean"] ** 2 / it["var"]).median()) > 20 for it in ref["inter"])
    if amb:                                                       # the slack is what the other side moves: the gradients through act', while
        slk = R.slack(c, ref, amb)                                # d W2 only sees the value of act, which is continuous at z = 0
        assert float(slk["dx"].max()) > 0
        assert all(bool((s <= R.AMB_C * m).all()) for s, m in zip(slk["dW2"], mag["M"]["dW2"]))          # (|z| is within its own bound of 0)


def _wrong(c, ref, variant):
    if variant != "no_mean_dsh":
        return R.reference(c, variant=variant)
    w = dict(ref)                                                 # d gamma = (d sc - mean d sh) rstd without its second term
    w["dgamma"] = [g + it["mean"] * db * it["rstd"] for g, db, it in zip(ref["dgamma"], ref["dbeta"], ref["inter"])]
    return w


@pytest.mark.parametrize("tooth", sorted(TEETH))
def test_wrong_references_miss_the_bounds_by_a_factor_of_two(tooth):
    variant, where = TEETH[tooth]
    seen, bad = {}, {}
    for dt, name in R.case_list():
        c, ref, mag = _case(dt, name)
        sc = R.score(c, _wrong(c, ref, variant), ref, mag)
        for q, cases in where.items():
            if c.forward_only and q not in R.FORWARD_KEYS:
                continue
            if q == "outside":
                v, k = max(((sc[r] or 0.0) / K_OUTSIDE[dt][r], r) for r in OUTSIDE)          # the region that misses its own k by most
                v, k = v * K_OUTSIDE[dt][k], K_OUTSIDE[dt][k]
            elif q == "interior":                                 # the pixels the 5x5 conv produces alone
                v, k = sc["dx/interior"], K_OUTSIDE[dt]["dx/interior"]
            elif q == "interior_k_dx":
                v, k = sc["dx/interior"], K[dt]["dx"]
            else:
                v, k = sc[q], K[dt][q]
            seen[(dt, name, q)] = round(v / k, 2) if k else None
            if name in cases and not v >= 2.0 * k:
                bad[(dt, name, q)] = (v, k)
    print(tooth, variant, seen)
    assert not bad, bad


def _d_beta_in_plain_fp32(c, ref):
    """d beta = sum_rows (d out . W2) act' evaluated in fp32, one term at a time, as gram_rows_bwd_kernel's loops do (no atomics)."""
    valid = (c.rows[:, 0] > 0).float().view(-1, 1)
    res = []
    for i, it in enumerate(ref["inter"]):
        dd, w2 = c.dout[:, c.offs[i]:c.offs[i] + c.ks[i]] * valid, c.w2[i].view(c.ks[i], -1)
        da = torch.zeros(dd.shape[0], w2.shape[1])
        for k in range(c.ks[i]):
            da = da + dd[:, k:k + 1] * w2[k:k + 1]
        der = lambda pos: torch.where(pos, torch.tensor(1.0), torch.tensor(float(c.slope)))          # noqa: E731
        g = da * der(it["pos_o"])
        if "pos_e" in it:
            g = torch.cat((g, c.dact.float() * der(it["pos_e"])))
        s = torch.zeros(w2.shape[1])
        for r in range(g.shape[0]):
            s = s + g[r]
        res.append(s.double())
    return res


def test_the_d_beta_constant_is_what_plain_fp32_arithmetic_needs():
    """K's d beta (4.1 / 4.2, observed 2.02 / 2.06 on the device) is the largest of the table and sits at the 'about 4' above which an error is not
    rounding.  Shown here, not argued: the same chain -- up to 20 products per (row, channel), then the sum over the rows -- evaluated in plain
    fp32 on the CPU misses float64 by 2.02 (base), 1.78 (eight), 0.72 (ragged) of 2^-24 sum |d out| |W2| -- the device's own figures for these
    cases to three digits: the kernel's error IS that of the fp32 chain.  M's d beta term has no count of terms; the count is what k holds."""
    seen = {}
    for dt, name in (("bf16", "base"), ("bf16", "eight"), ("bf16", "ragged"), ("fp16", "scaled_down")):
        c, ref, mag = _case(dt, name)
        got = _d_beta_in_plain_fp32(c, ref)
        seen[name] = max(float(R.ratios(c, "dbeta", g, r, m).max()) for g, r, m in zip(got, ref["dbeta"], mag["M"]["dbeta"]))
    print(seen)
    assert 1.5 <= seen["base"] <= K["bf16"]["dbeta"] and 1.3 <= seen["eight"] <= K["bf16"]["dbeta"], seen
    assert 1.0 <= seen["scaled_down"] <= K["fp16"]["dbeta"] and 0.5 <= seen["ragged"] <= 2.0, seen
