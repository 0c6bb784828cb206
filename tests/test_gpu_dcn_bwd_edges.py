"""The tile-owned DCN backward (monoflex_amd/csrc/dcn_bwd_tile.hip) pinned per element to float64 at its list and ring limits.

mfx_dcn_backward_v2_rt is called directly on the engineered offset fields of tests/dcn_bwd_cases.py, so every (sample, tap, corner) pair sits where
the census of tests/dcn_bwd_ref.py says it does: at exactly D and D + 1 pixels from its corner's tile, past the capacity of a pixel's LDS list (62
entries for 16-bit maps, 47 for fp32), past the 512 entries of a workgroup's far stage, in the ragged part of an edge tile, on the border band and
on the exact coordinates -1 / H.  tests/test_dcn_bwd_ref_cpu.py proves the census conditions and pins the reference to the C oracle.

Every output is pre-filled with NaN and compared element by element:  |got - ref| <= k (u_op M + u_out |ref|),  M = the same sum over absolute
values; grad_input adds  n_atomic(p) u_out M(p)  for the arrival-order rounding of the packed 16-bit atomics (n_atomic from the census: far pairs
plus pairs beyond the list capacity; zero in deterministic mode, whose fixed-point sum has no order).  u_op / u_out = 2^-8 / 2^-9 (bf16), 2^-11 (fp16),
2^-24 (fp32); d_raw rows written as fp32 take u_out = 2^-24.  The inputs are exact in every type, so nothing but the kernels' own rounding is left.

Forms (options; each proved by its dispatch-counter delta): fly1 = gcol-free tile and far kernels, fly2 = fused sample kernel writes d(columns) for
the second-generation tile kernel, fused = fused sample kernel behind a d(columns) GEMM, unfused = five launches (also fp32, the wide layers with
64- and 128-channel slices, and the 9 x 17 map), det = option `deterministic` (64-bit fixed-point grad_input; two calls must agree bit for bit).

k (K below) is twice the worst ratio measured on MI355X per (form, type, output), rounded up to one significant digit -- arrival order moves the
worst element from run to run; an output that came out exact takes the floor 0.02 (there is no spread to double).  The measured values are in
profiles/dcn_bwd_edges.md and, for the current run, in dcn_bwd_edges.json under $MFX_REPORT_DIR (default: the git-ignored artifacts/).  Whatever is
measured: k <= 8 for the 16-bit types, and k <= 2 (Cout + pairs per pixel) for fp32 (test_k_is_within_its_conditions).

Teeth: a deliberately wrong reference must miss the bound by at least 2x at some element -- (a) grad_input without the pairs beyond the list capacity
at the focus pixels, (b) with the pairs of samples exactly D + 1 pixels from a tile counted by both routes, (c) d_raw with a non-strict `inside` (a
sample at exactly -1 gets an offset gradient), (d) grad_input without the own-sample corners in the ragged part of an edge tile."""
import ctypes
import functools
import json
import os

import pytest
import torch

import dcn_bwd_cases as CS
import dcn_bwd_ref as R

pytestmark = pytest.mark.gpu
DEV = "cuda"
D64 = torch.float64
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
REPORT_DIR = os.environ.get("MFX_REPORT_DIR") or os.path.join(ROOT, "artifacts")
CONSTS = R.kernel_constants()
DT = {"bf16": torch.bfloat16, "fp16": torch.float16, "fp32": torch.float32}
U = {"bf16": (2.0 ** -8, 2.0 ** -9), "fp16": (2.0 ** -11, 2.0 ** -11), "fp32": (2.0 ** -24, 2.0 ** -24)}
OUTPUTS = ("dx", "d_raw", "dw", "db")
DEFAULTS = {"dcn_bt_fly": 1, "dcn_bt_fuse_wgrad": 1, "dcn_bt_fuse_min_chunks": 1024, "dcn_bt_cs": 0, "deterministic": 0}
COUNTERS = ("dcn_bt_fused", "dcn_bt_fly", "dcn_bt_tile", "dcn_bt_far", "dcn_bt_sample")
# form -> (options, expected counter deltas, list capacity of the 16-bit tile kernel it runs, d_raw rows in the activation type)
FORMS = {
    "fly1": (dict(dcn_bt_fly=1, dcn_bt_fuse_wgrad=1, dcn_bt_fuse_min_chunks=1), dict(dcn_bt_fused=1, dcn_bt_fly=1, dcn_bt_tile=0, dcn_bt_far=1, dcn_bt_sample=0), "FZ_LCAP", 1),
    "fly2": (dict(dcn_bt_fly=2, dcn_bt_fuse_wgrad=1, dcn_bt_fuse_min_chunks=1), dict(dcn_bt_fused=1, dcn_bt_fly=1, dcn_bt_tile=1, dcn_bt_far=1, dcn_bt_sample=0), "BT_LCAP_BF16", 1),
    "fused": (dict(dcn_bt_fly=0, dcn_bt_fuse_wgrad=1, dcn_bt_fuse_min_chunks=1), dict(dcn_bt_fused=1, dcn_bt_fly=0, dcn_bt_tile=1, dcn_bt_far=1, dcn_bt_sample=0), "BT_LCAP_BF16", 1),
    "unfused": (dict(dcn_bt_fuse_wgrad=0), dict(dcn_bt_fused=0, dcn_bt_fly=0, dcn_bt_tile=1, dcn_bt_far=1, dcn_bt_sample=1), "BT_LCAP_BF16", 0),
    "unfused_cs64": (dict(dcn_bt_fuse_wgrad=0, dcn_bt_cs=64), dict(dcn_bt_fused=0, dcn_bt_fly=0, dcn_bt_tile=1, dcn_bt_far=1, dcn_bt_sample=1), "BT_LCAP_BF16", 0),
    "unfused_cs128": (dict(dcn_bt_fuse_wgrad=0, dcn_bt_cs=128), dict(dcn_bt_fused=0, dcn_bt_fly=0, dcn_bt_tile=1, dcn_bt_far=1, dcn_bt_sample=1), "BT_LCAP_BF16", 0),
    "det": (dict(deterministic=1, dcn_bt_fuse_wgrad=0), dict(dcn_bt_fused=0, dcn_bt_fly=0, dcn_bt_tile=0, dcn_bt_far=0, dcn_bt_sample=1), None, 0),
}
_FLOOR = 0.02      # an output that came out exact (or within 1 % of a rounding unit: fp32 summation order on exact operands) has no spread to double
# k per (form family, type): max(_FLOOR, 2x the worst ratio observed on MI355X rounded up to one significant digit); profiles/dcn_bwd_edges.md
K = {
    ("fly1", "bf16"): dict(dx=2.0, d_raw=2.0, dw=0.2, db=_FLOOR),
    ("fly1", "fp16"): dict(dx=1.0, d_raw=1.0, dw=_FLOOR, db=_FLOOR),
    ("fly2", "bf16"): dict(dx=2.0, d_raw=2.0, dw=0.2, db=_FLOOR),
    ("fly2", "fp16"): dict(dx=1.0, d_raw=1.0, dw=_FLOOR, db=_FLOOR),
    ("fused", "bf16"): dict(dx=2.0, d_raw=2.0, dw=0.2, db=_FLOOR),
    ("fused", "fp16"): dict(dx=1.0, d_raw=1.0, dw=_FLOOR, db=_FLOOR),
    ("unfused", "bf16"): dict(dx=2.0, d_raw=0.6, dw=0.2, db=_FLOOR),
    ("unfused", "fp16"): dict(dx=1.0, d_raw=_FLOOR, dw=_FLOOR, db=_FLOOR),
    ("unfused", "fp32"): dict(dx=_FLOOR, d_raw=0.6, dw=_FLOOR, db=_FLOOR),
    ("det", "bf16"): dict(dx=2.0, d_raw=0.6, dw=_FLOOR, db=_FLOOR),
    ("det", "fp16"): dict(dx=1.0, d_raw=_FLOOR, dw=_FLOOR, db=_FLOOR),
    ("det", "fp32"): dict(dx=_FLOOR, d_raw=_FLOOR, dw=_FLOOR, db=_FLOOR),
}
_OBSERVED, _TEETH = {}, []


def _family(form):
    return "unfused" if form.startswith("unfused") else form


def _k(form, dtype, q):
    return K[(_family(form), dtype)][q]


@functools.lru_cache(maxsize=None)
def _ref(name):
    """Reference, magnitudes and census of a case: computed once, shared by every test that needs them, never modified."""
    k = CS.case(name)
    x, om, w, dy = CS.inputs(name)
    return R.backward(x, om, w, dy), R.census(om, k.H, k.W, CONSTS)


_WS = {}


def _workspace(nbytes):
    if "buf" not in _WS or _WS["buf"].numel() < nbytes:
        _WS["buf"] = None
        _WS["buf"] = torch.empty(nbytes, dtype=torch.uint8, device=DEV)
    return _WS["buf"]


def _call(name, form, dtype):
    """One launch of the backward under the form's options -> the four outputs on the CPU (raw tensors) and the counter deltas."""
    from monoflex_amd import lib as L
    lib_ = L.load()
    k = CS.case(name)
    dt, code = DT[dtype], {"bf16": L.MFX_BF16, "fp16": L.MFX_F16, "fp32": L.MFX_F32}[dtype]
    opts, _, _, raw16 = FORMS[form]
    raw16 = raw16 if dtype != "fp32" else 0
    x, om, w, dy = CS.inputs(name)
    xd, dyd = x.to(DEV).to(dt), dy.to(DEV).to(dt)
    assert torch.equal(xd.float().cpu(), x) and torch.equal(dyd.float().cpu(), dy)            # the operands are exact in the type
    assert torch.equal(w.to(dt).float(), w)
    omd, wd = om.to(DEV), w.to(DEV)
    nan = float("nan")
    dx = torch.full(x.shape, nan, dtype=dt, device=DEV)
    draw = torch.full(om.shape, nan, dtype=dt if raw16 else torch.float32, device=DEV)
    dw, db = torch.full(w.shape, nan, device=DEV), torch.full((k.Cout,), nan, device=DEV)
    nws = lib_.mfx_dcn_backward_v2_workspace_bytes(k.B, k.C, k.H, k.W, k.Cout, code)
    ws = _workspace(nws)
    ptr = lambda t: ctypes.c_void_p(t.data_ptr())                                              # noqa: E731
    try:
        for o, v in opts.items():
            L.check(lib_.mfx_set_option(o.encode(), v), "opt")
        before = {c: lib_.mfx_get_counter(c.encode()) for c in COUNTERS}
        L.check(lib_.mfx_dcn_backward_v2_rt(ptr(xd), ptr(omd), ptr(wd), ptr(dyd), ptr(dx), ptr(draw), raw16, ptr(dw), ptr(db), k.B, k.C, k.H, k.W, k.Cout,
                                            code, ptr(ws), nws, None), "mfx_dcn_backward_v2_rt")
        torch.cuda.synchronize()
        delta = {c: lib_.mfx_get_counter(c.encode()) - before[c] for c in COUNTERS}
    finally:
        for o, v in DEFAULTS.items():
            L.check(lib_.mfx_set_option(o.encode(), v), "opt")
    return dict(dx=dx.cpu(), d_raw=draw.cpu(), dw=dw.cpu(), db=db.cpu()), delta


_RUNS = {}


def _run(name, form, dtype):
    key = (name, form, dtype)
    if key not in _RUNS:
        _RUNS[key] = _call(name, form, dtype)
    return _RUNS[key]


def _denominators(name, form, dtype, ref=None, cen=None):
    """u_op M + u_out |ref| per output (+ the atomics term of grad_input): what k multiplies."""
    r0, c0 = _ref(name)
    ref, cen = ref or r0, cen or c0
    uop, uout = U[dtype]
    lcap_name, raw16 = FORMS[form][2], FORMS[form][3] and dtype != "fp32"
    den = {}
    for q in OUTPUTS:
        uo = uout if q == "dx" or (q == "d_raw" and raw16) else U["fp32"][1]
        den[q] = uop * ref["M"][q] + uo * ref[q].abs()
    if lcap_name is not None:
        lcap = CONSTS["LCAP_F32"] if dtype == "fp32" else CONSTS[lcap_name]
        den["dx"] = den["dx"] + (R.n_atomic(cen, lcap).to(D64) * uout).unsqueeze(-1) * ref["M"]["dx"]
    return den


def _ratio(got, ref, den):
    d = (got.to(D64) - ref).abs()
    return torch.where(d == 0, torch.zeros_like(d), d / den.clamp(min=1e-300))


def _check(name, form, dtype):
    got, delta = _run(name, form, dtype)
    ref, _ = _ref(name)
    raw16 = FORMS[form][3] and dtype != "fp32"
    assert got["dx"].dtype == DT[dtype] and got["d_raw"].dtype == (DT[dtype] if raw16 else torch.float32)
    assert got["dw"].dtype == torch.float32 and got["db"].dtype == torch.float32
    assert delta == FORMS[form][1], (form, delta)
    for q in OUTPUTS:
        assert got[q].shape == ref[q].shape and not bool(torch.isnan(got[q]).any()), "%s: NaN left in %s (an element was not written)" % (name, q)
        assert bool(torch.isfinite(got[q]).all()), q
    assert float(got["d_raw"][..., 27:].float().abs().max()) == 0
    den = _denominators(name, form, dtype)
    worst = {}
    for q in OUTPUTS:
        r = _ratio(got[q], ref[q], den[q])
        worst[q] = float(r.max())
        print("%-36s %-13s %-4s %-5s worst ratio %.4g (k = %g) at %s" % (name, form, dtype, q, worst[q], _k(form, dtype, q),
                                                                        tuple(int(v) for v in torch.nonzero(r == r.max())[0])))
        o = _OBSERVED.setdefault((_family(form), dtype), {}).setdefault(q, dict(max=0.0, case=None))
        if worst[q] >= o["max"]:
            o["max"], o["case"] = worst[q], "%s / %s" % (name, form)
    for q in OUTPUTS:
        assert worst[q] <= _k(form, dtype, q), (name, form, dtype, q, worst[q])
    return got


def _plan():
    p = []
    both16, all3 = ("bf16", "fp16"), ("bf16", "fp16", "fp32")
    for n in CS.names("translate_") + ["border_9x32"] + CS.names("focus16"):
        p += [(n, f, d) for f in ("fly1", "fly2", "fused") for d in both16]
        p += [(n, "unfused", d) for d in (both16 if n.startswith("focus16") else all3)]
    p += [(n, "unfused", "fp32") for n in CS.names("focus32")]
    p += [("border_9x17", "unfused", d) for d in all3]
    p += [(n, f, d) for n in CS.names("wide128") for f in ("unfused", "unfused_cs128") for d in all3]
    p += [(n, f, d) for n in CS.names("wide256") for f in ("unfused", "unfused_cs64", "unfused_cs128") for d in all3]
    return p


@pytest.fixture(scope="module", autouse=True)
def _report():
    yield
    os.makedirs(REPORT_DIR, exist_ok=True)
    rows = [dict(form=f, dtype=d, output=q, worst_ratio=v["max"], case=v["case"], k=K[(f, d)][q])
            for (f, d), qs in sorted(_OBSERVED.items()) for q, v in qs.items()]
    with open(os.path.join(REPORT_DIR, "dcn_bwd_edges.json"), "w") as f:
        json.dump(dict(constants=CONSTS, rows=rows, teeth=_TEETH), f, indent=1)


@pytest.mark.parametrize("name,form,dtype", _plan())
def test_dcn_backward_edges_vs_float64(name, form, dtype):
    _check(name, form, dtype)


@pytest.mark.parametrize("name,dtype", [("focus16_mid", "bf16"), ("focus16_corner", "fp16"), ("focus32_mid", "fp32"), ("focus32_corner", "fp32"),
                                        ("translate_cols_24", "bf16"), ("translate_cols_24", "fp16"), ("translate_cols_24", "fp32")])
def test_dcn_backward_deterministic_mode_vs_float64(name, dtype):
    """Option `deterministic`: grad_input through the 64-bit fixed-point map.  The bound holds WITHOUT the atomics term (`det` has no list
    capacity in FORMS, so _denominators adds none), and a second call gives the same bits in all four outputs."""
    first = _check(name, "det", dtype)
    second, _ = _call(name, "det", dtype)
    for q in OUTPUTS:
        assert torch.equal(first[q].view(torch.uint8), second[q].view(torch.uint8)), "%s differs between two deterministic calls" % q


def _tooth(tag, name, form, dtype, q, wrong, den):
    got, _ = _run(name, form, dtype)
    observed = float(_ratio(got[q], wrong, den).max())
    bound = _k(form, dtype, q)
    _TEETH.append(dict(tooth=tag, case=name, form=form, dtype=dtype, output=q, observed=observed, k=bound))
    print("tooth %s %s %s %s: observed %.4g, k %g" % (tag, name, form, dtype, observed, bound))
    assert observed >= 2 * bound, (tag, name, form, dtype, observed, bound)


@pytest.mark.parametrize("name,form,dtype", [("focus16_mid", "fly1", "bf16"), ("focus16_corner", "fused", "fp16"), ("focus16_mid", "unfused", "bf16"),
                                             ("focus32_corner", "unfused", "fp32")])
def test_tooth_a_pairs_beyond_the_list_capacity(name, form, dtype):
    ref, cen = _ref(name)
    lcap = CONSTS["LCAP_F32"] if dtype == "fp32" else CONSTS[FORMS[form][2]]
    dropped = R.beyond_capacity(cen, lcap)
    assert int(dropped.sum()) == int((cen["near_pp"] - lcap).clamp(min=0).sum()) > 0
    wrong = ref["dx"] - R.scatter_pairs(ref["geometry"], ref["gcol"], dropped)
    _tooth("(a) dx without the pairs beyond the list capacity", name, form, dtype, "dx", wrong, _denominators(name, form, dtype)["dx"])


@pytest.mark.parametrize("name,form,dtype", [("translate_cols_9", "fly1", "bf16"), ("translate_cols_m9", "fly2", "fp16"),
                                             ("translate_tall_rows_9", "unfused", "fp32"), ("translate_tall_rows_m9", "fused", "bf16")])
def test_tooth_b_seam_pairs_counted_by_both_routes(name, form, dtype):
    ref, cen = _ref(name)
    seam = cen["pairs"] & (cen["ring"] == CONSTS["BT_D_VAL"] + 1)
    assert int(seam.sum()) > 0
    wrong = ref["dx"] + R.scatter_pairs(ref["geometry"], ref["gcol"], seam)
    _tooth("(b) dx with the D + 1 pairs counted twice", name, form, dtype, "dx", wrong, _denominators(name, form, dtype)["dx"])


@pytest.mark.parametrize("name,form,dtype", [("border_9x32", "fly1", "bf16"), ("border_9x32", "fused", "fp16"), ("border_9x17", "unfused", "fp32")])
def test_tooth_c_non_strict_inside(name, form, dtype):
    x, om, w, dy = CS.inputs(name)
    wrong = R.backward(x, om, w, dy, strict_inside=False)
    _tooth("(c) d_raw with a non-strict inside", name, form, dtype, "d_raw", wrong["d_raw"], _denominators(name, form, dtype, ref=wrong)["d_raw"])


@pytest.mark.parametrize("dtype", ["bf16", "fp32"])
def test_tooth_d_own_corners_in_the_ragged_part_of_an_edge_tile(dtype):
    name, form = "border_9x17", "unfused"
    k = CS.case(name)
    ref, cen = _ref(name)
    sel = R.ragged_own(cen, k.H, k.W)
    assert int(sel.sum()) > 0
    wrong = ref["dx"] - R.scatter_pairs(ref["geometry"], ref["gcol"], sel)
    _tooth("(d) dx without the own corners of a ragged tile", name, form, dtype, "dx", wrong, _denominators(name, form, dtype)["dx"])


def test_k_is_within_its_conditions():
    """k <= 8 for the 16-bit types; for fp32 k <= 2 x the largest fan-in of the case: Cout for d(columns) plus the pairs per pixel -- taken from the
    case with the SMALLEST such fan-in that runs in fp32, so it holds for every one of them."""
    fan = []
    for name, form, dtype in _plan():
        if dtype == "fp32":
            _, cen = _ref(name)
            fan.append(CS.case(name).Cout + int((cen["near_pp"] + cen["far_pp"]).max()))
    for (form, dtype), ks in K.items():
        for q, v in ks.items():
            assert v > 0
            assert v <= (2 * min(fan) if dtype == "fp32" else 8), (form, dtype, q, v)
