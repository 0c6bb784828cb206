"""CPU tests of the float64 restatement of the DCN backward (tests/dcn_bwd_ref.py) and of the engineered offset fields (tests/dcn_bwd_cases.py)
that tests/test_gpu_dcn_bwd_edges.py runs the HIP kernels on.

1. The reference equals the project's C oracle (oracle/dcn_v2_ref.c, the restatement of the reference's col2im / col2im_coord) on EVERY engineered
   case, to the oracle's fp32 rounding: 5e-5 of the tensor's scale, the bar of tests/test_oracle_dcn.py.  The oracle carries the reference's own
   treatment of the coordinates -1, H and the integral ones, so this is where the strict `inside` rule is pinned: the non-strict variant (the tooth
   of the device test) misses the same bar on the border case.
2. On generic offsets (no multiple of 1/4, none integral) the reference equals the float64 autograd of the grid_sample formulation
   (oracle.dcn_ref.dcn_v2_grid_sample: the arithmetic of tests/test_gpu_layer_oracle._dcn64) to 1e-12 of the tensor's scale.
3. Every census condition the cases are built for holds.  If one fails, the CASE is wrong, not the kernel.
4. The five limits parse from the kernel's source."""
import pytest
import torch

import dcn_bwd_cases as CS
import dcn_bwd_ref as R

D64 = torch.float64
CONSTS = R.kernel_constants()
LCAP16 = CONSTS["BT_LCAP_BF16"]


def _oracle(x, om, w, dy):
    """The C oracle on the kernel's layout -> (dx NHWC, d_raw (B,H,W,32) with the mask-logit factor applied in float64, dw, db)."""
    from oracle import dcn_ref
    nchw = lambda t: t.permute(0, 3, 1, 2).contiguous()                       # noqa: E731
    off, msk = nchw(om[..., :18]), nchw(om[..., 18:27])
    gi, goff, gm, gw, gb = dcn_ref.dcn_v2_backward(nchw(x), w, torch.zeros(w.shape[0]), off, msk, nchw(dy), 3, 3, 1, 1, 1, 1, 1, 1, 1)
    raw = torch.zeros(om.shape, dtype=D64)
    raw[..., :18] = goff.permute(0, 2, 3, 1).to(D64)
    m = om[..., 18:27].to(D64)
    raw[..., 18:27] = gm.permute(0, 2, 3, 1).to(D64) * m * (1 - m)
    return dict(dx=gi.permute(0, 2, 3, 1).to(D64), d_raw=raw, dw=gw.to(D64), db=gb.to(D64))


def _miss(a, b):
    return float((a - b).abs().max() / b.abs().max().clamp(min=1.0))


def test_the_five_limits_parse_from_the_source():
    assert set(CONSTS) == {"BT_D_VAL", "BT_FCAP", "BT_LCAP_BF16", "FZ_LCAP", "LCAP_F32"}
    assert all(isinstance(v, int) and v > 0 for v in CONSTS.values())
    # what the cases below were laid out for; a retuned kernel must revisit them (the census conditions say which)
    assert CONSTS["BT_D_VAL"] == 8 and CONSTS["BT_FCAP"] == 512
    assert CONSTS["LCAP_F32"] < CONSTS["BT_LCAP_BF16"] and CONSTS["FZ_LCAP"] == CONSTS["BT_LCAP_BF16"]


@pytest.mark.parametrize("name", list(CS.all_cases()))
def test_reference_equals_c_oracle(name):
    x, om, w, dy = CS.inputs(name)
    ref, orc = R.backward(x, om, w, dy), _oracle(x, om, w, dy)
    for q in ("dx", "d_raw", "dw", "db"):
        assert _miss(ref[q], orc[q]) < 5e-5, (q, _miss(ref[q], orc[q]))
    assert float(ref["d_raw"][..., 27:].abs().max()) == 0
    for q in ("dx", "d_raw", "dw", "db"):                                       # M bounds |value|, element by element
        assert bool((ref["M"][q] >= ref[q].abs() * (1 - 1e-12)).all()), q


def test_c_oracle_pins_the_strict_inside_rule():
    """A sample at exactly -1 (or H) has no offset gradient in the reference; h >= -1 would give it one.  The wrong rule misses the oracle by far
    more than the bar on the border case, and only in the offset gradients."""
    x, om, w, dy = CS.inputs("border_9x17")
    orc = _oracle(x, om, w, dy)
    wrong = R.backward(x, om, w, dy, strict_inside=False)
    assert _miss(wrong["d_raw"], orc["d_raw"]) > 100 * 5e-5
    g = R.geometry(om, 9, 17)
    on_edge = ((g["h"] == -1) | (g["w"] == -1)) & (g["mask"] != 0)
    assert int(on_edge.sum()) > 50
    right = R.backward(x, om, w, dy)
    assert float(right["d_raw"][..., 0:18:2][on_edge].abs().max()) == 0 and float(right["d_raw"][..., 18:27][on_edge].abs().max()) == 0
    assert float(wrong["d_raw"][..., :18].abs().max()) > 0 and float((wrong["dx"] - right["dx"]).abs().max()) == 0


def test_reference_equals_float64_autograd_on_generic_offsets():
    from oracle import dcn_ref
    g = torch.Generator().manual_seed(31)
    B, C, Cout, H, W = 2, 6, 5, 9, 17
    x = torch.randn(B, H, W, C, generator=g, dtype=D64)
    dy = torch.randn(B, H, W, Cout, generator=g, dtype=D64)
    w = torch.randn(Cout, C, 3, 3, generator=g, dtype=D64)
    om = torch.zeros(B, H, W, 32, dtype=D64)
    # offsets on a 2^-16 grid (the fp32 coordinate is exact), std 3: samples cross the border band and leave the map; none on a multiple of 1/4
    off = torch.round(torch.randn(B, H, W, 18, generator=g, dtype=D64) * 3 * 65536) / 65536
    off = torch.where((off * 4) == torch.round(off * 4), off + 3.0 / 65536, off)
    om[..., :18] = off
    logit = torch.randn(B, H, W, 9, generator=g, dtype=D64)
    om[..., 18:27] = torch.sigmoid(logit)
    assert bool(((om[..., :18] * 4) != torch.round(om[..., :18] * 4)).all())
    nchw = lambda t: t.permute(0, 3, 1, 2)                                    # noqa: E731
    leaves = [t.clone().requires_grad_() for t in (x, om[..., :18].clone(), logit, w)]
    out = dcn_ref.dcn_v2_grid_sample(nchw(leaves[0]), nchw(leaves[1]), torch.sigmoid(nchw(leaves[2])), leaves[3], torch.zeros(Cout, dtype=D64))
    out.backward(nchw(dy))
    ref = R.backward(x, om, w, dy)
    inside = R.geometry(om, H, W)["inside"]
    assert 0.05 < float((~inside).double().mean()) < 0.6
    want_raw = torch.zeros_like(om)
    want_raw[..., :18], want_raw[..., 18:27] = leaves[1].grad, leaves[2].grad
    for q, a, b in (("dx", ref["dx"], leaves[0].grad), ("d_raw", ref["d_raw"], want_raw), ("dw", ref["dw"], leaves[3].grad),
                    ("db", ref["db"], dy.sum(dim=(0, 1, 2)))):
        assert _miss(a, b) < 1e-12, (q, _miss(a, b))


def _census(name):
    k = CS.case(name)
    return k, R.census(k.om, k.H, k.W, CONSTS)


@pytest.mark.parametrize("name", CS.names("translate_"))
def test_census_translate(name):
    """The shifts walk the near / far seam pixel by pixel: the census shows which side each case is on, and which cases overflow a far stage."""
    k, cen = _census(name)
    shift = float(k.om[0, 0, 0, 0] if "rows" in name else k.om[0, 0, 0, 1])
    assert int(cen["near_pp"].max()) <= CONSTS["LCAP_F32"], "translate cases leave every list below its capacity: only the far routes are in play"
    far = int(cen["far"].sum())
    rings = set(cen["ring"][cen["pairs"]].tolist())
    D = CONSTS["BT_D_VAL"]
    if name.startswith("translate_rows"):
        # 16 rows: both tile rows grown by D cover the whole map, no row shift can make a pair far (the tall cases are where rows do)
        assert far == 0 and max(rings) <= D
        assert int((cen["geometry"]["hc"] // R.TILE_H != torch.arange(k.H).view(1, k.H, 1, 1, 1) // R.TILE_H)[cen["pairs"]].sum()) > 0   # corners do cross the tile edge
        return
    # both sides of the seam are populated: pairs at exactly D pixels from the corner's tile (the last near ones) and at D + 1 (the first far ones)
    assert far > 0 and D + 1 in rings, (far, sorted(rings))
    if not name.endswith("tall_rows_17"):                         # (that one is all far: it is there for the stage, not for the seam)
        assert D in rings, sorted(rings)
    over = int(cen["far_pt"].max()) > CONSTS["BT_FCAP"]
    if (name.startswith("translate_cols") and abs(shift) >= 24) or (name.startswith("translate_tall_rows") and abs(shift) >= 17):
        assert over, "this shift was chosen to fill the far stage and force the per-corner path in the same workgroup"
    if abs(shift) <= 9:
        assert not over and int(cen["far_pt"].max()) > 0          # staged flush alone


@pytest.mark.parametrize("name", CS.names("focus16"))
def test_census_focus16(name):
    k, cen = _census(name)
    top = cen["near_pp"] > LCAP16
    assert int(top.sum()) == 4 * k.B
    v = cen["near_pp"][top]
    assert int(v.min()) >= LCAP16 + 8 and int(v.max()) <= LCAP16 + 32, v.tolist()
    assert int(cen["near_pp"][~top].max()) <= min(LCAP16, CONSTS["LCAP_F32"])
    assert int(cen["far"].sum()) == 0
    ys, xs = torch.nonzero(top[0], as_tuple=True)
    tiles = {(int(y) // R.TILE_H, int(x) // R.TILE_W) for y, x in zip(ys, xs)}
    assert len(tiles) == (4 if name.endswith("corner") else 1)


@pytest.mark.parametrize("name", CS.names("focus32"))
def test_census_focus32(name):
    k, cen = _census(name)
    cap = CONSTS["LCAP_F32"]
    assert int(cen["near_pp"].max()) > cap + CONSTS["BT_FCAP"], "one list fills, then the stage fills, and the rest go direct"
    assert int(R.stage_load(cen, cap).max()) > CONSTS["BT_FCAP"]
    assert int((cen["near_pp"] > cap).sum()) == 4 * k.B and int(cen["far"].sum()) == 0
    ys, xs = torch.nonzero(cen["near_pp"][0] > cap, as_tuple=True)
    assert len({(int(y) // R.TILE_H, int(x) // R.TILE_W) for y, x in zip(ys, xs)}) == (4 if name.endswith("corner") else 1)


@pytest.mark.parametrize("name", [n for n in CS.all_cases() if "border" in n])
def test_census_border(name):
    """Every border coordinate occurs on both axes with every mask value while the other axis is interior; the exact -1 / H samples are outside,
    the integral interior ones have exactly one or two live corners, and the ragged tiles receive pairs from their own samples."""
    k, cen = _census(name)
    g = cen["geometry"]
    for axis, other, n, m in (("h", "w", k.H, k.W), ("w", "h", k.W, k.H)):
        calm = (g[other] == 4.5)
        for t in CS.border_targets(n):
            for mv in CS.BORDER_MASKS:
                assert int(((g[axis] == t) & calm & (g["mask"] == mv)).sum()) > 0, (axis, t, mv)
        assert not bool(g["inside"][(g[axis] == -1) | (g[axis] == n)].any())
        assert bool(g["inside"][(g[axis] == -0.75) & calm].all()) and bool(g["inside"][(g[axis] == n - 0.25) & calm].all())
    both_integral = (g["h"] == 3) & (g["w"] == 3) & (g["mask"] != 0)
    assert int(both_integral.sum()) > 0 and bool((cen["pairs"][both_integral].sum(-1) == 1).all())
    if k.H % R.TILE_H or k.W % R.TILE_W:
        assert int(R.ragged_own(cen, k.H, k.W).sum()) > 50


@pytest.mark.parametrize("name", CS.names("wide"))
def test_census_wide(name):
    k, cen = _census(name)
    assert k.C >= 128 and int(cen["far"].sum()) > 0 and int(cen["near"].sum()) > 0
    if "16p25" in name:
        assert int(cen["far_pt"].max()) > CONSTS["BT_FCAP"]
