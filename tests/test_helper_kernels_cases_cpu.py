"""The preconditions tests/test_gpu_helper_kernels.py leans on, proved on the references alone (no GPU, no kernel).

For every exact case of tests/helper_kernels_cases.py:
  * the inputs survive a round trip through bf16 and fp16 unchanged;
  * the float32 evaluation of the reference equals the float64 one bit for bit (so the kernel's fp32 arithmetic, in whatever order, has
    one possible result), and `.to(bf16 / fp16)` of both agree;
  * the term counts stay inside the bound that makes every partial sum an fp32 number.
For the max-pool inputs: more than half of the windows have a tied maximum, and torch's autograd follows the first-maximum rule that the
kernel documents.  For the upsample weight-gradient kernel: each named case reaches the branch it is named after (dw_plan restates the
kernel's arithmetic).  For the grid-stride case: it exceeds the cap that the source sets.
"""
import pytest
import torch

import helper_kernels_cases as K


def _round_trips(t):
    t32 = t.float()
    assert torch.equal(t32.double(), t.double())
    for td in (torch.bfloat16, torch.float16):
        assert torch.equal(t32.to(td).float(), t32), td


def _same_in_fp32(ref64, ref32):
    assert ref32.dtype == torch.float32 and ref64.dtype == torch.float64
    assert torch.equal(ref32.double(), ref64)
    for td in (torch.bfloat16, torch.float16):
        assert torch.equal(ref64.to(td), ref32.to(td)), td


def test_canary_and_tables():
    for td in K.TORCH_DTYPE.values():
        assert float(torch.tensor(K.CANARY, dtype=td)) == K.CANARY
    for dt in K.DTYPES:                                   # every value of every axis of the upsample forward table appears in each dtype
        cases = [(B, f, K.chunk_of(C, dt), H, W, s) for (B, f, C, H, W, s) in K.UPSAMPLE_FWD_CASES]
        assert {c[1] for c in cases} == {2, 4, 8}
        assert {c[2] for c in cases} == {K.CHUNK[dt], 64, 128, 256}
        assert {(c[3], c[4]) for c in cases} == {(1, 1), (1, 5), (5, 1), (3, 7), (6, 10)}
        assert {c[5] for c in cases} == {True, False}
        for f in (2, 4, 8):
            assert {c[5] for c in cases if c[1] == f} == {True, False}


def test_grid_stride_case_exceeds_the_cap():
    from monoflex_amd.packing import STEM_PAD_H, STEM_PAD_WL, STEM_PAD_WR
    caps = K.grid_caps()
    assert caps["MFX_GRID"] == caps["TR_GRID"]
    cap, threads = caps["MFX_GRID"]
    B, H, W = K.PACK_GRID_STRIDE_CASE
    total = B * (H + 2 * STEM_PAD_H) * (W + STEM_PAD_WL + STEM_PAD_WR)
    assert cap * threads < total < cap * threads * 1.02, (cap, threads, total)      # just over: 36944 threads take a second pixel
    for (b, h, w) in K.PACK_CASES:
        assert b * (h + 2 * STEM_PAD_H) * (w + STEM_PAD_WL + STEM_PAD_WR) < cap * threads


@pytest.mark.parametrize("case", K.LAYOUT_CASES)
def test_layout_inputs(case):
    B, C, H, W, ld = case
    assert ld >= C
    _round_trips(K.dyadic((B, C, H, W), 11))


def test_specials_are_what_they_claim():
    s = K.specials_nchw()
    h, b = s.to(torch.float16).flatten(), s.to(torch.bfloat16).flatten()
    v = K.SPECIALS
    assert float(h[v.index(65519.0)]) == 65504.0 and float(h[v.index(65520.0)]) == float("inf") and float(h[v.index(-65520.0)]) == float("-inf")
    assert 0 < float(h[v.index(1e-6)]) < 2.0 ** -14 and float(h[v.index(6e-8)]) == 2.0 ** -24
    assert float(b[v.index(1 + 2.0 ** -8)]) == 1.0 and float(b[v.index(1 + 3 * 2.0 ** -8)]) == 1 + 2.0 ** -6       # ties to even: down, up
    assert float(h[v.index(1 + 2.0 ** -11)]) == 1.0 and float(h[v.index(1 + 3 * 2.0 ** -11)]) == 1 + 2.0 ** -9
    assert torch.isnan(h).sum() == 1 and torch.isnan(b).sum() == 1
    assert torch.signbit(s.flatten()[1]) and float(s.flatten()[1]) == 0.0


@pytest.mark.parametrize("case", K.PACK_CASES + [K.PACK_GRID_STRIDE_CASE])
def test_pack_inputs(case):
    B, H, W = case
    img = K.dyadic((B, 3, H, W), 21)
    _round_trips(img)
    for dt in K.DTYPES:
        y = K.pack_ref(img, dt)
        assert y.shape == (B, H + 6, W + 8, 4) and float(y[..., 3].abs().max()) == 0
        assert float(y[:, :3].abs().max()) == 0 and float(y[:, -3:].abs().max()) == 0 and float(y[:, :, :3].abs().max()) == 0 and float(y[:, :, -5:].abs().max()) == 0
        if dt != "fp32" and case == K.PACK_GRID_STRIDE_CASE:
            break


@pytest.mark.parametrize("dt", K.DTYPES)
def test_pool_inputs_tie_and_first_max_rule(dt):
    """Measured share of windows with a tied maximum in the generated inputs: between 0.75 (the 2x2 maps: 4 to 12 windows per channel) and 0.92
    over the shapes of the table, in every dtype; required above one half."""
    for i, (B, C, H, W) in enumerate(K.pool_cases(dt)):
        x = K.pool_input(B, C, H, W, 31 + i)
        dy = K.dyadic((B, C, H // 2, W // 2), 131 + i, nonzero=True)
        finite = x[torch.isfinite(x)]
        assert torch.equal(finite * 2, (finite * 2).round()) and float(finite.abs().max()) <= 2
        assert torch.isinf(x).any()
        share = K.tie_share(x)
        assert share > 0.5, (B, C, H, W, share)
        _round_trips(dy)
        y64, dx64 = K.pool_ref(x, dy)
        y32, dx32 = K.pool_ref(x.float(), dy.float())
        assert torch.equal(y32.double(), y64) and torch.equal(dx32.double(), dx64)
        # the rule: the first maximum in row-major order takes the whole gradient, the other three positions get exact zeros
        assert torch.equal(dx64, K.pool_first_max_grad(x, dy))
        assert torch.equal((dx64 != 0).sum(), torch.tensor(dy.numel()))


@pytest.mark.parametrize("dt", K.DTYPES)
def test_upsample_forward_references(dt):
    for i, (B, f, C, H, W, with_skip) in enumerate(K.UPSAMPLE_FWD_CASES):
        C = K.chunk_of(C, dt)
        x, w = K.dyadic((B, C, H, W), 41 + i), K.tap_weights(C, f, 141 + i)
        skip = K.dyadic((B, C, H * f, W * f), 241 + i) if with_skip else None
        _round_trips(x)
        _round_trips(w)
        assert float(w.min()) >= 0 and float(w.max()) <= 1 and torch.equal(w * 16, (w * 16).round())
        assert K.exact_terms_bound(5, 4.0, 1.0 / 128)
        _same_in_fp32(K.upsample_ref(x, w, skip, f), K.upsample_ref(x.float(), w.float(), None if skip is None else skip.float(), f))


@pytest.mark.parametrize("name", sorted(K.UPSAMPLE_BWD_CASES))
def test_upsample_backward_references(name):
    B, C, f, H, W = K.UPSAMPLE_BWD_CASES[name]
    x, w, skip, dy = K.upsample_bwd_inputs("fp32", B, C, f, H, W, 51)
    for t in (x, w, skip, dy):
        _round_trips(t)
    assert K.exact_terms_bound(4 * f * f, 4.0, 1.0 / 128)          # dx: (2f)^2 products dy * w
    assert K.exact_terms_bound(B * H * W, 16.0, 1.0 / 64)          # dw: one product x * dy per input pixel
    r64 = K.upsample_ref(x, w, skip, f, dy)
    r32 = K.upsample_ref(x.float(), w.float(), skip.float(), f, dy.float())
    for a, b in zip(r64, r32):
        _same_in_fp32(a, b)
    assert not (r64[1] == K.CANARY).any() and not (r64[2] == K.CANARY).any()


def test_upsample_backward_cases_reach_their_branches():
    P = lambda dt, name, ws=True: K.dw_plan(dt, *K.UPSAMPLE_BWD_CASES[name], workspace=ws)        # noqa: E731
    for dt in K.DTYPES:
        for name in K.UPSAMPLE_BWD_CASES:
            assert P(dt, name)["pow2"], (dt, name)
    p = P("fp32", "unrolled_w19")
    assert (p["items"], p["S"]) == (256, 4) and p["unrolled"] > 0 and p["tail"] > 0
    for dt in ("bf16", "fp16"):
        p = P(dt, "unrolled_w35")
        assert (p["items"], p["S"]) == (128, 8) and p["unrolled"] > 0 and p["tail"] > 0
        assert P(dt, "unrolled_w19")["unrolled"] == 0                                               # 3 S = 24 > 18: that is why the 16-bit types need W = 35
    for dt in K.DTYPES:
        p = P(dt, "tail_only")
        assert p["S"] > 3 and p["unrolled"] == 0 and p["tail"] > 0 and p["idle"] > 0                # W = 3 < S: some column groups own nothing
    p = P("fp32", "items_1024")
    assert (p["items"], p["S"], p["passes"]) == (1024, 1, 1)
    assert (P("fp32", "multi_pass")["items"], P("fp32", "multi_pass")["passes"]) == (4096, 4)
    assert (P("bf16", "multi_pass")["items"], P("bf16", "multi_pass")["passes"]) == (2048, 2)
    assert [P("fp32", n)["S"] for n in ("c128", "c256")] == [2, 1] and [P("bf16", n)["S"] for n in ("c128", "c256")] == [4, 2]
    for dt in K.DTYPES:
        p = P(dt, "ragged_rows")
        assert (p["rows_per_block"], p["blocks"], p["last_block_rows"]) == (2, 151, 1)
        assert P(dt, "ragged_rows", ws=False)["rows_per_block"] == 1                                # the atomic form: one row per workgroup below 1024 rows
    dt, B, C, f, H, W = K.UPSAMPLE_BWD_BAD_ITEMS
    assert not K.dw_plan(dt, B, C, f, H, W, True)["pow2"] and C % K.CHUNK[dt] == 0


@pytest.mark.parametrize("dt", K.DTYPES)
def test_zero_insert_cases(dt):
    for i, (B, Ho, Wo, C, H, W) in enumerate(K.ZERO_INSERT_CASES):
        C = K.chunk_of(C, dt)
        assert Ho == (H + 1) // 2 and Wo == (W + 1) // 2
        dy = K.dyadic((B, Ho, Wo, C), 61 + i, nonzero=True)
        _round_trips(dy)
        up = K.zero_insert_ref(dy, H, W)
        assert torch.equal(up[:, ::2, ::2], dy) and float(up[:, 1::2].abs().max()) == 0 and float(up[:, :, 1::2].abs().max()) == 0


@pytest.mark.parametrize("case", K.COLSUM_CHUNK_CASES + K.COLSUM_GENERIC_CASES)
def test_colsum_references(case):
    M, C0, ld0, dts = case
    route = "chunk" if case in K.COLSUM_CHUNK_CASES else "generic"
    for dt in dts:
        C, ld = K.chunk_of(C0, dt), K.chunk_of(ld0, dt)
        assert K.colsum_route(dt, C, ld) == route, (case, dt)
        assert M <= (1 << 18) + 5 and K.exact_terms_bound(M + 1, 4.0, 0.125)        # (+ the nonzero `out` of colsum_add, |v| <= 4)
        x = K.colsum_input(M, C, ld, 71)
        _round_trips(x)
        assert float(x[:, :C].abs().max()) <= 2
        s64 = x[:, :C].sum(0)
        s32 = x[:, :C].float().sum(0)
        assert torch.equal(s32.double(), s64)
        # any order: a different association gives the same fp32 number
        assert torch.equal(x[:, :C].float().flip(0).cumsum(0)[-1].double(), s64)
        assert not (s64 == K.CANARY).any()
    for c in K.COLSUM_DETERMINISTIC_CASES:
        assert c in K.COLSUM_CHUNK_CASES + K.COLSUM_GENERIC_CASES


def test_edge_inputs():
    e = K.EDGE
    out, v, xy, n = K.edge_inputs(81)
    _round_trips(out)
    _round_trips(v)
    cx, cy = e["canary_pixel"]
    assert n.tolist() == e["edge_len"] and xy.dtype == torch.int32
    assert int(xy[..., 0].min()) >= 0 and int(xy[..., 0].max()) < e["W"] and int(xy[..., 1].min()) >= 0 and int(xy[..., 1].max()) < e["H"]
    for b in range(e["B"]):
        pre = [tuple(p) for p in xy[b, :int(n[b])].tolist()]
        assert len(set(pre)) == len(pre) and (cx, cy) not in pre
        assert all(tuple(p) == (cx, cy) for p in xy[b, int(n[b]):].tolist())
    for ch_off, C, planar in K.EDGE_CASES:
        pl = K.dyadic((e["B"], C, e["H"] * e["W"]), 82).float() if planar else None
        r32 = K.edge_scatter_ref(out, ch_off, C, v, xy, n, pl)
        r64 = K.edge_scatter_ref(out.double(), ch_off, C, v.double(), xy, n, None if pl is None else pl.double())
        assert torch.equal(r32[0].double(), r64[0]) and (pl is None or torch.equal(r32[1].double(), r64[1]))
        assert int((r32[0] != out).sum()) == C * sum(e["edge_len"])                  # v is nonzero: every listed element changes, nothing else
        assert torch.equal(r32[0][:, cy, cx], out[:, cy, cx])
