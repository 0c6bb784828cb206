"""The preconditions of tests/test_gpu_wgrad_exact.py, proved on the references alone (no GPU): for every row of every table of
tests/wgrad_cases.py the term bound holds, no operand is zero, every operand is a bf16 and an fp16 number, the fp32 evaluation of the general
reference in a shuffled order equals the float64 one, and the general reference equals float64 F.conv2d autograd where that can state the row.
The route every row names is the one the restated dispatch (wgrad_cases.plan) takes, with the slab arithmetic the row exists for."""
import pytest
import torch

import wgrad_cases as K

IDS = dict(ids=K.row_id)


def _is_16bit_number(t):
    return torch.equal(t.to(torch.bfloat16).double(), t) and torch.equal(t.to(torch.float16).double(), t)


def _operands_ok(*ts):
    for t in ts:
        assert t.dtype == torch.float64
        assert int((t == 0).sum()) == 0
        assert float(t.abs().max()) <= 1.0 and torch.equal(t * 4, (t * 4).round())
        assert _is_16bit_number(t)
        assert torch.equal(t.float().double(), t)


def test_option_defaults_match_the_header():
    assert K.option_defaults() == K.DEFAULTS


def test_pad_channels_matches_packing():
    from monoflex_amd.packing import _pad_channels
    for dt in K.DTYPES:
        for n in (3, 8, 16, 20, 27, 32, 64, 100, 128):
            assert K.pad_channels(n, dt) == _pad_channels(n, K.TORCH_DTYPE[dt]), (n, dt)


def test_names_are_unique_and_tables_cover_the_forms():
    names = [c.name for c in K.ALL_WCASES]
    assert len(names) == len(set(names))
    assert {c.opts.get("wgrad_patch_waves") for c in K.PATCH_CASES} >= {6, 12}
    assert any(c.entry == "nhwc" for c in K.MFMA_CASES) and any(c.entry == "dil" for c in K.CALLER_CASES)
    assert any(c.ldy > c.Cout for c in K.ALL_WCASES) and any(c.xps > c.Ck for c in K.ALL_WCASES) and any(c.Ck > c.xps for c in K.ALL_WCASES)
    assert max(c.M for c in K.ALL_WCASES) == 2 * 46 * 46      # the largest case: B = 2, 91 x 91 at stride 2, 64 -> 128


@pytest.mark.parametrize("c", K.ALL_WCASES, **IDS)
def test_wgrad_row_bound_and_route(c):
    assert K.exact_terms_bound(c.M) <= K.BOUND_CAP and c.M < 10 ** 4
    assert c.Ck % 4 == 0 and c.Cout % 4 == 0                  # the C entry's own argument rule
    for dt in c.dts:
        p = K.plan(c, dt)
        assert p["route"] == K.row_route(c, dt), (dt, p)
        if dt != "fp32" or c.route == "valu":
            for k, v in c.expect.items():
                assert p[k] == v, (dt, k, p)
        assert p["ws_used"] <= (c.ws if c.entry == "oihw" else 0)
        assert p["reduce"] == (p["route"] in ("patch", "tr") or bool(p.get("ws_ok")))
    if c.entry == "oihw":
        assert 1 <= c.Cout_real <= c.Cout and 1 <= c.Cin_real <= c.Ck


@pytest.mark.parametrize("c", K.ALL_WCASES, **IDS)
def test_wgrad_row_operands_and_reference(c):
    x, dy, ref = K.case_data(c)
    _operands_ok(x, dy)
    assert ref.numel() == c.dw_numel()
    assert float(ref.abs().max()) * 16 <= K.exact_terms_bound(c.M)
    # fp32, pixels in a shuffled order, 61 at a time into one running sum: the same numbers
    got32 = K.case_ref(c, x.float(), dy.float(), shuffle=5)
    assert got32.dtype == torch.float32 and torch.equal(got32.double(), ref)
    assert torch.equal(ref.float().double(), ref)
    if K.is_standard(c):
        want = K.conv2d_wgrad_ref(x, dy, c)[:c.Cout_real, :c.Cin_real]
        have = ref if c.entry == "oihw" else K.as_oihw(ref, c.kh, c.kw, c.Cout, c.Ck)
        assert torch.equal(have, want)


def test_general_reference_non_standard_forms_against_a_direct_sum():
    """The rows F.conv2d cannot state (dilated super-taps over x_pixstride < Ck, the 3x5 form with Ho = H): the general reference against the
    definition written as python loops over the taps, on a cut-down geometry."""
    for c in K.CALLER_CASES:
        if K.is_standard(c):
            continue
        x, dy, _ = K.case_data(c)
        x, dy = x[:1], dy[:1]
        ref = K.wgrad_ref(x, dy, c.Ck, c.kh, c.kw, c.stride, c.pad_h, c.pad_w, c.dil_w, c.Ho, c.Wo, c.Cout)
        flat = torch.cat([x.reshape(-1), torch.zeros(c.Ck, dtype=x.dtype)])
        want = torch.zeros_like(ref)
        for i in range(c.kh):
            for j in range(c.kw):
                for oh in range(c.Ho):
                    ih = oh * c.stride - c.pad_h + i
                    if not 0 <= ih < c.H:
                        continue
                    for ow in range(c.Wo):
                        iw = ow * c.stride - c.pad_w + j * c.dil_w
                        if 0 <= iw < c.W:
                            a = (ih * c.W + iw) * c.xps
                            want[:, i * c.kw + j] += dy[0, oh, ow, :c.Cout, None] * flat[a:a + c.Ck]
        assert torch.equal(ref, want), c.name


@pytest.mark.parametrize("name", ["patch_2x23x45_64_27of32_w12", "tr_2x41x51_64_128", "mfma_2x13x37_3x3s2_64_64_ws", "stemform_2x9x36"])
def test_a_dropped_pixel_fails_the_comparison(name):
    """The 'no zeros' premise at work: with ONE pixel's contribution missing -- the last pixel, the first one of the second image, one in the last
    column of a row -- the comparison of the GPU test (torch.equal in fp32) fails, and every (o, c) entry of every tap that pixel reaches is off."""
    c = next(r for r in K.ALL_WCASES if r.name == name)
    x, dy, ref = K.case_data(c)
    for m in (c.M - 1, c.Ho * c.Wo, c.Wo - 1):
        bad = K.case_ref(c, x, dy, drop=m)
        assert not torch.equal(bad.float(), ref.float())
        full = K.wgrad_ref(x, dy, c.Ck, c.kh, c.kw, c.stride, c.pad_h, c.pad_w, c.dil_w, c.Ho, c.Wo, c.Cout)
        miss = K.wgrad_ref(x, dy, c.Ck, c.kh, c.kw, c.stride, c.pad_h, c.pad_w, c.dil_w, c.Ho, c.Wo, c.Cout, drop=m)
        changed = (full != miss).flatten(0, 0)
        oh, ow = (m % (c.Ho * c.Wo)) // c.Wo, m % c.Wo
        for i in range(c.kh):
            for j in range(c.kw):
                ih, iw = oh * c.stride - c.pad_h + i, ow * c.stride - c.pad_w + j * c.dil_w
                inside = 0 <= ih < c.H and 0 <= iw < c.W
                assert bool(changed[:, i * c.kw + j].all()) == inside and (inside or not bool(changed[:, i * c.kw + j].any())), (m, i, j)


@pytest.mark.parametrize("case", K.STEM_CASES, ids=str)
def test_stem_rows(case):
    B, H, W = case
    img, w, dy = K.stem_inputs(B, H, W)
    _operands_ok(img, w, dy)
    assert K.exact_terms_bound(B * H * W) <= K.BOUND_CAP
    ref = K.stem_wgrad_ref(img, dy)
    assert torch.equal(K.stem_general_ref(img, dy), ref)
    assert torch.equal(K.stem_general_ref(img.float(), dy.float()).double(), ref)
    assert torch.equal(K.stem_wgrad_ref(img.float(), dy.float()).double(), ref)


@pytest.mark.parametrize("dt", K.DTYPES)
@pytest.mark.parametrize("case", K.dgrad_cases(), ids=str)
def test_dgrad_rows(case, dt):
    k, s, H, W, cin, cout = case
    w, dy, res = K.dgrad_inputs(*case, dt)
    _operands_ok(w, dy, res)
    assert K.exact_terms_bound(K.dgrad_terms(k, cout, dt)) <= K.BOUND_CAP
    assert dy.shape[-1] == K.pad_channels(cout, dt) >= cout
    if s == 2:
        assert H in (2 * dy.shape[1], 2 * dy.shape[1] - 1) and W in (2 * dy.shape[2], 2 * dy.shape[2] - 1)
    for r in (None, res):
        ref = K.dgrad_ref(w, dy, r, k, s, H, W)
        assert ref.shape == (K.DGRAD_B, H, W, cin)
        assert float(ref.abs().max()) * 16 <= K.exact_terms_bound(K.dgrad_terms(k, cout, dt))
        assert torch.equal(K.dgrad_general(w, dy, r, k, s, H, W), ref)
        got32 = K.dgrad_general(w.float(), dy.float(), None if r is None else r.float(), k, s, H, W, shuffle=9)
        assert got32.dtype == torch.float32 and torch.equal(got32.double(), ref)


def test_a_dropped_tap_fails_the_dgrad_comparison():
    """dx: with one tap's weights of one output channel missing, the 16-bit comparison fails as well (the sums stay far below the 8 significant bits
    of bf16 only by accident; the comparison is with the ROUNDED reference, so this shows the rounding does not hide a missing term)."""
    case = (3, 2, 21, 37, 32, 64)
    w, dy, res = K.dgrad_inputs(*case, "bf16")
    ref = K.dgrad_ref(w, dy, res, *case[:4])
    w2 = w.clone()
    w2[:, :, 2, 2] = 0
    bad = K.dgrad_ref(w2, dy, res, *case[:4])
    assert not torch.equal(bad.float(), ref.float())
    assert not torch.equal(bad.to(torch.bfloat16), ref.to(torch.bfloat16)) and not torch.equal(bad.to(torch.float16), ref.to(torch.float16))
