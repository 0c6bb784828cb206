"""Every weight-gradient route and the convolution data gradient against float64 references, exactly.

Kernels: conv_wgrad_patch_kernel, conv_wgrad_tr_kernel (csrc/wgrad_tr.hip), conv_wgrad_mfma_kernel with 64- and 128-wide tiles, conv_wgrad_kernel,
wgrad_reduce_kernel (csrc/train_kernels.hip) through the C entries mfx_conv_wgrad_oihw / mfx_conv_wgrad_nhwc / mfx_conv_wgrad_nhwc_dil;
stem_wgrad_kernel through autograd.StemConvFn; the data gradient (mode-1 weight pack, mfx_zero_insert2_nhwc, the forward conv kernels with the
residual in their epilogue) through autograd._conv_backward.

Every comparison is torch.equal with the float64 CPU reference of tests/wgrad_cases.py: the operands are +-{1/4, 1/2, 3/4, 1}, never zero, and
every case accumulates so few terms that each partial sum, in any order, is an fp32 number (tests/test_wgrad_cases_cpu.py proves that on the
references), so slab count, summation order, atomics and the reduce pass cannot change the result, while one dropped, doubled or misplaced
(pixel, tap) pair changes a whole (Cout, Ck) slice.  Nothing here is measured or timed.

Per weight-gradient row:
  * dW is prefilled with a canary and followed by a guard of canaries: every element must be written (the workspace forms rely on
    wgrad_reduce_kernel for that, without a zero fill) and nothing behind the end touched;
  * the workspace belongs to the test and is prefilled with the canary: a stale partial tile that reaches the sum shows up as a wrong dW,
    and nothing behind the slabs the route may use is written;
  * the dispatch counters wgrad_patch / wgrad_tr / wgrad_mfma / wgrad_valu / stem_wgrad are read around the call: the row's route, and only
    that one, moved by exactly one, and wgrad_reduce moved exactly when a workspace form ran;
  * options are set inside try and restored with mfx_reset_options in finally.
The route conditions and the ragged ends each row exists for are tabulated next to the case tables in wgrad_cases.py.
"""
import ctypes

import pytest
import torch

import wgrad_cases as K

pytestmark = pytest.mark.gpu
DEV = "cuda"


def _mods():
    from monoflex_amd import autograd as AG, lib as L
    return L.load(), L, AG


def _code(L, dt):
    return {"fp32": L.MFX_F32, "bf16": L.MFX_BF16, "fp16": L.MFX_F16}[dt]


def _stream():
    return ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)


def _p(t):
    """(of a NAMED tensor: a temporary's memory goes back to the caching allocator before the kernel reads it)"""
    return ctypes.c_void_p(t.data_ptr())


def _counters(lib):
    return {n: int(lib.mfx_get_counter(n.encode())) for n in K.COUNTERS}


def _moved(before, after):
    return {n: after[n] - before[n] for n in K.COUNTERS if after[n] != before[n]}


def _expected_moves(route, reduce):
    want = {K.ROUTE_COUNTER[route]: 1}
    if reduce:
        want["wgrad_reduce"] = 1
    return want


def _dev(t, dt):
    """float64 CPU tensor -> contiguous device tensor of the dtype (the values are numbers of that dtype: exact)."""
    return t.to(K.TORCH_DTYPE[dt]).contiguous().to(DEV)


def _all_canary(t):
    return bool((t == K.CANARY).all().item())


def _run_wgrad_row(c, dt):
    lib, L, _ = _mods()
    x, dy, ref = K.case_data(c)
    p = K.plan(c, dt)
    assert p["route"] == K.row_route(c, dt)
    xd = _dev(x, dt)
    dyd = xd if c.same else _dev(dy, dt)
    n = c.dw_numel()
    dw = torch.full((n + K.GUARD,), K.CANARY, dtype=torch.float32, device=DEV)
    ws = torch.full((c.ws + K.GUARD,), K.CANARY, dtype=torch.float32, device=DEV)
    geom = (c.B, c.H, c.W, c.xps, c.Ck, c.kh, c.kw, c.stride, c.pad_h, c.pad_w)
    torch.cuda.synchronize()
    before = _counters(lib)
    try:
        L.set_options(c.opts)
        if c.entry == "oihw":
            rc = lib.mfx_conv_wgrad_oihw(_p(xd), _p(dyd), _p(dw), *geom, c.Ho, c.Wo, c.Cout, c.ldy, c.Cout_real, c.Cin_real, _code(L, dt),
                                         _p(ws), c.ws * 4, _stream())
        elif c.entry == "nhwc":
            rc = lib.mfx_conv_wgrad_nhwc(_p(xd), _p(dyd), _p(dw), *geom, c.Ho, c.Wo, c.Cout, c.ldy, _code(L, dt), _stream())
        else:
            rc = lib.mfx_conv_wgrad_nhwc_dil(_p(xd), _p(dyd), _p(dw), *geom, c.dil_w, c.Ho, c.Wo, c.Cout, c.ldy, _code(L, dt), _stream())
        L.check(rc, "mfx_conv_wgrad_%s" % c.entry)
        torch.cuda.synchronize()
    finally:
        L.check(lib.mfx_reset_options(), "mfx_reset_options")
    moved = _moved(before, _counters(lib))
    assert moved == _expected_moves(p["route"], p["reduce"]), (moved, p)
    got = dw.cpu()
    assert int((got[:n] == K.CANARY).sum()) == 0                # every element written
    assert _all_canary(dw[n:])                                  # nothing behind the end
    assert _all_canary(ws[p["ws_used"]:])                       # nothing behind the slabs of the route (the whole workspace on an atomic form)
    want = ref.float().reshape(-1)
    if not torch.equal(got[:n], want):
        bad = (got[:n] != want).nonzero().flatten()
        shape = tuple(ref.shape)
        first = [tuple(int(v) for v in torch.unravel_index(i, shape)) for i in bad[:4]]
        raise AssertionError("%s %s (%s): %d of %d entries differ; first %s got %s want %s" % (
            c.name, dt, p, bad.numel(), n, first, got[bad[:4]].tolist(), want[bad[:4]].tolist()))


@pytest.mark.parametrize("c,dt", K.rows(K.PATCH_CASES), ids=K.row_id)
def test_wgrad_patch_route(c, dt):
    """LDS-patch kernel: 4 x 32 tiles over the right / bottom border, the zero halo, padded output channels, the 16- and 32-channel forms,
    6 and 12 waves, one / ragged / four-tile slabs."""
    _run_wgrad_row(c, dt)


@pytest.mark.parametrize("c,dt", K.rows(K.TR_CASES), ids=K.row_id)
def test_wgrad_tr_route(c, dt):
    """Transposed-read kernel: ragged last 32-pixel step, slabs at the 512 floor / two slabs / one slab, stride 2, 1x1, Cout = 64 under wgrad_tr = 2,
    ldy > Cout and x_pixstride > Ck."""
    _run_wgrad_row(c, dt)


@pytest.mark.parametrize("c,dt", K.rows(K.MFMA_CASES), ids=K.row_id)
def test_wgrad_mfma_route(c, dt):
    """First-generation slab kernel, 64- and 128-wide tiles: workspace + reduce, atomics, a single deterministic slab, 32-pixel slabs cut mid-row and
    across the batch boundary, a workspace too small for one slab, the [Cout][tap][Ck] entry without a workspace."""
    _run_wgrad_row(c, dt)


@pytest.mark.parametrize("c,dt", K.rows(K.VALU_CASES), ids=K.row_id)
def test_wgrad_valu_route(c, dt):
    _run_wgrad_row(c, dt)


@pytest.mark.parametrize("c,dt", K.rows(K.CALLER_CASES), ids=K.row_id)
def test_wgrad_caller_geometries(c, dt):
    """The geometries gram_heads.py and StemConvFn pass, at the C boundary with default options: 5x5 / 3x5 with x as both operands, the matrix form,
    the stem's dilated super-taps, dy inside a wider map, x inside a wider map."""
    _run_wgrad_row(c, dt)


# ---- the stem through StemConvFn ------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("case", K.STEM_CASES, ids=str)
@pytest.mark.parametrize("dt,generic", [("bf16", False), ("bf16", True), ("fp16", False), ("fp16", True), ("fp32", False)])
def test_stem_wgrad(dt, generic, case):
    """StemConvFn's weight gradient: the Toeplitz-row kernel (stem_wgrad), the generic dilated-tap form (_STEM_WGRAD_GENERIC: the MFMA slab kernel
    with atomics) and the fp32 path (VALU kernel over the packed image; the switch does not reach it)."""
    lib, L, AG = _mods()
    B, H, W = case
    img, w, dy = K.stem_inputs(B, H, W)
    ref = K.stem_wgrad_ref(img, dy)
    imgd, dyd = _dev(img, "fp32"), _dev(dy, dt)
    wd = _dev(w, "fp32").requires_grad_()
    keep = AG._STEM_WGRAD_GENERIC[0]
    try:
        AG._STEM_WGRAD_GENERIC[0] = generic
        y = AG.StemConvFn.apply(imgd, wd, K.TORCH_DTYPE[dt])
        assert y.shape == dyd.shape and y.dtype == dyd.dtype
        torch.cuda.synchronize()
        before = _counters(lib)
        y.backward(dyd)
        torch.cuda.synchronize()
    finally:
        AG._STEM_WGRAD_GENERIC[0] = keep
    route = "valu" if dt == "fp32" else ("mfma" if generic else "stem")
    assert _moved(before, _counters(lib)) == _expected_moves(route, False)
    assert wd.grad.dtype == torch.float32 and torch.equal(wd.grad.cpu(), ref.float())


# ---- the data gradient through _conv_backward ---------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("dt", K.DTYPES)
@pytest.mark.parametrize("case", K.dgrad_cases(), ids=str)
def test_conv_dgrad(case, dt):
    """dx of 3x3 s2 over even and odd maps (zero insertion: the last inserted row / column is the last one of an odd map), 3x3 s1 and 1x1, with and
    without the residual (added in the epilogue, zero-padded alike where Cin = 20 is padded to 32 operand rows and dx is sliced); the padded channels of dy hold non-zero values.  A 16-bit dx is
    the float64 result rounded once to nearest even, on both sides."""
    lib, L, AG = _mods()
    k, s, H, W, cin, cout = case
    td = K.TORCH_DTYPE[dt]
    w, dy, res = K.dgrad_inputs(*case, dt)
    xd = torch.full((K.DGRAD_B, H, W, cin), K.CANARY, dtype=td, device=DEV)      # only its shape and dtype enter dx
    wd, dyd, resd = _dev(w, "fp32"), _dev(dy, dt), _dev(res, dt)
    before = _counters(lib)
    for r, rd in ((None, None), (res, resd)):
        ref = K.dgrad_ref(w, dy, r, k, s, H, W)
        dx, dw, db = AG._conv_backward(xd, wd, dyd, s, k // 2, False, cout, (True, False, False), res=rd)
        torch.cuda.synchronize()
        assert dw is None and db is None
        assert dx.dtype == td and tuple(dx.shape) == (K.DGRAD_B, H, W, cin)
        got, want = dx.cpu(), ref.to(td)
        if not torch.equal(got, want):
            bad = (got != want).nonzero()
            raise AssertionError("%s %s res=%s: %d entries differ, first (b, h, w, c) %s" % (case, dt, r is not None, bad.shape[0], bad[:4].tolist()))
    assert torch.equal(resd.cpu(), res.to(td))                   # the residual is read, not accumulated into
    assert _moved(before, _counters(lib)) == {}
