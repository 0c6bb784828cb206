"""The memory-bound helper kernels against float64 references, exactly.

Kernels: mfx_nchw_to_nhwc, mfx_nhwc_to_nchw, mfx_pack_image_nhwc4, mfx_maxpool2x2_nhwc, mfx_maxpool2x2_bwd_nhwc, mfx_upsample_add_nhwc,
mfx_upsample_bwd_nhwc, mfx_upsample_bwd_nhwc_oihw, mfx_zero_insert2_nhwc, mfx_colsum, mfx_colsum_add, mfx_edge_scatter_add -- through
ops / autograd where a wrapper exists (ops.nchw_to_nhwc, ops.nhwc_to_nchw, ops.pack_image, ops.maxpool2x2 + MaxPool2x2Fn, ops.upsample_add,
UpsampleAddFn, ops.edge_scatter_add) and through the C entry where the test has to own the output buffer.

Every comparison is torch.equal with the float64 CPU reference of tests/helper_kernels_cases.py converted with `.to(dtype)`: the operands sit on
dyadic grids on which every partial sum is an fp32 number, so the kernel's summation order, atomics, partial blocks and FMA contraction cannot
change the result (tests/test_helper_kernels_cases_cpu.py proves that on the references).  The exceptions are the four `randn` tests, which are
bounded per element: |got - ref| <= u |ref| + (n + 1) 2^-24 S + a (helper_kernels_cases.randn_bound).  Nothing here is measured or timed.

A buffer the test owns is longer than the kernel's output and prefilled with a finite canary: every element the kernel must write is compared with
a reference that never holds the canary, everything behind the end must still hold it.

Which case reaches which branch:
  layout      32x32 tiles over (pixel, channel), grid (ceil(HW / 32), ceil(ld / 32), B) forward and (.., ceil(C / 32), B) back.
              (2,3,5,7,4) 35 pixels = tiles of 32 + 3, C 3 < ld 4;  (1,27,9,13,32) 117 pixels, C 27 < ld 32 in one channel tile;
              (2,45,33,31,48) 1023 pixels (last tile lacks one), channel tiles 32 + 13 with padding 45..47;  (1,64,4,40,64) nothing ragged;
              (2,33,32,32,72) HW = 32 tiles exactly, channel tile 1 holds channel 32 + padding, channel tile 2 (64..71) padding only;  (1,1,1,1,8) one element.
  grid cap    MFX_GRID and TR_GRID cap a launch at 16384 workgroups of 256 threads = 4194304 items (read from the source by grid_caps()); the
              (1, 2050, 2050) image has 2056 * 2058 = 4231248 padded pixels, so 36944 threads take a second pixel in the grid-stride loop.
  upsample dw items = (2f)^2 * C / chunk, S = 1024 / items column groups, the 4x-unrolled loop needs iw_lo + grp + 3 S <= iw_hi (iw_hi <= W - 1),
              passes = items / 1024, rows_per_block = ceil(B H / 256) with the workspace and 1 (below 1024 rows) without:
              see the table above UPSAMPLE_BWD_CASES in helper_kernels_cases.py; dw_plan() restates the arithmetic and the CPU test asserts it per case.
  colsum      chunk route: C a power-of-two number of chunks, ld a multiple of the chunk ((333, 32, 64): ld != C).  Generic route: (500, 27) and (129, 3) odd C,
              129 rows = one 128-row workgroup + 1;  (777, 24) 6 chunks in fp32;  (300, 96) C > 64: two channel blocks of 64 lanes, the second one half empty;
              (2^18 + 5, 3 chunks) M >= 2^18: 1024 rows per workgroup, 257 workgroups, the last one holds 5 rows.
"""
import ctypes

import pytest
import torch

import helper_kernels_cases as K

pytestmark = pytest.mark.gpu
DEV = "cuda"
MFX_ERR_ARG = -1                                          # include/monoflex_hip.h


def _mods():
    from monoflex_amd import autograd as AG, lib as L, ops
    return L.load(), L, ops, AG


def _code(L, dt):
    return {"fp32": L.MFX_F32, "bf16": L.MFX_BF16, "fp16": L.MFX_F16}[dt]


def _stream():
    return ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)


def _p(t):
    """(of a NAMED tensor: a temporary's memory goes back to the caching allocator before the kernel reads it)"""
    return ctypes.c_void_p(t.data_ptr())


def _guarded(n, td, fill=None):
    """A flat device buffer of n + GUARD canaries; `fill` (n values) goes in front."""
    buf = torch.full((n + K.GUARD,), K.CANARY, dtype=td, device=DEV)
    if fill is not None:
        buf[:n] = fill.reshape(-1).to(device=DEV, dtype=td)
    return buf


def _guard_intact(buf, n):
    tail = buf[n:].cpu()
    return tail.numel() == K.GUARD and bool((tail.float() == K.CANARY).all())


def _untouched(buf):
    return bool((buf.cpu().float() == K.CANARY).all())


def _dev(t, dt):
    """float64 CPU tensor -> contiguous device tensor of the dtype (the values are numbers of that dtype: exact)."""
    return t.to(K.TORCH_DTYPE[dt]).contiguous().to(DEV)


# ---- 1. layout transforms ------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("case", K.LAYOUT_CASES, ids=str)
@pytest.mark.parametrize("dt", K.DTYPES)
def test_nchw_to_nhwc(dt, case):
    """mfx_nchw_to_nhwc: channels [0, C) = the cast input, [C, ld) exact zeros, nothing behind the map."""
    lib, L, _, _ = _mods()
    B, C, H, W, ld = case
    td = K.TORCH_DTYPE[dt]
    x = K.dyadic((B, C, H, W), 11)
    n = B * H * W * ld
    buf = _guarded(n, td)
    xd = _dev(x, "fp32")
    L.check(lib.mfx_nchw_to_nhwc(_p(xd), _p(buf), B, C, H, W, ld, _code(L, dt), _stream()), "mfx_nchw_to_nhwc")
    y = buf[:n].view(B, H, W, ld).cpu()
    assert torch.equal(y[..., :C], x.permute(0, 2, 3, 1).to(td))
    assert int((y[..., C:] != 0).sum()) == 0
    assert _guard_intact(buf, n)


@pytest.mark.parametrize("case", K.LAYOUT_CASES, ids=str)
@pytest.mark.parametrize("dt", K.DTYPES)
def test_nhwc_to_nchw(dt, case):
    """mfx_nhwc_to_nchw: the padding channels [C, ld) of the source hold NaN and must not reach the output."""
    lib, L, _, _ = _mods()
    B, C, H, W, ld = case
    td = K.TORCH_DTYPE[dt]
    x = K.dyadic((B, C, H, W), 12)
    src = torch.full((B, H, W, ld), float("nan"), dtype=td)
    src[..., :C] = x.permute(0, 2, 3, 1).to(td)
    n = B * C * H * W
    buf = _guarded(n, torch.float32)
    sd = src.to(DEV)
    L.check(lib.mfx_nhwc_to_nchw(_p(sd), _p(buf), B, C, H, W, ld, _code(L, dt), _stream()), "mfx_nhwc_to_nchw")
    y = buf[:n].view(B, C, H, W).cpu()
    assert not torch.isnan(y).any()
    assert torch.equal(y, x.float())
    assert _guard_intact(buf, n)


@pytest.mark.parametrize("dt", K.DTYPES)
def test_layout_wrappers_take_a_permuted_view(dt):
    """ops.nchw_to_nhwc on a non-contiguous NCHW input (a permuted NHWC tensor), channel axis padded, and ops.nhwc_to_nchw back."""
    _, _, ops, _ = _mods()
    B, C, H, W, ld = K.LAYOUT_CASES[2]
    td = K.TORCH_DTYPE[dt]
    x = K.dyadic((B, C, H, W), 13)
    view = x.float().permute(0, 2, 3, 1).contiguous().to(DEV).permute(0, 3, 1, 2)
    assert not view.is_contiguous()
    y = ops.nchw_to_nhwc(view, td, channels=ld)
    assert y.shape == (B, H, W, ld) and y.dtype == td
    assert torch.equal(y.cpu()[..., :C], x.permute(0, 2, 3, 1).to(td)) and int((y.cpu()[..., C:] != 0).sum()) == 0
    back = ops.nhwc_to_nchw(y, channels=C)
    assert back.shape == (B, C, H, W) and torch.equal(back.cpu(), x.float())


def _same_bits_or_both_nan(got, ref):
    bits = {2: torch.int16, 4: torch.int32}[ref.element_size()]
    nan = torch.isnan(ref)
    assert torch.equal(torch.isnan(got), nan)
    assert torch.equal(got.view(bits)[~nan], ref.view(bits)[~nan]), (got[~nan][got.view(bits)[~nan] != ref.view(bits)[~nan]], ref[~nan][got.view(bits)[~nan] != ref.view(bits)[~nan]])


@pytest.mark.parametrize("dt", ("bf16", "fp16"))
def test_layout_conversions_of_special_values(dt):
    """+-0, +-inf, NaN, the fp16 overflow boundary, fp16 subnormals and the round-to-even ties: the kernels' conversions against torch's own
    (NaN by position, everything else by bit pattern, the sign of zero included), both directions."""
    _, _, ops, _ = _mods()
    td = K.TORCH_DTYPE[dt]
    x = K.specials_nchw()
    ref = x.permute(0, 2, 3, 1).contiguous().to(td)
    _same_bits_or_both_nan(ops.nchw_to_nhwc(x.to(DEV), td).cpu(), ref)
    _same_bits_or_both_nan(ops.nhwc_to_nchw(ref.to(DEV)).cpu(), ref.float().permute(0, 3, 1, 2).contiguous())


# ---- 2. stem image packing ---------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("case", K.PACK_CASES, ids=str)
@pytest.mark.parametrize("dt", K.DTYPES)
def test_pack_image(dt, case):
    """mfx_pack_image_nhwc4 with the stem's pads: interior = the cast image, border and fourth channel exact zeros (pack_ref)."""
    from monoflex_amd.packing import STEM_PAD_H, STEM_PAD_WL, STEM_PAD_WR
    lib, L, _, _ = _mods()
    B, H, W = case
    img = K.dyadic((B, 3, H, W), 21)
    ref = K.pack_ref(img, dt)
    n = ref.numel()
    buf = _guarded(n, K.TORCH_DTYPE[dt])
    xd = _dev(img, "fp32")
    L.check(lib.mfx_pack_image_nhwc4(_p(xd), _p(buf), B, H, W, STEM_PAD_H, STEM_PAD_WL, STEM_PAD_WR, _code(L, dt), _stream()),
            "mfx_pack_image_nhwc4")
    assert torch.equal(buf[:n].view(ref.shape).cpu(), ref)
    assert _guard_intact(buf, n)


def test_pack_image_grid_stride():
    """fp32, (1, 2050, 2050): 4231248 padded pixels against 16384 * 256 = 4194304 threads -- the grid-stride branch (through ops.pack_image)."""
    _, _, ops, _ = _mods()
    B, H, W = K.PACK_GRID_STRIDE_CASE
    cap, threads = K.grid_caps()["MFX_GRID"]
    assert B * (H + 6) * (W + 8) > cap * threads
    img = K.dyadic((B, 3, H, W), 22).float()
    y = ops.pack_image(img.to(DEV), torch.float32)
    assert torch.equal(y.cpu(), K.pack_ref(img, "fp32"))


# ---- 3. max-pool ---------------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("C", K.POOL_C)
@pytest.mark.parametrize("dt", K.DTYPES)
def test_maxpool_forward_backward_with_ties(dt, C):
    """MaxPool2x2Fn on inputs where most windows have a tied maximum (and some +-inf): y = F.max_pool2d, dx = its float64 autograd = the whole
    gradient at the first maximum in row-major order, exact zeros at the other three positions."""
    _, _, _, AG = _mods()
    td = K.TORCH_DTYPE[dt]
    for i, (B, Cc, H, W) in enumerate(K.pool_cases(dt)):
        if Cc != K.chunk_of(C, dt):
            continue
        x = K.pool_input(B, Cc, H, W, 31 + i)
        dy = K.dyadic((B, Cc, H // 2, W // 2), 131 + i, nonzero=True)
        y_ref, dx_ref = K.pool_ref(x, dy)
        xd = _dev(K.nhwc(x), dt).requires_grad_()
        yd = AG.MaxPool2x2Fn.apply(xd)
        yd.backward(_dev(K.nhwc(dy), dt))
        assert torch.equal(K.nchw(yd.detach().cpu()), y_ref.to(td)), (B, Cc, H, W)
        dx = K.nchw(xd.grad.cpu())
        assert torch.equal(dx, dx_ref.to(td)), (B, Cc, H, W)
        assert torch.equal(dx, K.pool_first_max_grad(x, dy).to(td)), (B, Cc, H, W)


# ---- 4. upsample forward -------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("case", K.UPSAMPLE_FWD_CASES, ids=str)
@pytest.mark.parametrize("dt", K.DTYPES)
def test_upsample_add_forward(dt, case):
    """ops.upsample_add: f = 2 / 4 (compile-time stride) and 8 (runtime stride), one chunk to 256 channels, maps one pixel high or wide, skip and skip=None."""
    _, _, ops, _ = _mods()
    B, f, C, H, W, with_skip = case
    C = K.chunk_of(C, dt)
    i = K.UPSAMPLE_FWD_CASES.index(case)
    x, w = K.dyadic((B, C, H, W), 41 + i), K.tap_weights(C, f, 141 + i)
    skip = K.dyadic((B, C, H * f, W * f), 241 + i) if with_skip else None
    ref = K.upsample_ref(x, w, skip, f)
    y = ops.upsample_add(_dev(K.nhwc(x), dt), ops.pack_upsample(w.to(DEV)), f, skip=_dev(K.nhwc(skip), dt) if with_skip else None)
    assert y.shape == (B, H * f, W * f, C)
    assert torch.equal(K.nchw(y.cpu()), ref.to(K.TORCH_DTYPE[dt]))


def _within(got, ref, abs_sum, n, dt, what):
    err = (got.double() - ref).abs()
    bound = K.randn_bound(ref, abs_sum, n, dt)
    print("%s %s: max err %.3e, max err / bound %.3f" % (what, dt, float(err.max()), float((err / bound.clamp(min=1e-300)).max())))
    assert bool((err <= bound).all()), what


@pytest.mark.parametrize("dt", K.DTYPES)
def test_upsample_add_forward_randn(dt):
    """Realistic magnitudes, bounded per element: 4 products + skip (n = 5), S = the same sum over absolute values."""
    _, _, ops, _ = _mods()
    B, f, C, H, W, _ = K.UPSAMPLE_FWD_RANDN
    x, w, skip, _ = K.upsample_bwd_inputs(dt, B, C, f, H, W, 42, randn=True)
    y = ops.upsample_add(_dev(K.nhwc(x), dt), ops.pack_upsample(w.float().to(DEV)), f, skip=_dev(K.nhwc(skip), dt))
    wf = w.float().double()
    _within(K.nchw(y.cpu()), K.upsample_ref(x, wf, skip, f), K.upsample_ref(x.abs(), wf.abs(), skip.abs(), f), 5, dt, "upsample forward")


# ---- 5. upsample backward ------------------------------------------------------------------------------------------------------------------

def _upsample_autograd(AG, dt, x, w, skip, dy, f):
    xd, sd = _dev(K.nhwc(x), dt).requires_grad_(), _dev(K.nhwc(skip), dt).requires_grad_()
    wd = w.float().to(DEV).requires_grad_()
    yd = AG.UpsampleAddFn.apply(xd, wd, sd, f)
    yd.backward(_dev(K.nhwc(dy), dt))
    return yd.detach().cpu(), xd.grad.cpu(), wd.grad.cpu(), sd.grad.cpu()


@pytest.mark.parametrize("name", sorted(K.UPSAMPLE_BWD_CASES))
@pytest.mark.parametrize("dt", K.DTYPES)
def test_upsample_backward_autograd(dt, name):
    """UpsampleAddFn -> mfx_upsample_bwd_nhwc_oihw (workspace form, dw in the parameter's (C, 1, 2f, 2f) layout): y, dx, dw exact, the skip
    gradient is dy itself.  `name` says which branch of upsample_bwd_dw_kernel the case reaches (module docstring)."""
    _, _, _, AG = _mods()
    B, C, f, H, W = K.UPSAMPLE_BWD_CASES[name]
    td = K.TORCH_DTYPE[dt]
    x, w, skip, dy = K.upsample_bwd_inputs(dt, B, C, f, H, W, 51)
    y_ref, dx_ref, dw_ref = K.upsample_ref(x, w, skip, f, dy)
    y, dx, dw, ds = _upsample_autograd(AG, dt, x, w, skip, dy, f)
    assert torch.equal(K.nchw(y), y_ref.to(td))
    assert torch.equal(K.nchw(dx), dx_ref.to(td))
    assert dw.shape == w.shape and dw.dtype == torch.float32 and torch.equal(dw, dw_ref.float())
    assert torch.equal(K.nchw(ds), dy.to(td))


@pytest.mark.parametrize("workspace", (True, False), ids=("workspace", "atomic"))
@pytest.mark.parametrize("name", sorted(K.UPSAMPLE_BWD_CASES))
@pytest.mark.parametrize("dt", K.DTYPES)
def test_upsample_backward_direct_entry(dt, name, workspace):
    """mfx_upsample_bwd_nhwc, dw in the [tap][C] layout, with the workspace (ordered partial sums) and without (fp32 atomics: dw holds canaries
    and the entry has to zero it itself)."""
    lib, L, _, _ = _mods()
    B, C, f, H, W = K.UPSAMPLE_BWD_CASES[name]
    td = K.TORCH_DTYPE[dt]
    x, w, skip, dy = K.upsample_bwd_inputs(dt, B, C, f, H, W, 51)
    _, dx_ref, dw_ref = K.upsample_ref(x, w, skip, f, dy)
    taps = 4 * f * f
    ndx, ndw = B * H * W * C, taps * C
    dx, dw = _guarded(ndx, td), _guarded(ndw, torch.float32)
    nws = lib.mfx_upsample_bwd_workspace_bytes(B, H, C, f) if workspace else 0
    ws = _guarded(nws // 4, torch.float32) if workspace else None
    wt = w.float().reshape(C, taps).t().contiguous().to(DEV)
    xd, dyd = _dev(K.nhwc(x), dt), _dev(K.nhwc(dy), dt)
    L.check(lib.mfx_upsample_bwd_nhwc(_p(xd), _p(wt), _p(dyd), _p(dx), _p(dw), B, H, W, C, f, _code(L, dt),
                                      _p(ws) if workspace else None, nws, _stream()), "mfx_upsample_bwd_nhwc")
    assert torch.equal(K.nchw(dx[:ndx].view(B, H, W, C).cpu()), dx_ref.to(td))
    assert torch.equal(dw[:ndw].view(taps, C).cpu(), dw_ref.float().reshape(C, taps).t())
    assert _guard_intact(dx, ndx) and _guard_intact(dw, ndw)
    if workspace:
        assert nws == K.dw_plan(dt, B, C, f, H, W, True)["blocks"] * ndw * 4 and _guard_intact(ws, nws // 4)


@pytest.mark.parametrize("dt", K.DTYPES)
def test_upsample_backward_randn(dt):
    """Realistic magnitudes, bounded per element: dx sums (2f)^2 products dy * w, dw sums B H W products x * dy (fp32 output: no output rounding)."""
    _, _, _, AG = _mods()
    B, C, f, H, W = K.UPSAMPLE_BWD_RANDN
    x, w, skip, dy = K.upsample_bwd_inputs(dt, B, C, f, H, W, 52, randn=True)
    wf = w.float().double()
    _, dx_ref, dw_ref = K.upsample_ref(x, wf, skip, f, dy)
    _, dx_abs, dw_abs = K.upsample_ref(x.abs(), wf.abs(), skip, f, dy.abs())
    _, dx, dw, _ = _upsample_autograd(AG, dt, x, wf, skip, dy, f)
    _within(K.nchw(dx), dx_ref, dx_abs, 4 * f * f, dt, "upsample dx")
    _within(dw, dw_ref, dw_abs, B * H * W, "fp32", "upsample dw (%s activations)" % dt)


def test_upsample_backward_rejects_non_power_of_two_items():
    """fp32, C = 24, f = 2: 16 taps x 6 chunks = 96 items.  Both entries and both forms return MFX_ERR_ARG and launch nothing: dx and dw keep
    their canaries (the atomic form zero-fills dw only after the shape is accepted)."""
    lib, L, _, AG = _mods()
    dt, B, C, f, H, W = K.UPSAMPLE_BWD_BAD_ITEMS
    x, w, skip, dy = K.upsample_bwd_inputs(dt, B, C, f, H, W, 53)
    taps = 4 * f * f
    wt = w.float().reshape(C, taps).t().contiguous().to(DEV)
    xd, dyd = _dev(K.nhwc(x), dt), _dev(K.nhwc(dy), dt)
    nws = lib.mfx_upsample_bwd_workspace_bytes(B, H, C, f)
    for entry, with_ws in ((lib.mfx_upsample_bwd_nhwc, True), (lib.mfx_upsample_bwd_nhwc, False), (lib.mfx_upsample_bwd_nhwc_oihw, True)):
        dx, dw, ws = _guarded(B * H * W * C, torch.float32), _guarded(taps * C, torch.float32), _guarded(nws // 4, torch.float32)
        rc = entry(_p(xd), _p(wt), _p(dyd), _p(dx), _p(dw), B, H, W, C, f, _code(L, dt), _p(ws) if with_ws else None, nws if with_ws else 0, _stream())
        assert rc == MFX_ERR_ARG, rc
        assert b"power of two" in lib.mfx_last_error()
        torch.cuda.synchronize()
        assert _untouched(dx) and _untouched(dw) and _untouched(ws), with_ws
    xg = xd.clone().requires_grad_()
    y = AG.UpsampleAddFn.apply(xg, w.float().to(DEV).requires_grad_(), _dev(K.nhwc(skip), dt), f)       # the forward has no such limit
    assert torch.equal(K.nchw(y.detach().cpu()), K.upsample_ref(x, w, skip, f).float())
    with pytest.raises(RuntimeError, match="power of two"):
        y.backward(dyd)


# ---- 6. zero insertion -------------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("case", K.ZERO_INSERT_CASES, ids=str)
@pytest.mark.parametrize("dt", K.DTYPES)
def test_zero_insert2(dt, case):
    """mfx_zero_insert2_nhwc: dy at the even (h, w), exact zeros elsewhere; H = 2 Ho and H = 2 Ho - 1."""
    lib, L, _, _ = _mods()
    B, Ho, Wo, C, H, W = case
    C = K.chunk_of(C, dt)
    dy = K.dyadic((B, Ho, Wo, C), 61 + K.ZERO_INSERT_CASES.index(case), nonzero=True)
    n = B * H * W * C
    buf = _guarded(n, K.TORCH_DTYPE[dt])
    dyd = _dev(dy, dt)
    L.check(lib.mfx_zero_insert2_nhwc(_p(dyd), _p(buf), B, Ho, Wo, C, H, W, _code(L, dt), _stream()), "mfx_zero_insert2_nhwc")
    assert torch.equal(buf[:n].view(B, H, W, C).cpu(), K.zero_insert_ref(dy, H, W).to(K.TORCH_DTYPE[dt]))
    assert _guard_intact(buf, n)


# ---- 7. column sums ------------------------------------------------------------------------------------------------------------------------------

def _colsum_case(dt, M, C, ld, deterministic):
    lib, L, _, _ = _mods()
    if deterministic:
        L.check(lib.mfx_set_option(b"deterministic", 1), "set_option(deterministic)")      # (the autouse fixture of conftest.py resets it)
    x = K.colsum_input(M, C, ld, 71)
    ref = x[:, :C].sum(0)
    xd = _dev(x, dt)
    out = _guarded(C, torch.float32)
    L.check(lib.mfx_colsum(_p(xd), _p(out), M, C, ld, _code(L, dt), _stream()), "mfx_colsum")
    assert torch.equal(out[:C].cpu(), ref.float()), "colsum"
    assert _guard_intact(out, C)
    start = K.dyadic((C,), 72, nonzero=True)
    out = _guarded(C, torch.float32, fill=start)
    L.check(lib.mfx_colsum_add(_p(xd), _p(out), M, C, ld, _code(L, dt), _stream()), "mfx_colsum_add")
    assert torch.equal(out[:C].cpu(), (start + ref).float()), "colsum_add"
    assert _guard_intact(out, C)


def _colsum_params(cases):
    return [pytest.param(dt, M, C, ld, id="%s-%s-%s-%s" % (dt, M, C, ld)) for (M, C, ld, dts) in cases for dt in dts]


@pytest.mark.parametrize("dt,M,C,ld", _colsum_params(K.COLSUM_CHUNK_CASES))
def test_colsum_chunk_route(dt, M, C, ld):
    """mfx_colsum / mfx_colsum_add on colsum_chunk_kernel: one row, ragged row blocks, ld != C (the padding columns hold 1024 and are never summed)."""
    assert K.colsum_route(dt, C, ld) == "chunk"
    _colsum_case(dt, M, C, ld, False)


@pytest.mark.parametrize("dt,M,C,ld", _colsum_params(K.COLSUM_GENERIC_CASES))
def test_colsum_generic_route(dt, M, C, ld):
    """mfx_colsum / mfx_colsum_add on colsum_kernel: odd C, C > 64, a ragged last row block, M >= 2^18 (1024 rows per workgroup)."""
    C, ld = K.chunk_of(C, dt), K.chunk_of(ld, dt)
    assert K.colsum_route(dt, C, ld) == "generic"
    _colsum_case(dt, M, C, ld, False)


@pytest.mark.parametrize("dt,M,C,ld", _colsum_params(K.COLSUM_DETERMINISTIC_CASES))
def test_colsum_deterministic(dt, M, C, ld):
    """Option `deterministic`: one workgroup per destination on both routes; the same exact sums."""
    _colsum_case(dt, M, C, ld, True)


@pytest.mark.parametrize("dt", K.DTYPES)
def test_colsum_randn(dt):
    """Realistic magnitudes, bounded per element: n = M terms, S = the column sum of absolute values, fp32 output."""
    lib, L, _, _ = _mods()
    M, C, ld = K.COLSUM_RANDN
    x = torch.randn(M, ld, generator=torch.Generator().manual_seed(73)).to(K.TORCH_DTYPE[dt])
    out = _guarded(C, torch.float32)
    xd = x.to(DEV)
    L.check(lib.mfx_colsum(_p(xd), _p(out), M, C, ld, _code(L, dt), _stream()), "mfx_colsum")
    _within(out[:C].cpu(), x.double().sum(0), x.double().abs().sum(0), M, "fp32", "colsum (%s input)" % dt)
    assert _guard_intact(out, C)


# ---- 8. edge scatter-add ---------------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("ch_off,C,with_planar", K.EDGE_CASES)
def test_edge_scatter_add(ch_off, C, with_planar):
    """ops.edge_scatter_add, ldv (4) != C, edge_len [0, 16, 7]: the listed elements become out + v exactly (the planar copy too), every other
    element of the map, the planar buffer and the guards behind them is unchanged.  Ignored points (j >= edge_len) all name one in-range pixel
    that holds canaries."""
    _, _, ops, _ = _mods()
    e = K.EDGE
    out, v, xy, n = K.edge_inputs(81)
    cx, cy = e["canary_pixel"]
    out[:, cy, cx] = K.CANARY
    planar = K.dyadic((e["B"], C, e["H"] * e["W"]), 82).float() if with_planar else None
    if with_planar:
        planar[:, :, cy * e["W"] + cx] = K.CANARY
    out_ref, planar_ref = K.edge_scatter_ref(out, ch_off, C, v, xy, n, planar)
    obuf = _guarded(out.numel(), torch.float32, fill=out)
    pbuf = _guarded(planar.numel(), torch.float32, fill=planar) if with_planar else None
    ops.edge_scatter_add(obuf[:out.numel()].view(out.shape), ch_off, C, v.to(DEV), xy.to(DEV), n.to(DEV),
                         planar=pbuf[:planar.numel()].view(planar.shape) if with_planar else None)
    got = obuf[:out.numel()].view(out.shape).cpu()
    assert torch.equal(got, out_ref)
    assert int((got != out).sum()) == C * sum(e["edge_len"]) and bool((got[:, cy, cx] == K.CANARY).all())
    assert _guard_intact(obuf, out.numel())
    if with_planar:
        assert torch.equal(pbuf[:planar.numel()].view(planar.shape).cpu(), planar_ref)
        assert _guard_intact(pbuf, planar.numel())
