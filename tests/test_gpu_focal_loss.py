"""mfx_focal_loss (csrc/loss_kernels.hip: sigmoid + clamp + penalty-reduced focal loss + its gradient in one pass), called
directly through the library over its own shape space, against the float64 evaluation of the reference's focal_loss.py with
sigmoid_hm's clamp written out below.

The clamp bounds are the float32 numbers float32(1e-4) and float32(1 - 1e-4): the reference clamps a float32 tensor, so a
saturated pixel carries 1 - float32(0.9999) = 1.00017e-4, not 1e-4.  Logits in 9.20 <= |z| <= 9.22 are moved out of that band
(there fp32 and fp64 disagree on which side of the clamp a pixel lies).

Shapes: one element; less than one workgroup; ragged with four classes; one class; 276480 elements (> 1024*256: the grid-stride
loop's second trip).  Content: randn*3 logits with +-12, +-20, +-80 planted under positive and negative targets; targets with
exact 1.0 peaks, Gaussian shoulders, 0.0 and nextafter(1, 0).

Bounds (tests/test_gpu_train.py): loss sum 3e-5*max(1,|ref|), positive count exact, gradient 2e-5*max(1e-3, max|ref|) for
every element; on saturated pixels the gradient is exactly 0.
"""
import ctypes
import os
import sys

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

pytestmark = pytest.mark.gpu
DEV = "cuda"
P_LO, P_HI = float(np.float32(1e-4)), float(np.float32(1 - 1e-4))
NEAR_ONE = float(np.nextafter(np.float32(1), np.float32(0)))
PLANTED_Z = (12.0, -12.0, 20.0, -20.0, 80.0, -80.0)
SHAPES = [(1, 1, 1, 1), (2, 5, 7, 3), (1, 33, 65, 4), (2, 24, 40, 1), (3, 96, 320, 3)]
ALPHA_BETA = [(2.0, 4.0), (1.0, 1.0), (3.0, 2.0)]


def focal_reference(z, t, alpha, beta):
    """float64: (loss_sum, num_pos, d loss_sum / d z, saturated mask) for NHWC logits z and the NCHW target map t."""
    z64 = z.double().requires_grad_()
    s = torch.sigmoid(z64)
    p = s.clamp(min=P_LO, max=P_HI)                                            # sigmoid_hm
    tt = t.permute(0, 2, 3, 1).double()
    pos = tt.eq(1).double()
    neg = (tt.lt(1) & tt.ge(0)).double()
    pos_loss = torch.log(p) * torch.pow(1 - p, alpha) * pos
    neg_loss = torch.log(1 - p) * torch.pow(p, alpha) * torch.pow(1 - tt, beta) * neg
    loss = -neg_loss.sum() - pos_loss.sum()
    g, = torch.autograd.grad(loss, z64)
    sat = (s.detach() < P_LO) | (s.detach() > P_HI)
    return float(loss.detach()), float(pos.sum()), g, sat


def make_maps(shape, seed, positives=True):
    B, H, W, C = shape
    g = torch.Generator().manual_seed(seed)
    z = torch.randn(B, H, W, C, generator=g) * 3
    band = (z.abs() >= 9.19) & (z.abs() <= 9.23)
    z = torch.where(band, z.sign() * 9.0, z)
    ys, xs = torch.meshgrid(torch.arange(H, dtype=torch.float32), torch.arange(W, dtype=torch.float32), indexing="ij")
    t = torch.zeros(B, C, H, W)
    for b in range(B):
        for c in range(C):
            for k in range(2):                                                # Gaussian shoulders around an exact 1.0 peak
                cy, cx = int(torch.randint(0, H, (1,), generator=g)), int(torch.randint(0, W, (1,), generator=g))
                sig = 0.8 + 1.5 * k
                hill = torch.exp(-((xs - cx) ** 2 + (ys - cy) ** 2) / (2 * sig * sig))
                hill[cy, cx] = 1.0 if positives else 0.9
                t[b, c] = torch.maximum(t[b, c], hill)
    t[t < 1e-3] = 0.0
    n = z.numel()
    if n >= 4 * len(PLANTED_Z):
        # saturated logits on both sides, under a positive, a zero, a shoulder and an almost-one target
        kinds = (1.0 if positives else 0.0, 0.0, 0.5, NEAR_ONE)
        slots = torch.randperm(n, generator=g)[:4 * len(PLANTED_Z)].tolist()
        zf, tf = z.view(-1), t.permute(0, 2, 3, 1).contiguous().view(-1)
        for i, flat in enumerate(slots):
            zf[flat], tf[flat] = PLANTED_Z[i % len(PLANTED_Z)], kinds[i // len(PLANTED_Z)]
        t = tf.view(B, H, W, C).permute(0, 3, 1, 2).contiguous()
    return z.contiguous(), t.contiguous()


def run_kernel(z, t, alpha, beta):
    from monoflex_amd import lib as L
    B, H, W, C = z.shape
    zd, td = z.to(DEV).contiguous(), t.to(DEV).contiguous()
    sums = torch.full((2,), float("nan"), device=DEV)
    dz = torch.full_like(zd, float("nan"))
    stream = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
    L.check(L.load().mfx_focal_loss(ctypes.c_void_p(zd.data_ptr()), ctypes.c_void_p(td.data_ptr()), B, H, W, C, ctypes.c_float(alpha),
                                    ctypes.c_float(beta), ctypes.c_void_p(sums.data_ptr()), ctypes.c_void_p(dz.data_ptr()), stream), "mfx_focal_loss")
    torch.cuda.synchronize()
    return sums.cpu(), dz.cpu()


def check(z, t, alpha, beta, what):
    loss, npos, g, sat = focal_reference(z, t, alpha, beta)
    sums, dz = run_kernel(z, t, alpha, beta)
    e_loss = abs(float(sums[0]) - loss) / (3e-5 * max(1.0, abs(loss)))
    gmax = float(g.abs().max())
    e_grad = float((dz.double() - g).abs().max()) / (2e-5 * max(1e-3, gmax))
    print("%s: loss %.6g (ref %.6g, error/bound %.3f), positives %d, max|grad| %.4g, gradient error/bound %.3f, saturated %d"
          % (what, float(sums[0]), loss, e_loss, int(npos), gmax, e_grad, int(sat.sum())))
    assert float(sums[1]) == npos
    assert e_loss <= 1.0
    assert bool(torch.isfinite(dz).all()) and e_grad <= 1.0
    assert float(dz[sat].abs().max() if sat.any() else 0.0) == 0.0 and float(g[sat].abs().max() if sat.any() else 0.0) == 0.0
    return sums, dz, sat


@pytest.mark.parametrize("alpha,beta", ALPHA_BETA)
@pytest.mark.parametrize("shape", SHAPES)
def test_focal_kernel_vs_float64(shape, alpha, beta):
    z, t = make_maps(shape, seed=11 + sum(shape))
    if shape == (1, 1, 1, 1):
        z[...], t[...] = 0.7, 1.0
    _, _, sat = check(z, t, alpha, beta, "focal %s alpha %g beta %g" % (shape, alpha, beta))
    if z.numel() >= 4 * len(PLANTED_Z):
        assert int(sat.sum()) >= 4 * len(PLANTED_Z) and int(t.eq(1).sum()) >= 1 and int((t == NEAR_ONE).sum()) >= len(PLANTED_Z)


@pytest.mark.parametrize("alpha,beta", ALPHA_BETA)
@pytest.mark.parametrize("target", [1.0, 0.0, 0.5, NEAR_ONE])
def test_focal_kernel_one_saturated_pixel(target, alpha, beta):
    """A (1,1,1,1) map whose only pixel is saturated: the loss sum IS that pixel's contribution -- the clamped value's -- and its
    gradient is exactly 0, on both sides of the clamp and under every target kind."""
    for zval in PLANTED_Z:
        z, t = torch.full((1, 1, 1, 1), zval), torch.full((1, 1, 1, 1), target)
        p = P_HI if zval > 0 else P_LO
        want = -np.log(p) * (1 - p) ** alpha if target == 1.0 else -np.log1p(-p) * p ** alpha * (1 - float(np.float32(target))) ** beta
        sums, dz, sat = check(z, t, alpha, beta, "one pixel z %g target %r" % (zval, target))
        assert bool(sat.all()) and float(dz.abs().max()) == 0.0
        assert abs(float(sums[0]) - want) <= 3e-5 * max(1.0, abs(want)), (float(sums[0]), want)


@pytest.mark.parametrize("shape", [(2, 5, 7, 3), (3, 96, 320, 3)])
def test_focal_kernel_map_without_positives(shape):
    z, t = make_maps(shape, seed=5, positives=False)
    assert int(t.eq(1).sum()) == 0
    sums, _, _ = check(z, t, 2.0, 4.0, "focal %s without positives" % (shape,))
    assert float(sums[1]) == 0.0


@pytest.mark.parametrize("shape", [(2, 5, 7, 3), (1, 33, 65, 4), (3, 96, 320, 3)])
def test_focal_kernel_deterministic_option(shape):
    """Option `deterministic` (one workgroup, a single writer of the two sums): two runs agree bit for bit, meet the reference,
    and agree with the default mode within the loss bound; the gradient is elementwise and so identical in both modes."""
    from monoflex_amd import lib as L
    z, t = make_maps(shape, seed=23)
    base_sums, base_dz, _ = check(z, t, 2.0, 4.0, "focal %s default mode" % (shape,))
    lib_ = L.load()
    L.check(lib_.mfx_set_option(b"deterministic", 1), "opt")
    try:
        a_sums, a_dz, _ = check(z, t, 2.0, 4.0, "focal %s deterministic" % (shape,))
        b_sums, b_dz = run_kernel(z, t, 2.0, 4.0)
    finally:
        L.check(lib_.mfx_set_option(b"deterministic", 0), "opt")
    assert torch.equal(a_sums, b_sums) and torch.equal(a_dz, b_dz)
    assert abs(float(a_sums[0]) - float(base_sums[0])) <= 3e-5 * max(1.0, abs(float(base_sums[0]))) and float(a_sums[1]) == float(base_sums[1])
    assert torch.equal(a_dz, base_dz)
