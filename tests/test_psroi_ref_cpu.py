"""Known answers that pin tests/psroi_ref.py, the float64 restatement of the reference's deformable PSROI pooling every other psroi
test compares against.  None of them depends on the code under test."""
import numpy as np
import pytest

from tests import psroi_ref as R


def _inside_case(seed, shape=(2, 4, 12, 14), n_rois=3, scale=0.25, pooled=3, part=3, S=2, classes=2, trans_std=0.1):
    """ROIs well inside the map and small offsets: no sample is dropped or clamped."""
    rng = np.random.default_rng(seed)
    B, C, H, W = shape
    rois = np.zeros((n_rois, 5))
    for i in range(n_rois):
        x1, y1 = rng.integers(12, 20), rng.integers(10, 16)
        rois[i] = (i % B, x1, y1, x1 + rng.integers(9, 18), y1 + rng.integers(9, 18))
    d = {"input": rng.standard_normal(shape), "rois": rois, "trans": rng.standard_normal((n_rois, 2 * classes, part, part)) * 0.5,
         "grad_out": rng.standard_normal((n_rois, C, pooled, pooled)), "args": (scale, C, 1, pooled, part, S, trans_std)}
    m = R.margins(shape, rois, d["trans"], False, scale, C, pooled, part, S, trans_std)
    return d, m


def test_round_is_half_away_from_zero():
    assert R.c_round(np.float64(2.5)) == 3 and R.c_round(np.float64(-2.5)) == -3 and R.c_round(np.float64(3.5)) == 4
    assert R.c_round(np.float32(0.5)) == 1 and R.c_round(np.float64(2.4999)) == 2 and np.round(2.5) == 2      # (numpy rounds half to even)
    x = np.random.default_rng(0).standard_normal((1, 2, 16, 16))
    args = (1.0, 2, 1, 2, 2, 2, 0.0)
    half = R.forward(x, np.array([[0, 2.5, 2.5, 6.5, 6.5]]), None, True, *args)[0]
    up = R.forward(x, np.array([[0, 3.0, 3.0, 7.0, 7.0]]), None, True, *args)[0]
    down = R.forward(x, np.array([[0, 2.0, 2.0, 6.0, 6.0]]), None, True, *args)[0]
    assert np.array_equal(half, up) and not np.allclose(half, down)


def test_constant_input_gives_the_constant_wherever_a_sample_was_kept():
    for case in R.CASES[:3]:
        d = R.case_inputs(case)
        const = np.full(case[0], 1.75)
        for no_trans in (True, False):
            out, cnt = R.forward(const, d["rois"], None if no_trans else d["trans"], no_trans, *d["args"])
            assert (cnt > 0).any() and (cnt == 0).any()
            assert np.abs(out[cnt > 0] - 1.75).max() < 1e-12 and (out[cnt == 0] == 0).all()


def test_no_trans_equals_zero_offsets_and_zero_trans_std():
    d = R.case_inputs(R.CASES[2])
    a = d["args"]
    plain = R.forward(d["input"], d["rois"], None, True, *a)
    zero = R.forward(d["input"], d["rois"], np.zeros_like(d["trans"]), False, *a)
    nostd = R.forward(d["input"], d["rois"], d["trans"], False, *(a[:-1] + (0.0,)))
    for other in (zero, nostd):
        assert np.array_equal(plain[0], other[0]) and np.array_equal(plain[1], other[1])
    moved = R.forward(d["input"], d["rois"], d["trans"], False, *a)
    assert not np.allclose(plain[0], moved[0])


def test_linear_ramp_gives_the_ramp_at_the_mean_sample_position():
    d, m = _inside_case(3)
    assert m["kept"] == m["samples"] and m["clamped"] == 0
    scale, C, _, pooled, part, S, trans_std = d["args"]
    B, _, H, W = d["input"].shape
    a, b, c = 0.3, -0.7, 1.1
    ys, xs = np.mgrid[0:H, 0:W]
    ramp = np.broadcast_to(a * xs + b * ys + c, (B, C, H, W)).copy()
    out, cnt = R.forward(ramp, d["rois"], d["trans"], False, *d["args"])
    assert (cnt == S * S).all()
    cpc = C // (d["trans"].shape[1] // 2)
    for n, r in enumerate(d["rois"]):
        start_w, start_h = r[1] * scale - 0.5, r[2] * scale - 0.5
        roi_w, roi_h = (r[3] + 1) * scale - 0.5 - start_w, (r[4] + 1) * scale - 0.5 - start_h
        for ch in range(C):
            for ph in range(pooled):
                for pw in range(pooled):
                    tx, ty = d["trans"][n, 2 * (ch // cpc), ph, pw] * trans_std, d["trans"][n, 2 * (ch // cpc) + 1, ph, pw] * trans_std
                    mx = start_w + pw * roi_w / pooled + tx * roi_w + (S - 1) / 2 * roi_w / pooled / S
                    my = start_h + ph * roi_h / pooled + ty * roi_h + (S - 1) / 2 * roi_h / pooled / S
                    assert abs(out[n, ch, ph, pw] - (a * mx + b * my + c)) < 1e-12


def test_offset_of_k_pixels_equals_the_roi_moved_by_k_pixels():
    d, _ = _inside_case(4, classes=1)
    scale, C, _, pooled, part, S, trans_std = d["args"]
    k = 2                                                            # feature pixels = k / scale image pixels
    r = d["rois"]
    roi_w = (r[:, 3] + 1) * scale - r[:, 1] * scale
    trans = np.zeros_like(d["trans"])
    trans[:, 0] = (k / (trans_std * roi_w))[:, None, None]
    moved = r.copy()
    moved[:, 1] += k / scale
    moved[:, 3] += k / scale
    a, ca = R.forward(d["input"], r, trans, False, *d["args"])
    b, cb = R.forward(d["input"], moved, None, True, *d["args"])
    assert np.array_equal(ca, cb) and np.abs(a - b).max() < 1e-12 and not np.allclose(a, R.forward(d["input"], r, None, True, *d["args"])[0])


def test_explicit_backward_agrees_with_central_differences_of_the_forward():
    """Where no sample is dropped or clamped and none is within 1e-3 of a grid line, the reference's backward formulas ARE the derivative."""
    d, m = _inside_case(9)                                           # (seed chosen for the grid margin asserted next)
    assert m["kept"] == m["samples"] and m["clamped"] == 0 and m["grid"] >= 1e-3, m
    a = d["args"]
    out, cnt = R.forward(d["input"], d["rois"], d["trans"], False, *a)
    gi, gt = R.backward(d["grad_out"], d["input"], d["rois"], d["trans"], cnt, False, *a)
    loss = lambda x, t: float((R.forward(x, d["rois"], t, False, *a)[0] * d["grad_out"]).sum())
    rng = np.random.default_rng(0)
    eps = 1e-6
    touched = np.argwhere(gi != 0)
    assert len(touched) > 100
    for idx in list(touched[rng.choice(len(touched), 60, replace=False)]) + [np.array(np.unravel_index(i, gi.shape)) for i in rng.choice(gi.size, 20)]:
        hi, lo = d["input"].copy(), d["input"].copy()
        hi[tuple(idx)] += eps
        lo[tuple(idx)] -= eps
        num = (loss(hi, d["trans"]) - loss(lo, d["trans"])) / (2 * eps)
        assert abs(num - gi[tuple(idx)]) < 1e-7 * max(1.0, abs(num)), (idx, num, gi[tuple(idx)])
    assert m["grid"] > 10 * eps * a[-1] * 5                           # an offset step of eps moves a sample by eps * trans_std * roi size (< 5 px)
    for i in range(gt.size):
        idx = np.unravel_index(i, gt.shape)
        hi, lo = d["trans"].copy(), d["trans"].copy()
        hi[idx] += eps
        lo[idx] -= eps
        num = (loss(d["input"], hi) - loss(d["input"], lo)) / (2 * eps)
        assert abs(num - gt[idx]) < 1e-7 * max(1.0, abs(num)), (idx, num, gt[idx])
    assert np.abs(gt).max() > 1e-2


def test_reference_self_test_case_centre_bins():
    """testcuda.py:100-131: the centre bin of every channel lies wholly inside its block of 1.0 / 2.0; the border bins reach 0.25 px outside
    it, so the per-ROI MEAN is below 1.0 / 2.0."""
    x = np.zeros((2, 16, 64, 64))
    x[0, :, 16:26, 16:26] = 1.0
    x[1, :, 10:20, 20:30] = 2.0
    rois = np.array([[0, 65, 65, 103, 103], [1, 81, 41, 119, 79]], dtype=np.float64)
    args = (0.25, 16, 1, 7, 7, 4, 0.0)
    out, cnt = R.forward(x, rois, None, True, *args)
    assert (cnt == 16).all()
    assert np.abs(out[0, :, 3, 3] - 1.0).max() < 1e-12 and np.abs(out[1, :, 3, 3] - 2.0).max() < 1e-12
    assert out[0, 0, 0, 0] < 1.0 - 1e-3 and out[1, 0, 6, 6] < 2.0 - 1e-3 and out[0].mean() < 1.0 - 1e-3 and out[1].mean() < 2.0 - 1e-3
    dout, dcnt = R.forward(x, rois, np.zeros((20, 2, 7, 7)), False, *args)
    assert np.array_equal(out, dout) and np.array_equal(cnt, dcnt)


def test_roi_of_no_image_and_tiny_rois():
    x = np.random.default_rng(1).standard_normal((2, 2, 8, 8))
    rois = np.array([[-1, 4, 4, 20, 20], [2, 4, 4, 20, 20], [1, 4, 4, 20, 20], [0, 8, 8, 7, 7]], dtype=np.float64)
    args = (0.25, 2, 1, 2, 2, 2, 0.0)
    out, cnt = R.forward(x, rois, None, True, *args)
    assert (out[:2] == 0).all() and (cnt[:2] == 0).all() and (cnt[2] > 0).all()
    assert (cnt[3] == 4).all()                                       # x2 < x1: width floored at 0.1, still sampled
    gi, _ = R.backward(np.ones_like(out), x, rois, None, cnt, True, *args)
    assert (gi[0] != 0).any() and abs(gi.sum() - (cnt[2:] > 0).sum()) < 1e-9


@pytest.mark.parametrize("i", range(len(R.CASES)))
def test_committed_seeds_meet_the_margin_conditions(i):
    d = R.case_inputs(R.CASES[i])
    for no_trans in (True, False):
        R.check_case_conditions(R.CASES[i], d, no_trans, need_grid=False)
    if i < len(R.GOFF_CASES):
        g = R.case_inputs(R.GOFF_CASES[i])
        R.check_case_conditions(R.GOFF_CASES[i], g, False, need_grid=True)
