"""numpy restatement of the reference's deformable PSROI pooling (helper module of the psroi tests, not a test file).

Every expression cites model/backbone/DCNv2/src/cuda/dcn_v2_psroi_pooling_cuda.cu of the reference (`:N` below).  The arithmetic runs in
`dtype`: numpy.float64 is the reference the tests compare against, numpy.float32 is "the reference arithmetic in fp32" -- what the
reference's own float kernel computes -- and its distance to the float64 result is the unit the tests' bounds are measured in.

The backward is coded from the reference's formulas (:209-265), NOT obtained by differentiating the forward: where a sample was clamped
to the map the offset gradient ignores the clamp.

Two points where this restatement follows this project and not the reference's text: a ROI whose batch index is outside [0, B) gives
output 0, count 0 and no gradient (the reference reads out of bounds), and group_size must be 1 (with channels == output_dim, :295, any
other value indexes past the input).
"""
from collections import namedtuple

import numpy as np

SampleRec = namedtuple("SampleRec", "n cls ph pw part_h part_w batch w h valid clamped_x clamped_y x0 x1 y0 y1 dx dy roi_w roi_h")


def c_round(x):
    """C `round`: half away from zero (:89-92), not numpy's half-to-even."""
    x = np.asarray(x)
    return np.sign(x) * np.floor(np.abs(x) + x.dtype.type(0.5))


def num_classes_of(trans, no_trans):
    return 1 if no_trans else trans.shape[1] // 2                                     # :303


def iter_samples(rois, trans, no_trans, spatial_scale, output_dim, pooled, part, S, trans_std, B, H, W, dtype=np.float64):
    """Every (roi, class, bin, sample) in the reference's loop order, with its geometry in `dtype`.  ROIs of no image are left out."""
    T = dtype
    rois = np.asarray(rois, dtype=T)
    trans = None if no_trans else np.asarray(trans, dtype=T)
    scale, tstd, half = T(spatial_scale), T(trans_std), T(0.5)
    ncls = num_classes_of(trans, no_trans)
    for n in range(rois.shape[0]):
        batch = int(rois[n, 0])                                                       # :88 (truncation)
        if batch < 0 or batch >= B:
            continue
        start_w = c_round(rois[n, 1]) * scale - half                                  # :89
        start_h = c_round(rois[n, 2]) * scale - half                                  # :90
        end_w = (c_round(rois[n, 3]) + T(1)) * scale - half                           # :91
        end_h = (c_round(rois[n, 4]) + T(1)) * scale - half                           # :92
        roi_w = max(end_w - start_w, T(0.1))                                          # :95
        roi_h = max(end_h - start_h, T(0.1))                                          # :96
        bin_h, bin_w = roi_h / T(pooled), roi_w / T(pooled)                           # :99-100
        sub_h, sub_w = bin_h / T(S), bin_w / T(S)                                     # :102-103
        for cls in range(ncls):
            for ph in range(pooled):
                for pw in range(pooled):
                    part_h = int(np.floor(T(ph) / T(pooled) * T(part)))               # :105
                    part_w = int(np.floor(T(pw) / T(pooled) * T(part)))               # :106
                    tx = T(0) if no_trans else trans[n, 2 * cls, part_h, part_w] * tstd        # :108
                    ty = T(0) if no_trans else trans[n, 2 * cls + 1, part_h, part_w] * tstd    # :109
                    wstart = T(pw) * bin_w + start_w                                  # :111
                    wstart = wstart + tx * roi_w                                      # :112
                    hstart = T(ph) * bin_h + start_h                                  # :113
                    hstart = hstart + ty * roi_h                                      # :114
                    for ih in range(S):
                        for iw in range(S):
                            w = wstart + T(iw) * sub_w                                # :128
                            h = hstart + T(ih) * sub_h                                # :129
                            valid = not (w < T(-0.5) or w > T(W) - half or h < T(-0.5) or h > T(H) - half)    # :131
                            wc = min(max(w, T(0)), T(W - 1))                          # :135
                            hc = min(max(h, T(0)), T(H - 1))                          # :136
                            x0, x1 = int(np.floor(wc)), int(np.ceil(wc))              # :41-42 / :236-237
                            y0, y1 = int(np.floor(hc)), int(np.ceil(hc))              # :43-44 / :238-239
                            yield SampleRec(n, cls, ph, pw, part_h, part_w, batch, w, h, valid, wc != w, hc != h, x0, x1, y0, y1,
                                            wc - T(x0), hc - T(y0), roi_w, roi_h)     # :45-46 / :240


def _check(inp, trans, no_trans, output_dim, group_size):
    assert inp.shape[1] == output_dim, "input channels and output channels must equal (:295)"
    assert group_size == 1, "group_size must be 1"
    ncls = num_classes_of(trans, no_trans)
    assert output_dim % ncls == 0
    return ncls, output_dim // ncls                                                   # :303-304


def forward(inp, rois, trans, no_trans, spatial_scale, output_dim, group_size, pooled, part, S, trans_std, dtype=np.float64):
    """-> (output, output_count), both (N, output_dim, pooled, pooled) in `dtype`."""
    T = dtype
    inp = np.asarray(inp, dtype=T)
    B, C, H, W = inp.shape
    ncls, cpc = _check(inp, trans, no_trans, output_dim, group_size)
    N = np.asarray(rois).shape[0]
    sums = np.zeros((N, output_dim, pooled, pooled), dtype=T)
    count = np.zeros((N, output_dim, pooled, pooled), dtype=T)
    one = T(1)
    for s in iter_samples(rois, trans, no_trans, spatial_scale, output_dim, pooled, part, S, trans_std, B, H, W, T):
        if not s.valid:
            continue                                                                  # :131-134
        c0, c1 = s.cls * cpc, (s.cls + 1) * cpc                                       # :107 (class_id = ctop / channels_each_class)
        p = inp[s.batch, c0:c1]
        v11, v12, v21, v22 = p[:, s.y0, s.x0], p[:, s.y1, s.x0], p[:, s.y0, s.x1], p[:, s.y1, s.x1]            # :47-50
        val = (one - s.dx) * (one - s.dy) * v11 + (one - s.dx) * s.dy * v12 + s.dx * (one - s.dy) * v21 + s.dx * s.dy * v22   # :51-54
        sums[s.n, c0:c1, s.ph, s.pw] += val                                           # :139
        count[s.n, c0:c1, s.ph, s.pw] += one                                          # :140
    with np.errstate(invalid="ignore", divide="ignore"):
        out = np.where(count == 0, T(0), sums / count)                                # :143
    return out.astype(T), count


def backward(grad_out, inp, rois, trans, count, no_trans, spatial_scale, output_dim, group_size, pooled, part, S, trans_std,
             dtype=np.float64):
    """-> (grad_input (B,C,H,W), grad_trans (shape of trans, or None when no_trans)); `count` is the forward's output_count."""
    T = dtype
    inp, grad_out, count = np.asarray(inp, dtype=T), np.asarray(grad_out, dtype=T), np.asarray(count, dtype=T)
    B, C, H, W = inp.shape
    ncls, cpc = _check(inp, trans, no_trans, output_dim, group_size)
    gi = np.zeros_like(inp)
    gt = None if no_trans else np.zeros(np.asarray(trans).shape, dtype=T)
    one, tstd = T(1), T(trans_std)
    for s in iter_samples(rois, trans, no_trans, spatial_scale, output_dim, pooled, part, S, trans_std, B, H, W, T):
        if not s.valid:
            continue                                                                  # :228-231
        c0, c1 = s.cls * cpc, (s.cls + 1) * cpc
        cnt = count[s.n, c0:c1, s.ph, s.pw]
        live = cnt > 0                                                                # :209-212
        if not live.any():
            continue
        diff_val = np.where(live, grad_out[s.n, c0:c1, s.ph, s.pw] / np.where(live, cnt, one), T(0))           # :213
        q00 = (one - s.dx) * (one - s.dy)                                             # :241
        q01 = (one - s.dx) * s.dy                                                     # :242
        q10 = s.dx * (one - s.dy)                                                     # :243
        q11 = s.dx * s.dy                                                             # :244
        g = gi[s.batch, c0:c1]
        g[:, s.y0, s.x0] += q00 * diff_val                                            # :246
        g[:, s.y1, s.x0] += q01 * diff_val                                            # :247
        g[:, s.y0, s.x1] += q10 * diff_val                                            # :248
        g[:, s.y1, s.x1] += q11 * diff_val                                            # :249
        if no_trans:
            continue                                                                  # :251-254
        p = inp[s.batch, c0:c1]
        u00, u01, u10, u11 = p[:, s.y0, s.x0], p[:, s.y1, s.x0], p[:, s.y0, s.x1], p[:, s.y1, s.x1]            # :255-258
        diff_x = (u11 * s.dy + u10 * (one - s.dy) - u01 * s.dy - u00 * (one - s.dy)) * tstd * diff_val         # :259
        diff_x = diff_x * s.roi_w                                                     # :260
        diff_y = (u11 * s.dx + u01 * (one - s.dx) - u10 * s.dx - u00 * (one - s.dx)) * tstd * diff_val         # :261
        diff_y = diff_y * s.roi_h                                                     # :262
        for dxv, dyv in zip(diff_x[live], diff_y[live]):                              # one add per channel, in channel order (:264-265)
            gt[s.n, 2 * s.cls, s.part_h, s.part_w] += dxv
            gt[s.n, 2 * s.cls + 1, s.part_h, s.part_w] += dyv
    return gi, gt


def margins(inp_shape, rois, trans, no_trans, spatial_scale, output_dim, pooled, part, S, trans_std):
    """How far the samples of an input are from the places where float32 and float64 may legitimately disagree (all in float64):
    `boundary`  min distance of any sample coordinate to a drop boundary (-0.5, W - 0.5, H - 0.5);
    `grid`      min distance of a kept sample's unclamped coordinate to an integer grid line (where the corner pair changes);
    plus the counts `samples`, `kept`, `clamped` (kept samples with a clamped coordinate)."""
    B, C, H, W = inp_shape
    boundary, grid = np.inf, np.inf
    total = kept = clamped = 0
    for s in iter_samples(rois, trans, no_trans, spatial_scale, output_dim, pooled, part, S, trans_std, B, H, W, np.float64):
        total += 1
        boundary = min(boundary, abs(s.w + 0.5), abs(s.w - (W - 0.5)), abs(s.h + 0.5), abs(s.h - (H - 0.5)))
        if not s.valid:
            continue
        kept += 1
        clamped += bool(s.clamped_x or s.clamped_y)
        if not s.clamped_x:
            grid = min(grid, abs(s.w - np.round(s.w)))
        if not s.clamped_y:
            grid = min(grid, abs(s.h - np.round(s.h)))
    return {"boundary": float(boundary), "grid": float(grid), "samples": total, "kept": kept, "clamped": clamped}


def random_case(seed, shape, n_rois, spatial_scale, pooled, part, S, classes, trans_std, bad_batch=False):
    """The randomized inputs of the psroi tests: ROIs on a quarter-pixel grid + 1/8 (so that `round` never sees a tie) that reach outside
    the map on all four sides, some smaller than one feature pixel, both batch indices.  -> dict of float32 arrays."""
    rng = np.random.default_rng(seed)
    B, C, H, W = shape
    img_w, img_h = W / spatial_scale, H / spatial_scale
    inp = rng.standard_normal(shape).astype(np.float32)
    rois = np.zeros((n_rois, 5), dtype=np.float32)
    for i in range(n_rois):
        kind = i % 4
        if kind == 3:                                                                 # smaller than one feature pixel
            w, h = rng.uniform(0, 0.8 / spatial_scale, 2)
        else:
            w, h = rng.uniform(0.1, 0.7) * img_w, rng.uniform(0.1, 0.7) * img_h
        x = rng.uniform(-0.25 * img_w, 1.05 * img_w - w * 0.5)
        y = rng.uniform(-0.25 * img_h, 1.05 * img_h - h * 0.5)
        q = lambda v: np.floor(v * 4) / 4 + 0.125
        rois[i] = (i % B, q(x), q(y), q(x + w), q(y + h))
    trans = rng.standard_normal((n_rois, 2 * classes, part, part)).astype(np.float32)
    grad_out = rng.standard_normal((n_rois, C, pooled, pooled)).astype(np.float32)
    return {"input": inp, "rois": rois, "trans": trans, "grad_out": grad_out}


# The randomized cases of the shim and GPU tests: (input shape, ROIs, spatial scale, pooled, part, samples per part, classes, trans_std), each
# with the seed of `random_case` found once on the CPU so that every sample is at least MARGIN from a drop boundary, with and without offsets.
CASES = [
    ((2, 6, 20, 28), 12, 1.0 / 4, 3, 3, 4, 1, 0.1, 1),
    ((2, 6, 20, 28), 12, 1.0 / 4, 7, 7, 4, 2, 0.1, 1),
    ((2, 6, 20, 28), 12, 1.0 / 4, 6, 3, 2, 3, 0.3, 1),
    ((2, 16, 38, 50), 16, 1.0 / 16, 7, 7, 4, 1, 0.1, 1),
]
# grad_offset is discontinuous where a sample crosses an integer grid line, so it is compared on the first and third case with 4 ROIs only
# (576 and 1728 samples), seeded so that every unclamped coordinate of a kept sample is at least MARGIN from a grid line as well.
GOFF_CASES = [
    ((2, 6, 20, 28), 4, 1.0 / 4, 3, 3, 4, 1, 0.1, 101),
    ((2, 6, 20, 28), 4, 1.0 / 4, 6, 3, 2, 3, 0.3, 101),
]
# fp32 coordinate error: about 6 roundings at |coordinate| <= 64, 6 * 64 * 2^-24 = 2.3e-5; the margin is about 10x that.  Closer to a drop
# boundary (or grid line) a float kernel may legitimately keep (or pair) a sample differently from float64.
MARGIN = 2e-4
FACTOR = 4.0            # allowed error, in units of the fp32 reference's own error: a different but legal summation order, FMA contraction


def case_inputs(case):
    shape, n_rois, scale, pooled, part, S, classes, trans_std, seed = case
    d = random_case(seed, shape, n_rois, scale, pooled, part, S, classes, trans_std)
    d["args"] = (scale, shape[1], 1, pooled, part, S, trans_std)       # spatial_scale, output_dim, group_size, pooled, part, S, trans_std
    return d


def check_case_conditions(case, d, no_trans, need_grid):
    """The conditions on the inputs the comparisons rest on; asserted, never used to mask anything."""
    shape, n_rois, scale, pooled, part, S, classes, trans_std, _ = case
    m = margins(shape, d["rois"], d["trans"], no_trans, scale, shape[1], pooled, part, S, trans_std)
    assert m["boundary"] >= MARGIN, m
    assert not need_grid or m["grid"] >= MARGIN, m
    assert 0 < m["kept"] < m["samples"] and m["clamped"] > 0, m
    r, (H, W) = d["rois"], shape[2:]
    assert set(r[:, 0].astype(int)) == set(range(shape[0]))
    if n_rois >= 12:                                                  # outside the map on all four sides, some smaller than one feature pixel
        assert (r[:, 1] * scale < -0.5).any() and (r[:, 2] * scale < -0.5).any()
        assert (r[:, 3] * scale > W).any() and (r[:, 4] * scale > H).any()
        assert (((r[:, 3] - r[:, 1]) * scale < 1) & ((r[:, 4] - r[:, 2]) * scale < 1)).any()
    return m


def reference_pair(d, no_trans):
    """float64 reference and the fp32 reference's max abs error per tensor -> (ref dict, err dict)."""
    a = d["args"]
    trans = None if no_trans else d["trans"]
    ref, err = {}, {}
    out64, cnt64 = forward(d["input"], d["rois"], trans, no_trans, *a, dtype=np.float64)
    out32, cnt32 = forward(d["input"], d["rois"], trans, no_trans, *a, dtype=np.float32)
    assert np.array_equal(cnt64, cnt32.astype(np.float64))
    gi64, gt64 = backward(d["grad_out"], d["input"], d["rois"], trans, cnt64, no_trans, *a, dtype=np.float64)
    gi32, gt32 = backward(d["grad_out"], d["input"], d["rois"], trans, cnt64, no_trans, *a, dtype=np.float32)
    ref.update(output=out64, count=cnt64, grad_input=gi64, grad_offset=gt64)
    err.update(output=float(np.abs(out32 - out64).max()), grad_input=float(np.abs(gi32 - gi64).max()),
               grad_offset=None if no_trans else float(np.abs(gt32 - gt64).max()))
    return ref, err


def compare(name, got, ref, ref_err, what):
    """Print both errors, then assert the code under test within FACTOR x the fp32 reference's error (max abs over the tensor)."""
    e = float(np.abs(np.asarray(got, dtype=np.float64) - ref).max())
    print("%-34s %-12s fp32-reference error %.3e   measured error %.3e   (allowed %.3e)" % (what, name, ref_err, e, FACTOR * ref_err))
    assert e <= FACTOR * ref_err, (what, name, e, ref_err)
    return e
