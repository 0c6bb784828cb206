"""CPU tests of the float64 restatement of the box decode (tests/decode_ref.py) and of the structured inputs (tests/decode_cases.py).

1. Anchor: decode_ref against the reference's own PostProcessor rows (tests/golden/decode_structured.npz on the structured maps, every
   `output_depth`; tests/golden/decode_only.npz, every mode) and against oracle.decode_image image by image, on anchor maps of its own and on
   every pixel of the maps the device tests read.  Both sides of these
   comparisons differ by the float32 rounding of the reference alone.  Error per column = |a - b| / max(1, |b|).
   Measured worst per-column error of all these comparisons (= decode_ref.YARDSTICK), and the bound = 4x that:
     column   goldens + oracle on the anchor maps   oracle on the device cases' maps   yardstick (worst)   bound (4x)
     cls      0                                     0                                  0                   0
     alpha    3.82e-07                              4.45e-07                           4.45e-07            1.78e-06
     x1       1.76e-07                              9.54e-07                           9.54e-07            3.82e-06
     y1       1.72e-07                              4.77e-07                           4.77e-07            1.91e-06
     x2       4.77e-07                              9.54e-07                           9.54e-07            3.82e-06
     y2       2.98e-07                              4.77e-07                           4.77e-07            1.91e-06
     h        9.97e-08                              1.26e-07                           1.26e-07            5.04e-07
     w        1.13e-07                              1.49e-07                           1.49e-07            5.96e-07
     l        1.11e-07                              1.22e-07                           1.22e-07            4.88e-07
     X        2.91e-06                              2.15e-06                           2.91e-06            1.16e-05
     Y        1.11e-06                              1.26e-06                           1.26e-06            5.04e-06
     Z        2.76e-07                              2.97e-07                           2.97e-07            1.19e-06
     ry       5.55e-07                              6.90e-07                           6.90e-07            2.76e-06
     score    8.88e-08                              1.40e-07                           1.40e-07            5.60e-07
   (Anchor maps: 94 + 117 reference rows under 'soft', the 94 and 100 of them again under each other mode, 250 oracle rows per mode.
   Device cases' maps: all 960 pixels of every image of the nine cases, every mode.  The first column alone undersamples the box columns:
   x1 = (px - e) * 4 - pad carries 2^-20 = 9.54e-07 whenever (px - e) lies in [4, 8) and the pad cancels the result to below 1 -- the float32
   formula itself, which a few hundred rows met in x2 only.  Measured on the same maps the kernel reads, the reference shows it in x1 too.)
2. Census: every branch of the decode is taken AND missed by the stated share of the rows of every device case (conditions on the inputs,
   counted from decode_ref alone), and at most 2 % of a case's rows sit within 1e-5 of a discontinuous decision.
3. Sensitivity: seven wrong variants of the decode each miss the correct rows by at least 100x the device test's bound on the structured
   inputs.  On the inputs of decode_only.npz (seeded noise, B = 1) the same variants are measured and printed, not asserted:
     (worst column error / device bound of that column, 'soft'; decode_only over all 50 slots of its four maps)
     variant              structured b3_k50   decode_only.npz
     d3_from_d2_pairs          8.5e+05          1.1e+04   (one slot has a d2 pair below the clamp; no slot has a d3 pair below it)
     d2_one_pair               7.3e+05          9.2e+04
     calib_of_image0           7.3e+05                0   (B = 1)
     pad_of_image0             2.1e+06                0   (B = 1)
     clamp_per_image           6.6e+04                0   (B = 1)
     no_half_height            5.9e+05          7.7e+05
     dims_not_rolled           2.9e+07          1.9e+07
   Census of decode_only.npz (117 valid rows; printed by test_census_of_noise_maps): d1 / d2 / d3 below the 100 m clamp in 3 / 1 / 0 rows,
   no row with all five keypoint terms in 2-90 m, direct depth and sigma never at their lower clamps, sigma at 1 in 39 rows, the box clipped
   at the left / top / right / bottom in 2 / 1 / 0 / 0 rows.  The structured cases take each of these in 10-80 % of their rows.
"""
import os

import numpy as np
import pytest
import torch

from monoflex_amd import synthetic as S
from oracle import monoflex_ref as R
from tests import decode_cases as C
from tests import decode_ref as D


def _check(what, err):
    print("%-44s %s" % (what, D.format_errors(err)))
    bound = D.bounds()
    assert (err <= bound).all(), "%s: column(s) %s past 4x the yardstick: %s" % (
        what, [D.COLUMNS[i] for i in np.nonzero(err > bound)[0]], D.format_errors(err))


def _valid_rows(ref):
    assert ref["det"].shape[0] == 1
    return ref["det"][0][ref["valid"][0].astype(bool)]


def _err_rows(rows, ref, mode):
    """Reference rows (the valid ones, in order) against the restatement of one image."""
    keep = ref["valid"].astype(bool)
    full = ref["det"].copy()
    assert rows.shape == (int(keep.sum()), 14), (rows.shape, int(keep.sum()))
    full[keep] = rows
    return D.column_errors(full, ref, mode, rows=keep)


def _structured_golden(golden_dir):
    g = np.load(os.path.join(golden_dir, "decode_structured.npz"))
    images = tuple(int(i) for i in g["images"])
    maps = C.structured_maps(int(g["map_seed"]), images)
    scores, index = C.peak_lists(int(g["list_seed"]), len(images), int(g["K"]), [tuple(r) for r in g["score_ranges"]])
    return g, maps, scores, index


def _one_image(maps, scores, index, b, mode, threshold=C.THRESHOLD):
    return D.decode_boxes(maps["hmap"][b:b + 1], maps["reg_off"], scores[b:b + 1], index[b:b + 1], maps["calib"][b:b + 1], maps["pad"][b:b + 1],
                          maps["sizes"][b], threshold, mode)


@pytest.mark.parametrize("mode", D.MODES)
def test_ref_vs_reference_rows_on_structured_maps(golden_dir, mode):
    g, maps, scores, index = _structured_golden(golden_dir)
    worst, n_rows = np.zeros(14), 0
    for b in range(len(maps["images"])):
        ref = _one_image(maps, scores, index, b, mode)
        rows = g["img%d_result_soft" % b].copy()
        if mode != "soft":
            rows[:, 9:] = g["img%d_result_%s" % (b, mode)]
        assert 0 < rows.shape[0] < int(g["K"])
        worst = np.maximum(worst, _err_rows(rows, ref, mode))
        n_rows += rows.shape[0]
        assert D.near_rows(ref, mode).mean() <= D.NEAR_CAP
    assert n_rows >= 90
    _check("reference rows, structured, %s" % mode, worst)


def _decode_only_maps(g, n):
    gen = torch.Generator().manual_seed(int(g["case%d_seed" % n]))
    logits = torch.randn(1, 3, 96, 320, generator=gen) * 0.8 - 2.0 + float(g["case%d_shift" % n])
    cls = torch.sigmoid(logits).clamp(1e-4, 1 - 1e-4)
    reg = torch.randn(1, 50, 96, 320, generator=gen) * 0.7
    return cls, reg


def _decode_only_inputs(g, n):
    """The kernel's inputs for case n of decode_only.npz: the NHWC map and the per-class top-50 lists of the NMS-ed heat map."""
    cls, reg = _decode_only_maps(g, n)
    sc, ind = torch.topk(R.nms_hm(cls).view(1, 3, -1), 50)
    assert all(len(torch.unique(sc[0, c])) == 50 for c in range(3))
    tgt = S.synthetic_target(320, 96)
    hmap = np.ascontiguousarray(reg[0].permute(1, 2, 0).numpy())[None]
    return dict(hmap=hmap, reg_off=0, scores=sc.numpy(), index=ind.numpy().astype(np.int32), calib=R.Calib(tgt["P"]).as_f32()[None],
                pad=tgt["pad_size"].numpy()[None].astype(np.int32), img_size=np.array(tgt["size"]), sizes=np.array([tgt["size"]]),
                threshold=0.2), cls, reg, tgt


@pytest.mark.parametrize("mode", D.MODES)
def test_ref_vs_reference_rows_on_noise_maps(golden_dir, mode):
    g = np.load(os.path.join(golden_dir, "decode_only.npz"))
    worst = np.zeros(14)
    for n in ((0, 1, 2, 3) if mode == "soft" else (0, 1)):
        d = _decode_only_inputs(g, n)[0]
        ref = C.run_ref(d, mode)
        rows = g["case%d_result" % n if mode == "soft" else "case%d_result_%s" % (n, mode)]
        worst = np.maximum(worst, _err_rows(rows, ref, mode))
    _check("reference rows, decode_only, %s" % mode, worst)


@pytest.mark.parametrize("mode", D.MODES)
def test_ref_vs_oracle_decode_image(golden_dir, mode):
    """Image by image, every slot (threshold 0): the structured maps with isolated class peaks, and the first noise map."""
    worst = np.zeros(14)
    maps = C.structured_maps(31, (0, 1, 2, 3))
    scores, index = C.peak_lists(32, 4, 50)
    for b, i in enumerate(maps["images"]):
        cls = torch.from_numpy(C.peak_heat(scores, index, b))[None]
        reg = torch.from_numpy(maps["hmap"][b, :, :, maps["reg_off"]:maps["reg_off"] + 50]).permute(2, 0, 1)[None].contiguous()
        dec = R.decode_image(cls, reg, R.Calib(C.image_P(i)), C.IMAGES[i]["pad"], C.IMAGES[i]["size"], threshold=0.0, K=50, output_depth=mode)
        ref = _one_image(maps, scores, index, b, mode, threshold=0.0)
        assert np.array_equal(dec["indexs"].numpy(), ref["topk"][0, :, 1]) and np.array_equal(dec["clses"].numpy(), ref["topk"][0, :, 2])
        worst = np.maximum(worst, _err_rows(dec["result"].numpy(), ref, mode))
    g = np.load(os.path.join(golden_dir, "decode_only.npz"))
    d, cls, reg, tgt = _decode_only_inputs(g, 0)
    dec = R.decode_image(cls, reg, R.Calib(tgt["P"]), tgt["pad_size"], tgt["size"], threshold=0.0, output_depth=mode)
    worst = np.maximum(worst, _err_rows(dec["result"].numpy(), C.run_ref(dict(d, threshold=0.0), mode), mode))
    _check("oracle.decode_image, %s" % mode, worst)


@pytest.mark.parametrize("name", list(C.CASES))
def test_ref_vs_oracle_decode_image_on_the_device_maps(name):
    """The float32 reference arithmetic on the very head maps the device tests read: every pixel of every image of the case decoded by
    oracle.decode_image (four lattices of isolated peaks, 240 rows each, threshold 0, image 0's size as the clamp), every mode."""
    c = C.CASES[name]
    maps = C.structured_maps(c["seed"], c["images"], c["ld"], c["reg_off"])
    worst = np.zeros(14)
    for b, i in enumerate(maps["images"]):
        reg = torch.from_numpy(maps["hmap"][b, :, :, maps["reg_off"]:maps["reg_off"] + 50]).permute(2, 0, 1)[None].contiguous()
        for parity in range(4):
            scores, index = C.lattice_lists(c["seed"] + 10 * b + parity, parity)
            K = scores.shape[2]
            cls = torch.from_numpy(C.peak_heat(scores, index, 0))[None]
            for mode in D.MODES:
                dec = R.decode_image(cls, reg, R.Calib(C.image_P(i)), C.IMAGES[i]["pad"], tuple(maps["img_size"]), threshold=0.0, K=3 * K,
                                     output_depth=mode)
                ref = D.decode_boxes(maps["hmap"][b:b + 1], maps["reg_off"], scores, index, maps["calib"][b:b + 1], maps["pad"][b:b + 1],
                                     maps["img_size"], 0.0, mode)
                # (the oracle's lists are 3 K long and end in padding; the peaks come first, in the same order)
                rows = dec["result"].numpy()[:K]
                assert np.array_equal(dec["indexs"].numpy()[:K], ref["topk"][0, :, 1]) and np.array_equal(rows[:, 0], ref["det"][0, :, 0])
                worst = np.maximum(worst, _err_rows(rows, ref, mode))
    _check("oracle.decode_image on the maps of %s" % name, worst)



def test_stage2_merge_order():
    """Value descending, position ascending: equal scores across classes go to the lower position of the (3 K) list."""
    s = np.array([[0.9, 0.5, 0.5], [0.9, 0.9, 0.1], [0.5, 0.2, 0.2]], dtype=np.float32)
    assert list(D.stage2_merge(s)) == [0, 3, 4]
    s, _ = C.score_lists(5, 2, 8, "ties")
    for b in range(2):
        flat = s[b].reshape(-1)
        want = sorted(range(flat.size), key=lambda p: (-float(flat[p]), p))[:8]
        assert list(D.stage2_merge(s[b])) == want
        assert (flat[want[:6]] == C.SCORE_CLAMP).all() and [p // 8 for p in want[:6]] == [0, 0, 1, 1, 2, 2]


@pytest.mark.parametrize("name", list(C.CASES))
def test_census_of_device_cases(name):
    """The inputs of the device tests reach every branch: shares counted from the float64 restatement alone."""
    rows = len(C.CASES[name]["images"]) * C.CASES[name]["K"]
    for kind in C.LIST_KINDS:
        d = C.case_inputs(name, kind)
        for mode in D.MODES:
            ref = C.run_ref(d, mode)
            near = float(D.near_rows(ref, mode).mean())
            wrap_near = float(((ref["alpha_wrap_dist"] < D.NEAR_MARGIN) | (ref["ry_wrap_dist"] < D.NEAR_MARGIN)).mean())
            assert near <= D.NEAR_CAP and wrap_near <= D.NEAR_CAP, (name, kind, mode, near, wrap_near)
            assert np.isfinite(ref["det"]).all()
            if rows < C.CENSUS_MIN_ROWS:
                continue
            cen = C.census(ref, mode)
            if kind == "distinct" and mode in ("soft", "hard"):
                print("census %s %s (%d rows)\n%s" % (name, mode, rows, C.format_census(cen)))
            for k, (share, taken, missed) in cen.items():
                assert share >= taken and 1 - share >= missed, (name, kind, mode, k, share)
    if name == "b3_k50":
        d = C.case_inputs(name, "threshold")
        v = C.run_ref(d, "soft")
        thr = np.float32(C.THRESHOLD)
        sc = v["topk"][..., 0]
        for val, want in ((thr, 1), (np.nextafter(thr, np.float32(0)), 0), (np.nextafter(thr, np.float32(1)), 1)):
            assert (sc == float(val)).sum() >= 2 and (v["valid"][sc == float(val)] == want).all()
        d = C.case_inputs(name, "shared_pixel")
        v = C.run_ref(d, "soft")
        assert all(np.unique(v["topk"][b, :, 1]).size < 50 for b in range(3))       # one pixel in two rows, with two classes


def test_census_of_noise_maps(golden_dir):
    """The same census on the inputs of decode_only.npz, printed: what the suite's decode tests exercised before the structured cases."""
    g = np.load(os.path.join(golden_dir, "decode_only.npz"))
    total, keys = None, None
    n_valid = 0
    for n in range(4):
        d = _decode_only_inputs(g, n)[0]
        ref = C.run_ref(d, "soft")
        keep = ref["valid"].astype(bool)
        n_valid += int(keep.sum())
        cen = C.census({k: (v[keep][None] if v.shape[:2] == keep.shape else v) for k, v in ref.items()}, "soft") if keep.any() else None
        if cen is not None:
            cnt = np.array([v[0] * keep.sum() for v in cen.values()])
            total, keys = (cnt if total is None else total + cnt), list(cen)
    print("census of decode_only.npz, %d valid rows (count of rows per branch)" % n_valid)
    for k, c in zip(keys, total):
        print("  %-48s %4d" % (k, round(c)))
    assert n_valid == 117
    assert total[keys.index("d3 below the 100 m clamp")] == 0                    # the gap the structured cases close


def _sensitivity(d, mode="soft"):
    good = C.run_ref(d, mode)
    out = {}
    bound = D.bounds()
    for w in D.WRONG:
        err = D.column_errors(C.run_ref(d, mode, wrong=w)["det"], good, mode)
        with np.errstate(divide="ignore", invalid="ignore"):
            ratio = np.where(bound > 0, err / bound, np.where(err > 0, np.inf, 0.0))
        out[w] = float(ratio.max())
    return out


def test_wrong_variants_are_caught_on_structured_inputs(golden_dir):
    """Each wrong variant misses the correct rows by >= 100x the device bound on the structured inputs (asserted); on the noise maps of
    decode_only.npz the same figure is printed (recorded in the module docstring): below 100 there means the old inputs could not tell."""
    s = _sensitivity(C.case_inputs("b3_k50"))
    g = np.load(os.path.join(golden_dir, "decode_only.npz"))
    old = {w: 0.0 for w in D.WRONG}
    for n in range(4):
        d = _decode_only_inputs(g, n)[0]
        valid = C.run_ref(d, "soft")["valid"].astype(bool)[0]
        if not valid.any():
            continue
        dv = dict(d, scores=d["scores"])                                         # (all 50 slots: more than the goldens' valid rows see)
        for w, r in _sensitivity(dv).items():
            old[w] = max(old[w], r)
    print("variant              structured b3_k50   decode_only.npz   (worst column error / device bound of that column)")
    for w in D.WRONG:
        print("%-20s %12.3g %17.3g" % (w, s[w], old[w]))
    for w in D.WRONG:
        assert s[w] >= 100, (w, s[w])
    for name in ("b3_permuted", "k256", "ld72"):
        s2 = _sensitivity(C.case_inputs(name), "hard")
        assert all(v >= 100 for v in s2.values()), (name, s2)
