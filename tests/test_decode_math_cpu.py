"""The box decode's arithmetic without a GPU: monoflex_amd/csrc/box_decode_math.h (what decode.hip's decode_boxes_kernel runs per row)
compiled for the host (tests/shim/decode_row_host.cpp, g++ -ffp-contract=off) on the inputs of the device tests, against the float64
restatements and the reference's recorded rows, at the device tests' own bounds: decode_ref.bounds() / decode_cfg_ref.bounds(setting) =
4x the float32 reference's error per column, `topk` and `valid` EQUAL, `unc` within the score column's bound, near-decision rows left out
per column by decode_ref.column_errors and at most NEAR_CAP of a case.  No tolerance is defined here."""
import os

import numpy as np
import pytest

from monoflex_amd import lib as L
from tests import decode_cases as C
from tests import decode_cfg_ref as DC
from tests import decode_ref as D
from tests import decode_shim
from tests import head_sets_cases as HC
from tests import head_sets_ref as HS


@pytest.fixture(scope="module")
def shim(tmp_path_factory):
    return decode_shim.build(tmp_path_factory.mktemp("shim"))


def lib_cfg(s, mode):
    """lib.DecodeCfg of a decode_cfg_ref setting, built the way PostProcessor builds its own (lib.decode_cfg)."""
    head = dict(depth_mode=s["depth_mode"], depth_range=tuple(s["depth_range"]), depth_ref=tuple(s["depth_ref"]), dim_mean=s["dim_mean"],
                dim_std=s["dim_std"], dim_modes=["exp" if s["dim_exp"] else "linear", True, bool(s["dim_use_std"])], down_ratio=4, eps=1e-3)
    return L.decode_cfg(head, s["uncertainty_as_conf"], mode)


def full_layout():
    return L.HeadSet(HS.SETS["s111"], HS.channels("s111")).layout()


def compare(what, got, ref, mode, bound, reports_unc, rows=None):
    """The comparison of tests/test_gpu_decode_cfg.py `_compare`, on the rows selected by `rows` (default: all)."""
    det, topk, valid, unc = got
    assert np.isfinite(det).all() and np.isfinite(unc).all(), what
    assert np.array_equal(topk.astype(np.float64), ref["topk"]), what + ": topk differs from the restatement"
    assert np.array_equal(valid, ref["valid"]), what + ": valid differs from the restatement"
    assert float(D.near_rows(ref, mode).mean()) <= D.NEAR_CAP, what
    err = D.column_errors(det, ref, mode, rows=rows)
    print("%-44s %s" % (what, D.format_errors(err)))
    assert (err <= bound).all(), "%s: column(s) %s past 4x the float32 reference's error: %s" % (
        what, [D.COLUMNS[i] for i in np.nonzero(err > bound)[0]], D.format_errors(err))
    if reports_unc is None:                     # (a recording without uncertainties: the columns alone)
        return
    if reports_unc:
        keep = np.ones(valid.shape, dtype=bool) if rows is None else rows
        uerr = DC.unc_errors(unc[keep], dict(unc=ref["unc"][keep]))
        assert (uerr <= bound[13]).all(), "%s: unc [sigma, conf] errors %s past the score column's bound %.2e" % (what, uerr, bound[13])
    else:
        assert (unc == 0).all() and np.array_equal(det[..., 13], topk[..., 0]), what + ": no uncertainty is reported, the score is raw"


# ---- against the float64 restatements ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", list(C.CASES))
def test_every_case_and_mode_under_the_yaml_settings(shim, name):
    for kind in (C.LIST_KINDS if name == "b3_k50" else ("distinct",)):           # ties, a shared pixel and scores around the threshold: stage 2
        d = C.case_inputs(name, kind)
        for mode in D.MODES:
            ref = dict(C.run_ref(d, mode), unc=DC.run_ref(d, mode, DC.YAML)["unc"])
            compare("%s %s %s" % (name, kind, mode), shim(d, lib_cfg(DC.YAML, mode), full_layout()), ref, mode, D.bounds(), True)


@pytest.mark.parametrize("setting", list(DC.SETTINGS))
def test_every_setting_on_the_device_cases(shim, setting):
    s = DC.SETTINGS[setting]
    for name in DC.DEVICE_CASES:
        d = DC.case_inputs(name, setting)
        for mode in DC.GOLDEN_MODES:
            compare("%s %s %s" % (setting, name, mode), shim(d, lib_cfg(s, mode), full_layout()), DC.run_ref(d, mode, setting), mode,
                    DC.bounds(setting), s["uncertainty_as_conf"])


def head_set_inputs(name):
    """Case b3_k50 with its 50 channels sliced and permuted into the set's layout inside the 64-wide row (tests/test_gpu_head_sets.py)."""
    d = C.case_inputs("b3_k50")
    return dict(d, hmap=HS.take(d["hmap"][..., d["reg_off"]:d["reg_off"] + 50], name, 3, ld=d["hmap"].shape[3], off=d["reg_off"], junk=d["hmap"]))


@pytest.mark.parametrize("name", list(HS.SETS))
def test_every_head_set_under_the_yaml_settings(shim, name):
    d = head_set_inputs(name)
    heads = L.HeadSet(HS.SETS[name], HS.channels(name)).layout()
    for mode in HS.output_depths(name):
        for uac in (True, False):
            ref = HS.decode_ref(name, d["hmap"], d["reg_off"], d["scores"], d["index"], d["calib"], d["pad"], d["img_size"], d["threshold"], mode,
                                HC.settings(uncertainty_as_conf=uac))
            got = shim(d, lib_cfg(dict(DC.YAML, uncertainty_as_conf=uac), mode), heads)
            compare("%s %s uac=%d" % (name, mode, uac), got, ref, mode, DC.bounds("yaml"), uac and HS.has_depth_error(name, mode))
            if uac and HS.has_depth_error(name, mode):
                assert (got[3][..., 0] > 0).all()


# ---- against the reference's recorded rows -----------------------------------------------------------------------------------------------------
def golden_case(golden_dir, file):
    g = np.load(os.path.join(golden_dir, file))
    images = tuple(int(i) for i in g["images"])
    maps = C.structured_maps(int(g["map_seed"]), images)
    scores, index = C.peak_lists(int(g["list_seed"]), len(images), int(g["K"]), [tuple(r) for r in g["score_ranges"]])
    return g, maps, scores, index


def one_image(maps, scores, index, b, ncls=3):
    return dict(hmap=maps["hmap"][b:b + 1], reg_off=maps["reg_off"], scores=scores[b:b + 1, :ncls], index=index[b:b + 1, :ncls],
                calib=maps["calib"][b:b + 1], pad=maps["pad"][b:b + 1], img_size=maps["sizes"][b], threshold=C.THRESHOLD)


def against_rows(what, got, ref, rows, mode, bound, reports_unc, unc_rows=None):
    """The shim's valid rows against the reference's recorded ones (the restatement supplies the decision margins only)."""
    keep = ref["valid"].astype(bool)
    assert np.array_equal(got[2], ref["valid"]) and rows.shape == (int(keep.sum()), 14), what
    want = ref["det"].copy()
    want[keep] = rows
    gold = dict(ref, det=want)
    if unc_rows is not None:
        gold["unc"] = ref["unc"].copy()
        gold["unc"][keep] = unc_rows
    compare(what, got, gold, mode, bound, reports_unc, rows=keep)


@pytest.mark.parametrize("mode", D.MODES)
def test_reference_rows_on_structured_maps(shim, golden_dir, mode):
    g, maps, scores, index = golden_case(golden_dir, "decode_structured.npz")
    for b in range(len(maps["images"])):
        d = one_image(maps, scores, index, b)
        rows = g["img%d_result_soft" % b].copy()
        if mode != "soft":
            rows[:, 9:] = g["img%d_result_%s" % (b, mode)]
        against_rows("structured img%d %s" % (b, mode), shim(d, lib_cfg(DC.YAML, mode), full_layout()), DC.run_ref(d, mode, DC.YAML), rows, mode, D.bounds(),
                     None)


@pytest.mark.parametrize("setting", list(DC.SETTINGS))
def test_reference_rows_under_other_settings(shim, golden_dir, setting):
    g, maps, scores, index = golden_case(golden_dir, "decode_cfg.npz")
    s = DC.SETTINGS[setting]
    for mode in DC.GOLDEN_MODES:
        for b in range(len(maps["images"])):
            d = one_image(maps, scores, index, b, s["ncls"])
            key = "%s_%s_img%d" % (setting, mode, b)
            unc_rows = np.stack((g[key + "_estimated_depth_error"], g[key + "_uncertainty_conf"]), axis=1) if s["uncertainty_as_conf"] else None
            against_rows(key, shim(d, lib_cfg(s, mode), full_layout()), DC.run_ref(d, mode, setting), g[key + "_result"], mode, DC.bounds(setting),
                         s["uncertainty_as_conf"], unc_rows)


# ---- the inputs tell a broken header from a right one ------------------------------------------------------------------------------------------
def ratio(det, ref, mode, bound):
    err = D.column_errors(det, ref, mode)
    with np.errstate(divide="ignore", invalid="ignore"):
        return float(np.where(bound > 0, err / bound, np.where(err > 0, np.inf, 0.0)).max())


def test_wrong_variants_are_told_from_the_shim(shim):
    """Each wrong rule of decode_ref.WRONG / decode_cfg_ref.WRONG misses the SHIM's rows by >= 100x the bound where
    tests/test_decode_ref_cpu.py / tests/test_decode_cfg_ref_cpu.py show it missing the restatement's, and stays within the bound where the
    rule it breaks is not in use."""
    for name, mode in (("b3_k50", "soft"), ("b3_permuted", "hard"), ("k256", "hard"), ("ld72", "hard")):
        d = C.case_inputs(name)
        det = shim(d, lib_cfg(DC.YAML, mode), full_layout())[0]
        for w in D.WRONG:
            r = ratio(det, C.run_ref(d, mode, wrong=w), mode, D.bounds())
            assert r >= 100, (name, mode, w, r)
    ST = DC.SETTINGS
    expect = {"std_ignored": [s for s in ST if ST[s]["dim_use_std"]], "mean_of_class0": [s for s in ST if ST[s]["ncls"] > 1],
              "depth_ref_swapped": [s for s in ST if ST[s]["depth_mode"] == "linear"], "no_depth_clamp_direct": list(ST),
              "conf_always_applied": [s for s in ST if not ST[s]["uncertainty_as_conf"]], "exp_dims_when_linear": [s for s in ST if not ST[s]["dim_exp"]]}
    assert set(expect) == set(DC.WRONG)
    for setting in ST:
        mode = "direct" if setting in ("b_linear_depth", "e_car") else "soft"
        d = DC.case_inputs("b3_k50", setting)
        det = shim(d, lib_cfg(ST[setting], mode), full_layout())[0]
        for w in DC.WRONG:
            r = ratio(det, DC.run_ref(d, mode, setting, wrong=w), mode, DC.bounds(setting))
            assert (r >= 100) if setting in expect[w] else (r <= 1), (setting, w, r)


# ---- refusals: the matrix of mfx_decode_boxes_heads, same messages ------------------------------------------------------------------------------
def test_refusals(shim):
    d = DC.case_inputs("k7", "a_defaults")
    s = DC.SETTINGS["a_defaults"]

    def cfg(**kw):
        c = lib_cfg(s, "soft")
        for k, v in kw.items():
            if isinstance(v, tuple):
                getattr(c, k)[0], getattr(c, k)[1] = v
            else:
                setattr(c, k, v)
        return c
    for c, edit, msg in ((None, {}, "null cfg"), (cfg(depth_decode=3), {}, "depth_decode"), (cfg(depth_decode=-1), {}, "depth_decode"),
                         (cfg(output_depth=8), {}, "output_depth"), (cfg(output_depth=-1), {}, "output_depth"),
                         (cfg(depth_range=(2.0, 1.0)), {}, "depth_range"), (cfg(depth_range=(0.1, float("inf"))), {}, "depth_range"),
                         (cfg(depth_range=(float("nan"), 100.0)), {}, "depth_range"), (cfg(), dict(ncls=4), "ncls"), (cfg(), dict(ncls=0), "ncls"),
                         (cfg(), dict(K=257), "K <= 256")):
        with pytest.raises(ValueError, match=msg):
            shim(d, c, full_layout(), **edit)
    with pytest.raises(ValueError, match="null heads"):
        shim(d, cfg(), None)
    shim(d, cfg(), full_layout())

    d = head_set_inputs("s000")

    def call(name, mode, ld=None, reg_off=None, **edit):
        lay = L.HeadSet(HS.SETS[name], HS.channels(name)).layout()
        for k, v in edit.items():
            if k.startswith("ch"):
                lay.ch[int(k[2:])] = v
            else:
                setattr(lay, k, v)
        geom = {k: v for k, v in (("ld", ld), ("reg_off", reg_off)) if v is not None}
        return shim(d, lib_cfg(DC.YAML, mode), lay, **geom)
    for name in HS.SETS:                                                  # every output_depth a set cannot serve
        for mode in HS.OUTPUT_DEPTHS:
            if mode not in HS.output_depths(name):
                with pytest.raises(ValueError, match="output_depth %s needs" % ("keypoints_\\*" if mode.startswith("keypoints") else "soft / hard / mean")):
                    call(name, mode)
    for edit, msg in ((dict(ch7=-1), "required regression key is absent"), (dict(ch4=-1), "required regression key is absent"),
                      (dict(ch8=-2), "required regression key is absent"),                                   # only -1 marks an absent key
                      (dict(ch7=26), "reach past reg_width"), (dict(ch5=19), "reach past reg_width"),         # ch >= R; a key reaching past R
                      (dict(ld=33), "inside a row"), (dict(reg_off=39), "inside a row"),                      # reg_off + R > ld
                      (dict(reg_width=51), "reg_width must be 1..50"), (dict(reg_width=0), "reg_width must be 1..50")):
        with pytest.raises(ValueError, match=msg):
            call("s000", "direct", **edit)
    with pytest.raises(ValueError, match="corner_uncertainty without corner_offset"):
        call("s011", "direct", ch2=-1)
    assert np.isfinite(call("s000", "direct")[0]).all()
