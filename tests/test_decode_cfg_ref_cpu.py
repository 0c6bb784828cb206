"""CPU tests of the float64 restatement of the configurable box decode (tests/decode_cfg_ref.py, mfx_decode_boxes_cfg).

1. Under the runs/monoflex.yaml settings it EQUALS tests/decode_ref.py (det, topk, valid and every margin) on all the existing cases, every
   `output_depth`.
2. It reproduces the rows of the reference's own PostProcessor recorded under the seven settings of decode_cfg_ref.SETTINGS
   (tests/golden/decode_cfg.npz, tools/gen_decode_cfg_golden.py) -- including `estimated_depth_error` / `uncertainty_conf` where the
   reference reports them -- within 4x the yardstick.
3. Yardstick: per setting and column, the worst |a - b| / max(1, |b|) of the float32 reference arithmetic against the restatement: the
   recorded rows of 2., and decode_rows_f32 (float32 torch, the reference's operation order) on EVERY pixel of every map the device cases
   read, under soft / hard / direct.  Printed, and asserted to stay below 4x decode_cfg_ref.YARDSTICK, which holds these figures.
4. Census: the inputs reach every branch the settings add (shares counted from the restatement alone).
5. Near rows (an arg-max margin or an angle's distance from +-pi below NEAR_MARGIN) stay within NEAR_CAP of every case.
6. Sensitivity: each `wrong=` variant misses the correct rows by >= 100x the device bound under at least one setting.
"""
import os

import numpy as np
import pytest

from tests import decode_cases as C
from tests import decode_cfg_ref as DC
from tests import decode_ref as D

SETTINGS = list(DC.SETTINGS)


@pytest.mark.parametrize("name", list(C.CASES))
def test_equals_decode_ref_on_the_yaml_settings(name):
    kinds = C.LIST_KINDS if name in ("b3_k50", "k7", "k256") else ("distinct",)
    for kind in kinds:
        d = C.case_inputs(name, kind)
        for mode in D.MODES:
            old = C.run_ref(d, mode)
            new = DC.run_ref(d, mode, DC.YAML)
            for k, v in old.items():
                assert np.array_equal(new[k], v), (name, kind, mode, k)
            sigma = new["sigma"]
            assert np.array_equal(new["unc"][..., 0], sigma) and np.array_equal(new["unc"][..., 1], 1 - np.clip(sigma, 0.01, 1))


def _golden(golden_dir):
    g = np.load(os.path.join(golden_dir, "decode_cfg.npz"))
    images = tuple(int(i) for i in g["images"])
    maps = C.structured_maps(int(g["map_seed"]), images)
    scores, index = C.peak_lists(int(g["list_seed"]), len(images), int(g["K"]), [tuple(r) for r in g["score_ranges"]])
    return g, maps, scores, index


def _golden_errors(golden_dir, setting):
    """Worst per-column error of the recorded reference rows against the restatement -> (err (14,), unc err (2,), rows)."""
    g, maps, scores, index = _golden(golden_dir)
    s = DC.SETTINGS[setting]
    worst, worst_unc, n_rows = np.zeros(14), np.zeros(2), 0
    for mode in DC.GOLDEN_MODES:
        for b in range(len(maps["images"])):
            ref = DC.decode_boxes(maps["hmap"][b:b + 1], maps["reg_off"], scores[b:b + 1, :s["ncls"]], index[b:b + 1, :s["ncls"]], maps["calib"][b:b + 1],
                                  maps["pad"][b:b + 1], maps["sizes"][b], C.THRESHOLD, mode, s)
            key = "%s_%s_img%d" % (setting, mode, b)
            rows = g[key + "_result"]
            keep = ref["valid"].astype(bool)
            assert rows.shape == (int(keep.sum()), 14) and 0 < rows.shape[0] < int(g["K"]), (key, rows.shape, int(keep.sum()))
            full = ref["det"].copy()
            full[keep] = rows
            worst = np.maximum(worst, D.column_errors(full, ref, mode, rows=keep))
            assert D.near_rows(ref, mode).mean() <= D.NEAR_CAP
            if s["uncertainty_as_conf"]:
                got = np.stack((g[key + "_estimated_depth_error"], g[key + "_uncertainty_conf"]), axis=1)
                want = ref["unc"][keep]
                worst_unc = np.maximum(worst_unc, (np.abs(got - want) / np.maximum(1, np.abs(want))).max(axis=0))
                assert np.array_equal(rows[:, 13].astype(np.float32), (ref["topk"][keep][:, 0].astype(np.float32) * g[key + "_uncertainty_conf"]))
            else:
                assert (key + "_uncertainty_conf") not in g.files and (ref["unc"] == 0).all()
                assert np.array_equal(rows[:, 13], ref["topk"][keep][:, 0])                  # the raw score
            n_rows += rows.shape[0]
    return worst, worst_unc, n_rows


def _class_lists(rng, ncls, c):
    """Lists (1, ncls, K) over a random partition of all pixels, class c's scores above all others: the merged top K is class c's K pixels."""
    K = C.H * C.W // ncls
    index = rng.permutation(C.H * C.W)[:ncls * K].reshape(1, ncls, K).astype(np.int32)
    scores = np.zeros((1, ncls, K), dtype=np.float32)
    for k in range(ncls):
        lo, hi = (0.5, 0.98) if k == c else (0.02, 0.4)
        scores[0, k] = -np.sort(-C._distinct_scores(rng, K, lo, hi))
    return scores, index


def _pixel_errors(setting):
    """decode_rows_f32 against the restatement on every pixel of every image of the device cases' maps, soft / hard / direct."""
    s = DC.SETTINGS[setting]
    worst, worst_unc, n_rows = np.zeros(14), np.zeros(2), 0
    for name in DC.DEVICE_CASES:
        c = C.CASES[name]
        maps = C.structured_maps(c["seed"], c["images"], c["ld"], c["reg_off"])
        rng = np.random.default_rng(c["seed"] + 500)
        for b in range(len(c["images"])):
            for k in range(s["ncls"]):
                scores, index = _class_lists(rng, s["ncls"], k)
                args = (maps["hmap"][b:b + 1], maps["reg_off"], scores, index, maps["calib"][b:b + 1], maps["pad"][b:b + 1], maps["img_size"])
                for mode in DC.GOLDEN_MODES:
                    ref = DC.decode_boxes(*args, 0.0, mode, s)
                    assert (ref["det"][0, :, 0] == k).all() and np.array_equal(np.sort(ref["topk"][0, :, 1]), np.sort(index[0, k]))
                    det, unc = DC.decode_rows_f32(*args, mode, s)
                    worst = np.maximum(worst, D.column_errors(det, ref, mode))
                    worst_unc = np.maximum(worst_unc, DC.unc_errors(unc, ref))
                    n_rows += det.shape[1]
    return worst, worst_unc, n_rows


@pytest.mark.parametrize("setting", SETTINGS)
def test_yardstick_and_reference_rows(golden_dir, setting):
    """The two float32 evaluations against the restatement; their worst is the yardstick (decode_cfg_ref.YARDSTICK holds the figures of the
    first measurement), re-measured here and held below 4x itself -- which is also the check that the restatement reproduces the recorded
    reference rows."""
    g_err, g_unc, g_rows = _golden_errors(golden_dir, setting)
    p_err, p_unc, p_rows = _pixel_errors(setting)
    print("%s: reference rows (%d)   %s" % (setting, g_rows, D.format_errors(g_err)))
    print("%s: float32 torch (%d)    %s" % (setting, p_rows, D.format_errors(p_err)))
    print("%s: yardstick = worst     (%s)" % (setting, ", ".join("%.2e" % v for v in np.maximum(g_err, p_err))))
    print("%s: unc [sigma, conf]     reference rows %.2e %.2e   float32 torch %.2e %.2e" % (setting, g_unc[0], g_unc[1], p_unc[0], p_unc[1]))
    assert g_rows >= 30 and p_rows == 3 * len(DC.DEVICE_CASES) * 3 * (C.H * C.W // DC.SETTINGS[setting]["ncls"]) * DC.SETTINGS[setting]["ncls"]
    bound = DC.bounds(setting)
    for what, err in (("reference rows", g_err), ("float32 torch", p_err)):
        assert (err <= bound).all(), "%s, %s: column(s) %s past 4x the yardstick: %s" % (
            setting, what, [D.COLUMNS[i] for i in np.nonzero(err > bound)[0]], D.format_errors(err))


@pytest.mark.parametrize("setting", SETTINGS)
def test_census_and_near_rows_of_the_device_cases(setting):
    s = DC.SETTINGS[setting]
    for name in DC.DEVICE_CASES:
        rows = len(C.CASES[name]["images"]) * C.CASES[name]["K"]
        d = DC.case_inputs(name, setting)
        for mode in DC.GOLDEN_MODES:
            ref = DC.run_ref(d, mode, setting)
            near = float(D.near_rows(ref, mode).mean())
            wrap_near = float(((ref["alpha_wrap_dist"] < D.NEAR_MARGIN) | (ref["ry_wrap_dist"] < D.NEAR_MARGIN)).mean())
            assert near <= D.NEAR_CAP and wrap_near <= D.NEAR_CAP, (setting, name, mode, near, wrap_near)
            assert np.isfinite(ref["det"]).all() and np.isfinite(ref["unc"]).all()
            assert (ref["det"][..., 0] < s["ncls"]).all()
            if rows < C.CENSUS_MIN_ROWS:
                continue
            cen = DC.census(ref, s)
            if name == "b3_k50":
                print("census %s %s %s (%d rows)\n%s" % (setting, name, mode, rows, "\n".join("  %-58s %5.1f %%" % (k, 100 * v) for k, v in cen.items())))
            # the direct depth reaches both ends of the range and its inside, whatever the depth rule (exp, linear, inv_sigmoid)
            for k in ("direct depth below the range", "direct depth above the range", "direct depth inside the range"):
                assert cen[k] >= 0.05, (setting, name, mode, k, cen[k])
            assert cen["a keypoint span with relu(dy) == 0"] >= 0.10
            for k in ("sigma below 0.01", "sigma inside [0.01, 1]", "sigma above 1"):
                assert cen[k] >= 0.10, (setting, name, mode, k, cen[k])
            if not s["dim_exp"] and not s["dim_use_std"]:
                # a linear dimension off * mean turns negative with its offset; a negative height drives all three keypoint depths to the
                # lower clamp
                assert cen["a decoded dimension negative"] >= 0.10, (setting, name, mode, cen)
                assert cen["height negative: all keypoint depths at the lower clamp"] >= 0.05, (setting, name, mode, cen)
                assert cen["height negative, a keypoint depth NOT at the lower clamp"] == 0
            if s["dim_exp"] and not s["dim_use_std"]:
                assert cen["a decoded dimension negative"] == 0


def _sensitivity(setting, name="b3_k50", mode="soft"):
    d = DC.case_inputs(name, setting)
    good = DC.run_ref(d, mode, setting)
    bound = DC.bounds(setting)
    out = {}
    for w in DC.WRONG:
        bad = DC.run_ref(d, mode, setting, wrong=w)
        err = D.column_errors(bad["det"], good, mode)
        with np.errstate(divide="ignore", invalid="ignore"):
            ratio = np.where(bound > 0, err / bound, np.where(err > 0, np.inf, 0.0))
        out[w] = (float(ratio.max()), float(np.abs(bad["unc"] - good["unc"]).max()))
    return out


def test_wrong_variants_are_caught():
    """Each wrong rule changes the rows of at least one setting by >= 100x the device bound (worst column error / bound of that column), and
    only the settings whose rule it breaks: inputs that cannot tell a wrong rule from the right one prove nothing."""
    table = {s: _sensitivity(s, mode="direct" if s in ("b_linear_depth", "e_car") else "soft") for s in SETTINGS}
    print("%-24s" % "variant" + "".join("%16s" % s for s in SETTINGS))
    for w in DC.WRONG:
        print("%-24s" % w + "".join("%16.3g" % table[s][w][0] for s in SETTINGS))
    for w in DC.WRONG:
        assert max(table[s][w][0] for s in SETTINGS) >= 100, (w, [table[s][w] for s in SETTINGS])
    expect = {"std_ignored": [s for s in SETTINGS if DC.SETTINGS[s]["dim_use_std"]],
              "mean_of_class0": [s for s in SETTINGS if DC.SETTINGS[s]["ncls"] > 1],
              "depth_ref_swapped": [s for s in SETTINGS if DC.SETTINGS[s]["depth_mode"] == "linear"],
              "no_depth_clamp_direct": SETTINGS,
              "conf_always_applied": [s for s in SETTINGS if not DC.SETTINGS[s]["uncertainty_as_conf"]],
              "exp_dims_when_linear": [s for s in SETTINGS if not DC.SETTINGS[s]["dim_exp"]]}
    for w, where in expect.items():
        for s in SETTINGS:
            if s in where:
                assert table[s][w][0] >= 100, (w, s, table[s][w])
            else:
                assert table[s][w] == (0.0, 0.0), (w, s, table[s][w])
    # the uncertainty output tells `conf_always_applied` too
    assert all(table[s]["conf_always_applied"][1] > 0.5 for s in expect["conf_always_applied"])


def test_entry_point_refuses_bad_arguments_on_the_host():
    """mfx_decode_boxes_cfg validates before it touches the device: every MFX_ERR_ARG case returns -1 with its message (no GPU needed; the
    device module repeats this with real buffers and checks that nothing was launched)."""
    import ctypes
    from monoflex_amd import lib as L
    lib = L.load()
    s = DC.SETTINGS["e_car"]
    head = dict(depth_mode=s["depth_mode"], depth_range=tuple(s["depth_range"]), depth_ref=tuple(s["depth_ref"]), dim_mean=s["dim_mean"],
                dim_std=s["dim_std"], dim_modes=["linear", True, True], down_ratio=4, eps=1e-3)
    buf = (ctypes.c_float * 64)()
    p = ctypes.cast(buf, ctypes.c_void_p)                       # (never dereferenced: every call below fails its checks first)

    def call(ncls=1, K=7, null=False, **fields):
        c = L.decode_cfg(head, s["uncertainty_as_conf"], "hard")
        assert (c.depth_decode, c.dim_exp, c.dim_use_std, c.uncertainty_as_conf, c.output_depth) == (1, 0, 1, 1, 1)
        assert [round(v, 4) for v in c.dim_mean[:3]] == list(s["dim_mean"][0]) and list(c.depth_range) == [1.0, 60.0]
        for k, v in fields.items():
            if isinstance(v, tuple):
                getattr(c, k)[0], getattr(c, k)[1] = v
            else:
                setattr(c, k, v)
        rc = lib.mfx_decode_boxes_cfg(p, 64, 8, p, p, ncls, 1, 4, 4, K, p, p, p, ctypes.c_float(0.2), None if null else ctypes.byref(c), p, p, p, None, None)
        return rc, lib.mfx_last_error()
    for kw, msg in ((dict(null=True), b"null cfg"), (dict(depth_decode=3), b"depth_decode"), (dict(depth_decode=-1), b"depth_decode"),
                    (dict(output_depth=8), b"output_depth"), (dict(output_depth=-1), b"output_depth"), (dict(depth_range=(2.0, 1.0)), b"depth_range"),
                    (dict(depth_range=(0.1, float("inf"))), b"depth_range"), (dict(depth_range=(float("nan"), 100.0)), b"depth_range"),
                    (dict(ncls=4), b"ncls"), (dict(ncls=0), b"ncls"), (dict(K=257), b"K <= 256")):
        rc, err = call(**kw)
        assert rc == -1 and msg in err, (kw, rc, err)
