"""Device tests of the reduced head sets (the reference's ablation ladder): the per-object loss kernel (csrc/loss_kernels.hip with
cfg.ch[i] == -1 and cfg.reg_width < 50) and the box decode (csrc/decode.hip mfx_decode_boxes_heads) against the float64 restatement
tests/head_sets_ref.py, which tests/test_head_sets_ref_cpu.py anchors to the reference's own recorded outputs.

Loss kernel, per set x corner depth mode x MODIFY_INVALID_KEYPOINT_DEPTH: the small input of tests/head_sets_cases.py (B = 3, 24 x 80 map,
MAX_OBJECTS 40: an image with no object, truncated objects, invalid keypoint groups, uncertainties past and on both clamps, a 2D box of
zero area; tests/test_head_sets_cpu.py asserts all of that on the CPU, and that at most 5 % of its valid rows sit near a selection), in
the dense NHWC form -- the R channels at [8, 8 + R) of a 64-wide row whose other entries hold junk of the order 1e3 -- and in the
gathered (N, R) form.  Bounds of tests/test_gpu_object_loss_configs.py: terms 2e-5 max(1,|ref|), logged 1e-4 max(1,|ref|), gradients
2e-5 max(1,max|ref|); the backward kernel's weighted sum over the terms is held to 2e-5 max(1,max|want|) of that sum, as there, and must
write nothing outside the R channels (dense: the junk columns of the gradient map stay 0; gathered: a guard band behind the table stays 0).

Decode kernel, per set x OUTPUT_DEPTH it can serve x UNCERTAINTY_AS_CONFIDENCE: case b3_k50 of tests/decode_cases.py (24 x 40), its
50 channels sliced and permuted into the set's layout inside the 64-wide row, the rest left as it was (values a wrong offset would
read).  Per-column bounds of tests/test_gpu_decode_cfg.py (4x the float32 reference's error, decode_cfg_ref.YARDSTICK['yaml']);
topk and valid EQUAL the restatement; unc exactly 0, and the score exactly topk's, where the reference reports None.  The full set
through the new entry is bit-identical to mfx_decode_boxes_cfg.

Argument errors are checked by return code: nothing is launched.
"""
import ctypes
import functools

import numpy as np
import pytest
import torch

from tests import decode_cases as C
from tests import decode_cfg_ref as DC
from tests import decode_ref as D
from tests import head_sets_cases as HC
from tests import head_sets_ref as HS
from tests.head_sets_cases import compare_with_restatement, evaluator, small_case

pytestmark = pytest.mark.gpu
DEV = "cuda"
LD, CH_OFF = 64, 8
P = lambda t: ctypes.c_void_p(t.data_ptr())                     # noqa: E731


@functools.lru_cache(maxsize=None)
def _case(name, corner, modify):
    return small_case(name, corner, modify)


def _rows(ev, tg):
    from monoflex_amd.structures.params_3d import make_train_target
    _, tv = ev.prepare_targets([make_train_target(t) for t in tg])
    return tv["object_rows"].contiguous()


def _forms(reg_set, rows):
    """The two geometries of mfx_object_loss on the same data: dense (B, H, W, 64) with junk around the R channels, and the gathered
    (N, R) table (row n = the centre pixel of object row n) followed by a guard band."""
    B, R, H, W = reg_set.shape
    dense = torch.randn(B, H, W, LD, generator=torch.Generator().manual_seed(5)) * 1e3 + 777.0
    dense[..., CH_OFF:CH_OFF + R] = reg_set.permute(0, 2, 3, 1)
    b, cx, cy = rows[:, 57].long().clamp(0, B - 1), rows[:, 2].long().clamp(0, W - 1), rows[:, 3].long().clamp(0, H - 1)
    table = reg_set.permute(0, 2, 3, 1)[b, cy, cx].contiguous()
    return dense.contiguous(), table


@pytest.mark.parametrize("modify", [True, False])
@pytest.mark.parametrize("name,corner", HC.SET_MODES)
def test_loss_kernel_dense_and_gathered(name, corner, modify):
    from monoflex_amd import lib as L
    lib = L.load()
    ev, tg, reg_set, ref, grads_ref, drop, plan = _case(name, corner, modify)
    assert int(drop.sum()) <= 0.05 * ref.n
    cfg = ev.object_loss_cfg()
    rows = _rows(ev, tg)
    B, R, H, W = reg_set.shape
    N = rows.shape[0]
    assert cfg.reg_width == R == HS.WIDTHS[name] and list(cfg.ch) == HS.ch_table(name) and N == B * HC.SMALL["max_objs"]
    dense, table = _forms(reg_set, rows)
    rows_d = rows.to(DEV)
    valid = torch.nonzero(rows[:, 0] != 0).flatten()
    assert torch.equal(valid, ref.bi * HC.SMALL["max_objs"] + torch.tensor([s for _, s in plan["objects"]]))       # the restatement's row order
    gout = torch.tensor([1.0, 0.5, 1.5, 0.75, 1.25, 1.0, 0.25, 2.0, 0.6, 1.1])
    want_bwd = (gout.double().view(-1, 1, 1) * grads_ref).sum(0)                                                   # (n, R), per object
    bwd_bound = 2e-5 * max(1.0, float(want_bwd.abs().max()))
    for form in ("dense", "gathered"):
        if form == "dense":
            reg, geom, ld, off = dense.to(DEV), (B, H, W), LD, CH_OFF
            dreg = torch.zeros(B, H, W, LD, device=DEV)
        else:
            reg, geom, ld, off = table.to(DEV), (0, 1, N), R, 0
            dreg = torch.zeros(N * R + 256, device=DEV)                                  # the table + a guard band
        vals = torch.full((L.OBJ_VALUES,), float("nan"), device=DEV)
        G = torch.full((N, L.OBJ_TERMS, 64), float("nan"), device=DEV)
        L.check(lib.mfx_object_loss(P(reg), *geom, ld, off, P(rows_d), N, ctypes.byref(cfg), P(vals), P(G), None), "mfx_object_loss")
        g_d = gout.to(DEV)
        L.check(lib.mfx_object_loss_backward_width(P(G), P(g_d), P(rows_d), N, *geom, P(dreg), ld, off, R, None), "mfx_object_loss_backward_width")
        torch.cuda.synchronize()
        vals, G, dreg = vals.cpu(), G.cpu(), dreg.cpu()
        assert bool(torch.isfinite(vals).all()) and bool(torch.isfinite(G).all())
        assert float(G[..., R:].abs().max()) == 0.0 and float(G[rows[:, 0] == 0].abs().max()) == 0.0     # lanes >= R and empty rows carry nothing
        # each term's gradient per object, summed over the objects that share a pixel as the restatement's autograd does (none do here)
        assert len({(int(b), int(x), int(y)) for b, (x, y) in zip(ref.bi, ref.cen.tolist())}) == ref.n
        grads = G[valid][:, :, :R].permute(1, 0, 2)
        compare_with_restatement("%s/%s/modify=%d %s" % (name, corner, modify, form), name, ref, grads_ref, vals[:L.OBJ_TERMS], vals[L.OBJ_TERMS:],
                                 grads, 2e-5, drop)
        if form == "dense":
            got = dreg[ref.bi, ref.cen[:, 1], ref.cen[:, 0]]
            assert float(got[:, :CH_OFF].abs().max()) == 0.0 and float(got[:, CH_OFF + R:].abs().max()) == 0.0   # nothing outside the R channels
            rest = dreg.clone()
            rest[ref.bi, ref.cen[:, 1], ref.cen[:, 0]] = 0
            assert float(rest.abs().max()) == 0.0                                                                # nothing off the centres
            got = got[:, CH_OFF:CH_OFF + R]
        else:
            assert float(dreg[N * R:].abs().max()) == 0.0                                                        # the guard band is untouched
            tab = dreg[:N * R].view(N, R)
            assert float(tab[rows[:, 0] == 0].abs().max()) == 0.0
            got = tab[valid]
        keep = ~drop
        e = float((got[keep].double() - want_bwd[keep]).abs().max()) / bwd_bound
        print("%s/%s/modify=%d %s: backward error/bound %.3f" % (name, corner, modify, form, e))
        assert e <= 1.0


def test_loss_kernel_argument_errors():
    """MFX_ERR_ARG (-1) by return code; the output buffers keep their NaN fill: nothing ran."""
    from monoflex_amd import lib as L
    lib = L.load()
    ev, tg, reg_set, *_ = _case("s000", "direct", True)
    rows = _rows(ev, tg).to(DEV)
    B, R, H, W = reg_set.shape
    N = rows.shape[0]
    reg = torch.zeros(B, H, W, LD, device=DEV)
    vals = torch.full((L.OBJ_VALUES,), float("nan"), device=DEV)
    G = torch.full((N, L.OBJ_TERMS, 64), float("nan"), device=DEV)

    def call(name="s000", ld=LD, off=CH_OFF, **edit):
        c = L.ObjectLossCfg.from_buffer_copy(evaluator(name).object_loss_cfg())
        for k, v in edit.items():
            if k.startswith("ch"):
                c.ch[int(k[2:])] = v
            else:
                setattr(c, k, v)
        return lib.mfx_object_loss(P(reg), B, H, W, ld, off, P(rows), N, ctypes.byref(c), P(vals), P(G), None)

    assert call() == 0
    torch.cuda.synchronize()
    vals.fill_(float("nan"))
    G.fill_(float("nan"))
    for what, rc in (("absent required key", call(ch7=-1)), ("absent required key 2d_dim", call(ch0=-1)),
                     ("keypoint_mean without corner_offset", call(corner_depth_mode=1)), ("soft_combine without uncertainties", call("s011", corner_depth_mode=2)),
                     ("hard_combine without corner_uncertainty", call("s110", corner_depth_mode=3)),
                     ("ch >= R", call(ch7=26)), ("a key reaching past R", call(ch5=19)), ("ch_off + R > ld", call(ld=33)), ("ch_off + R > ld (2)", call(off=39)),
                     ("reg_width > 50", call(reg_width=51)), ("corner_uncertainty without corner_offset", call("s011", ch2=-1))):
        assert rc == -1, what
        assert L.load().mfx_last_error()
    dreg = torch.zeros(B, H, W, LD, device=DEV)
    g = torch.ones(10, device=DEV)
    bw = lambda ld, off, R_: lib.mfx_object_loss_backward_width(P(G), P(g), P(rows), N, B, H, W, P(dreg), ld, off, R_, None)
    assert bw(LD, CH_OFF, 0) == -1 and bw(LD, CH_OFF, 51) == -1 and bw(33, CH_OFF, 26) == -1 and bw(LD, 39, 26) == -1
    torch.cuda.synchronize()
    assert bool(torch.isnan(vals).all()) and bool(torch.isnan(G).all()) and float(dreg.abs().max()) == 0.0


# ---- decode ------------------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _decode_inputs(name):
    d = C.case_inputs("b3_k50")
    assert d["hmap"].shape == (3, C.H, C.W, LD) and d["reg_off"] == CH_OFF
    hm = HS.take(d["hmap"][..., CH_OFF:CH_OFF + 50], name, 3, ld=LD, off=CH_OFF, junk=d["hmap"])
    R = HS.WIDTHS[name]
    assert np.abs(hm[..., CH_OFF + R:]).max() > 1                          # non-zero junk behind the R channels
    return dict(d, hmap=hm)


def _device(d):
    t = lambda a, dt: torch.from_numpy(np.array(a)).to(DEV, dt)
    return (t(d["hmap"], torch.float32), d["reg_off"], t(d["scores"], torch.float32), t(d["index"], torch.int32), t(d["calib"], torch.float32),
            t(d["pad"], torch.int32), t(d["img_size"], torch.int32), float(d["threshold"]))


def _decode_cfg(uac):
    from monoflex_amd import lib as L
    s = HC.settings()
    head = dict(depth_mode=s["depth_mode"], depth_range=tuple(s["depth_range"]), depth_ref=tuple(s["depth_ref"]), dim_mean=s["dim_mean"],
                dim_std=s["dim_std"], dim_modes=["exp", True, False], down_ratio=4, eps=1e-3)
    return L.decode_cfg(head, uac)


DECODE_CASES = [(n, m) for n in HS.SETS for m in HS.output_depths(n)]


@pytest.mark.parametrize("uac", [True, False])
@pytest.mark.parametrize("name,mode", DECODE_CASES)
def test_decode_kernel_vs_restatement(name, mode, uac):
    from monoflex_amd import lib as L
    from monoflex_amd import ops
    d = _decode_inputs(name)
    ref = HS.decode_ref(name, d["hmap"], d["reg_off"], d["scores"], d["index"], d["calib"], d["pad"], d["img_size"], d["threshold"], mode,
                        HC.settings(uncertainty_as_conf=uac))
    hs = L.HeadSet(HS.SETS[name], HS.channels(name))
    out = ops.decode_boxes(*_device(d), depth_mode=mode, cfg=_decode_cfg(uac), return_unc=True, heads=hs.layout())
    torch.cuda.synchronize()
    det, topk, valid, unc = [t.cpu().numpy() for t in out]
    what = "%s %s uac=%d" % (name, mode, uac)
    assert np.isfinite(det).all() and np.isfinite(unc).all(), what
    assert np.array_equal(topk.astype(np.float64), ref["topk"]) and np.array_equal(valid, ref["valid"]), what
    assert float(D.near_rows(ref, mode).mean()) <= D.NEAR_CAP, what
    err = D.column_errors(det, ref, mode)
    uerr = DC.unc_errors(unc, ref)
    print("%-28s %s  sigma %.2e  conf %.2e" % (what, D.format_errors(err), uerr[0], uerr[1]))
    bound = DC.bounds("yaml")
    assert (err <= bound).all(), "%s: column(s) %s past 4x the float32 reference's error: %s" % (
        what, [D.COLUMNS[i] for i in np.nonzero(err > bound)[0]], D.format_errors(err))
    if uac and HS.has_depth_error(name, mode):
        assert (uerr <= bound[13]).all() and (unc[..., 0] > 0).all(), what
    else:                                                                 # the reference reports None: nothing reported, the raw score
        assert (unc == 0).all() and np.array_equal(det[..., 13], topk[..., 0]), what


@pytest.mark.parametrize("uac", [True, False])
@pytest.mark.parametrize("mode", D.MODES)
def test_full_set_through_the_new_entry_is_bitwise_the_cfg_entry(mode, uac):
    from monoflex_amd import lib as L
    from monoflex_amd import ops
    args = _device(C.case_inputs("b3_k50", "ties"))
    old = ops.decode_boxes(*args, depth_mode=mode, cfg=_decode_cfg(uac), return_unc=True)
    new = ops.decode_boxes(*args, depth_mode=mode, cfg=_decode_cfg(uac), return_unc=True, heads=L.HeadSet(HS.SETS["s111"], HS.channels("s111")).layout())
    torch.cuda.synchronize()
    assert all(torch.equal(a, b) for a, b in zip(old, new))


@pytest.mark.parametrize("uac", [True, False])
def test_decode_oracle_of_the_set_without_depth_uncertainty_vs_reference(uac):
    """OUTPUT_DEPTH 'oracle' for set s011 through PostProcessor.forward (decode_oracle: three keypoint-depth columns, their mean where a
    detection meets no object) against the rows the reference's own PostProcessor gave on the same maps and ground truth
    (tests/golden/head_sets.npz); tolerance of tests/test_gpu_ops.py test_decode_depth_modes_vs_reference_goldens, which compares the full
    set's oracle rows the same way.  The recorded rows leave the mean in a third of the cases and take each of the three columns."""
    from monoflex_amd.model.head.detector_infer import make_post_processor
    from monoflex_amd.structures.params_3d import Calibration, ParamsList
    g = HC.golden()
    images = tuple(int(i) for i in np.atleast_1d(g["decode_inputs/images"]))
    maps = C.structured_maps(int(g["decode_inputs/map_seed"]), images)
    scores, index = C.peak_lists(int(g["decode_inputs/list_seed"]), len(images), int(g["decode_inputs/K"]),
                                 [tuple(r) for r in np.atleast_2d(g["decode_inputs/score_ranges"])])
    name, i = "s011", images[0]
    hm = HS.take(maps["hmap"][..., CH_OFF:CH_OFF + 50], name, 3, ld=LD, off=CH_OFF, junk=maps["hmap"])
    hm[..., :3] = C.peak_logits(scores, index)
    post = make_post_processor(HC.cfg_for(name, extra=[HC.HEAD + "OUTPUT_DEPTH", "oracle", "TEST.UNCERTAINTY_AS_CONFIDENCE", uac,
                                                        "INPUT.WIDTH_TRAIN", C.W * 4, "INPUT.HEIGHT_TRAIN", C.H * 4]))
    assert post.head_set.oracle_columns() == ('keypoints_center', 'keypoints_02', 'keypoints_13')
    t = ParamsList(image_size=tuple(C.IMAGES[i]["size"]), is_train=False)
    t.add_field("pad_size", torch.tensor(C.IMAGES[i]["pad"], dtype=torch.int64))
    t.add_field("calib", Calibration(C.image_P(i)))
    boxes, cls, depth = (g["s011/decode/oracle/" + k] for k in ("gt_boxes", "gt_cls", "gt_depth"))
    n = boxes.shape[0]
    pad_rows = lambda a: torch.cat((torch.from_numpy(a), torch.zeros((3,) + a.shape[1:], dtype=torch.from_numpy(a).dtype)))
    t.add_field("reg_mask", torch.cat((torch.ones(n, dtype=torch.uint8), torch.zeros(3, dtype=torch.uint8))))
    t.add_field("cls_ids", pad_rows(cls))
    t.add_field("gt_bboxes", pad_rows(boxes))
    t.add_field("locations", pad_rows(np.stack((np.zeros(n, np.float32), np.zeros(n, np.float32), depth), axis=1)))
    res, ev, _ = post({"hm_nhwc": torch.from_numpy(hm).to(DEV), "cls": None}, [t])
    torch.cuda.synchronize()
    want = np.concatenate((g["s011/decode/cols0_9"], g["s011/decode/oracle/uac%d_cols9_14" % uac]), axis=1)
    got = res.cpu().numpy()
    assert got.shape == want.shape and 20 <= want.shape[0] < 50
    print("s011 oracle uac=%d: worst |got - want| %.2e" % (uac, np.abs(got - want).max()))
    assert np.allclose(got, want, rtol=1e-4, atol=2e-3), np.abs(got - want).max(axis=0)
    modes = [str(m) for m in g["s011/decode/modes"]]
    z = g["s011/decode/cols9_14"]
    took = [int((want[:, 11] == z[modes.index(m)][:, 2]).sum()) for m in ('keypoints_center', 'keypoints_02', 'keypoints_13')]
    assert min(took) >= 2 and float((want[:, 11] != z[modes.index('mean')][:, 2]).mean()) > 0.3      # the recorded choice is not one column
    if uac:
        err = g["s011/decode/oracle/error"]
        assert np.allclose(ev['estimated_depth_error'].cpu().numpy(), err[:, 0], rtol=1e-4, atol=1e-5)
        assert np.allclose(ev['uncertainty_conf'].cpu().numpy(), err[:, 1], rtol=1e-4, atol=1e-5)
    else:
        assert ev['estimated_depth_error'] is None and ev['uncertainty_conf'] is None
    with pytest.raises(NotImplementedError):                              # a set without corner_uncertainty has no oracle
        p0 = make_post_processor(HC.cfg_for("s010", extra=[HC.HEAD + "OUTPUT_DEPTH", "direct"]))
        p0.output_depth = "oracle"
        p0({"hm_nhwc": torch.from_numpy(hm).to(DEV), "cls": None}, [t])


def test_decode_argument_errors():
    from monoflex_amd import lib as L
    lib = L.load()
    hm, reg_off, sc, ix, calib, pad, size, thr = _device(_decode_inputs("s000"))
    B, H, W, ld = hm.shape
    K = sc.shape[2]
    det = torch.full((B, K, 14), float("nan"), device=DEV)
    topk, valid = torch.zeros(B, K, 5, device=DEV), torch.zeros(B, K, dtype=torch.int32, device=DEV)

    def call(name, mode, ld=ld, reg_off=reg_off, **edit):
        lay = L.HeadSet(HS.SETS[name], HS.channels(name)).layout()
        for k, v in edit.items():
            if k.startswith("ch"):
                lay.ch[int(k[2:])] = v
            else:
                setattr(lay, k, v)
        c = _decode_cfg(True)
        c.output_depth = L.DEPTH_MODES[mode]
        return lib.mfx_decode_boxes_heads(P(hm), ld, reg_off, P(sc), P(ix), 3, B, H, W, K, P(calib), P(pad), P(size), ctypes.c_float(thr),
                                          ctypes.byref(c), ctypes.byref(lay), P(det), P(topk), P(valid), None, None)

    for name in HS.SETS:                                                  # every output_depth a set cannot serve
        for mode in HS.OUTPUT_DEPTHS:
            if mode not in HS.output_depths(name):
                assert call(name, mode) == -1, (name, mode)
    assert call("s000", "direct", ch7=-1) == -1 and call("s000", "direct", ch4=-1) == -1              # an absent required key
    assert call("s000", "direct", ch7=26) == -1 and call("s000", "direct", ch5=19) == -1              # ch >= R; a key reaching past R
    assert call("s000", "direct", ld=33) == -1 and call("s000", "direct", reg_off=39) == -1           # reg_off + R > ld
    assert call("s011", "direct", ch2=-1) == -1 and call("s000", "direct", reg_width=51) == -1
    torch.cuda.synchronize()
    assert bool(torch.isnan(det).all())                                   # nothing was launched
    assert call("s000", "direct") == 0
    torch.cuda.synchronize()
    assert bool(torch.isfinite(det).all())
