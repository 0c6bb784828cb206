"""MODEL.INPLACE_ABN False (conv3x3 -> BatchNorm2d -> ReLU head trunks) on the CPU: the float64 statement tests/head_act_ref.py against the
reference's own results (tests/golden/head_act.npz), the conditions on the test inputs, the module / key / checkpoint surface of the
predictor, the refusals, SyncBN marking, the Gram form's torch node with ReLU, and the C entry points that carry the activation.

Bounds of the golden pin: the reference ran in fp32, the statement in float64.  A trunk value is a 576-term fp32 sum and a head output a
256-term one over activations of size O(1), so the reference's own error is bounded by about K * 2^-24 * sum |terms| ~ 576 * 6e-8 * O(1)
= 3.5e-5 of the largest value; the maps are held to 1e-4 of max(1, largest reference value), gradient sums (sums of up to 2e5 such
values, compared to their absolute sums) to 1e-3.
"""
import ctypes
import logging
import os

import numpy as np
import pytest
import torch

from tests import head_act_ref as HA

GPU_TOL = dict(fp32=1e-4, bf16=5e-2)            # tests/test_gpu_head_act.py's bounds (those of tests/test_gpu_ops.py test_heads_fused_vs_torch)


@pytest.fixture(scope="module")
def gold(golden_dir):
    return np.load(os.path.join(golden_dir, "head_act.npz"))


@pytest.fixture(scope="module")
def predictor():
    from monoflex_amd.model.head.detector_predictor import _predictor
    cfg = HA.make_cfg()
    m = _predictor(cfg, 64)
    m.load_state_dict(HA.synthetic_state(m.state_dict()))
    return cfg, m


@pytest.fixture(scope="module")
def runs(predictor):
    """The statement's eval and train results (slope 0), computed once."""
    cfg, m = predictor
    _, ei, el = HA.edge_targets()
    x = HA.features()
    ev = HA.HeadActRef(m.state_dict(), cfg)
    with torch.no_grad():
        e_cls, e_reg = ev.forward(x, ei, el, train=False)
    tr = HA.HeadActRef(m.state_dict(), cfg, requires_grad=True)
    xt = x.double().requires_grad_()
    t_cls, t_reg = tr.forward(xt, ei, el, train=True)
    g_cls, g_reg = HA.loss_weights(t_cls.shape[1], t_reg.shape[1])
    ((HA.HeadActRef.sigmoid_hm(t_cls) * g_cls).sum() + (t_reg * g_reg).sum()).backward()
    return dict(ev=ev, e_cls=e_cls, e_reg=e_reg, tr=tr, t_cls=t_cls.detach(), t_reg=t_reg.detach(), dx=xt.grad)


def _rel(got, want):
    want = torch.as_tensor(want).double()
    return float((got.double() - want).abs().max()) / max(1.0, float(want.abs().max()))


def test_recorded_seeds_are_the_ones_the_tests_use(gold):
    for k, v in HA.SEEDS.items():
        assert int(gold[k]) == v, k
    assert float(gold["beta_shift"]) == HA.BETA_SHIFT and int(gold["subset"]) == HA.SUBSET
    assert [tuple(int(v) for v in r) for r in gold["orig_sizes"]] == [tuple(r) for r in HA.ORIG_SIZES]
    assert tuple(str(s) for s in gold["stat_trunks"]) == HA.STAT_TRUNKS


def test_state_dict_keys_are_the_references(gold, predictor):
    _, m = predictor
    keys = [str(k) for k in gold["keys"]]
    assert list(m.state_dict().keys()) == keys                      # the same keys in the same order (synthetic_state_dict draws in key order)
    assert "class_head.3.weight" in keys and "class_head.3.bias" in keys and not any(k.startswith("class_head.2") for k in keys)
    assert "class_head.1.num_batches_tracked" in keys and "reg_features.7.1.running_var" in keys
    assert isinstance(m.class_head[1], torch.nn.BatchNorm2d) and isinstance(m.class_head[2], torch.nn.ReLU)
    assert all(isinstance(f[1], torch.nn.BatchNorm2d) and isinstance(f[2], torch.nn.ReLU) and len(f) == 3 for f in m.reg_features)
    assert m.class_head[1].momentum == HA.make_cfg().MODEL.HEAD.BN_MOMENTUM


def test_eval_statement_equals_the_reference(gold, runs):
    assert _rel(HA.HeadActRef.sigmoid_hm(runs["e_cls"]), gold["eval_cls"]) < 1e-4
    assert _rel(runs["e_reg"], gold["eval_reg"]) < 1e-4


def test_train_statement_equals_the_reference(gold, runs):
    sub = HA.pixel_subset()
    assert _rel(HA.HeadActRef.sigmoid_hm(runs["t_cls"]), gold["train_cls"]) < 1e-4
    assert _rel(runs["t_reg"].flatten(2)[:, :, sub], gold["train_reg_subset"]) < 1e-4
    # d features: a trunk pre-activation closer to zero than the fp32 rounding of its 576-term sum can sit on the other side of the ReLU in the
    # fp32 reference (terms of ~0.03, accumulated error ~24 * 2^-24 * 0.03 / std ~ 1e-7; 4e-6 leaves a factor of margin).  Such a unit moves the
    # gradient of the 3 x 3 pixels under its filter and nothing else: every pixel NOT next to such a near-tie is held to the bound of the maps.
    near = torch.zeros(HA.B, 1, HA.H, HA.W)
    for z in runs["tr"].pre.values():
        near += (z.abs() < 4e-6).any(1, keepdim=True).float()
    ties = int(near.sum())
    near = torch.nn.functional.max_pool2d(near, 3, 1, 1).flatten(1)[:, sub] > 0
    err = (runs["dx"].flatten(2)[:, :, sub] - torch.as_tensor(gold["train_dx_subset"]).double()).abs().amax(1)
    off = err > 1e-4 * max(1.0, float(np.abs(gold["train_dx_subset"]).max()))
    print("d features: %d pixels off, %d near-ties, %d of %d pixels next to one" % (int(off.sum()), ties, int(near.sum()), near.numel()))
    assert not bool((off & ~near).any()) and int(near.sum()) <= 0.1 * near.numel()         # (the check still covers nine pixels in ten)
    s, a = float(runs["dx"].sum()), float(runs["dx"].abs().sum())
    assert abs(s - gold["train_dx_sums"][0]) < 1e-3 * gold["train_dx_sums"][1] and abs(a - gold["train_dx_sums"][1]) < 1e-3 * gold["train_dx_sums"][1]
    tr = runs["tr"]
    for n in HA.STAT_TRUNKS:
        for s_ in ("running_mean", "running_var"):
            assert _rel(tr.running["%s.%s" % (n, s_)], gold["train_%s.%s" % (n, s_)]) < 1e-5, (n, s_)
    grads = tr.grads()
    names = [str(n) for n in gold["grad_names"]]
    assert set(names) == set(grads) and len(names) == 59           # every parameter has a gradient in the reference and in the statement
    # (floor: a Conv1d bias in front of a train-mode BatchNorm1d has the gradient zero; the reference's value there is its rounding noise, ~2^-24 of
    # the gradients it is the difference of)
    floor = 1e-7 * float(gold["grad_sums"][:, 1].max())
    for n, (gs, ga) in zip(names, gold["grad_sums"]):
        g = grads[n]
        assert abs(float(g.sum()) - gs) <= 1e-3 * ga + floor, (n, float(g.sum()), gs, ga)
        assert abs(float(g.abs().sum()) - ga) <= 1e-3 * ga + floor, (n, float(g.abs().sum()), ga)


def test_inputs_tell_relu_from_leaky_and_have_dead_activations(predictor, runs):
    """A device test cannot pass by still computing the leaky form: with this state the two forms differ by at least ten times the loosest
    bound any device test grants (bf16: 5e-2, absolute on the class logits, of the largest value on the regression maps), and at least a
    fifth of the trunk activations are exactly zero (the ReLU's flat side is exercised, forward and backward)."""
    cfg, m = predictor
    _, ei, el = HA.edge_targets()
    leaky = HA.HeadActRef(m.state_dict(), cfg, slope=0.01)
    with torch.no_grad():
        l_cls, l_reg = leaky.forward(HA.features(), ei, el, train=False)
    tol = max(GPU_TOL.values())
    d_cls = float((l_cls - runs["e_cls"]).abs().max())
    d_reg = float((l_reg - runs["e_reg"]).abs().max()) / max(1.0, float(runs["e_reg"].abs().max()))
    print("leaky - relu: class logits %.3f, regression %.3f of the largest value (ten bounds: %.2f)" % (d_cls, d_reg, 10 * tol))
    assert d_cls >= 10 * tol and d_reg >= 10 * tol
    for which in ("ev", "tr"):
        acts = runs[which].acts
        assert len(acts) == 9
        for name, a in acts.items():
            zero = float((a == 0).double().mean())
            assert zero >= 0.2, (which, name, zero)


def test_refusals_name_their_reason():
    from monoflex_amd.model.head.detector_predictor import _predictor
    with pytest.raises(NotImplementedError, match="'GN'.*TypeError"):
        _predictor(HA.make_cfg(extra=["MODEL.HEAD.USE_NORMALIZATION", "GN"]), 64)
    with pytest.raises(NotImplementedError, match="without a normalisation"):
        _predictor(HA.make_cfg(extra=["MODEL.HEAD.USE_NORMALIZATION", "none"]), 64)
    with pytest.raises(NotImplementedError, match="without a normalisation"):
        _predictor(HA.make_cfg(inplace_abn=True, extra=["MODEL.HEAD.USE_NORMALIZATION", "none"]), 64)
    with pytest.raises(NotImplementedError, match="64 -> 256"):     # the checks that were there stay
        _predictor(HA.make_cfg(extra=["MODEL.HEAD.NUM_CHANNEL", 128]), 64)
    with pytest.raises(NotImplementedError, match="64 -> 256"):
        _predictor(HA.make_cfg(), 32)


def test_abn_form_is_what_it_was():
    from monoflex_amd import lib as L
    from monoflex_amd.model.head.detector_predictor import InPlaceABN, _predictor
    m = _predictor(HA.make_cfg(inplace_abn=True), 64)
    assert m.trunk_act == L.ACT_LEAKY and len(m.class_head) == 3 and isinstance(m.class_head[1], InPlaceABN)
    assert "class_head.2.bias" in m.state_dict() and "class_head.3.bias" not in m.state_dict()
    b = _predictor(HA.make_cfg(), 64)
    assert b.trunk_act == L.ACT_RELU
    b.abn_abs_weight = True                                          # applies to the ABN form only
    s, _ = b._abn_fold(b.class_head[1])
    from monoflex_amd import ops
    assert torch.equal(s, ops.fold_bn(b.class_head[1])[0])


def test_checkpoint_round_trip_and_the_report_of_the_other_form(tmp_path, predictor, caplog):
    from monoflex_amd.model.head.detector_predictor import _predictor
    from monoflex_amd.utils.check_point import Checkpointer
    cfg, m = predictor
    Checkpointer(m, save_dir=str(tmp_path)).save("bn_form")
    other = _predictor(cfg, 64)
    ck = Checkpointer(other, save_dir=str(tmp_path))
    ck.load(os.path.join(str(tmp_path), "bn_form.pth"), use_latest=False)
    assert ck.last_load["missing"] == [] and ck.last_load["unexpected"] == []               # no key left over, on either side
    sa, sb = m.state_dict(), other.state_dict()
    assert all(torch.equal(sa[k], sb[k]) for k in sa)
    # a checkpoint with the reference's own key list (as a reference run of this form would write it, under its 'module.' prefix)
    ref_ckpt = {"model": {"module." + k: v.clone() for k, v in sa.items()}}
    torch.save(ref_ckpt, os.path.join(str(tmp_path), "ref_form.pth"))
    third = _predictor(cfg, 64)
    ck = Checkpointer(third, save_dir=str(tmp_path))
    ck.load(os.path.join(str(tmp_path), "ref_form.pth"), use_latest=False)
    assert ck.last_load["missing"] == [] and ck.last_load["unexpected"] == [] and all(torch.equal(sa[k], v) for k, v in third.state_dict().items())
    # the other form: reported both ways
    abn = _predictor(HA.make_cfg(inplace_abn=True), 64)
    with caplog.at_level(logging.WARNING, logger="monoflex.checkpointer"):
        ck = Checkpointer(abn, save_dir=str(tmp_path))
        ck.load(os.path.join(str(tmp_path), "bn_form.pth"), use_latest=False)
    assert ck.last_load["missing"] == ["class_head.2.weight", "class_head.2.bias"]
    assert ck.last_load["unexpected"] == ["class_head.3.weight", "class_head.3.bias"]
    assert "class_head.2.weight" in caplog.text and "class_head.3.weight" in caplog.text
    Checkpointer(abn, save_dir=str(tmp_path)).save("abn_form")
    caplog.clear()
    with caplog.at_level(logging.WARNING, logger="monoflex.checkpointer"):
        ck = Checkpointer(other, save_dir=str(tmp_path))
        ck.load(os.path.join(str(tmp_path), "abn_form.pth"), use_latest=False)
    assert ck.last_load["missing"] == ["class_head.3.weight", "class_head.3.bias"]
    assert ck.last_load["unexpected"] == ["class_head.2.weight", "class_head.2.bias"]
    assert "class_head.3.weight" in caplog.text


def test_sync_bn_conversion_reaches_the_head_norms_of_the_bn_form_only():
    from monoflex_amd.engine.trainer import convert_sync_batchnorm
    from monoflex_amd.model.head.detector_predictor import _predictor, _synced
    for inplace, want in ((False, 9), (True, 0)):
        m = _predictor(HA.make_cfg(inplace_abn=inplace), 64)
        norms = [m.class_head[1]] + [f[1] for f in m.reg_features]
        n = convert_sync_batchnorm(m)
        assert n == want + 2                                         # + the two BatchNorm1d of the edge fusion
        assert sum(_synced(t) for t in norms) == want
        m = torch.nn.SyncBatchNorm.convert_sync_batchnorm(_predictor(HA.make_cfg(inplace_abn=inplace), 64))       # torch's own converter
        norms = [m.class_head[1]] + [f[1] for f in m.reg_features]
        assert sum(isinstance(t, torch.nn.SyncBatchNorm) for t in norms) == want == sum(_synced(t) for t in norms)
        from monoflex_amd import autograd as AG, lib as L
        assert all(AG.trunk_act(t) == (L.ACT_LEAKY if inplace else L.ACT_RELU) for t in norms)


def test_act_entry_points_are_exported_and_refuse_null_and_unknown_activations():
    from monoflex_amd import build, lib as L
    cdll = ctypes.CDLL(build.build_lib())                            # loads without a GPU
    header = open(os.path.join(HA.ROOT, "include", "monoflex_hip.h")).read()
    null = ctypes.c_void_p(None)
    for name in ("mfx_heads_fused_act", "mfx_edge_chain_act", "mfx_head_sparse_fwd_act", "mfx_head_sparse_bwd_act", "mfx_gram_heads_act"):
        assert name in L.SYMBOLS and ("int %s(" % name) in header
        fn = getattr(cdll, name)
        fn.restype, fn.argtypes = L.SYMBOLS[name]
        args = (None, 0, L.ACT_RELU, null) if name == "mfx_gram_heads_act" else (None, L.ACT_RELU, null)
        assert fn(*args) == -1, name                                 # MFX_ERR_ARG
    assert "MFX_ABI_VERSION 3" in header
    cdll.mfx_last_error.restype = ctypes.c_char_p
    # anything but MFX_ACT_LEAKY / MFX_ACT_RELU: MFX_ERR_UNSUPPORTED (descriptors that pass the pointer checks; nothing is launched)
    buf = (ctypes.c_float * 64)()
    p = ctypes.addressof(buf)
    d = L.HeadsDesc()
    for f in ("x", "w1", "scale1", "shift1", "w2", "bias2", "out"):
        setattr(d, f, p)
    d.nbranch, d.K_pad, d.ld_out, d.dtype = 1, 576, 64, L.MFX_BF16
    d.c_out[0] = 3
    for act in (L.ACT_NONE, L.ACT_DCN_OFFMASK, 7):
        assert cdll.mfx_heads_fused_act(ctypes.byref(d), act, null) == -2 and b"MFX_ACT_LEAKY or MFX_ACT_RELU" in cdll.mfx_last_error()
    assert cdll.mfx_heads_fused_act(ctypes.byref(d), L.ACT_RELU, null) == 0         # B * H * W == 0: nothing to do
    e = L.EdgeChainDesc()
    for f in ("x", "edge_xy", "w_trunk", "scale_trunk", "shift_trunk", "w_conv", "scale_conv", "shift_conv", "w_out", "bias_out", "out"):
        setattr(e, f, p)
    e.B, e.H, e.W, e.C, e.L, e.head_conv, e.ksize, e.dtype = 1, 4, 4, 64, 0, 256, 3, L.MFX_BF16
    assert cdll.mfx_edge_chain_act(ctypes.byref(e), L.ACT_NONE, null) == -2
    assert cdll.mfx_edge_chain_act(ctypes.byref(e), L.ACT_RELU, null) == 0          # L == 0
    s = L.HeadSparseDesc()
    s.rows, s.nbranch, s.C, s.B, s.H, s.W = p, 1, 256, 1, 4, 4
    assert cdll.mfx_head_sparse_fwd_act(ctypes.byref(s), L.ACT_NONE, null) == -2 and cdll.mfx_head_sparse_bwd_act(ctypes.byref(s), 5, null) == -2
    g = L.GramDesc()
    g.x, g.rows, g.nbranch, g.C, g.ld_out, g.dtype = p, p, 1, 64, 8, L.MFX_BF16
    g.k[0] = 4
    assert cdll.mfx_gram_heads_act(ctypes.byref(g), 2, L.ACT_NONE, null) == -2


def test_gram_torch_node_with_relu_equals_the_dense_form(monkeypatch):
    """tests/test_gram_heads_cpu.py test_gram_reg_heads_node_end_to_end_on_cpu with the other trunk form: the whole GramRegHeadsFn with
    act = ACT_RELU and real nn.BatchNorm2d holders against conv3x3 -> train-mode BatchNorm2d -> ReLU -> 1x1 heads in fp64 torch (forward table,
    the extra activation rows, running statistics, every gradient), the node's three library launches swapped for torch equivalents and the
    bounds as there.  beta is drawn around zero, so both sides of the ReLU are taken, by the objects' and by the extra rows."""
    from types import SimpleNamespace
    import torch.nn.functional as F
    from monoflex_amd import gram_heads as GH, lib as L
    from tests.test_gram_heads_cpu import _autocorr5
    monkeypatch.setattr(GH, "_autocorr5", lambda x: _autocorr5(x.double()).float())
    monkeypatch.setattr(GH.AG, "_colsum", lambda t: t.reshape(-1, t.shape[-1]).double().sum(0).float())
    monkeypatch.setattr(GH.AG, "_c", lambda t: t.contiguous())
    monkeypatch.setattr(GH.ops, "pack_conv", lambda w, dt, scale, shift, stride, pad: SimpleNamespace(w=w, scale=scale, shift=shift, pad=pad))

    def conv2d(x, p):
        y = F.conv2d(x.permute(0, 3, 1, 2).double(), p.w.double(), None, 1, p.pad) * p.scale.double().view(1, -1, 1, 1) + p.shift.double().view(1, -1, 1, 1)
        return y.permute(0, 2, 3, 1).float().contiguous()
    monkeypatch.setattr(GH.ops, "conv2d", conv2d)

    g = torch.Generator().manual_seed(37)
    Bn, Hn, Wn, Cin, C, N, R2 = 2, 7, 9, 8, 16, 10, 23
    ks, offs = (3, 5), (0, 4)
    rows = torch.zeros(N, 72)
    rows[:, 0] = 1.0; rows[7:, 0] = 0.0
    rows[:, 57] = torch.randint(0, Bn, (N,), generator=g).float()
    rows[:, 2] = torch.randint(0, Wn, (N,), generator=g).float(); rows[:, 3] = torch.randint(0, Hn, (N,), generator=g).float()
    rows[0, 2:4] = torch.tensor([0.0, 0.0]); rows[1, 2:4] = torch.tensor([Wn - 1.0, Hn - 1.0]); rows[2] = rows[3]
    erows = torch.randint(0, Bn * Hn * Wn, (R2,), generator=g)
    x = torch.randn(Bn, Hn, Wn, Cin, generator=g)
    wt = [torch.randn(C, Cin, 3, 3, generator=g) / 8.0 for _ in ks]
    w2 = [torch.randn(k, C, 1, 1, generator=g) * 0.3 for k in ks]
    b2 = [torch.randn(k, generator=g) * 0.1 for k in ks]
    dout, dae = torch.randn(N, 10, generator=g), torch.randn(R2, C, generator=g) * 0.1
    holders = [torch.nn.BatchNorm2d(C) for _ in ks]
    for a in holders:
        with torch.no_grad():
            a.weight.copy_(torch.rand(C, generator=g) + 0.5); a.bias.copy_(torch.randn(C, generator=g) * 0.3)
    xr = x.double().permute(0, 3, 1, 2).clone().requires_grad_()
    rw = [w.double().clone().requires_grad_() for w in wt]
    rw2 = [w.double().clone().requires_grad_() for w in w2]
    rb2 = [b.double().clone().requires_grad_() for b in b2]
    bns = []
    for a in holders:
        m = torch.nn.BatchNorm2d(C).double()
        with torch.no_grad():
            m.weight.copy_(a.weight.double()); m.bias.copy_(a.bias.double())
        bns.append(m)
    bi, cy, cx, valid = rows[:, 57].long(), rows[:, 3].long(), rows[:, 2].long(), rows[:, 0].double()
    tot, outs = 0, []
    for i, k in enumerate(ks):
        act = F.relu(bns[i](F.conv2d(xr, rw[i], None, 1, 1)))
        o = F.conv2d(act, rw2[i], rb2[i]).permute(0, 2, 3, 1)[bi, cy, cx] * valid[:, None]
        outs.append(o)
        tot = tot + (o * dout[:, offs[i]:offs[i] + k].double()).sum()
        if i == 1:
            ae_ref = act.permute(0, 2, 3, 1).reshape(-1, C)[erows]
            tot = tot + (ae_ref * dae.double()).sum()
    tot.backward()
    xd = x.clone().requires_grad_()
    dw = [w.clone().requires_grad_() for w in wt]
    dw2 = [w.clone().requires_grad_() for w in w2]
    db2 = [b.clone().requires_grad_() for b in b2]
    out, ae = GH.gram_reg_heads(xd, rows, holders, offs, 10, dw, [a.weight for a in holders], [a.bias for a in holders], dw2, db2, sync=False,
                                extra_branch=1, extra_rows=erows, act=L.ACT_RELU)
    ((out * dout).sum() + (ae * dae).sum()).backward()
    rel = lambda a, b: float((a.detach().double() - b.detach().double()).abs().max() / b.detach().double().abs().max().clamp(min=1e-20))      # noqa: E731
    zero = float((ae == 0).float().mean())
    assert 0.2 < zero < 0.8, zero                                                                           # both sides of the ReLU
    assert bool(((ae == 0) == (ae_ref == 0)).all()) and rel(ae, ae_ref.detach()) < 1e-4
    assert rel(xd.grad, xr.grad.permute(0, 2, 3, 1)) < 2e-4, rel(xd.grad, xr.grad.permute(0, 2, 3, 1))
    for i, k in enumerate(ks):
        assert rel(out[:, offs[i]:offs[i] + k], outs[i].detach()) < 1e-4
        assert rel(dw[i].grad, rw[i].grad) < 2e-4 and rel(dw2[i].grad, rw2[i].grad) < 2e-4 and rel(db2[i].grad, rb2[i].grad) < 2e-4
        assert rel(holders[i].weight.grad, bns[i].weight.grad) < 2e-4 and rel(holders[i].bias.grad, bns[i].bias.grad) < 2e-4
        assert rel(holders[i].running_var, bns[i].running_var) < 1e-4 and rel(holders[i].running_mean, bns[i].running_mean) < 1e-4
        assert int(holders[i].num_batches_tracked) == 1
    assert float(out[rows[:, 0] == 0].abs().max()) == 0.0 and float(out[:, 3].abs().max()) == 0.0          # empty slots; the unused column
    # the leaky form of the same inputs is another function: the activation really travels
    out_l, _ = GH.gram_reg_heads(x.clone(), rows, holders, offs, 10, dw, [a.weight for a in holders], [a.bias for a in holders], dw2, db2, sync=False,
                                 extra_branch=1, extra_rows=erows)
    assert float((out_l - out).abs().max()) > 1e-4
    with pytest.raises(NotImplementedError, match="ACT_LEAKY or ACT_RELU"):
        GH.gram_reg_heads(xd, rows, holders, offs, 10, dw, [a.weight for a in holders], [a.bias for a in holders], dw2, db2, sync=False, act=L.ACT_NONE)
