"""The edge fusion's other settings (MODEL.HEAD.EDGE_FUSION_KERNEL_SIZE 1 / 3 / 5 / 7, EDGE_FUSION_NORM 'BN' or none, EDGE_FUSION_RELU) without a GPU:

  * tests/edge_fusion_ref.py, the float64 statement the device tests compare with, against tests/golden/edge_fusion_settings.npz -- what the reference's
    own predictor returned under five settings (tools/gen_edge_fusion_golden.py), eval and train mode.  The recording is fp32 arithmetic: the bound is
    1e-5 x max(1, |recorded|), as the edge-chain tests take for fp32 accumulation.  A statement with the window off by one tap, or with a BatchNorm1d
    where the setting has none, misses the recording by more than 100 x that bound: the recording tells the settings apart;
  * the predictor builds under every served setting with the reference's state-dict keys, and refuses even windows and windows above 7 by name;
  * make_edge_rowmap / edge_plan for halo 0 .. 3 against a plain loop; pack_edge_chain's shapes and fragment order per window, the no-norm fold;
  * mfx_edge_chain_ks's argument checks, which come before any device work.

The predictor's unfused forward_train is tensor indexing around AG.conv2d / AG.bn_act, which are HIP operators without a CPU form: that path is left to
tests/test_gpu_edge_fusion_settings.py."""
import ctypes
import os

import numpy as np
import pytest
import torch

import edge_fusion_ref as EF
from tests import head_act_ref as HA

D64 = torch.float64
ALL_SERVED = [(k, norm, relu) for k in (1, 3, 5, 7) for norm in ("BN", "none") for relu in (False, True)]


@pytest.fixture(scope="module")
def gold(golden_dir):
    return np.load(os.path.join(golden_dir, "edge_fusion_settings.npz"))


def _predictor(k, norm, relu, inplace_abn=False):
    from monoflex_amd.model.head.detector_predictor import _predictor as Predictor
    cfg = HA.make_cfg(inplace_abn=inplace_abn, extra=EF.setting_opts(k, norm, relu))
    m = Predictor(cfg, 64)
    m.load_state_dict(HA.synthetic_state(m.state_dict()))
    return cfg, m


def _border(t, ei, el):
    return torch.cat([t[b][:, ei[b, :el[b], 1], ei[b, :el[b], 0]] for b in range(t.shape[0])], 1)


def _statement(cfg, sd, mode, **wrong):
    """(cls after sigmoid_hm, the two 3d_offset channels) at the border pixels, and the statement itself"""
    _, ei, el = HA.edge_targets()
    st = EF.EdgeFusionRef(sd, cfg, **wrong)
    with torch.no_grad():
        cls, reg = st.forward(HA.features(), ei, el, train=mode == "train")
    oi, oj = st.offset_index
    lo = sum(sum(c) for c in st.channels[:oi]) + sum(st.channels[oi][:oj])
    return _border(st.sigmoid_hm(cls), ei, el), _border(reg[:, lo:lo + 2], ei, el), st


@pytest.mark.parametrize("k,norm,relu", EF.SETTINGS)
def test_statement_meets_the_reference_recording(k, norm, relu, gold):
    name = EF.setting_name(k, norm, relu)
    assert name in list(gold["settings"])
    cfg, m = _predictor(k, norm, relu)
    sd = m.state_dict()
    _, ei, el = HA.edge_targets()
    assert torch.equal(el, torch.from_numpy(gold["edge_len"])) and int(el[0]) != int(el[1])
    for mode in ("eval", "train"):
        w_cls, w_off = (torch.from_numpy(gold["%s/%s_%s" % (name, mode, q)]).double() for q in ("cls", "off"))
        assert w_cls.shape == (3, int(el.sum())) and w_off.shape == (2, int(el.sum()))
        b_cls, b_off = 1e-5 * max(1.0, float(w_cls.abs().max())), 1e-5 * max(1.0, float(w_off.abs().max()))
        g_cls, g_off, st = _statement(cfg, sd, mode)
        e_cls, e_off = float((g_cls - w_cls).abs().max()), float((g_off - w_off).abs().max())
        print("%s %s: cls %.2e (bound %.1e) 3d_offset %.2e (bound %.1e)" % (name, mode, e_cls, b_cls, e_off, b_off))
        assert e_cls <= b_cls and e_off <= b_off
        if mode == "train" and norm == "BN":
            for f in ("trunc_heatmap_conv", "trunc_offset_conv"):
                for s in ("running_mean", "running_var"):
                    want = torch.from_numpy(gold["%s/train_%s.1.%s" % (name, f, s)]).double()
                    assert float((st.running["%s.1.%s" % (f, s)] - want).abs().max()) <= 1e-5 * max(1.0, float(want.abs().max())), (f, s)
        # the counter-examples: the window off by one tap; a BatchNorm1d (the k = 3 'BN' model's own) where the setting has none
        wrong = [dict(tap_shift=1)] if k > 1 else []
        if norm != "BN":
            _, mb = _predictor(k, "BN", relu)
            wrong.append(dict(norm=True, norm_state={q: v for q, v in mb.state_dict().items() if q.startswith("trunc_") and ".1." in q}))
        for kw in wrong:
            x_cls, x_off, _ = _statement(cfg, sd, mode, **kw)
            assert float((x_off - w_off).abs().max()) >= 100 * b_off, (name, mode, list(kw))
            assert float((x_cls - w_cls).abs().max()) >= 100 * b_cls, (name, mode, list(kw))


def test_k1_recording_differs_from_a_shifted_tap(gold):
    """k = 1 has one tap: reading the NEXT position instead misses the recording as widely as the other windows' shifts do."""
    cfg, m = _predictor(1, "BN", False)
    w_off = torch.from_numpy(gold["k1_bn_lin/eval_off"]).double()
    x_cls, x_off, _ = _statement(cfg, m.state_dict(), "eval", tap_shift=1)
    assert float((x_off - w_off).abs().max()) >= 100 * 1e-5 * max(1.0, float(w_off.abs().max()))


@pytest.mark.parametrize("inplace_abn", [False, True])
def test_predictor_builds_under_every_served_setting(inplace_abn, gold):
    for k, norm, relu in ALL_SERVED:
        cfg, m = _predictor(k, norm, relu, inplace_abn)
        assert m.edge_halo == k // 2 and m.trunc_heatmap_conv[0].kernel_size == (k,) and m.trunc_offset_conv[0].padding_mode == "replicate"
        assert isinstance(m.trunc_heatmap_conv[1], torch.nn.BatchNorm1d) == (norm == "BN") and isinstance(m.trunc_offset_conv[2], torch.nn.ReLU) == relu
        keys = list(m.state_dict().keys())
        assert ("trunc_heatmap_conv.1.running_mean" in keys) == (norm == "BN")
        name = EF.setting_name(k, norm, relu)
        if name in list(gold["settings"]) and not inplace_abn:
            assert keys == list(gold[name + "/keys"]), name
        from monoflex_amd.engine.trainer import convert_sync_batchnorm                     # SyncBN conversion reaches the BatchNorm1d where there are any
        assert convert_sync_batchnorm(m) == (0 if inplace_abn else 9) + (2 if norm == "BN" else 0)
    # 'anything else means no norm': the reference compares with 'BN' only
    _, m = _predictor(3, "GN", False)
    assert isinstance(m.trunc_offset_conv[1], torch.nn.Identity)


@pytest.mark.parametrize("k,why", [(0, "1, 3, 5 or 7"), (2, "even"), (4, "even"), (6, "even"), (8, "even"), (9, "above 7"), (11, "above 7")])
def test_refused_windows_name_their_reason(k, why):
    with pytest.raises(NotImplementedError, match=why) as e:
        _predictor(k, "BN", False)
    assert "EDGE_FUSION_KERNEL_SIZE" in str(e.value) and ("1, 3, 5 and 7" in str(e.value) or "1, 3, 5 or 7" in str(e.value))       # ... and what is served


def test_checkpoints_across_the_norm_setting_report_their_keys():
    """A 'BN' checkpoint into a no-norm model and back through the project's checkpointer: the left-over / missing trunc_*_conv.1.* keys are reported
    (Checkpointer.last_load), the rest is loaded, nothing crashes."""
    from monoflex_amd.utils.check_point import Checkpointer
    _, bn = _predictor(5, "BN", False)
    _, no = _predictor(5, "none", True)
    norm_keys = sorted(k for k in bn.state_dict() if k.startswith("trunc_") and ".1." in k)
    assert len(norm_keys) == 10 and not any(".1." in k for k in no.state_dict() if k.startswith("trunc_"))
    with torch.no_grad():
        bn.trunc_offset_conv[0].weight.add_(1.0)
    ck = Checkpointer(no)
    ck._load_model({"model": {k: v.clone() for k, v in bn.state_dict().items()}})
    assert sorted(ck.last_load["unexpected"]) == norm_keys and not ck.last_load["missing"]
    assert torch.equal(no.trunc_offset_conv[0].weight, bn.trunc_offset_conv[0].weight)
    ck = Checkpointer(bn)
    ck._load_model({"model": {k: v.clone() for k, v in no.state_dict().items()}})
    assert sorted(ck.last_load["missing"]) == norm_keys and not ck.last_load["unexpected"]


@pytest.mark.parametrize("L", [1, 2, 3, 4, 9])
def test_rowmap_and_plan_against_a_plain_loop(L):
    from monoflex_amd.model.head.detector_predictor import make_edge_rowmap
    H, W, B = 6, 7, 3
    g = torch.Generator().manual_seed(L)
    ei = torch.stack((torch.randint(0, W, (B, L), generator=g), torch.randint(0, H, (B, L), generator=g)), -1).to(torch.int32)
    el = torch.tensor([L, max(L - 1, 0), 0], dtype=torch.int32)
    assert torch.equal(make_edge_rowmap(ei, H, W), make_edge_rowmap(ei, H, W, halo=1))
    for halo in (0, 1, 2, 3):
        want = EF.rowmap_loop(ei, H, W, halo)
        rm = make_edge_rowmap(ei, H, W, halo)
        assert rm.dtype == torch.int32 and rm.tolist() == want and len(want) == B * (L + 2 * halo)
        _, m = _predictor(2 * halo + 1, "none", False)
        plan = m.edge_plan(ei, el, None, H, W)
        assert plan["rowmap"].dtype == torch.int64 and plan["rowmap"].tolist() == want
        assert plan["rows_center"].tolist() == EF.rowmap_loop(ei, H, W, 0) and plan["rows_center"].is_contiguous()
        assert plan["valid_l"].shape == (B, L, 1) and plan["valid_l"].flatten().tolist() == [float(l < int(el[b])) for b in range(B) for l in range(L)]


@pytest.mark.parametrize("k", [1, 3, 5, 7])
def test_chain_packs_per_window(k):
    """pack_edge_chain at every window: shapes, and test_chain_packs_are_the_five_launches_operands_fragment_major's spot checks -- lane (k-group kq,
    row n) of fragment (nf, k-step ks) holds W[16 nf + n][32 ks + 8 kq .. + 7] of the five launches' [rows][K] matrix, K = (tap, channel)."""
    from monoflex_amd import ops
    for norm in ("BN", "none"):
        _, m = _predictor(k, norm, True)
        m.eval()
        assert m._pack(torch.float32).edge_chain is None and m._pack(ops.F16X2).edge_chain is None
        for dtype in (torch.bfloat16, torch.float16):
            p = m._pack(dtype)
            c = p.edge_chain
            pk1 = p.edge_branches[1][0]
            assert (pk1.kh, pk1.kw, pk1.Ck, pk1.Cout, pk1.K_pad) == (1, k, 256, 256, 256 * k)
            assert c is not None and c.ksize == k and c.relu and c.w_trunk.shape == (32, 18, 4, 16, 8)
            assert c.w_conv.shape == (2, 16, 8 * k, 4, 16, 8) and c.w_conv.dtype == dtype and c.w_out.shape == (2, 1, 8, 4, 16, 8)
            assert c.scale_conv.shape == (2, 256) and c.shift_conv.shape == (2, 256) and c.bias_out.shape == (2, 16)
            for bi in (0, 1):
                packed, w2d = c.w_conv[bi], p.edge_branches[bi][0].w
                for nf, ks, kq, n in ((0, 0, 0, 0), (15, 8 * k - 1, 3, 15), (8, min(5, 8 * k - 1), 2, 7), (3, 8 * (k // 2) + 1, 1, 9)):
                    assert torch.equal(packed[nf, ks, kq, n], w2d[16 * nf + n, 32 * ks + 8 * kq:32 * ks + 8 * kq + 8])
            # K = (tap, channel): column 256 t + c of the matrix is the Conv1d's weight [:, c, t]
            w = m.trunc_offset_conv[0].weight.detach()
            assert torch.equal(pk1.w[:256].view(256, k, 256), w.permute(0, 2, 1).to(dtype))
            if norm == "none":
                assert torch.equal(c.scale_conv, torch.ones(2, 256)) and torch.equal(c.shift_conv[1], m.trunc_offset_conv[0].bias.detach())
                assert torch.equal(c.shift_conv[0], m.trunc_heatmap_conv[0].bias.detach())
            else:
                s, t = ops.fold_bn(m.trunc_offset_conv[1], m.trunc_offset_conv[0].bias)
                assert torch.equal(c.scale_conv[1], s) and torch.equal(c.shift_conv[1], t) and not torch.equal(s, torch.ones(256))


def test_fold_without_a_norm():
    from monoflex_amd import ops
    b = torch.randn(8)
    for bn in (None, torch.nn.Identity(), torch.nn.Identity(256, momentum=0.1)):
        s, t = ops.fold_bn(bn, b)
        assert torch.equal(s, torch.ones(8)) and torch.equal(t, b)
    with pytest.raises(ValueError):
        ops.fold_bn(None)


def test_ks_entry_rejects_bad_arguments_before_any_device_work():
    """mfx_edge_chain_ks on a machine without a GPU: null pointers, unserved windows and bad sizes come back as a code and a message (nothing is
    launched, no pointer is followed), L = 0 is done, the counter does not move, and mfx_edge_chain_ks_applies follows the "edge_chain" switch."""
    from monoflex_amd import lib as L
    lib = L.load()
    c0 = lib.mfx_get_counter(b"edge_chain")
    assert lib.mfx_edge_chain_ks(None, L.ACT_LEAKY, None) == -1 and b"null pointer" in lib.mfx_last_error()
    assert lib.mfx_edge_chain_ks_applies(None) == 0
    d = L.EdgeChainDesc()
    d.B, d.H, d.W, d.C, d.L, d.head_conv, d.ksize, d.relu, d.dtype = 2, 24, 40, 64, 128, 256, 5, 1, L.MFX_BF16
    assert lib.mfx_edge_chain_ks(ctypes.byref(d), L.ACT_LEAKY, None) == -1 and b"null pointer" in lib.mfx_last_error()
    buf = (ctypes.c_char * 64)()
    names = ("x", "edge_xy", "w_trunk", "scale_trunk", "shift_trunk", "w_conv", "scale_conv", "shift_conv", "w_out", "bias_out", "out")
    for n in names:
        setattr(d, n, ctypes.addressof(buf))
    for n in names:                                            # each pointer on its own
        setattr(d, n, None)
        assert lib.mfx_edge_chain_ks(ctypes.byref(d), L.ACT_RELU, None) == -1 and b"null pointer" in lib.mfx_last_error(), n
        setattr(d, n, ctypes.addressof(buf))
    for k in (1, 3, 5, 7):
        d.ksize = k
        assert lib.mfx_edge_chain_ks_applies(ctypes.byref(d)) == 1
        assert lib.mfx_edge_chain_applies(ctypes.byref(d)) == (1 if k == 3 else 0)          # the old entries keep their one window
    for k in (0, 2, 4, 6, 8, 9, -1, -3):
        d.ksize = k
        assert lib.mfx_edge_chain_ks(ctypes.byref(d), L.ACT_LEAKY, None) == -2 and b"1, 3, 5 or 7" in lib.mfx_last_error(), k
        assert lib.mfx_edge_chain_ks_applies(ctypes.byref(d)) == 0
    d.ksize = 5
    for field, value, code in (("dtype", L.MFX_F32, -2), ("dtype", L.MFX_F16X2, -2), ("C", 128, -2), ("head_conv", 128, -2),
                               ("B", 0, -1), ("B", -2, -1), ("L", -1, -1), ("H", 0, -1), ("W", 0, -1), ("B", 65536, -2)):
        keep = getattr(d, field)
        setattr(d, field, value)
        assert lib.mfx_edge_chain_ks(ctypes.byref(d), L.ACT_LEAKY, None) == code and lib.mfx_last_error(), field
        if code == -2 and field != "B":
            assert lib.mfx_edge_chain_ks_applies(ctypes.byref(d)) == 0
        setattr(d, field, keep)
    assert lib.mfx_edge_chain_ks(ctypes.byref(d), L.ACT_NONE, None) == -2 and b"activation" in lib.mfx_last_error()
    d.L = 0
    assert lib.mfx_edge_chain_ks(ctypes.byref(d), L.ACT_LEAKY, None) == 0            # nothing to do, nothing launched
    d.L = 128
    try:
        assert lib.mfx_set_option(b"edge_chain", 0) == 0 and lib.mfx_edge_chain_ks_applies(ctypes.byref(d)) == 0
    finally:
        assert lib.mfx_reset_options() == 0
    assert lib.mfx_edge_chain_ks_applies(ctypes.byref(d)) == 1
    assert lib.mfx_get_counter(b"edge_chain") == c0
