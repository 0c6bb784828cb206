"""tests/edge_chain_ref.py -- the float64 yardstick of tests/test_gpu_edge_chain.py -- against the oracle Predictor's own edge-fusion output, so that
the yardstick itself is pinned without a GPU."""
import torch

from edge_chain_ref import D64, chain_operands, edge_chain_ref


def _oracle(seed, relu):
    from monoflex_amd import synthetic as S
    from oracle import monoflex_ref as R
    ref = R.Predictor().eval()
    sd = S.synthetic_state_dict({"heads.predictor." + k: v for k, v in ref.state_dict().items()}, seed=seed)
    ref.load_state_dict({k[len("heads.predictor."):]: v for k, v in sd.items()})
    if relu:
        ref.trunc_heatmap_conv[2], ref.trunc_offset_conv[2] = torch.nn.ReLU(), torch.nn.ReLU()
    return ref.double()


def _check(relu, lens):
    from monoflex_amd import synthetic as S
    ref = _oracle(3, relu)
    tgt = S.synthetic_target(40, 24)
    B = len(lens)
    x = torch.randn(B, 64, 24, 40, generator=torch.Generator().manual_seed(9), dtype=D64).relu()
    ei = torch.stack([tgt["edge_indices"]] * B)
    taps = {}
    with torch.no_grad():
        ref(x, ei, torch.tensor(lens), taps)
        got = edge_chain_ref(x, ei, chain_operands(ref))
    assert ei.shape[1] == 128 and tgt["edge_len"] == 120
    for g, want in zip(got, (taps["edge_cls"], taps["edge_off"])):
        assert g.shape == want.shape and g.dtype == D64
        # the oracle samples with grid_sample at integer points through normalised coordinates: exact up to float64 rounding of the coordinates
        assert float((g - want).abs().max()) <= 1e-10 * max(1.0, float(want.abs().max()))
    return got


def test_reference_equals_the_oracle_predictor():
    got = _check(False, [120, 120])
    assert got[0].shape == (2, 3, 128) and got[1].shape == (2, 2, 128)
    assert float(got[0].abs().max()) > 1e-2 and float(got[1].abs().max()) > 1e-2


def test_reference_equals_the_oracle_predictor_with_relu():
    _check(True, [120, 37])


def test_operand_rounding_is_applied_to_weights_only():
    ref = _oracle(3, False)
    a, b = chain_operands(ref), chain_operands(ref, torch.bfloat16)
    for pa, pb in zip(a, b):
        for k in ("w_trunk", "w_conv", "w_out"):
            assert torch.equal(pb[k], pa[k].to(torch.bfloat16).to(D64)) and not torch.equal(pb[k], pa[k])
        for k in ("s_trunk", "t_trunk", "s_conv", "t_conv", "b_out"):
            assert torch.equal(pb[k], pa[k])


def test_entry_rejects_bad_arguments_before_any_device_work():
    """mfx_edge_chain on a machine without a GPU: null pointers and unsupported sizes come back as a code and a message (nothing is launched, no
    pointer is followed); mfx_edge_chain_applies follows the "edge_chain" switch."""
    import ctypes
    from monoflex_amd import lib as L
    lib = L.load()
    c0 = lib.mfx_get_counter(b"edge_chain")
    assert lib.mfx_edge_chain(None, None) == -1 and b"null pointer" in lib.mfx_last_error()
    d = L.EdgeChainDesc()
    d.B, d.H, d.W, d.C, d.L, d.head_conv, d.ksize, d.relu, d.dtype = 2, 24, 40, 64, 128, 256, 3, 1, L.MFX_BF16
    assert lib.mfx_edge_chain(ctypes.byref(d), None) == -1 and b"null pointer" in lib.mfx_last_error()
    buf = (ctypes.c_char * 64)()
    for n in ("x", "edge_xy", "w_trunk", "scale_trunk", "shift_trunk", "w_conv", "scale_conv", "shift_conv", "w_out", "bias_out", "out"):
        setattr(d, n, ctypes.addressof(buf))
    assert lib.mfx_edge_chain_applies(ctypes.byref(d)) == 1 and lib.mfx_edge_chain_applies(None) == 0
    for field, value, code in (("dtype", L.MFX_F32, -2), ("dtype", L.MFX_F16X2, -2), ("C", 128, -2), ("head_conv", 128, -2), ("ksize", 5, -2),
                               ("B", 0, -1), ("L", -1, -1), ("H", 0, -1)):
        keep = getattr(d, field)
        setattr(d, field, value)
        assert lib.mfx_edge_chain(ctypes.byref(d), None) == code and lib.mfx_last_error(), field
        if code == -2:
            assert lib.mfx_edge_chain_applies(ctypes.byref(d)) == 0
        setattr(d, field, keep)
    try:
        assert lib.mfx_set_option(b"edge_chain", 0) == 0 and lib.mfx_edge_chain_applies(ctypes.byref(d)) == 0
    finally:
        assert lib.mfx_reset_options() == 0
    assert lib.mfx_edge_chain_applies(ctypes.byref(d)) == 1
    assert lib.mfx_get_counter(b"edge_chain") == c0


def test_ctypes_mirror_matches_the_header(tmp_path):
    """mfx_edge_chain_desc as gcc lays it out against lib.EdgeChainDesc: size and the offset of every member."""
    import ctypes
    import os
    import subprocess
    from monoflex_amd import lib as L
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    names = [n for n, _ in L.EdgeChainDesc._fields_]
    src = tmp_path / "layout.c"
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "%s"\nint main(void) {\nprintf("%%zu\\n", sizeof(mfx_edge_chain_desc));\n%s\nreturn 0; }\n'
                   % (os.path.join(root, "include", "monoflex_hip.h"),
                      "\n".join('printf("%%zu\\n", offsetof(mfx_edge_chain_desc, %s));' % n for n in names)))
    exe = str(tmp_path / "layout")
    r = subprocess.run(["gcc", "-std=c99", "-o", exe, str(src)], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    out = [int(v) for v in subprocess.run([exe], capture_output=True, text=True).stdout.split()]
    assert out[0] == ctypes.sizeof(L.EdgeChainDesc)
    assert out[1:] == [getattr(L.EdgeChainDesc, n).offset for n in names]


def test_chain_packs_are_the_five_launches_operands_fragment_major():
    """pack_edge_chain: the same matrices the five launches multiply ([rows][K], K = (tap, channel)), lane (k-group kq, row n) of fragment
    (nf, k-step ks) holding W[16 nf + n][32 ks + 8 kq .. + 7]; None for fp32 and for split precision."""
    import os
    from monoflex_amd import ops
    from monoflex_amd.config import get_cfg
    from monoflex_amd.model.head.detector_predictor import _predictor
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    m = _predictor(get_cfg(os.path.join(root, "runs", "monoflex.yaml"), ["MODEL.HEAD.EDGE_FUSION_RELU", True]), 64).eval()
    assert m._pack(torch.float32).edge_chain is None and m._pack(ops.F16X2).edge_chain is None
    for dtype in (torch.bfloat16, torch.float16):
        p = m._pack(dtype)
        c = p.edge_chain
        assert c.relu and c.w_trunk.dtype == dtype and c.w_trunk.shape == (32, 18, 4, 16, 8)
        assert c.w_conv.shape == (2, 16, 24, 4, 16, 8) and c.w_out.shape == (2, 1, 8, 4, 16, 8)
        assert c.scale_trunk.shape == (512,) and c.scale_conv.shape == (2, 256) and c.bias_out.shape == (2, 16)
        for packed, w2d in ((c.w_trunk, p.edge_trunk.w), (c.w_conv[1], p.edge_branches[1][0].w), (c.w_out[0], p.edge_branches[0][1].w)):
            for nf, ks, kq, n in ((0, 0, 0, 0), (packed.shape[0] - 1, packed.shape[1] - 1, 3, 15), (packed.shape[0] // 2, 5, 2, 7)):
                assert torch.equal(packed[nf, ks, kq, n], w2d[16 * nf + n, 32 * ks + 8 * kq:32 * ks + 8 * kq + 8])
        assert torch.equal(c.bias_out[1, :2], m.trunc_offset_conv[3].bias.detach()) and float(c.bias_out[1, 2:].abs().max()) == 0.0
