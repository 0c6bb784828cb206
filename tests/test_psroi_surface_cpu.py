"""The pooling half of the reference's DCNv2 surface, as far as it can be checked without a GPU: import names, constructor defaults,
parameter names and shapes (reference dcn_v2.py:187-257), the CPU refusal, and the two exported C symbols."""
import ctypes
import os
import subprocess
import sys

import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_reference_import_line_resolves_from_the_repository_root():
    """testcuda.py:12 of the reference, through the root alias package."""
    code = ("from model.backbone.DCNv2.dcn_v2 import dcn_v2_pooling, DCNv2Pooling, DCNPooling\n"
            "from model.backbone.DCNv2.dcn_v2 import dcn_v2_conv, DCNv2, DCN\n"
            "import monoflex_amd.model.backbone.DCNv2.dcn_v2 as real\n"
            "assert DCNPooling is real.DCNPooling and DCNv2Pooling is real.DCNv2Pooling and dcn_v2_pooling is real.dcn_v2_pooling\n"
            "assert issubclass(DCNPooling, DCNv2Pooling)\n")
    r = subprocess.run([sys.executable, "-c", code], cwd=ROOT, capture_output=True, text=True)
    assert r.returncode == 0, r.stderr


def test_constructor_defaults():
    from monoflex_amd.model.backbone.DCNv2.dcn_v2 import DCNPooling, DCNv2Pooling
    p = DCNv2Pooling(0.25, 7, 16, True)
    assert (p.spatial_scale, p.pooled_size, p.output_dim, p.no_trans) == (0.25, 7, 16, True)
    assert (p.group_size, p.part_size, p.sample_per_part, p.trans_std) == (1, 7, 4, 0.0)          # part_size=None -> pooled_size
    assert DCNv2Pooling(0.25, 7, 16, False, part_size=3).part_size == 3
    q = DCNPooling(spatial_scale=0.25, pooled_size=5, output_dim=8, no_trans=False)
    assert (q.group_size, q.part_size, q.sample_per_part, q.trans_std, q.deform_fc_dim) == (1, 5, 4, 0.0, 1024)
    assert list(DCNv2Pooling(0.25, 7, 16, False).parameters()) == []
    plain = DCNPooling(0.25, 7, 16, no_trans=True)
    assert list(plain.parameters()) == [] and not hasattr(plain, "offset_mask_fc")


def test_dcnpooling_state_dict_keys_and_shapes():
    from monoflex_amd.model.backbone.DCNv2.dcn_v2 import DCNPooling
    m = DCNPooling(spatial_scale=0.25, pooled_size=7, output_dim=32, no_trans=False, group_size=1, trans_std=0.1, deform_fc_dim=256)
    want = [("offset_mask_fc.0.weight", (256, 7 * 7 * 32)), ("offset_mask_fc.0.bias", (256,)),
            ("offset_mask_fc.2.weight", (256, 256)), ("offset_mask_fc.2.bias", (256,)),
            ("offset_mask_fc.4.weight", (7 * 7 * 3, 256)), ("offset_mask_fc.4.bias", (7 * 7 * 3,))]
    got = [(k, tuple(v.shape)) for k, v in m.state_dict().items()]
    assert got == want
    sd = m.state_dict()
    assert float(sd["offset_mask_fc.4.weight"].abs().max()) == 0.0 and float(sd["offset_mask_fc.4.bias"].abs().max()) == 0.0
    assert float(sd["offset_mask_fc.0.weight"].abs().max()) > 0.0
    assert isinstance(m.offset_mask_fc[1], torch.nn.ReLU) and isinstance(m.offset_mask_fc[3], torch.nn.ReLU)


def test_cpu_tensors_are_refused():
    from monoflex_amd.model.backbone.DCNv2 import _ext
    from monoflex_amd.model.backbone.DCNv2.dcn_v2 import DCNPooling, DCNv2Pooling
    x = torch.zeros(1, 4, 8, 8)
    rois = torch.tensor([[0.0, 0, 0, 16, 16]])
    with pytest.raises(RuntimeError, match="no CPU"):
        DCNv2Pooling(0.25, 3, 4, True)(x, rois, x.new())
    with pytest.raises(RuntimeError, match="no CPU"):
        DCNPooling(0.25, 3, 4, False, deform_fc_dim=8)(x, rois)
    with pytest.raises(RuntimeError, match="no CPU"):
        _ext.dcn_v2_psroi_pooling_forward(x, rois, torch.zeros(1, 2, 3, 3), 0, 0.25, 4, 1, 3, 3, 4, 0.1)
    with pytest.raises(RuntimeError, match="no CPU"):
        _ext.dcn_v2_psroi_pooling_backward(torch.zeros(1, 4, 3, 3), x, rois, torch.zeros(1, 2, 3, 3), torch.zeros(1, 4, 3, 3), 0, 0.25, 4, 1, 3, 3, 4, 0.1)
    with pytest.raises(AssertionError):                              # dcn_v2.py:209
        DCNv2Pooling(0.25, 3, 5, True)(x, rois, x.new())
    assert "not supported" not in open(os.path.join(ROOT, "monoflex_amd", "model", "backbone", "DCNv2", "_ext.py")).read()


def test_the_two_symbols_are_exported_and_check_their_arguments():
    """ctypes.CDLL loads without a GPU; argument errors are reported before any device work."""
    from monoflex_amd import build, lib as L
    cdll = ctypes.CDLL(build.build_lib())
    for name in ("mfx_dcn_v2_psroi_pooling_forward", "mfx_dcn_v2_psroi_pooling_backward"):
        assert hasattr(cdll, name) and name in L.SYMBOLS
    lib = L.load()
    null = ctypes.c_void_p(None)
    fwd = lambda C, od, gs, S=4: lib.mfx_dcn_v2_psroi_pooling_forward(null, null, null, null, null, 2, C, 8, 8, 3, 3, 2, 0, 0.25, od, gs, 3, 3, S, 0.1, null)
    assert fwd(4, 6, 1) == -1 and b"input channels and output channels must equal" in lib.mfx_last_error()          # MFX_ERR_ARG
    assert fwd(4, 4, 2) == -2 and b"group_size must be 1" in lib.mfx_last_error()                                   # MFX_ERR_UNSUPPORTED
    assert fwd(4, 4, 1, 33) == -2 and b"sample_per_part" in lib.mfx_last_error()
    bwd = lib.mfx_dcn_v2_psroi_pooling_backward(null, null, null, null, null, null, null, 2, 4, 8, 8, 3, 3, 2, 0, 0.25, 4, 2, 3, 3, 4, 0.1, null)
    assert bwd == -2 and b"group_size must be 1" in lib.mfx_last_error()
    # N == 0: MFX_OK without a launch (no device is touched in this process)
    assert lib.mfx_dcn_v2_psroi_pooling_forward(null, null, null, null, null, 2, 4, 8, 8, 0, 0, 2, 0, 0.25, 4, 1, 3, 3, 4, 0.1, null) == 0
