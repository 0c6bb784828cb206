"""mfx_dcn_module_group / ops.dcn_module_group: several same-shape DCN modules (offset/mask conv + gather kernel) as one grouped
offset-conv launch and one grouped gather launch, against the launches they replace.

The grouped kernels run the one-module kernels' loaders, main loop and epilogue on a (module, tile) index taken from blockIdx.x, so
every comparison here is torch.equal -- there is no tolerance to choose.

What the tests pin besides `dcn_group`:
  * The shapes are the smallest at which the grouped index math can go wrong (a partial last tile right before the next module's
    first, tiles spanning image rows, both N-tile widths).  Maps that small are not gather-kernel work in production: ops.dcn_module
    sends them to project-then-sample (ops.DCN_PS) and mfx_dcn_nhwc runs them split-K (another K order), and the grouped entry refuses
    both.  The tests therefore switch project-then-sample off and set dcn_ksplit = 1 -- for the grouped AND the separate launches, so
    the reference is still n separate ops.dcn_module calls on the same kernel family.  test_group_is_refused_* checks the refusals.
"""
import pytest
import torch

pytestmark = pytest.mark.gpu
DEV = "cuda"
DTYPES = {"bf16": torch.bfloat16, "fp16": torch.float16}


@pytest.fixture(autouse=True)
def _gather_kernel_only():
    from monoflex_amd import ops
    was = ops.DCN_PS[0]
    ops.DCN_PS[0] = False
    yield
    ops.DCN_PS[0] = was


def _counter(name="dcn_group"):
    from monoflex_amd import lib as L
    return int(L.load().mfx_get_counter(name.encode()))


def _modules(n, B, C, Co, H, W, tdt, seed):
    """n DCN modules with distinct random inputs, offset convs (offsets of sigma ~ 3 px: border and outside-image corners occur on
    every shape used here), weights and BN folds."""
    from monoflex_amd import lib as L, ops
    g = torch.Generator().manual_seed(seed)
    xs, p_offs, ps = [], [], []
    for _ in range(n):
        x = torch.randn(B, H, W, C, generator=g).relu()
        # sum over 9 C taps of relu(N(0,1)) (second moment 1/2) times w: std 3 px needs w of std 3 / sqrt(4.5 C)
        wo = torch.randn(27, C, 3, 3, generator=g) * (3.0 / (4.5 * C) ** 0.5)
        bo = torch.randn(27, generator=g) * 0.5
        w = torch.randn(Co, C, 3, 3, generator=g) / (3 * C ** 0.5)
        scale, shift = torch.rand(Co, generator=g) + 0.5, torch.randn(Co, generator=g) * 0.2
        p_offs.append(ops.add_f16_fragments(ops.pack_conv(wo.to(DEV), tdt, None, bo.to(DEV), stride=1, pad=1, act=L.ACT_DCN_OFFMASK, cout=32), wo.to(DEV)))
        ps.append(ops.add_f16_fragments(ops.pack_conv(w.to(DEV), tdt, scale.to(DEV), shift.to(DEV), stride=1, pad=1, act=L.ACT_RELU), w.to(DEV)))
        xs.append(x.to(tdt).to(DEV))
    return xs, p_offs, ps


def _separate(xs, p_offs, ps):
    from monoflex_amd import ops
    outs = [ops.dcn_module(x, q, p) for x, q, p in zip(xs, p_offs, ps)]
    return [o[0] for o in outs], [o[1] for o in outs]


# (B, C, Cout, H, W, gather tiles to force (0 = the dispatcher's own choice; 4 = 64x64, 6 = 64x128))
SHAPES = [
    (1, 128, 64, 5, 7, (0,)),           # M = 35: less than one pixel tile; module g's only (partial) workgroup sits right before module g + 1's
    (2, 128, 64, 9, 16, (0,)),          # M = 288: 4.5 tiles of 64
    (2, 256, 128, 6, 10, (0, 4, 6)),    # M = 120: two pixel tiles; N = 128 on the 64x64 tile (tiles_n = 2) and on the 64x128 tile
    (1, 256, 128, 3, 40, (0,)),         # a tile spanning image rows
]


@pytest.mark.parametrize("dt", ["bf16", "fp16"])
@pytest.mark.parametrize("n", [1, 2, 3])
@pytest.mark.parametrize("B,C,Co,H,W,tiles", SHAPES)
def test_grouped_launch_equals_separate_launches(B, C, Co, H, W, tiles, n, dt):
    from monoflex_amd import lib as L, ops
    xs, p_offs, ps = _modules(n, B, C, Co, H, W, DTYPES[dt], seed=1000 + 7 * n + H)
    for tile in tiles:
        L.set_options({"dcn_ksplit": 1, "dcn_tile": tile})
        want_y, want_om = _separate(xs, p_offs, ps)
        c0 = _counter()
        got_y, got_om = ops.dcn_module_group(xs, p_offs, ps)
        torch.cuda.synchronize()
        assert _counter() == c0 + 1, "the group did not run as a group (tile %d)" % tile
        off = torch.cat([o[..., :18].flatten() for o in want_om])
        assert 2.0 < float(off.std()) < 4.5, float(off.std())               # the offsets the docstring promises
        for i in range(n):
            assert torch.equal(got_om[i], want_om[i]), (tile, i, "offset/mask map")
            assert torch.equal(got_y[i], want_y[i]), (tile, i, "output")
        assert len({float(y.float().abs().sum()) for y in got_y}) == n      # distinct modules: no output is another module's


def test_border_and_outside_corners_occur():
    """The sigma = 3 px offsets put samples on the border rows / columns and outside the image on the smallest shape."""
    xs, p_offs, ps = _modules(2, 1, 128, 64, 5, 7, torch.bfloat16, seed=5)
    _, oms = _separate(xs, p_offs, ps)
    om = oms[0].float().cpu()
    H, W = 5, 7
    oh = torch.arange(H).view(1, H, 1, 1).float()
    ow = torch.arange(W).view(1, 1, W, 1).float()
    th = (torch.arange(9) // 3 - 1).view(1, 1, 1, 9).float()
    tw = (torch.arange(9) % 3 - 1).view(1, 1, 1, 9).float()
    h, w = oh + th + om[..., 0:18:2], ow + tw + om[..., 1:18:2]
    outside = (h <= -1) | (w <= -1) | (h >= H) | (w >= W)
    border = ~outside & ((h < 0) | (w < 0) | (h > H - 1) | (w > W - 1))
    assert int(outside.sum()) > 0 and int(border.sum()) > 0 and int((~outside & ~border).sum()) > 0


@pytest.mark.parametrize("dt", ["bf16", "fp16"])
def test_mismatched_shapes_are_refused_and_fall_back(dt):
    """Modules that differ in a size: nothing grouped is launched, the separate launches give the same tensors."""
    from monoflex_amd import lib as L, ops
    tdt = DTYPES[dt]
    L.set_options({"dcn_ksplit": 1})
    a = _modules(1, 2, 128, 64, 9, 16, tdt, seed=11)
    for other in ((2, 128, 64, 9, 8), (2, 256, 64, 9, 16), (2, 128, 128, 9, 16), (1, 128, 64, 9, 16)):      # W, Cin, Cout, B differ
        b = _modules(1, *other, tdt, seed=12)
        xs, p_offs, ps = a[0] + b[0], a[1] + b[1], a[2] + b[2]
        want_y, want_om = _separate(xs, p_offs, ps)
        c0 = _counter()
        got_y, got_om = ops.dcn_module_group(xs, p_offs, ps)
        torch.cuda.synchronize()
        assert _counter() == c0, other
        for i in range(2):
            assert torch.equal(got_y[i], want_y[i]) and torch.equal(got_om[i], want_om[i]), (other, i)


def test_group_is_refused_where_a_module_alone_is_not_plain_gather_work():
    """Option 0, a map small enough that the module alone runs split-K (default dcn_ksplit), a project-then-sample layer, fp32 maps, and a
    64 -> 64 layer (the LDS kernel forced on it; its 64-channel offset conv has no grouped form either): each is refused, the fall-back
    equals the separate launches."""
    from monoflex_amd import lib as L, ops
    xs, p_offs, ps = _modules(2, 2, 256, 128, 6, 10, torch.bfloat16, seed=21)

    def refused(opts, mods=(xs, p_offs, ps)):
        L.load().mfx_reset_options()
        L.set_options(opts)
        want_y, want_om = _separate(*mods)
        c0 = _counter()
        got_y, got_om = ops.dcn_module_group(*mods)
        torch.cuda.synchronize()
        assert _counter() == c0, opts
        for i in range(len(want_y)):
            assert torch.equal(got_y[i], want_y[i]), (opts, i)
            assert (got_om[i] is None and want_om[i] is None) or torch.equal(got_om[i], want_om[i]), (opts, i)

    refused({"dcn_group": 0, "dcn_ksplit": 1})
    refused({})                                                   # default dcn_ksplit: M = 120 runs split-K alone
    ops.DCN_PS[0] = True                                          # (the autouse fixture restores it)
    refused({"dcn_ksplit": 1})
    ops.DCN_PS[0] = False
    refused({"dcn_ksplit": 1}, _modules(2, 2, 128, 64, 9, 16, torch.float32, seed=22))
    refused({"dcn_ksplit": 1, "dcn_lds": 2}, _modules(2, 1, 64, 64, 16, 32, torch.bfloat16, seed=23))


@pytest.fixture(scope="module")
def backbone():
    from monoflex_amd.model.backbone.dla_dcn import DLASeg
    torch.manual_seed(3)
    m = DLASeg("dla34", pretrained=False, down_ratio=4, last_level=5).eval()
    g = torch.Generator().manual_seed(4)
    for mod in m.modules():                                       # offset convs are zero-initialised: give them offsets worth sampling
        if hasattr(mod, "conv_offset_mask"):
            mod.conv_offset_mask.weight.data.normal_(0.0, 0.02, generator=g)
            mod.conv_offset_mask.bias.data.normal_(0.0, 0.5, generator=g)
        if isinstance(mod, torch.nn.BatchNorm2d):
            mod.running_mean.normal_(0.0, 0.1, generator=g)
            mod.running_var.uniform_(0.5, 1.5, generator=g)
    images = torch.randn(1, 3, 64, 128, generator=g)
    return m.to(DEV), images.to(DEV)


@pytest.mark.parametrize("dt", ["bf16", "fp16"])
def test_whole_backbone_grouped_equals_ungrouped(backbone, dt):
    """forward_nhwc on a 1x3x64x128 image with dcn_group 1 and 0: equal outputs; with 1 the two groups of the network (dla_up.ida_1: two
    256 -> 128 modules, dla_up.ida_2: three 128 -> 64) ran grouped, with 0 none."""
    from monoflex_amd import lib as L
    m, images = backbone
    m.compute_dtype = DTYPES[dt]
    outs, counts = {}, {}
    with torch.no_grad():
        for grp in (1, 0):
            L.set_options({"dcn_group": grp, "dcn_ksplit": 1})
            c0, g0 = _counter(), _counter("dcn_gather")
            outs[grp] = m.forward_nhwc(images).clone()
            torch.cuda.synchronize()
            counts[grp] = (_counter() - c0, _counter("dcn_gather") - g0)
    assert counts[1][0] == 2 and counts[0][0] == 0, counts
    assert counts[0][1] - counts[1][1] == 5, counts               # the five grouped modules are the ones that left the one-module gather launches
    assert outs[1].dtype == DTYPES[dt] and bool(torch.isfinite(outs[1].float()).all())
    assert torch.equal(outs[1], outs[0])
