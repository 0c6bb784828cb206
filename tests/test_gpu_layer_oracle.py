"""Layer-by-layer oracle walk of the benchmarked inference step (bench.py: B = 8, 1280x384, bench.build_model / bench.bench_images).

One eager `detect_device` per mode runs with every `ops` entry point the model calls wrapped: each top-level call is compared, on its own
recorded inputs upcast to float64, with a plain float64 restatement of the layer built from the owning nn.Module's own fp32 parameters (conv
weights, BN running statistics, DCN weights and bias, up-sampling taps) -- never from the library's packs.  The float64 work runs as plain torch
ops on the GPU (no library kernel in any reference).  The library's dispatch counters (mfx_get_counter) tell which kernel family each call ran.

Error model (as tests/test_gpu_bf16_kernels_vs_oracle.py): fp32 accumulation, one rounding of the output to the activation type (2^-9 bf16,
2^-11 fp16); the weights of the 16-bit modes are rounded to the operand type as well, which the float64 reference does not do.  Bounds are
~2x the values observed on MI355X (layer_oracle_<mode>.json, written to $MFX_REPORT_DIR, default artifacts/) and never looser than the direct
oracle tests of the same family."""
import json
import os

import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
REPORT_DIR = os.environ.get("MFX_REPORT_DIR") or os.path.join(ROOT, "artifacts")      # where the observed numbers go (artifacts/ is git-ignored)
B = 8
D64 = torch.float64

# (conv max, conv mean, DCN max, DCN mean): bf16 = the direct tests' bounds, fp16 = x0.125 / x0.22 of them, fp16x2 = fp32 grade
# (fp16x2 observed on MI355X: conv 1.5e-6 / 5.3e-7, DCN 8.7e-6 / 1.7e-6)
BOUNDS = {"bf16": (6e-3, 2.9e-3, 7.5e-3, 4.5e-3), "fp16": (6e-3 * 0.125, 2.9e-3 * 0.125, 7.5e-3 * 0.22, 4.5e-3 * 0.22),
          "fp16x2": (4e-6, 1.2e-6, 2e-5, 4e-6)}
# |offset or mask error| <= bound * max(1, |value|); observed 4.3e-6 bf16, 6.3e-6 fp16, 9.1e-6 fp16x2 (the operands are exact: fp32 sums only)
OFF_BOUND = {"bf16": 1.5e-5, "fp16": 1.5e-5, "fp16x2": 2e-5}
DCN64_SCALE = 1.5                                                  # (c): the all-float64 module (reference offsets) vs the kernel; observed = (b)
# (max, mean); observed bf16 2.6e-3 / 1.5e-3, fp16 3.2e-4 / 1.9e-4, fp16x2 5.7e-7 / 3.0e-7 (test_heads_fused_vs_torch: 5e-2)
HEADS_BOUND = {"bf16": (5e-3, 3e-3), "fp16": (6.5e-4, 4e-4), "fp16x2": (1.2e-6, 6e-7)}
WRAPPED = ("conv2d", "cat_conv1x1", "dcn_module", "dcn", "dcn_ps", "maxpool2x2", "upsample_add", "f1_fused", "heads_fused",
           "edge_scatter_add", "decode_topk", "decode_boxes")
COUNTERS = ("dcn_lds", "dcn_lds_of", "dcn_lds_split", "dcn_patch", "dcn_wave", "dcn_gather",
            "conv_cw", "conv_cws", "conv_halo", "conv_igemm", "conv_splitk")
OP_FAMILY = {"cat_conv1x1": "cat_igemm", "maxpool2x2": "maxpool", "upsample_add": "upsample_add", "f1_fused": "f1_fused",
             "heads_fused": "heads_fused", "edge_scatter_add": "edge_scatter_add", "decode_topk": "decode", "decode_boxes": "decode"}
# kernel families of the B = 8 step, from the dispatch code (ops.dcn_module / dcn_ps_applies, mfx_dcn_nhwc, try_conv_halo, mfx_conv2d_nhwc):
# exactly these run -- a change of the benchmark's dispatch has to update this table on purpose
FAMILIES = {
    "bf16": {"dcn_lds", "dcn_lds_of", "dcn_gather", "dcn_wave", "project_as", "dcn_sample", "conv_cw", "conv_igemm", "cat_igemm",
             "f1_fused", "heads_fused", "upsample_add", "maxpool", "edge_scatter_add", "decode"},
}
FAMILIES["fp16"] = set(FAMILIES["bf16"])
FAMILIES["fp16x2"] = {"dcn_lds_split", "dcn_gather", "dcn_wave", "conv_cws", "conv_halo", "conv_igemm", "cat_igemm", "f1_fused", "heads_fused",
                      "upsample_add", "maxpool", "edge_scatter_add", "decode"}


def _counters(lib):
    return {n: int(lib.mfx_get_counter(n.encode())) for n in COUNTERS}


def _nchw64(t):
    return t.permute(0, 3, 1, 2).to(D64)


def _nhwc(t):
    return t.permute(0, 2, 3, 1)


def _fold64(bn, bias=None):
    scale = bn.weight.detach().to(D64) / torch.sqrt(bn.running_var.detach().to(D64) + bn.eps)
    shift = bn.bias.detach().to(D64) - bn.running_mean.detach().to(D64) * scale
    if bias is not None:
        shift = shift + bias.detach().to(D64) * scale
    return scale, shift


def _aff(z, scale, shift, res=None, relu=True):
    z = z * scale.view(1, -1, 1, 1) + shift.view(1, -1, 1, 1)
    if res is not None:
        z = z + res
    return F.relu(z) if relu else z


def _metrics(got, ref):
    """got / ref (B,C,H,W) float64: per image max-rel, mean-rel, the same on the border band (outer 2 rows and columns), and the worst channel's
    mean error relative to its own mean |ref| (at least the image's); returns the worst of each over the batch."""
    d = (got - ref).abs()
    H, W = ref.shape[2], ref.shape[3]
    band = torch.zeros(H, W, dtype=torch.bool, device=ref.device)
    band[:2], band[-2:], band[:, :2], band[:, -2:] = True, True, True, True
    out = dict(max_rel=0.0, mean_rel=0.0, border_max_rel=0.0, border_mean_rel=0.0, chan_mean_rel=0.0)
    for b in range(ref.shape[0]):
        db, rb = d[b], ref[b].abs()
        top, mean = max(1.0, float(rb.max())), max(1e-6, float(rb.mean()))
        out["max_rel"] = max(out["max_rel"], float(db.max()) / top)
        out["mean_rel"] = max(out["mean_rel"], float(db.mean()) / mean)
        out["border_max_rel"] = max(out["border_max_rel"], float(db[:, band].max()) / top)
        out["border_mean_rel"] = max(out["border_mean_rel"], float(db[:, band].mean()) / mean)
        out["chan_mean_rel"] = max(out["chan_mean_rel"], float((db.mean(dim=(1, 2)) / rb.mean(dim=(1, 2)).clamp(min=mean)).max()))
    return out


def _check(rec, name, m, bmax, bmean):
    rec.append((name, m, bmax, bmean))
    ok = (m["max_rel"] <= bmax and m["mean_rel"] <= bmean and m["border_max_rel"] <= bmax and m["border_mean_rel"] <= 2 * bmean
          and m["chan_mean_rel"] <= 3 * bmean)
    return ok


def _dcn64(x, off, msk, w, pad=1):
    """Modulated deformable 3x3 / stride 1 in float64 with torch's grid_sample as the sampler (oracle/dcn_ref.dcn_v2_grid_sample on the device)."""
    Bn, C, H, W = x.shape
    ys, xs = torch.meshgrid(torch.arange(H, dtype=D64, device=x.device), torch.arange(W, dtype=D64, device=x.device), indexing="ij")
    out = torch.zeros(Bn, w.shape[0], H, W, dtype=D64, device=x.device)
    for k in range(9):
        i, j = divmod(k, 3)
        py = ys + (i - pad) + off[:, 2 * k]
        px = xs + (j - pad) + off[:, 2 * k + 1]
        grid = torch.stack((2 * px / (W - 1) - 1, 2 * py / (H - 1) - 1), dim=-1)
        smp = F.grid_sample(x, grid, mode="bilinear", padding_mode="zeros", align_corners=True) * msk[:, k:k + 1]
        out = out + torch.einsum("oc,bchw->bohw", w[:, :, i, j], smp)
    return out


def _offmask64(dcn, x64, wr):
    c = dcn.conv_offset_mask
    om = F.conv2d(x64, wr(c.weight), c.bias.detach().to(D64), 1, 1)
    return om[:, :18], torch.sigmoid(om[:, 18:27])


def _halo_from_previous_image(x64, w64, stride, pad):
    """Deliberately wrong convolution: the images of the batch stacked into one tall map, so image b's top halo row is image b-1's last row."""
    Bn, C, H, W = x64.shape
    tall = x64.permute(1, 0, 2, 3).reshape(1, C, Bn * H, W)
    y = F.conv2d(tall, w64, None, stride, pad)
    return y.view(y.shape[1], Bn, -1, y.shape[3]).permute(1, 0, 2, 3)


class _Walk:
    def __init__(self, mode, model, lib, ops):
        self.mode, self.model, self.lib, self.ops = mode, model, lib, ops
        self.stack, self.depth, self.nested = [], 0, []
        self.rec, self.fail, self.families, self.seen, self.teeth = [], [], set(), {}, []
        cm, cmean, dmax, dmean = BOUNDS[mode]
        self.cb, self.db = (cm, cmean), (dmax, dmean)
        self.rnd = (lambda t: t) if mode == "fp16x2" else (lambda t: t.to(torch.bfloat16 if mode == "bf16" else torch.float16).to(D64))
        # the operands the kernels multiply: the module's fp32 weights rounded to the mode's type (the DCN LDS kernels and the offset conv
        # fused into them take IEEE fp16 weights in bf16 mode as well; split precision keeps fp32 grade)
        self.wr = lambda t: self.rnd(t.detach().to(D64))
        self.wr16 = (lambda t: t.detach().to(D64)) if mode == "fp16x2" else (lambda t: t.detach().to(torch.float16).to(D64))
        self.teeth_done = set()

    def owner(self):
        return self.stack[-1] if self.stack else None

    def see(self, module, what):
        key = (id(module), what)
        self.seen[key] = self.seen.get(key, 0) + 1

    def judge(self, name, m, bounds):
        if not _check(self.rec, name, m, *bounds):
            self.fail.append(name)

    def tooth(self, name, m, key, bound):
        """A deliberately wrong reference: the kernel must miss it by >= 2x the bound of the metric that is meant to catch it."""
        self.teeth.append((name, key, m[key], bound))

    # ---- per-call references --------------------------------------------------------------------------------------------------------
    def conv2d(self, mod, args, kw, y):
        from monoflex_amd.model.backbone import dla_dcn as D
        x, p = args[0], args[1]
        packs = mod.__dict__.get("_packs", {})
        key = next((k for k, v in packs.items() if v is p), None)
        if isinstance(mod, D.BasicBlock) and key is not None:
            conv, bn = (mod.conv1, mod.bn1) if key[0] == "c1" else (mod.conv2, mod.bn2)
            res = kw.get("res")
            relu = True
        elif isinstance(mod, D.Tree) and key is not None and key[0] == "proj":
            conv, bn, res, relu = mod.project[0], mod.project[1], None, False
        else:
            return "other"                                                   # (the Predictor's edge-fusion convs: the Predictor check covers them)
        w64 = self.wr(conv.weight)
        s, t = _fold64(bn)
        x64 = _nchw64(x)
        z = F.conv2d(x64, w64, None, conv.stride[0], conv.padding[0])
        res64 = _nchw64(res) if res is not None else None
        ref = _aff(z, s, t, res64, relu)
        got = _nchw64(y)
        name = "%s.%s" % (self.names[id(mod)], "proj" if key[0] == "proj" else key[0])
        self.judge(name, _metrics(got, ref), self.cb)
        self.see(mod, key[0])
        if res is not None and "conv" not in self.teeth_done:             # one BasicBlock conv2: teeth (i), (ii), (iv)
            self.teeth_done.add("conv")
            c = int(t.abs().argmax())
            t1 = t.clone()
            t1[c] = 0.0
            self.tooth(name + " (i) BN shift of channel %d dropped" % c, _metrics(got, _aff(z, s, t1, res64, relu)), "chan_mean_rel", 3 * self.cb[1])
            zh = _halo_from_previous_image(x64, w64, conv.stride[0], conv.padding[0])
            self.tooth(name + " (ii) halo row from the previous image", _metrics(got, _aff(zh, s, t, res64, relu)), "border_max_rel", self.cb[0])
            self.tooth(name + " (iv) residual omitted", _metrics(got, _aff(z, s, t, None, relu)), "max_rel", self.cb[0])
        return "ok"

    def cat_conv1x1(self, mod, args, kw, y):
        srcs = args[0]
        x64 = torch.cat([_nchw64(s_) for s_ in srcs], 1)
        s, t = _fold64(mod.bn)
        ref = _aff(F.conv2d(x64, self.wr(mod.conv.weight)), s, t)
        self.judge("%s (root)" % self.names[id(mod)], _metrics(_nchw64(y), ref), self.cb)
        self.see(mod, "root")

    def maxpool2x2(self, mod, args, kw, y):
        x = args[0]
        ref = _nhwc(F.max_pool2d(x.permute(0, 3, 1, 2).float(), 2, 2)).to(x.dtype)
        self.rec.append(("%s maxpool" % self.names.get(id(mod), "?"), dict(bit_equal=float(torch.equal(ref, y))), 0.0, 0.0))
        if not torch.equal(ref, y):
            self.fail.append("maxpool")

    def upsample_add(self, mod, args, kw, y):
        x, taps, f = args[0], args[1], args[2]
        skip = kw.get("skip", args[3] if len(args) > 3 else None)
        packs = mod.__dict__.get("_packs", {})
        k = next(k for k, v in packs.items() if v is taps)
        up = getattr(mod, "up_%d" % k)
        C = x.shape[3]
        ref = F.conv_transpose2d(_nchw64(x), up.weight.detach().to(D64), None, f, f // 2, groups=C) + _nchw64(skip)
        self.judge("%s.up_%d" % (self.names[id(mod)], k), _metrics(_nchw64(y), ref), self.cb)
        self.see(mod, "up_%d" % k)

    def f1_fused(self, mod, args, kw, y):
        images = args[0]
        b = mod
        r = self.rnd
        s0, t0 = _fold64(b.base_layer[1])
        s1, t1 = _fold64(b.level0[1])
        s2, t2 = _fold64(b.level1[1])
        z = r(_aff(F.conv2d(r(images.to(D64)), self.wr(b.base_layer[0].weight), None, 1, 3), s0, t0))
        z = r(_aff(F.conv2d(z, self.wr(b.level0[0].weight), None, 1, 1), s1, t1))
        ref = _aff(F.conv2d(z, self.wr(b.level1[0].weight), None, 2, 1), s2, t2)
        self.judge("base.f1 (stem+level0+level1)", _metrics(_nchw64(y), ref), self.cb)
        self.see(mod, "f1")

    def dcn_module(self, mod, args, kw, out):
        x, p_off, p = args[0], args[1], args[2]
        y, om = out
        name = self.names[id(mod)]
        fam = self.cur_families
        if om is None:                                                       # offset conv inside the kernel: ask for its map once more
            self.depth += 1
            try:
                y2, om = self.orig["dcn_module"](x, p_off, p, need_offmask=True)
            finally:
                self.depth -= 1
            torch.cuda.synchronize()
            if not torch.equal(y2, y):
                self.fail.append(name + " (a) y with need_offmask differs")
        dcn, bn = mod.conv, mod.actf[0]
        x64 = _nchw64(x)
        lds = "dcn_lds" in fam
        off_r, msk_r = _offmask64(dcn, x64, self.wr16 if "dcn_lds_of" in fam else self.wr)
        om64 = _nchw64(om)
        off_k, msk_k = om64[:, :18], om64[:, 18:27]
        e_off = float(((off_k - off_r).abs() / off_r.abs().clamp(min=1.0)).max())
        e_msk = float((msk_k - msk_r).abs().max())
        self.rec.append((name + " (a) offsets / mask", dict(off_rel=e_off, mask_abs=e_msk), OFF_BOUND[self.mode], OFF_BOUND[self.mode]))
        if not (e_off <= OFF_BOUND[self.mode] and e_msk <= OFF_BOUND[self.mode]):
            self.fail.append(name + " (a)")
        s, t = _fold64(bn, dcn.bias)
        w = (self.wr16 if lds else self.wr)(dcn.weight)
        got = _nchw64(y)
        ref_b = _aff(_dcn64(x64, off_k, msk_k, w), s, t)
        m = _metrics(got, ref_b)
        self.judge(name + " (b) [%s]" % "+".join(sorted(fam)), m, self.db)
        ref_c = _aff(_dcn64(x64, off_r, msk_r, w), s, t)
        self.judge(name + " (c) all-float64", _metrics(got, ref_c), (self.db[0] * DCN64_SCALE, self.db[1] * DCN64_SCALE))
        self.see(mod, "dcn")
        path = "lds" if ("dcn_lds" in fam or "dcn_lds_split" in fam) else "wave" if "dcn_wave" in fam else "ps" if "dcn_sample" in fam \
            else "gather" if "dcn_gather" in fam else "patch"
        if path not in self.teeth_done:                                      # teeth (i), (iii) once per dispatch path
            self.teeth_done.add(path)
            c = int(t.abs().argmax())
            t1 = t.clone()
            t1[c] = 0.0
            self.tooth(name + " [%s] (i) BN shift of channel %d dropped" % (path, c), _metrics(got, _aff(_dcn64(x64, off_k, msk_k, w), s, t1)),
                       "chan_mean_rel", 3 * self.db[1])
            ref_h = _aff(_dcn64(x64, off_k + torch.tensor([0.5, 0.0], dtype=D64, device=x.device).repeat(9).view(1, 18, 1, 1), msk_k, w), s, t)
            self.tooth(name + " [%s] (iii) sampling half a pixel off" % path, _metrics(got, ref_h), "mean_rel", self.db[1])

    def heads_fused(self, mod, args, kw, out):
        hm = out[0]
        ref = self.pred_ref
        x64 = _nchw64(args[0])
        cls = ref.class_head[-1](ref.class_head[:-1](x64))
        regs = []
        for i, feat in enumerate(ref.reg_features):
            f = feat(x64)
            regs += [h(f) for h in ref.reg_heads[i]]
        from monoflex_amd.model.head.detector_predictor import REG_OFF
        want = torch.cat([cls] + regs, 1)
        got = torch.cat((_nchw64(hm[..., :3]), _nchw64(hm[..., REG_OFF:REG_OFF + 50])), 1)
        m = _metrics(got, want)
        self.judge("heads_fused (before edge fusion)", m, HEADS_BOUND[self.mode])
        c = 0
        w1 = want.clone()
        w1[:, c] -= ref.class_head[-1].bias.detach().to(D64)[c]
        self.tooth("heads_fused (i) class-%d bias dropped" % c, _metrics(got, w1), "chan_mean_rel", 3 * HEADS_BOUND[self.mode][1])


@pytest.fixture(scope="module")
def _lib():
    from monoflex_amd import lib as L
    return L


@pytest.mark.parametrize("mode", ["bf16", "fp16", "fp16x2"])
def test_layer_oracle_walk_of_the_benchmarked_step(mode, monkeypatch, _lib):
    import bench
    from monoflex_amd import ops, synthetic as S
    from monoflex_amd.model.backbone import dla_dcn as D
    from monoflex_amd.model.head.detector_predictor import REG_OFF
    from monoflex_amd.structures.params_3d import make_test_target
    from oracle import monoflex_ref as R
    L = _lib
    lib = L.load()
    dev = torch.device("cuda:0")
    model, _, _ = bench.build_model(mode, dev)
    images = bench.bench_images(B, 0, dev)
    tgts = [S.synthetic_target(320, 96) for _ in range(B)]
    tg = model.device_targets([make_test_target(t) for t in tgts], dev)
    pred = model.heads.predictor
    w = _Walk(mode, model, lib, ops)
    w.names = {id(m): n for n, m in model.named_modules()}
    w.pred_ref = R.Predictor().eval()
    w.pred_ref.load_state_dict({k: (w.wr(v).float() if v.dim() >= 3 else v) for k, v in pred.state_dict().items()})   # conv / conv1d weights
    w.pred_ref = w.pred_ref.to(dev, D64)
    # every model file reaches the operators as `ops.X` (module attribute at call time): no `from ... ops import X` of a wrapped name
    for d_, _, files in os.walk(os.path.join(ROOT, "monoflex_amd")):
        for f in files:
            if f.endswith(".py"):
                src = open(os.path.join(d_, f)).read()
                for line in src.splitlines():
                    if line.lstrip().startswith("from") and "ops import" in line:
                        assert not any(n in line.split("import", 1)[1].replace(",", " ").split() for n in WRAPPED), (f, line)
    w.orig = {n: getattr(ops, n) for n in WRAPPED}

    def wrap(name, fn):
        def run(*args, **kw):
            if w.depth:
                w.nested.append(name)
                return fn(*args, **kw)
            w.depth += 1
            w.nested = []
            torch.cuda.synchronize()
            c0 = _counters(lib)
            try:
                out = fn(*args, **kw)
            finally:
                w.depth -= 1
            torch.cuda.synchronize()
            c1 = _counters(lib)
            fam = {k for k in COUNTERS if c1[k] != c0[k]}
            if name in OP_FAMILY:
                fam.add(OP_FAMILY[name])
            if "dcn_ps" in w.nested:                                     # project (1x1 conv: counted above, or gemm_as) + sample
                fam.add("dcn_sample")
                if "conv2d" not in w.nested[w.nested.index("dcn_ps"):]:
                    fam.add("project_as")
            w.families |= fam
            w.cur_families = fam
            mod = w.owner()
            ref = getattr(w, name, None)
            if ref is not None:
                with torch.no_grad():
                    ref(mod, args, kw, out)
            return out
        return run

    for n in WRAPPED:
        monkeypatch.setattr(ops, n, wrap(n, w.orig[n]))
    def leave(m_, a_, o_):                                               # (returns None: a forward hook's return value would replace the output)
        w.stack.pop()
    hooks = []
    kinds = (D.BasicBlock, D.Root, D.Tree, D.DeformConv, D.IDAUp, D.DLA, type(pred))
    for m in model.modules():
        if isinstance(m, kinds):
            hooks.append(m.register_forward_pre_hook(lambda m_, a_: w.stack.append(m_)))
            hooks.append(m.register_forward_hook(leave))
    # the Predictor is entered through forward_nhwc (no __call__): its calls are attributed by a wrapper of that method
    orig_fwd = pred.forward_nhwc

    def pred_fwd(features, *a, **k):
        w.stack.append(pred)
        try:
            hm = orig_fwd(features, *a, **k)
        finally:
            w.stack.pop()
        w.pred_in, w.pred_out = features, hm.clone()
        return hm
    monkeypatch.setattr(pred, "forward_nhwc", pred_fwd)
    # DLA.forward / IDAUp.forward are called as modules; DLASeg is entered through forward_nhwc and needs no owner
    try:
        if mode == "fp16x2":
            L.f16x2_range_ok(reset=True)
        with torch.no_grad():
            det, topk, valid, hm = model.detect_device(images, *tg)
        torch.cuda.synchronize()
        if mode == "fp16x2":
            assert L.f16x2_range_ok()
        # ---- the Predictor as a whole (edge fusion included): every written channel of the final head map
        with torch.no_grad():
            taps = {}
            x64 = _nchw64(w.pred_in)
            ei, el = tg[0].long(), tg[1].long()
            maps = w.pred_ref(x64, ei, el, taps)
            got = torch.cat((_nchw64(w.pred_out[..., :3]), _nchw64(w.pred_out[..., REG_OFF:REG_OFF + 50])), 1)
            want = torch.cat((taps["cls_logits"], maps["reg"]), 1)
            m = _metrics(got, want)
            w.judge("predictor (final head map, edge fusion included)", m, HEADS_BOUND[mode])
            w.see(pred, "predictor")
        # ---- decode: the reference's NMS + top-K + box decode on the HIP head map of every image
        hmc = w.pred_out.float().cpu()
        worst_row, same = 0.0, True
        for b in range(B):
            cls = torch.sigmoid(hmc[b:b + 1, ..., :3].permute(0, 3, 1, 2)).clamp(1e-4, 1 - 1e-4)
            reg = hmc[b:b + 1, ..., REG_OFF:REG_OFF + 50].permute(0, 3, 1, 2)
            t = tgts[b]
            dec = R.decode_image(cls, reg, R.Calib(t["P"]), t["pad_size"], t["size"], threshold=model.heads.post_processor.det_threshold,
                                 K=model.heads.post_processor.max_detection, output_depth=model.heads.post_processor.output_depth)
            tk = topk[b].cpu()
            same_b = bool((tk[:, 1].long() == dec["indexs"]).all()) and bool((tk[:, 2].long() == dec["clses"].long()).all())
            same = same and same_b
            v = valid[b].cpu().bool()
            rows = det[b].cpu()[v]
            if same_b and rows.shape[0] == dec["result"].shape[0] and rows.numel():
                worst_row = max(worst_row, float(((rows - dec["result"]).abs() / dec["result"].abs().clamp(min=1.0)).max()))
            elif not same_b or rows.shape[0] != dec["result"].shape[0]:
                worst_row = float("inf")
        w.rec.append(("decode (every image)", dict(same_topk=float(same), row_rel=worst_row), 1e-4, 1e-4))
        if not same or worst_row > 1e-4:
            w.fail.append("decode")
        w.see(model.heads.post_processor, "decode")
    finally:
        for h in hooks:
            h.remove()
    # ---- report
    os.makedirs(REPORT_DIR, exist_ok=True)
    with open(os.path.join(REPORT_DIR, "layer_oracle_%s.json" % mode), "w") as f:
        json.dump(dict(mode=mode, batch=B, families=sorted(w.families),
                       layers=[dict(layer=n, bound_max=bm, bound_mean=bn, **m) for n, m, bm, bn in w.rec],
                       teeth=[dict(case=n, metric=k, observed=v, bound=bd) for n, k, v, bd in w.teeth]), f, indent=1)
    for n, m, bm, bn in w.rec:
        print("%-6s %-60s %s" % (mode, n, " ".join("%s %.2e" % kv for kv in sorted(m.items()))))
    print("%s census: kernel families %s" % (mode, sorted(w.families)))
    # ---- census: every module of the network seen exactly once
    n_dcn = sum(1 for m in model.modules() if isinstance(m, D.DeformConv))
    assert n_dcn == 16
    for m in model.modules():
        if isinstance(m, D.DeformConv):
            assert w.seen.get((id(m), "dcn")) == 1, w.names[id(m)]
        elif isinstance(m, D.BasicBlock):
            assert w.seen.get((id(m), "c1")) == 1 and w.seen.get((id(m), "c2")) == 1, w.names[id(m)]
        elif isinstance(m, D.Root):
            assert w.seen.get((id(m), "root")) == 1, w.names[id(m)]
        elif isinstance(m, D.Tree) and m.project is not None and m.levels == 1:
            assert w.seen.get((id(m), "proj")) == 1, w.names[id(m)]
        elif isinstance(m, D.IDAUp):
            for k in range(1, 10):
                if hasattr(m, "up_%d" % k):
                    assert w.seen.get((id(m), "up_%d" % k)) == 1, (w.names[id(m)], k)
    assert w.seen.get((id(model.backbone.base), "f1")) == 1
    assert w.seen.get((id(pred), "predictor")) == 1 and w.seen.get((id(model.heads.post_processor), "decode")) == 1
    assert w.families == FAMILIES[mode], "missing %s, unexpected %s" % (sorted(FAMILIES[mode] - w.families), sorted(w.families - FAMILIES[mode]))
    # ---- teeth: each deliberately wrong reference is missed by >= 2x its bound
    weak = [(n, k, v, bd) for n, k, v, bd in w.teeth if not v >= 2 * bd]
    assert not weak, weak
    assert not w.fail, w.fail
