"""Digest of every packed weight operand of the detector, on the CPU: one line per pack with a SHA-256 of each tensor field's bytes and
every scalar field, for each compute tag (fp32, bf16, fp16, split precision).  Two commits pack identically exactly when this prints the same
text at both, so it only uses names both have: ops.pack_conv / pack_stem / pack_cat / add_f16_fragments / dcn_ps_pack / pack_upsample, the DCN
module's packed_offset / packed_main and the predictor's _pack.

    python tools/pack_digest.py > digest.txt
"""
import dataclasses
import hashlib
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from monoflex_amd import lib as L, ops                                       # noqa: E402
from monoflex_amd.config import get_cfg                                      # noqa: E402
from monoflex_amd.model.backbone import dla_dcn as D                         # noqa: E402
from monoflex_amd.model.detector import KeypointDetector                     # noqa: E402

# not printed with the pack: nested packs (lines of their own), run-time bookkeeping (transient, entry, f1_w160 -- a cached slice of `w`) and
# split_scale, which every hash of `w` and `scale` already depends on
NOT_HASHED = {"ps", "edge_trunk", "edge_branches", "split_scale", "transient", "entry", "f1_w160"}


def sha(t):
    t = t.detach().contiguous()
    return "%s%s:%s" % (str(t.dtype).replace("torch.", ""), list(t.shape), hashlib.sha256(t.view(torch.uint8).numpy().tobytes()).hexdigest())


def show(name, p):
    if torch.is_tensor(p):
        print(name, sha(p))
        return
    out = []
    for f in dataclasses.fields(p):
        v = getattr(p, f.name)
        if f.name not in NOT_HASHED:
            out.append("%s=%s" % (f.name, sha(v) if torch.is_tensor(v) else repr(v)))
    print(name, " ".join(out))


def build_model():
    torch.manual_seed(0)
    cfg = get_cfg(os.path.join(ROOT, "runs", "monoflex.yaml"))
    cfg.MODEL.PRETRAIN = False
    m = KeypointDetector(cfg).eval()
    g = torch.Generator().manual_seed(1)
    with torch.no_grad():
        for mod in m.modules():
            if hasattr(mod, "running_var"):                                   # BatchNorm2d / BatchNorm1d / the heads' ABN holder: fold_bn must see real statistics
                n = mod.running_var.numel()
                mod.running_mean.copy_(torch.randn(n, generator=g) * 0.2)
                mod.running_var.copy_(torch.rand(n, generator=g) + 0.5)
                mod.weight.copy_(torch.rand(n, generator=g) + 0.5)
                mod.bias.copy_(torch.randn(n, generator=g) * 0.1)
            if hasattr(mod, "conv_offset_mask"):                              # zero-initialised in the model: give the offset convs weights to pack
                c = mod.conv_offset_mask
                c.weight.copy_(torch.randn(c.weight.shape, generator=g) * 0.02)
                c.bias.copy_(torch.randn(c.bias.shape, generator=g) * 0.1)
                mod.bias.copy_(torch.randn(mod.bias.shape, generator=g) * 0.1)
    return m


def root_sources(tree, cin, children=()):
    """{Root module: channels of its sources}, following Tree.forward's bookkeeping (x2, x1, *children) without running it."""
    cout = tree.tree1.conv1.out_channels if tree.levels == 1 else None
    children = list(children) + ([cin] if tree.level_root else [])
    if tree.levels == 1:
        return {tree.root: (cout, cout, *children)}
    out = root_sources(tree.tree1, cin)
    c1 = tree.tree1.root.conv.out_channels if tree.tree1.levels == 1 else tree.tree1.tree2.root.conv.out_channels
    out.update(root_sources(tree.tree2, c1, children + [c1]))
    return out


def conv_bn(name, conv, bn, tag, act):
    scale, shift = ops.fold_bn(bn)
    show(name, ops.pack_conv(conv.weight, tag, scale, shift, stride=conv.stride[0], pad=conv.padding[0], act=act))


def digest(m, tag, tname):
    base = m.backbone.base
    chans = {}
    for i in range(2, 6):
        lvl = getattr(base, "level%d" % i)
        chans.update(root_sources(lvl, base.channels[i - 1]))
    for name, mod in m.named_modules():
        pre = "%s %s" % (tname, name)
        if isinstance(mod, D.DLA):
            scale, shift = ops.fold_bn(mod.base_layer[1])
            show(pre + ".stem", ops.pack_stem(mod.base_layer[0].weight, tag, scale, shift))
            for lvl in ("level0", "level1"):
                seq = getattr(mod, lvl)
                for j in range(0, len(seq), 3):
                    conv_bn("%s.%s.c%d" % (pre, lvl, j), seq[j], seq[j + 1], tag, L.ACT_RELU)
        elif isinstance(mod, D.BasicBlock):
            conv_bn(pre + ".c1", mod.conv1, mod.bn1, tag, L.ACT_RELU)
            conv_bn(pre + ".c2", mod.conv2, mod.bn2, tag, L.ACT_RELU)
        elif isinstance(mod, D.Tree) and mod.project is not None and mod.levels == 1:
            conv_bn(pre + ".proj", mod.project[0], mod.project[1], tag, L.ACT_NONE)
        elif isinstance(mod, D.Root):
            scale, shift = ops.fold_bn(mod.bn)
            show(pre + ".cat%s" % (chans[mod],), ops.pack_cat(mod.conv.weight, tag, scale, shift, chans[mod], act=L.ACT_RELU))
        elif isinstance(mod, D.DeformConv):
            mod.conv._packs.clear()
            show(pre + ".off", mod.conv.packed_offset(tag))
            p = mod.conv.packed_main(tag, mod.actf[0], L.ACT_RELU)
            show(pre + ".main", p)
            if tag in (torch.bfloat16, torch.float16) and mod.conv.in_channels >= 128:      # (a superset of the layers ops.dcn_ps_applies picks at B = 8)
                show(pre + ".main.ps", ops.dcn_ps_pack(p))
        elif isinstance(mod, D.IDAUp):
            k = 1
            while hasattr(mod, "up_%d" % k):
                show("%s.up_%d" % (pre, k), ops.pack_upsample(getattr(mod, "up_%d" % k).weight))
                k += 1
    pred = m.heads.predictor
    pred._packs.clear()
    p = pred._pack(tag)                                                       # both MFMA forms of the 16-bit packs are fields of the one pack
    show("%s heads" % tname, p)
    show("%s heads.edge_trunk" % tname, p.edge_trunk)
    for i, (pk1, pk2, cout, choff) in enumerate(p.edge_branches):
        show("%s heads.edge%d.k3 cout=%d choff=%d" % (tname, i, cout, choff), pk1)
        show("%s heads.edge%d.1x1" % (tname, i), pk2)
    # layouts the yaml's network does not reach: a stem that is not the dedicated 16-channel one, the 64-byte K row, a padded Cout
    g = torch.Generator().manual_seed(2)
    show("%s extra.stem32" % tname, ops.pack_stem(torch.randn(32, 3, 7, 7, generator=g), tag, torch.rand(32, generator=g) + 0.5, torch.randn(32, generator=g)))
    show("%s extra.k64" % tname, ops.pack_conv(torch.randn(20, 8, 1, 1, generator=g), tag, None, torch.randn(20, generator=g), cout=24))
    w = torch.randn(64, 32, 3, 3, generator=g)
    show("%s extra.s2" % tname, ops.add_f16_fragments(ops.pack_conv(w, tag, torch.rand(64, generator=g) + 0.5, None, stride=2, pad=1), w))


def main():
    m = build_model()
    for tname, tag in (("fp32", torch.float32), ("bf16", torch.bfloat16), ("fp16", torch.float16), ("f16x2", ops.F16X2)):
        digest(m, tag, tname)


if __name__ == "__main__":
    main()
