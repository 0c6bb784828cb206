#!/usr/bin/env python
"""The two DCN module groups of the benchmarked network (dla_up.ida_1: two 256 -> 128 @ 24x80, dla_up.ida_2: three 128 -> 64 @ 48x160; bf16), each
as ONE grouped launch pair (ops.dcn_module_group, option dcn_group = 1) against the sum of its modules launched one by one (dcn_group = 0), 10 groups
per hipGraph replay; every module has its own input map and weights.  Also checks that both forms give the same bits.
usage: python tools/dcn_group_bench.py [B=8] [std=3.0] [dcn_tile values to try on the grouped form, default 0 = the dispatcher's choice: 0,4,6,3]"""
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import torch
from monoflex_amd import lib, ops
from monoflex_amd.model.backbone.dla_dcn import DeformConv

L = lib.load()
B = int(sys.argv[1]) if len(sys.argv) > 1 else 8
STD = float(sys.argv[2]) if len(sys.argv) > 2 else 3.0
TILES = [int(t) for t in (sys.argv[3] if len(sys.argv) > 3 else "0").split(",")]
GROUPS = [(24, 80, 256, 128, 2), (48, 160, 128, 64, 3), (48, 160, 128, 64, 4)]
N = 10
dt = torch.bfloat16


def timed(fn):
    s = torch.cuda.Stream()
    with torch.cuda.stream(s):
        for _ in range(3):
            fn()
        torch.cuda.synchronize()
        g = torch.cuda.CUDAGraph()
        with torch.cuda.graph(g, stream=s):
            for _ in range(N):
                fn()
        g.replay(); torch.cuda.synchronize()
        ts = []
        for _ in range(5):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for _ in range(5):
                g.replay()
            e1.record(); torch.cuda.synchronize()
            ts.append(e0.elapsed_time(e1) / (5 * N) * 1e3)
    return sorted(ts)[2], max(ts) - min(ts)


print("| group (B=%d, std %.1f px) | separate us (median, spread of 5) | grouped us | dcn_tile | groups ran | same bits |" % (B, STD))
print("|---|---|---|---|---|---|")
for (H, W, Ci, Co, n) in GROUPS:
    torch.manual_seed(0)
    mods, xs = [], []
    for i in range(n):
        m = DeformConv(Ci, Co).eval().cuda()
        torch.nn.init.normal_(m.conv.conv_offset_mask.weight, std=STD / (0.7 * (9 * Ci) ** 0.5))
        mods.append(m)
        xs.append(torch.randn(B, H, W, Ci, device="cuda").relu().to(dt))
    offs = [m.conv.packed_offset(dt) for m in mods]
    mains = [m.conv.packed_main(dt, m.actf[0], lib.ACT_RELU) for m in mods]
    run = lambda: ops.dcn_module_group(xs, offs, mains)      # noqa: E731
    with torch.no_grad():
        lib.set_options({"dcn_group": 0})
        want = run()[0]
        t_sep, s_sep = timed(run)
        for tile in TILES:
            lib.set_options({"dcn_group": 1, "dcn_tile": tile})
            c0 = L.mfx_get_counter(b"dcn_group")
            got = run()[0]
            torch.cuda.synchronize()
            ran = L.mfx_get_counter(b"dcn_group") - c0
            same = all(torch.equal(a, b) for a, b in zip(got, want))
            t_grp, s_grp = timed(run)
            print("| %d x %d->%d @ %dx%d | %.1f (%.1f) | %.1f (%.1f) | %d | %d | %s |" % (n, Ci, Co, H, W, t_sep, s_sep, t_grp, s_grp, tile, ran, same), flush=True)
        L.mfx_reset_options()
