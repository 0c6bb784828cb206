"""The edge fusion's conv chain per Conv1d window: the one kernel (mfx_edge_chain_ks; k = 3: mfx_edge_chain_act) against the five mfx_conv2d_nhwc launches of
the same build, at the flagship shape (B = 8, 96 x 320 map, L = 832 border points), bf16 and fp16.  Both forms are captured into one hipGraph each
(as the inference step replays them) and the graphs are replayed alternately; the figure is the median of `--repeats` timed windows of `--iters` replays
(device events), with the fastest and slowest window beside it.  Prints one markdown table row per (type, window) -- profiles/edge_fusion_settings.md.

    python tools/edge_fusion_bench.py [--iters 200] [--repeats 7]
"""
import argparse
import os
import statistics
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

B, H, W = 8, 96, 320


def predictor(k, norm, relu):
    from monoflex_amd import synthetic as S
    from monoflex_amd.config import get_cfg
    from monoflex_amd.model.head.detector_predictor import _predictor
    cfg = get_cfg(os.path.join(ROOT, "runs", "monoflex.yaml"), ["MODEL.HEAD.EDGE_FUSION_KERNEL_SIZE", k, "MODEL.HEAD.EDGE_FUSION_NORM", norm,
                                                              "MODEL.HEAD.EDGE_FUSION_RELU", relu])
    m = _predictor(cfg, 64).eval()
    sd = S.synthetic_state_dict({"heads.predictor." + q: v for q, v in m.state_dict().items()}, seed=3)
    m.load_state_dict({q[len("heads.predictor."):]: v for q, v in sd.items()})
    return m.cuda()


def five_launches(ops, m, p, feats, ei32, rowmap):
    Lm, h = ei32.shape[1], m.edge_halo
    trunk = ops.conv2d(feats, p.edge_trunk, rowmap=rowmap).view(B, 1, Lm + 2 * h, 512)
    return [ops.conv2d(ops.conv2d(trunk, pk1, x_ch_off=bi * 256), pk2, out_dtype=torch.float32) for bi, (pk1, pk2, _, _) in enumerate(p.edge_branches)]


def capture(fn):
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        for _ in range(3):
            fn()
    torch.cuda.current_stream().wait_stream(s)
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        keep = fn()
    return g, keep


def window(g, iters):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(iters):
        g.replay()
    b.record()
    b.synchronize()
    return a.elapsed_time(b) * 1e3 / iters                                 # microseconds per replay


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=200)
    ap.add_argument("--repeats", type=int, default=7)
    ap.add_argument("--norm", default="BN")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("edge_fusion_bench: needs the GPU")
    from monoflex_amd import ops, synthetic as S
    from monoflex_amd.model.head.detector_predictor import make_edge_rowmap
    tgt = S.synthetic_target(W, H)
    ei32 = torch.stack([tgt["edge_indices"]] * B).to("cuda", torch.int32).contiguous()
    print("B = %d, %d x %d, L = %d, norm %s; microseconds per replay: median (fastest .. slowest) of %d windows of %d replays"
          % (B, H, W, ei32.shape[1], args.norm, args.repeats, args.iters))
    print("| type | k | one kernel | five launches | one / five | equal |")
    print("|---|---|---|---|---|---|")
    for dtype in (torch.bfloat16, torch.float16):
        feats = torch.randn(B, H, W, 64, generator=torch.Generator().manual_seed(9)).relu().to("cuda", dtype)
        for k in (1, 3, 5, 7):
            m = predictor(k, args.norm, False)
            p = m._pack(dtype)
            rowmap = make_edge_rowmap(ei32, H, W, m.edge_halo)              # (targets only: prepared with the batch, outside the step)
            g1, o1 = capture(lambda: ops.edge_chain(feats, ei32, p.edge_chain))
            g5, o5 = capture(lambda: five_launches(ops, m, p, feats, ei32, rowmap))
            g1.replay(); g5.replay()
            torch.cuda.synchronize()
            equal = all(torch.equal(o1[bi], o5[bi].view(B, -1, 4)) for bi in range(2))
            t1, t5 = [], []
            for _ in range(args.repeats):                                   # alternating
                t1.append(window(g1, args.iters))
                t5.append(window(g5, args.iters))
            print("| %s | %d | %.1f (%.1f .. %.1f) | %.1f (%.1f .. %.1f) | %.2f | %s |"
                  % (str(dtype).replace("torch.", ""), k, statistics.median(t1), min(t1), max(t1), statistics.median(t5), min(t5), max(t5),
                     statistics.median(t1) / statistics.median(t5), "yes" if equal else "NO"), flush=True)


if __name__ == "__main__":
    main()
