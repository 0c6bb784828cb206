"""Builds libmonoflex_hip.so (hand-written HIP for gfx950).

`hipcc --offload-arch=gfx950` cross-compiles without a GPU.  The .so is built in-tree
(monoflex_amd/csrc/libmonoflex_hip.so) so it travels to the GPU box with the repo snapshot.
"""
import hashlib
import os
import subprocess
import sys
from concurrent.futures import ThreadPoolExecutor

HERE = os.path.dirname(os.path.abspath(__file__))
CSRC = os.path.join(HERE, "csrc")
OBJ = os.path.join(CSRC, "build")
LIB = os.path.join(CSRC, "libmonoflex_hip.so")
SOURCES = ["capi.hip", "options.hip", "conv_kernels.hip", "conv_halo.hip", "conv_cw.hip", "conv_cws.hip", "misc_kernels.hip", "stem.hip", "f1_fused.hip", "heads.hip", "edge_chain.hip", "decode.hip", "decode_multi.hip", "dcn_wave.hip", "dcn_patch.hip", "dcn_lds.hip", "dcn_ps.hip", "gemm_as.hip", "dcn_ext.hip", "dcn_bwd.hip", "dcn_bwd_tile.hip", "psroi_pool.hip", "train_kernels.hip", "adamw.hip", "wgrad_tr.hip", "loss_kernels.hip", "box3d_iou.hip", "box_nms.hip", "eval_diag.hip", "head_sparse.hip", "gram_heads.hip", "kitti_encode.hip", "kitti_resident.hip", "kitti_eval.hip", "kitti_eval_pack.hip"]
FLAGS = ["--offload-arch=gfx950", "-O3", "-std=c++17", "-fPIC", "-Wall", "-Wno-unused-function"]
if os.environ.get("MFX_PROBES") == "1":      # probe build: compiles the timing-probe switches in (options heads_dbg / dcn_bt_dbg: wrong results by design)
    FLAGS.append("-DMFX_PROBES")
# the target encoder reproduces numpy's twice-rounded float32/float64 arithmetic: no fused multiply-add there
EXTRA_FLAGS = {"kitti_encode.hip": ["-ffp-contract=off"], "kitti_resident.hip": ["-ffp-contract=off"], "kitti_eval.hip": ["-ffp-contract=off"],
               # the record rule is numpy's float32 round(4): multiply, rint, divide, each rounded once
               "kitti_eval_pack.hip": ["-ffp-contract=off"],
               # r06: with the SLP vectoriser's packed-fp32 code (v_pk_fma_f32 / v_pk_mul_f32) the fused sample + weight-gradient kernels of this file gave
               # run-to-run different results in lanes 48..63 of ~0.03 % of the samples (a timing-dependent hazard this compiler does not cover; bisected in
               # profiles/r06_dcnbwd_repeatability.md: barriers, waits, nops and the LDS-read builtin do not cure it, scalar fp32 code does).  Costs nothing:
               # the training step is 0.5 % FASTER without it.  tests/test_gpu_train.py::test_dcn_backward_is_repeatable guards it.
               "dcn_bwd_tile.hip": ["-fno-slp-vectorize"]}


def _hipcc():
    return "/opt/rocm/bin/hipcc" if os.path.exists("/opt/rocm/bin/hipcc") else "hipcc"


def _headers_digest():
    h = hashlib.sha1()
    for root in (CSRC, os.path.join(os.path.dirname(HERE), "include")):
        for fn in sorted(os.listdir(root)):
            if fn.endswith(".h"):
                with open(os.path.join(root, fn), "rb") as f:
                    h.update(fn.encode() + f.read())
    return h.hexdigest()


def _source_stamp(src, headers):
    h = hashlib.sha1()
    with open(os.path.join(CSRC, src), "rb") as f:
        h.update(f.read())
    h.update((headers + " ".join(FLAGS + EXTRA_FLAGS.get(src, []))).encode())
    return h.hexdigest()


def build_lib(force=False, verbose=False):
    """Compile what changed (a translation unit is rebuilt when its source, any header or its flags changed) and relink."""
    os.makedirs(OBJ, exist_ok=True)
    hipcc = _hipcc()
    headers = _headers_digest()
    stamps = {src: _source_stamp(src, headers) for src in SOURCES}

    def stale(src):
        obj, st = os.path.join(OBJ, src.replace(".hip", ".o")), os.path.join(OBJ, src.replace(".hip", ".stamp"))
        return force or not os.path.exists(obj) or not os.path.exists(st) or open(st).read() != stamps[src]

    todo = [src for src in SOURCES if stale(src)]
    link_stamp_file = os.path.join(OBJ, "stamp")
    link_stamp = hashlib.sha1("".join(stamps[s] for s in SOURCES).encode()).hexdigest()
    if not todo and os.path.exists(LIB) and os.path.exists(link_stamp_file) and open(link_stamp_file).read() == link_stamp:
        return LIB

    def compile_one(src):
        obj = os.path.join(OBJ, src.replace(".hip", ".o"))
        cmd = [hipcc] + FLAGS + EXTRA_FLAGS.get(src, []) + ["-c", os.path.join(CSRC, src), "-o", obj]
        r = subprocess.run(cmd, capture_output=True, text=True)
        if r.returncode != 0:
            raise RuntimeError("hipcc failed for %s:\n%s" % (src, r.stderr))
        if verbose and r.stderr:
            sys.stderr.write(r.stderr)
        with open(os.path.join(OBJ, src.replace(".hip", ".stamp")), "w") as f:
            f.write(stamps[src])
        return obj
    with ThreadPoolExecutor(max_workers=min(8, os.cpu_count() or 4)) as ex:
        list(ex.map(compile_one, todo))
    objs = [os.path.join(OBJ, src.replace(".hip", ".o")) for src in SOURCES]
    r = subprocess.run([hipcc, "--offload-arch=gfx950", "-shared", "-fPIC", "-o", LIB] + objs, capture_output=True, text=True)
    if r.returncode != 0:
        raise RuntimeError("link failed:\n" + r.stderr)
    with open(link_stamp_file, "w") as f:
        f.write(link_stamp)
    return LIB


if __name__ == "__main__":
    print(build_lib(force="--force" in sys.argv, verbose=True))
