// The registry of the library's process-wide tuning switches (mfx_set_option) and dispatch counters (mfx_get_counter).
// These two lists are the complete set and its documentation: a new switch or counter is ONE line here, and every translation
// unit that includes this header can read g_opt_<name> / bump g_cnt_<name>.  options.hip defines the variables and the four
// entry points from the same lists; nothing else may define, declare or assign them (tests/test_host_cpu.py checks that, and
// that every listed name is used by some kernel unit).
#pragma once

// no bound on that side
#define MFX_NOLO (-2147483647 - 1)
#define MFX_NOHI 2147483647

// X(name, default, lo, hi, "what it does; what the values mean"): mfx_set_option clamps the value into [lo, hi].  The few rules
// that are not a clamp (dcn_bt_fuse_blocks, deterministic, the topk_merge_* range errors) are option_rule() in options.hip.
#define MFX_OPTION_LIST(X) \
    /* forward convolutions (conv_kernels.hip, conv_halo.hip, conv_cw.hip, conv_cws.hip) */ \
    X(conv_tile, 0, MFX_NOLO, MFX_NOHI, "implicit-GEMM tile of mfx_conv2d_nhwc: 0 = automatic, else a tile id (conv_kernels.hip: 1 = 256x16, 2 = 256x32, 3 = 128x64, " \
        "4 = 64x64, 5 = 128x128, 6 = 64x128, 7 = 256x64, 8 = 256x128 / 8 waves, 9 = 128x128 / 8 waves), taken where it fits Cout_pad") \
    X(dcn_tile, 0, MFX_NOLO, MFX_NOHI, "the same for the fused gather DCN kernel") \
    X(cat_tile, 0, MFX_NOLO, MFX_NOHI, "the same for mfx_cat_conv1x1_nhwc") \
    X(kc, 0, MFX_NOLO, MFX_NOHI, "16-byte chunks per LDS row of the implicit-GEMM main loop: 0 = automatic (8 where K_pad allows), 4 = force 4") \
    X(ksplit, 0, MFX_NOLO, MFX_NOHI, "split-K of mfx_conv2d_nhwc: 0 = automatic (never: measured neutral-to-slower on DLA level4/5), 1 = never split, " \
        "n = force n splits where legal") \
    X(dcn_ksplit, 0, MFX_NOLO, MFX_NOHI, "the same for the fused DCN kernel") \
    X(halo, 1, MFX_NOLO, MFX_NOHI, "LDS-staged halo kernels for 3x3 convs: 0 = generic kernel only, 1 = automatic, >= 2 = force variant (value - 1)") \
    X(halo_cg, 0, MFX_NOLO, MFX_NOHI, "max channels per patch pass of the halo kernel (0 = default)") \
    X(halo_s2, 1, MFX_NOLO, MFX_NOHI, "0 = stride-2 3x3 convs stay on the generic implicit-GEMM kernel") \
    X(halo_pair, 1, MFX_NOLO, MFX_NOHI, "split precision walks K in step pairs where mfx_conv_desc.w_frag_pair is given (0 = two mma_chunk per pair)") \
    X(halo_cw, 1, MFX_NOLO, MFX_NOHI, "0 = conv3x3_wave_kernel only, 1 = the compile-time-geometry kernel (conv_cw.hip) where an instantiation exists") \
    X(cw_rows6, 1, MFX_NOLO, MFX_NOHI, "0 = 8-row tiles everywhere in conv_cw.hip (1: 6-row tiles where Ho % 6 == 0, Ho % 8 != 0, Ho <= 48)") \
    X(halo_cws, 1, MFX_NOLO, MFX_NOHI, "0 = conv3x3_wave_kernel<f32s_t> only, 1 = the compile-time-geometry split-precision kernel (conv_cws.hip) where an instantiation exists") \
    /* forward deformable convolution (dcn_wave.hip, dcn_patch.hip, dcn_lds.hip) */ \
    X(dcn_wave, 1, MFX_NOLO, MFX_NOHI, "0 = first-generation kernel only, 1 = automatic, 2.. = force variant") \
    X(dcn_patch, 1, MFX_NOLO, MFX_NOHI, "LDS-patch DCN kernel: 0 = off, 1 = automatic, 2 = force (FM 4), 3 = force FM 2, 4 = force FM 1, 5-7 = wide margin FM 4/2/1, " \
        "8 = padded layout") \
    X(dcn_patch_fn8, 1, MFX_NOLO, MFX_NOHI, "1 = one workgroup of the LDS-patch kernel covers 128 output channels where Cout_pad % 128 == 0") \
    X(dcn_fuse_off, 1, MFX_NOLO, MFX_NOHI, "1 = the LDS-patch kernel computes the offset/mask conv itself where the caller supplies its weights") \
    X(dcn_lds, 1, MFX_NOLO, MFX_NOHI, "0 = off, 1 = automatic (64 -> 64 on large 16-bit maps), 2 = wherever the kernel applies") \
    X(dcn_lds_rows, 16, MFX_NOLO, MFX_NOHI, "tile rows, 16 | 8 (three workgroups per CU; measured slower: 2.570 vs 2.551 ms per step, profiles/r06_dcn_lds.md)") \
    X(dcn_group, 1, 0, 1, "1 = mfx_dcn_module_group runs same-shape 16-bit gather-kernel DCN modules as one offset-conv launch and one gather launch " \
        "(bit-identical output), 0 = it refuses every group and the caller launches module by module") \
    /* detection heads and decode (heads.hip, decode.hip) */ \
    X(heads_persist, 1, MFX_NOLO, MFX_NOHI, "1 = one workgroup per resident slot (n > 1: n workgroups), each a contiguous range of (tile, branch) units; " \
        "0 = one workgroup per tile.  B=8 bf16: 516 -> 503 us (tools/probes/heads_probe.py), bit-identical output") \
    X(heads_mfma32, 0, MFX_NOLO, MFX_NOHI, "1 = the v_mfma_f32_32x32x16 form of the kernel where the caller supplies its packs (mfx_heads_desc.w1_32 / w2_32)") \
    X(heads_planes, 0, MFX_NOLO, MFX_NOHI, "1 = four k-group planes (no LDS bank conflicts: 48 % -> 11 % of the LDS cycles, LDS-active cycles -42 %), " \
        "0 = one 144-byte record per pixel.  Same kernel time (555 vs 555 us, A/B in one run): not LDS-bound") \
    X(edge_chain, 1, MFX_NOLO, MFX_NOHI, "1 = the edge fusion's conv chain (trunk, Conv1d, 1x1 of both branches) as one kernel where mfx_edge_chain applies " \
        "(edge_chain.hip: 16-bit modes, bit-identical output), 0 = five mfx_conv2d_nhwc launches") \
    X(topk_strips, 8, MFX_NOLO, MFX_NOHI, "row strips per (class, image) map when a workspace is supplied; 1 = single-workgroup kernel") \
    X(topk_merge_z, 16, MFX_NOLO, MFX_NOHI, "workgroups per (class, image) map in the merge; values outside 1..64 are an error") \
    X(topk_merge_threads, 512, MFX_NOLO, MFX_NOHI, "their size; must be a multiple of 64 in 64..512 (the merge ranks by whole wavefronts; 512 = its __launch_bounds__)") \
    /* weight gradients (train_kernels.hip, wgrad_tr.hip) */ \
    X(wgrad_mfma, 1, MFX_NOLO, MFX_NOHI, "0 = VALU kernel for bf16 too, 1 = 64x64 MFMA tiles, 3 = 128x128 where they fit") \
    X(wgrad_blocks, 600, MFX_NOLO, MFX_NOHI, "target workgroup count of the MFMA weight-gradient kernel (measured, B=8 step: 64 -> 146 ms, 150 -> 90, 300 -> 78, " \
        "600 -> 73, 2048 -> 75, 8192 -> 81: the tile atomics of every slab cost more than the extra workgroups hide)") \
    X(wgrad_ws, 1, MFX_NOLO, MFX_NOHI, "0 = always accumulate the tiles with atomics") \
    X(wgrad_ws_blocks, 1200, MFX_NOLO, MFX_NOHI, "target workgroup count when partial tiles go to the workspace (step: 1200 -> 58.0 ms, 2400 -> 58.3, 4800 -> 58.6; " \
        "atomics: 59.6)") \
    X(wgrad_min_m, 128, MFX_NOLO, MFX_NOHI, "fewest pixels of a slab of the MFMA weight-gradient kernel.  r06: 1024 left the 1x1 / Root layers of the 24x80 and 12x40 " \
        "maps with 8-16 slabs (120-240 workgroups of 32 iterations each: 31 us per layer for 4 GFLOP); same-box step 17.50 (1024) / 17.31 (512) / 17.27 (256) / " \
        "17.23-17.31 (128) / 17.26 (64) ms") \
    X(wgrad_tr, 1, MFX_NOLO, MFX_NOHI, "0 = first-generation kernel everywhere (2: the transposed-read kernel also where Cout % 128 != 0)") \
    X(wgrad_tr_blocks, 512, 1, MFX_NOHI, "target workgroup count (tiles x pixel slabs)") \
    X(wgrad_patch, 1, MFX_NOLO, MFX_NOHI, "0 = off (the 3x3 / s1 / p1 weight-gradient form with the input patch in LDS)") \
    X(wgrad_patch_blocks, 256, 1, MFX_NOHI, "target workgroup count") \
    X(wgrad_patch_waves, 12, MFX_NOLO, MFX_NOHI, "6 (64 x 96 block per wave) or 12 (64 x 48)") \
    X(stem_wgrad_blocks, 512, 1, MFX_NOHI, "target workgroup count of the stem's weight-gradient kernel (mfx_stem_wgrad_16)") \
    /* train-mode BatchNorm (train_kernels.hip) */ \
    X(bn_apply_blocks, 1024, MFX_NOLO, MFX_NOHI, "workgroup cap of the two-launch forms' streaming kernels") \
    X(bn_blocks, 768, MFX_NOLO, MFX_NOHI, "target workgroup count of the column reductions (BN statistics / backward sums / bias sums)") \
    X(bn_onepass, 3, MFX_NOLO, MFX_NOHI, "bit 0 = backward, bit 1 = forward in one launch where the map fits (0 = the two-launch forms everywhere)") \
    X(bn_onepass_min_chunks, 200000, MFX_NOLO, MFX_NOHI, "smaller maps keep the two launches (backward)") \
    X(bn_onepass_fwd_min_chunks, 900000, MFX_NOLO, MFX_NOHI, "the same for the forward") \
    X(bn_onepass_grid, 0, MFX_NOLO, MFX_NOHI, "workgroup cap (0 = by map size, see bn_onepass_plan)") \
    /* deformable convolution backward (dcn_bwd.hip, dcn_bwd_tile.hip) */ \
    X(dcn_wgrad_m, 512, 64, MFX_NOHI, "pixels per workgroup slab of the DCN weight-gradient kernel (step: 512 -> 73.1 ms, 2048 -> 73.8, 8192 -> 83.6)") \
    X(ext_bwd_fast, 1, MFX_NOLO, MFX_NOHI, "0 = the first-generation scatter backward for every geometry of the `_ext` boundary") \
    X(dcn_bt_fuse_blocks, 170, MFX_NOLO, MFX_NOHI, "workgroups per tap group of the fused kernel; a value <= 0 means 170") \
    X(dcn_bt_fly_bias, 1, MFX_NOLO, MFX_NOHI, "the gcol-free sample kernel also sums grad_bias from the dy rows it loads (0: a separate column-sum pass)") \
    X(dcn_bt_gcol_as, 1, MFX_NOLO, MFX_NOHI, "d(columns) = dy . W^T of the 16-bit layers on the activation-stationary GEMM (gemm_as.hip); 0: the tiled 1x1 kernel") \
    X(dcn_bt_fly, 1, MFX_NOLO, MFX_NOHI, "64 -> 64 16-bit layers rebuild d(columns) from dy inside both consumers (no [M][9C] matrix in memory)") \
    X(dcn_bt_fuse_wgrad, 1, MFX_NOLO, MFX_NOHI, "64 -> 64 bf16 layers accumulate grad_weight inside the sample kernel (no columns in memory)") \
    X(dcn_bt_fuse_min_chunks, 1024, 1, MFX_NOHI, "fewer 32-pixel chunks than this keep the unfused kernels (tests lower it)") \
    X(dcn_bt_cs, 0, MFX_NOLO, MFX_NOHI, "channel slice of the tile kernel for C >= 128 (0 = by workgroup count, 64, 128)") \
    X(dcn_bt_cs_wgs, 1000, MFX_NOLO, MFX_NOHI, "below this many 128-channel workgroups the tile kernel takes 64-channel slices") \
    /* whole training path */ \
    X(deterministic, 0, MFX_NOLO, MFX_NOHI, "any non-zero value = 1: every floating-point reduction of the training path runs in a fixed order (single-writer partial " \
        "sums, one pixel slab per weight-gradient tile, 64-bit fixed-point accumulation of the DCN input gradient) so that two runs -- eager or replayed from a " \
        "hipGraph -- produce bit-identical results.  Slower; the default (0) keeps the atomics")

// Timing probes with WRONG results by design.  The variables always exist; mfx_set_option knows the names in probe builds only
// (MFX_PROBES=1 python -m monoflex_amd.build) and answers MFX_ERR_UNSUPPORTED otherwise.
#define MFX_PROBE_OPTION_LIST(X) \
    X(dcn_bt_dbg, 0, MFX_NOLO, MFX_NOHI, "experiment switches of dcn_bwd_tile_kernel (0 in production)") \
    X(heads_dbg, 0, MFX_NOLO, MFX_NOHI, "timing probes of the bf16 heads kernel (see DBG in heads.hip)")

// X(name, "what is counted"): host-side counts since process start of what the dispatchers chose
#define MFX_COUNTER_LIST(X) \
    /* mfx_dcn_nhwc / mfx_conv2d_nhwc: launches of each kernel family */ \
    X(dcn_lds, "launches of the fourth-generation DCN kernel (dcn_lds.hip) on 16-bit maps") \
    X(dcn_lds_of, "those of dcn_lds that computed the offset/mask conv themselves") \
    X(dcn_lds_split, "launches of dcn_lds.hip in split precision (not counted in dcn_lds)") \
    X(dcn_patch, "launches of the third-generation, LDS-patch DCN kernel (dcn_patch.hip)") \
    X(dcn_wave, "launches of the second-generation DCN kernel (dcn_wave.hip)") \
    X(dcn_gather, "launches of the first-generation fused gather DCN kernel (conv_kernels.hip)") \
    X(dcn_group, "calls of mfx_dcn_module_group that ran a group (two launches: the grouped offset/mask conv, the grouped gather kernel; " \
        "neither is counted in conv_cw / dcn_gather)") \
    X(conv_cw, "launches of the compile-time-geometry 3x3 kernel (conv_cw.hip)") \
    X(conv_cws, "launches of its split-precision form (conv_cws.hip)") \
    X(conv_halo, "launches of the LDS-staged halo kernel (conv_halo.hip)") \
    X(conv_igemm, "launches of the generic implicit-GEMM kernel (conv_kernels.hip)") \
    X(conv_splitk, "those that ran split-K") \
    X(conv_bn_stats, "convolutions whose epilogue accumulated the BatchNorm statistics") \
    X(edge_chain, "launches of the edge fusion's one-kernel conv chain (edge_chain.hip)") \
    X(box_nms, "launches of the duplicate suppression (box_nms.hip): one per mfx_box_nms call that had rows, whatever B") \
    X(decode_multi, "launches of the several-modes-and-oracle box decode (decode_multi.hip): one per mfx_decode_boxes_multi call with B > 0") \
    /* training-side families */ \
    X(wgrad_patch, "weight gradients by the LDS-patch kernel (wgrad_tr.hip)") \
    X(wgrad_tr, "weight gradients by the transposed-read kernel (wgrad_tr.hip)") \
    X(wgrad_mfma, "weight gradients by the first-generation MFMA kernel (train_kernels.hip)") \
    X(wgrad_valu, "weight gradients by the VALU kernel") \
    X(wgrad_reduce, "launches of the pass that sums their partial tiles (wgrad_reduce_kernel)") \
    X(stem_wgrad, "launches of the stem's weight-gradient kernel") \
    X(bn_fwd_onepass, "train-mode BatchNorm forwards in one launch") \
    X(bn_bwd_onepass, "BatchNorm backwards in one launch") \
    X(bn_fwd_two, "BatchNorm forwards in the two-launch form") \
    X(bn_bwd_two, "BatchNorm backwards in the two-launch form") \
    X(dcn_bt_fly, "DCN backward calls that took the gcol-free form") \
    X(dcn_bt_fused, "launches of dcn_bwd_sample_wgrad_kernel") \
    X(dcn_bt_tile, "launches of dcn_bwd_tile_kernel") \
    X(dcn_bt_sample, "launches of dcn_bwd_sample_kernel") \
    X(dcn_bt_far, "launches of dcn_bwd_far_kernel + dcn_bwd_far_fly_kernel") \
    X(gram, "phase calls of mfx_gram_heads on 16-bit maps") \
    X(adamw_multi, "calls of mfx_adamw_multi") \
    X(optim_multi, "calls of mfx_optim_multi (the one-launch update with a rule / a gradient coefficient)") \
    X(optim_multi_sched, "calls of mfx_optim_multi_sched (the one-launch update reading beta1 from the device)") \
    X(grad_norm_multi, "calls of mfx_grad_norm_multi")

#define MFX_DECLARE_OPTION(name, def, lo, hi, doc) extern int g_opt_##name;
#define MFX_DECLARE_COUNTER(name, doc) extern long g_cnt_##name;
MFX_OPTION_LIST(MFX_DECLARE_OPTION)
MFX_PROBE_OPTION_LIST(MFX_DECLARE_OPTION)
MFX_COUNTER_LIST(MFX_DECLARE_COUNTER)
#undef MFX_DECLARE_OPTION
#undef MFX_DECLARE_COUNTER
