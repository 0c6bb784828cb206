# Round artefacts of the current HEAD: the full bench line (`bench.py --full`: all legs) and the B=32 / training / split-precision
# lines under $ART (default: artifacts/), rocprofv3 kernel summaries of the inference and training steps, the PMC passes of the heads kernel and of the DCN backward group.
mkdir -p gpurun_out; export TMPDIR=/tmp; R=$GRAFT_REPO_ROOT; cd $R
ART=${ARTIFACT_DIR:-artifacts}; mkdir -p $ART
timeout 900 python bench.py --full > $ART/${RTAG:-r05}_bench_default.json 2> $ART/${RTAG:-r05}_bench_default.err; cut -c1-200 $ART/${RTAG:-r05}_bench_default.json; echo
timeout 600 python bench.py --full --batch 32 --no-cpu-baseline --legs none > $ART/${RTAG:-r05}_bench_infer_b32.json 2>/dev/null; cut -c1-200 $ART/${RTAG:-r05}_bench_infer_b32.json; echo
timeout 600 python bench.py --full --dtype fp16x2 --no-cpu-baseline --legs none > $ART/${RTAG:-r05}_bench_infer_fp16x2.json 2>/dev/null; cut -c1-200 $ART/${RTAG:-r05}_bench_infer_fp16x2.json; echo
timeout 900 python bench.py --full --mode train > $ART/${RTAG:-r05}_bench_train.json 2> $ART/${RTAG:-r05}_bench_train.err; cut -c1-200 $ART/${RTAG:-r05}_bench_train.json; echo
cd /tmp && rm -rf /tmp/prof_inf && timeout 400 rocprofv3 --kernel-trace --stats -d /tmp/prof_inf -o prof -- python $R/bench.py --legs none --no-cpu-baseline --no-families --steps 20 --repeats 1 > $R/gpurun_out/prof_inf.log 2>&1
cd $R; python tools/prof_summary.py $(find /tmp/prof_inf -name "*.db" | head -1) > gpurun_out/${RTAG:-r05}_b_inference_kernel_stats.md; head -8 gpurun_out/${RTAG:-r05}_b_inference_kernel_stats.md | cut -c1-140
bash tools/profile_infer_step.sh > /dev/null 2>&1; head -6 gpurun_out/${RTAG:-r05}_b_inference_replay_kernel_timeline.md | cut -c1-140
bash tools/profile_train_step.sh > /dev/null 2>&1; head -6 gpurun_out/${RTAG:-r05}_a_train_step_kernel_stats.md | cut -c1-140
bash tools/pmc_heads.sh ${RTAG:-r05} > /dev/null 2>&1; cat gpurun_out/${RTAG:-r05}_heads_traffic.json
bash tools/pmc_dcnbwd.sh ${RTAG:-r05} > /dev/null 2>&1; cat gpurun_out/${RTAG:-r05}_dcnbwd_traffic.json
