# One profiling round of the bench command on the GPU box: bench line, rocprofv3 kernel stats (default = two streams, and
# single stream), HBM traffic (FETCH_SIZE / WRITE_SIZE, separate passes) and MFMA utilisation (SQ counters) of the GEMM
# kernels.  usage: TAG=r02a bash tests/tools/profile_round.sh   -> $OUT/$TAG/ (copy what is to be judged to profiles/)
OUT=${OUT:-bench_out}   # output folder, relative to the repository root
set -e
T=${TAG:-r02}
rm -rf $OUT/$T
mkdir -p $OUT/$T
timeout -k 10 500 python bench.py --full > $OUT/$T/bench_default.json 2> $OUT/$T/bench_default.err
cut -c1-400 $OUT/$T/bench_default.json
KERNEL=$(python -c "import json,sys; print(json.load(open('$OUT/$T/bench_default.json'))['roofline']['kernel'])")
echo "dominant kernel: $KERNEL"
R=$PWD
cd /tmp && export TMPDIR=/tmp
CMD="bench.py --full --steps 3 --warmup 1 --no-cpu-baseline"
timeout -k 10 300 rocprofv3 --kernel-trace --stats --output-format csv -d $R/$OUT/$T/stats -o run -- python3 $R/bench.py --full --steps 3 --warmup 1 --no-cpu-baseline > $R/$OUT/$T/prof_cmd.json 2> $R/$OUT/$T/prof_cmd.err
# single-stream passes: per-kernel durations / counters without a concurrent kernel on the side stream
export STIL_WGRAD_STREAM=0
timeout -k 10 300 rocprofv3 --kernel-trace --stats --output-format csv -d $R/$OUT/$T/stats_single_stream -o run -- python3 $R/bench.py --full --steps 3 --warmup 1 --no-cpu-baseline > $R/$OUT/$T/prof_cmd_single_stream.json 2> $R/$OUT/$T/prof_cmd_single_stream.err
timeout -k 10 300 rocprofv3 --pmc FETCH_SIZE --output-format csv -d $R/$OUT/$T/pmc_fetch -o run -- python3 $R/bench.py --full --steps 2 --warmup 1 --no-cpu-baseline > $R/$OUT/$T/pmc_fetch.json 2> $R/$OUT/$T/pmc_fetch.err
timeout -k 10 300 rocprofv3 --pmc WRITE_SIZE --output-format csv -d $R/$OUT/$T/pmc_write -o run -- python3 $R/bench.py --full --steps 2 --warmup 1 --no-cpu-baseline > $R/$OUT/$T/pmc_write.json 2> $R/$OUT/$T/pmc_write.err
timeout -k 10 300 rocprofv3 --pmc SQ_VALU_MFMA_BUSY_CYCLES SQ_BUSY_CU_CYCLES GRBM_GUI_ACTIVE --output-format csv -d $R/$OUT/$T/pmc_mfma -o run -- python3 $R/bench.py --full --steps 2 --warmup 1 --no-cpu-baseline > $R/$OUT/$T/pmc_mfma.json 2> $R/$OUT/$T/pmc_mfma.err
unset STIL_WGRAD_STREAM
cd $R
set +e
python tests/tools/pmc_traffic.py $OUT/$T/pmc_fetch $OUT/$T/pmc_write $OUT/$T/$T "$KERNEL" "STIL_WGRAD_STREAM=0 $CMD" $OUT/$T/bench_default.json | head -14
python tests/tools/mfma_util.py $OUT/$T/pmc_mfma $OUT/$T/${T}_mfma_util.json "STIL_WGRAD_STREAM=0 bench.py --full --steps 2 --warmup 1 --no-cpu-baseline" | head -40
find $OUT/$T -name "*kernel_trace.csv" -size +20M -delete
find $OUT/$T -name "*counter_collection.csv" -size +20M -delete
for d in stats stats_single_stream; do f=$(find $OUT/$T/$d -name "*kernel_stats.csv" | head -1); [ -n "$f" ] && cp $f $OUT/$T/${T}_bench_kernel_stats_$d.csv; done
ls -la $OUT/$T | head -40
if [ -n "$OTHER_SHAPES" ]; then   # the other measurement shapes of SURVEY.md 8(d)
  timeout -k 10 200 python bench.py --full --variant saint --no-cpu-baseline > $OUT/$T/bench_saint.json 2>/dev/null
  timeout -k 10 200 python bench.py --full --img 128 --ncat 4 --ncon 13 --no-cpu-baseline > $OUT/$T/bench_native128.json 2>/dev/null
  timeout -k 10 200 python bench.py --full --variant cardiac --img 128 --batch 64 --no-cpu-baseline > $OUT/$T/bench_cardiac.json 2>/dev/null
  timeout -k 10 200 python bench.py --full --batch 32 --no-cpu-baseline > $OUT/$T/bench_b32.json 2>/dev/null
  timeout -k 10 200 python bench.py --full --variant cardiac --img 128 --batch 16 --no-cpu-baseline > $OUT/$T/bench_cardiac16.json 2>/dev/null
  for f in saint native128 cardiac b32 cardiac16; do cut -c1-200 $OUT/$T/bench_$f.json; done
fi
