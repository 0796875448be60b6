# rocprofv3 kernel stats (two-stream default and single-stream) + bench line of one bench variant.
# usage: TAG=r04_cardiac ARGS="--variant cardiac --img 128 --batch 64" bash tests/tools/profile_variant.sh   -> $OUT/$TAG/
OUT=${OUT:-bench_out}   # output folder, relative to the repository root
set -e
T=${TAG:?}; R=$PWD
rm -rf $OUT/$T; mkdir -p $OUT/$T
timeout -k 10 300 python bench.py --full $ARGS --no-cpu-baseline > $OUT/$T/bench.json 2> $OUT/$T/bench.err
cut -c1-160 $OUT/$T/bench.json
cd /tmp && export TMPDIR=/tmp
timeout -k 10 300 rocprofv3 --kernel-trace --stats --output-format csv -d $R/$OUT/$T/stats -o run -- python3 $R/bench.py --full $ARGS --steps 4 --warmup 2 --no-cpu-baseline > $R/$OUT/$T/prof_cmd.json 2> $R/$OUT/$T/prof_cmd.err
export STIL_WGRAD_STREAM=0
timeout -k 10 300 rocprofv3 --kernel-trace --stats --output-format csv -d $R/$OUT/$T/stats_single_stream -o run -- python3 $R/bench.py --full $ARGS --steps 4 --warmup 2 --no-cpu-baseline > $R/$OUT/$T/prof_cmd_single_stream.json 2> $R/$OUT/$T/prof_cmd_single_stream.err
unset STIL_WGRAD_STREAM
cd $R
find $OUT/$T -name "*kernel_trace.csv" -size +20M -delete
for d in stats stats_single_stream; do f=$(find $OUT/$T/$d -name "*kernel_stats.csv" | head -1); [ -n "$f" ] && cp $f $OUT/$T/${T}_kernel_stats_$d.csv; done
ls $OUT/$T
