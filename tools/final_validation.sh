# Round-end validation on a machine with an MI355X (run from the repo root): the GPU test selection with its durations,
# smoke(), the full bench line, a rocprofv3 kernel trace of the same command (per-kernel averages, the prefill step's
# timeline and edges), and the FETCH_SIZE / WRITE_SIZE passes.  SLOW=1 adds the gpu_slow twins to the test run.
# Results under $OUT_DIR/final (default: bench_out/final in the repo root).
set -x
R=$PWD
O=$(realpath -m "${OUT_DIR:-$R/bench_out}")/final
mkdir -p $O
SEL="gpu"; [ -n "$SLOW" ] && SEL="gpu or gpu_slow"
timeout 1500 python -m pytest tests -q -m "$SEL" --durations=15 2>&1 | tail -24 > $O/pytest_gpu.txt
timeout 300 python -c "import __graft_entry__ as g; g.smoke()" 2>&1 | tail -2 > $O/smoke.txt
timeout 600 python bench.py --full 2>&1 | grep '^{"metric"' > $O/bench.json
for i in 1 2 3 4 5; do  # the plain command as every change is measured with it, five fresh processes (the first with rooflines and CPU baseline)
  extra=""; [ "$i" = 1 ] && extra="--full"
  timeout 600 python3 bench.py --gpus 1 --steps 20 --warmup 5 $extra 2>/dev/null | grep '^{"metric"' > $O/bench_driver_cmd_$i.json
done
OUT_DIR=$(dirname $O) bash tools/serving_round.sh final > $O/serving_summary.txt 2>&1
cd /tmp && export TMPDIR=/tmp
# (--full: the roofline loop's 560 attention launches are the tail of the run that `--last ... 560` summarises)
timeout 600 rocprofv3 --kernel-trace --stats -d /tmp/prof_kt -- python $R/bench.py --full --no-cpu-baseline > /tmp/log_kt 2>&1
grep '^{"metric"' /tmp/log_kt > $O/bench_under_kernel_trace.json
db=$(find /tmp/prof_kt -name "*.db" | head -1)
python $R/tools/prof_db.py $db 40 > $O/kernel_trace.txt
python $R/tools/prof_db.py $db --last paged_attn_decode_kernel 560 >> $O/kernel_trace.txt
python $R/tools/prof_db.py $db --window paged_attn_prefill_kernel 28 "prefill step, 16 x 1024 tokens" > $O/prefill_step_breakdown.txt
python $R/tools/prof_db.py $db --edges paged_attn_prefill_kernel 28 > $O/prefill_step_edges.txt
python $R/tools/prof_db.py $db --layers paged_attn_prefill_kernel 28 2 > $O/prefill_steps_layer_by_layer.txt
for c in FETCH_SIZE WRITE_SIZE; do
  timeout 600 rocprofv3 --pmc $c --kernel-trace -d /tmp/prof_$c -- python $R/bench.py --full --no-cpu-baseline > /tmp/log_$c 2>&1
  db=$(find /tmp/prof_$c -name "*.db" | head -1)
  python $R/tools/prof_pmc.py $db 12 > $O/pmc_$c.txt
  python $R/tools/prof_pmc.py $db --last paged_attn_decode_kernel 560 >> $O/pmc_$c.txt
done
cd $R
python tools/attn_traffic_json.py $O/pmc_FETCH_SIZE.txt $O/pmc_WRITE_SIZE.txt \
  $O/bench_under_kernel_trace.json $O/attn_traffic.json > /dev/null
ls -la $O; cat $O/pytest_gpu.txt $O/smoke.txt; head -c 700 $O/bench.json; cat $O/prefill_step_breakdown.txt; tail -2 $O/pmc_FETCH_SIZE.txt; tail -1 $O/pmc_WRITE_SIZE.txt
