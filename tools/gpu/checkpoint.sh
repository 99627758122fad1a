# round checkpoint: full -m gpu suite, smoke, default bench (traffic + cpu baseline), fp16 preact+ASPP bench
# (traffic + cpu baseline), rocprofv3 kernel stats of both benches
# (the fp16 kernel stats are taken serialised, UPR_MS_STREAMS=0: see DESIGN §3, two streams per forward)
cd /tmp && export TMPDIR=/tmp && cd $GRAFT_REPO_ROOT
out=${OUT:-bench_out}/${CK:-ck}
mkdir -p $out
timeout -k 10 700 python -u -m pytest tests -m gpu -v -s --timeout 200 --timeout-method thread -p no:cacheprovider > $out/gpu_tests.log 2>&1
rc=$?
echo "pytest rc=$rc"; tail -5 $out/gpu_tests.log
if [ $rc -ne 0 ] && [ $rc -ne 1 ]; then exit $rc; fi
timeout -k 10 200 python -c "import __graft_entry__ as g; g.smoke()" > $out/smoke.log 2>&1 || exit $?
timeout -k 10 400 python bench.py --full > $out/bench_default.json 2> $out/bench_default.err || exit $?
cat $out/bench_default.json
timeout -k 10 400 python bench.py --full --precision fp16 --variant preact_aspp --ceilings --no-nested > $out/bench_fp16.json 2> $out/bench_fp16.err || exit $?
cat $out/bench_fp16.json
timeout -k 10 200 rocprofv3 --kernel-trace --stats -d $out/prof -o p --output-format csv -- python3 bench.py --steps 10 --warmup 3 --no-traffic --cpu-seconds 0 --no-nested > $out/bench_prof.json 2>&1 || exit $?
timeout -k 10 300 python bench.py --full --train --amp --steps 5 --warmup 2 --no-nested > $out/bench_train.json 2> $out/bench_train.err || exit $?
UPR_MS_STREAMS=0 timeout -k 10 200 rocprofv3 --kernel-trace --stats -d $out/prof16 -o p --output-format csv -- python3 bench.py --precision fp16 --variant preact_aspp --steps 20 --warmup 3 --no-traffic --cpu-seconds 0 --no-nested > $out/bench_prof16.json 2>&1 || exit $?
exit $rc
