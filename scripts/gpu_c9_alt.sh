A=$PWD/pymarl_amd/lib/libmq_learner_alt.so
O=${MQ_OUT:-$PWD/out}; mkdir -p $O
MQ_LEARNER_LIB=$A timeout -k 10 300 python -u -m pytest -q --timeout 200 --timeout-method thread -m gpu tests/test_gpu_coma.py > $O/c9_alt_tests.log 2>&1; tail -3 $O/c9_alt_tests.log
for i in 1 2; do for v in head alt; do E=""; [ $v = alt ] && E="MQ_LEARNER_LIB=$A"; env $E timeout -k 10 200 python bench.py --config cfg5 --steps 10 --warmup 2 --full --no-cpu-baseline > $O/c9_bench_${v}_$i.json 2>/dev/null || exit 1; python -c "import json;d=json.load(open('$O/c9_bench_${v}_$i.json'));print('$v $i', round(d['ms_per_step'],4), d['roofline'].get('phases_ms'))"; done; done
