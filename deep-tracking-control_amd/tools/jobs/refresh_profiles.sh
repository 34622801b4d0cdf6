# usage: bash refresh_profiles.sh OUT_DIR   (run from the repository root; everything lands in OUT_DIR)
R=$PWD
O=$(mkdir -p "${1:?output directory}" && cd "$1" && pwd)
timeout 1500 python -m pytest tests -m gpu -q -x 2>&1 | tail -3
timeout 900 python bench.py --full > $O/r01_bench_n1.json 2> $O/r01_bench_n1.err; tail -2 $O/r01_bench_n1.err
cd /tmp && export TMPDIR=/tmp
rm -rf $O/rp_serial $O/rp_overlap
DTC_OVERLAP_WGRAD=0 timeout 600 rocprofv3 --kernel-trace --stats -d $O/rp_serial -o bench --output-format csv -- python $R/bench.py --full --steps 3 --warmup 1 --no-cpu-baseline > $O/rp_serial.json 2> $O/rp_serial.err
timeout 600 rocprofv3 --kernel-trace --stats -d $O/rp_overlap -o bench --output-format csv -- python $R/bench.py --full --steps 3 --warmup 1 --no-cpu-baseline > $O/rp_overlap.json 2> $O/rp_overlap.err
ls $O/rp_serial $O/rp_overlap
python - <<PY
import json
for f in ('r01_bench_n1','rp_serial','rp_overlap'):
    d=json.load(open('$O/'+f+'.json'))
    print(f, d['value'], d['ms_per_step'], d['roofline']['achieved'], d['roofline']['avg_launch_us'], d.get('cpu_baseline',{}).get('value'))
PY
cd $R
for w in gru composite; do
timeout 600 python bench.py --full --workload $w --steps 3 --warmup 1 --no-cpu-baseline > $O/r01_bench_$w.json 2>/dev/null
python -c "import json; d=json.load(open('$O/r01_bench_$w.json')); print('$w', d['value'], d['ms_per_step'], d['roofline']['achieved'])"
done
