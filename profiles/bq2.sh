# front-end timing of a bench configuration (measurement helper): bash profiles/bq2.sh CONFIG [ENV=VAL ...]
export CSDR_BUILD_LAB=1
cfg=$1; shift
for kv in "$@"; do export "$kv"; done
mkdir -p bench_out
python bench.py --full --config $cfg --steps 3 --warmup 2 --cpu-seconds 0 --no-latency --no-strong > bench_out/bq.json 2> bench_out/bq.err; python -c "
import json; d=json.load(open('bench_out/bq.json')); r=d['roofline']; print('$cfg $*', round(d['value']), {k:round(v,4) for k,v in r['kernels_ms_per_batch'].items() if k.startswith('demod_front')})"
