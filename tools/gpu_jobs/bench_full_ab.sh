# Whole bench.py --full lines (4K headline + 1080p + 8K + variants) for
# libbmfr variants (BMFR_LIB), interleaved; the lines go to $BENCH_OUT
# (default bench_out/).
#   bash tools/gpu_jobs/bench_full_ab.sh base variant...
set -o pipefail
O=${BENCH_OUT:-bench_out}
mkdir -p $O
for v in "$@"; do
  lib=$v; [ "$v" = base ] && lib=""
  BMFR_LIB=$lib BMFR_ALLOW_FOREIGN_BUILD=1 timeout -k 10 500 python bench.py --full --cpu-frames 0 > $O/full_$v.json 2> $O/full_$v.err || exit $?
  python - "$v" "$O" <<'PY'
import json, sys
v, o = sys.argv[1:3]
d = json.loads(open(f"{o}/full_{v}.json").read().strip().splitlines()[-1])
keys = [k for k in d if k.startswith("ms_per_frame")]
print(v, "value", d["value"], d["kernel_ms"], {k: d[k]["value"] if isinstance(d[k], dict) else d[k] for k in keys})
PY
done
