# Scratch: the full bench run (--full) with its wall time and the wall time of every optional leg (run from the repo root on the GPU box).
cd $GRAFT_REPO_ROOT
O=${1:-.}                     # where the line, stderr and the detail file go
t0=$(date +%s.%N)
python bench.py --full --detail $O/bench_detail.json > $O/bench_line.json 2> $O/bench.err
t1=$(date +%s.%N)
echo "bench.py wall: $(echo "$t1 - $t0" | bc) s, line $(wc -c < $O/bench_line.json) bytes"
python - $O/bench_detail.json <<'PY'
import json, sys
d = json.load(open(sys.argv[1]))
print("before cpu baseline", d.get("wall_s_before_cpu_baseline"))
for c in d.get("configs", []): print(c["name"], round(c.get("leg_wall_s", 0), 1), c.get("error", ""))
PY
