OUT=${OUT:-$(mktemp -d)}; mkdir -p "$OUT"
S=$(date +%s)
python3 bench.py --full > "$OUT/bench_final.json" 2> "$OUT/bench_final.err"
echo "rc $? elapsed $(( $(date +%s) - S )) s"
tail -3 "$OUT/bench_final.err"
python3 - "$OUT/bench_final.json" <<'PY'
import json, sys
d=json.loads(open(sys.argv[1]).read().strip().splitlines()[-1])
r=d["roofline"]; print(d["value"], r["frac"], r["kernel_ms"], r["traffic"])
c=d["other_kernels"]["config3_end_to_end"]; print(c.get("cpu_baseline_at_full_size")); print(c.get("parity"))
PY
