#!/bin/bash
# A/B of the visit's short forms (csrc/pcp_visit_forms.hpp) against a parent build of libpcp_hip.so, on one box:
#   bash profiles/visit_forms_probe.sh <parent libpcp_hip.so> [out dir]
# ab_step.py and bench.py --steps 100 alternating (five runs each), one counter pass and one kernel trace per library (never
# together), the dumps of both compared.  Every GPU step has its own time limit; a fault, an abort or a time limit ends the script.
set -uo pipefail
PARENT=$(readlink -f "$1")
OUT=${2:-profiles/visit_forms_probe_out}
mkdir -p "$OUT"
run() {  # run <seconds> <log> cmd...
  local t=$1 log=$2; shift 2
  timeout -k 10 "$t" "$@" > "$log" 2>&1
  local rc=$?
  [ $rc -eq 0 ] || { echo "rc=$rc $log"; tail -20 "$log"; exit $rc; }
}
for i in 1 2 3 4 5; do
  PCP_HIP_LIBRARY=$PARENT run 200 "$OUT/ab_parent_$i.json" python3 profiles/ab_step.py
  run 200 "$OUT/ab_tree_$i.json" python3 profiles/ab_step.py
  PCP_HIP_LIBRARY=$PARENT run 200 "$OUT/bench_parent_$i.json" python3 bench.py --gpus 1 --steps 100 --warmup 5
  run 200 "$OUT/bench_tree_$i.json" python3 bench.py --gpus 1 --steps 100 --warmup 5
done
PCP_HIP_LIBRARY=$PARENT run 300 "$OUT/dump_parent.log" python3 bench.py --gpus 1 --steps 20 --warmup 5 --dump-outputs "$OUT/dump_parent"
run 300 "$OUT/dump_tree.log" python3 bench.py --gpus 1 --steps 20 --warmup 5 --dump-outputs "$OUT/dump_tree"
python3 - "$OUT" <<'PY'
import sys
import numpy as np
for k in ("index", "rgb", "has"):
    a, b = (np.load(f"{sys.argv[1]}/dump_{w}/{k}.npy") for w in ("parent", "tree"))
    print("dump", k, a.shape, "equal" if np.array_equal(a, b) else "DIFFERENT")
PY
BENCH="python3 bench.py --gpus 1 --steps 10 --warmup 2"
PCP_HIP_LIBRARY=$PARENT run 300 "$OUT/pmc_parent.log" rocprofv3 --pmc SQ_INSTS_VALU SQ_INSTS_SALU SQ_WAVES --output-format csv -d "$OUT/pmc_parent" -- $BENCH
run 300 "$OUT/pmc_tree.log" rocprofv3 --pmc SQ_INSTS_VALU SQ_INSTS_SALU SQ_WAVES --output-format csv -d "$OUT/pmc_tree" -- $BENCH
PCP_HIP_LIBRARY=$PARENT run 300 "$OUT/trace_parent.log" rocprofv3 --kernel-trace --stats --output-format csv -d "$OUT/trace_parent" -- $BENCH
run 300 "$OUT/trace_tree.log" rocprofv3 --kernel-trace --stats --output-format csv -d "$OUT/trace_tree" -- $BENCH
python3 - "$OUT" <<'PY'
import collections, csv, glob, re, sys
out = sys.argv[1]
for which in ("parent", "tree"):
    s = collections.defaultdict(lambda: collections.defaultdict(float)); n = collections.defaultdict(lambda: collections.defaultdict(int))
    for fn in glob.glob(f"{out}/pmc_{which}/**/*_counter_collection.csv", recursive=True):
        for r in csv.DictReader(open(fn)):
            k = re.sub(r"^void ", "", r["Kernel_Name"].split("(")[0])
            s[k][r["Counter_Name"]] += float(r["Counter_Value"]); n[k][r["Counter_Name"]] += 1
    for k in s:
        if "k_depth_pass" in k or "k_colour_pass" in k:
            print(which, k, {c: round(s[k][c] / n[k][c]) for c in s[k]}, "launches", max(n[k].values()))
    for fn in glob.glob(f"{out}/trace_{which}/**/*kernel_stats.csv", recursive=True):
        for r in csv.DictReader(open(fn)):
            if "k_depth_pass" in r["Name"] or "k_colour_pass" in r["Name"] or "k_tile_mask" in r["Name"]:
                print(which, r["Name"].split("(")[0], "calls", r["Calls"], "average ns", r["AverageNs"])
PY
