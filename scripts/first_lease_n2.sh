#!/bin/bash
# First multi-GPU lease (N >= 2 MI355X on one node): everything that has only ever run as a one-GPU rehearsal, in one
# command, with a JSON verdict.  Nothing here can run on the one-GPU boxes of the build pool.
#
#   bash scripts/first_lease_n2.sh [N]        (from the repo root; N defaults to 2)
#
#  1. bench.py --full --gpus N --verify under torch.distributed.run: RCCL all-reduce(MIN) of the depth maps, all-gather of the
#     keyframes over xGMI; the gathered colours must equal a one-GPU run of the same seeded map (verify.equal_to_one_gpu_run).
#     The same line times the two stages that need the whole map on every GPU (sharded_legs): hidden_points_removal over the
#     ranks (hulls of each rank's block of keyframes, all-gather of the verdicts on device memory, import into the index
#     shards: hpr_ms) and the smoothing stage (outlier removal + MLS, queries dealt out by slabs: smooth_ms).
#  2. the C++ host: PointCloudProcessor --gpus N against --gpus 1 on a generated scene, every output file byte for byte
#     (ncclCommInitAll, grouped ncclAllReduce(ncclMin), ncclBroadcast of the images, ncclAllReduce(ncclSum) of the NID
#     histograms with --enableNIDOptimize 1).
#     Also --cull hpr (the hulls taken on whole-map contexts, keyframe f on GPU f mod N, slices of the verdicts sent to the
#     shards by grouped ncclSend / ncclRecv on device memory) and
#     --enableMLS 1 (both outlier-removal brackets, MLS queries and voxel chunks dealt out): --gpus N against --gpus 1.
#  3. the RCCL plumbing tests of the suite (device-pointer all-reduce on the library's stream).
set -u -o pipefail
N=${1:-2}
R=$(cd "$(dirname "$0")/.." && pwd)
OUT=$R/gpurun_out/first_lease
mkdir -p "$OUT"
export MASTER_ADDR=127.0.0.1 HSA_ENABLE_IPC_MODE_LEGACY=0
cd "$R"
python3 -c "import __graft_entry__ as g; g.build()" > "$OUT/build.log" 2>&1 || { echo '{"ok": false, "stage": "build"}' > "$OUT/verdict.json"; exit 1; }

# 1 -- bench, sharded, verified
python3 -m torch.distributed.run --nnodes=1 --nproc-per-node "$N" --master-addr 127.0.0.1 --master-port 29555 bench.py --full \
  --gpus "$N" --steps 10 --warmup 3 --verify > "$OUT/bench_n$N.json" 2> "$OUT/bench_n$N.err"
RC_BENCH=$?
python3 bench.py --gpus 1 --steps 20 --warmup 5 --no-side-legs > "$OUT/bench_n1.json" 2> "$OUT/bench_n1.err"

# 2 -- the C++ host, N GPUs against one
python3 - "$OUT" <<'PY'
import os, sys
import numpy as np
sys.path.insert(0, os.getcwd())
from pointcloudprocessor_amd import synth
out = sys.argv[1]
scene = os.path.join(out, "scene")
os.makedirs(scene, exist_ok=True)
x, y, z, inten = synth.make_cloud(400_000, seed=3)
n = len(x)
hdr = ("# .PCD v0.7 - Point Cloud Data file format\nVERSION 0.7\nFIELDS x y z intensity\nSIZE 4 4 4 4\nTYPE F F F F\n"
       f"COUNT 1 1 1 1\nWIDTH {n}\nHEIGHT 1\nVIEWPOINT 0 0 0 1 0 0 0\nPOINTS {n}\nDATA binary\n")
with open(os.path.join(scene, "scans.pcd"), "wb") as f:
    f.write(hdr.encode())
    f.write(np.stack([x, y, z, inten], 1).astype(np.float32).tobytes())
poses, ts = synth.make_trajectory(6)
W, H = 1024, 750
with open(os.path.join(scene, "odo.txt"), "w") as f:
    for k, (t, p) in enumerate(zip(ts, poses)):
        f.write(synth.odometry_line(t, p))
        img = synth.make_image(k, W, H)
        with open(os.path.join(scene, "%f.ppm" % t), "wb") as g:
            g.write(b"P6\n%d %d\n255\n" % (W, H) + img[:, :, ::-1].tobytes())
PY
EXE=$R/pointcloudprocessor_amd/host/bin/PointCloudProcessor
RC_CLI=0
for G in 1 "$N"; do
  for NID in 0 1; do
    D=$OUT/cli_g${G}_nid${NID}; rm -rf "$D"; mkdir -p "$D"
    (cd "$D" && "$EXE" -p "$OUT/scene/scans.pcd" -o "$OUT/scene/odo.txt" -i "$OUT/scene/" -t "$D/" --gpus "$G" \
        --enableNIDOptimize "$NID" > "$D/stdout.log" 2> "$D/stderr.log") || RC_CLI=1
  done
done
diff -rq -x stdout.log -x stderr.log -x T_camera_lidar_optimized.txt "$OUT/cli_g1_nid0" "$OUT/cli_g${N}_nid0" > "$OUT/cli_diff_nid0.txt" 2>&1; D0=$?
# the NID refinement sums fp64 histograms in a different order on N GPUs: the optimum agrees to ~1e-5, the files may not
diff -rq -x stdout.log -x stderr.log -x T_camera_lidar_optimized.txt "$OUT/cli_g1_nid1" "$OUT/cli_g${N}_nid1" > "$OUT/cli_diff_nid1.txt" 2>&1; D1=$?

# hidden_points_removal and the smoothing stage over the GPUs
for G in 1 "$N"; do
  D=$OUT/cli_g${G}_hpr; rm -rf "$D"; mkdir -p "$D"
  (cd "$D" && "$EXE" -p "$OUT/scene/scans.pcd" -o "$OUT/scene/odo.txt" -i "$OUT/scene/" -t "$D/" --gpus "$G" --cull hpr \
      > "$D/stdout.log" 2> "$D/stderr.log") || RC_CLI=1
  D=$OUT/cli_g${G}_mls; rm -rf "$D"; mkdir -p "$D"
  (cd "$D" && "$EXE" -p "$OUT/scene/scans.pcd" -o "$OUT/scene/odo.txt" -i "$OUT/scene/" -t "$D/" --gpus "$G" --enableMLS 1 \
      --mlsUpsampling none --skip_filtered_dumps 1 > "$D/stdout.log" 2> "$D/stderr.log") || RC_CLI=1
done
diff -rq -x stdout.log -x stderr.log "$OUT/cli_g1_hpr" "$OUT/cli_g${N}_hpr" > "$OUT/cli_diff_hpr.txt" 2>&1; DH=$?
# the smoothed coordinates may differ in their last fp32 bit (re-uploaded intermediate clouds: another summation order)
diff -rq -x stdout.log -x stderr.log "$OUT/cli_g1_mls" "$OUT/cli_g${N}_mls" > "$OUT/cli_diff_mls.txt" 2>&1; DM=$?

# 3 -- the RCCL plumbing tests
python3 -m pytest tests/test_rccl_plumbing_gpu.py -x -q -m gpu > "$OUT/pytest.log" 2>&1
RC_TEST=$?

python3 - "$OUT" "$N" "$RC_BENCH" "$RC_CLI" "$D0" "$D1" "$RC_TEST" "$DH" "$DM" <<'PY'
import json, os, sys
out, n, rc_bench, rc_cli, d0, d1, rc_test, dh, dm = sys.argv[1], int(sys.argv[2]), *map(int, sys.argv[3:10])
def line(p):
    try:
        return json.loads([l for l in open(p).read().splitlines() if l.startswith("{")][-1])
    except Exception as e:
        return {"error": str(e)}
bn, b1 = line(os.path.join(out, f"bench_n{n}.json")), line(os.path.join(out, "bench_n1.json"))
v = {"n_gpus": n, "bench_rc": rc_bench, "bench_value": bn.get("value"), "bench_ms_per_step": bn.get("ms_per_step"),
     "bench_verify": bn.get("verify"), "bench_n1_value": b1.get("value"), "cli_rc": rc_cli,
     "hpr_ms": ((bn.get("sharded_legs") or {}).get("hpr") or {}).get("hpr_ms"),
     "hpr_exchange_ms": ((bn.get("sharded_legs") or {}).get("hpr") or {}).get("exchange_ms_max_rank"),
     "hpr_shards_equal_owner": ((bn.get("sharded_legs") or {}).get("hpr") or {}).get("keyframe0_shards_equal_owner"),
     "smooth_ms": ((bn.get("sharded_legs") or {}).get("smooth") or {}).get("smooth_ms"),
     "parity_gate": bn.get("parity_gate"),
     "cli_outputs_identical_to_one_gpu": d0 == 0, "cli_nid_outputs_identical_to_one_gpu": d1 == 0,
     "cli_hpr_outputs_identical_to_one_gpu": dh == 0, "cli_mls_outputs_identical_to_one_gpu": dm == 0, "pytest_rc": rc_test}
v["ok"] = bool(rc_bench == 0 and (bn.get("verify") or {}).get("equal_to_one_gpu_run") and rc_cli == 0 and d0 == 0 and dh == 0)
json.dump(v, open(os.path.join(out, "verdict.json"), "w"), indent=1)
print(json.dumps(v))
PY
