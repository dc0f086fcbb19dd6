#!/usr/bin/env python3
"""MovingLeastSquares with SAMPLE_LOCAL_PLANE upsampling (pcp_mls_process / pcp_cloud_smooth, upsampling 1) at the
reference's disk (0.05 m radius, 0.01 m step: 79 samples per fitted point) on a synthetic map of N points
(synth.make_cloud; C3 = 10 M).  One JSON line.  Not collected by pytest.  Run one map per process, each under its own time
limit:  python scripts/mls_slp_probe.py N [--shapes 0,1] [--oracle]

  fit_emit_ms       wall time of pcp_mls_process(SLP) on the uploaded map -- fit, compaction (one host sync) and emission --,
                    median of 3 after a warm-up call
  emit_ms / fit_ms  of that, the emission kernel alone (PCP_K_MLS_VOXEL) and the fit (PCP_K_MLS_FIT), per call
  emit_GBps         bytes the emission writes (32 B per row: xyz, normal, curvature, index) over emit_ms
  rows_before       rows of the chain's upsampled cloud: pcp_mls_process(SLP) on an upload of the first filter's survivors (the
                    filter with the parameters' sor_mean_k / sor_std_mul), which the chain's rows equal bit for bit
  sign_flips_reupload  fitted points whose NONE normal points the other way when the same survivors are uploaded in another
                    order (the upload re-sorts them, the fit's fp64 sums run in another order); bit_equal_normals_reupload
                    the points whose normal did not change in any bit.  --oracle: sign_flips_vs_oracle, the same count
                    against the CPU restatement
  chain_ms          wall time of pcp_cloud_smooth(SLP) (SOR -> MLS + SLP -> SOR), median of 3 after a warm-up call, per shape
                    of the last filter's selection (PCP_SOR_CLUSTERED=0 / 1; the library's choice is the plain shape);
                    chain_sor_ms = its outlier-removal kernels (PCP_K_SOR), rows_after = what the last filter keeps
"""
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from pointcloudprocessor_amd import capi, synth  # noqa: E402

REPS = 3


def _log(msg):
    print(f"[slp_probe {time.strftime('%H:%M:%S')}] {msg}", file=sys.stderr, flush=True)


def _median_call(ctx, fn, kernels):
    t0 = time.perf_counter()
    fn()  # warm-up (allocations)
    ctx.synchronize()
    _log(f"warm-up call {time.perf_counter() - t0:.2f} s")
    walls, per_k = [], {k: [] for k in kernels}
    for _ in range(REPS):
        ctx.timing_reset()
        ctx.timing_enable(True)
        t0 = time.perf_counter()
        out = fn()
        ctx.synchronize()
        walls.append((time.perf_counter() - t0) * 1e3)
        for k in kernels:
            per_k[k].append(ctx.timing_get(k)[0])
        ctx.timing_enable(False)
    return out, float(np.median(walls)), {k: float(np.median(v)) for k, v in per_k.items()}


def _normals_by_point(res, n, perm=None):
    out = np.zeros((n, 3), np.float64)
    idx = res["index"] if perm is None else perm[res["index"]]
    out[idx] = res["normal"]
    return out


def main():
    args = sys.argv[1:]
    n = int(args[0]) if args and not args[0].startswith("--") else 1_000_000
    shapes = args[args.index("--shapes") + 1].split(",") if "--shapes" in args else ["0", "1"]
    mp = capi.default_mls_params()
    mp.upsampling = capi.UPSAMPLING_SAMPLE_LOCAL_PLANE
    none_p = capi.default_mls_params()
    none_p.upsampling = capi.UPSAMPLING_NONE
    T = len(capi.mls_local_plane_samples(0.05, 0.01)[0])
    x, y, z, _ = synth.make_cloud(n)
    rec = {"points": n, "samples": T}
    with capi.Context(0) as ctx:
        ctx.upload_cloud(x, y, z)
        rows, wall, k = _median_call(ctx, lambda: ctx.mls_process(mp), [capi.K_MLS_VOXEL, capi.K_MLS_FIT])
        em = k[capi.K_MLS_VOXEL]
        rec.update(mls_rows=rows, fit_emit_ms=round(wall, 2), emit_ms=round(em, 3), fit_ms=round(k[capi.K_MLS_FIT], 3),
                   emit_GBps=round(rows * 32 / (em * 1e-3) / 1e9, 1) if em > 0 else None)
        keep, _ = ctx.sor(mp.sor_mean_k, mp.sor_std_mul)
    idx1 = np.nonzero(keep)[0]
    x1, y1, z1 = x[idx1], y[idx1], z[idx1]
    rec["survivors_first_filter"] = int(len(idx1))
    with capi.Context(0) as ctx1:
        ctx1.upload_cloud(x1, y1, z1)
        rec["rows_before"] = ctx1.mls_process(mp)
        a = _normals_by_point(ctx1.mls_fetch(ctx1.mls_process(none_p)), len(idx1))
    perm = np.random.default_rng(1).permutation(len(idx1))
    with capi.Context(0) as ctx2:
        ctx2.upload_cloud(x1[perm], y1[perm], z1[perm])
        b = _normals_by_point(ctx2.mls_fetch(ctx2.mls_process(none_p)), len(idx1), perm)
    both = np.any(a != 0, axis=1) & np.any(b != 0, axis=1)
    rec["fitted_survivors"] = int(both.sum())
    rec["sign_flips_reupload"] = int(((a * b).sum(axis=1)[both] < 0).sum())
    rec["bit_equal_normals_reupload"] = int(np.all(a[both] == b[both], axis=1).sum())
    if "--oracle" in args:
        from oracle import oracle_capi as oc

        oc.build()
        op = oc.default_mls_params()
        op.upsampling = 0
        op.threads = 16
        o = _normals_by_point(oc.mls(x1, y1, z1, op), len(idx1))
        both_o = np.any(a != 0, axis=1) & np.any(o != 0, axis=1)
        rec["sign_flips_vs_oracle"] = int(((a * o).sum(axis=1)[both_o] < 0).sum())
    _log(f"{n} points: {rows} rows, rows before the last filter {rec['rows_before']}")
    print(json.dumps(rec), flush=True)
    with capi.Context(0) as ctx:
        ctx.upload_cloud(x, y, z)
        for shape in shapes:
            os.environ["PCP_SOR_CLUSTERED"] = shape
            _log(f"chain, PCP_SOR_CLUSTERED={shape}")
            try:
                kept, wall, k = _median_call(ctx, lambda: ctx.cloud_smooth(mp), [capi.K_SOR])
            except capi.PcpError as e:  # the chain's refusal of rows its last filter cannot bound
                t0 = time.perf_counter()
                try:
                    ctx.cloud_smooth(mp)
                except capi.PcpError:
                    pass
                rec["chain_clustered" + shape] = {"refused": str(e)[:240], "refusal_ms": round((time.perf_counter() - t0) * 1e3, 1)}
                print(json.dumps(rec), flush=True)
                continue
            rec["chain_clustered" + shape] = {"chain_ms": round(wall, 1), "chain_sor_ms": round(k[capi.K_SOR], 1),
                                              "rows_after": kept}
            print(json.dumps(rec), flush=True)
        os.environ.pop("PCP_SOR_CLUSTERED", None)


if __name__ == "__main__":
    main()
