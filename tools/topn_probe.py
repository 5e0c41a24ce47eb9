"""Top-N probe: cf_mf_topn at the shape of the ALS probe (default 200k users x 20k items, D = 20,
N = 10, the exclusions = the ALS probe's synthetic ratings, about 20 M), timed by the HIP events
of the call.  Prints one JSON line and writes it to --out (profiles/topn/probe.json): score_ms and select_ms
(median of --repeats calls after --warmup calls; every call's pair is kept), scores per second,
the panel bytes moved by the byte model below, and each stage as a fraction of the 8 TB/s HBM
peak and of the 78.6 TF/s fp64 MFMA peak.  A probe, not a gate: there is no parent to compare.

Byte and flop model, S = users x items scores, Dp = D rounded up to 4:
  score stage    writes 8 S bytes of keys, reads the factor rows (L2-resident), 2 Dp S flops
  select stage   asks for 11 x 8 S bytes: one counting pass, 8 radix passes and 2 compaction
                 passes over a row of 8 n_items bytes that fits in L2 after its first pass, so only
                 8 S of them have to come from HBM; both figures are reported

    python tools/topn_probe.py [--users N --items M --nnz E --D d --N n --baseline 512 --out FILE]

--baseline K also times the numpy checker (tests/topn_ref.py: matmul, mask, lexsort) on the
first K users and reports numpy's time per score over the device's, with numpy's thread count."""
from __future__ import annotations

import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, os.path.join(ROOT, "tools"))

HBM_PEAK = 8.0e12      # bytes/s
F64_MFMA_PEAK = 78.6e12   # flop/s
SELECT_PASSES = 11


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--users", type=int, default=200_000)
    ap.add_argument("--items", type=int, default=20_000)
    ap.add_argument("--nnz", type=int, default=20_000_000)
    ap.add_argument("--D", type=int, default=20)
    ap.add_argument("--N", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--baseline", type=int, default=0)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "topn", "probe.json"))
    a = ap.parse_args()
    from als_probe import synth
    from collaborative_filtering_amd.api import Context

    user, item, _ = synth(a.users, a.items, a.nnz)
    rng = np.random.default_rng(1)
    U, V = rng.uniform(-1, 1, (a.users, a.D)), rng.uniform(-1, 1, (a.items, a.D))
    runs = []
    with Context(0) as ctx:
        for k in range(a.warmup + a.repeats):
            t0 = time.time()
            r = ctx.mf_topn(U, V, a.N, exclude=(user, item))
            wall = time.time() - t0
            if k >= a.warmup:
                runs.append((float(r.stats.score_ms), float(r.stats.select_ms), wall))
    score_ms = float(np.median([x[0] for x in runs]))
    select_ms = float(np.median([x[1] for x in runs]))
    S = a.users * a.items
    Dp = (a.D + 3) // 4 * 4
    panel_write = 8 * S
    select_asked = SELECT_PASSES * 8 * S
    flops = 2 * Dp * S
    listed = int(r.count.sum())
    out = {"probe": "topn", "users": a.users, "items": a.items, "D": a.D, "N": a.N, "exclusions": len(user),
           "blocks": int(r.stats.blocks), "n_nan": int(r.stats.n_nan), "listed": listed,
           "warmup": a.warmup, "repeats": a.repeats,
           "score_ms": round(score_ms, 3), "select_ms": round(select_ms, 3),
           "score_ms_runs": [round(x[0], 3) for x in runs], "select_ms_runs": [round(x[1], 3) for x in runs],
           "scores_per_s": round(S / ((score_ms + select_ms) * 1e-3), 1),
           "panel_bytes_written": panel_write, "panel_bytes_asked_by_select": select_asked,
           "panel_bytes_moved_model": panel_write + select_asked,
           "score_fraction_of_8TBps": round(panel_write / (score_ms * 1e-3) / HBM_PEAK, 4),
           "score_fraction_of_fp64_mfma_peak": round(flops / (score_ms * 1e-3) / F64_MFMA_PEAK, 4),
           "select_fraction_of_8TBps_asked_bytes": round(select_asked / (select_ms * 1e-3) / HBM_PEAK, 4),
           "select_fraction_of_8TBps_one_pass": round(panel_write / (select_ms * 1e-3) / HBM_PEAK, 4),
           "call_wall_s_with_host_csr_and_copies": round(float(np.median([x[2] for x in runs])), 2)}
    if a.baseline:
        import topn_ref as tr

        k = min(a.baseline, a.users)
        sel = user < k
        t0 = time.time()
        ref = tr.topn(U[:k], V, a.N, exclude=(user[sel], item[sel]))
        cpu_s = time.time() - t0
        same = bool(np.array_equal(ref[0], r.items[:k]))
        dev_s_per_score = (score_ms + select_ms) * 1e-3 / S
        out.update(numpy_baseline_users=k, numpy_s=round(cpu_s, 3),
                   numpy_threads=int(os.environ.get("OMP_NUM_THREADS", os.cpu_count() or 1)),
                   numpy_lists_equal_device=same,
                   numpy_over_device_per_score=round((cpu_s / (k * a.items)) / dev_s_per_score, 1))
    line = json.dumps(out)
    print(line)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
