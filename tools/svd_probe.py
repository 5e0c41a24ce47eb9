"""SVD probe: cf_svd_fit on the synthetic rating matrix of tools/als_probe.py (default 200k users x
20k items, about 20 M ratings: the graph of profiles/als/probe.json), cut after a fixed number of
restarts and timed by the HIP events of cf_svd_fit per kernel kind.  Prints one JSON line: passes,
products, converged triplets, the ms of each kernel kind and each kind against its byte model
(DESIGN 3.15), also as a fraction of the 8 TB/s HBM peak:
    product   nnz (4 + 4 + 8) + 8 n_out                       per product
    ortho     repeats (2 (j + 1) + [j > 0]) 8 ld + 16 ld      per step with j earlier vectors
              (j = 0: 8 ld for the norm, 16 ld to normalise)
    rotate    ceil(c / 8) m 8 ld + c 8 ld + c 16 ld           per side and pass (c new columns of m)
Lanczos vectors of these sizes stay in the 256 MiB Infinity Cache between kernels, so the ortho
and rotate figures can exceed what HBM alone would give.  A probe, not a gate.

    python tools/svd_probe.py [--users N --items M --nnz E --nsv s --nv v --passes p] > profiles/svd/probe.json
"""
from __future__ import annotations

import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

from als_probe import synth  # noqa: E402


def padded(n):
    return (n + 15) // 16 * 16


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--users", type=int, default=200_000)
    ap.add_argument("--items", type=int, default=20_000)
    ap.add_argument("--nnz", type=int, default=20_000_000)
    ap.add_argument("--nsv", type=int, default=10)
    ap.add_argument("--nv", type=int, default=40)
    ap.add_argument("--passes", type=int, default=3)
    ap.add_argument("--ortho_repeats", type=int, default=3)
    a = ap.parse_args()
    from collaborative_filtering_amd.api import Context

    user, item, obs = synth(a.users, a.items, a.nnz)
    nnz = len(user)
    with Context(0) as ctx:
        ctx.svd_fit(user[:1000], item[:1000], obs[:1000], a.users, a.items, 2, 4, max_iter=2)   # warm-up
        t0 = time.time()
        r = ctx.svd_fit(user, item, obs, a.users, a.items, a.nsv, a.nv, max_iter=a.passes + 1, tol=1e-8,
                        ortho_repeats=a.ortho_repeats)
        wall = time.time() - t0
    ld = (padded(a.users), padded(a.items))   # P side, Q side
    n_side = (a.users, a.items)
    model = {"matvec": 0, "ortho": 0, "rotate": 0}
    steps = 0
    nconv = 0
    R = a.ortho_repeats

    def step(side, j):
        nonlocal steps
        model["matvec"] += nnz * 16 + 8 * n_side[side]
        model["ortho"] += (R * (2 * (j + 1) + 1) * 8 * ld[side] if j else 8 * ld[side]) + 16 * ld[side]
        steps += 1

    for p in range(r.passes):
        k = nconv
        step(1, k)
        for i in range(k + 1, a.nv):
            step(0, i)
            step(1, i)
        step(0, a.nv)
        kk = int(r.kk_pass[p])
        m = a.nv - nconv
        last = p + 1 == r.passes and nconv + kk >= a.nsv
        for side, c in ((0, kk + (0 if last else 1)), (1, kk)):
            if c:
                model["rotate"] += (-(-c // 8) * m + 3 * c) * 8 * ld[side]
        nconv += kk
    n_out = min(a.nsv, r.nconv)
    model["matvec"] += n_out * (2 * nnz * 16 + 8 * (a.users + a.items))
    ms = {"matvec": r.matvec_ms, "ortho": r.ortho_ms, "rotate": r.rotate_ms}
    out = {"probe": "svd", "rows": a.users, "cols": a.items, "nnz": nnz, "nsv": a.nsv, "nv": a.nv,
           "ortho_repeats": R, "passes": r.passes, "products": r.products, "lanczos_steps": steps, "nconv": r.nconv,
           "kk_per_pass": [int(x) for x in r.kk_pass], "matvec_ms_per_product": round(r.matvec_ms / max(r.products, 1), 4),
           "ortho_ms_per_step": round(r.ortho_ms / max(steps, 1), 4),
           "rotate_ms_per_pass": round(r.rotate_ms / max(r.passes, 1), 4)}
    for k in ("matvec", "ortho", "rotate"):
        gbs = model[k] / (ms[k] * 1e-3) / 1e9 if ms[k] > 0 else 0.0
        out[k + "_ms"] = round(ms[k], 4)
        out[k + "_model_bytes"] = int(model[k])
        out[k + "_ms_at_8TBps"] = round(model[k] / 8e12 * 1e3, 4)
        out[k + "_GBps_vs_model"] = round(gbs, 1)
        out[k + "_fraction_of_8TBps"] = round(gbs / 8000.0, 4)
    out["sigma_head"] = [float("%.10g" % s) for s in r.sigma[:min(a.nsv, 5)]]
    out["fit_wall_s_with_host_csr_and_copies"] = round(wall, 2)
    print(json.dumps(out))


if __name__ == "__main__":
    main()
