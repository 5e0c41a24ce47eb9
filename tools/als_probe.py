"""ALS probe: one fit on a synthetic rating matrix (default 200k users x 20k items, D = 20,
about 20 M ratings), timed by the HIP events of cf_als_fit.  Prints one JSON line: supersteps,
updates, update and scatter ms per superstep, and the achieved GB/s of the update kernels
against the nnz (8 D + 8) bytes-per-half-sweep model, also as a fraction of the
8 TB/s HBM peak.  A probe, not a gate: there is nothing to compare against yet.

    python tools/als_probe.py [--users N --items M --nnz E --D d --supersteps S --baseline 2000]

--baseline K also times the numpy checker (tests/als_ref.py) on the first K users for one user
half-sweep and reports numpy's time per edge over the device's (numpy_over_device_per_edge): a
numpy baseline on this host's cores (OMP_NUM_THREADS)."""
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


def synth(n_users, n_items, nnz, seed=0):
    """Power-law item popularity, uniform users, integer ratings 1..5; duplicates dropped."""
    rng = np.random.default_rng(seed)
    p = 1.0 / np.arange(1, n_items + 1) ** 0.6
    p /= p.sum()
    item = rng.choice(n_items, size=nnz, p=p).astype(np.int64)
    user = rng.integers(0, n_users, nnz).astype(np.int64)
    key = np.unique(user * n_items + item)
    user, item = (key // n_items).astype(np.uint32), (key % n_items).astype(np.uint32)
    obs = rng.integers(1, 6, len(key)).astype(np.float32)
    return user, item, obs


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--users", type=int, default=200_000)
    ap.add_argument("--items", type=int, default=20_000)
    ap.add_argument("--nnz", type=int, default=20_000_000)
    ap.add_argument("--D", type=int, default=20)
    ap.add_argument("--supersteps", type=int, default=6)
    ap.add_argument("--baseline", type=int, default=0)
    a = ap.parse_args()
    from collaborative_filtering_amd.api import Context

    user, item, obs = synth(a.users, a.items, a.nnz)
    nnz = len(user)
    rng = np.random.default_rng(1)
    U0, V0 = rng.uniform(-1, 1, (a.users, a.D)), rng.uniform(-1, 1, (a.items, a.D))
    with Context(0) as ctx:
        t0 = time.time()
        r = ctx.als_fit(user, item, obs, a.users, a.items, U0, V0, lam=0.05, regnormal="degree", tol=1e-3,
                        max_supersteps=a.supersteps)
        wall = time.time() - t0
        rmse = ctx.als_rmse(user, item, obs, r.U, r.V, 1.0, 5.0)
    steps = max(r.supersteps, 1)
    model_bytes = nnz * (8 * a.D + 8)
    upd_ms = r.update_ms / steps
    gbs = model_bytes / (upd_ms * 1e-3) / 1e9 if upd_ms > 0 else 0.0
    out = {"probe": "als", "users": a.users, "items": a.items, "nnz": nnz, "D": a.D, "supersteps": r.supersteps,
           "updates": r.updates, "n_not_pd": r.n_not_pd, "update_ms_per_superstep": round(upd_ms, 4),
           "scatter_ms_per_superstep": round(r.scatter_ms / steps, 4), "model_bytes_per_half_sweep": model_bytes,
           "update_GBps_vs_model": round(gbs, 1), "fraction_of_8TBps": round(gbs / 8000.0, 4),
           "train_rmse": round(rmse, 5), "fit_wall_s_with_host_csr_and_copies": round(wall, 2)}
    if a.baseline:
        import als_ref as ar

        k = min(a.baseline, a.users)
        sel = user < k
        ru, ri = ar.reg_arrays(user[sel], item[sel], k, a.items, 0.05, "degree")
        t0 = time.time()
        ref = ar.fit(user[sel], item[sel], obs[sel], k, a.items, U0[:k], V0, ru, ri, max_supersteps=1)
        cpu_s = time.time() - t0
        # the device's first superstep updates every user: its share of the update time by edges
        dev_s_per_edge = (r.update_ms * 1e-3 / steps) / nnz
        out.update(numpy_baseline_users=k, numpy_baseline_edges=int(sel.sum()), numpy_half_sweep_s=round(cpu_s, 3),
                   numpy_threads=int(os.environ.get("OMP_NUM_THREADS", os.cpu_count() or 1)), numpy_updates=ref.updates,
                   numpy_over_device_per_edge=round((cpu_s / max(int(sel.sum()), 1)) / dev_s_per_edge, 1))
    print(json.dumps(out))


if __name__ == "__main__":
    main()
