"""SGD probe: one fit on the synthetic rating matrix of tools/als_probe.py (default 200k users x
20k items, D = 20, about 20 M ratings), timed by the HIP events of cf_sgd_fit.  Prints one JSON
line: supersteps, updates, messages, ms per user superstep of the reduction kernels (both sides:
the user sums and the items' messages are reduced in the user superstep), the same per side, the
apply kernels, and the achieved GB/s of each side against the nnz (8 D + 8) bytes model
(DESIGN 3.13), also as a fraction of the 8 TB/s HBM peak.  A probe, not a gate.

    python tools/sgd_probe.py [--users N --items M --nnz E --D d --updates K --bias] > profiles/sgd/probe.json
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


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--users", type=int, default=200_000)
    ap.add_argument("--items", type=int, default=20_000)
    ap.add_argument("--nnz", type=int, default=20_000_000)
    ap.add_argument("--D", type=int, default=20)
    ap.add_argument("--updates", type=int, default=3)
    ap.add_argument("--bias", action="store_true")
    a = ap.parse_args()
    from collaborative_filtering_amd.api import Context

    user, item, obs = synth(a.users, a.items, a.nnz)
    nnz = len(user)
    rng = np.random.default_rng(1)
    U0, V0 = rng.uniform(-1, 1, (a.users, a.D)) * 0.5, rng.uniform(-1, 1, (a.items, a.D)) * 0.5
    # the step is small: an item of this graph has up to tens of thousands of raters
    hyper = dict(lam=0.05, gamma=2e-5, step_dec=0.9, tol=0.5, minval=1.0, maxval=5.0)
    with Context(0) as ctx:
        ctx.sgd_fit(user[:1000], item[:1000], obs[:1000], a.users, a.items, U0, V0, max_updates=1, **hyper)   # warm-up
        t0 = time.time()
        r = ctx.sgd_fit(user, item, obs, a.users, a.items, U0, V0, bias=a.bias, max_updates=a.updates, trace=False,
                        **hyper)
        wall = time.time() - t0
        rmse = ctx.sgd_rmse(user, item, obs, r.U, r.V, r.bias_user, r.bias_item, r.global_mean, 1.0, 5.0)
    steps = max((r.supersteps + 1) // 2, 1)
    model_bytes = nnz * (8 * a.D + 8)

    def rate(ms):
        gbs = model_bytes / (ms * 1e-3) / 1e9 if ms > 0 else 0.0
        return round(gbs, 1), round(gbs / 8000.0, 4)

    u_ms, i_ms = r.user_reduce_ms / steps, r.item_reduce_ms / steps
    out = {"probe": "sgd", "bias": bool(a.bias), "users": a.users, "items": a.items, "nnz": nnz, "D": a.D,
           "supersteps": r.supersteps, "user_supersteps": steps, "updates": r.updates, "messages": r.messages,
           "n_nan": r.n_nan, "reduce_ms_per_user_superstep": round(r.reduce_ms / steps, 4),
           "user_side_ms": round(u_ms, 4), "item_side_ms": round(i_ms, 4),
           "apply_ms_per_user_superstep": round(r.apply_ms / steps, 4), "model_bytes_per_side": model_bytes,
           "user_side_GBps_vs_model": rate(u_ms)[0], "user_side_fraction_of_8TBps": rate(u_ms)[1],
           "item_side_GBps_vs_model": rate(i_ms)[0], "item_side_fraction_of_8TBps": rate(i_ms)[1],
           "train_rmse": round(rmse, 5),
           "fit_wall_s_with_host_csr_and_copies": round(wall, 2)}
    print(json.dumps(out))


if __name__ == "__main__":
    main()
