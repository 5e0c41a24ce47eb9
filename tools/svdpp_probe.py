"""SVD++ probe: one fit on the synthetic rating matrix of tools/als_probe.py (default 200k users x
20k items, D = 20, about 20 M ratings: the graph of profiles/sgd/probe.json), timed by the HIP
events of cf_svdpp_fit.  Every user starts in phase 1, so the user supersteps alternate between
the phases: the phase-1 reduction runs in supersteps 0, 4, .., the phase-2 user reduction and the
item message reduction in supersteps 2, 6, ...  Prints one JSON line: supersteps, updates,
messages, the ms of each kernel kind per superstep in which it runs, the apply kernels, and each
kind against its byte model, also as a fraction of the 8 TB/s HBM peak:
    phase 1      nnz_all (8 D + 4)     the Y half of the item row and the item index
    phase 2 user nnz (16 D + 16)       the whole item row, index, rating, item bias
    item         nnz (16 D + 21)       the whole user row, index, rating, user bias, usrNorm, the phase flag
A probe, not a gate.

    python tools/svdpp_probe.py [--users N --items M --nnz E --D d --updates K --implicit F] > profiles/svdpp/probe.json
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
    ap.add_argument("--updates", type=int, default=4, help="max_updates: phase-1 and phase-2 updates alike")
    ap.add_argument("--implicit", type=float, default=0.0, help="fraction of the ratings moved to the implicit list")
    a = ap.parse_args()
    from collaborative_filtering_amd.api import Context

    user, item, obs = synth(a.users, a.items, a.nnz)
    imp = None
    if a.implicit > 0:
        move = np.random.default_rng(2).random(len(user)) < a.implicit
        imp = (user[move], item[move])
        user, item, obs = user[~move], item[~move], obs[~move]
    nnz = len(user)
    nnz_all = nnz + (len(imp[0]) if imp else 0)
    rng = np.random.default_rng(1)
    U0, V0 = rng.uniform(-1, 1, (a.users, a.D)) * 0.5, rng.uniform(-1, 1, (a.items, a.D)) * 0.5
    W0, Y0 = rng.uniform(-1, 1, (a.users, a.D)) * 0.1, rng.uniform(-1, 1, (a.items, a.D)) * 0.1
    # the steps are small: an item of this graph has up to tens of thousands of raters
    names = ("user_bias", "item_bias", "user_factor", "item_factor", "item_factor2")
    hyper = {k + "_step": 2e-5 for k in names}
    hyper.update({k + "_reg": 0.05 for k in names})
    hyper.update(step_dec=0.9, minval=1.0, maxval=5.0)
    with Context(0) as ctx:
        ctx.svdpp_fit(user[:1000], item[:1000], obs[:1000], a.users, a.items, U0, V0, W0, Y0, max_updates=2, **hyper)   # warm-up
        t0 = time.time()
        r = ctx.svdpp_fit(user, item, obs, a.users, a.items, U0, V0, W0, Y0, implicit=imp, max_updates=a.updates,
                          trace=False, **hyper)
        wall = time.time() - t0
        rmse = ctx.svdpp_rmse(user, item, obs, r.U, r.V, r.bias_user, r.bias_item, r.global_mean, 1.0, 5.0)
    user_steps = max((r.supersteps + 1) // 2, 1)
    n1, n2 = max((user_steps + 1) // 2, 1), max(user_steps // 2, 1)
    model = {"phase1": nnz_all * (8 * a.D + 4), "user": nnz * (16 * a.D + 16), "item": nnz * (16 * a.D + 21)}
    ms = {"phase1": r.phase1_reduce_ms / n1, "user": r.user_reduce_ms / n2, "item": r.item_reduce_ms / n2}
    out = {"probe": "svdpp", "users": a.users, "items": a.items, "nnz": nnz, "nnz_all_roles": nnz_all, "D": a.D,
           "supersteps": r.supersteps, "user_supersteps": user_steps, "phase1_supersteps": n1, "phase2_supersteps": n2,
           "updates": r.updates, "messages": r.messages, "n_nan": r.n_nan,
           "apply_ms_per_user_superstep": round(r.apply_ms / user_steps, 4)}
    for k in ("phase1", "user", "item"):
        gbs = model[k] / (ms[k] * 1e-3) / 1e9 if ms[k] > 0 else 0.0
        out[k + "_reduce_ms"] = round(ms[k], 4)
        out[k + "_model_bytes"] = model[k]
        out[k + "_ms_at_8TBps"] = round(model[k] / 8e12 * 1e3, 4)
        out[k + "_GBps_vs_model"] = round(gbs, 1)
        out[k + "_fraction_of_8TBps"] = round(gbs / 8000.0, 4)
    out["train_rmse_without_Y"] = round(rmse, 5)
    out["fit_wall_s_with_host_csr_and_copies"] = round(wall, 2)
    print(json.dumps(out))


if __name__ == "__main__":
    main()
