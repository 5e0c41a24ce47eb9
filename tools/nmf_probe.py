"""NMF probe: KL-divergence NMF in both modes on the synthetic rating matrix of tools/als_probe.py
(default 200k users x 20k items, D = 20, about 20 M edges), timed by the HIP events of cf_nmf_fit,
with SGD's vertex reduction timed on the same graph and D in the same process as the yardstick
(same skeleton, same gathers, same machine, same clocks).  Writes one JSON object to --out
(default profiles/nmf/probe.json) and prints it:

  column-sum / update / loss ms per half-sweep for each mode; edges per second of a half-sweep's
  update; the achieved GB/s of the update against the nnz (8 D + 8) + n 8 D bytes-per-half-sweep
  model, also as a fraction of the 8 TB/s HBM peak; the ms and edges per second of SGD's user and
  item reductions (one superstep, every user active, tol = 0), and the ratios NMF / SGD per edge,
  both taken as the mean of the two sides.

    python tools/nmf_probe.py [--users N --items M --nnz E --D d --sweeps S --out FILE]

A probe, not a gate."""
from __future__ import annotations

import argparse
import json
import os
import sys

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
    ap.add_argument("--sweeps", type=int, default=3)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "nmf", "probe.json"))
    a = ap.parse_args()
    from collaborative_filtering_amd.api import Context

    user, item, obs = synth(a.users, a.items, a.nnz)
    nnz = len(user)
    rng = np.random.default_rng(1)
    U0, V0 = rng.uniform(0.1, 1.0, (a.users, a.D)), rng.uniform(0.1, 1.0, (a.items, a.D))
    half = 2 * a.sweeps
    out = {"probe": "nmf", "users": a.users, "items": a.items, "nnz": nnz, "D": a.D, "sweeps": a.sweeps}
    model = nnz * (8 * a.D + 8) + (a.users + a.items) // 2 * 8 * a.D   # the mean of the two sides' n 8 D
    out["model_bytes_per_half_sweep"] = model
    with Context(0) as ctx:
        for mode in ("grid", "observed"):
            ctx.nmf_fit(user, item, obs, a.users, a.items, U0, V0, mode=mode, n_sweeps=1)   # warm-up
            r = ctx.nmf_fit(user, item, obs, a.users, a.items, U0, V0, mode=mode, n_sweeps=a.sweeps)
            upd = r.update_ms / half
            gbs = model / (upd * 1e-3) / 1e9
            out[mode] = {"sum_ms_per_half_sweep": round(r.sum_ms / half, 4), "update_ms_per_half_sweep": round(upd, 4),
                         "loss_ms_per_half_sweep": round(r.loss_ms / half, 4),
                         "update_Gedges_per_s": round(nnz / (upd * 1e-3) / 1e9, 3),
                         "update_GBps_vs_model": round(gbs, 1), "fraction_of_8TBps": round(gbs / 8000.0, 4),
                         "n_floored": r.n_floored, "loss_first": float(r.loss_trace[0]), "loss_last": float(r.loss_trace[-1])}
        # the yardstick: one user superstep of plain SGD with every user active and tol = 0, so that
        # every item is signalled and every edge carries a message: both of its reductions then walk
        # every edge, through the same skeleton over the same CSRs; best of three
        Us, Vs = rng.uniform(-0.1, 0.1, (a.users, a.D)), rng.uniform(-0.1, 0.1, (a.items, a.D))
        sgd_u = sgd_i = None
        for _ in range(3):
            s = ctx.sgd_fit(user, item, obs, a.users, a.items, Us, Vs, tol=0.0, max_supersteps=1, trace=False)
            sgd_u = s.user_reduce_ms if sgd_u is None else min(sgd_u, s.user_reduce_ms)
            sgd_i = s.item_reduce_ms if sgd_i is None else min(sgd_i, s.item_reduce_ms)
    sgd_mean = 0.5 * (sgd_u + sgd_i)   # an NMF half-sweep figure is the mean of the two sides as well
    out["sgd_user_reduce_ms"] = round(sgd_u, 4)
    out["sgd_item_reduce_ms"] = round(sgd_i, 4)
    out["sgd_user_reduce_Gedges_per_s"] = round(nnz / (sgd_u * 1e-3) / 1e9, 3)
    out["sgd_mean_reduce_Gedges_per_s"] = round(nnz / (sgd_mean * 1e-3) / 1e9, 3)
    for mode in ("grid", "observed"):
        out[f"{mode}_update_over_sgd_mean_reduce"] = round(out[mode]["update_ms_per_half_sweep"] / sgd_mean, 3)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as fh:
        json.dump(out, fh, indent=1)
        fh.write("\n")
    print(json.dumps(out))


if __name__ == "__main__":
    main()
