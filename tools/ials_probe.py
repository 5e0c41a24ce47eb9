"""iALS probe: implicit-feedback ALS on the synthetic rating matrix of tools/als_probe.py (default
200k users x 20k items, D = 20, about 20 M edges), timed by the HIP events of cf_ials_fit, with
explicit ALS timed on the same graph in the same process as the yardstick for the update kernels
(same machine, same clocks).  Writes one JSON object to --out (default profiles/ials/probe.json)
and prints it:

  gram / update / loss ms per half-sweep; the achieved GB/s of update + Gram against the
  nnz (8 D + 12) + n 8 D bytes-per-half-sweep model, also as a fraction of the
  8 TB/s HBM peak; explicit ALS's update ms per superstep with every vertex active (tol = 0) and
  the ratio iALS / ALS; and the global Gram alone at D = 20 and D = 64 over --gram-users rows
  (default 2 M: at the fit's own 200k rows a Gram is a few launches of a few microseconds each)
  in GB/s of the n 8 D bytes it reads, with the fp64 fma rate that implies (n D^2 fma per Gram).

    python tools/ials_probe.py [--users N --items M --nnz E --D d --sweeps S --out FILE]

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


def gram_alone(ctx, n_users, n_items, D, rng):
    """The three Grams of one sweep (items, users, items) on a graph with few edges, so that the
    events time little else: (ms per sweep, bytes read, fma done)."""
    user = rng.integers(0, n_users, 1000).astype(np.uint32)
    item = rng.integers(0, n_items, 1000).astype(np.uint32)
    U0, V0 = rng.uniform(-1, 1, (n_users, D)), rng.uniform(-1, 1, (n_items, D))
    best = None
    for _ in range(3):
        r = ctx.ials_fit(user, item, np.full(1000, 2.0, np.float32), n_users, n_items, U0, V0, n_sweeps=1, trace=False)
        best = r.gram_ms if best is None else min(best, r.gram_ms)
    rows = n_users + 2 * n_items
    return best, rows * 8 * D, rows * D * D


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--users", type=int, default=200_000)
    ap.add_argument("--items", type=int, default=20_000)
    ap.add_argument("--nnz", type=int, default=20_000_000)
    ap.add_argument("--D", type=int, default=20)
    ap.add_argument("--sweeps", type=int, default=3)
    ap.add_argument("--gram-users", type=int, default=2_000_000, help="rows of the Gram-alone measurement")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "ials", "probe.json"))
    a = ap.parse_args()
    from collaborative_filtering_amd.api import Context

    user, item, obs = synth(a.users, a.items, a.nnz)
    nnz = len(user)
    conf = (1.0 + 0.5 * obs).astype(np.float32)
    pref = (obs > 2).astype(np.float32)
    rng = np.random.default_rng(1)
    U0, V0 = rng.uniform(-1, 1, (a.users, a.D)), rng.uniform(-1, 1, (a.items, a.D))
    half = 2 * a.sweeps
    with Context(0) as ctx:
        ctx.ials_fit(user, item, conf, a.users, a.items, U0, V0, pref=pref, lam=0.1, n_sweeps=1)   # warm-up
        r = ctx.ials_fit(user, item, conf, a.users, a.items, U0, V0, pref=pref, lam=0.1, n_sweeps=a.sweeps)
        # the yardstick: explicit ALS with every vertex active in every superstep (tol = 0 signals all)
        ctx.als_fit(user, item, obs, a.users, a.items, U0, V0, lam=0.05, regnormal="degree", tol=0.0, max_supersteps=2)
        als = ctx.als_fit(user, item, obs, a.users, a.items, U0, V0, lam=0.05, regnormal="degree", tol=0.0,
                          max_supersteps=half)
        grams = {D: gram_alone(ctx, a.gram_users, a.items, D, rng) for D in (20, 64)}
    upd, gram, loss = r.update_ms / half, r.gram_ms / (half + 1), r.loss_ms / half
    als_upd = als.update_ms / max(als.supersteps, 1)
    model = nnz * (8 * a.D + 12) + (a.users + a.items) // 2 * 8 * a.D   # the mean of the two sides' n 8 D
    gbs = model / ((upd + gram) * 1e-3) / 1e9
    out = {"probe": "ials", "users": a.users, "items": a.items, "nnz": nnz, "D": a.D, "sweeps": r.sweeps,
           "n_not_pd": r.n_not_pd, "gram_ms_per_half_sweep": round(gram, 4), "update_ms_per_half_sweep": round(upd, 4),
           "loss_ms_per_half_sweep": round(loss, 4), "model_bytes_per_half_sweep": model,
           "update_plus_gram_GBps_vs_model": round(gbs, 1), "fraction_of_8TBps": round(gbs / 8000.0, 4),
           "als_supersteps": als.supersteps, "als_updates": als.updates,
           "als_update_ms_per_superstep": round(als_upd, 4), "ials_over_als_update": round(upd / als_upd, 3),
           "loss_first": float(r.loss_trace[0]), "loss_last": float(r.loss_trace[-1])}
    out["gram_alone_rows_per_sweep"] = a.gram_users + 2 * a.items
    for D, (ms, nbytes, fma) in grams.items():
        out[f"gram_D{D}_ms_per_sweep"] = round(ms, 4)
        out[f"gram_D{D}_GBps"] = round(nbytes / (ms * 1e-3) / 1e9, 1)
        out[f"gram_D{D}_Gfma_per_s"] = round(fma / (ms * 1e-3) / 1e9, 1)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as fh:
        json.dump(out, fh, indent=1)
        fh.write("\n")
    print(json.dumps(out))


if __name__ == "__main__":
    main()
