"""BPR probe: cf_bpr_fit on the synthetic rating matrix of tools/als_probe.py (default 200k users x
20k items, D = 20, about 20 M edges, every edge a positive), timed by the HIP events of the fit
(cf_bpr_timing), with SGD's user reduction timed on the same graph and D in the same process as the
yardstick (same skeleton, same machine, same clocks).  Writes one JSON object to --out (default
profiles/bpr/probe.json) and prints it:

  per sweep the ms of the sample and gradient kernel, of the negative lists (sort, offsets, class
  lists), of the user, item-positive and item-negative reductions and of the commit; each stage's
  share of the sweep; the user reduction over SGD's (the BPR edge gathers two item rows, one at a
  random address: about 2 is the expectation); the share of the sort plus the negative-side
  reduction, which no other model here pays.

    python tools/bpr_probe.py [--users N --items M --nnz E --D d --sweeps S --out FILE]

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

STAGES = ("sample", "negative_lists", "user_reduce", "item_positive_reduce", "item_negative_reduce", "commit")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--users", type=int, default=200_000)
    ap.add_argument("--items", type=int, default=20_000)
    ap.add_argument("--nnz", type=int, default=20_000_000)
    ap.add_argument("--D", type=int, default=20)
    ap.add_argument("--sweeps", type=int, default=3)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "bpr", "probe.json"))
    a = ap.parse_args()
    from collaborative_filtering_amd.api import Context

    user, item, obs = synth(a.users, a.items, a.nnz)
    nnz = len(user)
    rng = np.random.default_rng(1)
    U0, V0 = rng.uniform(-0.1, 0.1, (a.users, a.D)), rng.uniform(-0.1, 0.1, (a.items, a.D))
    out = {"probe": "bpr", "users": a.users, "items": a.items, "nnz": nnz, "D": a.D, "sweeps": a.sweeps}
    kw = dict(bias0=np.zeros(a.items), lr=0.5, seed=1)
    with Context(0) as ctx:
        ctx.bpr_fit(user, item, a.users, a.items, U0, V0, n_sweeps=1, **kw)   # warm-up
        r = ctx.bpr_fit(user, item, a.users, a.items, U0, V0, n_sweeps=a.sweeps, **kw)
        # the yardstick: one user superstep of plain SGD with every user active (tools/nmf_probe.py); best of three
        sgd_u = None
        for _ in range(3):
            s = ctx.sgd_fit(user, item, obs, a.users, a.items, U0, V0, tol=0.0, max_supersteps=1, trace=False)
            sgd_u = s.user_reduce_ms if sgd_u is None else min(sgd_u, s.user_reduce_ms)
    per = r.stage_ms.astype(np.float64) / r.sweeps
    total = float(per.sum())
    for k, name in enumerate(STAGES):
        out[f"{name}_ms_per_sweep"] = round(float(per[k]), 4)
        out[f"{name}_share"] = round(float(per[k]) / total, 4)
    out["sweep_ms"] = round(total, 4)
    out["sweep_Gedges_per_s"] = round(nnz / (total * 1e-3) / 1e9, 3)
    out["sgd_user_reduce_ms"] = round(sgd_u, 4)
    out["user_reduce_over_sgd_user_reduce"] = round(float(per[2]) / sgd_u, 3)
    out["negative_side_share"] = round(float(per[1] + per[4]) / total, 4)
    out["triples"], out["n_skipped"], out["n_nan"] = r.triples, r.n_skipped, r.n_nan
    out["mean_softplus_first"] = float(r.loss_trace[0, 0] / r.loss_trace[0, 1])
    out["mean_softplus_last"] = float(r.loss_trace[-1, 0] / r.loss_trace[-1, 1])
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as fh:
        json.dump(out, fh, indent=1)
        fh.write("\n")
    print(json.dumps(out))


if __name__ == "__main__":
    main()
