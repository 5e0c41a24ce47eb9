"""Rank-evaluation probe: cf_mf_rank_eval at the shape of the top-N probe (default 200k users x 20k
items, D = 20, N = 10, the exclusions = the ALS probe's synthetic ratings, about 20 M) with
--held held-out items per user drawn from the user's unrated pairs, timed by the HIP events of
the call.  In the same run, on the same factors and exclusions, cf_mf_topn at the same N for its
select_ms.  Prints one JSON line and writes it to --out (profiles/rank/probe.json): score_ms and
rank_ms (median of --repeats calls after --warmup calls; every call's pair is kept), select_ms of
cf_mf_topn measured the same way, and the rank stage against its byte model.  A probe, not a gate.

Byte model, S = evaluated users x items keys:
  score stage    writes 8 S bytes of keys (as in the top-N probe)
  rank stage     the exclusion kernel's stores, then ceil(m / T) walks per row of m held-out items;
                 a row of 8 n_items bytes stays in L2 after its first walk, so 8 S bytes have to
                 come from HBM once; each key meets T comparisons of (key, item) pairs per walk

    python tools/rank_probe.py [--users N --items M --nnz E --D d --N n --held h --out FILE]"""
from __future__ import annotations

import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))

HBM_PEAK = 8.0e12      # bytes/s
SELECT_PASSES = 11


def draw_held(rng, n_users, n_items, user, item, per_user):
    """per_user distinct unrated items for every user: a surplus of uniform draws per user, minus
    the rated and the repeated ones, the first per_user of the rest in draw order."""
    width = 2 * per_user + 8
    cand = rng.integers(0, n_items, (n_users, width), dtype=np.int64)
    rows = np.arange(n_users, dtype=np.int64)[:, None]
    order = np.argsort(cand, axis=1, kind="stable")
    srt = np.take_along_axis(cand, order, axis=1)
    ok_sorted = np.ones((n_users, width), dtype=bool)
    ok_sorted[:, 1:] = srt[:, 1:] != srt[:, :-1]
    rated = np.unique(user.astype(np.int64) * n_items + item.astype(np.int64))
    ok_sorted &= ~np.isin(rows * n_items + srt, rated)
    ok = np.zeros_like(ok_sorted)
    np.put_along_axis(ok, order, ok_sorted, axis=1)
    ok &= np.cumsum(ok, axis=1) <= per_user
    if not (ok.sum(axis=1) == per_user).all():
        raise SystemExit("a user has fewer unrated draws than --held: lower --held or --nnz")
    hu = np.broadcast_to(rows, cand.shape)[ok]
    return hu.astype(np.uint32), cand[ok].astype(np.uint32)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--users", type=int, default=200_000)
    ap.add_argument("--items", type=int, default=20_000)
    ap.add_argument("--nnz", type=int, default=20_000_000)
    ap.add_argument("--D", type=int, default=20)
    ap.add_argument("--N", type=int, default=10)
    ap.add_argument("--held", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "rank", "probe.json"))
    a = ap.parse_args()
    from als_probe import synth
    from collaborative_filtering_amd import _native
    from collaborative_filtering_amd.api import Context

    user, item, _ = synth(a.users, a.items, a.nnz)
    rng = np.random.default_rng(1)
    U, V = rng.uniform(-1, 1, (a.users, a.D)), rng.uniform(-1, 1, (a.items, a.D))   # the top-N probe's factors
    held = draw_held(np.random.default_rng(2), a.users, a.items, user, item, a.held)
    T = _native.load().cf_debug_rank_targets()
    rank_runs, topn_runs = [], []
    with Context(0) as ctx:
        for k in range(a.warmup + a.repeats):   # the two calls alternate
            t0 = time.time()
            r = ctx.mf_rank_eval(U, V, a.N, held, exclude=(user, item))
            wall = time.time() - t0
            t = ctx.mf_topn(U, V, a.N, exclude=(user, item))
            if k >= a.warmup:
                rank_runs.append((float(r.stats.score_ms), float(r.stats.rank_ms), wall))
                topn_runs.append((float(t.stats.score_ms), float(t.stats.select_ms)))
    # every held-out item on a user's top-N list is a hit, and the other way round
    listed = np.zeros(a.users, dtype=np.int64)
    on_list = (t.items[held[0]] == held[1][:, None]).any(axis=1)
    np.add.at(listed, held[0], on_list)
    score_ms = float(np.median([x[0] for x in rank_runs]))
    rank_ms = float(np.median([x[1] for x in rank_runs]))
    select_ms = float(np.median([x[1] for x in topn_runs]))
    evaluated = int(r.summary["users_evaluated"])
    S = evaluated * a.items
    walks = -(-a.held // T)
    out = {"probe": "rank", "users": a.users, "items": a.items, "D": a.D, "N": a.N, "exclusions": len(user),
           "held_per_user": a.held, "held_edges": len(held[0]), "targets_per_walk": T, "walks_per_row": walks,
           "blocks": int(r.stats.blocks), "users_evaluated": evaluated, "edges_skipped": int(r.summary["edges_skipped"]),
           "hits_equal_topn_lists": bool(np.array_equal(listed, r.users["hits"].astype(np.int64))),
           "warmup": a.warmup, "repeats": a.repeats,
           "score_ms": round(score_ms, 3), "rank_ms": round(rank_ms, 3),
           "score_ms_runs": [round(x[0], 3) for x in rank_runs], "rank_ms_runs": [round(x[1], 3) for x in rank_runs],
           "topn_score_ms": round(float(np.median([x[0] for x in topn_runs])), 3), "topn_select_ms": round(select_ms, 3),
           "topn_select_ms_runs": [round(x[1], 3) for x in topn_runs],
           "rank_ms_over_topn_select_ms": round(rank_ms / select_ms, 4),
           "panel_bytes_written": 8 * S, "panel_bytes_asked_by_rank": walks * 8 * S,
           "panel_bytes_asked_by_select": SELECT_PASSES * 8 * S,
           "rank_fraction_of_8TBps_one_pass": round(8 * S / (rank_ms * 1e-3) / HBM_PEAK, 4),
           "pair_comparisons_per_s": round(walks * T * S / (rank_ms * 1e-3), 1),
           "keys_per_s_whole_call": round(S / ((score_ms + rank_ms) * 1e-3), 1),
           "summary": {k: round(float(r.summary[k]), 6) for k in ("precision", "recall", "ndcg", "map", "mrr", "auc", "mpr")},
           "call_wall_s_with_host_csr_and_copies": round(float(np.median([x[2] for x in rank_runs])), 2)}
    line = json.dumps(out)
    print(line)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
