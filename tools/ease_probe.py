"""EASE probe: the stage times of one cf_ease_fit and of one cf_ease_topn scoring pass at one synthetic
shape (default 100k users x 10k items, the ALS probe's synthetic ratings, about 50 per user, N = 10).
The GPU step runs in a child process of its own under a time limit and is not tried again.  Prints
one JSON line and writes it to --out (profiles/ease/probe.json).  A probe, not a gate: no target is
set.

Work models, printed beside the times they are tested against:
  gram       sum_u deg(u)^2 read-modify-writes of 8 bytes
  invert     n / b block steps; a step's trailing update reads and writes every tile once (16 n^2
             bytes) for 2 b n^2 flops: invert_bytes_model = 16 n^3 / b, invert_flops = 2 n^3
  score      every profile entry of a scored user reads one row of B: 8 n_items bytes.  If
             score_b_bytes_per_s is above what HBM delivers, the slab B[:, tile] of the workgroups
             that run together came from the Infinity Cache.

    python tools/ease_probe.py [--users N --items M --nnz E --lam L --N n --out FILE]"""
from __future__ import annotations

import argparse
import json
import os
import subprocess
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))


def step(a):
    """The GPU step in this process; prints its JSON."""
    from als_probe import synth
    from collaborative_filtering_amd import _native
    from collaborative_filtering_amd.api import Context

    user, item, obs = synth(a.users, a.items, a.nnz, 0)   # sorted by user, then item; pairs distinct
    off = np.zeros(a.users + 1, dtype=np.uint64)
    off[1:] = np.cumsum(np.bincount(user, minlength=a.users))
    deg = np.diff(off.astype(np.int64))
    lib = _native.load()
    b, n = lib.cf_debug_ease_block(), a.items
    out = {"edges": int(len(item)), "profile_len_mean": round(float(deg.mean()), 2), "profile_len_max": int(deg.max()),
           "block": b, "score_cols": lib.cf_debug_ease_cols(), "score_unroll": lib.cf_debug_ease_unroll(),
           "gram_rmw": int((deg * deg).sum()), "invert_flops": 2 * n ** 3, "invert_bytes_model": 16 * n ** 3 // b,
           "b_bytes": 8 * n * n}
    with Context(0) as ctx:
        fits = []
        for _ in range(a.warmup + a.repeats):
            fits.append([float(x) for x in ctx.ease_fit(off, item, obs, n, a.lam)])
        fits = np.array(fits[a.warmup:])
        gram, inv, norm = (round(float(np.median(fits[:, k])), 3) for k in range(3))
        out["fit"] = {"gram_ms": gram, "invert_ms": inv, "normalise_ms": norm,
                      "runs": [[round(x, 3) for x in r] for r in fits.tolist()],
                      "gram_rmw_per_s": round(out["gram_rmw"] / (gram * 1e-3), 1),
                      "invert_flops_per_s": round(out["invert_flops"] / (inv * 1e-3), 1),
                      "invert_model_bytes_per_s": round(out["invert_bytes_model"] / (inv * 1e-3), 1)}
        score, select = [], []
        for k in range(a.warmup + a.repeats):
            r = ctx.ease_topn(off, item, obs, a.N)
            if k >= a.warmup:
                score.append(float(r.stats.score_ms))
                select.append(float(r.stats.select_ms))
        b_bytes = 8 * n * int(len(item))
        ms = float(np.median(score))
        out["topn"] = {"score_ms": round(ms, 3), "select_ms": round(float(np.median(select)), 3),
                       "score_ms_runs": [round(x, 3) for x in score], "blocks": int(r.stats.blocks),
                       "n_nan": int(r.stats.n_nan), "score_b_bytes": b_bytes,
                       "score_b_bytes_per_s": round(b_bytes / (ms * 1e-3), 1),
                       "slab_bytes": 8 * n * out["score_cols"]}
    print("STEP " + json.dumps(out))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--users", type=int, default=100_000)
    ap.add_argument("--items", type=int, default=10_000)
    ap.add_argument("--nnz", type=int, default=5_000_000)
    ap.add_argument("--lam", type=float, default=100.0)
    ap.add_argument("--N", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--repeats", type=int, default=2)
    ap.add_argument("--step-timeout", type=int, default=300)
    ap.add_argument("--step", action="store_true")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "ease", "probe.json"))
    a = ap.parse_args()
    if a.step:
        return step(a)
    out = {"probe": "ease", "users": a.users, "items": a.items, "nnz_drawn": a.nnz, "lambda": a.lam, "N": a.N,
           "warmup": a.warmup, "repeats": a.repeats}
    cmd = [sys.executable, os.path.abspath(__file__), "--step"] + [
        x for k in ("users", "items", "nnz", "lam", "N", "warmup", "repeats") for x in (f"--{k}", str(getattr(a, k)))]
    print(f"step fit_and_score (at most {a.step_timeout} s)", flush=True)
    try:
        p = subprocess.run(cmd, capture_output=True, text=True, timeout=a.step_timeout)
        lines = [ln for ln in p.stdout.split("\n") if ln.startswith("STEP ")]
        if p.returncode != 0 or not lines:
            out["failed"] = f"exit status {p.returncode}"
            out["stderr_tail"] = p.stderr[-400:]
        else:
            out.update(json.loads(lines[-1][5:]))
    except subprocess.TimeoutExpired:
        out["failed"] = f"no result within {a.step_timeout} s"
    line = json.dumps(out)
    print(line)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(line + "\n")
    return 1 if "failed" in out else 0


if __name__ == "__main__":
    sys.exit(main())
