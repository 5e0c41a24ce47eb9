"""Item-kNN top-N probe: cf_knn_topn at the shape of the other top-N probes (default 200k users x
20k items, the ALS probe's synthetic ratings as profiles, about 100 per user, N = 10) on a
synthetic CSR graph of --degree out-neighbours per item (default 300, uniform random columns,
weights uniform in (0, 1), so about 0.9 x degree entries per in-list at w_min = 0.1).  Every GPU
step runs in a child process of its own under a time limit and is not tried again; the first
step that fails ends the probe.  Prints one JSON line and writes it to --out
(profiles/knn_topn/probe.json).  A probe, not a gate: no target is set.

  uniform   SUM and MEAN mode, score_ms and select_ms as the medians of --repeats calls after
            --warmup calls with cached in-lists; the in-list build as the score_ms of calls that
            rebuild them (another w_min of the same effect) minus that median; cf_mf_topn on
            random factors at the same shape, exclusions and N in the same process
  skewed    the same edge count with users drawn by a power law (exponent 0.8), so the heaviest
            profile is about the whole catalogue: the tail of one workgroup per user
  uniform_wgs<w>  (--wgs-sweep w,..) the uniform step's two modes with CF_KNN_TOPN_WGS=w: w users
            in flight per CU instead of the library's default, in the same run

Work model: a profile entry (i, r) costs |in(i)| read-modify-writes of an 8-byte
accumulator (16 in MEAN mode) plus the 8 bytes of the in-list entry: bytes_implied counts 8 read +
8 written per plane + 8 of the entry.  What the memory system moves is more: a user's accumulators
are 8 n_items bytes (160 kB here), and the rows of all the workgroups in flight together do not
fit the L2, so an update costs a cache line each way, not 8 bytes.

    python tools/knn_topn_probe.py [--users N --items M --nnz E --degree K --N n --out FILE]"""
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

W_MIN = 0.1
W_MIN_REBUILD = 0.1 + 2.0 ** -40   # no weight of the graph lies between the two


def graph(n, degree, seed=3):
    """CSR (row_ptr, col, w): per row `degree` uniform draws of a column, repeats dropped."""
    rng = np.random.default_rng(seed)
    col = np.sort(rng.integers(0, n, (n, degree), dtype=np.int64), axis=1)
    keep = np.ones(col.shape, dtype=bool)
    keep[:, 1:] = col[:, 1:] != col[:, :-1]
    w = rng.random(col.shape, dtype=np.float32)
    rp = np.zeros(n + 1, dtype=np.uint64)
    rp[1:] = np.cumsum(keep.sum(axis=1))
    return rp, col[keep].astype(np.uint32), w[keep]


def profiles(n_users, n_items, nnz, skew, seed=0):
    """(off, item, rating) sorted by user then item: the ALS probe's ratings, or with users drawn by
    a power law (skew > 0)."""
    from als_probe import synth

    if skew <= 0:
        user, item, obs = synth(n_users, n_items, nnz, seed)
    else:
        rng = np.random.default_rng(seed)
        pi = 1.0 / np.arange(1, n_items + 1) ** 0.6
        pu = 1.0 / np.arange(1, n_users + 1) ** skew
        it = rng.choice(n_items, size=nnz, p=pi / pi.sum()).astype(np.int64)
        us = rng.choice(n_users, size=nnz, p=pu / pu.sum()).astype(np.int64)
        key = np.unique(us * n_items + it)
        user, item = (key // n_items).astype(np.uint32), (key % n_items).astype(np.uint32)
        obs = rng.integers(1, 6, len(key)).astype(np.float32)
    off = np.zeros(n_users + 1, dtype=np.uint64)
    off[1:] = np.cumsum(np.bincount(user, minlength=n_users))
    return off, user, item, obs


def med(xs):
    return round(float(np.median(xs)), 3)


def step(a):
    """One GPU step in this process; prints its JSON."""
    if a.wgs:
        os.environ["CF_KNN_TOPN_WGS"] = str(a.wgs)   # read once per context
    from collaborative_filtering_amd.api import Context

    rp, col, w = graph(a.items, a.degree)
    in_len = np.bincount(col[w.astype(np.float64) > W_MIN], minlength=a.items)
    off, user, item, obs = profiles(a.users, a.items, a.nnz, 0.8 if a.step == "skewed" else 0.0)
    plen = np.diff(off.astype(np.int64))
    rmw = int(in_len[item].sum())
    per_user = np.add.reduceat(in_len[item], off[:-1].astype(np.int64)[plen > 0]) if len(item) else np.zeros(1)
    out = {"profile_entries": int(len(item)), "profile_len_mean": round(float(plen.mean()), 2),
           "profile_len_max": int(plen.max()), "in_list_mean": round(float(in_len.mean()), 2),
           "in_list_max": int(in_len.max()), "rmw_per_call": rmw, "rmw_heaviest_user": int(per_user.max()),
           "rmw_heaviest_user_share": round(float(per_user.max()) / max(rmw, 1), 6)}
    out["CF_KNN_TOPN_WGS"] = a.wgs
    with Context(0) as ctx:
        ctx.set_graph_layout("csr")
        ctx.upload_graph_csr(a.items, rp, col, w)
        for mode in ("sum", "mean"):
            score, select, build = [], [], []
            for k in range(a.warmup + a.repeats):
                r = ctx.knn_topn(off, item, obs, a.N, mode=mode, w_min=W_MIN)
                if k >= a.warmup:
                    score.append(float(r.stats.score_ms))
                    select.append(float(r.stats.select_ms))
            for k in range(a.repeats if mode == "sum" else 0):   # calls that rebuild the in-lists
                r = ctx.knn_topn(off, item, obs, a.N, mode=mode, w_min=W_MIN_REBUILD if k % 2 == 0 else W_MIN)
                build.append(float(r.stats.score_ms) - float(np.median(score)))
            planes = 2 if mode == "mean" else 1
            out[mode] = {"score_ms": med(score), "select_ms": med(select), "score_ms_runs": [round(x, 3) for x in score],
                         "select_ms_runs": [round(x, 3) for x in select], "blocks": int(r.stats.blocks),
                         "n_nan": int(r.stats.n_nan),
                         "rmw_per_s": round(planes * rmw / (np.median(score) * 1e-3), 1),
                         "bytes_implied": (16 * planes + 8) * rmw,
                         "bytes_implied_per_s": round((16 * planes + 8) * rmw / (np.median(score) * 1e-3), 1)}
            if build:
                out["in_list_build_ms"] = med(build)
                out["in_list_build_ms_runs"] = [round(x, 3) for x in build]
        if a.step == "uniform":
            rng = np.random.default_rng(1)
            U, V = rng.uniform(-1, 1, (a.users, a.D)), rng.uniform(-1, 1, (a.items, a.D))   # the top-N probe's factors
            score, select = [], []
            for k in range(a.warmup + a.repeats):
                t = ctx.mf_topn(U, V, a.N, exclude=(user, item))
                if k >= a.warmup:
                    score.append(float(t.stats.score_ms))
                    select.append(float(t.stats.select_ms))
            out["mf_topn"] = {"D": a.D, "score_ms": med(score), "select_ms": med(select)}
    print("STEP " + json.dumps(out))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--users", type=int, default=200_000)
    ap.add_argument("--items", type=int, default=20_000)
    ap.add_argument("--nnz", type=int, default=20_000_000)
    ap.add_argument("--degree", type=int, default=300)
    ap.add_argument("--D", type=int, default=20)
    ap.add_argument("--N", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--step-timeout", type=int, default=300)
    ap.add_argument("--step", default="")
    ap.add_argument("--wgs", type=int, default=0, help="CF_KNN_TOPN_WGS of a step (0: the library's default)")
    ap.add_argument("--wgs-sweep", default="", help="comma-separated CF_KNN_TOPN_WGS values: one more uniform step each")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "knn_topn", "probe.json"))
    a = ap.parse_args()
    if a.step:
        return step(a)
    out = {"probe": "knn_topn", "users": a.users, "items": a.items, "nnz_drawn": a.nnz, "graph_degree": a.degree,
           "graph_layout": "csr", "w_min": W_MIN, "N": a.N, "warmup": a.warmup, "repeats": a.repeats}
    steps = [("uniform", "uniform", 0), ("skewed", "skewed", 0)]
    steps += [(f"uniform_wgs{int(v)}", "wgs", int(v)) for v in a.wgs_sweep.split(",") if v]
    for name, kind, wgs in steps:
        cmd = [sys.executable, os.path.abspath(__file__), "--step", kind, "--wgs", str(wgs)] + [
            x for k in ("users", "items", "nnz", "degree", "D", "N", "warmup", "repeats") for x in (f"--{k}", str(getattr(a, k)))]
        print(f"step {name} (at most {a.step_timeout} s)", flush=True)
        try:
            p = subprocess.run(cmd, capture_output=True, text=True, timeout=a.step_timeout)
        except subprocess.TimeoutExpired:
            out[name] = {"failed": f"no result within {a.step_timeout} s"}
            break
        lines = [ln for ln in p.stdout.split("\n") if ln.startswith("STEP ")]
        if p.returncode != 0 or not lines:
            out[name] = {"failed": f"exit status {p.returncode}", "stderr_tail": p.stderr[-400:]}
            break   # nothing more is started on the GPU
        out[name] = json.loads(lines[-1][5:])
    line = json.dumps(out)
    print(line)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(line + "\n")
    return 0 if all("failed" not in out.get(n, {"failed": 1}) for n, _, _ in steps) else 1


if __name__ == "__main__":
    sys.exit(main())
