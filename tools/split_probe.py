"""Split probe: the device time of cf_holdout_split by step on the rating set of bench.py's prep leg
(config 2: 100k users x 10k items, about 10.7M ratings, resident on the device), the rounds of a
5/5 core on it, and for comparison the time of the numpy checker tests/split_ref.py on the same
input on the host.  Four rules are timed: leave-2-out with the 5/5 core (random order), with a
100/200 core (one that takes rounds on this set), without a core, and 5 folds.  The GPU step runs in a child process of its own under a time limit
and is not tried again.  Prints one JSON line and writes it to --out (profiles/split/probe.json).
A probe, not a gate: no target is set.

Work model: four stable sorts of n entries (64-bit keys with 32-bit values twice,
32-bit keys with 32-bit values twice), each reading and writing its keys and values once per merge
pass, plus about 5 B per edge and core round; sort_bytes_model counts one pass of each sort.

    python tools/split_probe.py [--users N --items M --repeats R --no-host --out FILE]"""
from __future__ import annotations

import argparse
import json
import os
import subprocess
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

SEED = 2026101502   # bench.py CONFIGS["c2"]
STATS = ("kept", "alive", "users_alive", "items_alive", "train", "validate", "items_without_train", "rounds")


def ratings(n_users, n_items):
    from collaborative_filtering_amd import synth

    k = synth.degrees(SEED, n_users, k_median=100.0, sigma=0.5, kmin=20, kmax=180)
    off, items, _ = synth.user_items(SEED, k, n_items, threads=16)
    user = np.repeat(np.arange(n_users, dtype=np.uint32), k.astype(np.int64))
    return user, np.ascontiguousarray(items, dtype=np.uint32)


def step(a):
    """The GPU step in this process; prints its JSON."""
    import torch

    from collaborative_filtering_amd import _native
    from collaborative_filtering_amd._native import ptr
    from collaborative_filtering_amd.api import Context

    user, item = ratings(a.users, a.items)
    n = len(user)
    T = lambda x: torch.from_numpy(np.ascontiguousarray(x)).to("cuda:0")   # noqa: E731
    d_user, d_item = T(user.view(np.int32)), T(item.view(np.int32))
    d_part = torch.zeros(n, dtype=torch.uint8, device="cuda:0")
    d_stats = torch.zeros(8, dtype=torch.int64, device="cuda:0")
    torch.cuda.synchronize()
    out = {"edges": n, "sort_bytes_model": n * 2 * (12 + 8 + 12 + 8), "rules": {}}
    # the 100/200 core is there to make the rounds do something: this set's items all have 5 raters
    rules = {"leave2_core5": (_native.CF_SPLIT_LEAVE_K, 2, 0, 5, 5),
             "leave2_core100_200": (_native.CF_SPLIT_LEAVE_K, 2, 0, 100, 200),
             "leave2": (_native.CF_SPLIT_LEAVE_K, 2, 0, 0, 0), "folds5": (_native.CF_SPLIT_FOLDS, 5, 0, 0, 0)}
    with Context(0) as ctx:
        for name, (mode, x, y, mu, mi) in rules.items():
            runs = []
            for _ in range(a.warmup + a.repeats):
                rc = ctx.lib.cf_holdout_split_run(ctx.h, n, a.users, a.items, ptr(d_user), ptr(d_item), None, 7, mu, mi, mode,
                                                  x, y, 3, ptr(d_part), ptr(d_stats), None)
                ctx._chk(rc, "cf_holdout_split_run")
                runs.append([float(t) for t in ctx.split_timing()] + [float(ctx.prep_timing())])
            runs = np.array(runs[a.warmup:])
            med = [round(float(np.median(runs[:, k])), 3) for k in range(5)]
            out["rules"][name] = {"lists_ms": med[0], "core_ms": med[1], "order_ms": med[2], "parts_ms": med[3],
                                  "total_ms": med[4], "edges_per_s": round(n / (med[4] * 1e-3), 1),
                                  "sort_model_bytes_per_s": round(out["sort_bytes_model"] / ((med[0] + med[2]) * 1e-3), 1),
                                  "runs_total_ms": [round(float(t), 3) for t in runs[:, 4]],
                                  "stats": dict(zip(STATS, (int(s) for s in d_stats.cpu().numpy())))}
        if not a.no_host:
            import split_ref as sr

            part = d_part.cpu().numpy()   # the last rule's: folds5
            t0 = time.perf_counter()
            want, wstats = sr.holdout_split(user, item, a.users, a.items, sr.FOLDS, 5, seed=7, min_train=3)
            out["host_checker_folds5_s"] = round(time.perf_counter() - t0, 3)
            out["host_equal"] = bool(np.array_equal(part, want) and list(wstats) == list(out["rules"]["folds5"]["stats"].values()))
            t0 = time.perf_counter()
            _, rounds = sr.kcore(user, item, a.users, a.items, 5, 5)
            out["host_checker_core5_s"] = round(time.perf_counter() - t0, 3)
            out["host_core_rounds_equal"] = rounds == out["rules"]["leave2_core5"]["stats"]["rounds"]
            keep, rounds = sr.kcore(user, item, a.users, a.items, 100, 200)
            st = out["rules"]["leave2_core100_200"]["stats"]
            out["host_core100_200_equal"] = bool(rounds == st["rounds"] and int(keep.sum()) == st["alive"])
    print("STEP " + json.dumps(out))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--users", type=int, default=100_000)
    ap.add_argument("--items", type=int, default=10_000)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--no-host", action="store_true")
    ap.add_argument("--step-timeout", type=int, default=400)
    ap.add_argument("--step", action="store_true")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "split", "probe.json"))
    a = ap.parse_args()
    if a.step:
        return step(a)
    out = {"probe": "split", "users": a.users, "items": a.items, "warmup": a.warmup, "repeats": a.repeats}
    cmd = [sys.executable, os.path.abspath(__file__), "--step"] + [
        x for k in ("users", "items", "warmup", "repeats") for x in (f"--{k}", str(getattr(a, k)))]
    if a.no_host:
        cmd.append("--no-host")
    print(f"step split (at most {a.step_timeout} s)", flush=True)
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
