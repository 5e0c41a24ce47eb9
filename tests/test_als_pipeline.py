"""bin/als, the drop-in for als.cpp, on a tiny movielens/ directory with all three roles."""
import os
import subprocess

import numpy as np
import pytest

import pipeline_util as pu

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BIN = os.path.join(ROOT, "bin", "als")


def write_inputs(wd, bad_rating=False):
    rng = np.random.default_rng(4)
    ml = os.path.join(wd, "movielens")
    os.makedirs(ml, exist_ok=True)
    os.makedirs(os.path.join(wd, "out"), exist_ok=True)
    lines = {"train": [], "validate": [], "predict": []}
    for u in range(1, 41):
        for m in rng.choice(15, size=int(rng.integers(4, 9)), replace=False) + 100:
            r = int(rng.integers(1, 6))
            x = rng.random()
            if x < 0.7:   # the three separators the loader accepts
                lines["train"].append(f"{u}\t{m}\t{r}\n" if u % 3 else (f"{u},{m},{r}\n" if u % 2 else f"{u} {m} {r}\n"))
            elif x < 0.85:
                lines["validate"].append(f"{u} {m} {r}\n")
            else:
                lines["predict"].append(f"{u}\t{m}\n")
    if bad_rating:
        lines["train"].append("3\t101\t9\n")
    for role, ls in lines.items():
        open(os.path.join(ml, "r.train" if role == "train" else f"r.{role}"), "w").writelines(ls)
    return lines


def parse_triplets(ls):
    return [ln.replace(",", " ").split() for ln in ls]


def test_stage_als(tmp_path):
    wd = str(tmp_path)
    lines = write_inputs(wd)
    p = subprocess.run([BIN, "movielens/", "--D", "5", "--max_iter", "3", "--predictions", "out/p", "--seed", "1",
                        "--minval", "1", "--maxval", "5", "--engine", "synchronous", "--interval", "10"],
                       cwd=wd, capture_output=True, text=True, timeout=120)
    assert p.returncode == 0, p.stdout + p.stderr
    out = p.stdout
    assert f"Training edges: {len(lines['train'])} validation edges: {len(lines['validate'])}" in out
    assert "Updates executed: " in out
    U, V = {}, {}
    for ln in pu.read_shards(wd, "out/p.U_"):
        t = ln.split()
        U[int(t[0])] = np.array([float(x) for x in t[1:]])
    for ln in pu.read_shards(wd, "out/p.V_"):
        t = ln.split()
        assert t[0].endswith(")")
        V[int(t[0][:-1])] = np.array([float(x) for x in t[1:]])
    every = parse_triplets(lines["train"] + lines["validate"] + lines["predict"])
    assert set(U) == {int(t[0]) for t in every} and set(V) == {int(t[1]) for t in every}
    assert all(len(f) == 5 for f in list(U.values()) + list(V.values()))
    updates = int(out.split("Updates executed: ")[1].split()[0])
    assert len(U) <= updates <= 3 * (len(U) + len(V))
    preds = [ln.split("\t") for ln in pu.read_shards(wd, "out/p_")]
    assert sorted((int(a), int(b)) for a, b, _ in preds) == sorted((int(t[0]), int(t[1])) for t in parse_triplets(lines["predict"]))
    for a, b, c in preds:   # printed with 6 significant digits
        assert float(c) == float("%g" % float(U[int(a)] @ V[int(b)])), (a, b, c)
    rm = out.split("Training RMSE: ")[1].split("\n")[0]
    got = [float(rm.split("\t")[0]), float(rm.split("Validation RMSE: ")[1])]
    for role, g in zip(("train", "validate"), got):
        t = parse_triplets(lines[role])
        pred = np.array([np.clip(U[int(a)] @ V[int(b)], 1.0, 5.0) for a, b, _ in t])
        want = np.sqrt(np.mean((np.array([float(r) for _, _, r in t]) - pred) ** 2))
        assert abs(g - want) <= 1e-5 * max(1.0, want), (role, g, want)


def test_rating_outside_range_is_fatal(tmp_path):
    wd = str(tmp_path)
    write_inputs(wd, bad_rating=True)
    p = subprocess.run([BIN, "--matrix", "movielens/", "--D", "5", "--minval", "1", "--maxval", "5"], cwd=wd,
                       capture_output=True, text=True, timeout=120)
    assert p.returncode != 0
    assert "Rating values should be between 1 and 5. Got value: 9 [ user: 3 to item: 101 ]" in p.stderr
