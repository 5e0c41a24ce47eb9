"""bin/nmf on a tiny movielens/ directory with all three roles (the recipe of
test_ials_pipeline.py, rebuilt here), then bin/recommend and bin/rankeval on the factor files it
wrote."""
import os
import subprocess

import numpy as np
import pytest

import pipeline_util as pu

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BIN = os.path.join(ROOT, "bin")
SWEEPS = 3
D = 5


def write_inputs(wd):
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
    for role, ls in lines.items():
        open(os.path.join(ml, "r.train" if role == "train" else f"r.{role}"), "w").writelines(ls)
    return lines


def parse_triplets(ls):
    return [ln.replace(",", " ").split() for ln in ls]


def run(wd, *cmd):
    return subprocess.run(list(cmd), cwd=wd, capture_output=True, text=True, timeout=120)


@pytest.mark.parametrize("grid", [1, 0])
def test_stage_nmf_then_recommend_and_rankeval(tmp_path, grid):
    wd = str(tmp_path)
    lines = write_inputs(wd)
    p = run(wd, os.path.join(BIN, "nmf"), "movielens/", "--D", str(D), "--max_iter", str(SWEEPS), "--predictions", "out/p",
            "--seed", "1", "--grid", str(grid))
    assert p.returncode == 0, p.stdout + p.stderr
    out = p.stdout
    assert f"Training edges: {len(lines['train'])} validation edges: {len(lines['validate'])}" in out
    loss = [float(ln.split(": ")[1]) for ln in out.split("\n") if ln.startswith("loss after sweep")]
    assert len(loss) == 2 * SWEEPS and np.all(np.diff(loss) <= 0) and loss[-1] < loss[0], loss
    assert "Training RMSE: " in out and "\tValidation RMSE: " in out
    every = parse_triplets(lines["train"] + lines["validate"] + lines["predict"])
    train = parse_triplets(lines["train"])
    # only a vertex without TRAIN edges meets the floor, and only where the whole grid is fitted
    idle = len({int(t[0]) for t in every} - {int(t[0]) for t in train}) + len({int(t[1]) for t in every} - {int(t[1]) for t in train})
    floored = int(next(ln for ln in out.split("\n") if ln.startswith("Sweeps: ")).split("floored: ")[1])
    assert floored == (idle * D * SWEEPS if grid else 0)
    assert ("warning" in out) == (floored > 0)
    U, V = {}, {}
    for ln in pu.read_shards(wd, "out/p.U_"):
        t = ln.split()
        U[int(t[0])] = np.array([float(x) for x in t[1:]])
    for ln in pu.read_shards(wd, "out/p.V_"):
        t = ln.split()
        assert t[0].endswith(")")
        V[int(t[0][:-1])] = np.array([float(x) for x in t[1:]])
    assert set(U) == {int(t[0]) for t in every} and set(V) == {int(t[1]) for t in every}
    assert all(len(f) == D and np.all(f > 0) for f in list(U.values()) + list(V.values()))
    preds = [ln.split("\t") for ln in pu.read_shards(wd, "out/p_")]
    assert sorted((int(a), int(b)) for a, b, _ in preds) == sorted((int(t[0]), int(t[1])) for t in parse_triplets(lines["predict"]))
    for a, b, c in preds:   # unclamped, printed with 6 significant digits
        assert float(c) == float("%g" % float(U[int(a)] @ V[int(b)])), (a, b, c)

    rated = {(int(t[0]), int(t[1])) for t in parse_triplets(lines["train"] + lines["validate"])}
    p = run(wd, os.path.join(BIN, "recommend"), "--factors", "out/p", "--matrix", "movielens/", "--topn", "3", "--output",
            "out/r")
    assert p.returncode == 0, p.stdout + p.stderr
    assert "Users: 40 items: 15 D: 5" in p.stdout
    got = [ln.split("\t") for ln in pu.read_shards(wd, "out/r_")]
    assert len(got) >= 40 and not any((int(a), int(b)) in rated for a, b, _ in got)
    assert all(int(b) in V for _, b, _ in got)

    p = run(wd, os.path.join(BIN, "rankeval"), "--factors", "out/p", "--matrix", "movielens/", "--topn", "3", "--output",
            "out/e")
    assert p.returncode == 0, p.stdout + p.stderr
    assert "Users: 40 items: 15 D: 5" in p.stdout
    b = next(ln for ln in p.stdout.split("\n") if ln.startswith("Evaluated users: ")).split()
    assert (int(b[5]), int(b[7])) == (len(lines["validate"]), 0)      # every held-out edge ranked, none skipped
    held = {(int(t[0]), int(t[1])) for t in parse_triplets(lines["validate"])}
    tr = {(int(t[0]), int(t[1])) for t in train}
    rows = [ln.split("\t") for ln in pu.read_shards(wd, "out/e_")]
    assert {(int(r[0]), int(r[1])) for r in rows} == held and not any((int(r[0]), int(r[1])) in tr for r in rows)


def test_negative_rating_is_fatal(tmp_path):
    wd = str(tmp_path)
    write_inputs(wd)
    with open(os.path.join(wd, "movielens", "r.train"), "a") as fh:
        fh.write("3\t101\t-1\n")
    p = run(wd, os.path.join(BIN, "nmf"), "movielens/", "--D", "5", "--max_iter", "1")
    assert p.returncode != 0 and "Got value: -1 [ user: 3 to item: 101 ]" in p.stderr
