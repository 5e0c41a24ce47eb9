"""bin/sgd and bin/biassgd, the drop-ins for sgd.cpp and biassgd.cpp, on the tiny three-role
movielens/ directory of test_als_pipeline.py."""
import os
import subprocess

import numpy as np
import pytest

import pipeline_util as pu
from test_als_pipeline import parse_triplets, write_inputs

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
COMMON = ["--D", "5", "--gamma", "0.02", "--lambda", "0.05", "--tol", "0.5", "--seed", "1", "--minval", "1", "--maxval", "5"]


def run(name, wd, *args):
    return subprocess.run([os.path.join(ROOT, "bin", name), *args], cwd=wd, capture_output=True, text=True, timeout=120)


def read_vertex_file(wd, prefix, paren):
    out = {}
    for ln in pu.read_shards(wd, prefix):
        t = ln.split()
        assert t[0].endswith(")") == paren, ln
        out[int(t[0].rstrip(")"))] = np.array([float(x) for x in t[1:]])
    return out


@pytest.mark.parametrize("name", ["sgd", "biassgd"])
def test_stage(tmp_path, name):
    bias = name == "biassgd"
    wd = str(tmp_path)
    lines = write_inputs(wd)
    p = run(name, wd, "movielens/", *COMMON, "--max_iter", "3", "--predictions", "out/p", "--engine", "synchronous",
            "--interval", "0")
    assert p.returncode == 0, p.stdout + p.stderr
    out = p.stdout
    train, val = parse_triplets(lines["train"]), parse_triplets(lines["validate"])
    assert f"Training edges: {len(train)} validation edges: {len(val)}" in out
    mean = 0.0
    if bias:
        mean = float(np.mean([float(r) for _, _, r in train]))
        assert float(out.split("Global mean is: ")[1].split()[0]) == float("%g" % mean)
    else:
        assert "Global mean is" not in out
    # one "time train_rmse validate_rmse" line per user superstep: --max_iter 3 gives three
    body = out.split("RMSE        RMSE \n")[1].split("-----")[0].strip().split("\n")
    rows = [[float(x) for x in ln.split()] for ln in body]
    assert len(rows) == 3 and all(len(r) == 3 for r in rows), body
    assert "Supersteps: 6 " in out and "Updates executed: " in out
    U, V = read_vertex_file(wd, "out/p.U_", not bias), read_vertex_file(wd, "out/p.V_", not bias)
    every = parse_triplets(lines["train"] + lines["validate"] + lines["predict"])
    assert set(U) == {int(t[0]) for t in every} and set(V) == {int(t[1]) for t in every}
    assert all(len(f) == 5 for f in list(U.values()) + list(V.values()))
    bu = {k: 0.0 for k in U}
    bi = {k: 0.0 for k in V}
    if bias:
        bu = {k: float(v[0]) for k, v in read_vertex_file(wd, "out/p.bias.U_", False).items()}
        bi = {k: float(v[0]) for k, v in read_vertex_file(wd, "out/p.bias.V_", False).items()}
        assert set(bu) == set(U) and set(bi) == set(V) and any(v != 0.0 for v in bi.values())
    else:
        assert not [f for f in os.listdir(os.path.join(wd, "out")) if "bias" in f]

    def raw(a, b):
        return mean + bu[int(a)] + bi[int(b)] + float(U[int(a)] @ V[int(b)]) if bias else float(U[int(a)] @ V[int(b)])

    preds = [ln.split("\t") for ln in pu.read_shards(wd, "out/p_")]
    assert sorted((int(a), int(b)) for a, b, _ in preds) == sorted((int(t[0]), int(t[1])) for t in parse_triplets(lines["predict"]))
    for a, b, c in preds:   # printed with 6 significant digits; the bias saver clamps, the plain one does not
        want = float(np.clip(raw(a, b), 1.0, 5.0)) if bias else raw(a, b)
        assert float(c) == float("%g" % want), (a, b, c, want)
    rm = out.split("Training RMSE: ")[1].split("\n")[0]
    got = [float(rm.split("\t")[0]), float(rm.split("Validation RMSE: ")[1])]
    for t, g in zip((train, val), got):
        pred = np.array([np.clip(raw(a, b), 1.0, 5.0) for a, b, _ in t])
        want = np.sqrt(np.mean((np.array([float(r) for _, _, r in t]) - pred) ** 2))
        assert abs(g - want) <= 1e-5 * max(1.0, want), (g, want)
    # the last per-superstep line is taken before the last item superstep: not the final error
    assert rows[-1][1] != got[0]


@pytest.mark.parametrize("name", ["sgd", "biassgd"])
def test_refusals(tmp_path, name):
    wd = str(tmp_path)
    write_inputs(wd)
    p = run(name, wd, "--matrix", "movielens/", *COMMON)
    assert p.returncode != 0 and "--max_iter or --max_supersteps is required" in p.stderr
    p = run(name, wd, "--matrix", "movielens/", *COMMON, "--max_iter", "2", "--interval", "5")
    assert p.returncode != 0 and "--interval other than 0 is not supported" in p.stderr
    p = run(name, wd, "--matrix", "movielens/", *COMMON, "--max_supersteps", "3")   # a cap of the other kind is enough
    assert p.returncode == 0 and "Supersteps: 3 " in p.stdout, p.stdout + p.stderr


@pytest.mark.parametrize("name", ["sgd", "biassgd"])
def test_rating_outside_range_is_fatal(tmp_path, name):
    wd = str(tmp_path)
    write_inputs(wd, bad_rating=True)
    p = run(name, wd, "--matrix", "movielens/", *COMMON, "--max_iter", "2")
    assert p.returncode != 0
    assert "Rating values should be between 1 and 5. Got value: 9 [ user: 3 to item: 101 ]" in p.stderr
