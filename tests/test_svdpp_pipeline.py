"""bin/svdpp, the drop-in for svdpp.cpp, on the tiny three-role movielens/ directory of
test_als_pipeline.py: the .validate and .predict edges are its implicit list."""
import os
import subprocess

import numpy as np
import pytest

import pipeline_util as pu
from test_als_pipeline import parse_triplets, write_inputs
from test_sgd_pipeline import read_vertex_file

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
STEPS = ["user_bias_step", "item_bias_step", "user_factor_step", "item_factor_step", "item_factor2_step"]
REGS = ["user_bias_reg", "item_bias_reg", "user_factor_reg", "item_factor_reg", "item_factor2_reg"]
COMMON = ["--D", "5", "--seed", "1", "--minval", "1", "--maxval", "5", "--lambda", "0.05", "--gamma", "0.02", "--tol", "0.5"]
for _k in STEPS:
    COMMON += ["--" + _k, "0.02"]
for _k in REGS:
    COMMON += ["--" + _k, "0.05"]


def run(wd, *args):
    return subprocess.run([os.path.join(ROOT, "bin", "svdpp"), *args], cwd=wd, capture_output=True, text=True, timeout=120)


def test_stage(tmp_path, gpu_ctx):
    wd = str(tmp_path)
    lines = write_inputs(wd)
    p = run(wd, "movielens/", *COMMON, "--max_iter", "4", "--predictions", "out/p", "--engine", "synchronous",
            "--interval", "0")
    assert p.returncode == 0, p.stdout + p.stderr
    out = p.stdout
    train, val, prd = (parse_triplets(lines[k]) for k in ("train", "validate", "predict"))
    assert f"Training edges: {len(train)} validation edges: {len(val)}" in out and "Running SVD++" in out
    mean = float(np.mean([float(r) for _, _, r in train]))
    assert float(out.split("Global mean is: ")[1].split()[0]) == float("%g" % mean)
    # one "time train_rmse validate_rmse" line per user superstep of either phase: --max_iter 4 gives four
    body = out.split("RMSE        RMSE \n")[1].split("-----")[0].strip().split("\n")
    rows = [[float(x) for x in ln.split()] for ln in body]
    assert len(rows) == 4 and all(len(r) == 3 for r in rows), body
    assert "Supersteps: 8 " in out and "Updates executed: " in out
    # the five files, in the reference's line formats: "id f0 .. f4 " and "id bias"; no weight file
    U, V = read_vertex_file(wd, "out/p.U_", False), read_vertex_file(wd, "out/p.V_", False)
    every = train + val + prd
    assert set(U) == {int(t[0]) for t in every} and set(V) == {int(t[1]) for t in every}
    assert all(len(f) == 5 for f in list(U.values()) + list(V.values()))
    assert all(ln.endswith(" ") and len(ln.split(" ")) == 7 for ln in pu.read_shards(wd, "out/p.U_"))
    bu = {k: float(v[0]) for k, v in read_vertex_file(wd, "out/p.bias.U_", False).items()}
    bi = {k: float(v[0]) for k, v in read_vertex_file(wd, "out/p.bias.V_", False).items()}
    assert set(bu) == set(U) and set(bi) == set(V) and any(v != 0.0 for v in bi.values())
    assert all(len(ln.split(" ")) == 2 for ln in pu.read_shards(wd, "out/p.bias.V_"))
    names = {f.split("_")[0] for f in os.listdir(os.path.join(wd, "out"))}
    assert names == {"p", "p.U", "p.V", "p.bias.U", "p.bias.V"}, names
    # the final error line is extract_l2_error: without Y, from the written factors
    rm = out.split("Training RMSE: ")[1].split("\n")[0]
    got = [float(rm.split("\t")[0]), float(rm.split("Validation RMSE: ")[1])]
    for t, g in zip((train, val), got):
        pred = np.array([np.clip(mean + bu[int(a)] + bi[int(b)] + float(U[int(a)] @ V[int(b)]), 1.0, 5.0) for a, b, _ in t])
        want = np.sqrt(np.mean((np.array([float(r) for _, _, r in t]) - pred) ** 2))
        assert abs(g - want) <= 1e-5 * max(1.0, want), (g, want)
    # the predictions use Y, which is not saved: the same fit through Context.svdpp_fit, from the
    # binary's documented initial draw, gives the factors again and the Y they belong to
    uid, mid = sorted(U), sorted(V)
    ui, mi = {k: n for n, k in enumerate(uid)}, {k: n for n, k in enumerate(mid)}
    D = 5
    mats = [binary_draw(len(uid), D, 1, 0), binary_draw(len(mid), D, 1, 1), binary_draw(len(uid), D, 1, 2),
            binary_draw(len(mid), D, 1, 3)]
    tu = np.array([ui[int(a)] for a, _, _ in train], np.uint32)
    tm = np.array([mi[int(b)] for _, b, _ in train], np.uint32)
    to = np.array([float(r) for _, _, r in train], np.float32)
    # the first line follows a phase-1 superstep, which moves neither U nor V: the error of the initial draw
    first = np.sqrt(np.mean((to - np.clip(mean + np.einsum("ij,ij->i", mats[0][tu], mats[1][tm]), 1.0, 5.0)) ** 2))
    assert abs(rows[0][1] - first) <= 1e-5 * first and rows[1][1] != rows[0][1]
    imp = ([ui[int(t[0])] for t in val + prd], [mi[int(t[1])] for t in val + prd])
    hyper = {k: 0.02 for k in STEPS}
    hyper.update({k: 0.05 for k in REGS})
    r = gpu_ctx.svdpp_fit(tu, tm, to, len(uid), len(mid), *mats, implicit=imp, max_updates=4, minval=1.0, maxval=5.0,
                          step_dec=0.9, **hyper)
    assert r.supersteps == 8
    tol = 1e-12 * max(np.max(np.abs(r.U)), np.max(np.abs(r.V)))   # test_gpu_svdpp.py's bound: edge order may differ
    for n, k in enumerate(uid):
        assert np.max(np.abs(U[k] - r.U[n])) <= tol and abs(bu[k] - r.bias_user[n]) <= tol
    for n, k in enumerate(mid):
        assert np.max(np.abs(V[k] - r.V[n])) <= tol and abs(bi[k] - r.bias_item[n]) <= tol
    preds = [ln.split("\t") for ln in pu.read_shards(wd, "out/p_")]
    assert sorted((int(a), int(b)) for a, b, _ in preds) == sorted((int(t[0]), int(t[1])) for t in prd)
    pu_, pm_ = np.array([ui[int(a)] for a, _, _ in preds], np.uint32), np.array([mi[int(b)] for _, b, _ in preds], np.uint32)
    want = gpu_ctx.svdpp_predict(pu_, pm_, r.U, r.V, r.Y, r.bias_user, r.bias_item, r.global_mean, 1.0, 5.0)
    no_y = gpu_ctx.sgd_predict(pu_, pm_, r.U, r.V, r.bias_user, r.bias_item, r.global_mean, minval=1.0, maxval=5.0)
    assert [float(c) for _, _, c in preds] == [float("%g" % w) for w in want]
    assert [float(c) for _, _, c in preds] != [float("%g" % w) for w in no_y]


def binary_draw(n, D, seed, side):
    """cf_mf_cli.hpp's reproducible initial draw: element d of vertex i on `side` (0 U, 1 V, 2 W, 3 Y)."""
    M = (1 << 64) - 1

    def sm(x):
        x = (x + 0x9E3779B97F4A7C15) & M
        x = ((x ^ (x >> 30)) * 0xBF58476D1CE4E5B9) & M
        x = ((x ^ (x >> 27)) * 0x94D049BB133111EB) & M
        return x ^ (x >> 31)

    key = sm((seed + 0x9E3779B97F4A7C15 * (side + 1)) & M)
    return np.array([[2.0 * ((sm(key ^ (64 * i + d)) >> 11) * (1.0 / 9007199254740992.0)) - 1.0 for d in range(D)]
                     for i in range(n)])


def test_refusals(tmp_path):
    wd = str(tmp_path)
    write_inputs(wd)
    p = run(wd, "--matrix", "movielens/", *COMMON)
    assert p.returncode != 0 and "--max_iter or --max_supersteps is required" in p.stderr
    p = run(wd, "--matrix", "movielens/", *COMMON, "--max_iter", "2", "--interval", "1")
    assert p.returncode != 0 and "--interval other than 0 is not supported" in p.stderr
    p = run(wd, "--matrix", "movielens/", *COMMON, "--max_iter", "2", "--implicitratingtype", "1")
    assert p.returncode != 0 and "--implicitratingtype other than 0" in p.stderr
    p = run(wd, "--matrix", "movielens/", *COMMON, "--max_supersteps", "3")   # a cap of the other kind is enough
    assert p.returncode == 0 and "Supersteps: 3 " in p.stdout, p.stdout + p.stderr


def test_rating_outside_range_is_fatal(tmp_path):
    wd = str(tmp_path)
    write_inputs(wd, bad_rating=True)
    p = run(wd, "--matrix", "movielens/", *COMMON, "--max_iter", "2")
    assert p.returncode != 0
    assert "Rating values should be between 1 and 5. Got value: 9 [ user: 3 to item: 101 ]" in p.stderr
