"""bin/bpr on a tiny movielens/ directory with all three roles, then bin/rankeval and bin/recommend
on the factor files it wrote; the factor files against the Python fit with the same seed and
options."""
import os
import subprocess

import numpy as np
import pytest

import bpr_ref as br
import pipeline_util as pu

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BIN = os.path.join(ROOT, "bin")
SWEEPS, D, SEED, LR, REG = 6, 5, 3, 1.0, 0.02


def write_inputs(wd):
    rng = np.random.default_rng(9)
    ml = os.path.join(wd, "movielens")
    os.makedirs(ml, exist_ok=True)
    os.makedirs(os.path.join(wd, "out"), exist_ok=True)
    rows = {"train": [], "validate": [], "predict": []}
    for u in range(1, 41):
        for m in rng.choice(15, size=int(rng.integers(4, 9)), replace=False) + 100:
            x = rng.random()
            rows["train" if x < 0.7 else ("validate" if x < 0.85 else "predict")].append((u, int(m), int(rng.integers(1, 6))))
    rows["train"].append(rows["train"][0])   # a repeated pair: merged
    for role, ls in rows.items():
        with open(os.path.join(ml, f"r.{role}"), "w") as fh:
            fh.writelines(f"{u}\t{m}\n" if role == "predict" else f"{u}\t{m}\t{r}\n" for u, m, r in ls)
    return rows


def run(wd, *cmd):
    return subprocess.run(list(cmd), cwd=wd, capture_output=True, text=True, timeout=120)


def init_factors(n, seed, side):
    """host/cf_mf_cli.hpp's init_factors, times the 0.1 of bin/bpr."""
    key = br.sm((seed + 0x9E3779B97F4A7C15 * (side + 1)) & br.M64)
    return np.array([[0.1 * (2.0 * ((br.sm(key ^ (64 * i + d)) >> 11) * (1.0 / 9007199254740992.0)) - 1.0) for d in range(D)]
                     for i in range(n)])


def read_factors(wd, prefix, width):
    out = {}
    for ln in pu.read_shards(wd, prefix):
        t = ln.split()
        assert len(t) == width + 1
        out[int(t[0])] = np.array([float(x) for x in t[1:]])
    return out


@pytest.mark.parametrize("bias,minrating", [(1, None), (0, 3)])
def test_stage_bpr_then_rankeval_and_recommend(gpu_ctx, tmp_path, bias, minrating):
    wd = str(tmp_path)
    rows = write_inputs(wd)
    cmd = [os.path.join(BIN, "bpr"), "movielens/", "--D", str(D), "--max_iter", str(SWEEPS), "--lr", str(LR), "--reg", str(REG),
           "--bias", str(bias), "--seed", str(SEED), "--predictions", "out/p"]
    if minrating is not None:
        cmd += ["--minrating", str(minrating)]
    p = run(wd, *cmd)
    assert p.returncode == 0, p.stdout + p.stderr
    out = p.stdout
    assert f"Training edges: {len(rows['train'])} validation edges: {len(rows['validate'])}" in out
    pos = sorted({(u, m) for u, m, r in rows["train"] if minrating is None or r >= minrating})
    assert f"Positive pairs: {len(pos)}" in out
    every = rows["train"] + rows["validate"] + rows["predict"]
    uids, mids = sorted({t[0] for t in every}), sorted({t[1] for t in every})
    ui, mi = {x: k for k, x in enumerate(uids)}, {x: k for k, x in enumerate(mids)}
    # the Python fit with the same seed and options
    user, item = np.array([ui[u] for u, _ in pos]), np.array([mi[m] for _, m in pos])
    r = gpu_ctx.bpr_fit(user, item, len(uids), len(mids), init_factors(len(uids), SEED, 0), init_factors(len(mids), SEED, 1),
                        bias0=np.zeros(len(mids)) if bias else None, lr=LR, reg_user=REG, reg_item=REG, reg_bias=REG,
                        n_sweeps=SWEEPS, seed=SEED)
    lines = [ln.split() for ln in out.split("\n") if ln.startswith("loss at sweep")]
    assert len(lines) == SWEEPS
    for s, t in enumerate(lines):   # "loss at sweep k: mean triples: T skipped: S"
        assert int(t[3][:-1]) == s + 1 and int(t[6]) == int(r.loss_trace[s, 1]) and int(t[6]) + int(t[8]) == len(pos)
        assert float(t[4]) == r.loss_trace[s, 0] / r.loss_trace[s, 1]
    assert float(lines[-1][4]) < float(lines[0][4]) < 0.7
    U, V = read_factors(wd, "out/p.U_", D), read_factors(wd, "out/p.V_", D)
    bu, bi = read_factors(wd, "out/p.bias.U_", 1), read_factors(wd, "out/p.bias.V_", 1)
    assert sorted(U) == uids and sorted(V) == mids and sorted(bu) == uids and sorted(bi) == mids
    Uf, Vf = np.array([U[x] for x in uids]), np.array([V[x] for x in mids])
    bif = np.array([bi[x][0] for x in mids])
    assert Uf.tobytes() == r.U.tobytes() and Vf.tobytes() == r.V.tobytes()      # 17 digits: the same doubles
    assert all(v[0] == 0.0 for v in bu.values())
    assert bif.tobytes() == (r.bias_item if bias else np.zeros(len(mids))).tobytes() and (np.any(bif != 0) == bool(bias))
    preds = [ln.split("\t") for ln in pu.read_shards(wd, "out/p_")]
    assert sorted((int(a), int(b)) for a, b, _ in preds) == sorted((u, m) for u, m, _ in rows["predict"])
    for a, b, c in preds:
        assert float(c) == pytest.approx(float(U[int(a)] @ V[int(b)] + bi[int(b)][0]), rel=1e-5, abs=1e-9), (a, b, c)

    p = run(wd, os.path.join(BIN, "rankeval"), "--factors", "out/p", "--matrix", "movielens/", "--topn", "3", "--bias", "--mean",
            "0", "--output", "out/e")
    assert p.returncode == 0, p.stdout + p.stderr
    assert f"Users: {len(uids)} items: {len(mids)} D: {D}" in p.stdout
    held = sorted({(ui[u], mi[m]) for u, m, _ in rows["validate"]})
    train = sorted({(ui[u], mi[m]) for u, m, _ in rows["train"]})
    want = gpu_ctx.mf_rank_eval(r.U, r.V, 3, (np.array([h[0] for h in held]), np.array([h[1] for h in held])),
                                exclude=(np.array([t[0] for t in train]), np.array([t[1] for t in train])),
                                bias_user=np.zeros(len(uids)), bias_item=bif)
    t = next(ln for ln in p.stdout.split("\n") if ln.startswith("precision@N")).split()
    print(p.stdout)
    assert float(t[t.index("auc") + 1]) == float("%g" % want.summary["auc"])
    assert float(t[t.index("ndcg@N") + 1]) == float("%g" % want.summary["ndcg"])

    p = run(wd, os.path.join(BIN, "recommend"), "--factors", "out/p", "--matrix", "movielens/", "--topn", "3", "--bias", "--mean",
            "0", "--output", "out/r")
    assert p.returncode == 0, p.stdout + p.stderr
    rated = {(u, m) for u, m, _ in rows["train"] + rows["validate"]}
    got = [ln.split("\t") for ln in pu.read_shards(wd, "out/r_")]
    assert len(got) >= 40 and not any((int(a), int(b)) in rated for a, b, _ in got)


def test_bad_options_are_fatal(tmp_path):
    wd = str(tmp_path)
    write_inputs(wd)
    for opt in (("--D", "0"), ("--bias", "2"), ("--reg", "-1")):
        p = run(wd, os.path.join(BIN, "bpr"), "movielens/", "--max_iter", "1", *opt)
        assert p.returncode != 0, opt
