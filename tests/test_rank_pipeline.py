"""bin/rankeval on the factor files of bin/als and bin/ials, on a tiny movielens/ directory with
all three roles (the recipe of test_topn_pipeline.py, rebuilt here): every output row's rank lies
in the checker's window computed from the parsed factor files, n_cand is exact and the printed
summary equals the checker's after %g."""
import os
import subprocess

import numpy as np
import pytest

import pipeline_util as pu
import rank_ref as rr

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BIN = os.path.join(ROOT, "bin")
TOPN = 3


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


def run(wd, *cmd):
    return subprocess.run(list(cmd), cwd=wd, capture_output=True, text=True, timeout=120)


def fit(wd, which):
    extra = ["--threshold", "2"] if which == "ials" else ["--minval", "1", "--maxval", "5"]
    p = run(wd, os.path.join(BIN, which), "movielens/", "--D", "5", "--max_iter", "3", "--predictions", "out/p", "--seed", "1",
            *extra)
    assert p.returncode == 0, p.stdout + p.stderr


def rankeval(wd, *extra):
    return run(wd, os.path.join(BIN, "rankeval"), "--factors", "out/p", "--matrix", "movielens/", "--topn", str(TOPN), *extra)


def parse_factors(wd, prefix):
    out = {}
    for ln in pu.read_shards(wd, prefix):
        t = ln.split()
        out[int(t[0].rstrip(")"))] = np.array([float(x) for x in t[1:]])
    return out


def summary_of(stdout):
    """The three printed lines: (users, items, D), (evaluated, edges, skipped), {metric: value}."""
    ls = stdout.split("\n")
    a = next(ln for ln in ls if ln.startswith("Users: ")).split()
    b = next(ln for ln in ls if ln.startswith("Evaluated users: ")).split()
    c = next(ln for ln in ls if ln.startswith("precision@N ")).split()
    return (int(a[1]), int(a[3]), int(a[5])), (int(b[2]), int(b[5]), int(b[7])), {c[k]: float(c[k + 1]) for k in range(0, len(c), 2)}


def checker(wd, lines, weighted):
    Ud, Vd = parse_factors(wd, "out/p.U_"), parse_factors(wd, "out/p.V_")
    uids, mids = sorted(Ud), sorted(Vd)
    U, V = np.array([Ud[u] for u in uids]), np.array([Vd[m] for m in mids])
    urow, mrow = {u: k for k, u in enumerate(uids)}, {m: k for k, m in enumerate(mids)}
    train = [ln.replace(",", " ").split() for ln in lines["train"]]
    val = [ln.split() for ln in lines["validate"]]
    excl = (np.array([urow[int(t[0])] for t in train]), np.array([mrow[int(t[1])] for t in train]))
    held = (np.array([urow[int(t[0])] for t in val]), np.array([mrow[int(t[1])] for t in val]),
            np.array([float(t[2]) for t in val]) if weighted else None)
    rank, n_cand, users, s = rr.evaluate(U, V, TOPN, held, exclude=excl)
    lo, hi, gap, bmax = rr.rank_windows(U, V, held, exclude=excl)
    want = {(int(t[0]), int(t[1])): (int(lo[k]), int(hi[k]), int(n_cand[k])) for k, t in enumerate(val)}
    return want, s, (lo, hi, gap, bmax)


def check_rows(wd, want):
    got = {}
    for f in sorted(os.listdir(os.path.join(wd, "out"))):
        if not f.startswith("r_"):
            continue
        shard = int(f.split("_")[1])
        for ln in open(os.path.join(wd, "out", f)).read().split("\n"):
            if ln:
                a, b, c, d = ln.split("\t")
                assert int(a) % 4 + 1 == shard and f.endswith("_of_4")
                assert (int(a), int(b)) not in got
                got[(int(a), int(b))] = (int(c), int(d))
    assert set(got) == set(want)
    for k, (r, c) in got.items():
        lo, hi, n_cand = want[k]
        assert c == n_cand, (k, c, n_cand)
        if lo == rr.MAX:
            assert r == -1, (k, r)
        else:
            assert lo <= r <= hi, (k, r, lo, hi)


@pytest.mark.parametrize("which", ["als", "ials"])
def test_rankeval_matches_checker(tmp_path, which):
    wd = str(tmp_path)
    lines = write_inputs(wd)
    fit(wd, which)
    p = rankeval(wd, "--output", "out/r")
    assert p.returncode == 0, p.stdout + p.stderr
    assert "Users: 40 items: 15 D: 5" in p.stdout
    want, s, (lo, hi, gap, bmax) = checker(wd, lines, False)
    single = float((lo == hi).mean())
    print(which, "held-out edges", len(lo), "single-rank windows", single, "smallest gap", gap, "largest bound", bmax)
    assert single >= 0.9   # against a vacuous pass: the windows pin the ranks
    check_rows(wd, want)
    _, (evaluated, edges, skipped), printed = summary_of(p.stdout)
    assert (evaluated, edges, skipped) == (s["users_evaluated"], len(lines["validate"]), s["edges_skipped"])
    assert skipped == 0   # a VALIDATE edge is no TRAIN edge
    for name, key in (("precision@N", "precision"), ("recall@N", "recall"), ("ndcg@N", "ndcg"), ("map@N", "map"),
                      ("mrr", "mrr"), ("auc", "auc"), ("mpr", "mpr")):
        assert printed[name] == float("%g" % s[key]), (name, printed[name], s[key])

    # --weighted changes mpr alone
    pw = rankeval(wd, "--weighted")
    assert pw.returncode == 0, pw.stdout + pw.stderr
    _, counts_w, printed_w = summary_of(pw.stdout)
    _, sw, _ = checker(wd, lines, True)
    assert counts_w == (evaluated, edges, skipped)
    assert {k: v for k, v in printed_w.items() if k != "mpr"} == {k: v for k, v in printed.items() if k != "mpr"}
    assert printed_w["mpr"] == float("%g" % sw["mpr"]) and printed_w["mpr"] != printed["mpr"]


def test_factor_line_of_another_width_is_fatal(tmp_path):
    wd = str(tmp_path)
    write_inputs(wd)
    fit(wd, "als")
    f = sorted(x for x in os.listdir(os.path.join(wd, "out")) if x.startswith("p.V_"))[-1]
    with open(os.path.join(wd, "out", f), "a") as fh:
        fh.write("999) 0.5 0.25 \n")
    p = rankeval(wd)
    assert p.returncode != 0
    assert "factor line of another width" in p.stderr and f in p.stderr


def test_matrix_id_missing_from_factors_is_fatal(tmp_path):
    wd = str(tmp_path)
    write_inputs(wd)
    fit(wd, "als")
    # after the fit, the directory gains an item, then a user, that the factor files do not know
    train = os.path.join(wd, "movielens", "r.train")
    before = open(train).read()
    open(train, "w").write(before + "3\t777\t4\n")
    p = rankeval(wd)
    assert p.returncode != 0 and "item 777 of movielens/ has no line in out/p.V_*" in p.stderr
    open(train, "w").write(before)
    with open(os.path.join(wd, "movielens", "r.validate"), "a") as fh:
        fh.write("555 101 4\n")
    p = rankeval(wd)
    assert p.returncode != 0 and "user 555 of movielens/ has no line in out/p.U_*" in p.stderr
