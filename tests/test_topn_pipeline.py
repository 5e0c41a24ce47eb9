"""bin/recommend on the factor files of bin/als and bin/sgd, on a tiny movielens/ directory with
all three roles (the recipe of test_als_pipeline.py, rebuilt here)."""
import os
import subprocess

import numpy as np
import pytest

import pipeline_util as pu
import topn_ref as tr

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
    p = run(wd, os.path.join(BIN, which), "movielens/", "--D", "5", "--max_iter", "3", "--predictions", "out/p", "--seed", "1",
            "--minval", "1", "--maxval", "5")
    assert p.returncode == 0, p.stdout + p.stderr


def parse_factors(wd, prefix):
    out = {}
    for ln in pu.read_shards(wd, prefix):
        t = ln.split()
        out[int(t[0].rstrip(")"))] = np.array([float(x) for x in t[1:]])
    return out


def check_lists(wd, lines):
    """out/r_* against topn_ref on the parsed factors: the same users, rank order, no TRAIN or
    VALIDATE item, scores equal after %g."""
    Ud, Vd = parse_factors(wd, "out/p.U_"), parse_factors(wd, "out/p.V_")
    uids, mids = sorted(Ud), sorted(Vd)
    U, V = np.array([Ud[u] for u in uids]), np.array([Vd[m] for m in mids])
    urow, mrow = {u: k for k, u in enumerate(uids)}, {m: k for k, m in enumerate(mids)}
    rated = [ln.replace(",", " ").split() for ln in lines["train"] + lines["validate"]]
    eu = np.array([urow[int(t[0])] for t in rated])
    em = np.array([mrow[int(t[1])] for t in rated])
    items, scores, count, _ = tr.topn(U, V, TOPN, exclude=(eu, em))
    want = {}
    for k, u in enumerate(uids):
        want[u] = [(mids[int(items[k, r])], float("%g" % scores[k, r])) for r in range(int(count[k]))]
    got = {}
    for f in sorted(os.listdir(os.path.join(wd, "out"))):
        if not f.startswith("r_"):
            continue
        shard = int(f.split("_")[1])
        for ln in open(os.path.join(wd, "out", f)).read().split("\n"):
            if ln:
                a, b, c = ln.split("\t")
                assert int(a) % 4 + 1 == shard and f.endswith("_of_4")
                got.setdefault(int(a), []).append((int(b), float(c)))   # file order is rank order
    assert set(got) == {u for u in uids if want[u]}
    excluded = {(int(t[0]), int(t[1])) for t in rated}
    for u, lst in got.items():
        assert not any((u, m) in excluded for m, _ in lst)
        assert lst == want[u], (u, lst, want[u])
    assert any(len(v) == TOPN for v in got.values())


@pytest.mark.parametrize("which", ["als", "sgd"])
def test_recommend_matches_checker(tmp_path, which):
    wd = str(tmp_path)
    lines = write_inputs(wd)
    fit(wd, which)
    # als writes "id " for users and "id) " for items, sgd "id) " for both
    assert all(ln.split()[0].endswith(")") for ln in pu.read_shards(wd, "out/p.V_"))
    assert all(ln.split()[0].endswith(")") == (which == "sgd") for ln in pu.read_shards(wd, "out/p.U_"))
    p = run(wd, os.path.join(BIN, "recommend"), "--factors", "out/p", "--matrix", "movielens/", "--topn", str(TOPN),
            "--output", "out/r")
    assert p.returncode == 0, p.stdout + p.stderr
    assert "Users: 40 items: 15 D: 5" in p.stdout and "scoring kernels:" in p.stdout
    check_lists(wd, lines)


def test_users_file_selects_and_orders(tmp_path):
    wd = str(tmp_path)
    write_inputs(wd)
    fit(wd, "als")
    open(os.path.join(wd, "who"), "w").write("8\n4\n")
    p = run(wd, os.path.join(BIN, "recommend"), "--factors", "out/p", "--topn", "2", "--output", "out/r", "--nshards", "1",
            "--users", "who")
    assert p.returncode == 0, p.stdout + p.stderr
    got = [ln.split("\t") for ln in pu.read_shards(wd, "out/r_")]
    assert [int(t[0]) for t in got] == [8, 8, 4, 4]   # no --matrix: nothing excluded, two items each


def test_factor_line_of_another_width_is_fatal(tmp_path):
    wd = str(tmp_path)
    write_inputs(wd)
    fit(wd, "als")
    f = sorted(x for x in os.listdir(os.path.join(wd, "out")) if x.startswith("p.V_"))[-1]
    with open(os.path.join(wd, "out", f), "a") as fh:
        fh.write("999) 0.5 0.25 \n")
    p = run(wd, os.path.join(BIN, "recommend"), "--factors", "out/p", "--matrix", "movielens/", "--topn", "3", "--output",
            "out/r")
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
    p = run(wd, os.path.join(BIN, "recommend"), "--factors", "out/p", "--matrix", "movielens/", "--topn", "3", "--output",
            "out/r")
    assert p.returncode != 0 and "item 777 of movielens/ has no line in out/p.V_*" in p.stderr
    open(train, "w").write(before)
    with open(os.path.join(wd, "movielens", "r.validate"), "a") as fh:
        fh.write("555 101 4\n")
    p = run(wd, os.path.join(BIN, "recommend"), "--factors", "out/p", "--matrix", "movielens/", "--topn", "3", "--output",
            "out/r")
    assert p.returncode != 0 and "user 555 of movielens/ has no line in out/p.U_*" in p.stderr
