"""bin/knn -> bin/knn2 -> bin/recommend --graph out_fin_ and bin/rankeval --graph out_fin_ on a small
movielens/ directory with a per-user hold-out (pipeline_util.write_movielens splits users
disjointly, which would leave every held-out user without a profile), against the checker
knn_topn_ref.py run on the parsed out_fin_* text.  Both sides parse the same float32 weights, so
ids, order and ranks are exact and scores agree after %g.  One case shows that the --factors path
of both binaries still gives what its own pipeline tests expect."""
import os
import subprocess

import numpy as np
import pytest

import knn_topn_ref as kr
import pipeline_util as pu

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BIN = os.path.join(ROOT, "bin")
TOPN = 4


def run(wd, *cmd):
    return subprocess.run([os.path.join(BIN, cmd[0]), *cmd[1:]], cwd=wd, capture_output=True, text=True, timeout=120)


def ok(wd, *cmd):
    p = run(wd, *cmd)
    assert p.returncode == 0, p.stdout + p.stderr
    return p.stdout


@pytest.fixture(scope="module")
def work(tmp_path_factory):
    """80 users x 30 items, integer ratings, every rating held out with probability 0.2; item 900
    occurs only as a VALIDATE edge of user 3 (an item of DIR that is not in the graph)."""
    if not __import__("torch").cuda.is_available():
        pytest.skip("no GPU visible")
    wd = str(tmp_path_factory.mktemp("knn_topn"))
    rng = np.random.default_rng(12)
    ml = os.path.join(wd, "movielens")
    os.makedirs(ml)
    os.makedirs(os.path.join(wd, "out"))
    train, val = [], []
    for u in range(1, 81):
        for m in rng.choice(30, size=int(rng.integers(8, 16)), replace=False) + 200:
            (val if rng.random() < 0.2 else train).append((u, int(m), int(rng.integers(1, 6))))
    val.append((3, 900, 4))
    rng.shuffle(train)   # the binaries order a profile by item id themselves
    open(os.path.join(ml, "u0.train"), "w").writelines(f"{u}\t{m}\t{r}\n" for u, m, r in train)
    open(os.path.join(ml, "u0.validate"), "w").writelines(f"{u}\t{m}\t{r}\n" for u, m, r in val)
    ok(wd, "knn")
    ok(wd, "knn2")
    fin = pu.parse_edges(pu.read_shards(wd, "out_fin_"))
    assert len(fin) > 100
    uids = sorted({u for u, _, _ in train + val})
    mids = sorted({m for _, m, _ in train + val} | {a for a, _ in fin} | {b for _, b in fin})
    urow, mrow = {u: k for k, u in enumerate(uids)}, {m: k for k, m in enumerate(mids)}
    W = np.zeros((len(mids), len(mids)), np.float32)
    for (a, b), w in fin.items():
        W[mrow[a], mrow[b]] = np.float32(w)
    assert (W.astype(np.float64) > 0.1).sum() > 50   # knn2's cosine is symmetric; test_gpu_knn_topn.py has the directed graphs
    prof = sorted((urow[u], mrow[m], r) for u, m, r in train)
    off = np.zeros(len(uids) + 1, np.uint64)
    off[1:] = np.cumsum(np.bincount([p[0] for p in prof], minlength=len(uids)))
    items = np.array([p[1] for p in prof], np.uint32)
    ratings = np.array([p[2] for p in prof], np.float32)
    pairs = lambda es: (np.array([urow[u] for u, _, _ in es]), np.array([mrow[m] for _, m, _ in es]))   # noqa: E731
    return dict(wd=wd, train=train, val=val, uids=uids, mids=mids, W=W, off=off, items=items, ratings=ratings,
                excl_all=pairs(train + val), excl_train=pairs(train), held=pairs(val))


def read_lists(wd, prefix, nshards=4):
    got = {}
    for f in sorted(os.listdir(os.path.join(wd, "out"))):
        if not f.startswith(prefix + "_"):
            continue
        shard = int(f.split("_")[1])
        assert f.endswith(f"_of_{nshards}")
        for ln in open(os.path.join(wd, "out", f)).read().split("\n"):
            if ln:
                t = ln.split("\t")
                assert int(t[0]) % nshards + 1 == shard
                got.setdefault(int(t[0]), []).append(tuple(t[1:]))   # file order
    return got


@pytest.mark.parametrize("flags,mode,w_min", [((), "sum", 0.1), (("--score", "mean", "--wmin", "0.2"), "mean", 0.2)])
def test_recommend_from_the_graph(work, flags, mode, w_min):
    wd = work["wd"]
    out = ok(wd, "recommend", "--graph", "out_fin_", "--matrix", "movielens/", "--topn", str(TOPN), "--output", "out/k", *flags)
    assert f"Users: {len(work['uids'])} items: {len(work['mids'])}\n" in out and "scoring kernels:" in out
    items, scores, count, n_nan = kr.topn(work["W"], work["off"], work["items"], work["ratings"], TOPN, mode=mode,
                                          w_min=w_min, exclude=work["excl_all"])
    assert n_nan == 0 and (count == TOPN).all()
    want = {u: [(work["mids"][int(items[k, r])], float("%g" % scores[k, r])) for r in range(TOPN)]
            for k, u in enumerate(work["uids"])}
    got = {u: [(int(m), float(sc)) for m, sc in lst] for u, lst in read_lists(wd, "k").items()}
    assert got == want
    assert len({lst[0] for lst in got.values()}) > 3   # the lists depend on the profile


def test_recommend_users_file_with_the_graph(work):
    wd = work["wd"]
    open(os.path.join(wd, "who"), "w").write("8\n4\n")
    ok(wd, "recommend", "--graph", "out_fin_", "--matrix", "movielens/", "--topn", "2", "--output", "out/w", "--nshards", "1",
       "--users", "who")
    got = [(int(a), int(b), float(c)) for a, b, c in (ln.split("\t") for ln in pu.read_shards(wd, "out/w_"))]
    items, scores, count, _ = kr.topn(work["W"], work["off"], work["items"], work["ratings"], 2, exclude=work["excl_all"],
                                      users=[work["uids"].index(8), work["uids"].index(4)])
    assert got == [(u, work["mids"][int(items[j, r])], float("%g" % scores[j, r])) for j, u in enumerate((8, 4))
                   for r in range(2)]


def test_rankeval_from_the_graph(work):
    wd = work["wd"]
    out = ok(wd, "rankeval", "--graph", "out_fin_", "--matrix", "movielens/", "--topn", str(TOPN), "--output", "out/e",
             "--weighted")
    weights = np.array([float(r) for _, _, r in work["val"]])
    rank, n_cand, users, s = kr.evaluate(work["W"], work["off"], work["items"], work["ratings"], TOPN,
                                         (work["held"][0], work["held"][1], weights), exclude=work["excl_train"])
    want = {}
    for k, (u, m, _) in enumerate(work["val"]):
        want.setdefault(u, []).append((m, str(m), str(-1 if rank[k] == kr.rr.MAX else int(rank[k])), str(int(n_cand[k]))))
    want = {u: [t[1:] for t in sorted(v)] for u, v in want.items()}   # by user, then item
    assert read_lists(wd, "e") == want
    ls = out.split("\n")
    b = next(ln for ln in ls if ln.startswith("Evaluated users: ")).split()
    assert (int(b[2]), int(b[5]), int(b[7])) == (s["users_evaluated"], len(work["val"]), s["edges_skipped"])
    assert s["edges_skipped"] == 0 and s["users_evaluated"] > 40
    c = next(ln for ln in ls if ln.startswith("precision@N ")).split()
    printed = {c[k]: float(c[k + 1]) for k in range(0, len(c), 2)}
    for name, key in (("precision@N", "precision"), ("recall@N", "recall"), ("ndcg@N", "ndcg"), ("map@N", "map"),
                      ("mrr", "mrr"), ("auc", "auc"), ("mpr", "mpr")):
        assert printed[name] == float("%g" % s[key]), (name, printed[name], s[key])
    assert s["precision"] > 0.0   # a graph fitted on the profiles ranks held-out items above chance somewhere


def test_source_flags_are_checked(work):
    wd = work["wd"]
    base = ("--matrix", "movielens/", "--topn", "3", "--output", "out/x")
    for tool in ("recommend", "rankeval"):
        p = run(wd, tool, *base)
        assert p.returncode != 0 and "usage:" in p.stderr and "--graph" in p.stderr
        p = run(wd, tool, "--graph", "out_fin_", "--factors", "out/p", *base)
        assert p.returncode != 0 and "usage:" in p.stderr
        p = run(wd, tool, "--graph", "out_fin_", "--bias", *base)
        assert p.returncode != 0 and "--bias and --mean belong to --factors" in p.stderr
        p = run(wd, tool, "--graph", "out_fin_", "--mean", "3", *base)
        assert p.returncode != 0 and "--bias and --mean belong to --factors" in p.stderr
        p = run(wd, tool, "--graph", "out_fin_", "--score", "median", *base)
        assert p.returncode != 0 and "--score must be sum or mean" in p.stderr
        p = run(wd, tool, "--graph", "out_fin_", "--wmin", "-1", *base)
        assert p.returncode != 0 and "--wmin" in p.stderr
        p = run(wd, tool, "--graph", "no_such_", *base)
        assert p.returncode != 0 and "no edge in no_such_*" in p.stderr
    p = run(wd, "recommend", "--graph", "out_fin_", "--topn", "3", "--output", "out/x")
    assert p.returncode != 0 and "--graph needs --matrix" in p.stderr
    assert not any(f.startswith("x_") for f in os.listdir(os.path.join(wd, "out")))


def test_factors_path_is_unchanged(tmp_path):
    """The recipe and the checks of test_topn_pipeline.py and test_rank_pipeline.py on one fit."""
    import test_rank_pipeline as trp
    import test_topn_pipeline as ttp

    wd = str(tmp_path)
    lines = ttp.write_inputs(wd)
    ttp.fit(wd, "als")
    p = ttp.run(wd, os.path.join(BIN, "recommend"), "--factors", "out/p", "--matrix", "movielens/", "--topn", str(ttp.TOPN),
                "--output", "out/r")
    assert p.returncode == 0, p.stdout + p.stderr
    assert "Users: 40 items: 15 D: 5" in p.stdout
    ttp.check_lists(wd, lines)
    for f in os.listdir(os.path.join(wd, "out")):
        if f.startswith("r_"):
            os.remove(os.path.join(wd, "out", f))
    p = trp.rankeval(wd, "--output", "out/r")
    assert p.returncode == 0, p.stdout + p.stderr
    assert "Users: 40 items: 15 D: 5" in p.stdout
    want, s, _ = trp.checker(wd, lines, False)
    trp.check_rows(wd, want)
    _, _, printed = trp.summary_of(p.stdout)
    assert printed["ndcg@N"] == float("%g" % s["ndcg"])
