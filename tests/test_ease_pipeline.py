"""bin/ease --recommend and --rankeval on a small movielens/ directory with a per-user hold-out (the
data of test_knn_topn_pipeline.py), against the checker ease_ref.py run on the B that api.ease_fit
gives for the same parsed edges: the binary and the API run the same fit, so B is the same bytes,
and ids, order and ranks are exact; scores agree after %g.  One case shows that recommend --factors
and rankeval --graph, whose writers moved into a shared header, still print what their own pipeline
tests expect."""
import os
import subprocess

import numpy as np
import pytest

import ease_ref as er
import pipeline_util as pu
from test_knn_topn_pipeline import read_lists
from test_knn_topn_pipeline import work as knn_work  # noqa: F401  (that module's data, as a fixture of this one)

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BIN = os.path.join(ROOT, "bin")
TOPN = 4
LAM = 2.5


def run(wd, *cmd):
    return subprocess.run([os.path.join(BIN, cmd[0]), *cmd[1:]], cwd=wd, capture_output=True, text=True, timeout=120)


def ok(wd, *cmd):
    p = run(wd, *cmd)
    assert p.returncode == 0, p.stdout + p.stderr
    return p.stdout


@pytest.fixture(scope="module")
def work(tmp_path_factory, gpu_ctx):
    """80 users x 30 items, integer ratings, every rating held out with probability 0.2; item 900
    occurs only as a VALIDATE edge of user 3 (an item without a TRAIN edge); one TRAIN pair is listed
    twice (its last value stays)."""
    wd = str(tmp_path_factory.mktemp("ease"))
    rng = np.random.default_rng(12)
    ml = os.path.join(wd, "movielens")
    os.makedirs(ml)
    os.makedirs(os.path.join(wd, "out"))
    train, val = [], []
    for u in range(1, 81):
        for m in rng.choice(30, size=int(rng.integers(8, 16)), replace=False) + 200:
            (val if rng.random() < 0.2 else train).append((u, int(m), int(rng.integers(1, 6))))
    val.append((3, 900, 4))
    rng.shuffle(train)   # the binary orders a profile by item id itself
    u0, m0, r0 = train[0]
    lines = train + [(u0, m0, r0 % 5 + 1)]   # the same pair again with another rating
    open(os.path.join(ml, "u0.train"), "w").writelines(f"{u}\t{m}\t{r}\n" for u, m, r in lines)
    open(os.path.join(ml, "u0.validate"), "w").writelines(f"{u}\t{m}\t{r}\n" for u, m, r in val)
    train[0] = (u0, m0, r0 % 5 + 1)
    uids = sorted({u for u, _, _ in train + val})
    mids = sorted({m for _, m, _ in train + val})
    urow, mrow = {u: k for k, u in enumerate(uids)}, {m: k for k, m in enumerate(mids)}
    prof = sorted((urow[u], mrow[m], r) for u, m, r in train)
    off = np.zeros(len(uids) + 1, np.uint64)
    off[1:] = np.cumsum(np.bincount([p[0] for p in prof], minlength=len(uids)))
    items = np.array([p[1] for p in prof], np.uint32)
    ratings = np.array([p[2] for p in prof], np.float32)
    B = {}
    for binary in (False, True):
        gpu_ctx.ease_fit(off, items, ratings, len(mids), LAM, binary=binary)
        B[binary] = gpu_ctx.ease_weights()
    assert not B[False][mrow[900]].any() and not np.array_equal(B[False], B[True])
    pairs = lambda es: (np.array([urow[u] for u, _, _ in es]), np.array([mrow[m] for _, m, _ in es]))   # noqa: E731
    return dict(wd=wd, train=train, val=val, uids=uids, mids=mids, B=B, off=off, items=items, ratings=ratings,
                excl_all=pairs(train + val), excl_train=pairs(train), held=pairs(val))


@pytest.mark.parametrize("binary", [False, True])
def test_recommend(work, binary):
    wd = work["wd"]
    out = ok(wd, "ease", "--matrix", "movielens/", "--lambda", str(LAM), "--recommend", "out/r", "--topn", str(TOPN),
             *(("--binary",) if binary else ()))
    fit = next(ln for ln in out.split("\n") if ln.startswith("EASE fit: "))
    assert f"users: {len(work['uids'])} items: {len(work['mids'])} nnz: {len(work['train'])} " in fit
    assert "gram:" in fit and "invert:" in fit and "normalise:" in fit and "scoring kernels:" in out
    items, scores, count, n_nan = er.topn(work["B"][binary], work["off"], work["items"], work["ratings"], TOPN,
                                          binary=binary, exclude=work["excl_all"])
    assert n_nan == 0 and (count == TOPN).all()
    want = {u: [(work["mids"][int(items[k, r])], float("%g" % scores[k, r])) for r in range(TOPN)]
            for k, u in enumerate(work["uids"])}
    got = {u: [(int(m), float(sc)) for m, sc in lst] for u, lst in read_lists(wd, "r").items()}
    assert got == want
    assert len({lst[0] for lst in got.values()}) > 3   # the lists depend on the profile
    for f in os.listdir(os.path.join(wd, "out")):
        os.remove(os.path.join(wd, "out", f))


def test_recommend_users_file(work):
    wd = work["wd"]
    open(os.path.join(wd, "who"), "w").write("8\n4\n")
    ok(wd, "ease", "--matrix", "movielens/", "--lambda", str(LAM), "--recommend", "out/w", "--topn", "2", "--nshards", "1",
       "--users", "who")
    got = [(int(a), int(b), float(c)) for a, b, c in (ln.split("\t") for ln in pu.read_shards(wd, "out/w_"))]
    items, scores, count, _ = er.topn(work["B"][False], work["off"], work["items"], work["ratings"], 2,
                                      exclude=work["excl_all"], users=[work["uids"].index(8), work["uids"].index(4)])
    assert got == [(u, work["mids"][int(items[j, r])], float("%g" % scores[j, r])) for j, u in enumerate((8, 4))
                   for r in range(2)]


def test_rankeval(work):
    wd = work["wd"]
    out = ok(wd, "ease", "--matrix", "movielens/", "--lambda", str(LAM), "--rankeval", "--cutoff", str(TOPN), "--output",
             "out/e", "--weighted")
    weights = np.array([float(r) for _, _, r in work["val"]])
    rank, n_cand, users, s = er.evaluate(work["B"][False], work["off"], work["items"], work["ratings"], TOPN,
                                         (work["held"][0], work["held"][1], weights), exclude=work["excl_train"])
    want = {}
    for k, (u, m, _) in enumerate(work["val"]):
        want.setdefault(u, []).append((m, str(m), str(-1 if rank[k] == er.rr.MAX else int(rank[k])), str(int(n_cand[k]))))
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


def test_flags_are_checked(work):
    wd = work["wd"]
    p = run(wd, "ease", "--matrix", "movielens/")
    assert p.returncode != 0 and "usage:" in p.stderr
    p = run(wd, "ease", "--matrix", "movielens/", "--lambda", "0")
    assert p.returncode != 0 and "--lambda" in p.stderr
    p = run(wd, "ease", "--matrix", "movielens/", "--lambda", "1", "--recommend", "out/x")
    assert p.returncode != 0 and "usage:" in p.stderr
    p = run(wd, "ease", "--matrix", "movielens/", "--lambda", "1", "--recommend", "out/x", "--topn", "0")
    assert p.returncode != 0 and "--topn" in p.stderr
    assert not any(f.startswith("x_") for f in os.listdir(os.path.join(wd, "out")))


def test_recommend_factors_and_rankeval_graph_are_unchanged(tmp_path, knn_work):
    """The recipe and the checks of test_topn_pipeline.py on one fit, and test_knn_topn_pipeline.py's
    rankeval --graph case on its own data (its fixture, imported above as knn_work)."""
    import test_knn_topn_pipeline as tkp
    import test_topn_pipeline as ttp

    wd = str(tmp_path)
    lines = ttp.write_inputs(wd)
    ttp.fit(wd, "als")
    p = ttp.run(wd, os.path.join(BIN, "recommend"), "--factors", "out/p", "--matrix", "movielens/", "--topn", str(ttp.TOPN),
                "--output", "out/r")
    assert p.returncode == 0, p.stdout + p.stderr
    assert "Users: 40 items: 15 D: 5" in p.stdout and "scoring kernels:" in p.stdout
    ttp.check_lists(wd, lines)
    tkp.test_rankeval_from_the_graph(knn_work)
