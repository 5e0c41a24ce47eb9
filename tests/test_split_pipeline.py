"""bin/split on a small four-column rating file (120 users x 40 items, a few repeated pairs, shuffled):
the files it writes equal what the checker tests/split_ref.py gives for the parsed edges, a permuted
input gives the same lines, --by time holds out the latest edges, --folds partitions the alive
edges, and bin/ease --rankeval reads the hold-out directory and evaluates as many held-out edges
as split reports."""
import os
import subprocess

import numpy as np
import pytest

import split_ref as sr

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BIN = os.path.join(ROOT, "bin")
CORE = ("--kcore-user", "5", "--kcore-item", "3")
HOLD = ("--holdout", "2", "--min-train", "3") + CORE


def run(wd, *cmd):
    return subprocess.run([os.path.join(BIN, cmd[0]), *cmd[1:]], cwd=wd, capture_output=True, text=True, timeout=120)


def ok(wd, *cmd):
    p = run(wd, *cmd)
    assert p.returncode == 0, p.stdout + p.stderr
    return p.stdout


def summary(out):
    w = next(ln for ln in out.split("\n") if ln.startswith("split: ")).split()
    return {w[k]: int(w[k + 1]) for k in range(1, len(w), 2)}


def read(wd, *path):
    return open(os.path.join(wd, *path)).read().splitlines()


@pytest.fixture(scope="module")
def work(tmp_path_factory):
    """Lines (user, item, rating, time): users 10 + 3 k, items 200 + 2 m (ids with gaps, so compaction
    matters), 2 .. 14 items per user, times with many ties; four pairs are listed again later with
    another rating and time.  `lines` is the shuffled read order."""
    wd = str(tmp_path_factory.mktemp("split"))
    rng = np.random.default_rng(21)
    lines = []
    for k in range(120):
        for m in rng.choice(40, size=int(rng.integers(2, 15)), replace=False):
            lines.append((10 + 3 * k, 200 + 2 * int(m), int(rng.integers(1, 6)), 1000 + int(rng.integers(0, 25))))
    rng.shuffle(lines)
    lines = [tuple(int(x) for x in ln) for ln in lines]
    for j in (3, 50, 51, 400):
        u, m, r, t = lines[j]
        lines.append((u, m, r % 5 + 1, t + 7))
    seps = ("\t", " ", "  ", "\t")   # tabs or blanks
    open(os.path.join(wd, "data"), "w").writelines(
        seps[i % 4].join(str(x) for x in ln) + ("\r\n" if i % 9 == 0 else "\n") for i, ln in enumerate(lines))
    return dict(wd=wd, lines=lines)


def parsed(lines):
    uids = sorted({ln[0] for ln in lines})
    mids = sorted({ln[1] for ln in lines})
    user = np.array([uids.index(ln[0]) for ln in lines], np.uint32)
    item = np.array([mids.index(ln[1]) for ln in lines], np.uint32)
    return user, item, len(uids), len(mids)


def expected_files(lines, part, held=1):
    text = [f"{u}\t{m}\t{r}" for u, m, r, _ in lines]
    return ([t for t, p in zip(text, part) if p != sr.DROPPED and p != held], [t for t, p in zip(text, part) if p == held])


def test_holdout_files_equal_the_checker(work):
    wd, lines = work["wd"], work["lines"]
    out = ok(wd, "split", "data", "--out", "h", *HOLD, "--seed", "4")
    user, item, n_users, n_items = parsed(lines)
    part, stats = sr.holdout_split(user, item, n_users, n_items, sr.LEAVE_K, 2, seed=4, min_user=5, min_item=3, min_train=3)
    train, validate = expected_files(lines, part)
    assert read(wd, "h", "u0.train") == train and read(wd, "h", "u0.validate") == validate
    s = summary(out)
    assert s["lines"] == s["read"] == len(lines) and s["kept"] == len(lines) - 4
    assert [s[k] for k in ("kept", "alive", "users", "items", "train", "validate", "items_without_train", "rounds")] == list(stats)
    assert 0 < stats.alive < stats.kept and stats.validate > 100 and stats.users_alive < 120
    # the files are not overwritten
    p = run(wd, "split", "data", "--out", "h", *HOLD, "--seed", "4")
    assert p.returncode != 0 and "exists and is not empty" in p.stderr
    assert read(wd, "h", "u0.train") == train


def test_permuted_lines_give_the_same_files(work):
    """Another line order (the lines of a repeated pair keep their order among themselves, which is what
    decides between them): the sorted output is byte-identical."""
    wd, lines = work["wd"], work["lines"]
    rng = np.random.default_rng(22)
    order = rng.permutation(len(lines)).tolist()
    where = {}
    for pos, i in enumerate(order):
        where.setdefault(lines[i][:2], []).append(pos)
    for slots in where.values():
        for pos, i in zip(sorted(slots), sorted(order[p] for p in slots)):
            order[pos] = i
    assert sorted(order) == list(range(len(lines))) and order != list(range(len(lines)))
    open(os.path.join(wd, "data_perm"), "w").writelines("\t".join(str(x) for x in lines[i]) + "\n" for i in order)
    ok(wd, "split", "data", "--out", "p0", *HOLD, "--seed", "4")
    ok(wd, "split", "data_perm", "--out", "p1", *HOLD, "--seed", "4")
    for f in ("u0.train", "u0.validate"):
        a, b = read(wd, "p0", f), read(wd, "p1", f)
        assert a != b and sorted(a) == sorted(b)
        assert "\n".join(sorted(a)).encode() == "\n".join(sorted(b)).encode()
    ok(wd, "split", "data", "--out", "p2", *HOLD, "--seed", "5")
    assert sorted(read(wd, "p2", "u0.validate")) != sorted(read(wd, "p0", "u0.validate"))
    assert sorted(read(wd, "p2", "u0.train") + read(wd, "p2", "u0.validate")) == sorted(
        read(wd, "p0", "u0.train") + read(wd, "p0", "u0.validate"))


def test_by_time_holds_out_the_two_latest(work):
    wd, lines = work["wd"], work["lines"]
    ok(wd, "split", "data", "--out", "t", *HOLD, "--by", "time")
    user, item, n_users, n_items = parsed(lines)
    key = np.array([2**64 - 1 - ln[3] for ln in lines], np.uint64)
    part, _ = sr.holdout_split(user, item, n_users, n_items, sr.LEAVE_K, 2, order_key=key, min_user=5, min_item=3,
                               min_train=3)
    train, validate = expected_files(lines, part)
    assert read(wd, "t", "u0.train") == train and read(wd, "t", "u0.validate") == validate
    # and from the definition: per alive user the two largest times, ties to the smaller item
    alive = {}
    for ln, p in zip(lines, part):
        if p != sr.DROPPED:
            alive.setdefault(ln[0], []).append(ln)
    want = set()
    for u, es in alive.items():
        assert len(es) >= 5
        want |= {f"{u}\t{m}\t{r}" for _, m, r, _ in sorted(es, key=lambda e: (-e[3], e[1]))[:2]}
    assert set(validate) == want and len(validate) == len(want)
    p = run(wd, "split", "data", "--out", "t2", *HOLD, "--by", "time", "--min-rating", "x")
    assert p.returncode != 0
    three = os.path.join(wd, "three")
    open(three, "w").write("1 2 3\n")
    p = run(wd, "split", "three", "--out", "t3", "--holdout", "1", "--by", "time")
    assert p.returncode != 0 and "fourth field" in p.stderr


def test_folds_partition_the_alive_edges(work):
    wd, lines = work["wd"], work["lines"]
    out = ok(wd, "split", "data", "--out", "f", "--folds", "3", *CORE, "--seed", "2", "--name", "ml")
    user, item, n_users, n_items = parsed(lines)
    part, stats = sr.holdout_split(user, item, n_users, n_items, sr.FOLDS, 3, seed=2, min_user=5, min_item=3)
    assert sorted(os.listdir(os.path.join(wd, "f"))) == ["fold0", "fold1", "fold2"]
    every = []
    for f in range(3):
        train, validate = expected_files(lines, part, held=f)
        assert read(wd, "f", f"fold{f}", "ml.train") == train and read(wd, "f", f"fold{f}", "ml.validate") == validate
        assert sorted(os.listdir(os.path.join(wd, "f", f"fold{f}"))) == ["ml.train", "ml.validate"]
        every += validate
    alive = [f"{u}\t{m}\t{r}" for (u, m, r, _), p in zip(lines, part) if p != sr.DROPPED]
    assert sorted(every) == sorted(alive) and len(set(every)) == len(every) == stats.alive
    assert summary(out)["alive"] == stats.alive


def test_min_rating_drops_lines_first(work):
    wd, lines = work["wd"], work["lines"]
    out = ok(wd, "split", "data", "--out", "m", "--ratio", "1/4", "--min-rating", "3", "--seed", "1")
    left = [ln for ln in lines if ln[2] >= 3]
    user, item, n_users, n_items = parsed(left)
    part, stats = sr.holdout_split(user, item, n_users, n_items, sr.RATIO, 1, 4, seed=1)
    train, validate = expected_files(left, part)
    assert read(wd, "m", "u0.train") == train and read(wd, "m", "u0.validate") == validate
    s = summary(out)
    assert s["lines"] == len(lines) and s["read"] == len(left) and s["validate"] == stats.validate
    for bad in (("--ratio", "4/4"), ("--ratio", "3"), ("--folds", "1"), ("--holdout", "2", "--folds", "3"), ()):
        p = run(wd, "split", "data", "--out", "bad", *bad)
        assert p.returncode != 0, bad
    assert not os.path.exists(os.path.join(wd, "bad"))


def test_ease_rankeval_reads_the_split(work):
    wd = work["wd"]
    s = summary(ok(wd, "split", "data", "--out", "e", *HOLD, "--seed", "4"))
    out = ok(wd, "ease", "--matrix", "e/", "--lambda", "2.5", "--rankeval", "--cutoff", "5")
    b = next(ln for ln in out.split("\n") if ln.startswith("Evaluated users: ")).split()
    assert int(b[5]) == s["validate"] > 100 and int(b[2]) == s["users"]
    fit = next(ln for ln in out.split("\n") if ln.startswith("EASE fit: "))
    assert f"users: {s['users']} items: {s['items']} nnz: {s['train']} " in fit
