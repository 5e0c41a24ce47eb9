"""The checker tests/split_ref.py against a brute-force restatement (Python dicts and sorted) on small
random graphs, its splitmix64 against the published vector, and the fixed tail case whose round
counts are known (CPU only)."""
import numpy as np
import pytest

import split_ref as sr


def test_splitmix64_is_the_cli_generator():
    # the first outputs of splitmix64 seeded with 0 (the vector of test_bpr_ref.py)
    assert sr.sm(0) == 0xE220A8397B1DCDAF
    assert sr.sm(0x9E3779B97F4A7C15) == 0x6E789E6AA1B965F4
    x = np.array([0, 0x9E3779B97F4A7C15, 12345, sr.M64], np.uint64)
    assert [int(v) for v in sr.sm_np(x)] == [sr.sm(int(v)) for v in x]


def brute(user, item, n_users, n_items, mode, a, b, key, seed, min_user, min_item, min_train):
    """(part list, stats tuple) from the definitions, one edge at a time."""
    n = len(user)
    last = {}
    for i in range(n):
        last[(int(user[i]), int(item[i]))] = i
    alive = set(last.values())
    kept = len(alive)
    rounds = 0
    while True:
        ud, md = {}, {}
        for i in alive:
            ud[int(user[i])] = ud.get(int(user[i]), 0) + 1
            md[int(item[i])] = md.get(int(item[i]), 0) + 1
        dead = {i for i in alive
                if (min_user > 1 and ud[int(user[i])] < min_user) or (min_item > 1 and md[int(item[i])] < min_item)}
        if not dead:
            break
        alive -= dead
        rounds += 1
    part = [sr.DROPPED] * n
    by_user = {}
    for i in alive:
        k = int(key[i]) if key is not None else sr.sm(sr.sm(sr.sm(seed) ^ int(user[i])) ^ int(item[i]))
        by_user.setdefault(int(user[i]), []).append((k, int(item[i]), i))
    for u, edges in by_user.items():
        n_u = len(edges)
        t = max(n_u - min_train, 0)
        for p, (_, _, i) in enumerate(sorted(edges)):
            if mode == sr.FOLDS:
                part[i] = p % a
            else:
                h = min(a if mode == sr.LEAVE_K else n_u * a // b, t)
                part[i] = 1 if p < h else 0
    items_alive = {int(item[i]) for i in alive}
    with_train = {int(item[i]) for i in alive if part[i] == 0}
    stats = (kept, len(alive), len(by_user), len(items_alive), sum(part[i] == 0 for i in alive),
             sum(part[i] == 1 for i in alive), 0 if mode == sr.FOLDS else len(items_alive - with_train), rounds)
    return part, stats


@pytest.mark.parametrize("seed", range(12))
def test_checker_equals_brute_force(seed):
    rng = np.random.default_rng(seed)
    n_users, n_items = int(rng.integers(1, 30)), int(rng.integers(1, 20))
    n = int(rng.integers(0, 260))
    user = rng.integers(0, n_users, n).astype(np.uint32)
    item = rng.integers(0, n_items, n).astype(np.uint32)   # repeats are likely
    key = rng.integers(0, 4, n).astype(np.uint64) if seed % 2 else None   # few values: ties inside a user
    min_user, min_item = int(rng.integers(0, 5)), int(rng.integers(0, 5))
    min_train = int(rng.integers(0, 4))
    for mode, a, b in ((sr.LEAVE_K, int(rng.integers(0, 4)), 0), (sr.RATIO, 1, int(rng.integers(2, 6))),
                       (sr.RATIO, 3, 4), (sr.FOLDS, int(rng.integers(2, 7)), 0)):
        part, stats = sr.holdout_split(user, item, n_users, n_items, mode, a, b, order_key=key, seed=seed,
                                       min_user=min_user, min_item=min_item, min_train=min_train)
        want, wstats = brute(user, item, n_users, n_items, mode, a, b, key, seed, min_user, min_item, min_train)
        assert part.tolist() == want
        assert tuple(stats) == wstats
        keep, rounds = sr.kcore(user, item, n_users, n_items, min_user, min_item)
        assert keep.tolist() == [p != sr.DROPPED for p in want] and rounds == wstats[7]


def test_tail_case_rounds():
    user, item, n_users, n_items = sr.tail_case()
    assert len(user) == 88
    keep, rounds = sr.kcore(user, item, n_users, n_items, 2, 2)
    assert rounds == 79 and keep.sum() == 9 and keep[:9].all()
    keep, rounds = sr.kcore(user, item, n_users, n_items, 1, 1)
    assert rounds == 0 and keep.all()
    keep, rounds = sr.kcore(user, item, n_users, n_items, 4, 1)
    assert rounds == 1 and not keep.any()
