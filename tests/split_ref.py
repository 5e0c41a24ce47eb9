"""Checker for cf_kcore / cf_holdout_split: numpy integers, written from the contract in
include/cf_abi.h (not from the kernels).

1. duplicates: of the edges with one (user, item) the last one read stays.
2. k-core in synchronous rounds: degrees over the edges alive after the previous round; users below
   min_user and items below min_item die (0 or 1: no limit), and every edge with a dead end; stop at
   the first round in which no edge dies; rounds = the rounds in which one did.
3. a user's n_u alive edges ordered by (order_key, item); without keys the key is
   sm(sm(sm(seed) ^ user) ^ item), sm = splitmix64.
4. p = the position in that order, t = max(n_u - min_train, 0):
   LEAVE_K h = min(K, t); RATIO h = min(n_u num // den, t); part = 1 if p < h else 0; FOLDS part = p mod F.
   Dropped and dead edges: 255.
stats: kept, alive, users alive, items alive, part 0, part 1, alive items without a part-0 edge
(0 for folds), rounds."""
from __future__ import annotations

from collections import namedtuple

import numpy as np

LEAVE_K, RATIO, FOLDS = 0, 1, 2
DROPPED = 255
M64 = (1 << 64) - 1
STAT_NAMES = ("kept", "alive", "users_alive", "items_alive", "train", "validate", "items_without_train", "rounds")
Stats = namedtuple("Stats", STAT_NAMES)


def sm(x: int) -> int:
    x = (x + 0x9E3779B97F4A7C15) & M64
    x = ((x ^ (x >> 30)) * 0xBF58476D1CE4E5B9) & M64
    x = ((x ^ (x >> 27)) * 0x94D049BB133111EB) & M64
    return x ^ (x >> 31)


def sm_np(x):
    """sm over a uint64 array (array arithmetic wraps modulo 2^64)."""
    x = np.asarray(x, np.uint64) + np.uint64(0x9E3779B97F4A7C15)
    x = (x ^ (x >> np.uint64(30))) * np.uint64(0xBF58476D1CE4E5B9)
    x = (x ^ (x >> np.uint64(27))) * np.uint64(0x94D049BB133111EB)
    return x ^ (x >> np.uint64(31))


def random_keys(user, item, seed):
    user, item = np.asarray(user, np.uint64), np.asarray(item, np.uint64)
    return sm_np(sm_np(np.uint64(sm(int(seed))) ^ user) ^ item)


def last_of_pairs(user, item):
    """bool[n]: the last edge read of every (user, item)."""
    user, item = np.asarray(user, np.uint64), np.asarray(item, np.uint64)
    kept = np.zeros(len(user), bool)
    if len(user):
        key = user << np.uint64(32) | item
        order = np.argsort(key, kind="stable")
        ks = key[order]
        kept[order[np.concatenate((ks[1:] != ks[:-1], [True]))]] = True
    return kept


def kcore(user, item, n_users, n_items, min_user, min_item):
    """(keep bool[n], rounds)."""
    user, item = np.asarray(user, np.int64), np.asarray(item, np.int64)
    alive = last_of_pairs(user, item)
    lim_u = min_user if min_user > 1 else 0
    lim_i = min_item if min_item > 1 else 0
    rounds = 0
    while True:
        udeg = np.bincount(user[alive], minlength=n_users)
        ideg = np.bincount(item[alive], minlength=n_items)
        dies = alive & ((udeg[user] < lim_u) | (ideg[item] < lim_i))
        if not dies.any():
            return alive, rounds
        alive = alive & ~dies
        rounds += 1


def holdout_split(user, item, n_users, n_items, mode, a, b=0, *, order_key=None, seed=0, min_user=0, min_item=0,
                  min_train=0):
    """(part uint8[n] in read order, Stats)."""
    user, item = np.asarray(user, np.int64), np.asarray(item, np.int64)
    if mode == RATIO:
        assert 0 < a < b
    elif mode == FOLDS:
        assert 2 <= a <= 254
    else:
        assert mode == LEAVE_K
    kept = last_of_pairs(user, item)
    alive, rounds = kcore(user, item, n_users, n_items, min_user, min_item)
    key = random_keys(user, item, seed) if order_key is None else np.asarray(order_key, np.uint64)
    idx = np.flatnonzero(alive)
    order = idx[np.lexsort((item[idx], key[idx], user[idx]))]   # by user, then key, then item
    uu = user[order]
    n_u = np.bincount(uu, minlength=n_users).astype(np.int64)
    start = np.concatenate(([0], np.cumsum(n_u)))[:-1]
    p = np.arange(len(order), dtype=np.int64) - start[uu]
    if mode == FOLDS:
        pt = p % a
    else:
        t = np.maximum(n_u - min_train, 0)
        want = np.full(n_users, a, np.int64) if mode == LEAVE_K else (n_u.astype(np.uint64) * np.uint64(a) // np.uint64(b)).astype(np.int64)
        h = np.minimum(want, t)
        pt = (p < h[uu]).astype(np.int64)
    part = np.full(len(user), DROPPED, np.uint8)
    part[order] = pt.astype(np.uint8)
    items_alive = np.unique(item[order])
    no_train = 0 if mode == FOLDS else len(np.setdiff1d(items_alive, item[order][pt == 0]))
    stats = Stats(int(kept.sum()), len(order), int((n_u > 0).sum()), len(items_alive), int((pt == 0).sum()),
                  int((pt == 1).sum()), no_train, rounds)
    return part, stats


def tail_case():
    """K3,3 on users and items 0..2 plus a tail of 40 users hanging off item 2: user 3 + t rates items
    2 + t and 3 + t, the last user only its first.  88 edges; at 2/2 the tail unravels one edge per
    round."""
    user = [u for u in range(3) for _ in range(3)]
    item = [m for _ in range(3) for m in range(3)]
    for t in range(40):
        user += [3 + t] * (2 if t < 39 else 1)
        item += [2 + t, 3 + t][: 2 if t < 39 else 1]
    return np.array(user, np.uint32), np.array(item, np.uint32), 43, 42
