"""cf_kcore / cf_holdout_split (csrc/cf_split.hip) against the numpy checker tests/split_ref.py: every
comparison is integer equality.  The cases sit where the kernels branch: the list length at which
the degree count changes kernels (kLongList = 2048), more long lists than one pass of its grid (64),
more lists than the wave-per-list grid covers in one pass (65536 workgroups of four waves), more
vertices than one pass of the stats kernel (256 workgroups), the key widths of bits_for, and the
boundaries of the hold-out rules."""
import ctypes

import numpy as np
import pytest

import split_ref as sr
from collaborative_filtering_amd import _native
from collaborative_filtering_amd._native import CF_EINVAL, CF_ERANGE, CF_OK, ptr

pytestmark = pytest.mark.gpu

LONG = 2048          # kLongList of cf_split.hip
LIST_GRID = 65536 * 4   # lists one pass of degree_kernel's capped grid covers
STATS = sr.STAT_NAMES


def api_mode(mode, a, b):
    return {sr.LEAVE_K: dict(holdout=a), sr.RATIO: dict(ratio=(a, b)), sr.FOLDS: dict(folds=a)}[mode]


def check_split(ctx, user, item, n_users, n_items, mode, a, b=0, **kw):
    """The device split equals the checker's: parts and all eight stats.  Returns (result, reference stats)."""
    want, wstats = sr.holdout_split(user, item, n_users, n_items, mode, a, b, **kw)
    got = ctx.holdout_split(n_users, n_items, user, item, **api_mode(mode, a, b), **kw)
    assert got.part.dtype == np.uint8 and np.array_equal(got.part, want)
    assert tuple(getattr(got, f) for f in STATS) == tuple(wstats)
    return got, wstats


def check_core(ctx, user, item, n_users, n_items, min_user, min_item):
    want, wrounds = sr.kcore(user, item, n_users, n_items, min_user, min_item)
    keep, rounds = ctx.kcore(n_users, n_items, user, item, min_user, min_item)
    assert np.array_equal(keep, want) and rounds == wrounds
    return keep, rounds


def edges_of(degrees, n_items, rng):
    """A user of every listed degree, items drawn without repeats; shuffled read order."""
    user, item = [], []
    for u, d in enumerate(degrees):
        user += [u] * d
        item += rng.choice(n_items, size=d, replace=False).tolist()
    p = rng.permutation(len(user))
    return np.array(user, np.uint32)[p], np.array(item, np.uint32)[p]


# ---- k-core --------------------------------------------------------------------------------------
def test_kcore_tail_unravels_one_edge_per_round(gpu_ctx):
    user, item, n_users, n_items = sr.tail_case()
    keep, rounds = check_core(gpu_ctx, user, item, n_users, n_items, 2, 2)
    assert rounds == 79 and keep.sum() == 9 and keep[:9].all()
    keep, rounds = check_core(gpu_ctx, user, item, n_users, n_items, 1, 1)
    assert rounds == 0 and keep.all()
    keep, rounds = check_core(gpu_ctx, user, item, n_users, n_items, 4, 1)
    assert rounds == 1 and not keep.any()
    res, _ = check_split(gpu_ctx, user, item, n_users, n_items, sr.LEAVE_K, 1, min_user=2, min_item=2)
    assert (res.rounds, res.alive, res.users_alive, res.items_alive, res.validate) == (79, 9, 3, 3, 3)


def test_kcore_random_graph(gpu_ctx):
    rng = np.random.default_rng(6)
    n_users, n_items, n = 300, 120, 2000
    user = rng.integers(0, n_users, n).astype(np.uint32)
    item = (rng.random(n) ** 2 * n_items).astype(np.uint32)   # skewed: some items below 5, repeats of pairs
    keep, rounds = check_core(gpu_ctx, user, item, n_users, n_items, 5, 5)
    assert rounds >= 2 and 0 < keep.sum() < sr.last_of_pairs(user, item).sum()
    check_split(gpu_ctx, user, item, n_users, n_items, sr.RATIO, 1, 4, min_user=5, min_item=5, min_train=2, seed=9)


def test_kcore_one_item_rated_by_200000_users(gpu_ctx):
    """degree_long_kernel on one list of 200,000 entries (3 full passes of its 64 workgroups and a
    partial one); the hot item's count decides who lives.  Users 0 .. 299 also rate small items."""
    rng = np.random.default_rng(6)
    n_users, n_items = 200_000, 8
    user = np.arange(n_users, dtype=np.uint32)
    item = np.zeros(n_users, np.uint32)
    extra_u = np.repeat(np.arange(300, dtype=np.uint32), 2)
    extra_i = np.tile(np.array([1, 2], np.uint32), 300) + np.repeat((np.arange(300) % 3 * 2).astype(np.uint32), 2)
    user, item = np.concatenate((user, extra_u)), np.concatenate((item, extra_i))
    p = rng.permutation(len(user))
    user, item = user[p], item[p]
    keep, rounds = check_core(gpu_ctx, user, item, n_users, n_items, 2, 1)     # 199,700 users die in round 1
    assert rounds == 1 and keep.sum() == 900
    keep, rounds = check_core(gpu_ctx, user, item, n_users, n_items, 1, 301)   # the hot item alone stays
    assert rounds == 1 and keep.sum() == 200_000
    keep, rounds = check_core(gpu_ctx, user, item, n_users, n_items, 3, 301)   # 300 users, then nothing
    assert rounds == 2 and not keep.any()
    res, _ = check_split(gpu_ctx, user, item, n_users, n_items, sr.LEAVE_K, 1, min_user=0, min_item=101)
    assert res.users_alive == 200_000 and res.validate == 200_000 and res.items_alive == 1


def test_kcore_list_lengths_around_the_long_threshold(gpu_ctx):
    """Lists of exactly 2048 entries (the wave loop) and 2049 (the long kernel) on both sides, with 70
    long item lists: more than one pass of the long kernel's 64 rows."""
    users = np.arange(LONG + 1, dtype=np.uint32)
    user = np.concatenate([users] * 70 + [users[:LONG]])                           # items 0..69: 2049 raters; item 70: 2048
    item = np.concatenate([np.full(LONG + 1, m, np.uint32) for m in range(70)] + [np.full(LONG, 70, np.uint32)])
    big = 3000   # user 3000 rates 2049 items of its own, user 3001 2048
    user = np.concatenate((user, np.full(LONG + 1, big, np.uint32), np.full(LONG, big + 1, np.uint32)))
    item = np.concatenate((item, 100 + np.arange(LONG + 1, dtype=np.uint32), 3000 + np.arange(LONG, dtype=np.uint32)))
    n_users, n_items = big + 2, 3000 + LONG
    p = np.random.default_rng(7).permutation(len(user))
    user, item = user[p], item[p]
    keep, rounds = check_core(gpu_ctx, user, item, n_users, n_items, 1, LONG + 1)
    assert rounds == 1 and keep.sum() == 70 * (LONG + 1)
    keep, rounds = check_core(gpu_ctx, user, item, n_users, n_items, LONG + 1, 1)
    assert rounds == 1 and keep.sum() == LONG + 1
    check_core(gpu_ctx, user, item, n_users, n_items, 71, LONG)
    check_split(gpu_ctx, user, item, n_users, n_items, sr.FOLDS, 3, min_user=2, min_item=2)


def test_more_users_than_one_pass_of_the_list_grid(gpu_ctx):
    """n_users = 262,144 + 40: degree_kernel's loop over lists takes a second trip.  Every user has one
    edge on items 0..9 except a few below and above the cap with three."""
    n_users, n_items = LIST_GRID + 40, 16
    user = np.arange(n_users, dtype=np.uint32)
    item = (user % 10).astype(np.uint32)
    three = np.array([0, 5, 70_000, LIST_GRID - 1, LIST_GRID, LIST_GRID + 7, n_users - 1], np.uint32)
    user = np.concatenate((user, np.repeat(three, 2)))
    item = np.concatenate((item, np.tile(np.array([12, 13], np.uint32), len(three))))
    keep, rounds = check_core(gpu_ctx, user, item, n_users, n_items, 3, 1)
    assert rounds == 1 and keep.sum() == 3 * len(three)
    res, _ = check_split(gpu_ctx, user, item, n_users, n_items, sr.LEAVE_K, 1, min_user=3, min_train=1, seed=3)
    assert res.users_alive == len(three) and res.validate == len(three)
    res, _ = check_split(gpu_ctx, user, item, n_users, n_items, sr.LEAVE_K, 1, seed=3)   # stats over all users
    assert res.users_alive == n_users and res.validate == n_users and res.train == 2 * len(three)


# ---- duplicates ----------------------------------------------------------------------------------
def test_last_of_a_repeated_pair_wins_with_its_own_key(gpu_ctx):
    """(0, 1) three times, not adjacent, keys 5, 1, 9: the third stays and is user 0's latest-keyed edge.
    User 1 has three lines but two pairs: at min_user = 3 it lives only if repeats were counted."""
    user = np.array([0, 0, 1, 0, 1, 0, 1, 0], np.uint32)
    item = np.array([1, 0, 0, 1, 2, 2, 0, 1], np.uint32)
    key = np.array([5, 3, 1, 1, 2, 4, 7, 9], np.uint64)
    res, _ = check_split(gpu_ctx, user, item, 2, 3, sr.LEAVE_K, 1, order_key=key)
    assert res.part.tolist() == [255, 1, 255, 255, 1, 0, 0, 0] and res.kept == 5
    res, _ = check_split(gpu_ctx, user, item, 2, 3, sr.LEAVE_K, 1, order_key=np.uint64(2**64 - 1) - key)
    assert res.part.tolist() == [255, 0, 255, 255, 0, 0, 1, 1]   # the key 9 of the last line, not 5 or 1
    keep, rounds = check_core(gpu_ctx, user, item, 2, 3, 3, 1)
    assert keep.tolist() == [False, True, False, False, False, True, False, True] and rounds == 1


# ---- hold-out boundaries ---------------------------------------------------------------------------
def validate_per_user(res, user, n_users):
    return np.bincount(user[res.part == 1], minlength=n_users).tolist()


def test_leave_k_at_the_min_train_boundaries(gpu_ctx):
    rng = np.random.default_rng(8)
    K, M = 2, 3
    degrees = [K + M, K + M - 1, M, 1, 0, K + M + 4]
    user, item = edges_of(degrees, 12, rng)
    res, _ = check_split(gpu_ctx, user, item, len(degrees), 12, sr.LEAVE_K, K, min_train=M, seed=1)
    assert validate_per_user(res, user, len(degrees)) == [2, 1, 0, 0, 0, 2]
    res, _ = check_split(gpu_ctx, user, item, len(degrees), 12, sr.LEAVE_K, 0, min_train=M, seed=1)
    assert res.validate == 0 and res.train == len(user)
    res, _ = check_split(gpu_ctx, user, item, len(degrees), 12, sr.LEAVE_K, 2**32 - 1, seed=1)   # everything held out
    assert res.train == 0 and res.items_without_train == res.items_alive


def test_ratio_rounds_down(gpu_ctx):
    rng = np.random.default_rng(9)
    degrees = [4, 5, 9, 10]
    user, item = edges_of(degrees, 15, rng)
    res, _ = check_split(gpu_ctx, user, item, 4, 15, sr.RATIO, 1, 5, seed=2)
    assert validate_per_user(res, user, 4) == [0, 1, 1, 2]
    res, _ = check_split(gpu_ctx, user, item, 4, 15, sr.RATIO, 4, 5, seed=2, min_train=3)
    assert validate_per_user(res, user, 4) == [1, 2, 6, 7]
    res, _ = check_split(gpu_ctx, user, item, 4, 15, sr.RATIO, 2**32 - 2, 2**32 - 1, seed=2)   # 64-bit product
    assert validate_per_user(res, user, 4) == [3, 4, 8, 9]


def test_folds_shorter_and_longer_than_a_user(gpu_ctx):
    rng = np.random.default_rng(10)
    F = 4
    degrees = [F - 1, F + 1, 1, 0, 2 * F]
    user, item = edges_of(degrees, 10, rng)
    res, _ = check_split(gpu_ctx, user, item, len(degrees), 10, sr.FOLDS, F, seed=4)
    for u, want in enumerate(([1, 1, 1, 0], [2, 1, 1, 1], [1, 0, 0, 0], [0, 0, 0, 0], [2, 2, 2, 2])):
        assert np.bincount(res.part[user == u], minlength=F).tolist() == want
    assert res.items_without_train == 0
    check_split(gpu_ctx, user, item, len(degrees), 10, sr.FOLDS, 254, seed=4)
    check_split(gpu_ctx, user, item, len(degrees), 10, sr.FOLDS, 2, seed=4)


def test_equal_keys_fall_back_on_the_item(gpu_ctx):
    """Time-style keys with ties inside a user: among equal keys the smaller item id comes first."""
    user = np.array([0, 0, 0, 0, 1, 1, 1], np.uint32)
    item = np.array([7, 2, 5, 3, 4, 1, 9], np.uint32)
    key = np.array([8, 8, 8, 9, 6, 6, 1], np.uint64)
    res, _ = check_split(gpu_ctx, user, item, 2, 10, sr.LEAVE_K, 2, order_key=key)
    assert res.part.tolist() == [0, 1, 1, 0, 0, 1, 1]
    rng = np.random.default_rng(11)
    user, item = edges_of([40] * 30, 60, rng)
    check_split(gpu_ctx, user, item, 30, 60, sr.RATIO, 1, 3, order_key=rng.integers(0, 3, len(user)).astype(np.uint64))
    top = np.uint64(2**64 - 1) - rng.integers(0, 3, len(user)).astype(np.uint64)   # the high bits of the key sort
    check_split(gpu_ctx, user, item, 30, 60, sr.FOLDS, 5, order_key=top)


@pytest.mark.parametrize("n_users", [1, 2, 255, 256, 257])
def test_key_widths(gpu_ctx, n_users):
    """bits_for(n_users) in the first sort and bits_for(n_users + 1) in the last: the highest user ids
    must keep their bits, and the mark n_users of a dead edge must sort behind them."""
    rng = np.random.default_rng(n_users)
    n_items = 9
    degrees = [int(d) for d in rng.integers(1, 8, n_users)]
    degrees[-1] = 7
    user, item = edges_of(degrees, n_items, rng)
    check_split(gpu_ctx, user, item, n_users, n_items, sr.LEAVE_K, 2, min_train=1, min_user=3, seed=n_users)
    check_split(gpu_ctx, user, item, n_users, n_items, sr.FOLDS, 3, seed=n_users)


# ---- invariance ------------------------------------------------------------------------------------
def test_split_does_not_depend_on_the_read_order(gpu_ctx):
    rng = np.random.default_rng(12)
    user, item = edges_of([int(d) for d in rng.integers(0, 30, 200)], 80, rng)
    kw = dict(min_user=4, min_item=3, min_train=2)
    a, _ = check_split(gpu_ctx, user, item, 200, 80, sr.LEAVE_K, 3, seed=77, **kw)
    p = rng.permutation(len(user))
    b, _ = check_split(gpu_ctx, user[p], item[p], 200, 80, sr.LEAVE_K, 3, seed=77, **kw)
    assert np.array_equal(a.part[p], b.part)
    again = gpu_ctx.holdout_split(200, 80, user, item, holdout=3, seed=77, **kw)
    assert again.part.tobytes() == a.part.tobytes() and all(getattr(again, f) == getattr(a, f) for f in STATS)
    c, _ = check_split(gpu_ctx, user, item, 200, 80, sr.LEAVE_K, 3, seed=78, **kw)
    assert c.validate == a.validate and not np.array_equal(c.part, a.part)


def test_host_and_device_forms_agree(gpu_ctx):
    import torch

    rng = np.random.default_rng(13)
    n_users, n_items = 500, 90
    user, item = edges_of([int(d) for d in rng.integers(0, 25, n_users)], n_items, rng)
    key = rng.integers(0, 50, len(user)).astype(np.uint64)
    n = len(user)
    T = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to("cuda:0")   # noqa: E731
    d_user, d_item, d_key = T(user.view(np.int32)), T(item.view(np.int32)), T(key.view(np.int64))
    for k in (None, key):
        host = gpu_ctx.holdout_split(n_users, n_items, user, item, ratio=(1, 4), order_key=k, seed=5, min_user=3,
                                     min_item=4, min_train=1)
        d_part = torch.full((n,), 7, dtype=torch.uint8, device="cuda:0")
        d_stats = torch.zeros(8, dtype=torch.int64, device="cuda:0")
        torch.cuda.synchronize()
        rc = gpu_ctx.lib.cf_holdout_split_run(gpu_ctx.h, n, n_users, n_items, ptr(d_user), ptr(d_item),
                                              ptr(d_key) if k is not None else None, 5, 3, 4, _native.CF_SPLIT_RATIO, 1, 4,
                                              1, ptr(d_part), ptr(d_stats), None)
        assert rc == CF_OK
        assert np.array_equal(d_part.cpu().numpy(), host.part)
        assert d_stats.cpu().numpy().tolist() == [getattr(host, f) for f in STATS]
        ms = gpu_ctx.split_timing()
        assert len(ms) == 4 and all(t >= 0 for t in ms) and gpu_ctx.prep_timing() >= max(ms)
    keep, rounds = gpu_ctx.kcore(n_users, n_items, user, item, 3, 4)
    d_keep = torch.full((n,), 7, dtype=torch.uint8, device="cuda:0")
    r = ctypes.c_uint32(99)
    torch.cuda.synchronize()
    rc = gpu_ctx.lib.cf_kcore_run(gpu_ctx.h, n, n_users, n_items, ptr(d_user), ptr(d_item), 3, 4, ptr(d_keep),
                                  ctypes.byref(r), None)
    assert rc == CF_OK and r.value == rounds and np.array_equal(d_keep.cpu().numpy().astype(bool), keep)
    assert np.array_equal(keep, host.part != 255)
    assert gpu_ctx.split_timing()[2:] == (0.0, 0.0)


# ---- arguments -------------------------------------------------------------------------------------
def test_no_edge_is_a_valid_call(gpu_ctx):
    e = np.zeros(0, np.uint32)
    for n_users, n_items in ((0, 0), (5, 7)):
        res = gpu_ctx.holdout_split(n_users, n_items, e, e, holdout=2)
        assert len(res.part) == 0 and [getattr(res, f) for f in STATS] == [0] * 8
        keep, rounds = gpu_ctx.kcore(n_users, n_items, e, e, 3, 3)
        assert len(keep) == 0 and rounds == 0
    res, _ = check_split(gpu_ctx, np.array([4], np.uint32), np.array([6], np.uint32), 5, 7, sr.LEAVE_K, 1)
    assert res.part.tolist() == [1]


def test_argument_errors(gpu_ctx):
    lib, h = gpu_ctx.lib, gpu_ctx.h
    user, item = np.array([0, 1, 2], np.uint32), np.array([0, 1, 1], np.uint32)
    part, keep, stats = np.zeros(3, np.uint8), np.zeros(3, np.uint8), np.zeros(8, np.uint64)
    rounds = ctypes.c_uint32()

    def split(n=3, n_users=3, n_items=2, u=user, m=item, mode=0, a=1, b=0, out=part):
        return lib.cf_holdout_split(h, n, n_users, n_items, ptr(u) if u is not None else None,
                                    ptr(m) if m is not None else None, None, 0, 0, 0, mode, a, b, 0,
                                    ptr(out) if out is not None else None, ptr(stats))

    def core(n=3, n_users=3, n_items=2, u=user, m=item, out=keep, r=rounds):
        return lib.cf_kcore(h, n, n_users, n_items, ptr(u) if u is not None else None, ptr(m) if m is not None else None,
                            2, 2, ptr(out) if out is not None else None, ctypes.byref(r) if r is not None else None)

    assert split() == CF_OK and core() == CF_OK
    for bad in (dict(n_users=2), dict(n_items=1), dict(u=None), dict(m=None), dict(out=None)):   # ids, null arrays
        assert split(**bad) == CF_EINVAL, bad
        assert core(**bad) == CF_EINVAL, bad
        assert b"cf_" in lib.cf_last_error(h)
    assert core(r=None) == CF_EINVAL
    for bad in (dict(mode=3), dict(mode=-1), dict(mode=1, a=0, b=5), dict(mode=1, a=5, b=5), dict(mode=1, a=6, b=5),
                dict(mode=2, a=1), dict(mode=2, a=0), dict(mode=2, a=255)):
        assert split(**bad) == CF_EINVAL, bad
    assert split(mode=1, a=4, b=5) == CF_OK and split(mode=2, a=2) == CF_OK and split(mode=2, a=254) == CF_OK
    assert split(n=1 << 31) == CF_ERANGE and core(n=1 << 31) == CF_ERANGE   # checked before anything is read
    assert lib.cf_split_timing(h, None) == CF_EINVAL

    import torch   # the device forms find a bad id themselves

    d_user = torch.tensor([0, 1, 3], dtype=torch.int32, device="cuda:0")
    d_item = torch.tensor([0, 1, 1], dtype=torch.int32, device="cuda:0")
    d_part = torch.zeros(3, dtype=torch.uint8, device="cuda:0")
    torch.cuda.synchronize()
    assert lib.cf_holdout_split_run(h, 3, 3, 2, ptr(d_user), ptr(d_item), None, 0, 0, 0, 0, 1, 0, 0, ptr(d_part), None,
                                    None) == CF_EINVAL
    assert lib.cf_kcore_run(h, 3, 3, 2, ptr(d_user), ptr(d_item), 2, 2, ptr(d_part), ctypes.byref(rounds), None) == CF_EINVAL
    assert lib.cf_holdout_split_run(h, 3, 4, 2, ptr(d_user), ptr(d_item), None, 0, 0, 0, 0, 1, 0, 0, ptr(d_part), None,
                                    None) == CF_OK
    res = gpu_ctx.holdout_split(3, 2, user, item, holdout=1)   # the context still works
    assert res.part.tolist() == [1, 1, 1]
