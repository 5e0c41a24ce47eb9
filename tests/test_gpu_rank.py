"""Ranking evaluation of fitted factors on the GPU (cf_mf_rank_eval) against the numpy checker
tests/rank_ref.py.

Exact cases use integer-valued factors in [-4, 4] and integer-valued biases, so every score is an
exact integer in any summation order (and ties are heavy): rank, n_cand, n_rel and hits must equal
the checker's exactly.  The per-user metrics are normalised sums of at most 1024 terms in [0, 1],
each a few roundings of 1.1e-16, and the library's log2 may differ from numpy's by an ulp:
1024 * 3 * 1.1e-16 = 3.4e-13, so they are held to 1e-12 absolute and the summary means to 1e-11.
The real-valued case first shows in the checker that every held-out edge's rank window under the
score bound of test_gpu_topn.py is a single rank, and then asks for exact ranks as well."""
import ctypes

import numpy as np
import pytest

import rank_ref as rr
import topn_ref as tr
from collaborative_filtering_amd import _native
from collaborative_filtering_amd._native import ptr
from collaborative_filtering_amd.api import RANK_USER_DTYPE

pytestmark = pytest.mark.gpu

MAX = 0xFFFFFFFF
USER_TOL = 1e-12
MEAN_TOL = 1e-11


def consts():
    """TU, TI (the score tile), T (targets per walk), W (keys per trip of the walk)."""
    lib = _native.load()
    return lib.cf_debug_topn_tile_users(), lib.cf_debug_topn_tile_items(), lib.cf_debug_rank_targets(), lib.cf_debug_rank_walk()


def int_factors(rng, n, D):
    return rng.integers(-4, 5, (n, D)).astype(np.float64)


def random_exclusions(rng, n_users, n_items, frac):
    m = rng.random((n_users, n_items)) < frac
    u, i = np.nonzero(m)
    p = rng.permutation(len(u))
    return u[p].astype(np.uint32), i[p].astype(np.uint32)


def held_by_counts(rng, counts, n_items):
    """counts[u] distinct items per user (excluded ones may be among them), shuffled over users."""
    hu = np.concatenate([np.full(c, u) for u, c in enumerate(counts)] + [np.zeros(0, np.int64)])
    hi = np.concatenate([rng.choice(n_items, c, replace=False) for c in counts] + [np.zeros(0, np.int64)])
    p = rng.permutation(len(hu))
    return hu[p].astype(np.uint32), hi[p].astype(np.uint32)


def assert_matches(got, want, *, n_nan_held=None):
    rank, n_cand, users, s = want
    assert np.array_equal(got.rank, rank), (got.rank, rank)
    assert np.array_equal(got.n_cand, n_cand)
    assert len(got.users) == len(users)
    for f in ("n_cand", "n_rel", "hits"):
        assert got.users[f].tolist() == [r[f] for r in users], f
    assert not got.users["reserved"].any()
    worst = 0.0
    for f in ("precision", "recall", "ndcg", "ap", "rr", "auc"):
        ref = np.array([r[f] for r in users], dtype=np.float64)
        if len(ref):
            worst = max(worst, float(np.abs(got.users[f] - ref).max()))
    print("largest per-user metric difference:", worst)
    assert worst <= USER_TOL
    for f in ("users_evaluated", "users_auc", "edges_counted", "edges_skipped"):
        assert got.summary[f] == s[f], (f, got.summary[f], s[f])
    assert got.summary["n_nan_held"] == (s["n_nan_held"] if n_nan_held is None else n_nan_held)
    for f in rr.MEAN_FIELDS:
        print(f, got.summary[f], s[f])
        assert abs(got.summary[f] - s[f]) <= MEAN_TOL, f
    # an unevaluated user's record is all zeros
    idle = got.users["n_rel"] == 0
    assert not np.frombuffer(got.users[idle].tobytes(), dtype=np.uint8).any()


EXACT_NAMES = ["one", "row_under_tile", "tile_exact", "tile_plus_one", "many_tiles", "max_d", "all_equal", "walk_minus",
               "walk", "walk_plus"]


def exact_cases():
    """name -> (n_users, n_items, D, N, kind): n_items over {1, TI-1, TI, TI+1, 3 TI + 5, W-1, W,
    W+1} (the last three with at most 3 users), n_users over {1, TU+1, 2 TU + 3}, D over {1, 5,
    20, 64}, N over {1, 7, 1024}."""
    TU, TI, T, W = consts()
    big = 3 * TI + 5
    return {
        "one": (1, 1, 1, 1, "plain"),
        "row_under_tile": (1, TI - 1, 5, 7, "bias"),
        "tile_exact": (TU + 1, TI, 5, 7, "plain"),
        "tile_plus_one": (TU + 1, TI + 1, 20, 1, "bias_excl"),
        "many_tiles": (2 * TU + 3, big, 20, 7, "counts_excl"),
        "max_d": (2 * TU + 3, big, 64, 1024, "bias_excl"),
        "all_equal": (TU + 1, big, 20, 7, "v_zero_excl"),
        "walk_minus": (3, W - 1, 5, 7, "plain_excl"),
        "walk": (2, W, 1, 1024, "bias"),
        "walk_plus": (3, W + 1, 20, 7, "plain_excl"),
    }


def exact_inputs(name):
    _, _, T, _ = consts()
    nu, ni, D, N, kind = exact_cases()[name]
    rng = np.random.default_rng(300 + EXACT_NAMES.index(name))
    U, V = int_factors(rng, nu, D), int_factors(rng, ni, D)
    kw = {}
    if kind.startswith("bias"):
        kw = dict(bias_user=rng.integers(-3, 4, nu).astype(np.float64),
                  bias_item=rng.integers(-3, 4, ni).astype(np.float64), mean=2.0)
    if kind.startswith("v_zero"):
        V = np.zeros((ni, D))
    if kind.endswith("_excl"):
        kw["exclude"] = random_exclusions(rng, nu, ni, 0.3)
    if kind.startswith("counts"):   # every held-out count at which the kernel takes another number of walks
        pattern = [0, 1, T - 1, T, T + 1, 2 * T + 3]
        counts = [pattern[u % len(pattern)] for u in range(nu)]
    else:
        counts = rng.integers(0, min(ni, 6) + 1, nu).tolist()
        counts[0] = max(counts[0], 1)
    return U, V, N, held_by_counts(rng, counts, ni), kw


@pytest.mark.parametrize("name", EXACT_NAMES)
def test_exact_case_equals_checker(gpu_ctx, name):
    U, V, N, held, kw = exact_inputs(name)
    S = tr.score_matrix(U, V, kw.get("bias_user"), kw.get("bias_item"), kw.get("mean", 0.0))
    assert np.array_equal(S, np.round(S)) and np.abs(S).max() < 2.0 ** 52   # exact integers
    want = rr.evaluate(U, V, N, held, **kw)
    if "exclude" in kw and len(held[0]) > 50:
        assert want[3]["edges_skipped"] > 0 and want[3]["edges_counted"] > 0   # held-out and excluded both occur
    if S.size > 1000 and not exact_cases()[name][4].startswith("v_zero"):
        ties = sum(int((S[u] == S[u, i]).sum()) - 1 for u, i in zip(held[0].astype(int), held[1].astype(int)))
        print(name, "held-out edges", len(held[0]), "equal scores among their rows", ties)
        assert ties >= len(held[0]) // 2   # ties are common: the item order decides many ranks
    got = gpu_ctx.mf_rank_eval(U, V, N, held, **kw)
    print(name, "blocks", got.stats.blocks, "score_ms", got.stats.score_ms, "rank_ms", got.stats.rank_ms)
    assert_matches(got, want)
    assert got.stats.blocks >= 1


def test_special_users(gpu_ctx):
    """User 0 excludes every item, user 1's only held-out item is excluded, user 2 holds out every
    candidate (C = m), user 3 has no held-out edge, user 4 is ordinary; on an all-equal row as well."""
    _, TI, _, _ = consts()
    ni, D = TI + 1, 5
    rng = np.random.default_rng(21)
    U, V = int_factors(rng, 5, D), int_factors(rng, ni, D)
    ex2 = rng.choice(ni, ni - 9, replace=False)
    excl_rows = [np.arange(ni), np.array([3, 8]), ex2, np.array([1]), rng.choice(ni, 10, replace=False)]
    held_rows = [np.array([2, 5]), np.array([8]), np.setdiff1d(np.arange(ni), ex2), np.zeros(0, np.int64),
                 rng.choice(ni, 6, replace=False)]
    eu = np.concatenate([np.full(len(r), u) for u, r in enumerate(excl_rows)]).astype(np.uint32)
    ei = np.concatenate(excl_rows).astype(np.uint32)
    hu = np.concatenate([np.full(len(r), u) for u, r in enumerate(held_rows)]).astype(np.uint32)
    hi = np.concatenate(held_rows).astype(np.uint32)
    for N in (1, 7, 1024):
        for Vx in (V, np.zeros_like(V)):
            want = rr.evaluate(U, Vx, N, (hu, hi), exclude=(eu, ei))
            got = gpu_ctx.mf_rank_eval(U, Vx, N, (hu, hi), exclude=(eu, ei))
            assert_matches(got, want)
            assert (got.rank[hu == 0] == MAX).all() and (got.rank[hu == 1] == MAX).all()
            assert got.users["n_cand"].tolist()[:4] == [0, 0, 9, 0] and got.users["n_rel"][2] == 9
            assert sorted(got.rank[hu == 2].tolist()) == list(range(9))
            assert got.users["auc"][2] == 0.0 and got.summary["users_auc"] == 1 and got.summary["users_evaluated"] == 2
            assert got.summary["edges_skipped"] == 3 + int(np.isin(held_rows[4], excl_rows[4]).sum())


_REAL = {}


def real_inputs():
    """The inputs of test_gpu_topn.real_inputs rebuilt (seed 11, 150 x (2 TI + 37), D = 20, uniform
    factors, U before V, a fifth of the pairs excluded), then the held-out pairs random < 0.06
    minus the exclusions from the same generator; built once, never modified."""
    if not _REAL:
        _, TI, _, _ = consts()
        rng = np.random.default_rng(11)
        nu, ni, D = 150, 2 * TI + 37, 20
        U, V = rng.uniform(-1, 1, (nu, D)), rng.uniform(-1, 1, (ni, D))
        mask = rng.random((nu, ni)) < 0.2   # the exclusion set of test_gpu_topn.real_inputs
        hu, hi = np.nonzero((rng.random((nu, ni)) < 0.06) & ~mask)
        eu, ei = np.nonzero(mask)
        p = np.random.default_rng(12).permutation(len(eu))   # the list's order is its own draw
        exclude = (eu[p].astype(np.uint32), ei[p].astype(np.uint32))
        _REAL.update(U=U, V=V, N=10, exclude=exclude, mask=mask, held=(hu.astype(np.uint32), hi.astype(np.uint32)))
    return _REAL


def real_device(ctx):
    r = real_inputs()
    if "got" not in r:
        r["got"] = ctx.mf_rank_eval(r["U"], r["V"], r["N"], r["held"], exclude=r["exclude"])
    return r["got"]


def test_real_valued_case(gpu_ctx):
    r = real_inputs()
    U, V, N, held = r["U"], r["V"], r["N"], r["held"]
    per_user = np.bincount(held[0], minlength=U.shape[0])
    print("held-out edges", len(held[0]), "per user", per_user.min(), "to", per_user.max())
    assert len(held[0]) == 1186 and per_user.min() == 2 and per_user.max() == 18
    lo, hi, gap, bmax = rr.rank_windows(U, V, held, mask=r["mask"])
    print("smallest score gap", gap, "largest bound", bmax)
    assert gap > 1000 * bmax and np.array_equal(lo, hi)   # every window is a single rank
    want = rr.evaluate(U, V, N, held, exclude=r["exclude"])
    assert np.array_equal(want[0], lo.astype(np.uint32))
    got = real_device(gpu_ctx)
    assert_matches(got, want)


def test_ranks_of_topn_lists_are_their_positions(gpu_ctx):
    r = real_inputs()
    U, V, N, ex = r["U"], r["V"], r["N"], r["exclude"]
    top = gpu_ctx.mf_topn(U, V, N, exclude=ex)
    assert (top.count == N).all()
    hu = np.repeat(np.arange(U.shape[0], dtype=np.uint32), N)
    hi = top.items.reshape(-1)
    got = gpu_ctx.mf_rank_eval(U, V, N, (hu, hi), exclude=ex)
    assert np.array_equal(got.rank.reshape(-1, N), np.tile(np.arange(N, dtype=np.uint32), (U.shape[0], 1)))
    assert (got.users["hits"] == N).all() and (got.users["ndcg"] == 1.0).all() and (got.users["ap"] == 1.0).all()
    assert got.summary["edges_skipped"] == 0 and got.summary["precision"] == 1.0


def same_bytes(a, b):
    return (np.array_equal(a.rank, b.rank) and np.array_equal(a.n_cand, b.n_cand) and a.users.tobytes() == b.users.tobytes()
            and all(np.float64(a.summary[k]).tobytes() == np.float64(b.summary[k]).tobytes() for k in a.summary))


def test_results_do_not_depend_on_blocking_or_history(gpu_ctx):
    TU, _, _, _ = consts()
    r = real_inputs()
    U, V, N, held, ex = r["U"], r["V"], r["N"], r["held"], r["exclude"]
    base = real_device(gpu_ctx)
    assert base.stats.blocks == 1
    try:
        for ub in (1, TU + 1):
            gpu_ctx.set_topn_block(ub)
            got = gpu_ctx.mf_rank_eval(U, V, N, held, exclude=ex)
            assert got.stats.blocks == -(-U.shape[0] // ub)   # every user has a held-out edge
            assert same_bytes(got, base)
    finally:
        gpu_ctx.set_topn_block(0)
    assert same_bytes(gpu_ctx.mf_rank_eval(U, V, N, held, exclude=ex), base)   # a repeat
    gpu_ctx.release_workspaces()
    assert same_bytes(gpu_ctx.mf_rank_eval(U, V, N, held, exclude=ex), base)


def test_nan_held_out_items_are_skipped_and_counted(gpu_ctx):
    TU, TI, _, _ = consts()
    nu, ni, D, N, bad = TU + 1, TI + 1, 5, 9, 7
    rng = np.random.default_rng(13)
    U, V = int_factors(rng, nu, D), int_factors(rng, ni, D)
    eu, ei = random_exclusions(rng, nu, ni, 0.1)
    excluding = np.unique(eu[ei == bad])
    assert 0 < len(excluding) < nu
    counts = rng.integers(1, 6, nu).tolist()
    hu, hi = held_by_counts(rng, counts, ni)
    keep = hi != bad
    hu = np.concatenate([hu[keep], np.arange(0, nu, 2, dtype=np.uint32)])   # every second user holds the bad item out
    hi = np.concatenate([hi[keep], np.full(len(range(0, nu, 2)), bad, np.uint32)])
    holders = np.arange(0, nu, 2)
    assert np.isin(holders, excluding).any() and not np.isin(holders, excluding).all()
    Vn = V.copy()
    Vn[bad, 2] = np.nan
    # the checker with the item masked for everyone, on finite data
    every = (np.concatenate([eu, np.arange(nu, dtype=np.uint32)]), np.concatenate([ei, np.full(nu, bad, np.uint32)]))
    want = rr.evaluate(U, V, N, (hu, hi), exclude=every)
    got = gpu_ctx.mf_rank_eval(U, Vn, N, (hu, hi), exclude=(eu, ei))
    n_nan = len(holders) - int(np.isin(holders, excluding).sum())
    assert (got.rank[hi == bad] == MAX).all()
    assert_matches(got, want, n_nan_held=n_nan)
    # the checker's own NaN handling agrees
    ref = rr.evaluate(U, Vn, N, (hu, hi), exclude=(eu, ei))
    assert np.array_equal(ref[0], want[0]) and ref[3]["n_nan_held"] == n_nan


def test_weighted_mpr(gpu_ctx):
    U, V, N, held, kw = exact_inputs("many_tiles")
    rng = np.random.default_rng(5)
    w = rng.integers(1, 6, len(held[0])).astype(np.float64)
    want = rr.evaluate(U, V, N, (held[0], held[1], w), **kw)
    plain = rr.evaluate(U, V, N, held, **kw)
    assert abs(want[3]["mpr"] - plain[3]["mpr"]) > 1e-6   # the weights matter here
    got = gpu_ctx.mf_rank_eval(U, V, N, (held[0], held[1], w), **kw)
    assert_matches(got, want)
    unweighted = gpu_ctx.mf_rank_eval(U, V, N, held, **kw)
    assert unweighted.users.tobytes() == got.users.tobytes() and np.array_equal(unweighted.rank, got.rank)
    assert all(unweighted.summary[k] == got.summary[k] for k in got.summary if k != "mpr")


def test_api_rejects_a_repeated_pair(gpu_ctx):
    U, V = np.ones((2, 3)), np.ones((4, 3))
    with pytest.raises(ValueError):
        gpu_ctx.mf_rank_eval(U, V, 2, (np.array([1, 0, 1]), np.array([2, 2, 2])))


FILL = 0xAB


def raw_call(ctx, nu, ni, D, N, *, eoff=None, eitem=None, hoff="zeros", hitem="one", out=None):
    U = np.zeros((max(nu, 1), max(D, 1)))
    V = np.zeros((max(ni, 1), max(D, 1)))
    if isinstance(hoff, str):
        hoff = np.zeros(nu + 1, np.uint64)
    if isinstance(hitem, str):
        hitem = np.zeros(1, np.uint32)
    n_held = int(hoff[-1]) if hoff is not None else 0
    rank = np.full(max(n_held, 1), 12345, np.uint32)
    users = np.frombuffer(bytes([FILL]) * (RANK_USER_DTYPE.itemsize * max(nu, 1)), dtype=RANK_USER_DTYPE).copy()
    st = _native.RankSummary()
    st.users_evaluated = 99
    rc = ctx.lib.cf_mf_rank_eval(ctx.h, nu, ni, D, ptr(U), ptr(V), None, None, 0.0, ptr(eoff), ptr(eitem), ptr(hoff),
                                 ptr(hitem), None, N, ptr(rank), ptr(users), ctypes.byref(st))
    if out is not None:
        out.update(rank=rank, users=users, st=st)
    return rc


def untouched(out):
    return ((out["rank"] == 12345).all() and (np.frombuffer(out["users"].tobytes(), np.uint8) == FILL).all()
            and out["st"].users_evaluated == 99)


def test_argument_checks(gpu_ctx):
    ctx = gpu_ctx
    ok_off = np.array([0, 1, 2], np.uint64)
    ok_item = np.array([0, 2], np.uint32)
    out = {}
    assert raw_call(ctx, 2, 3, 0, 1, out=out) == _native.CF_ERANGE and untouched(out)
    assert raw_call(ctx, 2, 3, _native.CF_ALS_MAX_D + 1, 1) == _native.CF_ERANGE
    assert raw_call(ctx, 2, 3, 4, _native.CF_TOPN_MAX_N + 1) == _native.CF_ERANGE
    assert raw_call(ctx, 2, 3, 4, 0) == _native.CF_EINVAL
    assert raw_call(ctx, 2, 3, 0, 0) == _native.CF_ERANGE   # the range checks come first
    assert raw_call(ctx, 2, 3, 4, 1, eoff=ok_off) == _native.CF_EINVAL
    assert raw_call(ctx, 2, 3, 4, 1, eitem=ok_item) == _native.CF_EINVAL
    assert raw_call(ctx, 2, 3, 4, 1, eoff=np.array([0, 2, 1], np.uint64), eitem=ok_item) == _native.CF_EINVAL
    assert raw_call(ctx, 2, 3, 4, 1, eoff=ok_off, eitem=np.array([0, 3], np.uint32)) == _native.CF_EINVAL
    assert raw_call(ctx, 2, 3, 4, 1, hoff=None) == _native.CF_EINVAL                                   # no held-out CSR
    assert raw_call(ctx, 2, 3, 4, 1, hoff=ok_off, hitem=None) == _native.CF_EINVAL
    assert raw_call(ctx, 2, 3, 4, 1, hoff=np.array([1, 1, 2], np.uint64), hitem=ok_item) == _native.CF_EINVAL
    assert raw_call(ctx, 2, 3, 4, 1, hoff=np.array([0, 2, 1], np.uint64), hitem=ok_item) == _native.CF_EINVAL
    assert raw_call(ctx, 2, 3, 4, 1, hoff=ok_off, hitem=np.array([0, 3], np.uint32)) == _native.CF_EINVAL   # item >= n_items
    two = np.array([0, 2, 2], np.uint64)
    assert raw_call(ctx, 2, 3, 4, 1, hoff=two, hitem=np.array([1, 1], np.uint32)) == _native.CF_EINVAL    # a pair twice
    assert raw_call(ctx, 2, 3, 4, 1, hoff=two, hitem=np.array([2, 1], np.uint32), out=out) == _native.CF_EINVAL   # descending
    assert untouched(out)
    assert b"cf_mf_rank_eval" in ctx.lib.cf_last_error(ctx.h)
    assert raw_call(ctx, 2, 3, 4, 1, eoff=ok_off, eitem=ok_item, hoff=two, hitem=np.array([1, 2], np.uint32), out=out) == _native.CF_OK
    assert out["rank"].tolist() == [0, 1] and out["st"].users_evaluated == 1 and out["users"]["n_cand"].tolist() == [2, 0]
    assert raw_call(ctx, 2, 3, 4, _native.CF_TOPN_MAX_N, hoff=ok_off, hitem=ok_item) == _native.CF_OK


def test_empty_calls_write_zeros(gpu_ctx):
    ctx = gpu_ctx
    out = {}

    def zeroed(n):
        return (not np.frombuffer(out["users"][:n].tobytes(), np.uint8).any() and out["st"].users_evaluated == 0
                and out["st"].edges_counted == 0 and out["st"].mpr == 0.0 and out["st"].blocks == 0)

    assert raw_call(ctx, 0, 3, 4, 2, out=out) == _native.CF_OK   # no users
    assert zeroed(0) and (np.frombuffer(out["users"].tobytes(), np.uint8) == FILL).all() and (out["rank"] == 12345).all()
    assert raw_call(ctx, 3, 0, 4, 2, out=out) == _native.CF_OK   # no items
    assert zeroed(3) and (out["rank"] == 12345).all()
    assert raw_call(ctx, 3, 5, 4, 2, out=out) == _native.CF_OK   # no held-out edges
    assert zeroed(3) and (out["rank"] == 12345).all()
    r = ctx.mf_rank_eval(np.zeros((0, 4)), np.zeros((6, 4)), 3, (np.zeros(0, np.uint32), np.zeros(0, np.uint32)))
    assert r.rank.shape == (0,) and r.users.shape == (0,) and r.summary["users_evaluated"] == 0
    r = ctx.mf_rank_eval(np.zeros((2, 4)), np.zeros((3, 4)), 3, (np.zeros(0, np.uint32), np.zeros(0, np.uint32)),
                         exclude=(np.array([0]), np.array([1])))
    assert r.rank.shape == (0,) and not r.users["n_cand"].any() and r.summary["mpr"] == 0.0
