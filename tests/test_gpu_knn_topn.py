"""Top-N recommendation and ranking evaluation from the item graph on the GPU (cf_knn_topn,
cf_knn_rank_eval) against the numpy checker tests/knn_topn_ref.py.

The checker does, per user and profile entry in order, the same IEEE operations in float64 from
the same float32 weights as the device (the product of two floats is exact in fp64), so every
list, score, rank and record is compared byte for byte, for real-valued weights and two-decimal
ratings too.  MEAN mode divides two doubles once per score: IEEE division on both sides."""
import ctypes

import numpy as np
import pytest

import knn_topn_ref as kr
from collaborative_filtering_amd import _native
from collaborative_filtering_amd._native import ptr
from collaborative_filtering_amd.api import Context

pytestmark = pytest.mark.gpu

MAX = 0xFFFFFFFF
T = 256   # kAT, the threads of a workgroup (cf_mf_common.h)
MODES = ("sum", "mean")


def consts():
    """TU, TI (the score tile of the mf source: the sizes the panel is tested at) and Wk."""
    lib = _native.load()
    wk = lib.cf_debug_knn_topn_walk()
    assert wk % T == 0 and wk > T
    return lib.cf_debug_topn_tile_users(), lib.cf_debug_topn_tile_items(), wk


def csr_of(W):
    rp = np.zeros(W.shape[0] + 1, np.uint64)
    rp[1:] = np.cumsum((W != 0).sum(axis=1))
    r, c = np.nonzero(W)
    return rp, c.astype(np.uint32), W[r, c].astype(np.float32)


def profiles(lists, rng, decimals=2):
    """lists of item arrays -> (off, items, ratings) with two-decimal ratings."""
    off = np.cumsum([0] + [len(x) for x in lists]).astype(np.uint64)
    items = np.concatenate([np.asarray(x, np.int64) for x in lists] + [np.zeros(0, np.int64)]).astype(np.uint32)
    ratings = np.round(rng.normal(3.0, 1.5, len(items)), decimals).astype(np.float32)
    return off, items, ratings


def assert_same_bytes(got, want):
    items, scores, count = want[:3]
    assert np.array_equal(got.count, count), (got.count, count)
    assert np.array_equal(got.items, items)
    assert np.array_equal(got.scores.view(np.uint64), scores.view(np.uint64))
    if len(want) > 3:
        assert got.stats.n_nan == want[3]


def random_graph(rng, n, density):
    """Real-valued weights in (0, 1), about a third of them under the default w_min, zero diagonal."""
    W = (rng.random((n, n)) ** 2 * (rng.random((n, n)) < density)).astype(np.float32)
    np.fill_diagonal(W, 0.0)
    return W


# ---- the panel sizes ------------------------------------------------------------------------------
SIZE_NAMES = ["one", "under_tile", "tile", "tile_plus_one", "many_tiles"]


def size_of(name):
    _, TI, _ = consts()
    return {"one": 1, "under_tile": TI - 1, "tile": TI, "tile_plus_one": TI + 1, "many_tiles": 3 * TI + 5}[name]


@pytest.mark.parametrize("name", SIZE_NAMES)
def test_panel_sizes_both_modes(gpu_ctx, name):
    n = size_of(name)
    rng = np.random.default_rng(500 + SIZE_NAMES.index(name))
    W = random_graph(rng, n, 0.5)
    if n == 1:
        W[0, 0] = 0.75   # i_t == m is no special case
    lists = [rng.choice(n, min(k, n), replace=False) for k in (0, 1, 2, 9, 30)] + [np.array([0, n - 1, 0])]   # a repeated item
    off, items, ratings = profiles(lists, rng)
    gpu_ctx.upload_graph_dense(W)
    for mode in MODES:
        for N in sorted({1, 7, n}):
            want = kr.topn(W, off, items, ratings, N, mode=mode)
            assert_same_bytes(gpu_ctx.knn_topn(off, items, ratings, N, mode=mode), want)
        want = kr.topn(W, off, items, ratings, n, mode=mode, exclude=None)
        got = gpu_ctx.knn_topn(off, items, ratings, n, mode=mode, exclude=None)
        assert_same_bytes(got, want)
        # the empty profile: every score 0, the lowest ids
        assert got.items[0].tolist() == list(range(n)) and not got.scores[0].any()


# ---- in-list lengths by construction --------------------------------------------------------------
_BIG = {}


def big_case():
    """One graph of 2 Wk + 3 + 48 items: columns 0..7 have in-lists (entries above w_min = 0.1) of
    exactly 0, 1, T-1, T, T+1, Wk, Wk+1 and 2 Wk + 3 entries, each also with entries at or under
    w_min; columns 8..47 share one set of 600 rows, so consecutive profile items hit the same m; the
    rest is sparse and random.  Asymmetric by construction.  Users: profiles of 0, 1, 2 and T + 44
    items, a repeated item, the eight constructed columns in both orders, the shared block."""
    if _BIG:
        return _BIG
    _, _, Wk = consts()
    rng = np.random.default_rng(77)
    lens = [0, 1, T - 1, T, T + 1, Wk, Wk + 1, 2 * Wk + 3]
    n = 2 * Wk + 3 + 48
    W = (rng.random((n, n)) * (rng.random((n, n)) < 0.01)).astype(np.float32)
    for c, L in enumerate(lens):
        W[:, c] = 0.0
        rows = rng.choice(n, max(L - 1, 0), replace=False)
        W[rows, c] = (0.11 + 0.89 * rng.random(len(rows))).astype(np.float32)
        rest = np.setdiff1d(np.arange(n), rows)
        low = rng.choice(rest, 40, replace=False)
        W[low, c] = np.float32(0.09) * rng.random(len(low)).astype(np.float32)   # under w_min: out
        if L:
            W[low[0], c] = np.float32(0.1)   # (double) float32(0.1) > 0.1 holds: the L-th entry
    shared = rng.choice(n, 600, replace=False)
    for c in range(8, 48):
        W[:, c] = 0.0
        W[shared, c] = (0.2 + 0.8 * rng.random(600)).astype(np.float32)
    above = (W.astype(np.float64) > 0.1).sum(axis=0)
    assert above[:8].tolist() == lens
    assert not np.array_equal(W, W.T)
    lists = [np.zeros(0, np.int64), np.array([5]), np.array([7, 2]), rng.choice(n, T + 44, replace=False),
             np.array([6, 7, 6, 60, 7]), np.arange(8), np.arange(8)[::-1], np.arange(8, 48),
             np.concatenate([np.arange(8, 48), rng.choice(n, 30, replace=False), np.arange(47, 7, -1)])]
    off, items, ratings = profiles(lists, rng)
    _BIG.update(W=W, off=off, items=items, ratings=ratings, n=n, want={})
    return _BIG


def big_want(mode, N):
    b = big_case()
    if (mode, N) not in b["want"]:
        b["want"][(mode, N)] = kr.topn(b["W"], b["off"], b["items"], b["ratings"], N, mode=mode)
    return b["want"][(mode, N)]


def test_in_list_lengths_profiles_and_overlap(gpu_ctx):
    b = big_case()
    gpu_ctx.upload_graph_dense(b["W"])
    for mode in MODES:
        for N in (7, 1024):   # a row longer than 1024 with N = 1024
            got = gpu_ctx.knn_topn(b["off"], b["items"], b["ratings"], N, mode=mode)
            assert_same_bytes(got, big_want(mode, N))
            assert got.stats.blocks == 1
    # the transposed scatter gives other lists
    wrong = kr.topn(b["W"].T, b["off"], b["items"], b["ratings"], 7)
    assert not np.array_equal(wrong[0], big_want("sum", 7)[0])


def test_same_bytes_for_blocking_layout_selection_and_history(gpu_ctx):
    b = big_case()
    off, items, ratings = b["off"], b["items"], b["ratings"]
    n_users = len(off) - 1
    try:
        for layout in ("dense", "csr"):
            gpu_ctx.set_graph_layout(layout)
            gpu_ctx.upload_graph_dense(b["W"])
            assert gpu_ctx.graph_info()[0] == layout
            for mode in MODES:
                want = big_want(mode, 7)
                for ub in (1, 3, 0):
                    gpu_ctx.set_topn_block(ub)
                    got = gpu_ctx.knn_topn(off, items, ratings, 7, mode=mode)
                    assert got.stats.blocks == (-(-n_users // ub) if ub else 1)
                    assert_same_bytes(got, want)
    finally:
        gpu_ctx.set_topn_block(0)
        gpu_ctx.set_graph_layout("dense")
    # the same graph uploaded as a CSR
    gpu_ctx.upload_graph_csr(b["n"], *csr_of(b["W"]))
    want = big_want("mean", 7)
    assert_same_bytes(gpu_ctx.knn_topn(off, items, ratings, 7, mode="mean"), want)
    assert_same_bytes(gpu_ctx.knn_topn(off, items, ratings, 7, mode="mean"), want)   # a repeat: cached in-lists
    sel = np.array([8, 3, 0, 3], np.uint32)
    got = gpu_ctx.knn_topn(off, items, ratings, 7, mode="mean", users=sel)
    assert_same_bytes(got, (want[0][sel], want[1][sel], want[2][sel]))
    gpu_ctx.release_workspaces()
    assert_same_bytes(gpu_ctx.knn_topn(off, items, ratings, 7, mode="mean"), want)


def test_new_graph_and_new_w_min_replace_the_cached_in_lists(gpu_ctx):
    rng = np.random.default_rng(9)
    n = 70
    W1, W2 = random_graph(rng, n, 0.4), random_graph(rng, n, 0.4)
    off, items, ratings = profiles([rng.choice(n, k, replace=False) for k in (5, 12, 1)], rng)
    gpu_ctx.upload_graph_dense(W1)
    assert_same_bytes(gpu_ctx.knn_topn(off, items, ratings, 9), kr.topn(W1, off, items, ratings, 9))
    gpu_ctx.upload_graph_dense(W2)
    want2 = kr.topn(W2, off, items, ratings, 9)
    assert not np.array_equal(want2[0], kr.topn(W1, off, items, ratings, 9)[0])
    assert_same_bytes(gpu_ctx.knn_topn(off, items, ratings, 9), want2)
    want3 = kr.topn(W2, off, items, ratings, 9, w_min=0.5)
    assert not np.array_equal(want3[1], want2[1])
    assert_same_bytes(gpu_ctx.knn_topn(off, items, ratings, 9, w_min=0.5), want3)
    assert_same_bytes(gpu_ctx.knn_topn(off, items, ratings, 9), want2)


def test_threshold_is_strict(gpu_ctx):
    W = np.zeros((3, 3), np.float32)
    W[1, 0] = 0.125
    W[2, 0] = 0.125 + 2.0 ** -20
    off, items, ratings = np.array([0, 1], np.uint64), np.array([0], np.uint32), np.array([1.0], np.float32)
    gpu_ctx.upload_graph_dense(W)
    got = gpu_ctx.knn_topn(off, items, ratings, 3, w_min=0.125, exclude=None)
    assert got.items.tolist() == [[2, 0, 1]] and got.scores.tolist() == [[0.125 + 2.0 ** -20, 0.0, 0.0]]
    got = gpu_ctx.knn_topn(off, items, ratings, 3, w_min=0.0, exclude=None)
    assert got.items.tolist() == [[2, 1, 0]] and got.scores.tolist() == [[0.125 + 2.0 ** -20, 0.125, 0.0]]


def test_nan_rating_gives_nan_scores_that_are_counted(gpu_ctx):
    rng = np.random.default_rng(21)
    n = 40
    W = random_graph(rng, n, 0.5)
    off, items, ratings = profiles([rng.choice(n, 6, replace=False), rng.choice(n, 4, replace=False)], rng)
    ratings[2] = np.nan
    gpu_ctx.upload_graph_dense(W)
    for mode in MODES:
        want = kr.topn(W, off, items, ratings, 12, mode=mode)
        assert want[3] > 0
        assert_same_bytes(gpu_ctx.knn_topn(off, items, ratings, 12, mode=mode), want)


def test_mean_mode_lists_the_predictions_of_knn_predict(gpu_ctx):
    rng = np.random.default_rng(33)
    n = 300
    W = random_graph(rng, n, 0.3)
    W[17, :] = np.float32(0.05)   # an item without a neighbour above 0.1
    lists = [np.sort(rng.choice(n, k, replace=False)) for k in (1, 2, 40, 120)] + [np.array([17, 40, 41])]
    off, items, ratings = profiles(lists, rng)
    gpu_ctx.upload_graph_dense(W)
    pred, _, _ = gpu_ctx.knn_predict(off, items, ratings)
    got = gpu_ctx.knn_topn(off, items, ratings, n, mode="mean", w_min=0.1, exclude=None)
    assert (got.count == n).all()
    listed = np.zeros(len(items))
    for u in range(len(lists)):
        pos = np.argsort(got.items[u])   # pos[i] = the place of item i in the list
        b, e = int(off[u]), int(off[u + 1])
        listed[b:e] = got.scores[u, pos[items[b:e]]]
    print("largest |listed - pred|:", float(np.abs(listed - pred).max()))
    assert np.array_equal(listed.view(np.uint64), pred.view(np.uint64))
    assert pred[int(off[4])] == 0.0 and pred[0] == 0.0   # no neighbour: 0 on both sides


# ---- ranking evaluation ---------------------------------------------------------------------------
def assert_rank_matches(got, want):
    rank, n_cand, users, s = want
    assert np.array_equal(got.rank, rank), (got.rank, rank)
    assert np.array_equal(got.n_cand, n_cand)
    for f in ("n_cand", "n_rel", "hits"):
        assert got.users[f].tolist() == [r[f] for r in users], f
    assert not got.users["reserved"].any()
    for f in ("precision", "recall", "ndcg", "ap", "rr", "auc"):
        ref = np.array([r[f] for r in users], dtype=np.float64)
        print(f, "largest difference", float(np.abs(got.users[f] - ref).max()))
    for f in kr.rr.MEAN_FIELDS:
        print(f, got.summary[f], s[f])
    for f in ("precision", "recall", "ndcg", "ap", "rr", "auc"):
        ref = np.array([r[f] for r in users], dtype=np.float64)
        assert np.array_equal(got.users[f].view(np.uint64), ref.view(np.uint64)), f
    for f in ("users_evaluated", "users_auc", "edges_counted", "edges_skipped", "n_nan_held"):
        assert got.summary[f] == s[f], (f, got.summary[f], s[f])
    for f in kr.rr.MEAN_FIELDS:
        assert np.float64(got.summary[f]).tobytes() == np.float64(s[f]).tobytes(), f


def test_rank_eval_matches_checker_and_lists(gpu_ctx):
    b = big_case()
    W, off, items, ratings, n = b["W"], b["off"], b["items"], b["ratings"], b["n"]
    n_users = len(off) - 1
    rng = np.random.default_rng(55)
    counts = [3, 0, 1, 17, 5, 16, 2, 33, 4]   # around the kRankT = 16 targets of a walk
    hu = np.concatenate([np.full(c, u) for u, c in enumerate(counts)])
    hi = np.concatenate([rng.choice(n, c, replace=False) for c in counts])
    start = np.cumsum([0] + counts)
    for u, c in enumerate(counts):   # hits below the cutoff: items of the checker's own top 7
        top = big_want("sum", 7)[0][u]
        hi[start[u]: start[u] + min(c, 2)] = top[[2, 5]][: min(c, 2)]
    hi[2] = items[int(off[3])]   # an item of another user's profile: a candidate for user 0
    hi[start[3] + 4] = items[int(off[3]) + 1]   # user 3's own profile item: excluded, skipped
    p = rng.permutation(len(hu))
    held = (hu[p].astype(np.uint32), hi[p].astype(np.uint32))
    weights = np.round(rng.random(len(hu)) * 4 + 1, 2)
    gpu_ctx.upload_graph_dense(W)
    for mode in MODES:
        want = kr.evaluate(W, off, items, ratings, 7, (held[0], held[1], weights), mode=mode)
        got = gpu_ctx.knn_rank_eval(off, items, ratings, 7, held, mode=mode, weights=weights)
        assert_rank_matches(got, want)
        assert got.summary["edges_skipped"] >= 1
    # the item at position p of a user's list has rank p
    lists = gpu_ctx.knn_topn(off, items, ratings, 50)
    lu = np.repeat(np.arange(n_users), lists.count.astype(np.int64))
    li = np.concatenate([lists.items[u, : lists.count[u]] for u in range(n_users)])
    got = gpu_ctx.knn_rank_eval(off, items, ratings, 7, (lu, li))
    assert got.rank.tolist() == [int(x) for u in range(n_users) for x in range(lists.count[u])]
    try:
        gpu_ctx.set_topn_block(2)
        again = gpu_ctx.knn_rank_eval(off, items, ratings, 7, (lu, li))
        assert again.stats.blocks == -(-n_users // 2)
        assert again.rank.tobytes() == got.rank.tobytes() and again.users.tobytes() == got.users.tobytes()
    finally:
        gpu_ctx.set_topn_block(0)


def test_rank_eval_skips_and_counts_nan_held_items(gpu_ctx):
    rng = np.random.default_rng(21)
    n = 40
    W = random_graph(rng, n, 0.5)
    off, items, ratings = profiles([rng.choice(n, 6, replace=False), rng.choice(n, 4, replace=False)], rng)
    ratings[2] = np.nan
    S = kr.score_matrix(W, off, items, ratings)
    nan_items = np.flatnonzero(np.isnan(S[0]) & ~np.isin(np.arange(n), items[:6]))
    fine = np.flatnonzero(~np.isnan(S[0]) & ~np.isin(np.arange(n), items[:6]))
    other = np.flatnonzero(~np.isin(np.arange(n), items[6:]))   # candidates of user 1
    assert len(nan_items) >= 2 and len(fine) >= 1 and not np.isnan(S[1]).any()
    held = (np.array([0, 0, 0, 0, 1]), np.array([nan_items[0], fine[0], nan_items[1], items[0], other[1]]))
    gpu_ctx.upload_graph_dense(W)
    want = kr.evaluate(W, off, items, ratings, 5, held)
    got = gpu_ctx.knn_rank_eval(off, items, ratings, 5, held)
    assert_rank_matches(got, want)
    assert got.summary["n_nan_held"] == 2 and got.summary["edges_skipped"] == 3
    assert got.rank[[0, 2, 3]].tolist() == [MAX, MAX, MAX]


# ---- arguments ------------------------------------------------------------------------------------
def raw_topn(ctx, nu, N, *, off=None, items=None, ratings=None, mode=0, w_min=0.1, eoff=None, eitem=None, n_sel=0,
             sel=None, out=None, null_off=False):
    off = np.zeros(nu + 1, np.uint64) if off is None else off
    items = np.zeros(1, np.uint32) if items is None else items
    ratings = np.zeros(max(len(items), 1), np.float32) if ratings is None else ratings
    n_out = nu if sel is None else n_sel
    o_items = np.full((max(n_out, 1), max(N, 1)), 12345, np.uint32)
    o_scores = np.full((max(n_out, 1), max(N, 1)), 5.5)
    count = np.full(max(n_out, 1), 77, np.uint32)
    st = _native.TopnStats()
    rc = ctx.lib.cf_knn_topn(ctx.h, nu, None if null_off else ptr(off), ptr(items), ptr(ratings), mode, w_min, ptr(eoff),
                             ptr(eitem), n_sel, ptr(sel), N, ptr(o_items), ptr(o_scores), ptr(count), ctypes.byref(st))
    if out is not None:
        out.update(items=o_items, scores=o_scores, count=count)
    return rc


def raw_rank(ctx, nu, N, *, off=None, items=None, mode=0, w_min=0.1, eoff=None, eitem=None, hoff=None, hitem=None,
             out=None):
    off = np.zeros(nu + 1, np.uint64) if off is None else off
    items = np.zeros(1, np.uint32) if items is None else items
    ratings = np.zeros(max(len(items), 1), np.float32)
    hoff_p = None if hoff is None else ptr(hoff)
    hitem = np.zeros(1, np.uint32) if hitem is None else hitem
    rank = np.full(max(len(hitem), 1), 4242, np.uint32)
    users = np.zeros(max(nu, 1), dtype=np.dtype([("raw", np.uint8, 64)]))
    users["raw"] = 9
    st = _native.RankSummary()
    rc = ctx.lib.cf_knn_rank_eval(ctx.h, nu, ptr(off), ptr(items), ptr(ratings), mode, w_min, ptr(eoff), ptr(eitem), hoff_p,
                                  ptr(hitem), None, N, ptr(rank), ptr(users), ctypes.byref(st))
    if out is not None:
        out.update(rank=rank, users=users, st=st)
    return rc


def test_argument_checks(gpu_ctx):
    ctx = gpu_ctx
    E, R = _native.CF_EINVAL, _native.CF_ERANGE
    ctx.upload_graph_dense(np.zeros((3, 3), np.float32))
    ok_off = np.array([0, 1, 2], np.uint64)
    ok_item = np.array([0, 2], np.uint32)
    assert raw_topn(ctx, 2, 1, off=ok_off, items=ok_item) == _native.CF_OK
    assert raw_topn(ctx, 2, 1, mode=2) == E and raw_topn(ctx, 2, 1, mode=-1) == E
    for bad in (-0.5, np.inf, np.nan):
        assert raw_topn(ctx, 2, 1, w_min=bad) == E
    assert raw_topn(ctx, 2, 0) == E
    assert raw_topn(ctx, 2, _native.CF_TOPN_MAX_N + 1) == R
    assert raw_topn(ctx, 2, _native.CF_TOPN_MAX_N) == _native.CF_OK
    assert raw_topn(ctx, 2, 1, null_off=True) == E
    assert raw_topn(ctx, 2, 1, off=np.array([1, 1, 2], np.uint64), items=ok_item) == E
    assert raw_topn(ctx, 2, 1, off=np.array([0, 2, 1], np.uint64), items=ok_item) == E
    assert raw_topn(ctx, 2, 1, off=ok_off, items=np.array([0, 3], np.uint32)) == E
    assert b"cf_knn_topn" in ctx.lib.cf_last_error(ctx.h)
    # the exclusion and selection errors of cf_mf_topn
    assert raw_topn(ctx, 2, 1, eoff=ok_off) == E
    assert raw_topn(ctx, 2, 1, eitem=ok_item) == E
    assert raw_topn(ctx, 2, 1, eoff=np.array([0, 2, 1], np.uint64), eitem=ok_item) == E
    assert raw_topn(ctx, 2, 1, eoff=ok_off, eitem=np.array([0, 3], np.uint32)) == E
    assert raw_topn(ctx, 2, 1, n_sel=2, sel=np.array([1, 2], np.uint32)) == E
    assert raw_topn(ctx, 2, 1, eoff=ok_off, eitem=ok_item, n_sel=2, sel=np.array([1, 0], np.uint32)) == _native.CF_OK
    # cf_knn_rank_eval: its own and the held-out errors of cf_mf_rank_eval
    h_off = np.array([0, 1, 2], np.uint64)
    assert raw_rank(ctx, 2, 1, hoff=h_off, hitem=np.array([1, 0], np.uint32)) == _native.CF_OK
    assert raw_rank(ctx, 2, 1, mode=5, hoff=h_off, hitem=ok_item) == E
    assert raw_rank(ctx, 2, 1, w_min=-1.0, hoff=h_off, hitem=ok_item) == E
    assert raw_rank(ctx, 2, 0, hoff=h_off, hitem=ok_item) == E
    assert raw_rank(ctx, 2, _native.CF_TOPN_MAX_N + 1, hoff=h_off, hitem=ok_item) == R
    assert raw_rank(ctx, 2, 1, off=ok_off, items=np.array([0, 3], np.uint32), hoff=h_off, hitem=ok_item) == E
    assert raw_rank(ctx, 2, 1) == E   # a null held_off
    assert b"cf_knn_rank_eval" in ctx.lib.cf_last_error(ctx.h)
    assert raw_rank(ctx, 2, 1, hoff=np.array([1, 1, 2], np.uint64), hitem=ok_item) == E
    assert raw_rank(ctx, 2, 1, hoff=np.array([0, 2, 1], np.uint64), hitem=ok_item) == E
    assert raw_rank(ctx, 2, 1, hoff=h_off, hitem=np.array([0, 3], np.uint32)) == E
    assert raw_rank(ctx, 2, 1, hoff=np.array([0, 2, 2], np.uint64), hitem=np.array([2, 2], np.uint32)) == E
    assert raw_rank(ctx, 2, 1, eoff=ok_off, hoff=h_off, hitem=ok_item) == E
    with pytest.raises(ValueError):
        ctx.knn_topn(ok_off, ok_item, np.ones(2, np.float32), 1, mode="median")
    with pytest.raises(ValueError):
        ctx.knn_topn(ok_off, ok_item, np.ones(2, np.float32), 1, exclude="everything")


def test_no_graph_is_a_state_error(gpu_ctx):
    with Context(0) as ctx:   # a context of its own: the shared one holds a graph
        assert raw_topn(ctx, 2, 1) == _native.CF_ESTATE
        assert b"cf_knn_topn: no item graph uploaded" in ctx.lib.cf_last_error(ctx.h)
        assert raw_rank(ctx, 2, 1, hoff=np.zeros(3, np.uint64)) == _native.CF_ESTATE
        assert b"cf_knn_rank_eval: no item graph uploaded" in ctx.lib.cf_last_error(ctx.h)


def test_empty_calls_write_zeros(gpu_ctx):
    ctx = gpu_ctx
    ctx.upload_graph_dense(np.zeros((5, 5), np.float32))
    out = {}
    assert raw_topn(ctx, 0, 2, out=out) == _native.CF_OK
    assert (out["items"] == 12345).all() and (out["scores"] == 5.5).all()
    assert raw_topn(ctx, 3, 2, n_sel=0, sel=np.array([0], np.uint32), out=out) == _native.CF_OK
    assert out["count"].tolist() == [77] and (out["items"] == 12345).all() and (out["scores"] == 5.5).all()
    r = ctx.knn_topn(np.zeros(1, np.uint64), np.zeros(0, np.uint32), np.zeros(0, np.float32), 3)
    assert r.items.shape == (0, 3) and r.count.shape == (0,)
    r = ctx.knn_topn(np.zeros(3, np.uint64), np.zeros(0, np.uint32), np.zeros(0, np.float32), 3, users=np.zeros(0, np.uint32))
    assert r.items.shape == (0, 3)
    # no users, and users without a held-out edge
    assert raw_rank(ctx, 0, 2, hoff=np.zeros(1, np.uint64), out=out) == _native.CF_OK
    assert out["st"].users_evaluated == 0 and (out["rank"] == 4242).all()
    assert raw_rank(ctx, 3, 2, hoff=np.zeros(4, np.uint64), out=out) == _native.CF_OK
    assert not out["users"]["raw"].any() and out["st"].edges_counted == 0 and out["st"].blocks == 0
    r = ctx.knn_rank_eval(np.zeros(3, np.uint64), np.zeros(0, np.uint32), np.zeros(0, np.float32), 3,
                          (np.zeros(0, np.uint32), np.zeros(0, np.uint32)))
    assert r.rank.shape == (0,) and r.summary["users_evaluated"] == 0 and len(r.users) == 2
