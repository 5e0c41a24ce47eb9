"""EASE on the GPU (cf_ease_fit, cf_ease_gram, cf_ease_topn, cf_ease_rank_eval, ..) against the numpy
checker tests/ease_ref.py.

The Gram matrix and every score are compared byte for byte: the checker sums in the device's order
(users ascending for G; the profile's order, product rounded and then added, for a score).  The
inverse is compared through the standard first-order bounds of a backward-stable inversion, with
kappa_2 = numpy.linalg.cond(G) and n = n_items:
    max |G P - I| (formed in long double) <= n 2^-52 kappa_2
    max |B - B_ref|                       <= n 2^-52 kappa_2 max(1, max |B_ref|)
End-to-end lists and ranks are compared against the checker run on the B the GPU produced, which is
exact and cannot flip a near-tie between two inverses."""
import ctypes

import numpy as np
import pytest

import ease_ref as er
from collaborative_filtering_amd import _native
from collaborative_filtering_amd._native import ptr
from collaborative_filtering_amd.api import Context
from test_ease_ref import random_train
from test_gpu_knn_topn import assert_rank_matches, assert_same_bytes

pytestmark = pytest.mark.gpu

EPS = 2.0 ** -52
T = 256   # kAT, the threads of a workgroup (cf_mf_common.h)


def consts():
    """b (the inversion's block width), cols (items per workgroup of the score kernel), unroll."""
    lib = _native.load()
    b, cols, unroll = lib.cf_debug_ease_block(), lib.cf_debug_ease_cols(), lib.cf_debug_ease_unroll()
    assert b >= 4 and cols >= 4 and unroll >= 2
    return b, cols, unroll


def same_bytes(a, b):
    return a.shape == b.shape and np.array_equal(a.view(np.uint64), b.view(np.uint64))


# ---- Gram ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind,binary", [("int", False), ("half", False), ("float", False), ("float", True)])
def test_gram_bytes_and_symmetry(gpu_ctx, kind, binary):
    b, _, _ = consts()
    n = T + b + 7
    rng = np.random.default_rng(11)
    off, items, ratings = random_train(rng, 300, n, 0.05, kind, skip=3)   # item 3 has no edge
    lists = [items[int(off[u]):int(off[u + 1])] for u in range(300)]
    lists[0] = lists[0][:0]       # an empty user
    lists[1] = np.array([n - 1], np.uint32)   # a user with one item
    lists[2] = np.arange(n, dtype=np.uint32)[np.arange(n) != 3]   # a list longer than the workgroup has lanes
    off = np.cumsum([0] + [len(x) for x in lists]).astype(np.uint64)
    items = np.concatenate(lists).astype(np.uint32)
    ratings = np.resize(ratings, len(items)).astype(np.float32)
    want = er.gram(off, items, ratings, n, 0.3, binary)
    got = gpu_ctx.ease_gram(off, items, ratings, n, 0.3, binary=binary)
    assert same_bytes(got, want)
    assert same_bytes(got, np.ascontiguousarray(got.T))
    assert got[3, 3] == 0.3 and not np.delete(got[3], 3).any()
    # no users at all
    assert same_bytes(gpu_ctx.ease_gram(np.zeros(1, np.uint64), [], [], 5, 2.0), 2.0 * np.eye(5))


@pytest.mark.parametrize("nnz", [T, T + 1])
@pytest.mark.parametrize("n", [T - 1, T])
def test_gram_bytes_at_the_by_item_workgroup_edges(gpu_ctx, n, nnz):
    """The by-item lists come from T threads per workgroup, one per edge and one per offset (n + 1 of
    them): both counts at T and T + 1, items 0 and n - 1 without an edge."""
    rng = np.random.default_rng(12)
    flat = np.sort(rng.choice(200 * (n - 2), nnz, replace=False))
    off = np.searchsorted(flat // (n - 2), np.arange(201)).astype(np.uint64)
    items = (flat % (n - 2) + 1).astype(np.uint32)
    ratings = rng.integers(1, 6, nnz).astype(np.float32)
    want = er.gram(off, items, ratings, n, 0.3, False)
    assert want[0, 0] == 0.3 and want[n - 1, n - 1] == 0.3 and np.count_nonzero(np.diag(want) > 0.3) > n // 2
    assert same_bytes(gpu_ctx.ease_gram(off, items, ratings, n, 0.3), want)


# ---- fit accuracy ----------------------------------------------------------------------------------
FIT_SHAPES = ["one", "two", "b_minus_1", "b", "b_plus_1", "two_b_plus_3", "few_users", "few_users_binary"]


def fit_case(name):
    """Fewer users than items in the last two: lambda alone keeps G regular."""
    b, _, _ = consts()
    n, users, density, lam = {"one": (1, 40, 0.2, 5.0), "two": (2, 60, 0.2, 5.0), "b_minus_1": (b - 1, 100, 0.15, 5.0),
                              "b": (b, 200, 0.1, 5.0), "b_plus_1": (b + 1, 300, 0.05, 5.0),
                              "two_b_plus_3": (2 * b + 3, 400, 0.05, 5.0), "few_users": (2 * b + 2, 30, 0.1, 0.5),
                              "few_users_binary": (2 * b + 2, 30, 0.1, 0.5)}[name]
    rng = np.random.default_rng(100 + FIT_SHAPES.index(name))
    off, items, ratings = random_train(rng, users, n, density, "int")
    return n, lam, off, items, ratings


@pytest.mark.parametrize("name", FIT_SHAPES)
def test_fit_accuracy(gpu_ctx, name):
    n, lam, off, items, ratings = fit_case(name)
    binary = name == "few_users_binary"
    G =er.gram(off, items, ratings, n, lam, binary)
    kappa = float(np.linalg.cond(G))
    P = gpu_ctx.ease_inverse(off, items, ratings, n, lam, binary=binary)
    resid = np.abs(G.astype(np.longdouble) @ P.astype(np.longdouble) - np.eye(n, dtype=np.longdouble)).max()
    bound = n * EPS * kappa
    print(f"{name}: n = {n}, kappa = {kappa:.3g}, max|G P - I| = {float(resid):.3g}, bound {bound:.3g}")
    assert resid <= bound
    gpu_ctx.ease_fit(off, items, ratings, n, lam, binary=binary)
    B = gpu_ctx.ease_weights()
    assert B.shape == (n, n) and not np.diag(B).any()
    assert same_bytes(B, er.weights_from_inverse(P))   # the last stage is one division per entry
    B_ref = er.weights(G)
    err = np.abs(B - B_ref).max() if n else 0.0
    bbound = n * EPS * kappa * max(1.0, float(np.abs(B_ref).max()))
    print(f"{name}: max|B - B_ref| = {err:.3g}, bound {bbound:.3g}")
    assert err <= bbound
    ms = gpu_ctx.ease_timing()
    assert ms.shape == (3,) and (ms >= 0).all() and ms[0] > 0


def test_item_without_an_edge_gets_a_zero_row_and_column(gpu_ctx):
    b, _, _ = consts()
    n = b + 5
    rng = np.random.default_rng(7)
    off, items, ratings = random_train(rng, 150, n, 0.1, "half", skip=b)   # in the ragged last block
    gpu_ctx.ease_fit(off, items, ratings, n, 1.0)
    B = gpu_ctx.ease_weights()
    assert not B[b].any() and not B[:, b].any() and np.abs(B).max() > 0


def test_fit_is_repeatable(gpu_ctx):
    n1, lam1, off1, items1, ratings1 = fit_case("two_b_plus_3")
    n2, lam2, off2, items2, ratings2 = fit_case("b_plus_1")
    gpu_ctx.ease_fit(off1, items1, ratings1, n1, lam1)
    first = gpu_ctx.ease_weights()
    gpu_ctx.ease_fit(off1, items1, ratings1, n1, lam1)
    assert same_bytes(gpu_ctx.ease_weights(), first)
    gpu_ctx.ease_fit(off2, items2, ratings2, n2, lam2)
    assert gpu_ctx.ease_weights().shape == (n2, n2)
    gpu_ctx.release_workspaces()   # B is no workspace
    assert gpu_ctx.ease_weights().shape == (n2, n2)
    gpu_ctx.ease_fit(off1, items1, ratings1, n1, lam1)
    assert same_bytes(gpu_ctx.ease_weights(), first)


# ---- scoring bytes ---------------------------------------------------------------------------------
SCORE_SIZES = ["one", "cols_minus_1", "cols_plus_1", "two_cols_plus_5"]


def score_case(name):
    _, cols, unroll = consts()
    n = {"one": 1, "cols_minus_1": cols - 1, "cols_plus_1": cols + 1, "two_cols_plus_5": 2 * cols + 5}[name]
    rng = np.random.default_rng(300 + SCORE_SIZES.index(name))
    B = rng.normal(0.0, 1.0, (n, n))
    B[n // 2, n // 3] = np.nan
    lens = [0, 1, unroll - 1, unroll, unroll + 1, 2 * unroll + 1, 30] * 10   # 70 users
    lists = [rng.choice(n, min(k, n), replace=False) for k in lens]
    lists[8] = np.array([n // 2] * 3)   # the row of B with the NaN, three times: profiles need not ascend
    off = np.cumsum([0] + [len(x) for x in lists]).astype(np.uint64)
    items = np.concatenate(lists).astype(np.uint32)
    ratings = np.round(rng.normal(3.0, 1.5, len(items)), 2).astype(np.float32)
    if len(ratings) > 5:
        ratings[5] = np.nan
    return n, B, off, items, ratings


@pytest.mark.parametrize("name", SCORE_SIZES)
def test_scoring_bytes(gpu_ctx, name):
    n, B, off, items, ratings = score_case(name)
    n_users = len(off) - 1
    gpu_ctx.ease_upload(B)
    assert same_bytes(gpu_ctx.ease_weights(), B)
    for binary in (False, True):
        S = er.score_matrix(B, off, items, ratings, binary)
        for exclude in ("profile", None):
            mask = er._mask(B, off, items, exclude)
            for N in sorted({1, 7, min(n, 1024)}):
                want = er.tr.topn_from_scores(S, mask, N)
                got = gpu_ctx.ease_topn(off, items, ratings, N, binary=binary, exclude=exclude)
                assert_same_bytes(got, want)
                assert got.stats.blocks == 1
        if n > 1:
            assert want[3] > 0   # NaN scores were met and counted
    # the empty profile: every score 0, the lowest ids
    got = gpu_ctx.ease_topn(off, items, ratings, min(n, 9), exclude=None)
    assert got.items[0].tolist() == list(range(min(n, 9))) and not got.scores[0].any()
    # user blocks and a selection in no order: the same bytes
    S = er.score_matrix(B, off, items, ratings)
    mask = er._mask(B, off, items, "profile")
    want = er.tr.topn_from_scores(S, mask, 7)
    sel = np.array([69, 8, 0, 33, 8, 5], np.uint32)
    try:
        for ub in (1, 3, 65):
            gpu_ctx.set_topn_block(ub)
            got = gpu_ctx.ease_topn(off, items, ratings, 7)
            assert got.stats.blocks == -(-n_users // ub)
            assert_same_bytes(got, want)
            got = gpu_ctx.ease_topn(off, items, ratings, 7, users=sel)
            assert_same_bytes(got, (want[0][sel], want[1][sel], want[2][sel]))
    finally:
        gpu_ctx.set_topn_block(0)


def test_score_is_product_then_sum_in_profile_order(gpu_ctx):
    e = 2.0 ** -53
    B = np.zeros((3, 3))
    B[:, 0] = (1.0, e, e)
    B[0, 1], B[1, 1] = -3.0, 1.0 + 2 * e
    gpu_ctx.ease_upload(B)
    off = np.array([0, 3, 6, 8], np.uint64)
    items = np.array([0, 1, 2, 2, 1, 0, 0, 1], np.uint32)
    ratings = np.array([1, 1, 1, 1, 1, 1, 1, 3], np.float32)
    got = gpu_ctx.ease_topn(off, items, ratings, 3, exclude=None)
    score = {(u, int(i)): s for u in range(3) for i, s in zip(got.items[u], got.scores[u])}
    assert score[(0, 0)] == 1.0 and score[(1, 0)] == 1.0 + 2 * e
    assert score[(2, 1)] == 8 * e   # 3 (1 + 2 e) rounds to 3 + 8 e before -3 is added; an fma leaves 6 e


# ---- end to end ------------------------------------------------------------------------------------
def test_fit_then_lists_and_ranks_match_the_checker_on_the_device_b(gpu_ctx):
    b, _, _ = consts()
    n, n_users = 2 * b + 3, 120
    rng = np.random.default_rng(42)
    off, items, ratings = random_train(rng, n_users, n, 0.12, "half")
    gpu_ctx.ease_fit(off, items, ratings, n, 3.0)
    B = gpu_ctx.ease_weights()
    for binary in (False, True):
        assert_same_bytes(gpu_ctx.ease_topn(off, items, ratings, 10, binary=binary),
                          er.topn(B, off, items, ratings, 10, binary=binary))
    # a user who was not in the fit
    noff = np.array([0, 4], np.uint64)
    nit, nrat = np.array([5, 1, n - 1, 17], np.uint32), np.array([4.0, 2.5, 5.0, 1.0], np.float32)
    assert_same_bytes(gpu_ctx.ease_topn(noff, nit, nrat, 10), er.topn(B, noff, nit, nrat, 10))
    # held-out items: users with 0, 1 and several, one of them the user's own (excluded)
    counts = np.array([0, 1, 3, 17, 2] * (n_users // 5))
    hu = np.repeat(np.arange(n_users), counts)
    hi = np.concatenate([rng.choice(n, c, replace=False) for c in counts])
    assert off[3] > off[2]
    own = int(items[int(off[2])])
    hi[1:4] = [own, (own + 1) % n, (own + 2) % n]   # user 2: its own first item (excluded, skipped) and two more
    p =rng.permutation(len(hu))
    held = (hu[p].astype(np.uint32), hi[p].astype(np.uint32))
    weights = np.round(rng.random(len(hu)) * 4 + 1, 2)
    want = er.evaluate(B, off, items, ratings, 10, (held[0], held[1], weights))
    got = gpu_ctx.ease_rank_eval(off, items, ratings, 10, held, weights=weights)
    assert_rank_matches(got, want)
    assert got.summary["users_evaluated"] > 50 and got.summary["edges_skipped"] >= 1
    try:
        gpu_ctx.set_topn_block(7)
        again = gpu_ctx.ease_rank_eval(off, items, ratings, 10, held, weights=weights)
        assert again.rank.tobytes() == got.rank.tobytes() and again.users.tobytes() == got.users.tobytes()
    finally:
        gpu_ctx.set_topn_block(0)


# ---- state and errors ------------------------------------------------------------------------------
def raw_fit(ctx, nu, ni, *, off=None, items=None, obs=None, lam=1.0, null_off=False, null_items=False, fn="cf_ease_fit"):
    off = np.zeros(nu + 1, np.uint64) if off is None else off
    items = np.zeros(1, np.uint32) if items is None else items
    obs = np.ones(max(len(items), 1), np.float32) if obs is None else obs
    args = [ctx.h, nu, ni, None if null_off else ptr(off), None if null_items else ptr(items), ptr(obs), 0, lam]
    if fn == "cf_ease_fit":
        return ctx.lib.cf_ease_fit(*args)
    out = np.zeros(max(ni * ni, 1))
    return getattr(ctx.lib, fn)(*args, ptr(out))


def raw_topn(ctx, nu, N, *, off=None, items=None, eoff=None, eitem=None, n_sel=0, sel=None, out=None, null_off=False):
    off = np.zeros(nu + 1, np.uint64) if off is None else off
    items = np.zeros(1, np.uint32) if items is None else items
    ratings = np.zeros(max(len(items), 1), np.float32)
    n_out = nu if sel is None else n_sel
    o_items = np.full((max(n_out, 1), max(N, 1)), 12345, np.uint32)
    o_scores = np.full((max(n_out, 1), max(N, 1)), 5.5)
    count = np.full(max(n_out, 1), 77, np.uint32)
    st = _native.TopnStats()
    rc = ctx.lib.cf_ease_topn(ctx.h, nu, None if null_off else ptr(off), ptr(items), ptr(ratings), 0, ptr(eoff), ptr(eitem),
                              n_sel, ptr(sel), N, ptr(o_items), ptr(o_scores), ptr(count), ctypes.byref(st))
    if out is not None:
        out.update(items=o_items, scores=o_scores, count=count)
    return rc


def raw_rank(ctx, nu, N, *, off=None, items=None, eoff=None, eitem=None, hoff=None, hitem=None, out=None):
    off = np.zeros(nu + 1, np.uint64) if off is None else off
    items = np.zeros(1, np.uint32) if items is None else items
    ratings = np.zeros(max(len(items), 1), np.float32)
    hoff_p = None if hoff is None else ptr(hoff)
    hitem = np.zeros(1, np.uint32) if hitem is None else hitem
    rank = np.full(max(len(hitem), 1), 4242, np.uint32)
    users = np.zeros(max(nu, 1), dtype=np.dtype([("raw", np.uint8, 64)]))
    users["raw"] = 9
    st = _native.RankSummary()
    rc = ctx.lib.cf_ease_rank_eval(ctx.h, nu, ptr(off), ptr(items), ptr(ratings), 0, ptr(eoff), ptr(eitem), hoff_p,
                                   ptr(hitem), None, N, ptr(rank), ptr(users), ctypes.byref(st))
    if out is not None:
        out.update(rank=rank, users=users, st=st)
    return rc


def test_no_weights_is_a_state_error():
    with Context(0) as ctx:   # a context of its own: the shared one holds weights
        assert raw_topn(ctx, 2, 1) == _native.CF_ESTATE
        assert b"cf_ease_topn: no EASE weights resident" in ctx.lib.cf_last_error(ctx.h)
        assert raw_rank(ctx, 2, 1, hoff=np.zeros(3, np.uint64)) == _native.CF_ESTATE
        assert b"cf_ease_rank_eval" in ctx.lib.cf_last_error(ctx.h)
        n = ctypes.c_uint32(9)
        assert ctx.lib.cf_ease_weights(ctx.h, ctypes.byref(n), None) == _native.CF_ESTATE
        ms = ctx.ease_timing()
        assert not ms.any()
        # a fit over no items succeeds and leaves nothing resident
        assert raw_fit(ctx, 2, 0) == _native.CF_OK
        assert raw_topn(ctx, 2, 1) == _native.CF_ESTATE
        # a failed fit leaves nothing resident either
        ctx.ease_upload(np.eye(3))
        assert raw_fit(ctx, 1, 3, off=np.array([0, 2], np.uint64), items=np.array([1, 1], np.uint32)) == _native.CF_EINVAL
        assert ctx.ease_weights().shape == (3, 3)   # the checks run before the old weights go


def test_weights_and_graph_are_independent(gpu_ctx):
    import knn_topn_ref as kr

    rng = np.random.default_rng(13)
    n = 40
    W = (rng.random((n, n)) ** 2 * (rng.random((n, n)) < 0.5)).astype(np.float32)
    B = rng.normal(0, 1, (n + 3, n + 3))   # another item count than the graph's
    off, items, ratings = random_train(rng, 6, n, 0.2, "half")
    gpu_ctx.ease_upload(B)
    gpu_ctx.upload_graph_dense(W)
    want_knn = kr.topn(W, off, items, ratings, 5)
    want_ease = er.topn(B, off, items, ratings, 5)
    assert_same_bytes(gpu_ctx.knn_topn(off, items, ratings, 5), want_knn)
    assert_same_bytes(gpu_ctx.ease_topn(off, items, ratings, 5), want_ease)   # B survived the graph and knn_topn
    gpu_ctx.ease_fit(off, items, ratings, n, 2.0)
    assert gpu_ctx.ease_weights().shape == (n, n)
    assert_same_bytes(gpu_ctx.knn_topn(off, items, ratings, 5), want_knn)     # and the reverse


def test_argument_checks(gpu_ctx):
    ctx = gpu_ctx
    E, R, OK = _native.CF_EINVAL, _native.CF_ERANGE, _native.CF_OK
    ok_off = np.array([0, 1, 3], np.uint64)
    ok_item = np.array([0, 1, 2], np.uint32)
    for fn in ("cf_ease_fit", "cf_ease_gram", "cf_debug_ease_inverse"):
        assert raw_fit(ctx, 2, 3, off=ok_off, items=ok_item, fn=fn) == OK
        for bad in (0.0, -1.0, np.inf, np.nan):
            assert raw_fit(ctx, 2, 3, off=ok_off, items=ok_item, lam=bad, fn=fn) == E
        assert raw_fit(ctx, 2, 3, null_off=True, fn=fn) == E
        assert raw_fit(ctx, 2, 3, off=ok_off, items=ok_item, null_items=True, fn=fn) == E
        assert raw_fit(ctx, 2, 3, off=np.array([1, 1, 3], np.uint64), items=ok_item, fn=fn) == E
        assert raw_fit(ctx, 2, 3, off=np.array([0, 3, 1], np.uint64), items=ok_item, fn=fn) == E
        assert raw_fit(ctx, 2, 3, off=ok_off, items=np.array([0, 1, 3], np.uint32), fn=fn) == E
        assert raw_fit(ctx, 2, 3, off=ok_off, items=np.array([0, 2, 1], np.uint32), fn=fn) == E   # descending
        assert raw_fit(ctx, 2, 3, off=ok_off, items=np.array([0, 1, 1], np.uint32), fn=fn) == E   # listed twice
        assert fn.encode() in ctx.lib.cf_last_error(ctx.h)
        assert raw_fit(ctx, 0, (1 << 24) + 1, fn="cf_ease_fit") == R
    assert raw_fit(ctx, 0, 4) == OK and np.array_equal(ctx.ease_weights(), np.zeros((4, 4)))   # no users: G = lam I
    assert ctx.lib.cf_ease_upload(ctx.h, 0, ptr(np.zeros(1))) == E
    assert ctx.lib.cf_ease_upload(ctx.h, 3, None) == E
    assert ctx.lib.cf_ease_upload(ctx.h, (1 << 24) + 1, ptr(np.zeros(1))) == R
    assert ctx.lib.cf_ease_timing(ctx.h, None) == E
    with pytest.raises(ValueError):
        ctx.ease_upload(np.zeros((2, 3)))
    # scoring: its own errors, then those of the mf calls
    ctx.ease_upload(np.zeros((3, 3)))
    p_off = np.array([0, 1, 2], np.uint64)
    p_item = np.array([2, 0], np.uint32)   # a profile need not ascend
    assert raw_topn(ctx, 2, 1, off=p_off, items=p_item) == OK
    assert raw_topn(ctx, 2, 0) == E
    assert raw_topn(ctx, 2, _native.CF_TOPN_MAX_N + 1) == R
    assert raw_topn(ctx, 2, _native.CF_TOPN_MAX_N) == OK
    assert raw_topn(ctx, 2, 1, null_off=True) == E
    assert raw_topn(ctx, 2, 1, off=np.array([1, 1, 2], np.uint64), items=p_item) == E
    assert raw_topn(ctx, 2, 1, off=np.array([0, 2, 1], np.uint64), items=p_item) == E
    assert raw_topn(ctx, 2, 1, off=p_off, items=np.array([0, 3], np.uint32)) == E
    assert b"cf_ease_topn" in ctx.lib.cf_last_error(ctx.h)
    assert raw_topn(ctx, 2, 1, eoff=p_off) == E
    assert raw_topn(ctx, 2, 1, eitem=p_item) == E
    assert raw_topn(ctx, 2, 1, eoff=np.array([0, 2, 1], np.uint64), eitem=p_item) == E
    assert raw_topn(ctx, 2, 1, eoff=p_off, eitem=np.array([0, 3], np.uint32)) == E
    assert raw_topn(ctx, 2, 1, n_sel=2, sel=np.array([1, 2], np.uint32)) == E
    assert raw_topn(ctx, 2, 1, eoff=p_off, eitem=p_item, n_sel=2, sel=np.array([1, 0], np.uint32)) == OK
    h_off = np.array([0, 1, 2], np.uint64)
    assert raw_rank(ctx, 2, 1, hoff=h_off, hitem=np.array([1, 0], np.uint32)) == OK
    assert raw_rank(ctx, 2, 0, hoff=h_off, hitem=p_item) == E
    assert raw_rank(ctx, 2, _native.CF_TOPN_MAX_N + 1, hoff=h_off, hitem=p_item) == R
    assert raw_rank(ctx, 2, 1, off=p_off, items=np.array([0, 3], np.uint32), hoff=h_off, hitem=p_item) == E
    assert raw_rank(ctx, 2, 1) == E   # a null held_off
    assert b"cf_ease_rank_eval" in ctx.lib.cf_last_error(ctx.h)
    assert raw_rank(ctx, 2, 1, hoff=np.array([1, 1, 2], np.uint64), hitem=p_item) == E
    assert raw_rank(ctx, 2, 1, hoff=np.array([0, 2, 1], np.uint64), hitem=p_item) == E
    assert raw_rank(ctx, 2, 1, hoff=h_off, hitem=np.array([0, 3], np.uint32)) == E
    assert raw_rank(ctx, 2, 1, hoff=np.array([0, 2, 2], np.uint64), hitem=np.array([2, 2], np.uint32)) == E
    assert raw_rank(ctx, 2, 1, eoff=p_off, hoff=h_off, hitem=p_item) == E
    with pytest.raises(ValueError):
        ctx.ease_topn(p_off, p_item, np.ones(2, np.float32), 1, exclude="everything")


def test_empty_calls_write_zeros(gpu_ctx):
    ctx = gpu_ctx
    ctx.ease_upload(np.zeros((5, 5)))
    out = {}
    assert raw_topn(ctx, 0, 2, out=out) == _native.CF_OK
    assert (out["items"] == 12345).all() and (out["scores"] == 5.5).all()
    assert raw_topn(ctx, 3, 2, n_sel=0, sel=np.array([0], np.uint32), out=out) == _native.CF_OK
    assert out["count"].tolist() == [77] and (out["items"] == 12345).all()
    r = ctx.ease_topn(np.zeros(1, np.uint64), np.zeros(0, np.uint32), np.zeros(0, np.float32), 3)
    assert r.items.shape == (0, 3) and r.count.shape == (0,)
    assert raw_rank(ctx, 0, 2, hoff=np.zeros(1, np.uint64), out=out) == _native.CF_OK
    assert out["st"].users_evaluated == 0 and (out["rank"] == 4242).all()
    assert raw_rank(ctx, 3, 2, hoff=np.zeros(4, np.uint64), out=out) == _native.CF_OK
    assert not out["users"]["raw"].any() and out["st"].edges_counted == 0 and out["st"].blocks == 0
    r = ctx.ease_rank_eval(np.zeros(3, np.uint64), np.zeros(0, np.uint32), np.zeros(0, np.float32), 3,
                           (np.zeros(0, np.uint32), np.zeros(0, np.uint32)))
    assert r.rank.shape == (0,) and r.summary["users_evaluated"] == 0
    assert ctx.ease_gram(np.zeros(1, np.uint64), [], [], 0, 1.0).shape == (0, 0)
