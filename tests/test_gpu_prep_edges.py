"""GPU data prep (csrc/cf_prep.hip) where its kernels branch: cf_knn_regroup on the constructed
cases of tests/prep_cases.py against the restatement oracle.cf_prep_oracle.knn_regroup, the
co-rated capacity contract, cf_fold_order at the key widths of bits_for, and the argument checks.

Every comparison is of integers or of copied float bits against numpy: no tolerance anywhere.
The CPU assertions that a case reaches the branch it is named for are in prep_cases.COVERAGE
(run without a GPU by tests/test_prep_cases.py, and here again before each device call)."""
import numpy as np
import pytest

import prep_cases as pc
from collaborative_filtering_amd import _native
from collaborative_filtering_amd._native import CF_EINVAL, CF_ERANGE, CF_OK, ptr

pytestmark = pytest.mark.gpu

SENTINEL = 0xFFFFFFFF
GRID_CAP = pc.GRID_CAP  # grid_for() of cf_prep.hip caps the element-wise kernels at 65536 blocks as well


@pytest.mark.parametrize("name", pc.NAMES)
def test_regroup_case_matches_restatement(gpu_ctx, name):
    """Pins, by case: wave_trips -- corated_bits_kernel's `b0 += 64` loop, a same-word segment
    over two trips (two atomicOr on one word) and the 32-lane suffix OR from an odd lane;
    row_chunks -- row_write_kernel's `w0 += kPrepThreads` loop and its `base += s_run` carry;
    many_users -- `u += gridDim.x` of corated_bits_kernel; many_movies -- `a += gridDim.x` of
    row_write_kernel (0.54 GB of bitmap scratch); roles_* -- ntr == 0 in regroup_split_kernel and
    one (user, movie) in both roles; one_run -- the stable sort and run_flag_kernel's last-of-run
    flag over a 200,000-long run; bit_edges_* -- the self bit and the first / last bit of a word."""
    case = pc.case(name)
    ref = pc.reference(name)
    pc.COVERAGE[name](case, ref)
    n_users, n_movies, user, movie, rating, validate = case
    g = gpu_ctx.knn_regroup(n_users, n_movies, user, movie, rating, validate)
    pc.assert_regroup_equal(g, ref)
    assert len(g["edg_movie"]) == sum(len(c) for c in ref[2])


def regroup_raw(ctx, case, edg, edg_cap):
    """cf_knn_regroup called directly: (rc, the three offset arrays); `edg` is written in place."""
    n_users, n_movies, user, movie, rating, validate = case
    n = len(user)
    offs = [np.full(n_movies + 1, 0xDEADBEEF, np.uint64) for _ in range(3)]
    tu, te = np.zeros(max(n, 1), np.uint32), np.zeros(max(n, 1), np.uint32)
    tr, ter = np.zeros(max(n, 1), np.float32), np.zeros(max(n, 1), np.float32)
    rc = ctx.lib.cf_knn_regroup(ctx.h, n, n_users, n_movies, ptr(user), ptr(movie), ptr(rating), ptr(validate),
                                ptr(offs[0]), ptr(tu), ptr(tr), ptr(offs[1]), ptr(te), ptr(ter), ptr(offs[2]),
                                ptr(edg), edg_cap)
    return rc, offs


def test_corated_capacity_contract(gpu_ctx):
    """CF_ERANGE with complete offsets (cf_prep.hip: "writes past cap are dropped; the offsets are
    complete regardless"): for edg_cap in {0, 1, need // 2, need - 1} the return is CF_ERANGE, the
    three offset arrays equal the restatement's, the first edg_cap entries are the prefix of the
    full list and every later entry of the caller's buffer keeps its sentinel; edg_cap = need
    gives CF_OK and the whole list.  Pins row_write_kernel's `if (o < cap)` and cf_knn_regroup's
    min(ne, edg_cap) copy."""
    case = pc.case("wave_trips")
    ref = pc.reference("wave_trips")
    want_off = pc.reference_offsets(ref)
    full = pc.reference_corated_flat(ref)
    need = len(full)
    assert need > 1000
    for cap in (0, 1, need // 2, need - 1):
        edg = np.full(need, SENTINEL, np.uint32)
        rc, offs = regroup_raw(gpu_ctx, case, edg, cap)
        assert rc == CF_ERANGE, (cap, rc)
        for got, want in zip(offs, want_off):
            assert np.array_equal(got, want), cap
        assert np.array_equal(edg[:cap], full[:cap]), cap
        assert np.all(edg[cap:] == SENTINEL), cap
    edg = np.full(need, SENTINEL, np.uint32)
    rc, offs = regroup_raw(gpu_ctx, case, edg, need)
    assert rc == CF_OK
    assert np.array_equal(offs[2], want_off[2]) and np.array_equal(edg, full)


def test_corated_capacity_on_the_device_buffer(gpu_ctx):
    """The same contract seen on the device: cf_knn_regroup_run writes into a device buffer of
    `need` entries prefilled with the sentinel while told edg_cap < need; entries from edg_cap on
    must keep the sentinel (row_write_kernel's `if (o < cap)` is the only guard of that buffer)."""
    import torch

    n_users, n_movies, user, movie, rating, validate = pc.case("wave_trips")
    ref = pc.reference("wave_trips")
    full = pc.reference_corated_flat(ref)
    need, n = len(full), len(user)
    T = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to("cuda:0")                      # noqa: E731
    Z = lambda k, dt: torch.zeros(k, dtype=dt, device="cuda:0")                               # noqa: E731
    d_user, d_movie = T(user.view(np.int32)), T(movie.view(np.int32))
    d_rat, d_val = T(rating), T(validate)
    for cap in (0, 1, need // 2, need - 1, need):
        offs = [Z(n_movies + 1, torch.int64) for _ in range(3)]
        tu, te = Z(n, torch.int32), Z(n, torch.int32)
        tr, ter = Z(n, torch.float32), Z(n, torch.float32)
        d_edg = torch.full((need,), -1, dtype=torch.int32, device="cuda:0")
        rc = gpu_ctx.lib.cf_knn_regroup_run(gpu_ctx.h, n, n_users, n_movies, ptr(d_user), ptr(d_movie), ptr(d_rat),
                                            ptr(d_val), ptr(offs[0]), ptr(tu), ptr(tr), ptr(offs[1]), ptr(te),
                                            ptr(ter), ptr(offs[2]), ptr(d_edg), cap, None)
        assert rc == CF_OK, (cap, rc)
        torch.cuda.synchronize()
        edg = d_edg.cpu().numpy().view(np.uint32)
        assert np.array_equal(edg[:cap], full[:cap]), cap
        assert np.all(edg[cap:] == SENTINEL), cap
        for got, want in zip(offs, pc.reference_offsets(ref)):
            assert np.array_equal(got.cpu().numpy().view(np.uint64), want), cap


# ---- cf_fold_order -------------------------------------------------------------------------------
def fold_reference(user, rank):
    return np.argsort(np.asarray(rank)[np.asarray(user, np.int64)], kind="stable").astype(np.uint32)


def bits_for(n):
    """cf_sort.h bits_for: bits to represent 0 .. n-1, at least 1."""
    b = 1
    while (1 << b) < n:
        b += 1
    return b


@pytest.mark.parametrize("n_users", [1, 2, 3, 256, 257, 65536, 65537])
def test_fold_order_at_key_widths(gpu_ctx, n_users):
    """bits_for at 1, 2^k and 2^k + 1 users: the sort reads exactly bits_for(n_users) key bits, so
    the largest rank n_users - 1 must fit them.  The users of rank 0 and of rank n_users - 1 both
    have ratings, scattered among the others: one bit too few would file the largest rank with
    rank n_users - 1 - 2^(bits-1)."""
    rng = np.random.default_rng(n_users)
    rank = rng.permutation(n_users).astype(np.uint32)
    n = 3000
    user = rng.integers(0, n_users, size=n).astype(np.uint32)
    first, last = int(np.argmin(rank)), int(np.argmax(rank))
    user[rng.choice(n, size=20, replace=False)] = np.repeat([first, last], 10)
    assert bits_for(n_users) == {1: 1, 2: 1, 3: 2, 256: 8, 257: 9, 65536: 16, 65537: 17}[n_users]
    assert int(rank[last]) == n_users - 1 and (n_users == 1 or (n_users - 1) >> (bits_for(n_users) - 1) == 1)
    assert (user == first).sum() >= 10 and (user == last).sum() >= 10
    order = gpu_ctx.fold_order(user, rank)
    assert np.array_equal(order, fold_reference(user, rank))


@pytest.mark.parametrize("n", [0, 1])
def test_fold_order_no_rating_and_one(gpu_ctx, n):
    """n = 0 (cf_fold_order_run's `if (n)`: no launch, no sort of an empty range) and n = 1."""
    rank = np.array([2, 0, 1], np.uint32)
    user = np.array([1], np.uint32)[:n]
    order = gpu_ctx.fold_order(user, rank)
    assert order.tolist() == list(range(n))


def test_fold_order_one_user_is_the_identity(gpu_ctx):
    """200,000 ratings of one user: all keys equal, the stable sort must return read order
    (fold_keys_kernel's idx through every merge level)."""
    n = 200_000
    rank = np.array([3, 1, 4, 0, 2], np.uint32)
    order = gpu_ctx.fold_order(np.full(n, 2, np.uint32), rank)
    assert np.array_equal(order, np.arange(n, dtype=np.uint32))


def test_fold_order_most_users_without_a_rating(gpu_ctx):
    """70,000 users of whom 40 have ratings (more ranks than ratings, more users than the
    65536-block cap of grid_for)."""
    rng = np.random.default_rng(8)
    n_users = 70_000
    assert n_users > GRID_CAP
    rank = rng.permutation(n_users).astype(np.uint32)
    active = rng.choice(n_users, size=40, replace=False)
    user = rng.choice(active, size=5000).astype(np.uint32)
    assert len(np.unique(user)) <= 40 < n_users // 1000
    order = gpu_ctx.fold_order(user, rank)
    assert np.array_equal(order, fold_reference(user, rank))


# ---- argument checks -----------------------------------------------------------------------------
def test_ids_out_of_range_are_refused(gpu_ctx):
    """A user id == n_users, a movie id == n_movies, and a rank array that is no permutation
    (a repeated rank; a rank == n_users) return CF_EINVAL before anything is allocated or
    written."""
    lib = _native.load()
    n_users, n_movies, user, movie, rating, validate = pc.case("roles_mixed")
    for which in ("user", "movie"):
        u, m = user.copy(), movie.copy()
        if which == "user":
            u[len(u) // 2] = n_users
        else:
            m[len(m) // 2] = n_movies
        edg = np.full(16, SENTINEL, np.uint32)
        rc, offs = regroup_raw(gpu_ctx, (n_users, n_movies, u, m, rating, validate), edg, 16)
        assert rc == CF_EINVAL, which
        assert b"out of range" in lib.cf_last_error(gpu_ctx.h)
        assert np.all(edg == SENTINEL) and all(np.all(o == 0xDEADBEEF) for o in offs)
    users = np.array([0, 1, 2, 1], np.uint32)
    for rank, ids in (([0, 1, 1], users), ([0, 3, 1], users), ([2, 0, 1], np.array([0, 3], np.uint32))):
        rank = np.array(rank, np.uint32)
        order = np.full(len(ids), SENTINEL, np.uint32)
        rc = lib.cf_fold_order(gpu_ctx.h, len(ids), 3, ptr(ids), ptr(rank), ptr(order))
        assert rc == CF_EINVAL, rank
        assert np.all(order == SENTINEL)
    order = gpu_ctx.fold_order(users, np.array([2, 0, 1], np.uint32))     # the context still works
    assert order.tolist() == [1, 3, 2, 0]
