"""The dense -> CSR compaction of the item graph (csrc/cf_graph.hip, cf_dense_to_csr) with its
optional top-K, and the CSR upload rules, where the kernels branch.

The unit under test is cf_dense_to_csr: its input is whatever dense matrix knn2 produced
(cf_item_cosine, pinned by test_gpu_knn.py) and the reference is numpy on that matrix, so every
comparison is of indices and float bits, with no tolerance.  Each test asserts on W first that the
matrix reaches the branch the test is named for."""
import numpy as np
import pytest

from test_gpu_knn import synth_train, topk_reference

pytestmark = pytest.mark.gpu

GT = 256                # kGT of cf_graph.hip: columns per trip of row_nnz / row_topk / row_compact_kernel
WAVE = 64               # lanes per ballot in row_compact_kernel
ROW_THREADS = 16        # most host threads cf_item_graph_upload's CSR path spreads the rows over
PLAIN_WIDTHS = [1, WAVE - 1, WAVE, WAVE + 1, GT - 1, GT, GT + 1, 2 * GT - 1, 2 * GT + 1, 600]


def bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def csr_of(W):
    """numpy's compaction of a dense matrix: (offsets, ascending columns, weights)."""
    r, c = np.nonzero(W)
    off = np.zeros(W.shape[0] + 1, np.uint64)
    off[1:] = np.cumsum(np.bincount(r, minlength=W.shape[0]))
    return off, c.astype(np.uint32), W[r, c]


# ---- plain compaction ----------------------------------------------------------------------------
def plain_ratings(n_items):
    """40 users, ratings 1..5.  Item 0 is rated by every user, item n_items // 2 by nobody, every
    other item by at least one user: row 0 then holds every column but its own and the empty
    item's, and row n_items // 2 is empty.  (W is symmetric -- knn2_store writes w(b, a) = w(a, b)
    -- so beside an empty row no row can hold all n - 1 other columns; n - 2 is the longest.)"""
    rng = np.random.default_rng(n_items)
    n_users = 40
    empty = n_items // 2 if n_items >= 3 else -1
    off, items, rats = [0], [], []
    for u in range(n_users):
        pick = rng.random(n_items) < 0.15
        pick[np.arange(n_items) % n_users == u] = True
        pick[0] = True
        if empty >= 0:
            pick[empty] = False
        its = np.nonzero(pick)[0]
        items += its.tolist()
        rats += rng.integers(1, 6, size=len(its)).tolist()
        off.append(len(items))
    return np.array(off, np.uint64), np.array(items, np.uint32), np.array(rats, np.float32), empty


@pytest.mark.parametrize("n_items", PLAIN_WIDTHS)
def test_plain_compaction_at_the_trip_edges(gpu_ctx, n_items):
    """Pins row_nnz_kernel's `j += kGT` count and row_compact_kernel's `j0 += kGT` loop with its
    `pos += all` carry at widths 1, 63 / 64 / 65 (one ballot and its neighbours), 255 / 256 / 257
    (one trip and one lane of a second), 511 / 513 and 600 (a third trip): offsets equal the
    bincount of the nonzero rows, columns ascend and equal np.nonzero, weights are the same bits.
    An empty row and a row with every possible column are asserted on W."""
    off, items, rats, empty = plain_ratings(n_items)
    W = gpu_ctx.item_cosine(n_items, off, items, rats, cnt_min=0)
    eoff, col, w = gpu_ctx.item_cosine_edges(n_items, off, items, rats, cnt_min=0)
    nnz_row = np.count_nonzero(W, axis=1)
    if n_items >= 3:
        assert nnz_row[empty] == 0 and not W[:, empty].any()
        assert nnz_row[0] == n_items - 2                       # every column but itself and the empty item's
        assert W[0, n_items - 1] != 0 and W[n_items - 1, 0] != 0   # the last lane of the last trip is live
        assert 0 < np.count_nonzero(W) < (n_items - 1) * (n_items - 1)
    else:
        assert not W.any()
    want_off, want_col, want_w = csr_of(W)
    assert np.array_equal(eoff, want_off)
    assert np.array_equal(col, want_col)
    assert np.array_equal(bits(w), bits(want_w))


# ---- top-K across column trips -------------------------------------------------------------------
TRIPLE_N, TRIPLE_BASE = 600, 200
TOPK_KS = [1, 2, 7, 100, 599, 600]


def tripled_ratings():
    """Profiles over 200 items, tripled: items j, j + 200 and j + 400 get identical rating
    columns, so every weight of a row appears three times, in columns 400 apart -- always in two
    or three different 256-column trips."""
    off, items, rats = synth_train(1500, TRIPLE_BASE, seed=31, kmax=40)
    k = np.diff(off.astype(np.int64))
    uo = np.concatenate([[0], np.cumsum(3 * k)]).astype(np.uint64)
    it3, rt3 = [], []
    for u in range(len(k)):
        b, e = int(off[u]), int(off[u + 1])
        it3.append(np.concatenate([items[b:e], items[b:e] + TRIPLE_BASE, items[b:e] + 2 * TRIPLE_BASE]))
        rt3.append(np.tile(rats[b:e], 3))
    return uo, np.concatenate(it3).astype(np.uint32), np.concatenate(rt3).astype(np.float32)


def cut_rows(W, K):
    """Rows whose K-th largest weight is tied, with ties in at least two 256-column trips, of
    which top-K takes some and not all: (such rows, rows where all ties are taken but lie in two
    trips)."""
    partial, whole = [], []
    for a in range(W.shape[0]):
        nz = np.nonzero(W[a])[0]
        if len(nz) <= K:
            continue
        v = np.sort(W[a, nz])[::-1][K - 1]
        ties = nz[W[a, nz] == v]
        taken = K - int((W[a, nz] > v).sum())
        if len(ties) > 1 and len(set((ties // GT).tolist())) >= 2:
            (partial if 0 < taken < len(ties) else whole).append(a)
    return partial, whole


@pytest.fixture(scope="module")
def tripled(gpu_ctx):
    uo, it3, rt3 = tripled_ratings()
    W = gpu_ctx.item_cosine(TRIPLE_N, uo, it3, rt3)
    W.setflags(write=False)
    return uo, it3, rt3, W


@pytest.mark.parametrize("K", TOPK_KS)
def test_topk_ties_across_column_trips(gpu_ctx, tripled, K):
    """n_items = 600 > 2 kGT.  Pins row_topk_kernel's histogram loop over `j += kGT` and
    row_compact_kernel's `ties += tall` carry: with the K-th value tied in two or three trips and
    only some of its ties taken, `trank < tk` is right only if the ties of earlier trips are
    counted.  K = 2 cuts exactly behind the two weights a row shares with its own copies (items
    a +- 200, a +- 400: all ties taken, in two trips, trank == tk - 1 at the last); K = 599 and
    600 are not below any row's length and take the `total <= K` branch."""
    uo, it3, rt3, W = tripled
    nnz_row = np.count_nonzero(W, axis=1)
    partial, whole = cut_rows(W, K)
    if K in (1, 7, 100):
        assert len(partial) >= 20, (K, len(partial))
    elif K == 2:
        assert len(whole) >= 20, (K, len(whole))
    else:
        assert GT < nnz_row.max() <= K                         # `total <= K` in every row, long ones too
    want = topk_reference(W, K)
    try:
        eg, cg, wg = gpu_ctx.item_cosine_edges(TRIPLE_N, uo, it3, rt3, topk=K)
    finally:
        gpu_ctx.lib.cf_set_knn2_topk(gpu_ctx.h, 0)
    assert np.array_equal(eg, want[0])
    assert np.array_equal(cg, want[1])
    assert np.array_equal(bits(wg), bits(want[2]))
    if K < 599:
        assert int(eg[-1]) < int(np.count_nonzero(W))          # the cap binds
        assert np.array_equal(np.diff(eg.astype(np.int64)), np.minimum(nnz_row, K))
    else:
        assert int(eg[-1]) == int(np.count_nonzero(W))         # K >= every row: everything kept


# ---- negative weights ----------------------------------------------------------------------------
NEG_N = 300
NEG_KS = [40, 100]      # rows of 41..80 entries, about half of them negative, end below zero at K = 40


def kth_values(W, K):
    """The K-th largest nonzero weight of every row with more than K nonzeros."""
    out = []
    for a in range(W.shape[0]):
        nz = W[a][W[a] != 0]
        if len(nz) > K:
            out.append(float(np.sort(nz)[::-1][K - 1]))
    return np.array(out)


@pytest.fixture(scope="module")
def signed(gpu_ctx):
    off, items, rats = synth_train(2000, NEG_N, seed=41, values=[-5, -4, -3, -2, -1, 1, 2, 3, 4, 5], kmax=40)
    rats = rats.astype(np.float32)
    W = gpu_ctx.item_cosine(NEG_N, off, items, rats, w_min=-1.0)
    W.setflags(write=False)
    return off, items, rats, W


@pytest.mark.parametrize("K", NEG_KS)
def test_topk_with_negative_weights(gpu_ctx, signed, K):
    """w_min = -1 keeps negative cosines.  Pins order_key's branch for a set sign bit (`~bits`):
    negative weights must rank below every positive one and among themselves by value, in
    row_topk_kernel's radix select and in row_compact_kernel's `key > T`.  Some row's K-th value
    is negative (the threshold key comes from the flipped branch) and some row's is positive."""
    off, items, rats, W = signed
    assert (W < 0).sum() >= 100 and (W > 0).sum() >= 100
    kth = kth_values(W, K)
    assert (kth < 0).any() and (kth > 0).any(), (K, (kth < 0).sum(), (kth > 0).sum())
    want = topk_reference(W, K)
    try:
        eg, cg, wg = gpu_ctx.item_cosine_edges(NEG_N, off, items, rats, w_min=-1.0, topk=K)
    finally:
        gpu_ctx.lib.cf_set_knn2_topk(gpu_ctx.h, 0)
    assert np.array_equal(eg, want[0])
    assert np.array_equal(cg, want[1])
    assert np.array_equal(bits(wg), bits(want[2]))
    assert int(eg[-1]) < int(np.count_nonzero(W))


def test_negative_weights_all_kept_without_topk(gpu_ctx, signed):
    """topk = 0: every nonzero of W, negative ones included (row_nnz_kernel's `!= 0.0f`)."""
    off, items, rats, W = signed
    eoff, col, w = gpu_ctx.item_cosine_edges(NEG_N, off, items, rats, w_min=-1.0, topk=0)
    want_off, want_col, want_w = csr_of(W)
    assert (want_w < 0).sum() >= 100
    assert np.array_equal(eoff, want_off) and np.array_equal(col, want_col)
    assert np.array_equal(bits(w), bits(want_w))


# ---- upload rules --------------------------------------------------------------------------------
def upload_case(n):
    """CSR input for n items and the dense W it means by last-assignment-wins
    (precompute_local_threads.cpp:284): row 0 holds a nonzero followed later by an explicit zero
    for the same column (the edge vanishes) and, for n > 1, a zero followed by a nonzero (the
    edge exists); the last row of n >= 3 is empty; the rest is random with repeats."""
    rng = np.random.default_rng(50 + n)
    W = np.zeros((n, n), np.float32)
    rp, cols, ws = [0], [], []
    for a in range(n):
        ent, lo = [], 0
        if a == 0:
            ent = [(0, 0.5), (0, 0.0)] if n == 1 else [(0, 0.5), (1, 0.0), (0, 0.0), (1, 0.25)]
            lo = 2                                   # the random entries of row 0 leave columns 0 and 1 alone
        if lo < n and not (n >= 3 and a == n - 1):
            for b in rng.integers(lo, n, size=min(2 * n, 30)):
                if b != a:                           # the diagonal stays empty, as knn2 leaves it
                    ent.append((int(b), 0.0 if rng.random() < 0.2 else float(np.float32(0.05 + rng.random()))))
        for b, v in ent:
            W[a, b] = v
        cols += [b for b, _ in ent]
        ws += [v for _, v in ent]
        rp.append(len(cols))
    return W, np.array(rp, np.uint64), np.array(cols, np.uint32), np.array(ws, np.float32)


@pytest.mark.parametrize("n", [1, 3, 40])
def test_csr_upload_rules(gpu_ctx, n):
    """cf_item_graph_upload's CSR path (stable sort by column, the last duplicate kept, zeros
    dropped, gaps closed) at n = 1 and 3, below the host's row-thread count (threads with empty
    row ranges), and at 40: the stored edge count is count_nonzero(W), and eigen blocks from the
    CSR graph are the bits of those from W uploaded dense."""
    from collaborative_filtering_amd.api import Context

    W, rp, cols, ws = upload_case(n)
    assert n < ROW_THREADS or n == 40
    assert W[0, 0] == 0.0 and (n == 1 or W[0, 1] == np.float32(0.25))
    assert n < 3 or (rp[n] == rp[n - 1] and not W[n - 1].any())
    assert n == 1 or 0 < np.count_nonzero(W) < len(cols)
    rng = np.random.default_rng(n)
    ks = [n] + [int(k) for k in rng.integers(1, n + 1, size=5)]
    uoff = np.concatenate([[0], np.cumsum(ks)]).astype(np.uint64)
    uitems = np.concatenate([np.sort(rng.choice(n, size=k, replace=False)) for k in ks]).astype(np.uint32)
    with Context(0) as d, Context(0) as c:
        d.set_graph_layout("dense")
        d.upload_graph_dense(W)
        c.set_graph_layout("csr")
        c.upload_graph_csr(n, rp, cols, ws)
        assert c.graph_info() == ("csr", n, int(np.count_nonzero(W)))
        ref, got = d.eigen_batch(uoff, uitems), c.eigen_batch(uoff, uitems)
        assert np.array_equal(got.m, ref.m)
        assert np.array_equal(bits(got.sigs), bits(ref.sigs))
        assert np.array_equal(bits(got.evals), bits(ref.evals))
        assert np.array_equal(bits(got.evecs), bits(ref.evecs))


@pytest.mark.parametrize("n", [1, WAVE + 1, GT - 1, GT, GT + 1, 2 * GT + 1])
def test_dense_adopt_compacts_any_matrix(gpu_ctx, n):
    """cf_dense_to_csr on a matrix knn2 cannot produce: a dense upload onto a CSR-layout context
    compacts W as given.  W holds -0.0 entries (absent for row_nnz_kernel's `!= 0.0f` and for
    row_compact_kernel's `v != 0.0f` alike: a count that kept them would shift every later row),
    an empty row, and a row with all n - 1 other columns (which a symmetric knn2 matrix cannot
    hold beside an empty row).  The stored edge count is numpy's count_nonzero, and the eigen
    blocks equal those of the dense layout."""
    from collaborative_filtering_amd.api import Context

    rng = np.random.default_rng(70 + n)
    W = np.where(rng.random((n, n)) < 0.4, rng.random((n, n)) + 0.05, 0.0).astype(np.float32)
    W = np.maximum(W, W.T)
    np.fill_diagonal(W, 0.0)
    W[rng.random((n, n)) < 0.1] = -0.0
    if n > 1:
        full = n // 3
        W[n // 2, :] = 0.0                                            # an empty row
        W[full, :] = 0.5 + np.arange(n, dtype=np.float32) / (2 * n)   # a row with every other column,
        W[full, full] = 0.0                                           # rows after both of them
        assert np.count_nonzero(W[full]) == n - 1 and np.count_nonzero(W[n // 2]) == 0 and full < n // 2 < n - 1
    else:
        W[0, 0] = -0.0
    assert np.signbit(W).sum() >= 1 and not (W < 0).any()
    assert np.count_nonzero(W) == int((W > 0).sum())                  # numpy: -0.0 is no entry
    ks = [min(n, 40)] + [int(k) for k in rng.integers(1, min(n, 40) + 1, size=4)]
    uoff = np.concatenate([[0], np.cumsum(ks)]).astype(np.uint64)
    uitems = np.concatenate([np.sort(rng.choice(n, size=k, replace=False)) for k in ks]).astype(np.uint32)
    with Context(0) as d, Context(0) as c:
        d.set_graph_layout("dense")
        d.upload_graph_dense(W)
        c.set_graph_layout("csr")
        c.upload_graph_dense(W)
        assert c.graph_info() == ("csr", n, int(np.count_nonzero(W)))
        ref, got = d.eigen_batch(uoff, uitems), c.eigen_batch(uoff, uitems)
        # values, not bits: the dense layout reads a -0.0 where the CSR one reads a missing edge
        # as +0.0, and the two may differ in the sign of an exact zero, nowhere else
        assert np.array_equal(got.m, ref.m)
        assert np.array_equal(got.sigs, ref.sigs, equal_nan=True)
        assert np.array_equal(got.evals, ref.evals, equal_nan=True)
        assert np.array_equal(got.evecs, ref.evecs, equal_nan=True)
