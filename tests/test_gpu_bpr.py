"""BPR on the GPU (cf_bpr_fit / cf_bpr_sample) against the numpy checker tests/bpr_ref.py.

The negatives are integers and are compared exactly, as are the triple and skip counts.
How the bounds of the fitted values were measured (tools/bpr_drift.py, CPU): the checker against
itself on these cases with every vertex's triples summed in a permuted order, the initial factors
perturbed by 1e-15 relative and every g moved by up to 2 ulp drifts by at most
1.25e-15 * max|F| in U and V (case N), 9.58e-16 * max|b| in the bias (case N) and 3.21e-15 of a
loss-trace entry (case N; the entry is a sum of positive terms, so it is its own scale).  The
bounds leave the about 300-fold margin test_gpu_als.py documents for another summation tree:
    factors  3.8e-13 * max|F|     bias  2.9e-13 * max|b|     loss  9.6e-13 * entry
The device's worst figures on one MI355X: 6.8e-16 (factors, case N), 3.5e-16 (bias, case D5) and
2.1e-15 (loss, case N)."""
import ctypes

import numpy as np
import pytest

import bpr_ref as br
from collaborative_filtering_amd import _native
from collaborative_filtering_amd._native import ptr

pytestmark = pytest.mark.gpu

FACTOR_BOUND = 3.8e-13
BIAS_BOUND = 2.9e-13
LOSS_BOUND = 9.6e-13
_FITS = {}


def device_fit(ctx, c: br.Case, **over):
    kw = dict(bias0=c.bias0, lr=c.lr, reg_user=c.reg, reg_item=c.reg, reg_bias=c.reg, n_sweeps=c.n_sweeps, seed=c.seed)
    kw.update(over)
    return ctx.bpr_fit(c.user, c.item, c.n_users, c.n_items, kw.pop("U0", c.U0), kw.pop("V0", c.V0), **kw)


def case_fit(ctx, name):
    """The device's run of a case, computed once and shared (not modified by the tests)."""
    if name not in _FITS:
        _FITS[name] = device_fit(ctx, br.case_inputs(name))
    return _FITS[name]


def same_bytes(a, b):
    return all((x is None and y is None) or x.tobytes() == y.tobytes()
               for x, y in ((a.U, b.U), (a.V, b.V), (a.bias_item, b.bias_item), (a.loss_trace, b.loss_trace)))


@pytest.mark.parametrize("seed", (5, 2**63 + 11))
@pytest.mark.parametrize("sweep", (0, 7))
@pytest.mark.parametrize("name", ("P", "M", "N"))
def test_sample_equals_checker(gpu_ctx, name, sweep, seed):
    c = br.case_inputs(name)
    want = br.sample(c.user, c.item, c.n_users, c.n_items, seed, sweep)
    # the pairs in another order: the python layer sorts them
    p = np.random.default_rng(1).permutation(len(c.user))
    got, skipped = gpu_ctx.bpr_sample(c.user[p], c.item[p], c.n_users, c.n_items, seed=seed, sweep=sweep)
    assert got.dtype == np.uint32 and np.array_equal(got, want)
    assert skipped == int((want == br.MAX).sum())


@pytest.mark.parametrize("name", br.CASES)
def test_case_matches_checker(gpu_ctx, name):
    c, ref, r = br.case_inputs(name), br.case_reference(name), case_fit(gpu_ctx, name)
    assert (r.sweeps, r.triples, r.n_skipped, r.n_nan) == (c.n_sweeps, ref.triples, ref.n_skipped, 0)
    for got, want in ((r.U, ref.U), (r.V, ref.V)):
        err = np.max(np.abs(got - want))
        print(name, "max|dF| / max|F|", err / np.max(np.abs(want)))
        assert err <= FACTOR_BOUND * np.max(np.abs(want))
    if c.bias0 is None:
        assert r.bias_item is None
    else:
        err = np.max(np.abs(r.bias_item - ref.bias))
        print(name, "max|db| / max|b|", err / np.max(np.abs(ref.bias)))
        assert err <= BIAS_BOUND * np.max(np.abs(ref.bias))
    assert r.loss_trace.shape == (c.n_sweeps, 2)
    assert np.array_equal(r.loss_trace[:, 1], ref.loss_trace[:, 1])          # triples per sweep, exactly
    err = np.abs(r.loss_trace[:, 0] - ref.loss_trace[:, 0]) / ref.loss_trace[:, 0]
    print(name, "loss error / entry", err.max())
    assert np.all(err <= LOSS_BOUND)
    # a vertex that never had a triple keeps its row bit for bit
    assert r.U[~ref.user_counted].tobytes() == c.U0[~ref.user_counted].tobytes()
    assert r.V[~ref.item_counted].tobytes() == c.V0[~ref.item_counted].tobytes()
    if c.bias0 is not None:
        assert r.bias_item[~ref.item_counted].tobytes() == c.bias0[~ref.item_counted].tobytes()
    assert r.U[ref.user_counted].tobytes() != c.U0[ref.user_counted].tobytes()
    assert r.stage_ms.shape == (6,) and r.sample_ms > 0 and r.reduce_ms > 0


def test_repeat_is_bit_identical(gpu_ctx):
    for name in ("P", "M", "N"):
        assert same_bytes(case_fit(gpu_ctx, name), device_fit(gpu_ctx, br.case_inputs(name))), name


@pytest.mark.parametrize("name", ("P", "N"))
def test_continued_fit_is_bit_identical(gpu_ctx, name):
    c = br.case_inputs(name)
    a = device_fit(gpu_ctx, c, n_sweeps=5)
    h = device_fit(gpu_ctx, c, n_sweeps=2)
    b = device_fit(gpu_ctx, c, n_sweeps=3, first_sweep=2, U0=h.U, V0=h.V, bias0=h.bias_item)
    assert a.U.tobytes() == b.U.tobytes() and a.V.tobytes() == b.V.tobytes()
    assert a.bias_item.tobytes() == b.bias_item.tobytes()
    assert a.loss_trace[:2].tobytes() == h.loss_trace.tobytes() and a.loss_trace[2:].tobytes() == b.loss_trace.tobytes()
    assert (a.triples, a.n_skipped) == (h.triples + b.triples, h.n_skipped + b.n_skipped)


def test_heavy_user_is_independent_of_other_users(gpu_ctx):
    """Case M's user 1 (above the segment length) refitted for one sweep with every other user's
    edges removed: its negatives, its own list and the item rows are unchanged, so its new row is
    the same bytes.  The other users' rows are not."""
    c = br.case_inputs("M")
    keep = c.user == 1
    assert keep.sum() > _native.load().cf_debug_als_segment()
    a = device_fit(gpu_ctx, c, n_sweeps=1, trace=False)
    b = gpu_ctx.bpr_fit(c.user[keep], c.item[keep], c.n_users, c.n_items, c.U0, c.V0, bias0=c.bias0, lr=c.lr, reg_user=c.reg,
                        reg_item=c.reg, reg_bias=c.reg, n_sweeps=1, seed=c.seed, trace=False)
    assert a.U[1].tobytes() == b.U[1].tobytes() and a.U[1].tobytes() != c.U0[1].tobytes()
    assert a.U[0].tobytes() != b.U[0].tobytes() and b.U[0].tobytes() == c.U0[0].tobytes()
    assert a.loss_trace.size == 0


def test_ranks_of_the_fitted_factors(gpu_ctx):
    """Device against checker on P through the existing rank evaluation: every positive pair ranked
    among all items, nothing excluded.  test_bpr_ref.py shows that no two scores of the checker's
    fit are closer than 1e-9, so the rank arrays are compared exactly, and the mean AUC with them."""
    c, ref, r = br.case_inputs("P"), br.case_reference("P"), case_fit(gpu_ctx, "P")
    want_auc, want_rank = br.train_auc(c, ref.U, ref.V, ref.bias)
    got = gpu_ctx.mf_rank_eval(r.U, r.V, 10, (c.user, c.item), bias_item=r.bias_item)
    print("AUC device", got.summary["auc"], "checker", want_auc)
    assert np.array_equal(got.rank, want_rank)
    assert abs(got.summary["auc"] - want_auc) <= 1e-9 and got.summary["auc"] > 0.95


def test_nan_ends_the_fit(gpu_ctx):
    c = br.case_inputs("D5")
    U0 = c.U0.copy()
    U0[3, 2] = np.nan
    r = device_fit(gpu_ctx, c, U0=U0)
    assert r.sweeps == 1 and r.n_nan == int((c.user == 3).sum()) - int((br.sample(c.user, c.item, c.n_users, c.n_items, c.seed, 0)[c.user == 3] == br.MAX).sum())
    assert r.loss_trace.shape == (1, 2) and np.isnan(r.loss_trace[0, 0])


def test_argument_checks(gpu_ctx):
    lib, h = gpu_ctx.lib, gpu_ctx.h
    u64, u32 = np.uint64, np.uint32

    def call(n_users, n_items, D, uoff, uitem, ioff, iuser, U=None, V=None, b=None, lr=0.5, reg=(0.01, 0.01, 0.01), n_sweeps=1,
             trace=None):
        U = np.ones((max(n_users, 1), max(D, 1))) if U is None else U
        V = np.ones((max(n_items, 1), max(D, 1))) if V is None else V
        par = _native.BprParams(lr, reg[0], reg[1], reg[2], 1, 0, n_sweeps)
        st = _native.BprStats()
        return lib.cf_bpr_fit(h, n_users, n_items, D, ptr(uoff), ptr(uitem), ptr(ioff), ptr(iuser), ctypes.byref(par),
                              ptr(U), ptr(V), ptr(b), ptr(trace), ctypes.byref(st)), st

    # two users, three items: user 0 rates items 0 and 2, user 1 item 2
    uoff, uitem = np.array([0, 2, 3], u64), np.array([0, 2, 2], u32)
    ioff, iuser = np.array([0, 1, 1, 3], u64), np.array([0, 0, 1], u32)
    g = (2, 3, 4, uoff, uitem, ioff, iuser)
    rc, st = call(*g)
    assert rc == _native.CF_OK and st.sweeps == 1 and st.triples + st.n_skipped == 3 and st.n_nan == 0
    assert call(2, 3, 65, uoff, uitem, ioff, iuser)[0] == _native.CF_ERANGE
    assert call(2, 3, 0, uoff, uitem, ioff, iuser)[0] == _native.CF_EINVAL
    for bad in (np.nan, np.inf, -np.inf):
        assert call(*g, lr=bad)[0] == _native.CF_EINVAL
        for k in range(3):
            reg = [0.01, 0.01, 0.01]
            reg[k] = bad
            assert call(*g, reg=reg)[0] == _native.CF_EINVAL
    for k in range(3):
        reg = [0.0, 0.0, 0.0]
        assert call(*g, reg=reg)[0] == _native.CF_OK
        reg[k] = -1e-3
        assert call(*g, reg=reg)[0] == _native.CF_EINVAL
    assert call(*g, lr=-0.5)[0] == _native.CF_OK                                                    # a descent step is the caller's business
    assert call(2, 3, 4, uoff, np.array([2, 0, 2], u32), ioff, iuser)[0] == _native.CF_EINVAL      # a user list that descends
    assert call(2, 3, 4, uoff, np.array([2, 2, 2], u32), ioff, iuser)[0] == _native.CF_EINVAL      # an edge twice
    assert call(2, 3, 4, uoff, uitem, ioff, np.array([0, 1, 0], u32))[0] == _native.CF_EINVAL      # an item list that descends
    assert call(2, 3, 4, uoff, uitem, ioff, np.array([1, 0, 1], u32))[0] == _native.CF_EINVAL      # not the transpose
    assert call(2, 3, 4, uoff, uitem, np.array([0, 1, 1, 2], u64), iuser)[0] == _native.CF_EINVAL  # edge totals differ
    assert call(2, 3, 4, uoff, uitem, np.array([0, 1, 2, 3], u64), iuser)[0] == _native.CF_EINVAL  # per-item counts differ
    assert call(2, 3, 4, uoff, np.array([0, 3, 2], u32), ioff, iuser)[0] == _native.CF_EINVAL      # item index out of range
    # n_sweeps = 0 leaves everything untouched
    U, V, b = np.arange(1.0, 9.0).reshape(2, 4), np.arange(1.0, 13.0).reshape(3, 4), np.arange(3.0)
    rc, st = call(*g, U=U, V=V, b=b, n_sweeps=0)
    assert rc == _native.CF_OK and st.sweeps == 0
    assert np.array_equal(U, np.arange(1.0, 9.0).reshape(2, 4)) and np.array_equal(V, np.arange(1.0, 13.0).reshape(3, 4))
    assert np.array_equal(b, np.arange(3.0))
    # an empty graph, no edges, an empty side: valid, nothing moves, the trace is zeros
    none = (np.zeros(1, u64), np.zeros(0, u32))
    assert call(0, 0, 4, *none, *none)[0] == _native.CF_OK
    U, V, trace = np.ones((2, 4)), np.ones((3, 4)), np.full(4, 7.0)
    rc, st = call(2, 3, 4, np.zeros(3, u64), np.zeros(0, u32), np.zeros(4, u64), np.zeros(0, u32), U=U, V=V, n_sweeps=2,
                  trace=trace)
    assert rc == _native.CF_OK and st.sweeps == 2 and st.triples == 0 and np.all(U == 1) and np.all(V == 1) and not np.any(trace)
    assert call(0, 3, 4, *none, np.zeros(4, u64), np.zeros(0, u32))[0] == _native.CF_OK
    assert call(2, 0, 4, np.zeros(3, u64), np.zeros(0, u32), *none)[0] == _native.CF_OK
    # the sampler's own checks
    neg, sk = np.zeros(3, u32), ctypes.c_uint64()
    assert lib.cf_bpr_sample(h, 2, 3, ptr(uoff), ptr(uitem), 1, 0, ptr(neg), ctypes.byref(sk)) == _native.CF_OK
    assert lib.cf_bpr_sample(h, 2, 3, ptr(uoff), ptr(np.array([2, 0, 2], u32)), 1, 0, ptr(neg), None) == _native.CF_EINVAL
    assert lib.cf_bpr_sample(h, 2, 2, ptr(uoff), ptr(uitem), 1, 0, ptr(neg), None) == _native.CF_EINVAL
    assert lib.cf_bpr_sample(h, 0, 0, ptr(none[0]), ptr(none[1]), 1, 0, None, ctypes.byref(sk)) == _native.CF_OK and sk.value == 0


def test_python_layer(gpu_ctx):
    r = gpu_ctx.bpr_fit([], [], 0, 0, np.zeros((0, 4)), np.zeros((0, 4)), n_sweeps=2)
    assert r.U.shape == (0, 4) and r.V.shape == (0, 4) and r.bias_item is None and r.triples == 0
    neg, skipped = gpu_ctx.bpr_sample([], [], 3, 4)
    assert neg.shape == (0,) and skipped == 0
    c = br.case_inputs("D5")
    with pytest.raises(ValueError):
        gpu_ctx.bpr_fit(np.append(c.user, c.user[0]), np.append(c.item, c.item[0]), c.n_users, c.n_items, c.U0, c.V0)
    with pytest.raises(ValueError):
        gpu_ctx.bpr_fit(c.user, c.item, c.n_users, c.n_items - 1, c.U0, c.V0[:-1])
    with pytest.raises(ValueError):
        gpu_ctx.bpr_fit(c.user, c.item, c.n_users, c.n_items, c.U0, c.V0, bias0=np.zeros(c.n_items + 1))
    with pytest.raises(ValueError):
        gpu_ctx.bpr_fit(c.user, c.item, c.n_users, c.n_items, c.U0, c.V0[:, :-1])
    with pytest.raises(ValueError):
        gpu_ctx.bpr_sample(np.append(c.user, c.user[0]), np.append(c.item, c.item[0]), c.n_users, c.n_items)
    with pytest.raises(_native.NativeError):
        device_fit(gpu_ctx, c, reg_item=-1.0)
    # the pairs in any order, and without a trace: the same factors
    p = np.random.default_rng(2).permutation(len(c.user))
    r = gpu_ctx.bpr_fit(c.user[p], c.item[p], c.n_users, c.n_items, c.U0, c.V0, bias0=c.bias0, lr=c.lr, reg_user=c.reg,
                        reg_item=c.reg, reg_bias=c.reg, n_sweeps=c.n_sweeps, seed=c.seed, trace=False)
    want = case_fit(gpu_ctx, "D5")
    assert r.loss_trace.size == 0 and r.U.tobytes() == want.U.tobytes() and r.V.tobytes() == want.V.tobytes()
    assert r.bias_item.tobytes() == want.bias_item.tobytes()
