"""KL-divergence NMF on the GPU (cf_nmf_fit / cf_nmf_loss / cf_mf_colsum) against the dense numpy
checker tests/nmf_ref.py, which forms the whole grid and does not use the column-sum trick.

How the bounds were measured (tools/nmf_drift.py, CPU): the checker against itself on these cases
with the edge order permuted and the initial factors perturbed by 1e-15 relative drifts by at most
2.76e-15 * max|factor| in the factors (case D32, grid) and 1.47e-16 * loss_scale in a loss-trace
entry (case S, grid; loss_scale is the sum of the absolute values of the loss terms); numpy's
column sum against itself with the rows permuted and perturbed drifts by 2.08e-14 of sum |F|
(1 to 40,961 rows).  The bounds leave the about 300-fold margin test_gpu_als.py documents for
another summation tree:
    factors  8.3e-13 * max|factor|     loss  4.4e-14 * loss_scale     column sum  6.2e-12 * sum |F|
n_floored is compared exactly: test_nmf_ref.py shows that no case produces a value within a factor
2 of the floor.  The device's worst figures on one MI355X: 2.4e-15, 1.7e-16 and 1.4e-14."""
import ctypes

import numpy as np
import pytest

import nmf_ref as nr
from collaborative_filtering_amd import _native
from collaborative_filtering_amd._native import ptr

pytestmark = pytest.mark.gpu

FACTOR_BOUND = 8.3e-13
LOSS_BOUND = 4.4e-14
COLSUM_BOUND = 6.2e-12
_FITS = {}


def device_fit(ctx, c: nr.Case, mode, **over):
    kw = dict(mode=mode, n_sweeps=c.n_sweeps)
    kw.update(over)
    return ctx.nmf_fit(c.user, c.item, c.obs, c.n_users, c.n_items, c.U0, c.V0, **kw)


def case_fit(ctx, name, mode):
    """The device's run of a case, computed once and shared (not modified by the tests)."""
    if (name, mode) not in _FITS:
        _FITS[name, mode] = device_fit(ctx, nr.case_inputs(name), mode)
    return _FITS[name, mode]


@pytest.mark.parametrize("mode", nr.MODES)
@pytest.mark.parametrize("name", nr.CASES)
def test_case_matches_checker(gpu_ctx, name, mode):
    c, ref, r = nr.case_inputs(name), nr.case_reference(name, mode), case_fit(gpu_ctx, name, mode)
    assert r.sweeps == c.n_sweeps
    for got, want in ((r.U, ref.U), (r.V, ref.V)):
        err = np.max(np.abs(got - want))
        print(name, mode, "max|dF|", err, "max|F|", np.max(np.abs(want)))
        assert err <= FACTOR_BOUND * np.max(np.abs(want))
    err = np.abs(r.loss_trace - ref.loss_trace) / ref.loss_scale
    print(name, mode, "loss", r.loss_trace, "error / loss_scale", err, "floored", r.n_floored)
    assert r.loss_trace.shape == (2 * c.n_sweeps,) and np.all(err <= LOSS_BOUND)
    assert r.n_floored == ref.n_floored
    # the device trace decreases wherever the checker's does by more than rounding
    strict = -np.diff(ref.loss_trace) / np.abs(ref.loss_trace[:-1]) >= 1e-6
    assert np.all(np.diff(r.loss_trace)[strict] < 0)
    # vertices without edges: untouched (observed), the floor exactly (grid)
    n_empty = 0
    for F, F0, idx, n in ((r.U, c.U0, c.user, c.n_users), (r.V, c.V0, c.item, c.n_items)):
        empty = np.bincount(idx, minlength=n) == 0
        n_empty += int(empty.sum())
        want = F0[empty] if mode == nr.OBSERVED else np.full((int(empty.sum()), c.D), nr.EPS)
        assert F[empty].tobytes() == np.ascontiguousarray(want, dtype=np.float64).tobytes()
    assert n_empty > 0 or name.startswith("D")     # A, B, H and S hold such vertices
    # the loss the fit traced last is the loss of the factors it returned
    got = gpu_ctx.nmf_loss(c.user, c.item, c.obs, c.n_users, c.n_items, r.U, r.V, mode=mode)
    assert np.float64(got).tobytes() == r.loss_trace[-1].tobytes()


@pytest.mark.parametrize("mode", nr.MODES)
def test_repeat_is_bit_identical(gpu_ctx, mode):
    for name in ("A", "H"):
        a, b = case_fit(gpu_ctx, name, mode), device_fit(gpu_ctx, nr.case_inputs(name), mode)
        for x, y in ((a.U, b.U), (a.V, b.V), (a.loss_trace, b.loss_trace)):
            assert x.tobytes() == y.tobytes()
        assert a.n_floored == b.n_floored


@pytest.mark.parametrize("mode", nr.MODES)
def test_loss_of_any_factors(gpu_ctx, mode):
    c, r = nr.case_inputs("B"), case_fit(gpu_ctx, "B", mode)
    rng = np.random.default_rng(2)
    # the fitted factors hold components at the floor: they are only ever scaled up here
    for U, V in ((c.U0, c.V0), (3.0 * r.U, r.V), (r.U * (1 + 0.1 * rng.uniform(0, 1, r.U.shape)), 1.5 * r.V)):
        want, scale = nr.loss(c.user, c.item, c.obs, c.n_users, c.n_items, U, V, mode)
        got = gpu_ctx.nmf_loss(c.user, c.item, c.obs, c.n_users, c.n_items, U, V, mode=mode)
        print(mode, "loss", got, want, abs(got - want) / scale)
        assert abs(got - want) <= LOSS_BOUND * scale
        again = gpu_ctx.nmf_loss(c.user, c.item, c.obs, c.n_users, c.n_items, U, V, mode=mode)
        assert np.float64(got).tobytes() == np.float64(again).tobytes()


@pytest.mark.parametrize("mode", nr.MODES)
def test_heavy_item_is_independent_of_other_vertices(gpu_ctx, mode):
    """Case H's item 0 (above the segment length) with the edges of every other item removed: its
    own edge list and the users' rows are unchanged, and so is the users' column sum (the other
    items stay as vertices), so its new row is the same bytes.  The sides are swapped (items passed
    as the first side) so that the heavy vertex is updated in the first half-sweep, straight from
    the initial factors."""
    c = nr.case_inputs("H")
    keep = c.item == 0
    assert keep.sum() > _native.load().cf_debug_als_segment()
    a = gpu_ctx.nmf_fit(c.item, c.user, c.obs, c.n_items, c.n_users, c.V0, c.U0, mode=mode, n_sweeps=1, trace=False)
    b = gpu_ctx.nmf_fit(c.item[keep], c.user[keep], c.obs[keep], c.n_items, c.n_users, c.V0, c.U0, mode=mode, n_sweeps=1,
                        trace=False)
    assert a.U[0].tobytes() == b.U[0].tobytes() and a.U[0].tobytes() != c.V0[0].tobytes()
    assert a.U[1:7].tobytes() != b.U[1:7].tobytes()       # the other items did change


def test_colsum(gpu_ctx):
    R = _native.load().cf_debug_nmf_sum_rows()
    rng = np.random.default_rng(6)
    worst = 0.0
    for n in (1, R - 1, R, R + 1, 2 * R + 3, 40 * R + 1):   # the last: more slices than the slice-order sum loads ahead
        for D in (1, 5, 33, 64):
            F = rng.uniform(0, 1, (n, D))   # non-negative, as the factors are (and as tools/nmf_drift.py measures)
            s = gpu_ctx.mf_colsum(F)
            scale = np.abs(F).sum(0)
            worst = max(worst, float(np.max(np.abs(s - F.sum(0)) / scale)))
            assert np.all(np.abs(s - F.sum(0)) <= COLSUM_BOUND * scale), (n, D)
            assert gpu_ctx.mf_colsum(F).tobytes() == s.tobytes(), (n, D)            # the same bytes on repeat
            if n == R + 1:   # rows of zeros appended to the last slice and as new slices change nothing
                assert gpu_ctx.mf_colsum(np.vstack([F, np.zeros((R + 7, D))])).tobytes() == s.tobytes(), D
    print("worst column-sum error relative to sum |F|", worst)
    s = gpu_ctx.mf_colsum(np.zeros((0, 4)))
    assert s.shape == (4,) and not np.any(s)


def test_argument_checks(gpu_ctx):
    lib, h = gpu_ctx.lib, gpu_ctx.h
    u64, u32, f32 = np.uint64, np.uint32, np.float32

    def call(n_users, n_items, D, uoff, uitem, ioff, iuser, obs=None, mode=_native.CF_NMF_GRID, n_sweeps=1, U=None, V=None):
        nnz = len(uitem)
        obs = np.full(max(nnz, 1), 2.0, f32) if obs is None else obs
        U = np.ones((max(n_users, 1), max(D, 1))) if U is None else U
        V = np.ones((max(n_items, 1), max(D, 1))) if V is None else V
        st = _native.NmfStats()
        return lib.cf_nmf_fit(h, n_users, n_items, D, ptr(uoff), ptr(uitem), ptr(obs), ptr(ioff), ptr(iuser), ptr(obs),
                              mode, n_sweeps, ptr(U), ptr(V), None, ctypes.byref(st)), st

    uoff, uitem = np.array([0, 1, 2], u64), np.array([0, 0], u32)
    ioff, iuser = np.array([0, 2], u64), np.array([0, 1], u32)
    g = (2, 1, 4, uoff, uitem, ioff, iuser)
    for mode in (_native.CF_NMF_GRID, _native.CF_NMF_OBSERVED):
        rc, st = call(*g, mode=mode)
        assert rc == _native.CF_OK and st.sweeps == 1 and st.n_floored == 0 and st.loss_ms == 0.0
    assert call(2, 1, 65, uoff, uitem, ioff, iuser)[0] == _native.CF_ERANGE
    assert call(2, 1, 0, uoff, uitem, ioff, iuser)[0] == _native.CF_EINVAL
    assert call(*g, mode=2)[0] == _native.CF_EINVAL and call(*g, mode=-1)[0] == _native.CF_EINVAL
    assert call(*g, obs=np.array([2.0, -0.5], f32))[0] == _native.CF_EINVAL
    assert call(*g, obs=np.array([np.nan, 2.0], f32))[0] == _native.CF_EINVAL
    assert call(*g, obs=np.array([np.inf, 2.0], f32))[0] == _native.CF_EINVAL
    assert call(*g, obs=np.array([0.0, 2.0], f32))[0] == _native.CF_OK                            # a zero rating is fine
    for bad in (0.0, 0.5e-16, -1.0, np.nan, np.inf):
        U = np.ones((2, 4))
        U[1, 2] = bad
        assert call(*g, U=U)[0] == _native.CF_EINVAL, bad
        V = np.ones((1, 4))
        V[0, 3] = bad
        assert call(*g, V=V)[0] == _native.CF_EINVAL, bad
    assert call(*g, U=np.full((2, 4), nr.EPS))[0] == _native.CF_OK                                # the floor itself
    assert call(2, 1, 4, uoff, uitem, np.array([0, 1], u64), iuser)[0] == _native.CF_EINVAL       # edge totals differ
    assert call(2, 2, 4, uoff, uitem, np.array([0, 1, 2], u64), iuser)[0] == _native.CF_EINVAL    # per-item counts differ
    # n_sweeps = 0 leaves U and V untouched
    U, V = np.arange(1.0, 9.0).reshape(2, 4), np.arange(1.0, 5.0).reshape(1, 4)
    rc, st = call(*g, n_sweeps=0, U=U, V=V)
    assert rc == _native.CF_OK and st.sweeps == 0
    assert np.array_equal(U, np.arange(1.0, 9.0).reshape(2, 4)) and np.array_equal(V, np.arange(1.0, 5.0).reshape(1, 4))
    # an empty graph, no edges, an empty side
    none = (np.zeros(1, u64), np.zeros(0, u32))
    assert call(0, 0, 4, *none, *none)[0] == _native.CF_OK
    for mode, want in ((_native.CF_NMF_OBSERVED, 1.0), (_native.CF_NMF_GRID, nr.EPS)):
        U, V = np.ones((2, 4)), np.ones((1, 4))
        rc, st = call(2, 1, 4, np.zeros(3, u64), np.zeros(0, u32), np.zeros(2, u64), np.zeros(0, u32), mode=mode, U=U, V=V)
        assert rc == _native.CF_OK and st.sweeps == 1 and np.all(U == want) and np.all(V == want)
        assert st.n_floored == (0 if want == 1.0 else 12)
        V = np.ones((3, 4))
        rc, st = call(0, 3, 4, *none, np.zeros(4, u64), np.zeros(0, u32), mode=mode, V=V)
        assert rc == _native.CF_OK and np.all(V == want)


def test_python_layer(gpu_ctx):
    r = gpu_ctx.nmf_fit([], [], [], 0, 0, np.zeros((0, 4)), np.zeros((0, 4)), n_sweeps=2)
    assert r.U.shape == (0, 4) and r.V.shape == (0, 4)
    c = nr.case_inputs("D8")
    with pytest.raises(ValueError):
        gpu_ctx.nmf_fit(c.user, c.item, c.obs, c.n_users, c.n_items, c.U0, c.V0, mode="dense")
    with pytest.raises(_native.NativeError):
        gpu_ctx.nmf_fit(c.user, c.item, -c.obs - 1, c.n_users, c.n_items, c.U0, c.V0, n_sweeps=1)
    with pytest.raises(_native.NativeError):
        gpu_ctx.nmf_fit(c.user, c.item, c.obs, c.n_users, c.n_items, 0.0 * c.U0, c.V0, n_sweeps=1)
    for mode in nr.MODES:
        r = gpu_ctx.nmf_fit(c.user, c.item, c.obs, c.n_users, c.n_items, c.U0, c.V0, mode=mode, n_sweeps=c.n_sweeps,
                            trace=False)
        assert r.loss_trace.size == 0 and r.loss_ms == 0.0 and r.U.tobytes() == case_fit(gpu_ctx, "D8", mode).U.tobytes()
