"""SGD / bias-SGD matrix factorization on the GPU (cf_sgd_fit / cf_sgd_error / cf_sgd_predict)
against the numpy checker tests/sgd_ref.py.

The cases' schedules are decided far from any rounding (test_sgd_ref.py: every error is at least
1e-6 relative away from tol and 1e-6 float ulps away from a float midpoint), so update counts,
supersteps and message counts are compared exactly.  Factor and bias bound: BOUND = 1e-12 *
max|factor| after every superstep -- 100 times the checker's own drift under permuted edge lists
and initial factors perturbed by 1e-15 relative (3.1e-15, measured in test_sgd_ref.py), rounded
up to a power of ten."""
import ctypes

import numpy as np
import pytest

import als_ref as ar
import sgd_ref as sr
from collaborative_filtering_amd import _native
from collaborative_filtering_amd._native import ptr
from test_sgd_ref import BOUND

pytestmark = pytest.mark.gpu

_FITS = {}
U64_MAX = (1 << 64) - 1


def device_fit(ctx, name, bias, **over):
    g, U0, V0, mu = sr.case_inputs(name)
    kw = dict(sr.HYPER, bias=bias, max_updates=mu, activate_user=g.out_degree > 0,
              validate=(g.vuser, g.vitem, g.vobs))
    kw.update(over)
    return ctx.sgd_fit(g.user, g.item, g.obs, g.n_users, g.n_items, U0, V0, **kw)


def case_fit(ctx, name, bias):
    """The device's run of a case, computed once and shared (not modified by the tests)."""
    if (name, bias) not in _FITS:
        _FITS[(name, bias)] = device_fit(ctx, name, bias)
    return _FITS[(name, bias)]


def assert_close(tag, got, want, scale):
    err = float(np.max(np.abs(got - want))) if want.size else 0.0
    print(tag, "max|d|", err, "scale", scale)
    assert err <= BOUND * scale, (tag, err, scale)


def assert_state(tag, r, snap):
    U, V, bu, bi = snap
    scale = max(np.max(np.abs(U)), np.max(np.abs(V)))
    assert_close(tag + " U", r.U, U, scale)
    assert_close(tag + " V", r.V, V, scale)
    if bu is not None:
        assert_close(tag + " bu", r.bias_user, bu, scale)
        assert_close(tag + " bi", r.bias_item, bi, scale)
    else:
        assert r.bias_user is None and r.bias_item is None


@pytest.mark.parametrize("name,bias", sr.KEYS)
def test_case_matches_checker(gpu_ctx, name, bias):
    g, U0, V0, mu = sr.case_inputs(name)
    ref = sr.case_reference(name, bias)
    deg = np.bincount(g.item, minlength=g.n_items)
    assert deg.max() > _native.load().cf_debug_als_low_max() >= deg[deg > 0].min()   # both wave and workgroup paths
    r = case_fit(gpu_ctx, name, bias)
    print(name, bias, "supersteps", r.supersteps, ref.supersteps, "updates", r.updates, ref.updates, "messages",
          r.messages, ref.messages)
    assert r.supersteps == ref.supersteps and r.updates == ref.updates and r.messages == ref.messages
    assert r.n_nan == 0
    assert np.array_equal(r.nupdates_user, ref.nupdates_user) and np.array_equal(r.nupdates_item, ref.nupdates_item)
    assert np.float64(r.gamma_next).tobytes() == np.float64(ref.gamma_next).tobytes()
    if bias:
        assert r.global_mean == sr.train_mean(g.obs)
    assert_state(f"{name} final", r, ref.snapshots[-1])
    # after every superstep: the run cut there
    for s in range(1, ref.supersteps):
        cut = device_fit(gpu_ctx, name, bias, max_supersteps=s)
        assert cut.supersteps == s
        assert_state(f"{name} s={s}", cut, ref.snapshots[s - 1])
        gamma = sr.HYPER["gamma"]
        for _ in range((s + 1) // 2):   # one multiplication per user superstep
            gamma *= sr.HYPER["step_dec"]
        assert cut.gamma_next == gamma


@pytest.mark.parametrize("name,bias", sr.KEYS)
def test_trace_error_and_predictions(gpu_ctx, name, bias):
    g, *_ = sr.case_inputs(name)
    ref = sr.case_reference(name, bias)
    r = case_fit(gpu_ctx, name, bias)
    want = np.array(ref.trace)
    assert r.trace.shape == want.shape == (ref.supersteps // 2, 2)
    print(name, bias, "trace", r.trace[:, 0], want[:, 0])
    for t in range(len(want)):
        cut = device_fit(gpu_ctx, name, bias, max_supersteps=2 * t + 1)
        for col, (u, i, o) in enumerate(((g.user, g.item, g.obs), (g.vuser, g.vitem, g.vobs))):
            w = sr.sum_sq_error(u, i, o, cut.U, cut.V, cut.bias_user, cut.bias_item, cut.global_mean, 1.0, 5.0)
            assert abs(cut.trace[t, col] - w) <= 1e-12 * w, (t, col, cut.trace[t, col], w)
            assert cut.trace[t, col] == r.trace[t, col]          # the full run's row: same bits
            assert abs(cut.trace[t, col] - want[t, col]) <= 1e-12 * want[t, col]   # the checker's own trace
    mean = r.global_mean
    for u, i, o in ((g.user, g.item, g.obs), (g.vuser, g.vitem, g.vobs)):
        w = sr.sum_sq_error(u, i, o, r.U, r.V, r.bias_user, r.bias_item, mean, 1.0, 5.0)
        got = gpu_ctx.sgd_sum_sq_error(u, i, o, r.U, r.V, r.bias_user, r.bias_item, mean, 1.0, 5.0)
        assert abs(got - w) <= 1e-12 * w
        assert abs(gpu_ctx.sgd_rmse(u, i, o, r.U, r.V, r.bias_user, r.bias_item, mean, 1.0, 5.0) - np.sqrt(w / len(u))) \
            <= 1e-12 * np.sqrt(w / len(u))
    rng = np.random.default_rng(3)
    pu = rng.integers(0, g.n_users, 50).astype(np.uint32)
    pi = rng.integers(0, g.n_items, 50).astype(np.uint32)
    got = gpu_ctx.sgd_predict(pu, pi, r.U, r.V, r.bias_user, r.bias_item, mean, minval=1.0, maxval=5.0)
    prod = r.U[pu] * r.V[pi]
    want_p, scale = prod.sum(axis=1), np.abs(prod).sum(axis=1)
    if bias:   # the bias predictor clamps (biassgd.cpp:423-428)
        want_p = mean + r.bias_user[pu] + r.bias_item[pi] + want_p
        scale = scale + abs(mean) + np.abs(r.bias_user[pu]) + np.abs(r.bias_item[pi])
        clamped = np.clip(want_p, 1.0, 5.0)
        assert np.any(clamped != want_p)
        assert np.all((got >= 1.0) & (got <= 5.0))
        assert np.all(np.abs(got - clamped) <= 1e-13 * scale)
    else:      # the plain one does not (sgd.cpp:418-419); test_gpu_als.py's rule
        assert np.any((want_p < 1.0) | (want_p > 5.0)) and np.any((got < 1.0) | (got > 5.0))
        plain = np.abs(want_p) >= 0.1 * scale
        assert plain.sum() >= 10
        assert np.all(np.abs(got - want_p)[plain] <= 1e-13 * np.abs(want_p)[plain])
        assert np.all(np.abs(got - want_p)[~plain] <= 1e-13 * scale[~plain])


def test_without_biases_equals_the_als_entry_points(gpu_ctx):
    g, *_ = sr.case_inputs("A")
    r = case_fit(gpu_ctx, "A", False)
    for u, i, o in ((g.user, g.item, g.obs), (g.vuser, g.vitem, g.vobs)):
        a = gpu_ctx.als_sum_sq_error(u, i, o, r.U, r.V, 1.0, 5.0)
        b = gpu_ctx.sgd_sum_sq_error(u, i, o, r.U, r.V, None, None, 0.0, 1.0, 5.0)
        assert np.float64(a).tobytes() == np.float64(b).tobytes()
    rng = np.random.default_rng(3)
    pu = rng.integers(0, g.n_users, 200).astype(np.uint32)
    pi = rng.integers(0, g.n_items, 200).astype(np.uint32)
    assert gpu_ctx.als_predict(pu, pi, r.U, r.V).tobytes() == gpu_ctx.sgd_predict(pu, pi, r.U, r.V, clamp=False).tobytes()


@pytest.mark.parametrize("bias", [False, True])
def test_repeat_is_bit_identical(gpu_ctx, bias):
    a, b = case_fit(gpu_ctx, "A", bias), device_fit(gpu_ctx, "A", bias)
    pairs = [(a.U, b.U), (a.V, b.V), (a.nupdates_user, b.nupdates_user), (a.nupdates_item, b.nupdates_item),
             (a.trace, b.trace)]
    if bias:
        pairs += [(a.bias_user, b.bias_user), (a.bias_item, b.bias_item)]
    for x, y in pairs:
        assert x.tobytes() == y.tobytes()
    assert a.messages == b.messages


@pytest.mark.parametrize("bias", [False, True])
def test_independent_of_the_active_set(gpu_ctx, bias):
    g, *_ = sr.case_inputs("A")
    full = device_fit(gpu_ctx, "A", bias, max_supersteps=1)
    even = (np.arange(g.n_users) % 2 == 0) & (g.out_degree > 0)
    part = device_fit(gpu_ctx, "A", bias, max_supersteps=1, activate_user=even)
    assert part.U[even].tobytes() == full.U[even].tobytes()
    if bias:
        assert part.bias_user[even].tobytes() == full.bias_user[even].tobytes()
    assert not np.any(part.nupdates_user[~even]) and np.all(part.nupdates_user[even] == 1)
    # the subset against the checker, two supersteps on: the items' messages only hold even users
    ref = sr.run_case("A", bias, activate_user=even, max_supersteps=3)
    got = device_fit(gpu_ctx, "A", bias, activate_user=even, max_supersteps=3)
    assert got.supersteps == ref.supersteps == 3 and got.messages == ref.messages and got.updates == ref.updates
    assert_state("subset", got, ref.snapshots[-1])
    assert np.array_equal(got.nupdates_user, ref.nupdates_user) and np.array_equal(got.nupdates_item, ref.nupdates_item)


@pytest.mark.parametrize("D", [4, 28])
@pytest.mark.parametrize("bias", [False, True])
def test_segmented_vertex(gpu_ctx, bias, D):
    """Item 0 is rated by segment + 52 users (two segment partials in HBM), item 1 and user 0 are
    above the low cut (one workgroup each), everything else takes one wave."""
    lib = _native.load()
    user, item, obs, nu, ni = sr.segmented_problem(lib.cf_debug_als_segment(), lib.cf_debug_als_low_max())
    rng = np.random.default_rng(6)
    U0, V0 = rng.uniform(-1, 1, (nu, D)), rng.uniform(-1, 1, (ni, D))
    hyper = dict(sr.HYPER, gamma=0.002)
    mean = sr.train_mean(obs) if bias else 0.0
    ref = sr.fit(user, item, obs, nu, ni, U0, V0, bias=bias, mean=mean, max_updates=2, keep_snapshots=True, **hyper)
    assert ref.supersteps == 4 and ref.thr_margin >= 1e-6 and ref.round_margin >= 1e-6 and ref.messages > 0 < ref.silent
    runs = [gpu_ctx.sgd_fit(user, item, obs, nu, ni, U0, V0, bias=bias, max_updates=2, **hyper) for _ in range(2)]
    r = runs[0]
    assert r.supersteps == 4 and r.messages == ref.messages and r.updates == ref.updates and r.n_nan == 0
    assert_state("segmented", r, ref.snapshots[-1])
    assert runs[1].U.tobytes() == r.U.tobytes() and runs[1].V.tobytes() == r.V.tobytes()
    if bias:
        assert runs[1].bias_item.tobytes() == r.bias_item.tobytes()


def test_caps(gpu_ctx):
    g, U0, V0, _ = sr.case_inputs("A")
    one = device_fit(gpu_ctx, "A", True, max_updates=1)
    ref = sr.run_case("A", True, max_updates=1)
    assert one.supersteps == ref.supersteps == 2 and one.updates == ref.updates
    assert one.nupdates_user.max() == 1 and one.nupdates_item.max() == 1
    assert_state("max_updates=1", one, ref.snapshots[-1])
    odd = device_fit(gpu_ctx, "A", True, max_supersteps=3)   # the pending messages are dropped
    two = device_fit(gpu_ctx, "A", True, max_supersteps=2)
    assert odd.supersteps == 3 and odd.V.tobytes() == two.V.tobytes() and odd.bias_item.tobytes() == two.bias_item.tobytes()
    assert odd.U.tobytes() != two.U.tobytes() and np.array_equal(odd.nupdates_item, two.nupdates_item)
    assert odd.trace.shape == (2, 2) and two.trace.shape == (1, 2)
    assert one.nupdates_user[0] == 0 and np.array_equal(one.U[0], U0[0])   # no edges at all: never signalled
    assert one.nupdates_user[2] == 1 and np.array_equal(one.U[2], U0[2])   # VALIDATE only: the increment alone
    assert one.nupdates_item[-1] == 0 and np.array_equal(one.V[-1], V0[-1])


def raw_fit(ctx, n_users, n_items, D, uoff, uitem, ioff, iuser, max_updates=3, max_supersteps=0, bu=True, bi=True):
    nnz = len(uitem)
    obs = np.ones(max(nnz, 1), np.float32)
    U, V = np.zeros((max(n_users, 1), D)), np.zeros((max(n_items, 1), D))
    z = lambda n, t: np.zeros(max(n, 1), t)   # noqa: E731
    par = _native.SgdParams(0.05, 0.02, 0.9, 0.5, 1.0, 5.0, 3.0, max_updates, max_supersteps)
    st = _native.SgdStats()
    rc = ctx.lib.cf_sgd_fit(ctx.h, n_users, n_items, D, ptr(uoff), ptr(uitem), ptr(obs), ptr(ioff), ptr(iuser), ptr(obs),
                            ctypes.byref(par), ptr(U), ptr(V), ptr(z(n_users, np.float64)) if bu else None,
                            ptr(z(n_items, np.float64)) if bi else None, ptr(z(n_users, np.uint32)),
                            ptr(z(n_items, np.uint32)), None, 0, None, None, None, None, 0, ctypes.byref(st))
    return rc, st


def test_argument_checks(gpu_ctx):
    u64, u32 = np.uint64, np.uint32
    uoff, uitem = np.array([0, 1, 2], u64), np.array([0, 0], u32)
    ioff, iuser = np.array([0, 2], u64), np.array([0, 1], u32)
    rc, st = raw_fit(gpu_ctx, 2, 1, 4, uoff, uitem, ioff, iuser)
    assert rc == _native.CF_OK and st.supersteps == 6 and st.updates == 9
    assert raw_fit(gpu_ctx, 2, 1, 4, uoff, uitem, ioff, iuser, max_updates=U64_MAX)[0] == _native.CF_EINVAL   # no cap
    assert raw_fit(gpu_ctx, 2, 1, 4, uoff, uitem, ioff, iuser, max_updates=U64_MAX, max_supersteps=3)[0] == _native.CF_OK
    assert raw_fit(gpu_ctx, 2, 1, 4, uoff, uitem, ioff, iuser, bi=False)[0] == _native.CF_EINVAL   # one bias pointer
    assert raw_fit(gpu_ctx, 2, 1, 4, uoff, uitem, ioff, iuser, bu=False)[0] == _native.CF_EINVAL
    assert raw_fit(gpu_ctx, 2, 1, 4, uoff, uitem, ioff, iuser, bu=False, bi=False)[0] == _native.CF_OK
    assert raw_fit(gpu_ctx, 2, 1, 65, uoff, uitem, ioff, iuser)[0] == _native.CF_ERANGE
    assert raw_fit(gpu_ctx, 2, 1, 4, uoff, uitem, np.array([0, 1], u64), iuser)[0] == _native.CF_EINVAL   # edge totals differ
    assert raw_fit(gpu_ctx, 2, 2, 4, uoff, uitem, np.array([0, 1, 2], u64), iuser)[0] == _native.CF_EINVAL   # per-item counts
    assert raw_fit(gpu_ctx, 2, 1, 4, uoff, np.array([0, 1], u32), ioff, iuser)[0] == _native.CF_EINVAL   # item out of range
    rc, st = raw_fit(gpu_ctx, 0, 0, 4, np.zeros(1, u64), np.zeros(0, u32), np.zeros(1, u64), np.zeros(0, u32))
    assert rc == _native.CF_OK and st.supersteps == 0 and st.updates == 0 and st.gamma_next == 0.02
    rc, st = raw_fit(gpu_ctx, 2, 1, 4, np.zeros(3, u64), np.zeros(0, u32), np.zeros(2, u64), np.zeros(0, u32))   # no edges
    assert rc == _native.CF_OK and st.supersteps == 1 and st.updates == 2 and st.messages == 0
    rc, st = raw_fit(gpu_ctx, 2, 0, 4, np.zeros(3, u64), np.zeros(0, u32), np.zeros(1, u64), np.zeros(0, u32))   # no items
    assert rc == _native.CF_OK and st.supersteps == 1 and st.updates == 2


def test_python_layer_accepts_an_empty_side(gpu_ctx):
    r = gpu_ctx.sgd_fit([], [], [], 0, 0, np.zeros((0, 4)), np.zeros((0, 4)), max_updates=2, bias=True)
    assert r.supersteps == 0 and r.updates == 0 and r.U.shape == (0, 4) and r.trace.shape == (0, 2)
    with pytest.raises(_native.NativeError):
        gpu_ctx.sgd_fit([0], [0], [3.0], 1, 1, np.ones((1, 2)), np.ones((1, 2)))   # no cap


def test_nan_stops_the_fit(gpu_ctx):
    g, U0, V0, _ = sr.case_inputs("A")
    V0 = V0.copy()
    V0[0, 3] = np.nan   # item 0: rated by every user with edges
    r = gpu_ctx.sgd_fit(g.user, g.item, g.obs, g.n_users, g.n_items, U0, V0, max_supersteps=8,
                        activate_user=g.out_degree > 0, **sr.HYPER)
    assert r.n_nan == int(np.sum(g.item == 0)) and r.supersteps == 1
    assert np.array_equal(r.V[1:], V0[1:])   # the messages were never applied


def test_workspace_release(gpu_ctx):
    """SGD carves the context's ALS workspace: released, then allocated again; ALS after SGD too."""
    a = case_fit(gpu_ctx, "C", True)
    gpu_ctx.release_workspaces()
    b = device_fit(gpu_ctx, "C", True)
    assert a.U.tobytes() == b.U.tobytes() and a.V.tobytes() == b.V.tobytes() and a.bias_item.tobytes() == b.bias_item.tobytes()
    g, U0, V0, *_ = ar.case_inputs("C")
    x = gpu_ctx.als_fit(g.user, g.item, g.obs, g.n_users, g.n_items, U0, V0, lam=0.01, max_updates=2)
    gpu_ctx.release_workspaces()
    y = gpu_ctx.als_fit(g.user, g.item, g.obs, g.n_users, g.n_items, U0, V0, lam=0.01, max_updates=2)
    assert x.U.tobytes() == y.U.tobytes()
