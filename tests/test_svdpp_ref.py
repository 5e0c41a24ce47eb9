"""The SVD++ checker (tests/svdpp_ref.py) checks itself on the CPU, and the header and the built
library carry the new entry points.

Device bound: BOUND = 1e-12 * max|factor|.  The checker against itself, with every vertex's TRAIN
and implicit edge lists permuted and the four initial matrices perturbed by 1e-15 relative, drifts
by at most 2.0e-15 of max|factor| over every snapshot of the four GPU cases (measured and
asserted below against DRIFT_SEEN = 1e-14); the bound is 100 times the worst drift, 2.0e-13, rounded
up to a power of ten, because lane-partial sums associate differently than any permutation does."""
import ctypes
import dataclasses
import os
import re

import numpy as np
import pytest

import sgd_ref
import svdpp_ref as pr
from collaborative_filtering_amd import _native

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DRIFT_SEEN = 1e-14   # the assertion of test_permuted_edges_drift; measured: see its docstring
BOUND = 1e-12        # 100 * the worst measured drift, rounded up: what test_gpu_svdpp.py holds the device to
f32 = np.float32


def hand_fit(**over):
    """One user; items 0 and 1 TRAIN (obs 4 and 2), item 2 VALIDATE only.  D = 2.  Every step is
    0.125, every regulariser 0.25, step_dec 0.5 (all exact in float32), mean 3, range [1, 5]."""
    hyper = {k: 0.125 for k in pr.STEP_NAMES}
    hyper.update({k: 0.25 for k in pr.REG_NAMES})
    kw = dict(hyper, implicit=([0], [2]), step_dec=0.5, minval=1.0, maxval=5.0, mean=3.0, max_updates=4,
              validate=([0], [2], [3.0]), keep_snapshots=True)
    kw.update(over)
    U0, W0 = np.array([[1.0, 0.5]]), np.array([[9.0, 9.0]])
    V0 = np.array([[1.0, 2.0], [0.5, -1.0], [3.0, 3.0]])
    Y0 = np.array([[0.1, 0.2], [0.3, -0.1], [0.2, 0.4]])
    return pr.fit([0, 0], [0, 1], [4.0, 2.0], 1, 3, U0, V0, W0, Y0, **kw), (U0, V0, W0, Y0)


def test_case_worked_by_hand():
    r, (U0, V0, W0, Y0) = hand_fit()
    assert r.supersteps == 8 and r.updates == 4 + 3 + 2 + 3 + 2 and r.messages == 4 and r.n_nan == 0
    n = np.float64(f32(1.0 / np.sqrt(3.0)))   # usrNorm: three edges of any role
    S = r.snapshots
    # superstep 0, user in phase 1: W = usrNorm (Y0 + Y1 + Y2), the VALIDATE-only item included
    W1 = n * np.array([0.1 + 0.3 + 0.2, 0.2 - 0.1 + 0.4])
    assert np.allclose(S[0][2][0], W1, rtol=1e-15, atol=0) and np.array_equal(S[0][0], U0) and S[0][4][0] == 0.0
    assert list(S[0][6]) == [1] and list(S[0][7]) == [0, 0, 0]
    # superstep 1: the three items (item 2 signalled by phase 1 alone) run phase 1: an update count and nothing else
    assert list(S[1][7]) == [1, 1, 1] and np.array_equal(S[1][1], V0) and np.array_equal(S[1][3], Y0)
    # superstep 2, user in phase 2 with step 0.0625 (one decay): p0 = 3 + 1.1 + 1.1 = 5.2 -> 5, err0 = -1;
    # p1 = 3 + 0.8 - 0.55 = 3.25, err1 = -1.25
    s, reg = 0.0625, 0.25
    e = [-1.0, -1.25]
    U2 = U0[0] + s * (e[0] * (V0[0] - reg * U0[0])) + s * (e[1] * (V0[1] - reg * U0[0]))
    assert np.allclose(S[2][0][0], U2, rtol=1e-15, atol=0)
    assert abs(S[2][4][0] - s * (e[0] + e[1])) <= 1e-16 and np.array_equal(S[2][2][0], S[0][2][0])
    assert np.array_equal(S[2][1], V0) and list(S[2][6]) == [2]
    # superstep 3, items 0 and 1 in phase 2 add the messages made from the OLD U and the new W; item 2 was not signalled
    c = np.float64(f32(f32(s) * f32(n)))
    mult = np.float64(f32(f32(s) * f32(reg)))
    for i in (0, 1):
        dV = s * (e[i] * (U0[0] + W1) - reg * V0[i])
        dY = (e[i] * V0[i]) * c - mult * Y0[i]
        assert np.allclose(S[3][1][i], V0[i] + dV, rtol=1e-15, atol=0)
        assert np.allclose(S[3][3][i], Y0[i] + dY, rtol=1e-15, atol=0)
        assert abs(S[3][5][i] - s * e[i]) <= 1e-16
    assert list(S[3][7]) == [2, 2, 1] and np.array_equal(S[3][1][2], V0[2]) and np.array_equal(S[3][3][2], Y0[2])
    # superstep 4, phase 1 again: W from the new Y0, Y1 and the old Y2
    W5 = n * (S[3][3][0] + S[3][3][1] + Y0[2])
    assert np.allclose(S[4][2][0], W5, rtol=1e-15, atol=0) and np.array_equal(S[4][0], S[2][0])
    # superstep 5: items 0, 1 (phase 1) and item 2 (phase 2, but nobody sends to a VALIDATE-only item) stay
    assert list(S[5][7]) == [3, 3, 2] and np.array_equal(S[5][1], S[3][1]) and np.array_equal(S[5][3], S[3][3])
    # supersteps 6, 7: the second gradient pass, step 0.125 / 8; everybody reaches max_updates = 4
    assert not np.array_equal(S[6][0], S[4][0]) and not np.array_equal(S[7][1][:2], S[5][1][:2])
    assert list(S[7][6]) == [4] and list(S[7][7]) == [4, 4, 2]
    assert np.array_equal(r.steps_next, np.full(5, 0.125 / 16, f32))
    # the trace leaves Y out
    t0 = (4 - min(5.0, 3 + U0[0] @ V0[0])) ** 2 + (2 - max(1.0, 3 + U0[0] @ V0[1])) ** 2
    assert abs(r.trace[0][0] - t0) <= 1e-15 * t0 and len(r.trace) == 4
    assert r.trace[0][1] == (3.0 - 5.0) ** 2   # 3 + 4.5 clamped to 5


def test_max_updates_2k_gives_4k_supersteps():
    c = pr.case_inputs("A")
    trained = np.bincount(c.g.user, minlength=c.g.n_users) > 0
    for k in (1, 2):
        r = pr.run_case("A", max_updates=2 * k)
        assert r.supersteps == 4 * k and len(r.trace) == 2 * k
        assert np.all(r.nupdates_user[trained] == 2 * k)
        assert np.all(r.nupdates_item[:-1] == 2 * k) and r.nupdates_item[-1] == 0
        assert r.mixed_supersteps == 0 and r.discarded == 0


def test_validate_only_vertices():
    c = pr.case_inputs("A")
    r = pr.case_reference("A")
    assert c.g.out_degree[2] == 3 and not np.any(c.g.user == 2) and c.g.out_degree[0] == 0
    # user 2 (VALIDATE edges only): phase 1 gives it a W, phase 2 never comes (no item signals it)
    assert r.nupdates_user[2] == 1 and not np.array_equal(r.W[2], c.W0[2]) and np.array_equal(r.U[2], c.U0[2])
    assert r.nupdates_user[0] == 0 and np.array_equal(r.W[0], c.W0[0])   # no edges of any role: never signalled
    assert r.nupdates_item[-1] == 0 and np.array_equal(r.Y[-1], c.Y0[-1])


def test_inactive_users_run_phase_1_beside_phase_2_and_phase_1_items_ignore_messages():
    c = pr.case_inputs("A")
    even = (np.arange(c.g.n_users) % 2 == 0) & (c.g.out_degree > 0)
    r = pr.run_case("A", activate_user=even, max_supersteps=6)
    S = r.snapshots
    assert r.supersteps == 6 and r.mixed_supersteps == 2   # supersteps 2 and 4
    odd_trained = ~even & (np.bincount(c.g.user, minlength=c.g.n_users) > 0)
    # superstep 2: the even users run phase 2 (U moves), the odd ones phase 1 (W moves, U does not)
    assert np.all(np.any(S[2][2][odd_trained] != S[1][2][odd_trained], axis=1))
    assert np.array_equal(S[2][0][odd_trained], S[1][0][odd_trained])
    assert np.any(S[2][0][even] != S[1][0][even]) and np.array_equal(S[2][2][even], S[1][2][even])
    assert np.all(S[2][6][odd_trained] == 1) and np.all(S[2][6][even & (np.bincount(c.g.user, minlength=c.g.n_users) > 0)] == 2)
    # superstep 4: the odd users are in phase 2, every item has nupdates 2 (phase 1): their messages are discarded
    assert r.discarded > 0 and np.array_equal(S[5][1], S[4][1]) and np.array_equal(S[5][3], S[4][3])
    assert np.any(S[4][0][odd_trained] != S[3][0][odd_trained])
    assert np.any(S[5][7] != S[4][7])


def test_odd_cut_drops_the_pending_messages():
    full = pr.case_reference("A")
    c = pr.case_inputs("A")
    cut = pr.run_case("A", max_supersteps=3)
    assert cut.supersteps == 3 and cut.messages > 0
    assert np.array_equal(cut.V, c.V0) and np.array_equal(cut.Y, c.Y0) and not np.any(cut.bias_item)
    assert np.array_equal(cut.U, full.snapshots[2][0]) and not np.array_equal(cut.U, c.U0)
    assert np.array_equal(cut.nupdates_item, np.minimum(full.nupdates_item, 1))


@pytest.mark.parametrize("name", pr.NAMES)
def test_cases_move_and_are_far_from_rounding(name):
    """Conditions on the inputs of the GPU cases: the factors move by more than 1e-3 of max|factor|
    in some superstep (a kernel that does nothing cannot pass the device bound), no error is near
    a float midpoint, the implicit list is not empty, and the trace is sgd_ref's error without Y."""
    c = pr.case_inputs(name)
    r = pr.case_reference(name)
    print(name, "max_change", r.max_change, "round_margin", r.round_margin, "messages", r.messages)
    assert r.max_change > 1e-3 and r.round_margin >= 1e-6 and r.messages > 0 and r.n_nan == 0
    assert r.supersteps == 2 * c.max_updates and len(c.imp_user) > len(c.g.vuser) > 0
    for k in (0, 1, 3):   # U, V and Y each move
        assert max(np.max(np.abs(b[k] - a[k])) for a, b in zip(r.snapshots, r.snapshots[1:])) > 1e-3
    g = c.g
    for t, row in enumerate(r.trace):
        U, V, _, _, bu, bi, _, _ = r.snapshots[2 * t]
        assert row[0] == sgd_ref.sum_sq_error(g.user, g.item, g.obs, U, V, bu, bi, sgd_ref.train_mean(g.obs), 1.0, 5.0)
        assert row[1] == sgd_ref.sum_sq_error(g.vuser, g.vitem, g.vobs, U, V, bu, bi, sgd_ref.train_mean(g.obs), 1.0, 5.0)
    with_y = np.sum((g.obs - pr.predict(g.user, g.item, r.U, r.V, r.Y, r.bias_user, r.bias_item,
                                        sgd_ref.train_mean(g.obs), 1.0, 5.0)) ** 2)
    assert abs(with_y - sgd_ref.sum_sq_error(g.user, g.item, g.obs, r.U, r.V, r.bias_user, r.bias_item,
                                             sgd_ref.train_mean(g.obs), 1.0, 5.0)) > 1e-3   # Y matters to the predictor


def permuted(c, seed):
    """The same case with the TRAIN and implicit edges in another order and the initial matrices
    perturbed by 1e-15 relative."""
    rng = np.random.default_rng(seed)
    p, q = rng.permutation(len(c.g.user)), rng.permutation(len(c.imp_user))
    g = dataclasses.replace(c.g, user=c.g.user[p], item=c.g.item[p], obs=c.g.obs[p])
    return dataclasses.replace(c, g=g, imp_user=c.imp_user[q], imp_item=c.imp_item[q], U0=c.U0 * (1 + 1e-15),
                               V0=c.V0 * (1 - 1e-15), W0=c.W0 * (1 + 1e-15), Y0=c.Y0 * (1 - 1e-15))


def drift(name):
    r = pr.case_reference(name)
    r2 = pr.run_case(name, case=permuted(pr.case_inputs(name), 9))
    assert r2.supersteps == r.supersteps and r2.messages == r.messages
    assert np.array_equal(r2.nupdates_user, r.nupdates_user) and np.array_equal(r2.nupdates_item, r.nupdates_item)
    worst = 0.0
    for a, b in zip(r.snapshots, r2.snapshots):
        scale = max(np.max(np.abs(a[k])) for k in range(4))
        for x, y in zip(a[:6], b[:6]):
            worst = max(worst, float(np.max(np.abs(x - y))) / scale)
    return worst


@pytest.mark.parametrize("name", pr.NAMES)
def test_permuted_edges_drift(name):
    """Measured (every snapshot, relative to max|factor|): A 1.9e-15, B 1.5e-15, C 2.0e-15, E 1.4e-15."""
    d = drift(name)
    print(name, "drift", d)
    assert d <= DRIFT_SEEN < BOUND


def test_segmented_case_shape():
    user, item, obs, nu, ni, iu, ii, mats = pr.segmented_case(2048, 64)
    du, di = np.bincount(user, minlength=nu), np.bincount(item, minlength=ni)
    da = du + np.bincount(iu, minlength=nu)
    assert di[0] == nu > 2048 and 64 < di[1] <= 2048 and 64 < du[0] <= 2048
    assert du[1] <= 64 < da[1] and du[1:].max() <= 64   # user 1: above the low cut through its implicit edges alone
    assert not set(zip(user[user == 1].tolist(), item[user == 1].tolist())) & set(zip(iu[iu == 1].tolist(), ii[iu == 1].tolist()))


def test_header_and_library_have_the_svdpp_entry_points():
    text = open(os.path.join(ROOT, "include", "cf_abi.h")).read()
    text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    lib = ctypes.CDLL(_native.LIB_PATH)
    for fn in ("cf_svdpp_fit", "cf_svdpp_predict", "cf_svdpp_timing"):
        assert re.search(r"^int\s+" + fn + r"\s*\(", text, flags=re.M), fn
        assert hasattr(lib, fn), fn
        assert fn in _native.SIGNATURES
    assert not re.search(r"cf_svdpp_error", text)   # the error is cf_sgd_error: no new entry point
