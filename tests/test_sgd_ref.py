"""The SGD checker (tests/sgd_ref.py) checks itself on the CPU, and the header and the built
library carry the new entry points.

Device bound: BOUND = 1e-12 * max|factor|.  The checker against itself, with every vertex's edge
list permuted and the initial factors perturbed by 1e-15 relative, drifts by at most 3.1e-15 of
max|factor| over every snapshot of the eight GPU cases (measured and asserted below against
DRIFT_SEEN = 1e-14); the bound is 100 times the worst drift, 3.1e-13, rounded up to a power of
ten, because lane-partial sums associate differently than any permutation does."""
import ctypes
import os
import re

import numpy as np
import pytest

import sgd_ref as sr
from collaborative_filtering_amd import _native

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DRIFT_SEEN = 1e-14   # the assertion of test_permuted_edges_drift; measured: see its docstring
BOUND = 1e-12        # 100 * the worst measured drift, rounded up: what test_gpu_sgd.py holds the device to


def hand_case(**over):
    kw = dict(lam=0.0, gamma=0.1, step_dec=0.9, tol=1e-3, minval=-1e100, maxval=1e100, keep_snapshots=True)
    kw.update(over)
    return sr.fit([0], [0], [5.0], 1, 1, np.array([[1.0]]), np.array([[2.0]]), **kw)


def test_case_worked_by_hand():
    """U = 1, V = 2, obs = 5, gamma = 0.1, lambda = 0: err = -3, U -> 1 + 0.1 * 3 * 2 = 1.6, the
    message is 0.1 * 3 * 1 = +0.3, V -> 2.3 one superstep later, gamma -> 0.09."""
    r = hand_case(max_supersteps=2)
    assert r.supersteps == 2 and r.updates == 2 and r.messages == 1
    (U1, V1, _, _), (U2, V2, _, _) = r.snapshots
    assert abs(U1[0, 0] - 1.6) <= 1e-15 and V1[0, 0] == 2.0
    assert U2[0, 0] == U1[0, 0] and abs(V2[0, 0] - 2.3) <= 1e-15
    assert r.gamma_next == 0.1 * 0.9
    assert abs(r.trace[0][0] - (5.0 - 1.6 * 2.0) ** 2) <= 1e-14
    # the second user superstep uses gamma = 0.09: err = 1.6 * 2.3 - 5 = -1.32 (as a float)
    r3 = hand_case(max_supersteps=3)
    err = float(np.float32(1.6 * 2.3 - 5.0))
    assert abs(r3.U[0, 0] - (1.6 - 0.09 * err * 2.3)) <= 1e-15 and r3.gamma_next == 0.1 * 0.9 * 0.9
    # a huge tol: the item is still signalled (the scatter ignores tol) but receives zero
    quiet = hand_case(max_supersteps=2, tol=1e30)
    assert quiet.messages == 0 and quiet.V[0, 0] == 2.0 and quiet.nupdates_item[0] == 1 and quiet.supersteps == 2


def test_validate_only_user_is_updated_once():
    g, U0, V0, mu = sr.case_inputs("A")
    assert g.out_degree[2] == 3 and not np.any(g.user == 2) and g.out_degree[0] == 0
    for bias in (False, True):
        r = sr.case_reference("A", bias)
        assert r.nupdates_user[2] == 1 and np.array_equal(r.U[2], U0[2])
        assert r.nupdates_user[0] == 0 and np.array_equal(r.U[0], U0[0])   # no edges of any role: never signalled
        assert r.nupdates_item[-1] == 0 and np.array_equal(r.V[-1], V0[-1])
        if bias:
            assert r.bias_user[2] == 0.0 and r.bias_item[-1] == 0.0


def test_max_updates_k_gives_2k_supersteps():
    g, *_ = sr.case_inputs("A")
    for k in (1, 3):
        r = sr.run_case("A", False, max_updates=k)
        assert r.supersteps == 2 * k
        assert np.all(r.nupdates_user[np.bincount(g.user, minlength=g.n_users) > 0] == k)
        assert np.all(r.nupdates_item[:-1] == k) and r.nupdates_item[-1] == 0


def test_odd_cut_drops_the_pending_messages():
    full = sr.case_reference("A", True)
    cut = sr.run_case("A", True, max_supersteps=3)
    assert cut.supersteps == 3
    assert np.array_equal(cut.V, full.snapshots[1][1]) and np.array_equal(cut.bias_item, full.snapshots[1][3])
    assert np.array_equal(cut.U, full.snapshots[2][0])
    assert np.array_equal(cut.nupdates_item, np.minimum(full.nupdates_item, 1))
    # sides alternate: user supersteps touch U only, item supersteps V only
    for s in range(1, len(full.snapshots)):
        dU = np.any(full.snapshots[s][0] != full.snapshots[s - 1][0])
        dV = np.any(full.snapshots[s][1] != full.snapshots[s - 1][1])
        assert (dU, dV) == ((True, False) if s % 2 == 0 else (False, True))


@pytest.mark.parametrize("name,bias", sr.KEYS)
def test_cases_are_far_from_rounding(name, bias):
    """Conditions on the inputs of the GPU cases: no error near the threshold or near a float
    midpoint, messages sent, and edges that stayed silent."""
    r = sr.case_reference(name, bias)
    print(name, bias, "thr_margin", r.thr_margin, "round_margin", r.round_margin, "messages", r.messages,
          "silent", r.silent)
    assert r.thr_margin >= 1e-6 and r.round_margin >= 1e-6
    assert r.messages > 0 and r.silent > 0 and r.n_nan == 0
    assert r.supersteps == 2 * sr.CASES[name][4]


def permuted(g, seed):
    """The same graph with the TRAIN edges in another order: every vertex's list is permuted."""
    import dataclasses

    p = np.random.default_rng(seed).permutation(len(g.user))
    return dataclasses.replace(g, user=g.user[p], item=g.item[p], obs=g.obs[p])


def drift(name, bias):
    g, U0, V0, _ = sr.case_inputs(name)
    r = sr.case_reference(name, bias)
    r2 = sr.run_case(name, bias, g=permuted(g, 9), U0=U0 * (1 + 1e-15), V0=V0 * (1 - 1e-15))
    assert r2.supersteps == r.supersteps and r2.messages == r.messages
    assert np.array_equal(r2.nupdates_user, r.nupdates_user) and np.array_equal(r2.nupdates_item, r.nupdates_item)
    worst = 0.0
    for a, b in zip(r.snapshots, r2.snapshots):
        scale = max(np.max(np.abs(a[0])), np.max(np.abs(a[1])))
        for x, y in zip(a, b):
            if x is not None:
                worst = max(worst, float(np.max(np.abs(x - y))) / scale)
    return worst


@pytest.mark.parametrize("name,bias", sr.KEYS)
def test_permuted_edges_drift(name, bias):
    """Measured (every snapshot, relative to max|factor|): between 1.7e-15 and 3.1e-15 on the eight cases."""
    d = drift(name, bias)
    print(name, bias, "drift", d)
    assert d <= DRIFT_SEEN < BOUND


def test_segmented_problem_shape():
    user, item, obs, nu, ni = sr.segmented_problem(2048, 64)
    du, di = np.bincount(user, minlength=nu), np.bincount(item, minlength=ni)
    assert di[0] == nu > 2048 and 64 < di[1] <= 2048 and 64 < du[0] <= 2048 and du[1:].max() <= 64
    assert len(set(zip(user.tolist(), item.tolist()))) == len(user)


def test_header_and_library_have_the_sgd_entry_points():
    text = open(os.path.join(ROOT, "include", "cf_abi.h")).read()
    text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    lib = ctypes.CDLL(_native.LIB_PATH)
    for fn in ("cf_sgd_fit", "cf_sgd_error", "cf_sgd_predict"):
        assert re.search(r"^int\s+" + fn + r"\s*\(", text, flags=re.M), fn
        assert hasattr(lib, fn), fn
        assert fn in _native.SIGNATURES
