"""The iALS checker (tests/ials_ref.py) on the CPU: the input conditions the GPU tests rely on,
checked where they can be checked.  The checker is dense on purpose; here it is tied to the
Gram-trick formulas the kernels implement."""
import numpy as np
import pytest

import als_ref as ar
import ials_ref as ir


def test_dense_update_equals_the_gram_trick():
    c = ir.case_inputs("B8")
    Cw, Bw, _ = ir.dense_weights(c.user, c.item, c.conf, c.pref, c.n_users, c.n_items)
    off, nbr, conf, perm = ar.build_csr(c.user, c.item, c.conf, c.n_users)
    pref = c.pref[perm].astype(np.float64)
    for u in range(c.n_users):
        b, e = int(off[u]), int(off[u + 1])
        dense = ir.dense_update(c.V0, Cw[u], Bw[u], c.reg_user[u])
        trick = ir.gram_trick_update(c.V0, nbr[b:e], conf[b:e].astype(np.float64), pref[b:e], c.reg_user[u])
        assert np.max(np.abs(dense - trick)) <= 1e-12 * max(1.0, np.max(np.abs(dense))), u
        if e == b:
            assert not np.any(dense)   # no edges: b = 0, the minimiser is the zero vector


def test_repeated_edges_each_count():
    c = ir.gram_fit_case(64)
    Cw, Bw, _ = ir.dense_weights(c.user, c.item, c.conf, c.pref, c.n_users, c.n_items)
    u, i = int(c.user[-1]), int(c.item[-1])
    twice = (c.user == u) & (c.item == i)
    assert twice.sum() == 2
    cc = c.conf[twice].astype(np.float64)
    assert Cw[u, i] == pytest.approx(1.0 + np.sum(cc - 1.0), rel=1e-15)
    assert Bw[u, i] == pytest.approx(np.sum(cc * c.pref[twice]), rel=1e-15)
    sel = c.user == u
    trick = ir.gram_trick_update(c.V0, c.item[sel], c.conf[sel].astype(np.float64), c.pref[sel].astype(np.float64), 0.1)
    assert np.max(np.abs(ir.dense_update(c.V0, Cw[u], Bw[u], 0.1) - trick)) <= 1e-12


@pytest.mark.parametrize("name", ["A", "B8"])
def test_dense_loss_equals_the_closed_form(name):
    c = ir.case_inputs(name)
    for U, V in ((c.U0, c.V0), (0.3 * c.U0, -2.0 * c.V0)):
        dense = ir.loss(c.user, c.item, c.conf, c.pref, c.n_users, c.n_items, U, V, c.reg_user, c.reg_item)
        closed = ir.closed_form_loss(c.user, c.item, c.conf, c.pref, U, V, c.reg_user, c.reg_item)
        assert abs(dense - closed) <= 1e-12 * dense


def test_dense_loss_is_the_literal_sum_without_repeats():
    c = ir.case_inputs("B8")
    C, P = np.ones((c.n_users, c.n_items)), np.zeros((c.n_users, c.n_items))
    C[c.user, c.item], P[c.user, c.item] = c.conf, c.pref
    want = np.sum(C * (P - c.U0 @ c.V0.T) ** 2) + np.sum(c.reg_user * np.sum(c.U0 ** 2, axis=1)) + \
        np.sum(c.reg_item * np.sum(c.V0 ** 2, axis=1))
    got = ir.loss(c.user, c.item, c.conf, c.pref, c.n_users, c.n_items, c.U0, c.V0, c.reg_user, c.reg_item)
    assert abs(got - want) <= 1e-13 * want


@pytest.mark.parametrize("name", list(ir.CASES) + ["G"])
def test_loss_trace_is_non_increasing(name):
    ref = ir.fit_case(ir.gram_fit_case(512)) if name == "G" else ir.case_reference(name)
    assert ref.loss_trace.shape == (2 * ir.N_SWEEPS,)
    assert np.all(np.diff(ref.loss_trace) <= 0), ref.loss_trace
    assert ref.min_eig_ratio >= 1e-3
