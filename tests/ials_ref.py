"""Checker for the implicit-feedback ALS entry points (cf_ials_fit / cf_ials_loss): plain numpy
fp64, written from the model's equations.  It does NOT use the Gram trick the kernels rely on:
per vertex it builds the full weighted normal equations over ALL rows of the other side from
dense weight vectors and calls np.linalg.solve, and its loss is the double sum over the dense
n_users x n_items grid.

A pair (u, i) with edges e_1 .. e_k (k = 0 for most pairs, repeated edges each count) enters as
    weight   Cw = 1 + sum_e (c_e - 1)      (1 without an edge, c with one)
    target   Bw = sum_e c_e p_e            (0 without an edge, c p with one)
so vertex u solves (V^T diag(Cw[u]) V + reg I) x = V^T Bw[u], and the pair's loss is
Cw (Bw / Cw - s)^2 + (sum_e c_e p_e^2 - Bw^2 / Cw): with at most one edge that is c (p - s)^2.
Also holds the case table the GPU tests share; the graphs come from als_ref.make_graph."""
from __future__ import annotations

from dataclasses import dataclass

import numpy as np

import als_ref as ar


def dense_weights(user, item, conf, pref, n_users, n_items):
    """(Cw, Bw, Qw) over the dense grid; Qw = sum_e c_e p_e^2."""
    user, item = np.asarray(user, np.int64), np.asarray(item, np.int64)
    c = np.asarray(conf, np.float32).astype(np.float64)
    p = np.ones(len(c)) if pref is None else np.asarray(pref, np.float32).astype(np.float64)
    Cw, Bw, Qw = np.ones((n_users, n_items)), np.zeros((n_users, n_items)), np.zeros((n_users, n_items))
    np.add.at(Cw, (user, item), c - 1.0)
    np.add.at(Bw, (user, item), c * p)
    np.add.at(Qw, (user, item), c * p * p)
    return Cw, Bw, Qw


def dense_update(X, cw, bw, reg):
    """The minimiser of one vertex: X = ALL rows of the other side, cw / bw its dense weights."""
    A = X.T @ (cw[:, None] * X)
    A[np.diag_indices_from(A)] += reg
    return np.linalg.solve(A, X.T @ bw)


def dense_loss(Cw, Bw, Qw, U, V, reg_user, reg_item):
    S = U @ V.T
    grid = np.sum(Cw * (Bw / Cw - S) ** 2) + np.sum(Qw - Bw * Bw / Cw)
    return float(grid + np.sum(reg_user * np.sum(U * U, axis=1)) + np.sum(reg_item * np.sum(V * V, axis=1)))


def loss(user, item, conf, pref, n_users, n_items, U, V, reg_user, reg_item):
    Cw, Bw, Qw = dense_weights(user, item, conf, pref, n_users, n_items)
    return dense_loss(Cw, Bw, Qw, np.asarray(U, np.float64), np.asarray(V, np.float64), reg_user, reg_item)


@dataclass
class RefResult:
    U: np.ndarray
    V: np.ndarray
    loss_trace: np.ndarray       # after each half-sweep
    min_eig_ratio: float         # smallest lambda_min / lambda_max of a solved system


def fit(user, item, conf, pref, n_users, n_items, U0, V0, reg_user, reg_item, n_sweeps) -> RefResult:
    Cw, Bw, Qw = dense_weights(user, item, conf, pref, n_users, n_items)
    U, V = np.array(U0, dtype=np.float64), np.array(V0, dtype=np.float64)
    D = U.shape[1]
    trace, ratio = [], np.inf
    for _ in range(n_sweeps):
        for F, X, C, B, reg in ((U, V, Cw, Bw, reg_user), (V, U, Cw.T, Bw.T, reg_item)):
            for v in range(F.shape[0]):
                F[v] = dense_update(X, C[v], B[v], reg[v])
                if v % 16 == 0:   # conditioning sampled: it is a property of the case, not a bound
                    w = np.linalg.eigvalsh(X.T @ (C[v][:, None] * X) + reg[v] * np.eye(D))
                    ratio = min(ratio, float(w[0] / w[-1]))
            trace.append(dense_loss(Cw, Bw, Qw, U, V, reg_user, reg_item))
    return RefResult(U, V, np.array(trace), ratio)


# ---- the Gram-trick formulas, for the CPU test that ties the checker to what the kernels do ----

def gram_trick_update(Xall, nbr, c, p, reg):
    """(G + sum (c - 1) x x^T + reg I) f = sum c p x over the vertex's edge list."""
    X = Xall[nbr]
    A = Xall.T @ Xall + X.T @ ((c - 1.0)[:, None] * X)
    A[np.diag_indices_from(A)] += reg
    return np.linalg.solve(A, X.T @ (c * p))


def closed_form_loss(user, item, conf, pref, U, V, reg_user, reg_item):
    """<G_U, G_V>_F + sum_obs [c (p - s)^2 - s^2] + the reg terms."""
    user, item = np.asarray(user, np.int64), np.asarray(item, np.int64)
    c = np.asarray(conf, np.float32).astype(np.float64)
    p = np.ones(len(c)) if pref is None else np.asarray(pref, np.float32).astype(np.float64)
    s = np.einsum("ij,ij->i", U[user], V[item])
    return float(np.sum((U.T @ U) * (V.T @ V)) + np.sum(c * (p - s) ** 2 - s * s) +
                 np.sum(reg_user * np.sum(U * U, axis=1)) + np.sum(reg_item * np.sum(V * V, axis=1)))


# ---- the shared cases -----------------------------------------------------------------------

@dataclass
class Case:
    n_users: int
    n_items: int
    D: int
    user: np.ndarray
    item: np.ndarray
    conf: np.ndarray
    pref: np.ndarray | None
    reg_user: np.ndarray
    reg_item: np.ndarray
    U0: np.ndarray
    V0: np.ndarray


N_SWEEPS = 2

CASES = {
    # name: (users, items, D, min raters per item, preferences given)
    "A": (96, 40, 20, 0, True),      # graph A of als_ref: low and mid items, empty user and item
    "B": (96, 40, 33, 0, False),     # DP = 64 padding, pref = None
    "B1": (24, 10, 1, 0, False),     # the cut-down graph
    "B8": (24, 10, 8, 0, True),
    "E": (96, 40, 13, 0, True),      # D = 9..16: the DP = 16 tier, low and mid items
    "H": (2100, 12, 4, 60, True),    # item 0 above the segment length
}


def make_case(n_users, n_items, D, min_raters, with_pref, seed=7) -> Case:
    """TRAIN edges of als_ref.make_graph; confidence 1 + 0.37 rating (not an integer), preference
    0 for rating 1 and 1 otherwise; reg varies per vertex around 0.1."""
    g = ar.make_graph(n_users, n_items, seed=seed, min_raters=min_raters)
    conf = (1.0 + 0.37 * g.obs.astype(np.float64)).astype(np.float32)
    pref = (g.obs > 1).astype(np.float32) if with_pref else None
    U0, V0 = g.factors(D, seed=11)
    reg_user = 0.1 * (1.0 + 0.25 * np.cos(np.arange(n_users)))
    reg_item = 0.1 * (1.0 + 0.25 * np.sin(np.arange(n_items)))
    return Case(n_users, n_items, D, g.user, g.item, conf, pref, reg_user, reg_item, U0, V0)


def gram_fit_case(gram_rows, seed=3) -> Case:
    """8 users x (gram_rows + 1) items, D = 5: the item Gram spans two slices.  Holds a repeated
    edge (both copies count), a user without edges and many items nobody rated."""
    rng = np.random.default_rng(seed)
    n_users, n_items, D = 8, gram_rows + 1, 5
    user = np.repeat(np.arange(1, n_users), 30)
    item = np.concatenate([rng.choice(n_items, 30, replace=False) for _ in range(1, n_users)])
    item[-1] = n_items - 1   # the last item (the second slice) is rated
    user, item = np.append(user, user[0]), np.append(item, item[0])   # a repeated edge
    conf = (1.0 + 4.0 * rng.random(len(user))).astype(np.float32)
    pref = (rng.random(len(user)) < 0.8).astype(np.float32)
    return Case(n_users, n_items, D, user.astype(np.uint32), item.astype(np.uint32), conf, pref,
                np.full(n_users, 0.1), np.full(n_items, 0.1), rng.uniform(-1, 1, (n_users, D)),
                rng.uniform(-1, 1, (n_items, D)))


_CASES, _REFS = {}, {}


def case_inputs(name) -> Case:
    if name not in _CASES:
        _CASES[name] = make_case(*CASES[name])
    return _CASES[name]


def fit_case(c: Case, n_sweeps=N_SWEEPS) -> RefResult:
    return fit(c.user, c.item, c.conf, c.pref, c.n_users, c.n_items, c.U0, c.V0, c.reg_user, c.reg_item, n_sweeps)


def case_reference(name) -> RefResult:
    """The checker's run of a case, computed once and shared (callers must not modify it)."""
    if name not in _REFS:
        _REFS[name] = fit_case(case_inputs(name))
    return _REFS[name]
