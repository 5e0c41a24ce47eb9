"""Checker for the KL-divergence NMF entry points (cf_nmf_fit / cf_nmf_loss): plain numpy fp64,
written from the model's equations as weighted NMF over the dense grid.  It does NOT use the
column-sum trick and does not walk edge lists: it forms the dense n_users x n_items matrices
    R   the ratings, summed per pair (0 without an edge; repeated edges each count)
    W   the weight of the pair's prediction: the number of its edges (OBSERVED), or 1 everywhere (GRID)
    P   U V^T
and updates a whole side by   F <- F * ((R / P) X) / (W X)   with X the other side, so a GRID
denominator is the product of a matrix of ones with X and an OBSERVED one of the edge-count
matrix with X.  The loss is
    sum_grid [W P - R log P] + sum_edges [r log r - r]      (0 log 0 = 0)
which is sum_edges [r log(r / p) - r] + sum_grid W P term by term.
A vertex without edges has W = 0 on its whole OBSERVED row: it is left as it is.  After the rule a
value below EPS becomes EPS.  Also holds the cases the GPU tests share."""
from __future__ import annotations

from dataclasses import dataclass, field

import numpy as np

EPS = 1e-16
OBSERVED, GRID = "observed", "grid"
MODES = (OBSERVED, GRID)


def dense(user, item, obs, n_users, n_items, mode):
    """(R, W, C, sum over the edges of r log r, sum over the edges of r); C counts the edges of a pair."""
    user, item = np.asarray(user, np.int64), np.asarray(item, np.int64)
    r = np.asarray(obs, np.float32).astype(np.float64)
    R, C = np.zeros((n_users, n_items)), np.zeros((n_users, n_items))
    np.add.at(R, (user, item), r)
    np.add.at(C, (user, item), 1.0)
    W = np.ones((n_users, n_items)) if mode == GRID else C
    pos = r[r > 0]
    return R, W, C, float(np.sum(pos * np.log(pos))), float(np.sum(r))


def _xlogp(R, P):
    out = np.zeros_like(R)
    m = R > 0
    out[m] = R[m] * np.log(P[m])
    return out


def dense_loss(R, W, rlogr, rsum, U, V):
    """(loss, sum of the absolute values of its terms)."""
    P = U @ V.T
    x = _xlogp(R, P)
    return float(np.sum(W * P) - np.sum(x) + rlogr - rsum), float(np.sum(W * P) + np.sum(np.abs(x)) + abs(rlogr) + rsum)


def loss(user, item, obs, n_users, n_items, U, V, mode):
    R, W, _, rlogr, rsum = dense(user, item, obs, n_users, n_items, mode)
    return dense_loss(R, W, rlogr, rsum, np.asarray(U, np.float64), np.asarray(V, np.float64))


def edge_loss(user, item, obs, U, V, mode):
    """The form the kernels use: the edge terms, plus s_U . s_V in GRID mode."""
    user, item = np.asarray(user, np.int64), np.asarray(item, np.int64)
    r = np.asarray(obs, np.float32).astype(np.float64)
    p = np.einsum("ij,ij->i", U[user], V[item])
    m = r > 0
    t = np.zeros_like(r)
    t[m] = r[m] * np.log(r[m] / p[m]) - r[m]
    if mode == GRID:
        return float(np.sum(t) + U.sum(0) @ V.sum(0))
    return float(np.sum(t + p))


@dataclass
class RefResult:
    U: np.ndarray
    V: np.ndarray
    loss_trace: np.ndarray       # after each half-sweep
    n_floored: int
    loss_scale: float            # the largest sum of |terms| of a trace entry
    prefloor: np.ndarray = field(repr=False, default=None)   # every value the rule produced, before the floor


def fit(user, item, obs, n_users, n_items, U0, V0, mode, n_sweeps) -> RefResult:
    R, W, C, rlogr, rsum = dense(user, item, obs, n_users, n_items, mode)
    U, V = np.array(U0, dtype=np.float64), np.array(V0, dtype=np.float64)
    trace, pre_all, floored, scale = [], [], 0, 0.0
    has_u, has_i = C.sum(1) > 0, C.sum(0) > 0
    if mode == GRID:
        has_u, has_i = np.ones(n_users, bool), np.ones(n_items, bool)
    for _ in range(n_sweeps):
        for side in (0, 1):
            if side == 0:
                U, pre, nf = _side(U, V, R, W, has_u)
            else:
                V, pre, nf = _side(V, U, R.T, W.T, has_i)
            floored += nf
            pre_all.append(pre)
            l, s = dense_loss(R, W, rlogr, rsum, U, V)
            trace.append(l)
            scale = max(scale, s)
    return RefResult(U, V, np.array(trace), floored, scale, np.concatenate(pre_all) if pre_all else np.zeros(0))


def _side(F, X, R, W, run):
    P = F @ X.T
    num, den = (R / P) @ X, W @ X
    new = F.copy()
    with np.errstate(invalid="ignore", divide="ignore"):
        val = F * num / den
    pre = val[run]
    new[run] = np.where(pre < EPS, EPS, pre)
    return new, pre.ravel(), int(np.sum(pre < EPS))


# ---- the shared cases -----------------------------------------------------------------------

@dataclass
class Case:
    n_users: int
    n_items: int
    D: int
    user: np.ndarray
    item: np.ndarray
    obs: np.ndarray
    U0: np.ndarray
    V0: np.ndarray
    n_sweeps: int = 2


def _factors(rng, n_users, n_items, D):
    return rng.uniform(0.1, 1.0, (n_users, D)), rng.uniform(0.1, 1.0, (n_items, D))


def make_graph_a(D, integer, seed=5) -> Case:
    """72 users x 30 items (an item must have more than 64 raters to leave the wave path, so "about
    50 users" is not enough).  Item 0 is rated by users 2..69 (68 raters: the workgroup path), the
    other items by a few users each (the wave path), item 29 by nobody; user 0 has no edges; every
    rating of user 1 is 0; user 2's edge to item 0 is there twice; user 3 has 11 edges (a partial
    lane group).  Ratings: integers 0..5, or (integer = False) 0.25 + 4.5 u."""
    rng = np.random.default_rng(seed)
    n_users, n_items = 72, 30
    user, item = [], []
    for u in range(1, n_users):
        k = 11 if u == 3 else int(rng.integers(3, 9))
        its = rng.choice(np.arange(1, n_items - 1), size=k - (2 <= u < 70), replace=False)
        if 2 <= u < 70:
            its = np.append(its, 0)
        user += [u] * len(its)
        item += list(its)
    user, item = np.array(user), np.array(item)
    obs = rng.integers(0, 6, len(user)).astype(np.float64) if integer else 0.25 + 4.5 * rng.random(len(user))
    obs[user == 1] = 0.0
    first = int(np.flatnonzero((user == 2) & (item == 0))[0])
    user, item, obs = np.append(user, 2), np.append(item, 0), np.append(obs, obs[first] if integer else 1.75)
    perm = rng.permutation(len(user))
    U0, V0 = _factors(rng, n_users, n_items, D)
    return Case(n_users, n_items, D, user[perm].astype(np.uint32), item[perm].astype(np.uint32),
                obs[perm].astype(np.float32), U0, V0)


def make_graph_d(D, seed=9) -> Case:
    """12 x 10, every user rates 3 to 6 items: the D sweep."""
    rng = np.random.default_rng(seed)
    user, item = [], []
    for u in range(12):
        its = rng.choice(10, size=int(rng.integers(3, 7)), replace=False)
        user += [u] * len(its)
        item += list(its)
    obs = rng.integers(0, 6, len(user)).astype(np.float32)
    U0, V0 = _factors(rng, 12, 10, D)
    return Case(12, 10, D, np.array(user, np.uint32), np.array(item, np.uint32), obs, U0, V0)


def make_graph_h(seg=2048, seed=13) -> Case:
    """seg + 52 users x 8 items, D = 5: item 0 is rated by every user (above the segment length and
    not a multiple of it), items 1..6 by 60 users each, item 7 by nobody."""
    rng = np.random.default_rng(seed)
    n_users, n_items, D = seg + 52, 8, 5
    user = [np.arange(n_users)] + [rng.choice(n_users, 60, replace=False) for _ in range(1, 7)]
    item = [np.full(len(x), i) for i, x in enumerate(user)]
    user, item = np.concatenate(user), np.concatenate(item)
    obs = rng.integers(0, 6, len(user)).astype(np.float32)
    perm = rng.permutation(len(user))
    U0, V0 = _factors(rng, n_users, n_items, D)
    return Case(n_users, n_items, D, user[perm].astype(np.uint32), item[perm].astype(np.uint32), obs[perm], U0, V0)


def make_graph_s(sum_rows=1024, seed=3) -> Case:
    """8 users x (sum_rows + 1) items, D = 5: the column sum over the items has two slices, the
    second of one row.  Users 1..7 rate 30 items each, the last item among them; user 0 nothing."""
    rng = np.random.default_rng(seed)
    n_users, n_items, D = 8, sum_rows + 1, 5
    user = np.repeat(np.arange(1, n_users), 30)
    item = np.concatenate([rng.choice(n_items, 30, replace=False) for _ in range(1, n_users)])
    item[-1] = n_items - 1 if n_items - 1 not in item[-30:] else item[-1]
    obs = rng.integers(0, 6, len(user)).astype(np.float32)
    U0, V0 = _factors(rng, n_users, n_items, D)
    return Case(n_users, n_items, D, user.astype(np.uint32), item.astype(np.uint32), obs, U0, V0)


D_SWEEP = (1, 8, 9, 16, 17, 24, 25, 32, 33, 64)

_MAKERS = {"A": lambda: make_graph_a(5, True), "B": lambda: make_graph_a(20, False), "H": make_graph_h,
           "S": make_graph_s}
_MAKERS.update({f"D{d}": (lambda d=d: make_graph_d(d)) for d in D_SWEEP})
CASES = tuple(_MAKERS)

_CASES, _REFS = {}, {}


def case_inputs(name) -> Case:
    if name not in _CASES:
        _CASES[name] = _MAKERS[name]()
    return _CASES[name]


def fit_case(c: Case, mode, n_sweeps=None) -> RefResult:
    return fit(c.user, c.item, c.obs, c.n_users, c.n_items, c.U0, c.V0, mode, c.n_sweeps if n_sweeps is None else n_sweeps)


def case_reference(name, mode) -> RefResult:
    """The checker's run of a case, computed once and shared (callers must not modify it)."""
    if (name, mode) not in _REFS:
        _REFS[name, mode] = fit_case(case_inputs(name), mode)
    return _REFS[name, mode]
