"""Checker for the BPR entry points (cf_bpr_fit / cf_bpr_sample): plain numpy fp64 and python-int
hashing, written from the contract in include/cf_abi.h.

The sample.  sm is splitmix64 (host/cf_mf_cli.hpp).  For sweep s, user u and the edge at rank r of
u's ascending item list, with T = TRIES:
    key_s = sm(sm(seed) ^ s);  h(t) = sm(sm(key_s ^ u) ^ (r T + t));  cand(t) = ((h(t) >> 32) n_items) >> 32
and the negative j is the first cand(t), t < T, that is not in u's list; none: the edge is skipped.

A sweep (every value as it was at its start), over the triples (u, i, j):
    x = U_u . (V_i - V_j) + b_i - b_j,   g = 1 / (1 + exp(x))
    U_u += lr ((sum g (V_i - V_j)) / c_u - reg_user U_u)
    V_i += lr ((sum_{i positive} g U_u - sum_{i negative} g U_u) / c_i - reg_item V_i),  b_i alike with 1 for U_u
with c the vertex's number of triples (an item: as the positive plus as the negative); a vertex with
c = 0 keeps its row.  The sums are np.add.at over the triples in user-CSR order.  Trace row s:
(sum of softplus(-x), number of triples), from the start-of-sweep factors.

Also holds the cases the GPU tests share (CASES, case_inputs, case_reference)."""
from __future__ import annotations

from dataclasses import dataclass, field

import numpy as np

TRIES = 8
MAX = 0xFFFFFFFF
M64 = (1 << 64) - 1


def sm(x: int) -> int:
    x = (x + 0x9E3779B97F4A7C15) & M64
    x = ((x ^ (x >> 30)) * 0xBF58476D1CE4E5B9) & M64
    x = ((x ^ (x >> 27)) * 0x94D049BB133111EB) & M64
    return x ^ (x >> 31)


def sort_pairs(user, item):
    """The positive pairs by (user, item), without repeats: the order of the user CSR."""
    user, item = np.asarray(user, np.int64), np.asarray(item, np.int64)
    p = np.lexsort((item, user))
    user, item = user[p], item[p]
    if len(user) > 1:
        keep = np.concatenate(([True], (user[1:] != user[:-1]) | (item[1:] != item[:-1])))
        user, item = user[keep], item[keep]
    return user, item


def sample(user, item, n_users, n_items, seed, sweep, tries=TRIES):
    """neg[p] for every position p of the user CSR of the sorted pairs (MAX = skipped)."""
    user, item = sort_pairs(user, item)
    neg = np.full(len(user), MAX, dtype=np.uint32)
    key = sm(sm(int(seed)) ^ int(sweep))
    start = np.searchsorted(user, np.arange(n_users + 1))
    for u in range(n_users):
        b, e = int(start[u]), int(start[u + 1])
        if b == e:
            continue
        mine = set(int(i) for i in item[b:e])
        ku = sm(key ^ u)
        for r in range(e - b):
            for t in range(tries):
                c = (((sm(ku ^ (r * tries + t)) >> 32) * n_items) >> 32) & 0xFFFFFFFF
                if c not in mine:
                    neg[b + r] = c
                    break
    return neg


def softplus(z):
    """log(1 + exp(z)) without overflow."""
    return np.maximum(z, 0.0) + np.log1p(np.exp(-np.abs(z)))


@dataclass
class Case:
    n_users: int
    n_items: int
    D: int
    user: np.ndarray      # the positive pairs, sorted by (user, item)
    item: np.ndarray
    U0: np.ndarray
    V0: np.ndarray
    bias0: np.ndarray | None
    n_sweeps: int
    lr: float
    reg: float
    seed: int


@dataclass
class Fit:
    U: np.ndarray
    V: np.ndarray
    bias: np.ndarray | None
    loss_trace: np.ndarray            # n_sweeps x 2
    triples: int
    n_skipped: int
    n_nan: int
    skipped_per_sweep: list = field(default_factory=list)
    user_counted: np.ndarray = None   # the vertex had a triple in some sweep
    item_counted: np.ndarray = None
    item_negative: np.ndarray = None  # the item was a negative in some sweep


def fit(c: Case, *, n_sweeps=None, first_sweep=0, U0=None, V0=None, bias0=None, jitter=None) -> Fit:
    """jitter: a numpy Generator; then the triples of every sweep are summed in a random order and
    every g moves by up to 2 ulp (tools/bpr_drift.py)."""
    n_sweeps = c.n_sweeps if n_sweeps is None else n_sweeps
    U = np.array(c.U0 if U0 is None else U0, dtype=np.float64)
    V = np.array(c.V0 if V0 is None else V0, dtype=np.float64)
    b_in = c.bias0 if bias0 is None else bias0
    b = None if b_in is None else np.array(b_in, dtype=np.float64)
    trace = np.zeros((n_sweeps, 2))
    out = Fit(U, V, b, trace, 0, 0, 0, [], np.zeros(c.n_users, bool), np.zeros(c.n_items, bool), np.zeros(c.n_items, bool))
    for k in range(n_sweeps):
        neg = sample(c.user, c.item, c.n_users, c.n_items, c.seed, first_sweep + k)
        ok = neg != MAX
        u, i, j = c.user[ok], c.item[ok], neg[ok].astype(np.int64)
        if jitter is not None:
            p = jitter.permutation(len(u))
            u, i, j = u[p], i[p], j[p]
        dV = V[i] - V[j]
        x = np.einsum("ij,ij->i", U[u], dV)
        if b is not None:
            x = x + (b[i] - b[j])
        g = 1.0 / (1.0 + np.exp(x))
        if jitter is not None:
            g = g + jitter.integers(-2, 3, len(g)) * np.spacing(g)
        trace[k] = (float(np.sum(softplus(-x))), float(len(u)))
        out.triples += len(u)
        out.n_skipped += int((~ok).sum())
        out.skipped_per_sweep.append(int((~ok).sum()))
        out.n_nan += int(np.isnan(x).sum())
        cu = np.bincount(u, minlength=c.n_users).astype(np.float64)
        ci = (np.bincount(i, minlength=c.n_items) + np.bincount(j, minlength=c.n_items)).astype(np.float64)
        out.user_counted |= cu > 0
        out.item_counted |= ci > 0
        out.item_negative |= np.bincount(j, minlength=c.n_items) > 0
        GU, GV, Gb = np.zeros_like(U), np.zeros_like(V), np.zeros(c.n_items)
        np.add.at(GU, u, g[:, None] * dV)
        np.add.at(GV, i, g[:, None] * U[u])
        np.add.at(GV, j, -g[:, None] * U[u])
        np.add.at(Gb, i, g)
        np.add.at(Gb, j, -g)
        mu, mi = cu > 0, ci > 0
        U[mu] += c.lr * (GU[mu] / cu[mu, None] - c.reg * U[mu])
        V[mi] += c.lr * (GV[mi] / ci[mi, None] - c.reg * V[mi])
        if b is not None:
            b[mi] += c.lr * (Gb[mi] / ci[mi] - c.reg * b[mi])
        if out.n_nan:
            out.loss_trace = trace[: k + 1]
            break
    return out


def train_auc(c: Case, U, V, bias):
    """(mean AUC, ranks) of the positive pairs among all items, by tests/rank_ref.py: every positive
    of a user against the user's complement, nothing excluded."""
    import rank_ref as rr

    rank, _, _, s = rr.evaluate(U, V, 10, (c.user, c.item), bias_item=bias)
    return s["auc"], rank


# ---- the cases ------------------------------------------------------------------------------

def planted_graph():
    """60 users x 40 items in 4 clusters; user 0 rates everything, user 1 everything but item 17."""
    rng = np.random.default_rng(11)
    nu, ni = 60, 40
    cu, ci = rng.integers(0, 4, nu), rng.integers(0, 4, ni)
    A = rng.random((nu, ni)) < np.where(cu[:, None] == ci[None, :], 0.5, 0.05)
    A[0] = True
    A[1] = True
    A[1, 17] = False
    user, item = np.nonzero(A)
    return nu, ni, user.astype(np.int64), item.astype(np.int64)


def _init(seed, nu, ni, D, bias=True):
    rng = np.random.default_rng(seed)
    return rng.uniform(-0.1, 0.1, (nu, D)), rng.uniform(-0.1, 0.1, (ni, D)), (np.zeros(ni) if bias else None)


D_SWEEP = (1, 5, 20, 33, 64)
NO_BIAS = "D20"
# name: (n_items, edges, seed): edges and n_items + 1 = 256 and 257; the seeds draw no negative at
# item 0 or at the last item in sweep 0 (test_bpr_ref.py)
T_CASES = {"T256": (255, 256, 1), "T257": (256, 257, 1)}
CASES = ("P",) + tuple(f"D{d}" for d in D_SWEEP) + ("M", "N", "E") + tuple(T_CASES)
SEG, LOW = 2048, 64   # the cuts the cases are built around; test_bpr_ref.py checks them against the library


def _make(name) -> Case:
    if name == "P" or name.startswith("D"):
        nu, ni, user, item = planted_graph()
        D, sweeps = (8, 40) if name == "P" else (int(name[1:]), 3)
        U0, V0, b0 = _init(3 + D, nu, ni, D, bias=name != NO_BIAS)
        return Case(nu, ni, D, user, item, U0, V0, b0, sweeps, 2.0, 0.01, 5)
    if name == "M":   # user 0 in the workgroup class, user 1 in the segment class
        rng = np.random.default_rng(12)
        nu, ni = 14, 2 * SEG + 200
        lists = [rng.choice(ni, 100, replace=False), rng.choice(ni, SEG + 251, replace=False)]
        lists += [rng.choice(ni, int(rng.integers(1, 9)), replace=False) for _ in range(nu - 2)]
        user = np.concatenate([np.full(len(x), k) for k, x in enumerate(lists)])
        user, item = sort_pairs(user, np.concatenate(lists))
        U0, V0, b0 = _init(13, nu, ni, 9)
        return Case(nu, ni, 9, user, item, U0, V0, b0, 2, 1.0, 0.01, 6)
    if name == "N":   # item 0: a positive list above the segment length; item 1: about as many negatives
        nu, ni = 4200, 2
        user = np.concatenate([np.arange(nu), np.arange(50)])
        user, item = sort_pairs(user, np.concatenate([np.zeros(nu, np.int64), np.ones(50, np.int64)]))
        U0, V0, b0 = _init(14, nu, ni, 4)
        return Case(nu, ni, 4, user, item, U0, V0, b0, 3, 1.0, 0.01, 7)
    if name == "E":   # users 5, 6 and items 5.. without edges; few draws over many items
        nu, ni = 7, 40
        user = np.array([0, 0, 0, 1, 1, 2, 3, 3, 4, 4])
        item = np.array([0, 1, 2, 1, 3, 4, 0, 4, 2, 3])
        user, item = sort_pairs(user, item)
        U0, V0, b0 = _init(15, nu, ni, 3)
        return Case(nu, ni, 3, user, item, U0, V0, b0, 2, 1.0, 0.01, 8)
    if name in T_CASES:   # the negative lists at the edges of the 256-thread workgroups that build them
        ni, nnz, seed = T_CASES[name]
        rng = np.random.default_rng(16)
        nu = 200
        flat = np.sort(rng.choice(nu * (ni - 2), nnz, replace=False))   # items 0 and ni - 1 have no edge
        user, item = sort_pairs(flat // (ni - 2), flat % (ni - 2) + 1)
        U0, V0, b0 = _init(17, nu, ni, 4)
        return Case(nu, ni, 4, user, item, U0, V0, b0, 2, 1.0, 0.01, seed)
    raise KeyError(name)


_INPUTS, _REFS = {}, {}


def case_inputs(name) -> Case:
    if name not in _INPUTS:
        _INPUTS[name] = _make(name)
    return _INPUTS[name]


def case_reference(name) -> Fit:
    """The checker's fit of a case, computed once and shared (not modified by the tests)."""
    if name not in _REFS:
        _REFS[name] = fit(case_inputs(name))
    return _REFS[name]
