"""Checker for the ALS entry points: a plain numpy fp64 restatement of the synchronous
schedule of als.cpp (apply :313-334, scatter :343-357, signal_left :363-367), with a
per-vertex loop and np.linalg.solve.  Not a port: written from the description of the
update rule.  Also holds the deterministic graph generator the ALS tests share."""
from __future__ import annotations

from dataclasses import dataclass, field

import numpy as np


def build_csr(row, col, obs, n_rows):
    """Stable CSR of the edge list by `row`: (off uint64[n_rows + 1], col uint32, obs float32,
    perm) -- edges of one row keep their input order."""
    row = np.asarray(row, dtype=np.int64)
    perm = np.argsort(row, kind="stable")
    off = np.zeros(n_rows + 1, dtype=np.uint64)
    off[1:] = np.cumsum(np.bincount(row, minlength=n_rows))
    return off, np.asarray(col, dtype=np.uint32)[perm], np.asarray(obs, dtype=np.float32)[perm], perm


def reg_arrays(user, item, n_users, n_items, lam, regnormal, out_degree=None):
    """The value added to the diagonal per vertex.  regnormal True: lambda * num_out_edges,
    which counts every role for users and is 0 for every item (als.cpp:323-327);
    "degree": lambda * TRAIN degree on both sides; False: plain lambda."""
    du = np.bincount(np.asarray(user, dtype=np.int64), minlength=n_users).astype(np.float64)
    di = np.bincount(np.asarray(item, dtype=np.int64), minlength=n_items).astype(np.float64)
    if regnormal == "degree":
        return lam * du, lam * di
    if regnormal:
        od = du if out_degree is None else np.asarray(out_degree, dtype=np.float64)
        return lam * od, np.zeros(n_items)
    return np.full(n_users, float(lam)), np.full(n_items, float(lam))


@dataclass
class RefResult:
    U: np.ndarray
    V: np.ndarray
    nupdates_user: np.ndarray
    nupdates_item: np.ndarray
    residual_user: np.ndarray
    residual_item: np.ndarray
    supersteps: int = 0
    updates: int = 0
    margin: float = np.inf        # smallest |priority - tol| / tol seen
    min_eig_ratio: float = np.inf  # smallest lambda_min / lambda_max of a solved system
    snapshots: list = field(default_factory=list)   # (U, V) after each superstep when asked


def update_vertex(X, obs, reg):
    """One apply: X = the neighbours' factors (deg x D), obs float32.  Returns (factor, eig ratio)."""
    X = np.asarray(X, dtype=np.float64)
    A = X.T @ X
    b = X.T @ obs.astype(np.float64)
    A[np.diag_indices_from(A)] += reg
    w = np.linalg.eigvalsh(A)
    return np.linalg.solve(A, b), float(w[0] / w[-1])


def fit(user, item, obs, n_users, n_items, U0, V0, reg_user, reg_item, tol=1e-3, max_updates=None,
        max_supersteps=0, activate_user=None, nupdates=None, residual=None, keep_snapshots=False) -> RefResult:
    D = U0.shape[1]
    F = [np.array(U0, dtype=np.float64), np.array(V0, dtype=np.float64)]
    n = [n_users, n_items]
    reg = [np.asarray(reg_user, dtype=np.float64), np.asarray(reg_item, dtype=np.float64)]
    csr = [build_csr(user, item, obs, n_users)[:3], build_csr(item, user, obs, n_items)[:3]]
    nupd = [np.zeros(n_users, np.uint32), np.zeros(n_items, np.uint32)] if nupdates is None else \
        [np.array(nupdates[0], np.uint32), np.array(nupdates[1], np.uint32)]
    res = [np.zeros(n_users, np.float32), np.zeros(n_items, np.float32)] if residual is None else \
        [np.array(residual[0], np.float32), np.array(residual[1], np.float32)]
    cap = np.inf if max_updates is None else max_updates
    active = np.ones(n_users, bool) if activate_user is None else np.asarray(activate_user).astype(bool)
    out = RefResult(F[0], F[1], nupd[0], nupd[1], res[0], res[1])
    k = 0
    while active.any() and not (max_supersteps and out.supersteps >= max_supersteps):
        off, nbr, ob = csr[k]
        o = 1 - k
        verts = np.flatnonzero(active)
        for v in verts:
            b, e = int(off[v]), int(off[v + 1])
            if e == b:   # no TRAIN edge: residual 0, one more update, factor untouched
                res[k][v] = 0.0
                nupd[k][v] += 1
                continue
            new, ratio = update_vertex(F[o][nbr[b:e]], ob[b:e], reg[k][v])
            out.min_eig_ratio = min(out.min_eig_ratio, ratio)
            res[k][v] = np.float32(np.abs(new - F[k][v]).sum() / D)
            F[k][v] = new
            nupd[k][v] += 1
        nxt = np.zeros(n[o], bool)
        for v in verts:
            b, e = int(off[v]), int(off[v + 1])
            if e == b:
                continue
            others = nbr[b:e]
            pred = F[o][others] @ F[k][v]
            error = np.abs(ob[b:e].astype(np.float64) - pred).astype(np.float32)
            priority = (error * np.float32(res[k][v])).astype(np.float64)   # a float product
            if tol > 0:
                out.margin = min(out.margin, float(np.min(np.abs(priority - tol) / tol)))
            nxt[others[(priority > tol) & (nupd[o][others] < cap)]] = True
        out.supersteps += 1
        out.updates += len(verts)
        if keep_snapshots:
            out.snapshots.append((F[0].copy(), F[1].copy()))
        active = nxt
        k = o
    return out


def sum_sq_error(user, item, obs, U, V, minval, maxval):
    pred = np.einsum("ij,ij->i", U[np.asarray(user, np.int64)], V[np.asarray(item, np.int64)])
    pred = np.maximum(minval, np.minimum(maxval, pred))
    return float(np.sum((np.asarray(obs, np.float32).astype(np.float64) - pred) ** 2))


# ---- the shared graph generator ---------------------------------------------------------

@dataclass
class Graph:
    n_users: int
    n_items: int
    user: np.ndarray        # TRAIN edges
    item: np.ndarray
    obs: np.ndarray
    vuser: np.ndarray       # VALIDATE edges
    vitem: np.ndarray
    vobs: np.ndarray
    out_degree: np.ndarray  # per user, every role

    def factors(self, D, seed=11):
        rng = np.random.default_rng(seed)
        return rng.uniform(-1, 1, (self.n_users, D)), rng.uniform(-1, 1, (self.n_items, D))


def make_graph(n_users, n_items, seed=7, min_raters=0) -> Graph:
    """Power-law item popularity; item 0 rated by every user that has edges, the last item by
    nobody; user 0 without edges, user 1 with exactly one TRAIN edge, user 2 with VALIDATE
    edges only; about 15 % of the other edges VALIDATE; integer ratings 1..5."""
    rng = np.random.default_rng(seed)
    pop = 1.0 / np.arange(1, n_items) ** 0.7   # items 0 .. n_items-2; the last item stays empty
    want = np.maximum(min_raters, np.round(pop / pop[0] * (n_users - 3)).astype(int))
    eu, ei, role = [], [], []
    for i in range(n_items - 1):
        cand = np.arange(3, n_users)
        raters = cand if i == 0 else rng.choice(cand, size=min(len(cand), int(want[i])), replace=False)
        for u in np.sort(raters):
            eu.append(int(u))
            ei.append(i)
            role.append(0)
    eu, ei, role = np.array(eu), np.array(ei), np.array(role)
    role[rng.random(len(role)) < 0.15] = 1
    # every user >= 3 keeps at least one TRAIN edge: its item-0 edge
    role[(ei == 0)] = 0
    eu = np.concatenate([eu, [1, 2, 2, 2]])
    ei = np.concatenate([ei, [0, 0, 1, 2]])
    role = np.concatenate([role, [0, 1, 1, 1]])
    perm = rng.permutation(len(eu))   # edges arrive in no particular order
    eu, ei, role = eu[perm], ei[perm], role[perm]
    r = rng.integers(1, 6, len(eu)).astype(np.float32)
    t, v = role == 0, role == 1
    od = np.bincount(eu, minlength=n_users)
    return Graph(n_users, n_items, eu[t].astype(np.uint32), ei[t].astype(np.uint32), r[t],
                 eu[v].astype(np.uint32), ei[v].astype(np.uint32), r[v], od)


CASES = {
    # name: (users, items, D, regnormal, lambda, tol, max_updates, min raters per item)
    "A": (96, 40, 20, "degree", 0.05, 1e-3, 6, 0),
    "B": (96, 40, 33, False, 0.1, 1e-3, 4, 0),
    "C": (200, 12, 4, True, 0.01, 1e-3, 5, 60),
    "D": (96, 40, 20, "degree", 0.05, 1e-3, None, 0),
    "E": (96, 40, 13, "degree", 0.05, 1e-3, 6, 0),       # D = 9..16: the kernels' DP = 16 tier
}


def case_inputs(name):
    nu, ni, D, regn, lam, tol, mu, minr = CASES[name]
    g = make_graph(nu, ni, seed=7, min_raters=minr)
    U0, V0 = g.factors(D, seed=11)
    ru, ri = reg_arrays(g.user, g.item, nu, ni, lam, regn, g.out_degree)
    return g, U0, V0, ru, ri, tol, mu


_REF_CACHE = {}


def case_reference(name) -> RefResult:
    """The checker's run of a case, computed once and shared (callers must not modify it)."""
    if name not in _REF_CACHE:
        g, U0, V0, ru, ri, tol, mu = case_inputs(name)
        _REF_CACHE[name] = fit(g.user, g.item, g.obs, g.n_users, g.n_items, U0, V0, ru, ri, tol=tol,
                               max_updates=mu, activate_user=g.out_degree > 0, keep_snapshots=True)
    return _REF_CACHE[name]
