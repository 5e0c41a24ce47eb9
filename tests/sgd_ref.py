"""Checker for the SGD / bias-SGD entry points: a plain numpy fp64 restatement of the
synchronous schedule (user supersteps 0, 2, .., item supersteps 1, 3, ..) written from the
description of the update rule in include/cf_abi.h, with a per-vertex loop and the reference's
per-edge form of the delta, -gamma (err x + lambda own) summed over the edges.  Not a port.
The graph generator and build_csr are those of als_ref.py."""
from __future__ import annotations

from dataclasses import dataclass, field

import numpy as np

from als_ref import build_csr, make_graph


@dataclass
class SgdRef:
    U: np.ndarray
    V: np.ndarray
    bias_user: np.ndarray | None
    bias_item: np.ndarray | None
    nupdates_user: np.ndarray
    nupdates_item: np.ndarray
    supersteps: int = 0
    updates: int = 0
    messages: int = 0          # edges with u active and |err| > tol whose item was signalled
    silent: int = 0            # edges with u active whose |err| <= tol (did not send)
    n_nan: int = 0
    gamma_next: float = 0.0
    thr_margin: float = np.inf    # smallest ||err| - tol| / tol seen
    round_margin: float = np.inf  # smallest distance of p - obs to a float midpoint, in float ulps
    trace: list = field(default_factory=list)       # [sum sq TRAIN, sum sq VALIDATE] per user superstep
    snapshots: list = field(default_factory=list)   # (U, V, bu, bi) after every superstep


def predict(user, item, U, V, bu=None, bi=None, mean=0.0, minval=None, maxval=None):
    user, item = np.asarray(user, np.int64), np.asarray(item, np.int64)
    p = np.einsum("ij,ij->i", U[user], V[item])
    if bu is not None:
        p = mean + bu[user] + bi[item] + p
    if minval is not None:
        p = np.maximum(minval, np.minimum(maxval, p))
    return p


def sum_sq_error(user, item, obs, U, V, bu=None, bi=None, mean=0.0, minval=-1e100, maxval=1e100):
    p = predict(user, item, U, V, bu, bi, mean, minval, maxval)
    return float(np.sum((np.asarray(obs, np.float32).astype(np.float64) - p) ** 2))


def _errors(own, own_b, X, Xb, ob, mean, minval, maxval, bias, out):
    """err per edge of one vertex: float32 of clamp(mean + biases + X . own) - obs, as float64."""
    p = X @ own
    if bias:
        p = mean + own_b + Xb + p
    p = np.where(p > maxval, maxval, p)
    p = np.where(p < minval, minval, p)
    d = p - ob.astype(np.float64)
    f = d.astype(np.float32)
    ok = np.isfinite(d)
    if ok.any():
        ulp = np.spacing(np.abs(f[ok])).astype(np.float64)
        out.round_margin = min(out.round_margin, float(np.min(0.5 - np.abs(d[ok] - f[ok].astype(np.float64)) / ulp)))
    return f.astype(np.float64)


def fit(user, item, obs, n_users, n_items, U0, V0, *, lam, gamma, step_dec, tol, minval, maxval, bias=False,
        mean=0.0, bias_user=None, bias_item=None, max_updates=None, max_supersteps=0, activate_user=None,
        validate=None, keep_snapshots=False) -> SgdRef:
    assert max_updates is not None or max_supersteps, "the run would never end"
    U, V = np.array(U0, dtype=np.float64), np.array(V0, dtype=np.float64)
    bu = bi = None
    if bias:
        bu = np.zeros(n_users) if bias_user is None else np.array(bias_user, dtype=np.float64)
        bi = np.zeros(n_items) if bias_item is None else np.array(bias_item, dtype=np.float64)
    uoff, uitem, uobs, _ = build_csr(user, item, obs, n_users)
    ioff, iuser, iobs, _ = build_csr(item, user, obs, n_items)
    nup_u, nup_i = np.zeros(n_users, np.uint32), np.zeros(n_items, np.uint32)
    cap = np.inf if max_updates is None else max_updates
    active = np.ones(n_users, bool) if activate_user is None else np.asarray(activate_user).astype(bool)
    out = SgdRef(U, V, bu, bi, nup_u, nup_i, gamma_next=float(gamma))
    g = float(gamma)

    def snap():
        if keep_snapshots:
            out.snapshots.append((U.copy(), V.copy(), None if bu is None else bu.copy(), None if bi is None else bi.copy()))

    while active.any() and not (max_supersteps and out.supersteps >= max_supersteps):
        Uo, Vo = U.copy(), V.copy()
        buo, bio = (bu.copy(), bi.copy()) if bias else (None, None)
        # ---- user superstep ----
        signalled = np.zeros(n_items, bool)
        for u in np.flatnonzero(active):
            b, e = int(uoff[u]), int(uoff[u + 1])
            its = uitem[b:e].astype(np.int64)
            if e > b:
                err = _errors(Uo[u], buo[u] if bias else 0.0, Vo[its], bio[its] if bias else 0.0, uobs[b:e], mean,
                              minval, maxval, bias, out)
                out.n_nan += int(np.isnan(err).sum())
                if tol > 0:
                    fin = np.abs(err[np.isfinite(err)])
                    if len(fin):
                        out.thr_margin = min(out.thr_margin, float(np.min(np.abs(fin - tol) / tol)))
                U[u] = Uo[u] + (-g * (err[:, None] * Vo[its] + lam * Uo[u])).sum(axis=0)
                if bias:
                    bu[u] = buo[u] + (-g * (err + lam * buo[u])).sum()
                signalled[its[nup_i[its] < cap]] = True
            nup_u[u] += 1
        # the items' messages, from the same old values
        msg = np.zeros_like(V)
        msg_b = np.zeros(n_items)
        for i in np.flatnonzero(signalled):
            b, e = int(ioff[i]), int(ioff[i + 1])
            us = iuser[b:e].astype(np.int64)
            sel = active[us]
            us, ob = us[sel], iobs[b:e][sel]
            err = _errors(Vo[i], bio[i] if bias else 0.0, Uo[us], buo[us] if bias else 0.0, ob, mean, minval, maxval,
                          bias, out)
            send = np.abs(err) > tol
            out.messages += int(send.sum())
            out.silent += int((~send).sum())
            msg[i] = (-g * (err[send, None] * Uo[us[send]] + lam * Vo[i])).sum(axis=0)
            if bias:
                msg_b[i] = (-g * (err[send] + lam * bio[i])).sum()
        out.supersteps += 1
        out.updates += int(active.sum())
        g *= step_dec
        out.gamma_next = g
        row = [sum_sq_error(user, item, obs, U, V, bu, bi, mean, minval, maxval), 0.0]
        if validate is not None and len(validate[0]):
            row[1] = sum_sq_error(validate[0], validate[1], validate[2], U, V, bu, bi, mean, minval, maxval)
        out.trace.append(row)
        snap()
        if out.n_nan or not signalled.any() or (max_supersteps and out.supersteps >= max_supersteps):
            break   # numeric errors; nobody signalled; or cut here: the pending messages are dropped
        # ---- item superstep ----
        nxt = np.zeros(n_users, bool)
        for i in np.flatnonzero(signalled):
            V[i] = V[i] + msg[i]
            if bias:
                bi[i] = bi[i] + msg_b[i]
            nup_i[i] += 1
            us = iuser[int(ioff[i]):int(ioff[i + 1])].astype(np.int64)
            nxt[us[nup_u[us] < cap]] = True
        out.supersteps += 1
        out.updates += int(signalled.sum())
        snap()
        active = nxt
    return out


# ---- the cases the CPU and GPU tests share ------------------------------------------------

CASES = {
    # name: (users, items, D, min raters per item, max_updates)
    "A": (96, 40, 20, 0, 6),
    "B": (96, 40, 33, 0, 4),
    "C": (200, 12, 4, 60, 5),
    "E": (96, 40, 64, 0, 4),
    # the shape of "C" (items on the workgroup path) in the two D tiers the others leave out:
    # 9..16 (two row elements per lane) and 25..32 (four).  13, not 12: at D = 12 none of the 50
    # pairs that the GPU prediction tests draw is clamped with biases, which they require
    "F": (200, 12, 13, 60, 3),
    "G": (200, 12, 28, 60, 3),
}
HYPER = dict(lam=0.05, gamma=0.02, step_dec=0.9, tol=0.5, minval=1.0, maxval=5.0)
KEYS = [(name, bias) for name in CASES for bias in (False, True)]


def case_inputs(name):
    nu, ni, D, minr, mu = CASES[name]
    g = make_graph(nu, ni, seed=7, min_raters=minr)
    U0, V0 = g.factors(D, seed=11)
    return g, U0, V0, mu


def train_mean(obs):
    return float(np.asarray(obs, np.float32).astype(np.float64).sum() / len(obs))


def run_case(name, bias, *, g=None, U0=None, V0=None, **over):
    g0, U00, V00, mu = case_inputs(name)
    g = g0 if g is None else g
    kw = dict(HYPER, bias=bias, mean=train_mean(g.obs) if bias else 0.0, max_updates=mu,
              activate_user=g.out_degree > 0, validate=(g.vuser, g.vitem, g.vobs), keep_snapshots=True)
    kw.update(over)
    return fit(g.user, g.item, g.obs, g.n_users, g.n_items, U00 if U0 is None else U0, V00 if V0 is None else V0, **kw)


_REF_CACHE = {}


def case_reference(name, bias) -> SgdRef:
    """The checker's run of a case, computed once and shared (callers must not modify it)."""
    if (name, bias) not in _REF_CACHE:
        _REF_CACHE[(name, bias)] = run_case(name, bias)
    return _REF_CACHE[(name, bias)]


def segmented_problem(seg, low_max):
    """Item 0 is rated by every one of seg + 52 users (one full segment and a tail: high class),
    item 1 by low_max + 30 users (mid class); user 0 rates all low_max + 6 items (mid class on
    the user side), every other item has user 0 and two more raters.
    Returns (user, item, obs, n_users, n_items)."""
    n_users, n_items = seg + 52, low_max + 6
    rng = np.random.default_rng(5)
    pairs = {(int(u), 0) for u in range(n_users)}
    pairs |= {(int(u), 1) for u in rng.choice(n_users, low_max + 30, replace=False)}
    pairs |= {(0, i) for i in range(n_items)}
    for i in range(2, n_items):
        pairs |= {(int(u), i) for u in rng.choice(np.arange(1, n_users), 2, replace=False)}
    pairs = np.array(sorted(pairs))
    pairs = pairs[rng.permutation(len(pairs))]
    obs = rng.integers(1, 6, len(pairs)).astype(np.float32)
    return pairs[:, 0].astype(np.uint32), pairs[:, 1].astype(np.uint32), obs, n_users, n_items
