"""Checker for the SVD++ entry points: a plain numpy fp64 restatement of the synchronous
schedule (user supersteps 0, 2, .., item supersteps 1, 3, ..) written from the description of the
update rule in include/cf_abi.h, with a per-vertex loop and the reference's per-edge form of every
delta.  err, usrNorm, the ten hyper-parameters and the decay of the five steps are float32.  Not a
port.  The graph generator and build_csr are those of als_ref.py, the cases those of sgd_ref.py
with a seeded fifth of each case's TRAIN edges moved to the implicit list."""
from __future__ import annotations

import dataclasses
from dataclasses import dataclass, field

import numpy as np

from als_ref import build_csr
from sgd_ref import CASES, case_inputs as sgd_case_inputs, segmented_problem, train_mean  # noqa: F401

f32 = np.float32

STEP_NAMES = ("user_bias_step", "item_bias_step", "user_factor_step", "item_factor_step", "item_factor2_step")
REG_NAMES = ("user_bias_reg", "item_bias_reg", "user_factor_reg", "item_factor_reg", "item_factor2_reg")
# steps of about 0.02, regs of about 0.05 (sgd_ref.HYPER's size): the factors move
HYPER = dict(user_bias_step=0.02, user_bias_reg=0.05, item_bias_step=0.018, item_bias_reg=0.04, user_factor_step=0.02,
             user_factor_reg=0.05, item_factor_step=0.022, item_factor_reg=0.06, item_factor2_step=0.025,
             item_factor2_reg=0.045, step_dec=0.9, minval=1.0, maxval=5.0)


@dataclass
class SvdppRef:
    U: np.ndarray
    V: np.ndarray
    W: np.ndarray
    Y: np.ndarray
    bias_user: np.ndarray
    bias_item: np.ndarray
    nupdates_user: np.ndarray
    nupdates_item: np.ndarray
    supersteps: int = 0
    updates: int = 0
    messages: int = 0          # TRAIN edges of an active phase-2 user whose item's messages were reduced
    discarded: int = 0         # the same towards a signalled item in phase 1 (it ignores them)
    mixed_supersteps: int = 0  # user supersteps that held users of both phases
    n_nan: int = 0
    steps_next: np.ndarray = None
    round_margin: float = np.inf  # smallest distance of obs - p to a float midpoint, in float ulps
    trace: list = field(default_factory=list)       # [sum sq TRAIN, sum sq VALIDATE] per user superstep, without Y
    snapshots: list = field(default_factory=list)   # (U, V, W, Y, bu, bi, nup_u, nup_i) after every superstep
    max_change: float = 0.0    # largest per-superstep change of U, V or Y, relative to max|factor|


def predict(user, item, U, V, Y, bu, bi, mean, minval, maxval):
    user, item = np.asarray(user, np.int64), np.asarray(item, np.int64)
    p = mean + bu[user] + bi[item] + np.einsum("ij,ij->i", U[user], V[item] + Y[item])
    return np.maximum(minval, np.minimum(maxval, p))


def _errors(Uu, bu_u, Vr, Yr, bi_r, ob, mean, minval, maxval, out):
    """err per TRAIN edge: float32 of obs - clamp(mean + bu + bi + U_u . (V_i + Y_i)), as float64."""
    p = mean + bu_u + bi_r + (Vr + Yr) @ Uu
    p = np.where(p > maxval, maxval, p)
    p = np.where(p < minval, minval, p)
    d = ob.astype(np.float64) - p
    f = d.astype(f32)
    ok = np.isfinite(d)
    if ok.any():
        ulp = np.spacing(np.abs(f[ok])).astype(np.float64)
        out.round_margin = min(out.round_margin, float(np.min(0.5 - np.abs(d[ok] - f[ok].astype(np.float64)) / ulp)))
    return f.astype(np.float64)


def fit(user, item, obs, n_users, n_items, U0, V0, W0, Y0, *, implicit=None, step_dec, minval, maxval, mean,
        bias_user=None, bias_item=None, max_updates=None, max_supersteps=0, activate_user=None, validate=None,
        keep_snapshots=False, **hyper) -> SvdppRef:
    import sgd_ref

    assert max_updates is not None or max_supersteps, "the run would never end"
    step = {k: f32(hyper[k]) for k in STEP_NAMES}
    reg = {k: f32(hyper[k]) for k in REG_NAMES}
    U, V, W, Y = (np.array(x, dtype=np.float64) for x in (U0, V0, W0, Y0))
    bu = np.zeros(n_users) if bias_user is None else np.array(bias_user, dtype=np.float64)
    bi = np.zeros(n_items) if bias_item is None else np.array(bias_item, dtype=np.float64)
    uoff, uitem, uobs, _ = build_csr(user, item, obs, n_users)
    ioff, iuser, iobs, _ = build_csr(item, user, obs, n_items)
    if implicit is not None and len(implicit[0]):
        poff, pitem, _, _ = build_csr(implicit[0], implicit[1], np.zeros(len(implicit[0]), f32), n_users)
    else:
        poff, pitem = np.zeros(n_users + 1, np.int64), np.zeros(0, np.int64)
    deg_all = np.diff(uoff.astype(np.int64)) + np.diff(np.asarray(poff).astype(np.int64))
    with np.errstate(divide="ignore"):
        unorm = (1.0 / np.sqrt(deg_all.astype(np.float64))).astype(f32)
    nup_u, nup_i = np.zeros(n_users, np.uint32), np.zeros(n_items, np.uint32)
    cap = np.inf if max_updates is None else max_updates
    active = np.ones(n_users, bool) if activate_user is None else np.asarray(activate_user).astype(bool)
    out = SvdppRef(U, V, W, Y, bu, bi, nup_u, nup_i)
    out.steps_next = np.array([step[k] for k in STEP_NAMES], f32)

    def snap(prev):
        cur = (U.copy(), V.copy(), W.copy(), Y.copy(), bu.copy(), bi.copy(), nup_u.copy(), nup_i.copy())
        scale = max(np.max(np.abs(cur[0])), np.max(np.abs(cur[1])), np.max(np.abs(cur[3])))
        for k in (0, 1, 3):
            out.max_change = max(out.max_change, float(np.max(np.abs(cur[k] - prev[k]))) / scale)
        if keep_snapshots:
            out.snapshots.append(cur)
        return cur

    prev = (U.copy(), V.copy(), W.copy(), Y.copy())
    while active.any() and not (max_supersteps and out.supersteps >= max_supersteps):
        Uo, Vo, Wo, Yo, buo, bio = U.copy(), V.copy(), W.copy(), Y.copy(), bu.copy(), bi.copy()
        phase2_u = (nup_u % 2 == 1)
        # ---- user superstep ----
        signalled = np.zeros(n_items, bool)
        acts = np.flatnonzero(active)
        if phase2_u[acts].any() and (~phase2_u[acts]).any():
            out.mixed_supersteps += 1
        for u in acts:
            b, e = int(uoff[u]), int(uoff[u + 1])
            its = uitem[b:e].astype(np.int64)
            if not phase2_u[u]:
                every = np.concatenate([its, pitem[int(poff[u]):int(poff[u + 1])].astype(np.int64)])
                if len(every):
                    tot = np.zeros(U.shape[1])
                    for i in every:
                        tot = tot + Yo[i]
                    W[u] = tot * np.float64(unorm[u])
                    signalled[every] = True          # no max_updates check
            elif e > b:
                err = _errors(Uo[u], buo[u], Vo[its], Yo[its], bio[its], uobs[b:e], mean, minval, maxval, out)
                out.n_nan += int(np.isnan(err).sum())
                dU = np.zeros(U.shape[1])
                db = 0.0
                for k, i in enumerate(its):
                    dU = dU + np.float64(step["user_factor_step"]) * (err[k] * (Vo[i] - np.float64(reg["user_factor_reg"]) * Uo[u]))
                    db = db + np.float64(step["user_bias_step"]) * (err[k] - np.float64(reg["user_bias_reg"]) * 0.0)
                U[u] = Uo[u] + dU
                bu[u] = buo[u] + db
                signalled[its[nup_i[its] < cap]] = True
            nup_u[u] += 1
        # the items' messages, from the same old values: only an item in phase 2 with updates left adds them
        dV, dY, dbi = np.zeros_like(V), np.zeros_like(Y), np.zeros(n_items)
        mult = np.float64(f32(step["item_factor2_step"] * reg["item_factor2_reg"]))
        for i in np.flatnonzero(signalled):
            b, e = int(ioff[i]), int(ioff[i + 1])
            us = iuser[b:e].astype(np.int64)
            sel = active[us] & phase2_u[us]
            us, ob = us[sel], iobs[b:e][sel]
            if nup_i[i] % 2 == 0:
                out.discarded += int(sel.sum()) if nup_i[i] < cap else 0
                continue
            if not nup_i[i] < cap or not len(us):
                continue
            err = np.array([_errors(Uo[u], buo[u], Vo[i][None], Yo[i][None], bio[i], ob[k:k + 1], mean, minval, maxval, out)[0]
                            for k, u in enumerate(us)])
            out.messages += len(us)
            for k, u in enumerate(us):
                c = np.float64(f32(step["item_factor2_step"] * unorm[u]))
                dV[i] = dV[i] + np.float64(step["item_factor_step"]) * (err[k] * (Uo[u] + Wo[u]) - np.float64(reg["item_factor_reg"]) * Vo[i])
                dbi[i] = dbi[i] + np.float64(step["item_bias_step"]) * (err[k] - np.float64(reg["item_bias_reg"]) * 0.0)
                dY[i] = dY[i] + ((err[k] * Vo[i]) * c - mult * Yo[i])
        out.supersteps += 1
        out.updates += int(active.sum())
        for k in STEP_NAMES:
            step[k] = f32(np.float64(step[k]) * np.float64(step_dec))
        out.steps_next = np.array([step[k] for k in STEP_NAMES], f32)
        row = [sgd_ref.sum_sq_error(user, item, obs, U, V, bu, bi, mean, minval, maxval), 0.0]
        if validate is not None and len(validate[0]):
            row[1] = sgd_ref.sum_sq_error(validate[0], validate[1], validate[2], U, V, bu, bi, mean, minval, maxval)
        out.trace.append(row)
        prev = snap(prev)
        if out.n_nan or not signalled.any() or (max_supersteps and out.supersteps >= max_supersteps):
            break   # numeric errors; nobody signalled; or cut here: the pending messages are dropped
        # ---- item superstep ----
        nxt = np.zeros(n_users, bool)
        for i in np.flatnonzero(signalled):
            if nup_i[i] % 2 == 1:
                V[i] = V[i] + dV[i]
                Y[i] = Y[i] + dY[i]
                bi[i] = bi[i] + dbi[i]
            nup_i[i] += 1
            us = iuser[int(ioff[i]):int(ioff[i + 1])].astype(np.int64)
            nxt[us[nup_u[us] < cap]] = True
        out.supersteps += 1
        out.updates += int(signalled.sum())
        prev = snap(prev)
        active = nxt
    return out


# ---- the cases the CPU and GPU tests share ------------------------------------------------

NAMES = ["A", "B", "C", "E", "F", "G"]
MAX_UPDATES = {"A": 6, "B": 4, "C": 4, "E": 4, "F": 4, "G": 4}# phase-1 and phase-2 updates alike: 3 / 2 gradient passes


@dataclass
class Case:
    g: object                 # als_ref.Graph with a fifth of its TRAIN edges removed
    imp_user: np.ndarray      # the implicit list: the moved TRAIN edges, then the VALIDATE edges
    imp_item: np.ndarray
    U0: np.ndarray
    V0: np.ndarray
    W0: np.ndarray
    Y0: np.ndarray
    max_updates: int


_CASES = {}


def case_inputs(name) -> Case:
    if name not in _CASES:
        g, U0, V0, _ = sgd_case_inputs(name)
        rng = np.random.default_rng(21)
        move = rng.random(len(g.user)) < 0.2
        move &= g.item != 0            # every user keeps its item-0 TRAIN edge, item 0 stays in the mid class
        g2 = dataclasses.replace(g, user=g.user[~move], item=g.item[~move], obs=g.obs[~move])
        imp_user = np.concatenate([g.user[move], g.vuser]).astype(np.uint32)
        imp_item = np.concatenate([g.item[move], g.vitem]).astype(np.uint32)
        W0, Y0 = g.factors(U0.shape[1], seed=12)
        _CASES[name] = Case(g2, imp_user, imp_item, U0, V0, 0.5 * W0, 0.5 * Y0, MAX_UPDATES[name])
    return _CASES[name]


def run_case(name, *, case=None, **over):
    c = case_inputs(name) if case is None else case
    g = c.g
    kw = dict(HYPER, implicit=(c.imp_user, c.imp_item), mean=train_mean(g.obs), max_updates=c.max_updates,
              activate_user=g.out_degree > 0, validate=(g.vuser, g.vitem, g.vobs), keep_snapshots=True)
    kw.update(over)
    return fit(g.user, g.item, g.obs, g.n_users, g.n_items, c.U0, c.V0, c.W0, c.Y0, **kw)


_REF_CACHE = {}


def case_reference(name) -> SvdppRef:
    """The checker's run of a case, computed once and shared (callers must not modify it)."""
    if name not in _REF_CACHE:
        _REF_CACHE[name] = run_case(name)
    return _REF_CACHE[name]


def segmented_case(seg, low_max, D=4):
    """sgd_ref.segmented_problem (a high-class item, a mid-class item, user 0 in the mid class on
    the TRAIN list) plus implicit edges: user 1 has a few TRAIN edges and low_max implicit ones, so
    its all-role list crosses the low cut through the implicit edges alone."""
    user, item, obs, nu, ni = segmented_problem(seg, low_max)
    train_1 = set(item[user == 1].tolist())
    extra = [i for i in range(ni) if i not in train_1][:low_max]
    rng = np.random.default_rng(8)
    other_u = rng.integers(2, nu, 40).astype(np.uint32)
    other_i = rng.integers(0, ni, 40).astype(np.uint32)
    imp_user = np.concatenate([np.full(len(extra), 1, np.uint32), other_u])
    imp_item = np.concatenate([np.array(extra, np.uint32), other_i])
    rng = np.random.default_rng(6)
    mats = [rng.uniform(-1, 1, (n, D)) * s for n, s in ((nu, 1.0), (ni, 1.0), (nu, 0.5), (ni, 0.5))]
    return user, item, obs, nu, ni, imp_user, imp_item, mats
