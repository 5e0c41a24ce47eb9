"""Lane-packed small systems of the predictor's fast path (cf_set_pred_pack): ratings
whose system has n = min(nc, d) <= 14 rows run four to a wave, those of 15..30 rows two to a wave.

Every rating's arithmetic is that of the one-rating-per-wave path, so packing on and off must give
the same bits (mse, kk, pred; NaN == NaN), through the fp64 entry (predict_precomp), the timed
fp32 instantiation (plan.predict_run) and cf_step_run; and the packed path must match the oracle
like test_gpu_predict.py does.

The case's coverage is asserted on the CPU before any device output is looked at: per rating
(nc, d, n, mode) from the oracle's eigenpairs (C = w > 0.1, lim as in gram_cond), so a case that
stops exercising a tier, a tier bound, a short last group or the pivot hand-over fails loudly.
The device's own lists may differ from this formula by a rating or two (they exclude the
closed-form nc = 1 ratings and those sent to the block-wide path before their Gram), hence
margins instead of exact counts.
"""
import numpy as np
import pytest

import cases  # noqa: F401  (build_case draws from it)
import oracle_ref as orc
from collaborative_filtering_amd.api import CF_SIGS_COMPAT, CF_SIGS_OWN, evec_offsets
from test_gpu_predict import build_case, gram_cond

pytestmark = pytest.mark.gpu

QUAD_MAX, PAIR_MAX = 14, 30   # kQuadNMax, kPairNMax of cf_predict.hip
# The first eight users are the case's base; then k = 13 (quad-list remainder 1), k = 16, and
# k = 52 (at density 0.6 a single rating in the quad tier beside 51 pairs).  At density 0.6 every
# rating of k = 12, 18, 24, 13 and 16 is in the quad tier (12 of them for k = 12).
KS = [12, 18, 24, 33, 40, 50, 64, 90, 13, 16, 52]
DENSITIES = [0.05, 0.45, 0.6, 0.9]
MODES = [CF_SIGS_COMPAT, CF_SIGS_OWN]

_cases = {}


def get_case(density):
    """build_case(density, KS, seed=40) with the per-rating classification, built once."""
    if density not in _cases:
        W, off, items, rat, m, sigs, evals, evec_off, evecs, blocks = build_case(density, KS, seed=40)
        _cases[density] = dict(W=W, off=off, items=items, rat=rat, m=m, sigs=sigs, evals=evals, evec_off=evec_off,
                               evecs=evecs, blocks=blocks, cls={})
    return _cases[density]


def classify(case, mode):
    """Per rating: user, nc, d, n = min(nc, d), K-mode (nc <= d), tier (0 none: closed form or
    c = 0, 1 single, 2 pair, 3 quad) and whether U_CS^T U_CS is numerically singular (smallest
    eigenvalue < 1e-9: the candidates of the pivot-rule hand-over when K-mode)."""
    if mode in case["cls"]:
        return case["cls"][mode]
    off, items, W, m, sigs = case["off"], case["items"], case["W"], case["m"], case["sigs"]
    n_all = int(off[-1])
    out = dict(user=np.zeros(n_all, int), nc=np.zeros(n_all, int), d=np.zeros(n_all, int), n=np.zeros(n_all, int),
               kmode=np.zeros(n_all, bool), tier=np.zeros(n_all, int), sing=np.zeros(n_all, bool))
    for u in range(len(KS)):
        b, e = int(off[u]), int(off[u + 1])
        k = e - b
        it = items[b:e].astype(np.int64)
        ev, U = case["blocks"][u]
        mu = min(int(m[u]), k)
        tab = sigs[:k] if mode == CF_SIGS_COMPAT else sigs[b:e]
        for r in range(k):
            C = np.nonzero(np.asarray(W[it[r], it], dtype=np.float64) > 0.1)[0]
            above = np.nonzero(np.asarray(ev[:mu], dtype=np.float64) > tab[r])[0]
            lim = int(above[0]) if len(above) else int(m[u])
            lim = min(max(lim, 2), int(m[u]))
            nc, d = k - len(C), k - lim
            n = min(nc, d)
            g = b + r
            out["user"][g], out["nc"][g], out["d"][g], out["n"][g], out["kmode"][g] = u, nc, d, n, nc <= d
            r_out = r not in C
            if len(C) == 0 or nc == 1 or n == 0 or not r_out:
                out["tier"][g] = 0 if (len(C) == 0 or nc == 1) else 1
            else:
                out["tier"][g] = 3 if n <= QUAD_MAX else (2 if n <= PAIR_MAX else 1)
            if len(C) and out["tier"][g] >= 2 and nc <= d:
                G = U[np.ix_(C, np.arange(lim))]
                out["sing"][g] = np.linalg.eigvalsh(G.T @ G)[0] < 1e-9
    case["cls"][mode] = out
    return out


def assert_coverage(density, mode):
    """The preconditions of this file's header, on the CPU classification."""
    c = classify(get_case(density), mode)
    tier, n, km = c["tier"], c["n"], c["kmode"]
    if density == 0.6:
        for t, name in ((3, "quad"), (2, "pair")):
            assert int(np.sum((tier == t) & km)) >= 10, (name, "K-mode", int(np.sum((tier == t) & km)))
            assert int(np.sum((tier == t) & ~km)) >= 10, (name, "G-mode", int(np.sum((tier == t) & ~km)))
        assert int(np.sum((tier == 1) & (n > PAIR_MAX))) >= 10
        for edge in (QUAD_MAX, QUAD_MAX + 1, PAIR_MAX, PAIR_MAX + 1):
            assert int(np.sum((n == edge) & (tier > 0))) >= 1, edge
        nq = np.array([int(np.sum((tier == 3) & (c["user"] == u))) for u in range(len(KS))])
        npair = np.array([int(np.sum((tier == 2) & (c["user"] == u))) for u in range(len(KS))])
        assert {1, 2, 3} <= set((nq[nq > 0] % 4).tolist()), nq.tolist()
        assert 1 in set((npair[npair > 0] % 2).tolist()), npair.tolist()
        assert int(np.sum(c["sing"])) >= 10, int(np.sum(c["sing"]))
        # a user whose every solved rating is in one tier, and a user with a single rating in a tier
        assert any(nq[u] > 0 and npair[u] == 0 and not np.any((tier == 1) & (c["user"] == u)) for u in range(len(KS)))
        assert 1 in nq.tolist() or 1 in npair.tolist(), (nq.tolist(), npair.tolist())
    if density == 0.05:   # sparse graph: wide complements, small d: G-mode small systems
        assert int(np.sum((tier >= 2) & ~km)) >= 10
    return c


def same_bits(x, y):
    return np.array_equal(np.ascontiguousarray(x).view(np.uint8), np.ascontiguousarray(y).view(np.uint8))


def run_precomp(ctx, case, mode, pack):
    ctx.set_pred_pack(pack)
    try:
        return ctx.predict_precomp(case["off"], case["items"], case["rat"], case["m"], case["evals"], case["evec_off"],
                                   case["evecs"], case["sigs"].copy(), sig_mode=mode, want_pred=True)
    finally:
        ctx.set_pred_pack(1)


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("density", DENSITIES)
def test_packed_equals_unpacked_f64(gpu_ctx, density, mode):
    """predict_precomp (fp64 blocks): packing on == packing off, bit for bit."""
    c = assert_coverage(density, mode)
    case = get_case(density)
    gpu_ctx.upload_graph_dense(case["W"])
    off_ = run_precomp(gpu_ctx, case, mode, 0)
    on_ = run_precomp(gpu_ctx, case, mode, 1)
    for name, x, y in zip(("mse", "kk", "pred"), off_, on_):
        assert same_bits(x, y), (name, int(np.sum(x != y)))
    print(f"density={density} mode={mode} quad={int(np.sum(c['tier'] == 3))} pair={int(np.sum(c['tier'] == 2))} "
          f"single={int(np.sum(c['tier'] == 1))} NaN={int(np.sum(np.isnan(on_[0])))}")


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("density", DENSITIES)
def test_packed_equals_unpacked_f32_run(gpu_ctx, density, mode):
    """plan.predict_run on the device's own fp32 eigen blocks (the timed instantiation): packing
    on == off."""
    import torch

    assert_coverage(density, mode)
    case = get_case(density)
    gpu_ctx.upload_graph_dense(case["W"])
    dev = torch.device("cuda")
    T = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)
    off = case["off"]
    n = int(off[-1])
    eoff, ne = evec_offsets(off)
    plan = gpu_ctx.plan(off)
    d_off, d_items, d_eoff = T(off.view(np.int64)), T(case["items"].view(np.int32)), T(eoff.view(np.int64))
    m, sigs = torch.zeros(len(KS), dtype=torch.int32, device=dev), torch.zeros(n, device=dev)
    evals, evecs = torch.zeros(n, device=dev), torch.zeros(ne, device=dev)
    plan.eigen_run(d_off, d_items, d_eoff, m, sigs, evals, evecs)
    args = (d_off, d_items, T(case["rat"]), m, evals, d_eoff, evecs, sigs, mode)
    outs = []
    try:
        for pack in (0, 1):
            gpu_ctx.set_pred_pack(pack)
            o = (torch.zeros(n, dtype=torch.float32, device=dev), torch.zeros(n, dtype=torch.int32, device=dev),
                 torch.zeros(n, dtype=torch.float64, device=dev))
            plan.predict_run(*args, *o)
            torch.cuda.synchronize()
            outs.append([t.cpu().numpy() for t in o])
    finally:
        gpu_ctx.set_pred_pack(1)
        plan.close()
    for name, x, y in zip(("mse", "kk", "pred"), *outs):
        assert same_bits(x, y), (name, int(np.sum(x != y)))


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("density", DENSITIES)
def test_packed_matches_oracle(gpu_ctx, density, mode):
    """Packing on against the oracle, as test_predict_matches_oracle: kk exact, c = 0 => NaN on both
    sides, |d mse| <= 1e-6 max(1, mse) where cond(U_CS^T U_CS) <= 1e8."""
    c = assert_coverage(density, mode)
    case = get_case(density)
    off, items, rat, m, sigs, W = case["off"], case["items"], case["rat"], case["m"], case["sigs"], case["W"]
    gpu_ctx.upload_graph_dense(W)
    mse_g, kk_g, _ = run_precomp(gpu_ctx, case, mode, 1)
    n_good = {1: 0, 2: 0, 3: 0, 0: 0}
    bad = []
    for u in range(len(KS)):
        b, e = int(off[u]), int(off[u + 1])
        it = items[b:e].astype(np.int64)
        ev, U = case["blocks"][u]
        ev_full = np.zeros(m[u])
        ev_full[: min(m[u], e - b)] = ev[: min(m[u], e - b)]
        tab = sigs[: e - b] if mode == CF_SIGS_COMPAT else sigs[b:e]
        mse_o, kk_o, _ = orc.predict_user(it, rat[b:e], ev_full, U, tab, W)
        for r in range(e - b):
            g = b + r
            if kk_g[g] != kk_o[r]:
                bad.append((u, r, "kk", kk_g[g], kk_o[r]))
            elif kk_o[r] == 0:
                if not (np.isnan(mse_g[g]) and np.isnan(mse_o[r])):
                    bad.append((u, r, "c=0 not NaN", mse_g[g], mse_o[r]))
            elif gram_cond(it, ev_full, U, tab[r], W, r) <= 1e8:
                if np.isnan(mse_g[g]) or np.isnan(mse_o[r]):
                    bad.append((u, r, "nan", mse_g[g], mse_o[r]))
                    continue
                n_good[int(c["tier"][g])] += 1
                if abs(float(mse_g[g]) - float(mse_o[r])) > 1e-6 * max(1.0, float(mse_o[r])):
                    bad.append((u, r, "mse", float(mse_g[g]), float(mse_o[r])))
    assert not bad, bad[:10]
    if density == 0.6:   # the comparison reaches both packed tiers
        assert n_good[3] >= 10 and n_good[2] >= 10, n_good
    print(f"density={density} mode={mode} compared by tier (0 none, 1 single, 2 pair, 3 quad): {n_good}")


@pytest.mark.parametrize("mode", MODES)
def test_step_run_equals_sequential_packed(gpu_ctx, mode):
    """cf_step_run and eigen_run + predict_run stay bit-equal with packing on (the check of
    test_step_run_equals_sequential on this file's density-0.6 users)."""
    import torch

    assert_coverage(0.6, mode)
    case = get_case(0.6)
    off, items, rat = case["off"], case["items"], case["rat"]
    gpu_ctx.upload_graph_dense(case["W"])
    gpu_ctx.set_pred_pack(1)
    plan = gpu_ctx.plan(off)
    dev = torch.device("cuda")
    T = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)
    eoff, ne = evec_offsets(off)
    n, n_users = int(off[-1]), len(KS)

    def fresh():
        return dict(m=torch.zeros(n_users, dtype=torch.int32, device=dev), sigs=torch.zeros(n, device=dev),
                    evals=torch.zeros(n, device=dev), evecs=torch.zeros(ne, device=dev),
                    mse=torch.zeros(n, device=dev), kk=torch.zeros(n, dtype=torch.int32, device=dev),
                    pred=torch.zeros(n, dtype=torch.float64, device=dev))

    d_off, d_items, d_rat, d_eoff = T(off.view(np.int64)), T(items.view(np.int32)), T(rat), T(eoff.view(np.int64))
    a, b = fresh(), fresh()
    plan.eigen_run(d_off, d_items, d_eoff, a["m"], a["sigs"], a["evals"], a["evecs"])
    plan.predict_run(d_off, d_items, d_rat, a["m"], a["evals"], d_eoff, a["evecs"], a["sigs"], mode,
                     a["mse"], a["kk"], a["pred"])
    plan.step_run(d_off, d_items, d_rat, d_eoff, b["m"], b["sigs"], b["evals"], b["evecs"], mode,
                  b["mse"], b["kk"], b["pred"])
    torch.cuda.synchronize()
    for key in a:
        assert same_bits(a[key].cpu().numpy(), b[key].cpu().numpy()), key
    plan.close()
