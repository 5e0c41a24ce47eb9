"""numpy checker of cf_mf_rank_eval (cf_abi.h), built on topn_ref's score matrix and exclusion
mask.  Ranks come from direct counting with the tie rule of cf_mf_topn (score descending, item
ascending); the metrics follow the header's formulas term by term."""
from __future__ import annotations

import numpy as np

import topn_ref as tr

MAX = 0xFFFFFFFF
USER_FIELDS = ("n_cand", "n_rel", "hits", "precision", "recall", "ndcg", "ap", "rr", "auc")
MEAN_FIELDS = ("precision", "recall", "ndcg", "map", "mrr", "auc", "mpr")


def sort_edges(user, item, weight=None):
    """The held-out pairs by (user, item): the order the library counts in."""
    user, item = np.asarray(user, dtype=np.int64), np.asarray(item, dtype=np.int64)
    p = np.lexsort((item, user))
    return user[p], item[p], (None if weight is None else np.asarray(weight, dtype=np.float64)[p]), p


def rank_of(S_row, cand_row, h):
    """Rank of item h in a row: the candidates that come before it (MAX if h is no candidate)."""
    if not cand_row[h]:
        return MAX
    s = S_row[h]
    idx = np.arange(len(S_row))
    return int((cand_row & ((S_row > s) | ((S_row == s) & (idx < h)))).sum())


def user_metrics(C, ranks, N):
    """The cf_rank_user record of one user from its candidate count and its edges' ranks (MAX = skipped)."""
    r = sorted(int(x) for x in ranks if int(x) != MAX)
    m = len(r)
    rec = dict.fromkeys(USER_FIELDS, 0)
    if m == 0:
        return rec
    cut = min(m, N)
    hits = sum(1 for x in r if x < N)
    dcg = sum(1.0 / np.log2(x + 2.0) for x in r if x < N)
    idcg = sum(1.0 / np.log2(t + 2.0) for t in range(cut))
    ap = sum((j + 1.0) / (x + 1.0) for j, x in enumerate(r) if x < N) / cut
    auc = sum(C - m - x + j for j, x in enumerate(r)) / (m * (C - m)) if C > m else 0.0
    rec.update(n_cand=C, n_rel=m, hits=hits, precision=hits / N, recall=hits / m, ndcg=dcg / idcg, ap=ap,
               rr=1.0 / (r[0] + 1.0), auc=auc)
    return rec


def evaluate_scores(S, mask, N, user, item, weight=None):
    """(rank, n_cand_edge, users, summary) from a score matrix and an exclusion mask.  rank and
    n_cand_edge are in the caller's edge order; users is a list of records per user; summary holds
    the means, mpr and the edge counts."""
    n_users = S.shape[0]
    cand = ~mask & ~np.isnan(S)
    su, si, sw, perm = sort_edges(user, item, weight)
    ranks_sorted = np.array([rank_of(S[u], cand[u], i) for u, i in zip(su, si)], dtype=np.int64)
    users = []
    s = dict.fromkeys(MEAN_FIELDS, 0.0)
    s.update(users_evaluated=0, users_auc=0, edges_counted=0, edges_skipped=0, n_nan_held=0)
    num = den = 0.0
    for u in range(n_users):
        e = np.flatnonzero(su == u)
        rec = user_metrics(int(cand[u].sum()), ranks_sorted[e], N)
        users.append(rec)
        s["edges_counted"] += rec["n_rel"]
        s["edges_skipped"] += len(e) - rec["n_rel"]
        s["n_nan_held"] += int((np.isnan(S[u, si[e]]) & ~mask[u, si[e]]).sum())
        if rec["n_rel"] == 0:
            continue
        s["users_evaluated"] += 1
        for k, f in (("precision", "precision"), ("recall", "recall"), ("ndcg", "ndcg"), ("map", "ap"), ("mrr", "rr")):
            s[k] += rec[f]
        if rec["n_cand"] > rec["n_rel"]:
            s["users_auc"] += 1
            s["auc"] += rec["auc"]
        C = rec["n_cand"]
        for k in e:   # CSR order
            if ranks_sorted[k] == MAX:
                continue
            w = 1.0 if sw is None else float(sw[k])
            num += w * (ranks_sorted[k] / (C - 1) if C > 1 else 0.0)
            den += w
    for k in ("precision", "recall", "ndcg", "map", "mrr"):
        if s["users_evaluated"]:
            s[k] /= s["users_evaluated"]
    if s["users_auc"]:
        s["auc"] /= s["users_auc"]
    s["mpr"] = num / den if den != 0.0 else 0.0
    rank = np.zeros(len(su), dtype=np.uint32)
    rank[perm] = ranks_sorted.astype(np.uint32)
    n_cand_edge = np.zeros(len(su), dtype=np.uint32)
    n_cand_edge[perm] = np.array([users[u]["n_cand"] for u in su], dtype=np.uint32)
    return rank, n_cand_edge, users, s


def evaluate(U, V, N, held, exclude=None, bias_user=None, bias_item=None, mean=0.0):
    S = tr.score_matrix(U, V, bias_user, bias_item, mean)
    mask = tr.exclusion_mask(S.shape[0], S.shape[1], exclude)
    return evaluate_scores(S, mask, N, held[0], held[1], held[2] if len(held) > 2 else None)


def rank_windows(U, V, held, exclude=None, bias_user=None, bias_item=None, mean=0.0, mask=None):
    """For real-valued data: per held-out edge (caller order) the window [lo, hi] its rank must lie
    in when a device score may differ from numpy's by b = 1e-13 (|U| |V|^T) (the bound
    test_gpu_topn.py uses): lo = #{c != h : S_c - b_c > S_h + b_h}, hi = #{c != h : S_c + b_c >=
    S_h - b_h} over the candidates c.  Also the smallest score gap to another candidate and the
    largest bound met.  An edge that is no candidate gets (MAX, MAX)."""
    U, V = np.asarray(U, dtype=np.float64), np.asarray(V, dtype=np.float64)
    S = tr.score_matrix(U, V, bias_user, bias_item, mean)
    B = 1e-13 * (np.abs(U) @ np.abs(V).T)
    if mask is None:
        mask = tr.exclusion_mask(S.shape[0], S.shape[1], exclude)
    cand = ~mask & ~np.isnan(S)
    lo = np.zeros(len(held[0]), dtype=np.int64)
    hi = np.zeros(len(held[0]), dtype=np.int64)
    gap, bmax = np.inf, 0.0
    for k, (u, h) in enumerate(zip(np.asarray(held[0], dtype=np.int64), np.asarray(held[1], dtype=np.int64))):
        if not cand[u, h]:
            lo[k] = hi[k] = MAX
            continue
        c = cand[u].copy()
        c[h] = False
        lo[k] = int((c & (S[u] - B[u] > S[u, h] + B[u, h])).sum())
        hi[k] = int((c & (S[u] + B[u] >= S[u, h] - B[u, h])).sum())
        if c.any():
            gap = min(gap, float(np.abs(S[u, c] - S[u, h]).min()))
        bmax = max(bmax, float(B[u, cand[u]].max()))
    return lo, hi, gap, bmax
