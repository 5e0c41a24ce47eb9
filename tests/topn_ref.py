"""numpy checker of cf_mf_topn (cf_abi.h): the full score matrix, the exclusion mask, and a
lexsort by (-score, item) per user.  Scores are numpy's own dot products, so against the
device they agree to rounding; on integer-valued data they are exact in any order."""
from __future__ import annotations

import numpy as np

SENTINEL = np.uint32(0xFFFFFFFF)


def score_matrix(U, V, bias_user=None, bias_item=None, mean=0.0):
    """score[u, i] = U_u . V_i + (bias_item[i] + (mean + bias_user[u])); an absent bias is
    skipped, and without any bias the mean is too.  -0.0 is returned as +0.0."""
    U = np.asarray(U, dtype=np.float64)
    V = np.asarray(V, dtype=np.float64)
    with np.errstate(invalid="ignore", over="ignore"):
        S = U @ V.T
        if bias_user is not None or bias_item is not None:
            t = np.full((U.shape[0], 1), float(mean))
            if bias_user is not None:
                t = float(mean) + np.asarray(bias_user, dtype=np.float64)[:, None]
            if bias_item is not None:
                t = np.asarray(bias_item, dtype=np.float64)[None, :] + t
            S = S + t
    S = np.where(S == 0.0, 0.0, S)
    return S


def exclusion_mask(n_users, n_items, exclude=None):
    """mask[u, i] = True where (u, i) is listed (any order, repeats allowed)."""
    mask = np.zeros((n_users, n_items), dtype=bool)
    if exclude is not None and len(exclude[0]):
        mask[np.asarray(exclude[0], dtype=np.int64), np.asarray(exclude[1], dtype=np.int64)] = True
    return mask


def topn_from_scores(S, mask, N, users=None):
    """(items, scores, count, n_nan) of the selected rows of S: per row the candidates (not
    masked, not NaN) ordered by score descending, ties by item ascending, cut at N; the tail is
    UINT32_MAX / 0.0.  n_nan counts the NaN scores of unmasked pairs of the selected rows."""
    sel = np.arange(S.shape[0]) if users is None else np.asarray(users, dtype=np.int64)
    items = np.full((len(sel), N), SENTINEL, dtype=np.uint32)
    scores = np.zeros((len(sel), N), dtype=np.float64)
    count = np.zeros(len(sel), dtype=np.uint32)
    n_nan = 0
    for j, u in enumerate(sel):
        nan = np.isnan(S[u])
        n_nan += int((nan & ~mask[u]).sum())
        cand = np.flatnonzero(~mask[u] & ~nan)
        order = cand[np.lexsort((cand, -S[u, cand]))][:N]
        count[j] = len(order)
        items[j, : len(order)] = order
        scores[j, : len(order)] = S[u, order]
    return items, scores, count, n_nan


def topn(U, V, N, bias_user=None, bias_item=None, mean=0.0, exclude=None, users=None):
    S = score_matrix(U, V, bias_user, bias_item, mean)
    mask = exclusion_mask(S.shape[0], S.shape[1], exclude)
    return topn_from_scores(S, mask, N, users)
