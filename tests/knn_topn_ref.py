"""numpy checker of cf_knn_topn / cf_knn_rank_eval (cf_abi.h): item-kNN scores of every item for a
user's profile from the out-edges of the scored item.

Per user the profile is walked in its order and every entry does the two masked vector updates
over all m in float64 from the float32 W: the same sequence of IEEE operations as the device (the
product of two floats is exact in fp64, so an fma changes no bit), which makes the scores
comparable byte for byte, also for real-valued weights and ratings.  Lists come from
topn_ref.topn_from_scores and ranks and metrics from rank_ref.evaluate_scores, as they are."""
from __future__ import annotations

import numpy as np

import rank_ref as rr
import topn_ref as tr

SUM, MEAN = "sum", "mean"


def sums(W, user_off, items, ratings, w_min):
    """(sw, swr), each float64[n_users, n_items]: sw[u, m] = sum over the profile entries t of u in
    order of (double) W[m, i_t] where it is > w_min, swr the same of (double) W[m, i_t] * (double) r_t."""
    W = np.asarray(W, dtype=np.float32)
    off = np.asarray(user_off, dtype=np.int64)
    items = np.asarray(items, dtype=np.int64)
    ratings = np.asarray(ratings, dtype=np.float32)
    n_users, n_items = len(off) - 1, W.shape[0]
    sw = np.zeros((n_users, n_items), dtype=np.float64)
    swr = np.zeros((n_users, n_items), dtype=np.float64)
    Wd = W.astype(np.float64)
    with np.errstate(invalid="ignore", over="ignore"):
        for u in range(n_users):
            for t in range(int(off[u]), int(off[u + 1])):
                w = Wd[:, items[t]]
                keep = w > float(w_min)
                r = np.float64(ratings[t])
                sw[u, keep] = sw[u, keep] + w[keep]
                swr[u, keep] = swr[u, keep] + w[keep] * r
    return sw, swr


def score_matrix(W, user_off, items, ratings, mode=SUM, w_min=0.1):
    """score[u, m]: swr (sum) or swr / sw where sw > 0, else 0 (mean).  -0.0 is returned as +0.0."""
    sw, swr = sums(W, user_off, items, ratings, w_min)
    if mode == SUM:
        S = swr
    elif mode == MEAN:
        with np.errstate(invalid="ignore", divide="ignore", over="ignore"):
            S = np.where(sw > 0.0, swr / np.where(sw > 0.0, sw, 1.0), 0.0)
    else:
        raise ValueError(mode)
    return np.where(S == 0.0, 0.0, S)


def profile_pairs(user_off, items):
    """The profile as (user, item) index arrays: the exclusion list of exclude="profile"."""
    off = np.asarray(user_off, dtype=np.int64)
    return np.repeat(np.arange(len(off) - 1), np.diff(off)).astype(np.uint32), np.asarray(items, dtype=np.uint32)


def _mask(W, user_off, items, exclude):
    n_users, n_items = len(user_off) - 1, np.asarray(W).shape[0]
    if isinstance(exclude, str):
        assert exclude == "profile"
        exclude = profile_pairs(user_off, items)
    return tr.exclusion_mask(n_users, n_items, exclude)


def topn(W, user_off, items, ratings, N, mode=SUM, w_min=0.1, exclude="profile", users=None):
    S = score_matrix(W, user_off, items, ratings, mode, w_min)
    return tr.topn_from_scores(S, _mask(W, user_off, items, exclude), N, users)


def evaluate(W, user_off, items, ratings, N, held, mode=SUM, w_min=0.1, exclude="profile"):
    S = score_matrix(W, user_off, items, ratings, mode, w_min)
    return rr.evaluate_scores(S, _mask(W, user_off, items, exclude), N, held[0], held[1],
                              held[2] if len(held) > 2 else None)
