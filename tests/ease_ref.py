"""numpy checker of the EASE entry points (cf_abi.h): the Gram matrix in the device's summation
order, the weights through numpy's own inverse, and the scores of a profile with the device's
sequence of IEEE operations.

gram() adds one user at a time in ascending order from a zero accumulator; the product of two
float32 values is exact in float64, so G is comparable byte for byte.  weights() is the closed
form with numpy.linalg.inv: against the device it agrees to the conditioning of G, not to the bit.
score_matrix() walks the profile in its order and does, per entry, one rounded product and one
rounded sum per item: the bytes of the device for any B, NaN entries included.  Lists come from
topn_ref.topn_from_scores and ranks and metrics from rank_ref.evaluate_scores, as they are."""
from __future__ import annotations

import numpy as np

import rank_ref as rr
import topn_ref as tr


def values(ratings, binary):
    """x of every edge in float64: 1 when binary, else the float32 rating."""
    r = np.asarray(ratings, dtype=np.float32).astype(np.float64)
    return np.ones(len(r)) if binary else r


def dense(user_off, items, ratings, n_items, binary=False):
    """X [n_users, n_items] in float64 (a pair listed twice keeps its last value)."""
    off = np.asarray(user_off, dtype=np.int64)
    items = np.asarray(items, dtype=np.int64)
    x = values(ratings, binary)
    X = np.zeros((len(off) - 1, n_items))
    for u in range(len(off) - 1):
        X[u, items[off[u]:off[u + 1]]] = x[off[u]:off[u + 1]]
    return X


def gram(user_off, items, ratings, n_items, lam, binary=False):
    """G = X^T X + lam I: users in ascending order from a zero accumulator, lam last."""
    off = np.asarray(user_off, dtype=np.int64)
    items = np.asarray(items, dtype=np.int64)
    x = values(ratings, binary)
    G = np.zeros((n_items, n_items))
    for u in range(len(off) - 1):
        it, xu = items[off[u]:off[u + 1]], x[off[u]:off[u + 1]]
        assert len(np.unique(it)) == len(it)
        G[np.ix_(it, it)] = G[np.ix_(it, it)] + np.outer(xu, xu)
    G[np.diag_indices(n_items)] = G[np.diag_indices(n_items)] + float(lam)
    return G


def weights_from_inverse(P):
    """B[i][j] = -P[i][j] / P[j][j], zero on the diagonal."""
    P = np.asarray(P, dtype=np.float64)
    B = -P / np.diag(P)[None, :]
    np.fill_diagonal(B, 0.0)
    return B


def weights(G):
    return weights_from_inverse(np.linalg.inv(np.asarray(G, dtype=np.float64)))


def score_matrix(B, user_off, items, ratings, binary=False):
    """score[u, j] = sum over the profile of u in its order of x_t * B[i_t, j], each product rounded,
    then added, from zero.  -0.0 is returned as +0.0."""
    B = np.asarray(B, dtype=np.float64)
    off = np.asarray(user_off, dtype=np.int64)
    items = np.asarray(items, dtype=np.int64)
    x = values(ratings, binary)
    S = np.zeros((len(off) - 1, B.shape[0]))
    with np.errstate(invalid="ignore", over="ignore"):
        for u in range(len(off) - 1):
            for t in range(int(off[u]), int(off[u + 1])):
                S[u] = S[u] + x[t] * B[items[t]]
    return np.where(S == 0.0, 0.0, S)


def profile_pairs(user_off, items):
    """The profile as (user, item) index arrays: the exclusion list of exclude="profile"."""
    off = np.asarray(user_off, dtype=np.int64)
    return np.repeat(np.arange(len(off) - 1), np.diff(off)).astype(np.uint32), np.asarray(items, dtype=np.uint32)


def _mask(B, user_off, items, exclude):
    n_users, n_items = len(user_off) - 1, np.asarray(B).shape[0]
    if isinstance(exclude, str):
        assert exclude == "profile"
        exclude = profile_pairs(user_off, items)
    return tr.exclusion_mask(n_users, n_items, exclude)


def topn(B, user_off, items, ratings, N, binary=False, exclude="profile", users=None):
    S = score_matrix(B, user_off, items, ratings, binary)
    return tr.topn_from_scores(S, _mask(B, user_off, items, exclude), N, users)


def evaluate(B, user_off, items, ratings, N, held, binary=False, exclude="profile"):
    S = score_matrix(B, user_off, items, ratings, binary)
    return rr.evaluate_scores(S, _mask(B, user_off, items, exclude), N, held[0], held[1],
                              held[2] if len(held) > 2 else None)
