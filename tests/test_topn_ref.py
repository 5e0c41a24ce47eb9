"""The numpy checker of cf_mf_topn (topn_ref.py) on hand-written cases (CPU only)."""
import numpy as np

import topn_ref as tr

MAX = 0xFFFFFFFF

U35 = np.array([[1.0, 0.0], [0.0, 1.0], [1.0, 1.0]])
V35 = np.array([[3.0, 0.0], [1.0, 2.0], [2.0, 2.0], [0.0, -1.0], [3.0, 1.0]])
# scores:  user 0: 3 1 2  0 3     user 1: 0 2 2 -1 1     user 2: 3 3 4 -1 4
EXCL35 = (np.array([0, 2, 2, 1]), np.array([0, 2, 2, 3]))   # (2, 2) twice


def test_three_by_five_lists():
    items, scores, count, n_nan = tr.topn(U35, V35, 3, exclude=EXCL35)
    assert items.dtype == np.uint32 and scores.dtype == np.float64 and count.dtype == np.uint32
    assert items.tolist() == [[4, 2, 1], [1, 2, 4], [4, 0, 1]]
    assert scores.tolist() == [[3.0, 2.0, 1.0], [2.0, 2.0, 1.0], [4.0, 3.0, 3.0]]
    assert count.tolist() == [3, 3, 3] and n_nan == 0


def test_three_by_five_tail_selection_and_bias():
    items, scores, count, _ = tr.topn(U35, V35, 5, exclude=EXCL35, users=[2, 0])
    assert items.tolist() == [[4, 0, 1, 3, MAX], [4, 2, 1, 3, MAX]]
    assert scores.tolist() == [[4.0, 3.0, 3.0, -1.0, 0.0], [3.0, 2.0, 1.0, 0.0, 0.0]]
    assert count.tolist() == [4, 4]
    # bias_item + mean, no user bias: user 0's scores become 4 2 3 11 4
    items, scores, count, _ = tr.topn(U35, V35, 2, bias_item=[0, 0, 0, 10, 0], mean=1.0, exclude=EXCL35, users=[0])
    assert items.tolist() == [[3, 4]] and scores.tolist() == [[11.0, 4.0]]
    # without a bias the mean is not used
    assert tr.topn(U35, V35, 1, mean=7.0)[1].tolist() == [[3.0], [2.0], [4.0]]


def test_nan_is_left_out_and_counted():
    V = V35.copy()
    V[4, 0] = np.nan
    items, scores, count, n_nan = tr.topn(U35, V, 5, exclude=(np.array([1]), np.array([4])))
    assert n_nan == 2 and count.tolist() == [4, 4, 4]
    assert not (items == 4).any()
    assert items[0].tolist() == [0, 2, 1, 3, MAX]


def test_all_ties_list_the_candidates_in_ascending_order():
    U = np.zeros((2, 3))
    V = -np.ones((6, 3))   # every product is -0.0
    items, scores, count, _ = tr.topn(U, V, 4, exclude=(np.array([0, 0]), np.array([3, 1])))
    assert items.tolist() == [[0, 2, 4, 5], [0, 1, 2, 3]]
    assert count.tolist() == [4, 4]
    assert not np.signbit(scores).any() and (scores == 0.0).all()
