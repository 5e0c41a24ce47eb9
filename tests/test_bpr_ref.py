"""Conditions on the BPR checker (tests/bpr_ref.py) and on the cases the GPU tests take from it;
nothing here runs on a device.  The tests that read the cuts need the built library only."""
import numpy as np
import pytest

import bpr_ref as br
import rank_ref as rr
from collaborative_filtering_amd import _native


def degrees(c):
    return np.bincount(c.user, minlength=c.n_users), np.bincount(c.item, minlength=c.n_items)


def test_abi_symbols_and_cuts():
    lib = _native.load()
    assert lib.cf_debug_bpr_tries() == br.TRIES == _native.CF_BPR_TRIES
    assert (lib.cf_debug_als_low_max(), lib.cf_debug_als_segment()) == (br.LOW, br.SEG)
    for name in ("cf_bpr_fit", "cf_bpr_sample", "cf_bpr_timing"):
        assert hasattr(lib, name)


def test_splitmix64_is_the_cli_generator():
    # the first outputs of splitmix64 seeded with 0 (the published test vector): state += golden, then mix
    assert br.sm(0) == 0xE220A8397B1DCDAF
    assert br.sm(0x9E3779B97F4A7C15) == 0x6E789E6AA1B965F4


def test_planted_case_learns_to_rank():
    c, r = br.case_inputs("P"), br.case_reference("P")
    assert (c.n_users, c.n_items, c.D, c.n_sweeps, c.lr, c.reg) == (60, 40, 8, 40, 2.0, 0.01)
    du, _ = degrees(c)
    assert du[0] == c.n_items and du[1] == c.n_items - 1
    auc0, _ = br.train_auc(c, c.U0, c.V0, c.bias0)
    auc1, _ = br.train_auc(c, r.U, r.V, r.bias)
    mean = r.loss_trace[:, 0] / r.loss_trace[:, 1]
    print("AUC", auc0, auc1, "mean softplus", mean[0], mean[-1], "skipped", r.skipped_per_sweep)
    assert auc0 < 0.55 and auc1 > 0.95
    assert abs(mean[0] - np.log(2.0)) < 0.01 and mean[-1] < 0.2
    assert all(50 <= s <= 100 for s in r.skipped_per_sweep) and len(r.skipped_per_sweep) == 40
    # user 0 never has a triple; user 1's one free item is found or all tries fail
    assert r.U[0].tobytes() == c.U0[0].tobytes() and r.user_counted[1] and not r.user_counted[0]
    for s in (0, 7):
        neg = br.sample(c.user, c.item, c.n_users, c.n_items, c.seed, s)
        assert np.all(neg[c.user == 0] == br.MAX)
        n1 = neg[c.user == 1]
        assert set(n1.tolist()) == {17, br.MAX}
    # no tie among the fitted scores: ranks are comparable exactly (test_gpu_bpr.py does)
    _, _, gap, _ = rr.rank_windows(r.U, r.V, (c.user, c.item), bias_item=r.bias)
    print("smallest score gap", gap)
    assert gap > 1e-9


def test_sample_properties():
    c = br.case_inputs("P")
    a = br.sample(c.user, c.item, c.n_users, c.n_items, 5, 0)
    assert not np.array_equal(a, br.sample(c.user, c.item, c.n_users, c.n_items, 5, 1))
    assert not np.array_equal(a, br.sample(c.user, c.item, c.n_users, c.n_items, 6, 0))
    rated = set(zip(c.user.tolist(), c.item.tolist()))
    assert all((u, j) not in rated for u, j in zip(c.user.tolist(), a.tolist()) if j != br.MAX)
    assert a[a != br.MAX].max() < c.n_items
    # a user's negatives depend on its own list only: drop every other user
    keep = c.user == 7
    b = br.sample(c.user[keep], c.item[keep], c.n_users, c.n_items, 5, 0)
    assert np.array_equal(b, a[keep]) and keep.sum() > 1
    # the pairs may come in any order, repeated
    p = np.random.default_rng(0).permutation(len(c.user))
    assert np.array_equal(a, br.sample(np.append(c.user[p], c.user[:3]), np.append(c.item[p], c.item[:3]), c.n_users, c.n_items, 5, 0))


def test_structure_of_the_d_sweep():
    p = br.case_inputs("P")
    assert br.D_SWEEP == (1, 5, 20, 33, 64)   # the D < 8 tail and the register blocks 1, 3, 8 of launch_reduce
    for d in br.D_SWEEP:
        c = br.case_inputs(f"D{d}")
        assert (c.D, c.n_sweeps) == (d, 3) and np.array_equal(c.user, p.user) and np.array_equal(c.item, p.item)
        assert (c.bias0 is None) == (f"D{d}" == br.NO_BIAS)


def test_structure_of_m_n_and_e():
    m = br.case_inputs("M")
    du, _ = degrees(m)
    assert br.LOW < du[0] <= br.SEG < du[1] and du[1] % br.SEG != 0 and np.all(du[2:] <= br.LOW)
    assert m.n_items == 2 * br.SEG + 200 and m.n_items - du[1] > 1000
    n, rn = br.case_inputs("N"), br.case_reference("N")
    du, di = degrees(n)
    assert (n.n_users, n.n_items, n.n_sweeps) == (4200, 2, 3) and di[0] == 4200 > br.SEG and di[1] == 50
    assert np.all(du[:50] == 2) and np.all(du[50:] == 1)
    print("N skipped", rn.skipped_per_sweep, "triples", rn.loss_trace[:, 1])
    assert all(100 <= s <= 140 for s in rn.skipped_per_sweep)
    assert all(t > 2 * br.SEG for t in rn.loss_trace[:, 1])          # item 1's negatives: three segments
    e, re_ = br.case_inputs("E"), br.case_reference("E")
    du, di = degrees(e)
    assert np.any(du == 0) and np.any(di == 0)
    assert np.any(re_.item_negative & (di == 0))                      # never positive, drawn as a negative
    assert np.any(~re_.item_counted) and np.any(~re_.user_counted)    # never in any triple


@pytest.mark.parametrize("name", br.T_CASES)
def test_t_cases_sit_on_the_workgroup_edges(name):
    """256 threads build the negative lists: one per edge (the positions) and one per offset."""
    c = br.case_inputs(name)
    assert (len(c.user), c.n_items + 1) in ((256, 256), (257, 257))
    assert c.item.min() > 0 and c.item.max() < c.n_items - 1
    neg = [br.sample(c.user, c.item, c.n_users, c.n_items, c.seed, s) for s in range(c.n_sweeps)]
    assert not np.isin([0, c.n_items - 1], neg[0]).any()   # empty first and last lists
    assert np.isin([0, c.n_items - 1], neg[1]).all()       # and filled ones


@pytest.mark.parametrize("name", br.CASES)
def test_no_case_has_nan_and_counts_add_up(name):
    c, r = br.case_inputs(name), br.case_reference(name)
    assert r.n_nan == 0 and r.triples + r.n_skipped == c.n_sweeps * len(c.user)
    assert r.triples == int(r.loss_trace[:, 1].sum()) and np.all(np.isfinite(r.loss_trace))
    assert np.all(np.isfinite(r.U)) and np.all(np.isfinite(r.V))
    # vertices that never had a triple keep their rows
    assert r.U[~r.user_counted].tobytes() == c.U0[~r.user_counted].tobytes()
    assert r.V[~r.item_counted].tobytes() == c.V0[~r.item_counted].tobytes()


def test_continued_fit_is_the_same_fit():
    for name in ("P", "N"):
        c = br.case_inputs(name)
        a = br.fit(c, n_sweeps=5)
        h = br.fit(c, n_sweeps=2)
        b = br.fit(c, n_sweeps=3, first_sweep=2, U0=h.U, V0=h.V, bias0=h.bias)
        assert a.U.tobytes() == b.U.tobytes() and a.V.tobytes() == b.V.tobytes() and a.bias.tobytes() == b.bias.tobytes()
        assert a.loss_trace[2:].tobytes() == b.loss_trace.tobytes()
