"""Conditions on the NMF checker (tests/nmf_ref.py) and on the cases the GPU tests take from it;
nothing here runs on a device.  The last test needs the built library only."""
import numpy as np
import pytest

import nmf_ref as nr
from collaborative_filtering_amd import _native


@pytest.mark.parametrize("mode", nr.MODES)
@pytest.mark.parametrize("name", nr.CASES)
def test_trace_is_non_increasing(name, mode):
    ref = nr.case_reference(name, mode)
    drop = -np.diff(ref.loss_trace) / np.abs(ref.loss_trace[:-1])
    print(name, mode, ref.loss_trace, drop)
    assert np.all(drop >= -1e-12)      # D = 1 is at its fixed point after one step and only jitters
    assert np.any(drop >= 1e-6)


@pytest.mark.parametrize("name", nr.CASES)
def test_grid_loss_is_edge_form_plus_column_sums(name):
    c, ref = nr.case_inputs(name), nr.case_reference(name, nr.GRID)
    for U, V in ((c.U0, c.V0), (ref.U, ref.V)):
        want, _ = nr.loss(c.user, c.item, c.obs, c.n_users, c.n_items, U, V, nr.GRID)
        got = nr.edge_loss(c.user, c.item, c.obs, U, V, nr.GRID)
        assert abs(got - want) <= 1e-12 * abs(want)
    # and the observed form, from the same dense matrices
    want, scale = nr.loss(c.user, c.item, c.obs, c.n_users, c.n_items, ref.U, ref.V, nr.OBSERVED)
    assert abs(nr.edge_loss(c.user, c.item, c.obs, ref.U, ref.V, nr.OBSERVED) - want) <= 1e-12 * scale


@pytest.mark.parametrize("mode", nr.MODES)
@pytest.mark.parametrize("name", nr.CASES)
def test_no_value_near_the_floor(name, mode):
    """n_floored is comparable exactly: nothing the rule produces lies within a factor 2 of EPS."""
    ref = nr.case_reference(name, mode)
    pre = ref.prefloor
    assert np.all(np.isfinite(pre)) and not np.any((pre > nr.EPS / 2) & (pre < 2 * nr.EPS))
    assert ref.n_floored == int(np.sum(pre < nr.EPS))
    assert np.all(ref.U >= nr.EPS) and np.all(ref.V >= nr.EPS)


def degrees(c):
    return np.bincount(c.user, minlength=c.n_users), np.bincount(c.item, minlength=c.n_items)


@pytest.mark.parametrize("name", ("A", "B"))
def test_structure_of_a_and_b(name):
    lib = _native.load()
    c = nr.case_inputs(name)
    du, di = degrees(c)
    assert (c.n_users, c.n_items, c.D) == (72, 30, 5 if name == "A" else 20)
    assert di.max() > lib.cf_debug_als_low_max() >= di[di > 0].min()      # wave and workgroup paths
    assert np.any(du % 8 != 0) and di.max() % 8 != 0                      # partial lane groups
    assert du[0] == 0 and di[29] == 0                                     # a user without edges, an unrated item
    assert du[1] > 0 and not np.any(c.obs[c.user == 1])                   # a user whose ratings are all 0
    pairs = c.user.astype(np.int64) * c.n_items + c.item
    assert len(np.unique(pairs)) == len(pairs) - 1                        # one repeated edge
    assert np.all(c.obs >= 0)
    if name == "A":
        assert np.all(c.obs == np.round(c.obs)) and c.obs.max() == 5 and c.obs.min() == 0
    else:
        assert np.any(c.obs != np.round(c.obs))
    for mode in nr.MODES:   # user 1 floors in every sweep
        assert nr.case_reference(name, mode).n_floored >= c.D


def test_structure_of_the_d_sweep():
    assert nr.D_SWEEP == (1, 8, 9, 16, 17, 24, 25, 32, 33, 64)
    for d in nr.D_SWEEP:
        c = nr.case_inputs(f"D{d}")
        assert (c.n_users, c.n_items, c.D, c.n_sweeps) == (12, 10, d, 2)


def test_structure_of_h_and_s():
    lib = _native.load()
    seg, R = lib.cf_debug_als_segment(), lib.cf_debug_nmf_sum_rows()
    c = nr.case_inputs("H")
    di = degrees(c)[1]
    assert seg == 2048 and di[0] > seg and di[0] % seg != 0 and (c.D, c.n_items, c.n_sweeps) == (5, 8, 2)
    assert np.all(di[1:] <= seg)
    c = nr.case_inputs("S")
    assert R == 1024 and c.n_items == R + 1 and c.n_users == 8
    assert degrees(c)[1][-1] > 0                                          # the one-row slice is rated


def test_abi_symbols():
    lib = _native.load()
    assert lib.cf_debug_nmf_sum_rows() > 0
    for name in ("cf_nmf_fit", "cf_nmf_loss", "cf_mf_colsum"):
        assert hasattr(lib, name)
