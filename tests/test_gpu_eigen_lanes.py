"""The full-LDS Jacobi kernel's two geometries in buckets 1-8 (cf_set_eigen_lanes): four
lanes per column pair against eight.

The 4-lane form gives a lane the rows of two lanes of the 8-lane form and keeps every reduction's tree
(the 8-lane butterfly's first stage becomes an in-lane add), the blocks shrink to the lane groups the
ordering needs, and the leading dimension may be 48 (mod 64).  None of that changes the arithmetic, so
every output is compared bit for bit (uint32 views, no tolerance):
  - one user at every bucket edge, at odd k (the padding column), in the buckets whose LD changed and
    at k below the lane count, plus k = 129 and 180 (split layout, untouched), on a dense, a sparse and
    an asymmetric graph, with the refinement and the sorted sweeps on and off;
  - 600 users of mixed k in one call (many co-resident blocks per CU), also against the oracle;
  - a small local_calc, whose kLocal and kSigma launches run the same kernel.
tests/test_eigen_geometry.py (CPU) tells which instantiation a setting launches.
"""
import numpy as np
import pytest

import cases
from test_gpu_eigen import _check_batch
from test_gpu_local import build_case

pytestmark = pytest.mark.gpu

KS = [2, 3, 15, 16, 17, 31, 32, 33, 47, 48, 49, 63, 64, 65, 79, 80, 81, 95, 96, 97, 111, 112, 113, 127, 128,
      129, 180]

GRAPHS = {
    "dense": dict(density=0.9, seed=51),
    "sparse": dict(density=0.02, seed=52, isolated_frac=0.2),
    # the two directions of an edge differ in the last digit (cases.item_graph's asym), at a density
    # that leaves lower and upper triangle visibly different after thresholding
    "asym": dict(density=0.3, seed=53, asym=True),
}


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


def _assert_same_bits(r8, r4, n_users, label):
    assert np.array_equal(r8.m, r4.m), label
    for u in range(n_users):
        for name, x, y in zip(("sigs", "evals", "evecs"), r8.block(u), r4.block(u)):
            assert x.shape == y.shape and np.array_equal(_bits(x), _bits(y)), (label, u, name)


def _run_both(ctx, off, items):
    try:
        ctx.set_eigen_lanes(8)
        r8 = ctx.eigen_batch(off, items)
        ctx.set_eigen_lanes(4)
        r4 = ctx.eigen_batch(off, items)
    finally:
        ctx.set_eigen_lanes(0)
    return r8, r4


@pytest.fixture(scope="module")
def unsorted_ctx():
    """A context whose sweeps keep the columns in place (CF_EIGEN_SORT is read at creation)."""
    import os

    from collaborative_filtering_amd.api import Context

    old = os.environ.get("CF_EIGEN_SORT")
    os.environ["CF_EIGEN_SORT"] = "0"
    try:
        ctx = Context(0)
    finally:
        if old is None:
            del os.environ["CF_EIGEN_SORT"]
        else:
            os.environ["CF_EIGEN_SORT"] = old
    yield ctx
    ctx.close()


@pytest.fixture(scope="module")
def graphs():
    out = {}
    for name, kw in GRAPHS.items():
        W = cases.item_graph(260, **kw)
        if name == "asym":   # make the asymmetry matter: drop a tenth of the edges in one direction only
            rng = np.random.default_rng(54)
            W = np.where(np.triu(rng.random(W.shape) < 0.1, 1), 0.0, W).astype(np.float32)
        off, items = cases.user_items(260, KS, seed=kw["seed"] + 100)
        out[name] = (W, off, items)
    return out


@pytest.mark.parametrize("sort", [True, False])
@pytest.mark.parametrize("refine", [True, False])
@pytest.mark.parametrize("graph", list(GRAPHS))
def test_lanes4_bit_equal_to_lanes8(gpu_ctx, unsorted_ctx, graphs, graph, refine, sort):
    ctx = gpu_ctx if sort else unsorted_ctx
    W, off, items = graphs[graph]
    ctx.upload_graph_dense(W)
    ctx.set_eigen_refine(refine)
    try:
        r8, r4 = _run_both(ctx, off, items)
    finally:
        ctx.set_eigen_refine(True)
    _assert_same_bits(r8, r4, len(KS), (graph, refine, sort))


def test_many_mixed_users_bit_equal_and_oracle(gpu_ctx):
    rng = np.random.default_rng(61)
    ks = rng.integers(20, 129, size=600)
    W = cases.item_graph(300, 0.3, seed=62)
    off, items = cases.user_items(300, ks, seed=63)
    gpu_ctx.upload_graph_dense(W)
    r8, r4 = _run_both(gpu_ctx, off, items)
    _assert_same_bits(r8, r4, len(ks), "mixed")
    try:
        gpu_ctx.set_eigen_lanes(4)
        _check_batch(gpu_ctx, W, off, items, "mixed-lanes4")
    finally:
        gpu_ctx.set_eigen_lanes(0)


def test_local_calc_bit_equal(gpu_ctx):
    """kLocal (the movies' eigenpairs) and kSigma (w_lim per pair) in both geometries."""
    G, test = build_case(7, n_items=60, n_users=20)
    n_items = G.shape[0]
    toff = np.zeros(n_items + 1, np.uint64)
    tuser, trat = [], []
    for mv in range(n_items):
        us = sorted(test.get(mv, {}))
        tuser += us
        trat += [test[mv][u] for u in us]
        toff[mv + 1] = toff[mv] + len(us)
    moff, mitems = [0], []
    for mv in range(n_items):
        mitems += [mv] + [j for j in range(n_items) if float(G[mv, j]) > 0.1]
        moff.append(len(mitems))
    sizes = np.diff(moff)
    assert sizes.min() >= 3 and len({(int(s) + 15) // 16 for s in sizes}) >= 2   # more than one bucket
    gpu_ctx.upload_graph_dense(G)
    outs = {}
    try:
        for lanes in (8, 4):
            gpu_ctx.set_eigen_lanes(lanes)
            outs[lanes] = gpu_ctx.local_calc(np.array(moff), np.array(mitems), toff, np.array(tuser), np.array(trat))
    finally:
        gpu_ctx.set_eigen_lanes(0)
    for name, x, y in zip(("mse", "kk", "pred", "w_lim", "lim"), outs[8], outs[4]):
        x, y = np.ascontiguousarray(x), np.ascontiguousarray(y)
        assert x.dtype == y.dtype and np.array_equal(x.view(np.uint8), y.view(np.uint8)), name
    assert np.isfinite(outs[4][3]).any()   # some w_lim was computed
