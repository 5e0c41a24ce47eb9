"""Graph-signal polynomial filters: cheby.cpp:152-274, binomials.cpp:145-253.

CPU: the oracle's superstep restatement (oracle/cf_oracle.cpp cfo_graph_filter) against
numpy closed forms on a dense matrix -- the Chebyshev series y = c0/2 x + sum_k c_k T_k(L - I) x
(T_1 = L - I, T_{k+1} = 2 (L - I) T_k - T_{k-1}; a1 = a2 = 1 for arange [0, 2]) and the
binomial product x <- (c_i I + c_{i+1} L + c_{i+2} L^2) x over rounds i with 3i < n_coeff
(ind = i: overlapping windows, binomials.cpp:357), L = I - D^-1/2 W D^-1/2 with W summing
parallel edges.  GPU: cf_graph_filter against the oracle (fp64 both sides, rel 1e-9).
Parity unpinned against the reference binaries (GraphLab is not buildable here); the
duplicate-edge rule (parallel edges kept) is this restatement's reading of add_edge.

The shapes where the kernel branches (tests/filter_ref.py).  cf_graph_filter gives every vertex
row a group of G = 4 / 16 / 64 lanes from the mean degree (cf_debug_filter_lanes tells which; the
tests never copy the thresholds); a lane enters the 4-deep unrolled gather only while
p + 3 G < e, so within one row some lanes take it and others the tail loop; n G meets the
256-thread block.  Three unions of complete bipartite graphs, one per G, prescribe the row
lengths {0, 1, G-1, G, G+1, 3G, 3G+1, 4G-1, 4G, 4G+1, 8G+3} (the G = 4 one adds a 5000-entry hub
row, self-lines and sub-threshold lines), and small graphs put n G one group below, at and above a
block, n = 1 and n < G.  The judge is a longdouble reference that makes no call into the oracle:
- short filters (3..7 coefficients: every phase of the t_old / t_cur / t_new rotation, and 1, 2, 3
  binomial rounds, so the result lands in either ping-pong buffer), random signals:
  |y_gpu - y_ref| <= bound per vertex, the reference's running forward-error bound of any fp64
  evaluation (derived in filter_ref.reference);
- long filters (12, 33, 64 coefficients, scaled so that max|y| / max|x| stays in [0.1, 10],
  asserted on the reference): max|y_gpu - y_ref| / max|y_ref| <= BOUND_LONG[n_coeff], at least
  200 times the fp64 drift that test_drift_sets_the_device_bounds measures on the CPU and never
  looser than 1e-9;
- eigenvector signals (S x = x on any graph, S x = -x on a bipartite one, S x = 0 on isolated
  vertices) against closed forms, independently of the reference, with coefficients whose three
  closed-form factors all lie in [0.1, 10] (asserted): no family is compared at the level of noise;
- bits: repeated calls, a part alone against the part inside its union, untouched inputs;
- the edge rule at w = 0.1 and the argument checks.

Observed on the MI355X: short filters use at most 0.224 of the running bound (0.154 on the
unions, the rest on the edge graphs; both kinds); long filters are within 9.3e-15 at 12, 4.7e-14
at 33 and 4.2e-14 at 64 coefficients of the reference (bounds 2e-11, 2e-10, 2e-10; the largest on
the G = 4 union with its hub row) and within 1.5e-13 max|x| of the closed forms, whose factors
all lie in [0.25, 2.9]; the four random
cases of test_gpu_filters_match_oracle are within 3.3e-14 max|y| of the oracle (bound 1e-11).
"""
import numpy as np
import pytest

import filter_ref as fr
import oracle_ref as orc
from collaborative_filtering_amd import _native
from collaborative_filtering_amd._native import ptr
from collaborative_filtering_amd.api import CF_FILTER_BINOMIAL, CF_FILTER_CHEBY
from filter_ref import BOUND_LONG, BOUND_RANDOM, CLOSED_FORM_FLOOR, MARGIN

KINDS = (CF_FILTER_CHEBY, CF_FILTER_BINOMIAL)
RANDOM_CASES = [(60, 400, 3), (500, 20000, 64), (3000, 5000, 17), (2000, 300000, 10)]
SHORT_KEYS = [4, 16, 64] + [e[0] for e in fr.EDGE_GRAPHS]


def random_topology(n, n_lines, seed, isolated=3):
    rng = np.random.default_rng(seed)
    va = rng.integers(0, n - isolated, n_lines)
    vb = rng.integers(0, n - isolated, n_lines)
    w = np.round(rng.random(n_lines), 2)          # mega_graph.py writes '{0:.2f}' weights
    va[:5] = vb[:5]                               # self-lines (dropped)
    va[5:10], vb[5:10] = vb[10:15], va[10:15]     # reversed duplicates (parallel edges)
    signal = rng.uniform(0, 10, n)
    return va.astype(np.int64), vb.astype(np.int64), w, signal


def random_coefficients(n_coeff):
    return np.random.default_rng(7).normal(size=n_coeff) / np.sqrt(n_coeff)


def dense_L(n, va, vb, w):
    W = np.zeros((n, n))
    for a, b, x in zip(va, vb, w):
        if x > 0.1 and a != b:
            W[a, b] += x
            W[b, a] += x
    d = W.sum(1)
    s = np.where(d > 0, 1.0 / np.sqrt(np.where(d > 0, d, 1.0)), 0.0)
    return np.eye(n) - s[:, None] * W * s[None, :]


def cheby_dense(L, x, c):
    M = L - np.eye(len(x))
    t_old, t_cur = x, M @ x
    y = 0.5 * c[0] * t_old + c[1] * t_cur
    for k in range(2, len(c)):
        t_new = 2 * (M @ t_cur) - t_old
        y = y + c[k] * t_new
        t_old, t_cur = t_cur, t_new
    return y


def binomial_dense(L, x, c):
    i = 0
    while 3 * i < len(c):
        x = c[i] * x + c[i + 1] * (L @ x) + c[i + 2] * (L @ (L @ x))
        i += 1
    return x


def lanes(n, va, vb, w):
    """The G cf_graph_filter takes for these lines (asked of the library, not restated)."""
    kept = int(np.sum((np.asarray(w) > 0.1) & (np.asarray(va) != np.asarray(vb))))
    return int(_native.load().cf_debug_filter_lanes(int(n), 2 * kept))


def assert_gains_of_order_one(kind, c):
    """On the closed form: every eigenvector family (S x = x, S x = -x, S x = 0 on isolated vertices)
    comes out at the scale of the input, so no closed-form comparison is one of noise."""
    g = fr.gains(kind, c)
    assert all(0.1 <= abs(f) <= 10.0 for f in g), (kind, len(c), g)


def relmax(y, y_ref, den):
    return float(np.max(np.abs(np.asarray(y).astype(fr.LD) - y_ref)) / den)


def bound_ratio(y, y_ref, bound):
    """max err / bound over the vertices (0 / 0 counts as 0: an exact result under a zero bound)."""
    err = np.abs(np.asarray(y).astype(fr.LD) - y_ref)
    assert np.all(err <= bound), (int(np.argmax(err - bound)), float(np.max(err - bound)))
    return float(np.max(np.where(bound > 0, err / np.where(bound > 0, bound, 1), 0)))


@pytest.mark.parametrize("n_coeff", [3, 4, 10, 33])
def test_oracle_filters_match_closed_forms(n_coeff):
    n = 60
    va, vb, w, x = random_topology(n, 400, seed=n_coeff)
    c = np.random.default_rng(99).normal(size=n_coeff)
    L = dense_L(n, va, vb, w)
    y0 = orc.graph_filter(0, n, va, vb, w, x, c)
    y1 = orc.graph_filter(1, n, va, vb, w, x, c)
    np.testing.assert_allclose(y0, cheby_dense(L, x, c), rtol=1e-10, atol=1e-9)
    np.testing.assert_allclose(y1, binomial_dense(L, x, c), rtol=1e-10, atol=1e-9)
    # isolated vertices: no gather, (L - I) acts as 0 there, so T_k x = T_k(0) x = cos(k pi/2) x
    f0 = 0.5 * c[0] + sum(c[k] * np.cos(k * np.pi / 2) for k in range(1, n_coeff))
    np.testing.assert_allclose(y0[-3:], f0 * x[-3:], rtol=1e-9, atol=1e-12)


# ---- the reference, the bounds and the cases (CPU) ----------------------------------------------------
@pytest.mark.parametrize("G", [4, 16, 64])
def test_reference_matches_closed_forms(G):
    """Both eigenvector families and the isolated vertices, both kinds, 3 to 64 coefficients: the
    longdouble reference reproduces the closed form to the rounding of its fp64 input, a few 1e-16
    of max|x| (printed by -s; CLOSED_FORM_FLOOR holds it)."""
    u = fr.union(G)
    assert u.isolated.sum() == 3
    worst = 0.0
    for kind in KINDS:
        for n_coeff in fr.SHORT + fr.LONG:
            for mu in (1, -1):
                if n_coeff in fr.LONG:
                    _, x, c, y = fr.long_case(G, kind, n_coeff, mu)
                else:
                    x = fr.eigen_signal(u, mu, seed=n_coeff)
                    c = fr.balanced_coefficients(kind, n_coeff, seed=3000 + n_coeff)
                    y = fr.reference(kind, u.n, u.va, u.vb, u.w, x, c, with_bound=False)[0]
                assert_gains_of_order_one(kind, c)
                d = relmax(fr.closed_form(kind, x, c, mu, u.isolated), y, np.abs(x).max())
                worst = max(worst, d)
                assert d <= CLOSED_FORM_FLOOR, (kind, n_coeff, mu, d)
    print(f"G = {G}: reference against closed forms, worst {worst:.3g} max|x|")


@pytest.mark.parametrize("key", SHORT_KEYS)
def test_oracle_inside_the_running_bound(key):
    """The oracle's fp64 output lies inside the reference's per-vertex bound on every short-filter
    case, and at 3 coefficients the bound is tight: median bound / |y| below 1e-11 (2.4e-12 on the
    G = 4 union with its 5000-entry row, 1e-13 on the others)."""
    worst = 0.0
    for kind in KINDS:
        for n_coeff in fr.SHORT:
            u, x, c, (y, bound) = fr.short_case(key, kind, n_coeff)
            worst = max(worst, bound_ratio(orc.graph_filter(kind, u.n, u.va, u.vb, u.w, x, c), y, bound))
            nz = np.abs(y) > 0
            assert n_coeff > 3 or np.median(bound[nz] / np.abs(y[nz])) < 1e-11
    print(f"{key}: oracle uses at most {worst:.3g} of the running bound")
    assert worst > 0


@pytest.mark.parametrize("G", [4, 16, 64])
def test_running_bound_catches_one_dropped_edge(G):
    """The bound bites: an fp64 evaluation of the graph with one line removed leaves it."""
    u, x, c, (y, bound) = fr.short_case(G, CF_FILTER_CHEBY, 3)
    line = int(np.nonzero((u.w > 0.1) & (u.va != u.vb))[0][0])
    keep = np.arange(len(u.w)) != line
    y_bad = fr.fp64_filter(CF_FILTER_CHEBY, u.n, u.va[keep], u.vb[keep], u.w[keep], x, c, ("lanes", G))
    assert np.any(np.abs(y_bad.astype(fr.LD) - y) > bound)


def test_drift_sets_the_device_bounds():
    """The fp64 oracle and an fp64 numpy restatement under four further summation orders (edges
    permuted; rows summed in lane-strided partials of 4, 16 and 64) against the longdouble
    reference, on every long-filter case: max|y - y_ref| / max|y_ref| for random signals, / max|x|
    for the eigenvector signals the closed-form tests use.  Measured here (printed by -s): at most
    6.3e-14 at 12, 3.1e-13 at 33 and 6.3e-13 at 64 coefficients, and 3.1e-14 on the random
    topologies of test_gpu_filters_match_oracle.  Each device bound keeps MARGIN = 200 above its
    drift and is no looser than the 1e-9 of test_gpu_filters_match_oracle."""
    orders = [("perm", 1), ("lanes", 4), ("lanes", 16), ("lanes", 64)]

    def drifts(kind, n, va, vb, w, x, c, y, den):
        d = [relmax(orc.graph_filter(kind, n, va, vb, w, x, c), y, den)]
        return d + [relmax(fr.fp64_filter(kind, n, va, vb, w, x, c, o), y, den) for o in orders]

    for n_coeff in fr.LONG:
        worst = 0.0
        for kind in KINDS:
            for G in (4, 16, 64):
                for signal in ("random", 1, -1):
                    u, x, c, y = fr.long_case(G, kind, n_coeff, signal)
                    den = np.abs(y).max() if signal == "random" else np.abs(x).max()
                    d = drifts(kind, u.n, u.va, u.vb, u.w, x, c, y, den)
                    print(f"n_coeff {n_coeff} kind {kind} G {G} signal {signal}: drift", " ".join(f"{v:.2g}" for v in d))
                    worst = max(worst, *d)
        print(f"n_coeff {n_coeff}: largest drift {worst:.3g}, bound {BOUND_LONG[n_coeff]:.3g}")
        assert worst > 0 and MARGIN * worst <= BOUND_LONG[n_coeff] <= 1e-9
    worst = 0.0
    for n, n_lines, n_coeff in RANDOM_CASES:
        va, vb, w, x = random_topology(n, n_lines, seed=n + n_coeff)
        c = random_coefficients(n_coeff)
        for kind in KINDS:
            y = fr.reference(kind, n, va, vb, w, x, c, with_bound=False)[0]
            d = drifts(kind, n, va, vb, w, x, c, y, np.abs(y).max())
            print(f"random {(n, n_lines, n_coeff)} kind {kind}: max|y| {float(np.abs(y).max()):.3g} drift",
                  " ".join(f"{v:.2g}" for v in d))
            worst = max(worst, *d)
    assert worst > 0 and MARGIN * worst <= BOUND_RANDOM <= 1e-9


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("n_coeff", fr.LONG)
@pytest.mark.parametrize("G", [4, 16, 64])
def test_long_filter_outputs_are_of_the_input_scale(G, n_coeff, kind):
    """scaled_coefficients keeps max|y| / max|x| in [0.1, 10]: no long case compares noise."""
    _, x, _, y = fr.long_case(G, kind, n_coeff)
    assert 0.1 <= float(np.abs(y).max() / np.abs(x).max()) <= 10.0


def test_row_lengths_and_lane_widths():
    """The prescribed row lengths are present and cf_debug_filter_lanes reports the intended G for
    every union and edge graph; at the thresholds a graph with nnz / n exactly 8 (48) takes 16 (64)
    lanes and the same graph with one isolated vertex more takes 4 (16)."""
    lib = _native.load()
    for G in (4, 16, 64):
        u = fr.union(G)
        g = fr.Csr(u.n, u.va, u.vb, u.w)
        have = set(np.nonzero(np.bincount(g.len))[0].tolist())
        assert set(fr.lane_lengths(G)) <= have, sorted(set(fr.lane_lengths(G)) - have)
        assert g.nnz == 2 * u.kept and lanes(u.n, u.va, u.vb, u.w) == G
        # lanes that take the unrolled gather beside lanes that only take the tail, in one row
        assert np.any((g.len > 3 * G) & (g.len < 4 * G))
    assert 5000 in fr.Csr(fr.union(4).n, fr.union(4).va, fr.union(4).vb, fr.union(4).w).len
    for name, G, _ in fr.EDGE_GRAPHS:
        u = fr.edge_graph(name)
        assert lanes(u.n, u.va, u.vb, u.w) == G, name
    blocks = {name: fr.edge_graph(name).n * G for name, G, _ in fr.EDGE_GRAPHS}
    for G, names in ((4, ("g4_n63", "g4_n64", "g4_n65")), (16, ("g16_n31", "g16_n32", "g16_n33")),
                     (64, ("g64_n127", "g64_n128", "g64_n129"))):
        assert [blocks[m] % 256 for m in names] == [256 - G, 0, G]
    assert fr.edge_graph("n1").n == 1 and fr.edge_graph("g4_n2").n < 4
    assert fr.edge_graph("g16_n7").n < 16 and fr.edge_graph("g64_n7").n < 64
    # K_{8,8}: 16 vertices, 128 directed edges; K_{24,24}: 48 vertices, 2304 directed edges
    assert lib.cf_debug_filter_lanes(16, 128) == 16 and lib.cf_debug_filter_lanes(17, 128) == 4
    assert lib.cf_debug_filter_lanes(48, 2304) == 64 and lib.cf_debug_filter_lanes(49, 2304) == 16
    assert lib.cf_debug_filter_lanes(0, 0) == 4 and lib.cf_debug_filter_lanes(5, 0) == 4


def test_union_builder():
    """Extras of bipartite_union: parallel edges lengthen the last part's rows only; self-lines and
    sub-threshold lines are present in the file and dropped by the edge rule."""
    u = fr.bipartite_union([(2, 3), (4, 5)], seed=1, isolated=2, duplicates=6, self_lines=3, sub_threshold=4)
    g = fr.Csr(u.n, u.va, u.vb, u.w)
    assert len(u.w) == 6 + 20 + 6 + 3 + 4 and u.kept == 32 and g.nnz == 64
    assert np.sum(u.va == u.vb) >= 3 and np.sum(u.w <= 0.1) == 4 and np.all(u.w[u.w > 0.1] <= 1.0)
    assert sorted(g.len[u.part_vertices[0]].tolist()) == [2, 2, 2, 3, 3]
    assert g.len[u.part_vertices[1]].sum() == 2 * 26 and np.all(g.len[u.isolated] == 0)
    assert np.all(u.side[u.va[u.part_lines[0]]] * u.side[u.vb[u.part_lines[0]]] == -1)
    n, va, vb, w, vid = fr.sub_union(u, 1)
    assert n == 9 and len(w) == 26 and np.array_equal(vid[va], u.va[u.part_lines[1]])


# ---- the device ---------------------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("n,n_lines,n_coeff", RANDOM_CASES)
def test_gpu_filters_match_oracle(gpu_ctx, n, n_lines, n_coeff):
    """Row groups of 4 / 16 / 64 lanes (mean degree ~13, ~80, ~3, ~300)."""
    va, vb, w, x = random_topology(n, n_lines, seed=n + n_coeff)
    c = random_coefficients(n_coeff)
    for kind in (CF_FILTER_CHEBY, CF_FILTER_BINOMIAL):
        y_g, ms, ne = gpu_ctx.graph_filter(kind, n, va, vb, w, x, c)
        y_o = orc.graph_filter(kind, n, va, vb, w, x, c)
        scale = max(1.0, float(np.abs(y_o).max()))
        assert np.abs(y_g - y_o).max() <= 1e-9 * scale, (kind, np.abs(y_g - y_o).max(), scale)
        assert ne == 2 * int(np.sum((w > 0.1) & (va != vb)))
        # relative to the output's own scale (8.4e-19 for the 64-coefficient binomial case)
        rel = float(np.abs(y_g - y_o).max() / np.abs(y_o).max())
        print(f"{(n, n_lines, n_coeff)} kind {kind}: max|y_gpu - y_oracle| / max|y_oracle| = {rel:.3g}")
        assert np.abs(y_o).max() > 0 and rel <= BOUND_RANDOM, (kind, rel)


@pytest.mark.gpu
@pytest.mark.parametrize("key", SHORT_KEYS)
def test_gpu_short_filters_inside_the_running_bound(gpu_ctx, key):
    worst = 0.0
    for kind in KINDS:
        for n_coeff in fr.SHORT:
            u, x, c, (y, bound) = fr.short_case(key, kind, n_coeff)
            y_g, _, ne = gpu_ctx.graph_filter(kind, u.n, u.va, u.vb, u.w, x, c)
            assert ne == 2 * u.kept
            r = bound_ratio(y_g, y, bound)
            print(f"{key} kind {kind} n_coeff {n_coeff}: err / bound {r:.3g}")
            worst = max(worst, r)
    print(f"{key}: the device uses at most {worst:.3g} of the running bound")


@pytest.mark.gpu
@pytest.mark.parametrize("n_coeff", fr.LONG)
@pytest.mark.parametrize("G", [4, 16, 64])
def test_gpu_long_filters(gpu_ctx, G, n_coeff):
    for kind in KINDS:
        u, x, c, y = fr.long_case(G, kind, n_coeff)
        assert 0.1 <= float(np.abs(y).max() / np.abs(x).max()) <= 10.0     # on the reference
        y_g, _, _ = gpu_ctx.graph_filter(kind, u.n, u.va, u.vb, u.w, x, c)
        rel = relmax(y_g, y, np.abs(y).max())
        print(f"G {G} kind {kind} n_coeff {n_coeff}: max|y_gpu - y_ref| / max|y_ref| = {rel:.3g}")
        assert rel <= BOUND_LONG[n_coeff], (kind, rel)


@pytest.mark.gpu
@pytest.mark.parametrize("n_coeff", fr.LONG)
@pytest.mark.parametrize("G", [4, 16, 64])
def test_gpu_filters_match_closed_forms(gpu_ctx, G, n_coeff):
    """Eigenvector inputs (mu = +1, mu = -1; the three isolated vertices hold random values) against
    closed_form alone, relative to max|x| as test_reference_matches_closed_forms measures it."""
    u = fr.union(G)
    for kind in KINDS:
        c = fr.balanced_coefficients(kind, n_coeff, seed=3000 + n_coeff)
        assert_gains_of_order_one(kind, c)
        for mu in (1, -1):
            x = fr.eigen_signal(u, mu, seed=n_coeff)
            y_cf = fr.closed_form(kind, x, c, mu, u.isolated)
            y_g, _, _ = gpu_ctx.graph_filter(kind, u.n, u.va, u.vb, u.w, x, c)
            rel = relmax(y_g, y_cf, np.abs(x).max())
            print(f"G {G} kind {kind} n_coeff {n_coeff} mu {mu}: max|y_gpu - closed form| / max|x| = {rel:.3g}")
            assert rel <= BOUND_LONG[n_coeff] + CLOSED_FORM_FLOOR, (kind, mu, rel)
            iso = u.isolated
            assert relmax(y_g[iso], y_cf[iso], np.abs(x[iso]).max()) <= BOUND_LONG[n_coeff] + CLOSED_FORM_FLOOR


@pytest.mark.gpu
@pytest.mark.parametrize("G", [4, 16, 64])
def test_gpu_filter_bits(gpu_ctx, G):
    """No atomics, and a row's sum depends on its own row only: a repeated call gives the same bits,
    and a K_{a,b} on its own (same relative line order) gives its vertices the bits they have inside
    the union whenever both graphs take the same G.  The inputs are not written."""
    u = fr.union(G)
    x = fr.random_signal(u, seed=31)
    matched = 0
    for kind, n_coeff in ((CF_FILTER_CHEBY, 5), (CF_FILTER_BINOMIAL, 4), (CF_FILTER_BINOMIAL, 7)):
        c = np.random.default_rng(n_coeff).normal(size=n_coeff)
        args = [np.ascontiguousarray(u.va, np.uint32), np.ascontiguousarray(u.vb, np.uint32), u.w.copy(), x.copy(), c.copy()]
        saved = [a.copy() for a in args]
        y1, _, ne = gpu_ctx.graph_filter(kind, u.n, *args)
        y2, _, _ = gpu_ctx.graph_filter(kind, u.n, *args)
        assert all(np.array_equal(a, b) for a, b in zip(args, saved))
        assert ne == 2 * u.kept
        assert np.array_equal(y1.view(np.uint64), y2.view(np.uint64))
        for p in range(len(u.parts)):
            n, va, vb, w, vid = fr.sub_union(u, p)
            if lanes(n, va, vb, w) != G:
                continue
            y_p, _, _ = gpu_ctx.graph_filter(kind, n, va, vb, w, x[vid], c)
            assert np.array_equal(y_p.view(np.uint64), y1[vid].view(np.uint64)), (kind, p)
            matched += 1
    assert matched >= 6, matched


def raw_filter(ctx, kind, n, va, vb, w, x, c, out, n_lines=None, n_coeff=None):
    """cf_graph_filter's return code (None passes a null pointer)."""
    conv = lambda a, t: None if a is None else np.ascontiguousarray(a, t)   # noqa: E731
    va, vb, w, x, c = conv(va, np.uint32), conv(vb, np.uint32), conv(w, np.float64), conv(x, np.float64), conv(c, np.float64)
    return ctx.lib.cf_graph_filter(ctx.h, int(kind), int(n), len(w) if n_lines is None else n_lines, ptr(va), ptr(vb),
                                   ptr(w), ptr(x), ptr(c), len(c) if n_coeff is None else n_coeff, ptr(out))


@pytest.mark.gpu
def test_gpu_filter_edge_rule(gpu_ctx):
    """w == 0.1 is dropped and the next double above it kept (w > 0.1, cheby.cpp:88); NaN and
    negative weights are dropped; an index out of range is an error on a kept line only."""
    above = np.nextafter(0.1, 1)
    va = np.array([0, 1, 2, 3, 4, 0, 6])
    vb = np.array([1, 2, 3, 4, 5, 5, 5])
    w = np.array([0.5, 0.1, above, 0.7, np.nan, -0.5, -np.inf])
    n = 7
    x = np.random.default_rng(1).uniform(-10, 10, n)
    c = np.random.default_rng(2).normal(size=4)
    kept = np.array([0, 2, 3])
    for kind in KINDS:
        y, _, ne = gpu_ctx.graph_filter(kind, n, va, vb, w, x, c)
        assert ne == 6
        y_k, _, _ = gpu_ctx.graph_filter(kind, n, va[kept], vb[kept], w[kept], x, c)
        assert np.array_equal(y.view(np.uint64), y_k.view(np.uint64))
        y_ref, bound = fr.reference(kind, n, va[kept], vb[kept], w[kept], x, c)
        bound_ratio(y, y_ref, bound)
        # vertices 5 and 6 have no kept line: the isolated closed form
        iso = np.zeros(n, bool)
        iso[5:] = True
        assert np.all(np.abs(y[iso] - fr.closed_form(kind, x, c, 1, iso)[iso]) <= bound[iso] * 1.001)
        # out of range on a dropped line and on a self-line: accepted, and changes nothing
        va2, vb2, w2 = np.append(va, [1000, 2000]), np.append(vb, [3, 2000]), np.append(w, [0.05, 0.9])
        y2, _, ne2 = gpu_ctx.graph_filter(kind, n, va2, vb2, w2, x, c)
        assert ne2 == 6 and np.array_equal(y2.view(np.uint64), y.view(np.uint64))
        out = np.full(n, -7.0)
        for bad_a, bad_b in ((n, 3), (3, n), (2 ** 32 - 1, 0)):
            rc = raw_filter(gpu_ctx, kind, n, np.append(va, bad_a), np.append(vb, bad_b), np.append(w, above), x, c, out)
            assert rc == _native.CF_EINVAL and np.all(out == -7.0)


@pytest.mark.gpu
def test_gpu_filter_arguments(gpu_ctx):
    u = fr.edge_graph("g4_n63")
    x = fr.random_signal(u, seed=3)
    c = np.random.default_rng(4).normal(size=5)
    out = np.full(u.n, -7.0)
    for kind in KINDS:
        for short in (0, 1, 2):       # both reference programs read coeff[2]
            assert raw_filter(gpu_ctx, kind, u.n, u.va, u.vb, u.w, x, c, out, n_coeff=short) == _native.CF_EINVAL
    for kind in (-1, 2):
        assert raw_filter(gpu_ctx, kind, u.n, u.va, u.vb, u.w, x, c, out) == _native.CF_EINVAL
    assert np.all(out == -7.0)
    for kind in KINDS:
        # no vertices: a no-op that leaves out untouched (with lines that are all dropped, and with none)
        assert raw_filter(gpu_ctx, kind, 0, [0], [0], [0.5], None, c, out) == _native.CF_OK
        assert raw_filter(gpu_ctx, kind, 0, None, None, None, None, c, out, n_lines=0) == _native.CF_OK
        assert np.all(out == -7.0)
        # isolated vertices only: null line pointers with no lines, and lines that are all dropped
        iso = np.ones(u.n, bool)
        y_cf = fr.closed_form(kind, x, c, 1, iso)
        _, bound = fr.reference(kind, u.n, [], [], [], x, c)
        for lines in ((None, None, None), ([0, 1, 5], [0, 2, 6], [0.9, 0.1, 0.03])):
            got = np.full(u.n, -7.0)
            assert raw_filter(gpu_ctx, kind, u.n, *lines, x, c, got, n_lines=0 if lines[0] is None else 3) == _native.CF_OK
            assert np.all(np.abs(got - y_cf) <= bound * 1.001)
            ms, ne = np.zeros(1, np.float32), np.zeros(1, np.uint64)
            assert gpu_ctx.lib.cf_graph_filter_timing(gpu_ctx.h, ptr(ms), ptr(ne)) == _native.CF_OK and int(ne[0]) == 0


@pytest.mark.gpu
@pytest.mark.parametrize("binary,kind", [("cheby", 0), ("binomials", 1)])
def test_filter_binaries(tmp_path, binary, kind):
    """bin/cheby and bin/binomials on mega_graph.py-shaped files (ids from 1, '{:.2f}'
    weights, both directions possible as separate lines) plus a topology-only vertex and a
    sub-threshold line; graph_filtered_signal_1_of_1 against the oracle to the 6 printed digits.
    The file contract of cf_filter_cli.hpp beyond that: topology and signal spread over several
    files of the prefix, a vertex given twice in graph_signal (the last line wins), and ids with
    large gaps (every id of the first run is multiplied by 9973 in a second one)."""
    import os
    import subprocess

    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    rng = np.random.default_rng(5)
    n = 400
    links = set()
    while len(links) < 0.02 * n * n:
        a, b = int(rng.integers(1, n + 1)), int(rng.integers(1, n + 1))
        if a != b:
            links.add((a, b))
    lines = [(a, b, round(float(rng.random()), 2)) for a, b in sorted(links)]
    lines += [(n + 7, 3, 0.5), (n + 9, 4, 0.05)]       # topology-only vertex; a dropped line
    sig = {i: float(rng.uniform(0, 10)) for i in range(1, n + 1)}
    coeff = rng.normal(size=12)

    def run(folder, gap, split):
        folder.mkdir()
        topo = [f"{a * gap} {b * gap} {w:.2f}\n" for a, b, w in lines]
        sigl = [f"{i * gap} {v!r}\n" for i, v in sig.items()]
        if split:
            # stale values first: id 17's winning line follows in the same file; id n's is in
            # graph_signal_b, so that one also pins that the files are read in name order
            sigl = [f"{17 * gap} 123.5\n", f"{n * gap} -4.25\n"] + sigl
            h, k = len(topo) // 3, len(sigl) // 2
            (folder / "graph_topology_a").write_text("".join(topo[:h]))
            (folder / "graph_topology_b").write_text("".join(topo[h:]))
            (folder / "graph_signal_b").write_text("".join(sigl[k:]))
            (folder / "graph_signal_a").write_text("".join(sigl[:k]))
            assert k > 18
        else:
            (folder / "graph_topology.txt").write_text("".join(topo))
            (folder / "graph_signal.txt").write_text("".join(sigl))
        (folder / "coeff.txt").write_text(" ".join(repr(float(c)) for c in coeff) + "\n")
        subprocess.run([os.path.join(root, "bin", binary)], cwd=folder, check=True, timeout=120,
                       capture_output=True)
        got = {}
        for ln in (folder / "graph_filtered_signal_1_of_1").read_text().split("\n"):
            if ln.strip():
                i, v = ln.split()
                got[int(i)] = float(v)
        return got

    ids = sorted(set(sig) | {a for a, b, w in lines if w > 0.1} | {b for a, b, w in lines if w > 0.1})
    pos = {v: i for i, v in enumerate(ids)}
    va = np.array([pos[a] for a, b, w in lines if w > 0.1])
    vb = np.array([pos[b] for a, b, w in lines if w > 0.1])
    w = np.array([w for a, b, w in lines if w > 0.1])
    x = np.array([sig.get(v, 0.0) for v in ids])
    y = orc.graph_filter(kind, len(ids), va, vb, w, x, coeff)
    got = run(tmp_path / "plain", 1, False)
    assert sorted(got) == ids
    for v, i in pos.items():
        assert abs(got[v] - y[i]) <= 1e-5 * max(1.0, abs(y[i])), (v, got[v], y[i])
    gap = 9973                                         # ids up to 4.08e6 for 402 vertices
    got_split = run(tmp_path / "split", gap, True)
    assert sorted(got_split) == [v * gap for v in ids]
    assert all(got_split[v * gap] == got[v] for v in ids)      # the same bits, printed alike
