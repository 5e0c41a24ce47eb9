"""A high-precision reference of the graph-signal filters (cf_graph_filter: cheby.cpp:152-274,
binomials.cpp:145-253), independent of the oracle: plain numpy in np.longdouble (80-bit on
x86-64) over a CSR built from the topology lines, with the kernel's edge rule -- a line is kept
iff w > 0.1 and va != vb, a kept line adds both directions, parallel edges are kept.  No dense
matrix, no call into oracle/.

reference()            the filtered signal and a per-vertex forward-error bound for ANY fp64
                       evaluation of the same supersteps (derivation in its docstring);
closed_form()          the exact output for eigenvector inputs of S = D^-1/2 W D^-1/2;
bipartite_union()      the input builder: unions of complete bipartite graphs, which prescribe
                       the set of row lengths and carry both eigenvector families;
scaled_coefficients()  coefficients scaled so that a long filter's output stays O(|x|);
balanced_coefficients() coefficients whose three closed-form factors are all of order 1;
fp64_filter()          an fp64 numpy restatement under a chosen summation order, for the drift
                       measurement that sets the device bounds of the long filters.
"""
import numpy as np

LD = np.longdouble
U53 = LD(2.0) ** -53

CHEBY, BINOMIAL = 0, 1          # CF_FILTER_CHEBY, CF_FILTER_BINOMIAL

SHORT = (3, 4, 5, 6, 7)         # every phase of the three-buffer rotation; 1, 2 and 3 binomial rounds
LONG = (12, 33, 64)

# Device bounds of the long filters, max|y - y_ref| / max|y_ref| per filter length.  Set from the
# fp64-against-longdouble drift that test_filters.py::test_drift_sets_the_device_bounds measures on
# the CPU (the oracle and the fp64 restatement under four further summation orders, on the three
# unions, both kinds, random and eigenvector signals; eigenvector signals relative to max|x|): at
# most 6.3e-14 at 12, 3.1e-13 at 33 and 6.3e-13 at 64 coefficients, the largest from sequential
# sums over the 5000-entry hub row of the G = 4 union.  MARGIN is the one test_gpu_svd.py
# documents: room for the kernel's own tree (lane-strided partials, a butterfly, two accumulators,
# contracted FMAs).
MARGIN = 200.0
BOUND_LONG = {12: 2e-11, 33: 2e-10, 64: 2e-10}
# The same for the four random-topology cases of test_gpu_filters_match_oracle, relative to
# max|y| (never max(1, .)): drift at most 3.1e-14 (Chebyshev, 64 coefficients).
BOUND_RANDOM = 1e-11
# Closed forms: the input is the fp64 rounding of sqrt(deg), an eigenvector to 2^-53 only.  The
# longdouble reference differs from the closed form by at most 4.6e-16 max|x| at up to 64
# coefficients (test_reference_matches_closed_forms holds it to this floor); the device is
# granted the floor on top of its bound.
CLOSED_FORM_FLOOR = 5e-15


# ---- graph ----------------------------------------------------------------------------------------
class Csr:
    """Directed edges by source.  pos = position of an edge inside its row, in line order (first
    all va -> vb in line order, interleaved with vb -> va as the kernel's fill does)."""

    def __init__(self, n, va, vb, w):
        va = np.asarray(va, np.int64)
        vb = np.asarray(vb, np.int64)
        w = np.asarray(w, np.float64)
        keep = (w > 0.1) & (va != vb)            # NaN > 0.1 is False
        a, b, wk = va[keep], vb[keep], w[keep]
        assert len(a) == 0 or (min(a.min(), b.min()) >= 0 and max(a.max(), b.max()) < n)
        # the two directions of a line are consecutive, as in the kernel's host fill
        src = np.stack([a, b], 1).reshape(-1)
        dst = np.stack([b, a], 1).reshape(-1)
        ww = np.stack([wk, wk], 1).reshape(-1)
        order = np.argsort(src, kind="stable")
        self.n = int(n)
        self.src, self.dst, self.w = src[order], dst[order], ww[order]
        self.len = np.bincount(self.src, minlength=n).astype(np.int64)
        self.ptr = np.concatenate([[0], np.cumsum(self.len)])
        self.nnz = int(self.ptr[-1])
        self.pos = np.arange(self.nnz) - self.ptr[self.src]
        self._rows = np.nonzero(self.len)[0]

    def rowsum(self, vals):
        """Per-row sums of a per-edge array (longdouble or float64, numpy's reduceat order)."""
        out = np.zeros(self.n, vals.dtype)
        if self.nnz:
            out[self._rows] = np.add.reduceat(vals, self.ptr[self._rows])
        return out


def _gamma(k):
    k = np.asarray(k, LD)
    return k * U53 / (1 - k * U53)


# ---- running-error arithmetic -----------------------------------------------------------------------
# A quantity is a pair (v, e): v the exact-arithmetic value (here: its longdouble evaluation) and e a
# bound on |computed fp64 value - v|.  One fp64 operation on computed operands a^, b^ returns
# (a^ op b^)(1 + d), |d| <= u = 2^-53, so its error is at most the propagated operand error p plus
# u (|v| + p).  A fused multiply-add skips the product's rounding (d = 0 there), which every bound
# below covers because each only assumes |d| <= u.
def _add(a, b, sign=1):
    v = a[0] + sign * b[0]
    p = a[1] + b[1]
    return v, p + U53 * (np.abs(v) + p)


def _mulc(c, a, c_err=0):
    """fp64 constant c (with absolute error c_err, for a rounded sum of two coefficients)."""
    c = LD(c)
    v = c * a[0]
    p = np.abs(c) * a[1] + c_err * (np.abs(a[0]) + a[1])
    return v, p + U53 * (np.abs(v) + p)


def reference(kind, n, va, vb, w, x, c, with_bound=True):
    """(y, bound): the filtered signal in longdouble and, per vertex, a bound on |y_fp64 - y| for an
    fp64 evaluation of the same supersteps in any summation order, with or without FMA.

    Derivation (u = 2^-53, gamma_k = k u / (1 - k u), len_i = directed edges of row i):
    - degrees d_i are sums of len_i positive weights: relative error <= (len_i - 1) u in any order;
    - a normalised weight wn_e = w_e / sqrt(d_j d_i) then carries the two degree errors, the
      product's rounding, the square root (which halves what is under it and adds its own rounding)
      and the division: ((len_i - 1 + len_j - 1 + 1) / 2 + 2) u plus second-order terms,
      bounded by theta_e = ((len_i + len_j) / 2 + 3) u;
    - a gather s_i = sum_e wn_e v_j over len_i terms, on computed weights and a computed vector v^
      with |v^ - v| <= E, satisfies
          |s^_i - s_i| <= sum_e wn_e E_j + sum_e wn_e ((1 + theta_e)(1 + gamma_{len_i + 1}) - 1)(|v_j| + E_j):
      the first term is the input error propagated through |S|, the second the weight errors and the
      dot product's gamma_{len + 1} sum |wn^| |v^| (one more than len: the products' roundings);
    - every vertex update is a handful of additions and multiplications by fp64 constants, each
      adding u (|value| + propagated error) (see _add / _mulc); the rounded sum c_i + c_{i+1} of the
      binomial step is a constant with relative error u.
    The bound is evaluated in longdouble, whose own error (the same expressions with 2^-64 for
    2^-53) is 2^-11 of it; the returned bound is inflated by 2^-10 to cover the reference's.  It grows
    like (2 ||S||)^n_coeff and is useful for short filters only.
    """
    g = Csr(n, va, vb, w)
    wl = g.w.astype(LD)
    deg = g.rowsum(wl)
    wn = wl / np.sqrt(deg[g.dst] * deg[g.src]) if g.nnz else wl
    theta = ((g.len[g.src] + g.len[g.dst]).astype(LD) / 2 + 3) * U53
    gam = _gamma(g.len[g.src] + 1)
    werr = wn * ((1 + theta) * (1 + gam) - 1)
    zero = np.zeros(n, LD)

    def gather(a):
        s = g.rowsum(wn * a[0][g.dst])
        if not with_bound:
            return s, zero
        return s, g.rowsum(wn * a[1][g.dst]) + g.rowsum(werr * (np.abs(a[0]) + a[1])[g.dst])

    xv = (np.asarray(x, np.float64).astype(LD), zero)
    c = np.asarray(c, np.float64)
    nc = len(c)
    assert nc >= 3
    if kind == CHEBY:
        s = gather(xv)
        # t_cur = (val - s - 1.0 val) / 1.0: two subtractions; the value is -s
        t_cur = (-s[0], _add(_add(xv, s, -1), xv, -1)[1])
        t_old = xv
        y = _add(_mulc(0.5 * c[0], xv), _mulc(c[1], t_cur))
        for k in range(2, nc):
            s = gather(t_cur)
            inner = _add(_add(t_cur, s, -1), t_cur, -1)          # value -s; doubling is exact
            t_new = _add((-2 * s[0], 2 * inner[1]), t_old, -1)
            y = _add(y, _mulc(c[k], t_new))
            t_old, t_cur = t_cur, t_new
    else:
        y = xv
        i = 0
        while 3 * i < nc:
            s = gather(y)
            c01 = LD(c[i]) + LD(c[i + 1])
            part_a = _add(_mulc(c01, y, c_err=U53 * abs(c01)), _mulc(c[i + 1], s), -1)
            tmp = _add(y, s, -1)
            s2 = gather(tmp)
            y = _add(part_a, _mulc(c[i + 2], _add(tmp, s2, -1)))
            i += 1
    return y[0], y[1] * (1 + LD(2.0) ** -10)


def closed_form(kind, x, c, mu, isolated):
    """The exact filtered signal of an eigenvector input, in longdouble.

    On any graph x = sqrt(deg), scaled freely per connected component, has S x = x (mu = +1): the
    Chebyshev argument L - I = -S acts as -1, T_k(-1) = (-1)^k, and L acts as 0.  On a bipartite
    graph x = +-sqrt(deg) by side has S x = -x (mu = -1): T_k(1) = 1 and L acts as 2.  On isolated
    vertices (any x) S acts as 0: T_k(0) = cos(k pi / 2) and L acts as 1.
      Chebyshev: (c0 / 2 + sum_k c_k T_k(-mu)) x;  binomial: prod_i (c_i + c_{i+1} l + c_{i+2} l^2) x
      over rounds 3 i < n_coeff, l = 1 - mu."""
    c = np.asarray(c, np.float64).astype(LD)
    nc = len(c)

    def factor(m):          # m = eigenvalue of S
        if kind == CHEBY:
            tk = {1: lambda k: (-1) ** k, -1: lambda k: 1, 0: lambda k: (0 if k % 2 else (-1) ** (k // 2))}[m]
            return c[0] / 2 + sum((c[k] * tk(k) for k in range(1, nc)), LD(0))
        lam = LD(1 - m)
        f, i = LD(1), 0
        while 3 * i < nc:
            f = f * (c[i] + c[i + 1] * lam + c[i + 2] * lam * lam)
            i += 1
        return f

    xl = np.asarray(x, np.float64).astype(LD)
    return np.where(isolated, factor(0), factor(int(mu))) * xl


# ---- inputs -----------------------------------------------------------------------------------------
class Union:
    pass


def bipartite_union(parts, seed, isolated=3, duplicates=0, self_lines=0, sub_threshold=0, repeat=1):
    """A disjoint union of complete bipartite graphs K_{a,b} (parts = [(a, b), ...]) plus `isolated`
    vertices without a kept line: every vertex of a K_{a,b} has a row of exactly b or a entries, so
    the parts prescribe the set of row lengths.  Weights are '{:.2f}' values in (0.1, 1] (what
    mega_graph.py writes); vertex ids are randomly permuted, the line order shuffled and each line's
    direction flipped at random.  Optional extras: `repeat` writes every line that many times and
    `duplicates` repeats that many lines of the LAST part once more (parallel edges, kept: they
    lengthen rows, so prescribed lengths belong in the other parts); `self_lines` (va == vb) and
    `sub_threshold` lines (w <= 0.1, between arbitrary vertices) must be dropped.
    Returns a Union with n, va, vb, w, side (+1 / -1, 0 for isolated), comp (part index, -1 for
    isolated), isolated (mask), part_vertices (ids per part) and part_lines (line indices per part,
    in file order)."""
    rng = np.random.default_rng(seed)
    n = sum(a + b for a, b in parts) + isolated
    ids = rng.permutation(n)
    side = np.zeros(n, np.int64)
    comp = np.full(n, -1, np.int64)
    la, lb, lp = [], [], []
    base = 0
    part_vertices = []
    for p, (a, b) in enumerate(parts):
        A, B = ids[base:base + a], ids[base + a:base + a + b]
        side[A], side[B] = 1, -1
        comp[A] = comp[B] = p
        part_vertices.append(np.concatenate([A, B]))
        aa, bb = np.repeat(A, b), np.tile(B, a)
        for _ in range(repeat):
            la.append(aa), lb.append(bb), lp.append(np.full(a * b, p))
        base += a + b
    empty = [np.zeros(0, np.int64)]
    la, lb, lp = np.concatenate(empty + la), np.concatenate(empty + lb), np.concatenate(empty + lp)
    if duplicates:
        last = np.nonzero(lp == len(parts) - 1)[0]
        pick = rng.choice(last, size=duplicates)
        la, lb, lp = np.concatenate([la, la[pick]]), np.concatenate([lb, lb[pick]]), np.concatenate([lp, lp[pick]])
    w = rng.integers(11, 101, size=len(la)) / 100.0
    if self_lines:
        v = rng.integers(0, n, size=self_lines)
        la, lb, lp = np.concatenate([la, v]), np.concatenate([lb, v]), np.concatenate([lp, np.full(self_lines, -1)])
        w = np.concatenate([w, rng.integers(11, 101, size=self_lines) / 100.0])
    if sub_threshold:
        la = np.concatenate([la, rng.integers(0, n, size=sub_threshold)])
        lb = np.concatenate([lb, rng.integers(0, n, size=sub_threshold)])
        lp = np.concatenate([lp, np.full(sub_threshold, -1)])
        w = np.concatenate([w, rng.integers(0, 11, size=sub_threshold) / 100.0])     # 0.00 .. 0.10
    w = np.array([float("{:.2f}".format(v)) for v in w])
    order = rng.permutation(len(la))
    la, lb, lp, w = la[order], lb[order], lp[order], w[order]
    flip = rng.random(len(la)) < 0.5
    u = Union()
    u.parts, u.n = list(parts), n
    u.va, u.vb, u.w = np.where(flip, lb, la), np.where(flip, la, lb), w
    u.side, u.comp, u.isolated = side, comp, comp < 0
    u.part_vertices = part_vertices
    u.part_lines = [np.nonzero(lp == p)[0] for p in range(len(parts))]
    u.kept = int(np.sum((u.w > 0.1) & (u.va != u.vb)))
    return u


def sub_union(u, p):
    """Part p of a union on its own: its vertices renumbered 0.. in ascending id order, its lines in
    the same relative order and direction.  Returns (n, va, vb, w, vertex ids in the union)."""
    vid = np.sort(u.part_vertices[p])
    new = np.full(u.n, -1, np.int64)
    new[vid] = np.arange(len(vid))
    ln = u.part_lines[p]
    return len(vid), new[u.va[ln]], new[u.vb[ln]], u.w[ln], vid


def random_signal(u, seed):
    return np.random.default_rng(seed).uniform(-10, 10, u.n)


def eigen_signal(u, mu, seed):
    """fp64 rounding of scale[comp] * (side if mu = -1) * sqrt(weighted degree); isolated vertices,
    which any value satisfies, get random ones."""
    rng = np.random.default_rng(seed)
    g = Csr(u.n, u.va, u.vb, u.w)
    deg = g.rowsum(g.w.astype(LD))
    scale = rng.uniform(0.5, 4.0, len(u.parts) + 1) * rng.choice([-1.0, 1.0], len(u.parts) + 1)
    x = scale[u.comp].astype(LD) * np.sqrt(deg)
    if mu == -1:
        x = x * u.side
    x = x.astype(np.float64)
    x[u.isolated] = rng.uniform(-10, 10, int(u.isolated.sum()))
    return x


def scaled_coefficients(kind, n_coeff, seed):
    """Random coefficients scaled in closed form so that a long filter neither dies out nor blows up.
    The unions' S has the eigenvalues +1 and -1 on every component (the two eigenvector families),
    0 on isolated vertices, and little else far from 0 (a complete bipartite graph with equal
    weights has exactly these three); a random signal has components along all of them.  With f(m)
    the closed-form factor at the eigenvalue m of S, a binomial filter's f scales as s^rounds and a
    Chebyshev filter's as s, so s = max_m |f(m)|^(-1 / rounds) resp. 1 / max_m |f(m)| makes the
    largest of the three gains exactly 1.  Callers assert max|y| / max|x| in [0.1, 10] on the
    reference."""
    rng = np.random.default_rng(seed)
    c = rng.normal(size=n_coeff)
    one = np.ones(1)
    gain = max(abs(float(closed_form(kind, one, c, m, np.array([m == 0]))[0])) for m in (1, -1, 0))
    rounds = -(-n_coeff // 3) if kind == BINOMIAL else 1
    return c * gain ** (-1.0 / rounds)


def gains(kind, c):
    """The closed-form factors (f(+1), f(-1), f(0)) at the eigenvalues +1, -1 and 0 of S."""
    one = np.ones(1)
    return tuple(float(closed_form(kind, one, c, m, np.array([m == 0]))[0]) for m in (1, -1, 0))


_PERIOD3 = []


def _period3():
    """(p0, p1, p2) with p0 + p1 + p2 = 1, p0 p1 p2 = -1 and
    (p0 + 2 p1 + 4 p2)(p1 + 2 p2 + 4 p0)(p2 + 2 p0 + 4 p1) = 1: binomial coefficients repeating with
    period 3 meet the windows (p0, p1, p2), (p1, p2, p0), (p2, p0, p1) in turn, so three rounds
    multiply the eigenvector of L = 0 by p0 p1 p2, that of L = 1 by (p0 + p1 + p2)^3 and that of
    L = 2 by the third product -- all of magnitude 1.  With p2 = t the first two conditions make
    p0, p1 the roots of z^2 - (1 - t) z - 1 / t = 0 (a closed form); the third fixes t by
    bisection: (0.2271, 2.5203, -1.7473)."""
    if not _PERIOD3:
        def family(t):
            s, p = 1 - t, -1 / t
            p0 = (s - np.sqrt(s * s - 4 * p)) / 2
            return p0, s - p0, t

        def third(t):
            p0, p1, p2 = family(t)
            return (p0 + 2 * p1 + 4 * p2) * (p1 + 2 * p2 + 4 * p0) * (p2 + 2 * p0 + 4 * p1) - 1

        lo, hi = -1.80, -1.70
        assert third(lo) * third(hi) < 0
        for _ in range(100):
            mid = (lo + hi) / 2
            lo, hi = (mid, hi) if third(lo) * third(mid) > 0 else (lo, mid)
        _PERIOD3.extend(family(lo))
    return tuple(_PERIOD3)


def balanced_coefficients(kind, n_coeff, seed):
    """Coefficients for the eigenvector signals: all three closed-form factors f(+1), f(-1), f(0)
    are of order 1 (callers assert [0.1, 10] on the closed form), so none of the three families is
    compared at the level of noise, and the 2^-53 the fp64-rounded sqrt(deg) holds of other
    eigenvectors is not amplified.
    Chebyshev: f is linear in c, f(m) = c0 / 2 + sum_k c_k T_k(-m); c_3.. are N(0, 1) / sqrt(n) and
    c0, c1, c2 solve the 3 x 3 system that sets the three factors to random targets of magnitude
    in [0.5, 2].  Binomial: the period-3 pattern of _period3, whose factors return to magnitude 1
    every three rounds (partial products between: 0.227, 0.572 at L = 0 and -1.72, 0.114 at L = 2),
    times 1 + 1e-3 N(0, 1) per coefficient, then scaled by s with s^rounds the inverse geometric
    mean of the three factors' magnitudes, which centres them on 1 (within [0.28, 2.5])."""
    rng = np.random.default_rng(seed)
    if kind == BINOMIAL:
        p = np.array(_period3())
        c = p[np.arange(n_coeff) % 3] * (1 + 1e-3 * rng.normal(size=n_coeff))
        rounds = -(-n_coeff // 3)
        return c * float(np.prod(np.abs(gains(kind, c)))) ** (-1.0 / (3 * rounds))
    c = rng.normal(size=n_coeff) / np.sqrt(n_coeff)
    target = rng.uniform(0.5, 2.0, 3) * rng.choice([-1.0, 1.0], 3)
    c[:3] = 0
    rest = np.array(gains(kind, c))
    ga, gb, gc = target - rest          # c0/2 - c1 + c2, c0/2 + c1 + c2, c0/2 - c2
    c[1] = (gb - ga) / 2
    c[0] = (ga + gb + 2 * gc) / 2
    c[2] = (ga + gb - 2 * gc) / 4
    return c


# ---- the cases ----------------------------------------------------------------------------------------
def lane_lengths(G):
    """Row lengths around the kernel's branches for a G-lane group: empty, one, the group width and
    its neighbours, the 4-deep unrolled gather's entry p + 3 G < e at its edge (3 G, 3 G + 1: no lane
    / lane 0 only), a full unrolled trip and its neighbours, and two trips plus a tail."""
    return sorted({0, 1, G - 1, G, G + 1, 3 * G, 3 * G + 1, 4 * G - 1, 4 * G, 4 * G + 1, 8 * G + 3})


UNION_PARTS = {
    4: [(1, 1), (1, 3), (1, 4), (1, 5), (2, 12), (2, 13), (1, 15), (1, 16), (1, 17), (3, 35), (1, 5000)],
    16: [(1, 1), (15, 16), (17, 48), (49, 63), (64, 65), (3, 131)],
    64: [(1, 1), (63, 64), (65, 192), (193, 255), (256, 257), (2, 515)],
}
_UNIONS = {}


def union(G):
    """The union of lane width G (built once, shared, never modified).  The G = 4 one carries the
    star K_{1,5000} (a hub row 1250 trips long under the narrowest group), self-lines and
    sub-threshold lines; all have three isolated vertices."""
    if G not in _UNIONS:
        _UNIONS[G] = bipartite_union(UNION_PARTS[G], seed=100 + G, isolated=3,
                                     self_lines=5 if G == 4 else 0, sub_threshold=7 if G == 4 else 0)
    return _UNIONS[G]


# Small graphs at the block edge: n G one group below, at and one above a multiple of the 256-thread
# block, n = 1, and fewer vertices than one group.  (name, intended G, builder arguments)
EDGE_GRAPHS = [
    ("g4_n63", 4, dict(parts=[(1, 3)] * 15, isolated=3)),
    ("g4_n64", 4, dict(parts=[(1, 3)] * 16, isolated=0)),
    ("g4_n65", 4, dict(parts=[(1, 3)] * 16, isolated=1)),
    ("g16_n31", 16, dict(parts=[(15, 16)], isolated=0)),
    ("g16_n32", 16, dict(parts=[(16, 16)], isolated=0)),
    ("g16_n33", 16, dict(parts=[(16, 16)], isolated=1)),
    ("g64_n127", 64, dict(parts=[(63, 64)], isolated=0)),
    ("g64_n128", 64, dict(parts=[(64, 64)], isolated=0)),
    ("g64_n129", 64, dict(parts=[(64, 65)], isolated=0)),
    ("n1", 4, dict(parts=[], isolated=1)),
    ("g4_n2", 4, dict(parts=[(1, 1)], isolated=0)),
    ("g16_n7", 16, dict(parts=[(3, 4)], isolated=0, repeat=10, duplicates=5)),     # parallel edges
    ("g64_n7", 64, dict(parts=[(3, 4)], isolated=0, repeat=20)),
]


def edge_graph(name):
    if name not in _UNIONS:
        _, _, kw = next(e for e in EDGE_GRAPHS if e[0] == name)
        _UNIONS[name] = bipartite_union(seed=len(name) + 7 * len(kw["parts"]), **kw)
    return _UNIONS[name]


_REFS = {}


def cached_reference(key, kind, u, x, c, with_bound):
    """reference() computed once per key and shared among the tests (not modified by them)."""
    if key not in _REFS:
        _REFS[key] = reference(kind, u.n, u.va, u.vb, u.w, x, c, with_bound=with_bound)
    return _REFS[key]


def short_case(G_or_name, kind, n_coeff):
    """(union, random signal, coefficients ~ N(0, 1), (y_ref, bound))."""
    u = union(G_or_name) if isinstance(G_or_name, int) else edge_graph(G_or_name)
    x = random_signal(u, seed=n_coeff)
    c = np.random.default_rng(1000 + n_coeff).normal(size=n_coeff)
    return u, x, c, cached_reference(("short", G_or_name, kind, n_coeff), kind, u, x, c, True)


def long_case(G, kind, n_coeff, signal="random"):
    """(union, signal, coefficients, y_ref); signal is 'random' (scaled_coefficients) or +1 / -1
    (an eigenvector, balanced_coefficients)."""
    u = union(G)
    if signal == "random":
        x, c = random_signal(u, seed=n_coeff), scaled_coefficients(kind, n_coeff, seed=2000 + n_coeff)
    else:
        x, c = eigen_signal(u, signal, seed=n_coeff), balanced_coefficients(kind, n_coeff, seed=3000 + n_coeff)
    return u, x, c, cached_reference(("long", G, kind, n_coeff, signal), kind, u, x, c, False)[0]


# ---- fp64 restatement under a summation order ----------------------------------------------------------
def fp64_filter(kind, n, va, vb, w, x, c, order):
    """The supersteps in fp64 numpy.  order = ('perm', seed): every row summed sequentially with its
    edges permuted; ('lanes', G): lane-strided partials (edge p of a row goes to lane p mod G,
    each lane sequential) summed by numpy's reduction over the lanes."""
    g = Csr(n, va, vb, w)
    if order[0] == "perm":
        perm = np.random.default_rng(order[1]).permutation(g.nnz)
        src, dst, ww = g.src[perm], g.dst[perm], g.w[perm]

        def rowsum(vals):
            return np.bincount(src, weights=vals, minlength=n)
    else:
        G = order[1]
        src, dst, ww = g.src, g.dst, g.w
        key = g.src * G + g.pos % G

        def rowsum(vals):
            return np.bincount(key, weights=vals, minlength=n * G).reshape(n, G).sum(1)
    deg = rowsum(ww)
    wn = ww / np.sqrt(deg[dst] * deg[src]) if g.nnz else ww

    def gather(v):
        return rowsum(wn * v[dst])

    x = np.asarray(x, np.float64)
    c = np.asarray(c, np.float64)
    if kind == CHEBY:
        t_old = x
        t_cur = x - gather(x) - x
        y = 0.5 * c[0] * t_old + c[1] * t_cur
        for k in range(2, len(c)):
            t_new = 2.0 * (t_cur - gather(t_cur) - t_cur) - t_old
            y = y + c[k] * t_new
            t_old, t_cur = t_cur, t_new
        return y
    y, i = x, 0
    while 3 * i < len(c):
        s = gather(y)
        part_a = (c[i] + c[i + 1]) * y - c[i + 1] * s
        tmp = y - s
        y = part_a + c[i + 2] * (tmp - gather(tmp))
        i += 1
    return y
