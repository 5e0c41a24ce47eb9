"""How far the NMF checker (tests/nmf_ref.py) drifts from itself on the test cases when the edge
order is permuted and the initial factors are perturbed by 1e-15 relative: the rounding-level
noise the bounds of tests/test_gpu_nmf.py are a few hundred times above.  CPU only.

    python tools/nmf_drift.py

Prints, per case and mode, max|dF| / max|F| over U and V and the largest change of a loss-trace
entry relative to loss_scale (the sum of the absolute values of the loss terms: near a perfect fit
the loss is a small difference of large terms, so |loss| is the wrong yardstick); then numpy's
column sum against itself with the rows permuted and perturbed, relative to sum |F|."""
from __future__ import annotations

import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))

import nmf_ref as nr  # noqa: E402


def perturbed(c: nr.Case, rng) -> nr.Case:
    perm = rng.permutation(len(c.user))
    jit = lambda F: F * (1.0 + 1e-15 * rng.uniform(-1, 1, F.shape))   # noqa: E731
    return nr.Case(c.n_users, c.n_items, c.D, c.user[perm], c.item[perm], c.obs[perm], jit(c.U0), jit(c.V0), c.n_sweeps)


def main():
    rng = np.random.default_rng(0)
    worst_f = worst_l = 0.0
    for name in nr.CASES:
        c = nr.case_inputs(name)
        for mode in nr.MODES:
            a = nr.fit_case(c, mode)
            df = dl = 0.0
            for _ in range(3):
                b = nr.fit_case(perturbed(c, rng), mode)
                df = max(df, np.max(np.abs(a.U - b.U)) / np.max(np.abs(a.U)), np.max(np.abs(a.V - b.V)) / np.max(np.abs(a.V)))
                dl = max(dl, float(np.max(np.abs(a.loss_trace - b.loss_trace)) / a.loss_scale))
                assert a.n_floored == b.n_floored
            print(f"case {name} {mode}: factor drift {df:.2e}  loss drift {dl:.2e}  floored {a.n_floored}  "
                  f"loss scale {a.loss_scale:.4g}  trace {a.loss_trace}")
            worst_f, worst_l = max(worst_f, df), max(worst_l, dl)
    print(f"worst factor drift {worst_f:.2e}, worst loss drift {worst_l:.2e}")
    worst_s = 0.0
    for n in (1, 1023, 1024, 1025, 2051, 40 * 1024 + 1):
        for D in (1, 5, 33, 64):
            F = rng.uniform(0, 1, (n, D))   # non-negative, as the factors are
            F2 = (F * (1.0 + 1e-15 * rng.uniform(-1, 1, F.shape)))[rng.permutation(n)]
            worst_s = max(worst_s, float(np.max(np.abs(F.sum(0) - F2.sum(0)) / np.abs(F).sum(0))))
    print(f"worst column-sum drift relative to sum |F|: {worst_s:.2e}")


if __name__ == "__main__":
    main()
