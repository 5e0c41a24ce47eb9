"""How far the iALS checker (tests/ials_ref.py) drifts from itself on the test cases when the edge
order is permuted and the initial factors are perturbed by 1e-15 relative: the rounding-level
noise the bounds of tests/test_gpu_ials.py are a few hundred times above.  CPU only.

    python tools/ials_drift.py

Prints, per case, max|dF| / max|F| over U and V, the largest relative change of a loss-trace
entry and the sampled conditioning; then the same for numpy's F^T F against itself with the rows
permuted and perturbed, relative to |F|^T |F| elementwise."""
from __future__ import annotations

import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))

import ials_ref as ir  # noqa: E402


def perturbed(c: ir.Case, rng) -> ir.Case:
    perm = rng.permutation(len(c.user))
    jit = lambda F: F * (1.0 + 1e-15 * rng.uniform(-1, 1, F.shape))   # noqa: E731
    return ir.Case(c.n_users, c.n_items, c.D, c.user[perm], c.item[perm], c.conf[perm],
                   None if c.pref is None else c.pref[perm], c.reg_user, c.reg_item, jit(c.U0), jit(c.V0))


def main():
    rng = np.random.default_rng(0)
    cases = {name: ir.case_inputs(name) for name in ir.CASES}
    cases["G"] = ir.gram_fit_case(512)
    worst_f = worst_l = 0.0
    for name, c in cases.items():
        a = ir.fit_case(c)
        df = dl = 0.0
        for _ in range(3):
            b = ir.fit_case(perturbed(c, rng))
            df = max(df, max(np.max(np.abs(a.U - b.U)) / np.max(np.abs(a.U)), np.max(np.abs(a.V - b.V)) / np.max(np.abs(a.V))))
            dl = max(dl, float(np.max(np.abs(a.loss_trace - b.loss_trace) / np.abs(a.loss_trace))))
        print(f"case {name}: factor drift {df:.2e}  loss drift {dl:.2e}  min eig ratio {a.min_eig_ratio:.2e}  "
              f"trace {a.loss_trace}")
        worst_f, worst_l = max(worst_f, df), max(worst_l, dl)
    print(f"worst factor drift {worst_f:.2e}, worst loss drift {worst_l:.2e}")
    worst_g = 0.0
    for n in (1, 511, 512, 513, 1027, 40 * 512 + 1):
        for D in (1, 5, 20, 33, 64):
            F = rng.uniform(-1, 1, (n, D))
            F2 = (F * (1.0 + 1e-15 * rng.uniform(-1, 1, F.shape)))[rng.permutation(n)]
            worst_g = max(worst_g, float(np.max(np.abs(F.T @ F - F2.T @ F2) / (np.abs(F).T @ np.abs(F)))))
    print(f"worst Gram drift relative to |F|^T |F|: {worst_g:.2e}")


if __name__ == "__main__":
    main()
