"""How far the BPR checker (tests/bpr_ref.py) drifts from itself on the test cases under three
changes that stand for what another correct implementation may do differently: the triples of
every vertex summed in another order, the initial factors perturbed by 1e-15 relative, and every
g = 1 / (1 + exp(x)) moved by up to 2 ulp (another exp).  The bounds of tests/test_gpu_bpr.py are
a few hundred times these figures.  CPU only.

    python tools/bpr_drift.py

Prints, per case, max|dF| / max|F| for U, V and the bias and the largest change of a loss-trace
entry relative to the entry (the loss is a sum of positive terms, so the entry is the sum of their
absolute values); then the worst of each.  The negatives are integers and do not move."""
from __future__ import annotations

import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))

import bpr_ref as br  # noqa: E402


def main():
    rng = np.random.default_rng(0)
    jit = lambda F: None if F is None else F * (1.0 + 1e-15 * rng.uniform(-1, 1, F.shape))   # noqa: E731
    worst_f = worst_b = worst_l = 0.0
    for name in br.CASES:
        c, a = br.case_inputs(name), br.case_reference(name)
        df = db = dl = 0.0
        for _ in range(3):
            b = br.fit(c, U0=jit(c.U0), V0=jit(c.V0), bias0=jit(c.bias0), jitter=rng)
            assert (a.triples, a.n_skipped, a.n_nan) == (b.triples, b.n_skipped, b.n_nan)
            df = max(df, np.max(np.abs(a.U - b.U)) / np.max(np.abs(a.U)), np.max(np.abs(a.V - b.V)) / np.max(np.abs(a.V)))
            if a.bias is not None:
                db = max(db, np.max(np.abs(a.bias - b.bias)) / np.max(np.abs(a.bias)))
            dl = max(dl, float(np.max(np.abs(a.loss_trace[:, 0] - b.loss_trace[:, 0]) / a.loss_trace[:, 0])))
        print(f"case {name}: factor drift {df:.2e}  bias drift {db:.2e}  loss drift {dl:.2e}  triples {a.triples}  "
              f"skipped {a.n_skipped}")
        worst_f, worst_b, worst_l = max(worst_f, df), max(worst_b, db), max(worst_l, dl)
    print(f"worst factor drift {worst_f:.2e}, worst bias drift {worst_b:.2e}, worst loss drift {worst_l:.2e}")


if __name__ == "__main__":
    main()
