"""Do two builds of the library compute the same bits in explicit and implicit-feedback ALS?

    python tools/als_same_results.py --old OLD/libcf_mi355x.so --new NEW/libcf_mi355x.so [--out FILE]

Each library runs in a process of its own (CF_MI355X_LIB) over the inputs of the GPU tests: every
case of tests/als_ref.py and the segmented vertex of tests/test_gpu_als.py at D = 8, 13, 33 (U, V,
residuals, update counts, supersteps), every case of tests/ials_ref.py and its two-slice Gram case
(U, V, loss trace).  Prints one line per output with the SHA-256 of its bytes under both libraries;
exit status 1 if any pair differs."""
from __future__ import annotations

import argparse
import hashlib
import json
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def child():
    sys.path.insert(0, ROOT)
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    import numpy as np

    import als_ref as ar
    import ials_ref as ir
    from collaborative_filtering_amd import _native
    from collaborative_filtering_amd.api import Context

    out = {}

    def put(name, **arrays):
        for k, v in arrays.items():
            out[f"{name}.{k}"] = hashlib.sha256(np.ascontiguousarray(v).tobytes()).hexdigest()

    def put_als(name, r):
        put(name, U=r.U, V=r.V, residual_user=r.residual_user, residual_item=r.residual_item,
            nupdates_user=r.nupdates_user, nupdates_item=r.nupdates_item,
            counts=np.array([r.supersteps, r.updates, r.n_not_pd], np.uint64))

    with Context(0) as ctx:
        for name, (_, _, _, regn, lam, tol, mu, _) in ar.CASES.items():
            g, U0, V0, *_ = ar.case_inputs(name)
            put_als(f"als {name}", ctx.als_fit(g.user, g.item, g.obs, g.n_users, g.n_items, U0, V0, regnormal=regn,
                                              lam=lam, tol=tol, max_updates=mu, out_degree=g.out_degree))
        seg = _native.load().cf_debug_als_segment()
        for D in (8, 13, 33):   # the inputs of test_gpu_als.test_segmented_vertex
            n_users = 2 * seg + 37
            rng = np.random.default_rng(5)
            user = rng.permutation(n_users).astype(np.uint32)
            item = np.zeros(n_users, np.uint32)
            obs = rng.integers(1, 6, n_users).astype(np.float32)
            U0, V0 = rng.uniform(-1, 1, (n_users, D)), rng.uniform(-1, 1, (1, D))
            put_als(f"als segmented D={D}", ctx.als_fit(user, item, obs, n_users, 1, U0, V0, lam=0.05,
                                                        regnormal="degree", max_supersteps=2))
        cases = {name: ir.case_inputs(name) for name in ir.CASES}
        cases["G"] = ir.gram_fit_case(_native.load().cf_debug_ials_gram_rows())
        for name, c in cases.items():
            r = ctx.ials_fit(c.user, c.item, c.conf, c.n_users, c.n_items, c.U0, c.V0, pref=c.pref, reg_user=c.reg_user,
                             reg_item=c.reg_item, n_sweeps=ir.N_SWEEPS)
            put(f"ials {name}", U=r.U, V=r.V, loss_trace=r.loss_trace, n_not_pd=np.array([r.n_not_pd], np.uint64))
    print("HASHES " + json.dumps(out))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--old")
    ap.add_argument("--new")
    ap.add_argument("--out")
    ap.add_argument("--child", action="store_true")
    a = ap.parse_args()
    if a.child:
        return child()
    res = []
    for lib in (a.old, a.new):
        env = dict(os.environ, CF_MI355X_LIB=os.path.abspath(lib))
        p = subprocess.run([sys.executable, os.path.abspath(__file__), "--child"], env=env, capture_output=True,
                           text=True, timeout=600)
        if p.returncode != 0:   # nothing more runs on the GPU after a failure
            sys.stderr.write(p.stdout + p.stderr)
            return p.returncode or 1
        res.append(json.loads(next(ln for ln in p.stdout.split("\n") if ln.startswith("HASHES "))[7:]))
    old, new = res
    lines = [f"{k:34s} {old[k][:16]} {new.get(k, '-')[:16]} {'same' if old[k] == new.get(k) else 'DIFFERENT'}"
             for k in old]
    n_diff = sum(ln.endswith("DIFFERENT") for ln in lines) + len(set(new) - set(old))
    lines.append(f"{len(lines)} outputs, {n_diff} different")
    text = "\n".join([f"{'output':34s} {'old sha256[:16]':16s} {'new sha256[:16]':16s}"] + lines) + "\n"
    sys.stdout.write(text)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as fh:
            fh.write(text)
    return 1 if n_diff else 0


if __name__ == "__main__":
    sys.exit(main())
