"""The split kernel's assembly and per-sweep reloads (cf_eigen_split.hip) at the shapes where their
loops change path.

Stage 2b (W rows re-read from the slot), stage 3 (B = sym_lower(L2) + I through 64-column tiles) and
the sweep start load several elements ahead of their stores, unconditionally from offsets clamped
into the user's own k x k slot.  Checked at:
  - k = 129 / 130 (odd and even k, LDT = k | 1; at 129 the last column block of stage 3 is one
    column wide), k = 144 / 176 (row tiles of 71 / 87 rows: three row blocks, the last of two rows);
  - the bucket edges 145, 160, 161, 177 and 179, 180, two users each so that two share a CU;
  - a graph with w(a, b) != w(b, a) well above the predictor's 0.1 threshold (a lower / upper mix-up
    in sym_lower shows) and a sparse one whose users hold isolated items (the 0 -> 1 degree rule);
  - the device-pointer path with the eigenvector buffer pre-filled with NaN, users packed back to
    back: a clamped load that picked up a neighbour's or a stale element instead of zero propagates.
Against the full-LDS kernel (cf_set_eigen_split(0)): sigs bit-identical, m equal except at cut ties,
eigenvalues within 1e-5 (test_gpu_split's comparison); against the oracle: test_gpu_eigen's
tolerances.
"""
import numpy as np
import pytest

import cases
from collaborative_filtering_amd.api import EigenResult, evec_offsets
from test_gpu_eigen import _check_batch
from test_gpu_split import _compare_split_full, _run

pytestmark = pytest.mark.gpu

KS_SINGLE = [129, 130, 144, 176]
KS_PAIRS = [145, 145, 160, 160, 161, 161, 177, 177, 179, 179, 180, 180]
N_ITEMS = 320


def _asym_graph(seed):
    """cases.item_graph with the two directions of every edge far apart, both above 0.1."""
    W = cases.item_graph(N_ITEMS, 0.9, seed=seed).astype(np.float64)
    iu = np.triu_indices(N_ITEMS, 1)
    up = W[iu]
    W[iu] = np.where(up > 0.0, 0.15 + 0.6 * up, 0.0)
    lo = W.T[iu]
    W.T[iu] = np.where(lo > 0.0, np.maximum(lo, 0.12), 0.0)
    W = W.astype(np.float32)
    both = (W > 0.1) & (W.T > 0.1)
    assert np.count_nonzero(both & (np.abs(W - W.T) > 0.01)) > N_ITEMS * N_ITEMS // 2
    return W


@pytest.mark.parametrize("ks", [KS_SINGLE, KS_PAIRS], ids=["tile_edges", "bucket_edges"])
def test_assembly_asymmetric_graph(gpu_ctx, ks):
    W = _asym_graph(81)
    off, items = cases.user_items(N_ITEMS, ks, seed=82)
    gpu_ctx.set_eigen_split(True)
    _check_batch(gpu_ctx, W, off, items, "asm_asym")
    assert _compare_split_full(gpu_ctx, W, off, items) > 0


def test_assembly_isolated_items(gpu_ctx):
    W = cases.item_graph(N_ITEMS, 0.05, seed=83, isolated_frac=0.25)
    ks = KS_SINGLE + [145, 161, 180, 180]
    off, items = cases.user_items(N_ITEMS, ks, seed=84)
    deg = np.array([W[np.ix_(items[int(off[u]):int(off[u + 1])], items[int(off[u]):int(off[u + 1])])].sum(axis=1).min()
                    for u in range(len(ks))])
    assert np.all(deg == 0.0)   # every user holds an item with no edge inside its set
    gpu_ctx.set_eigen_split(True)
    _check_batch(gpu_ctx, W, off, items, "asm_isolated")
    _compare_split_full(gpu_ctx, W, off, items)


def test_assembly_device_path_nan_prefill(gpu_ctx):
    torch = pytest.importorskip("torch")
    W = _asym_graph(85)
    ks = [180, 129, 144, 180, 176, 161, 130, 179]   # k = 180 and an odd k at the ends of the buffer
    off, items = cases.user_items(N_ITEMS, ks, seed=86)
    gpu_ctx.set_eigen_split(True)
    host = _run(gpu_ctx, W, off, items, True)
    eoff, ne = evec_offsets(off)
    dev = torch.device("cuda")
    T = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)
    n = int(off[-1])
    d_m = torch.zeros(len(ks), dtype=torch.int32, device=dev)
    d_sigs = torch.full((n,), float("nan"), device=dev)
    d_evals = torch.full((n,), float("nan"), device=dev)
    d_evecs = torch.full((ne,), float("nan"), device=dev)   # exactly the users' slots, back to back
    plan = gpu_ctx.plan(off)
    try:
        plan.eigen_run(T(off.view(np.int64)), T(items.view(np.int32)), T(eoff.view(np.int64)), d_m, d_sigs, d_evals,
                       d_evecs)
        torch.cuda.synchronize()
    finally:
        plan.close()
    res = EigenResult(off, eoff, d_m.cpu().numpy(), d_sigs.cpu().numpy(), d_evals.cpu().numpy(), d_evecs.cpu().numpy())
    assert np.array_equal(res.m, host.m)
    assert np.all(np.isfinite(res.sigs))
    for u in range(len(ks)):
        for x, y in zip(res.block(u), host.block(u)):
            assert np.all(np.isfinite(x)), u
            assert np.array_equal(x, y), u
