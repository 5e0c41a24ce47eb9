"""The out_eigen_ pack (csrc/cf_pack.hip, cf_pack_eigen_run) on synthetic device blocks.

cf_pack_eigen_run takes device pointers and reads m as an input, so no eigensolve is needed:
k in [1, 9] and m in [-1, k] are drawn per user, the slots lie at evec_offsets plus a gap of
0..3 floats per user (every source alignment), and evecs = arange, so every float is unique and
a misplaced copy shows.  Expected: packed_off = exclusive cumsum of k * max(m, 0) with the total
last, packed = the first k * max(m, 0) floats of every slot, concatenated.  Bit-exact copies and
integers: no tolerance."""
import numpy as np
import pytest

from collaborative_filtering_amd.api import evec_offsets

SCAN_THREADS = 1024     # kScanThreads of cf_pack.hip: above it a thread of pack_offsets_kernel owns > 1 user
GRID_CAP = 65536        # block cap of pack_copy_kernel's launch in cf_pack_eigen_run
GUARD = 64              # floats behind the packed run that must stay NaN
SIZES = [1, 2, SCAN_THREADS - 1, SCAN_THREADS, SCAN_THREADS + 1, 2500, GRID_CAP + 50]


def pack_case(n_users):
    """(item_off, m, evec_off, evecs, want_off, want_packed) on the host."""
    rng = np.random.default_rng(n_users)
    k = rng.integers(1, 10, size=n_users)
    m = rng.integers(-1, k + 1)
    idx = np.arange(n_users)
    if n_users <= 2:
        m[:] = [k[0], 0][:n_users]
    else:
        m[idx % 11 == 3] = 0
        m[idx % 11 == 5] = -1
        m[idx % 11 == 7] = k[idx % 11 == 7]
    item_off = np.concatenate([[0], np.cumsum(k)]).astype(np.uint64)
    base, _ = evec_offsets(item_off)
    gap = rng.integers(0, 4, size=n_users)
    evec_off = (base.astype(np.int64) + np.cumsum(gap)).astype(np.uint64)
    n_evec = int(evec_off[-1]) + int(k[-1] * max(k[-1], 2))
    assert n_evec < 2 ** 24                                  # arange stays exact (and unique) in float32
    evecs = np.arange(n_evec, dtype=np.float32)
    n = k * np.maximum(m, 0)
    want_off = np.concatenate([[0], np.cumsum(n)]).astype(np.uint64)
    start = np.repeat(evec_off.astype(np.int64) - want_off[:-1].astype(np.int64), n)
    want_packed = evecs[start + np.arange(int(want_off[-1]))]
    return item_off, m.astype(np.int32), evec_off, evecs, want_off, want_packed


def alignment_classes(item_off, m, evec_off, want_off):
    """What pack_copy_kernel's branches see for 16-byte aligned buffers: per user the source and
    destination misalignment in floats, the head length, the tail length and the block length."""
    n = np.diff(item_off.astype(np.int64)) * np.maximum(m, 0)
    mis_s, mis_d = evec_off.astype(np.int64) & 3, want_off[:-1].astype(np.int64) & 3
    head = np.minimum(n, (4 - mis_s) & 3)
    tail = (n - head) % 4
    return n, mis_s, mis_d, head, tail


def test_case_2500_reaches_every_copy_branch():
    """No GPU needed: the 2500-user case holds all 16 (source, destination) alignment pairs,
    equal-alignment users with head lengths 0..3 followed by a float4 body, unequal-alignment users (the scalar
    fallback), tails 0..3, a block shorter than its head (n = 1 or 2 at misalignment 1, where
    `head = min(n, ...)` binds and nv = 0), and an empty block between two non-empty ones."""
    item_off, m, evec_off, _, want_off, _ = pack_case(2500)
    n, mis_s, mis_d, head, tail = alignment_classes(item_off, m, evec_off, want_off)
    live = n > 0
    assert {(int(a), int(b)) for a, b in zip(mis_s[live], mis_d[live])} == {(a, b) for a in range(4) for b in range(4)}
    eq = live & (mis_s == mis_d)
    assert set(head[eq & (n >= head + 4)].tolist()) == {0, 1, 2, 3}
    assert set(tail[eq & (n >= head + 4)].tolist()) == {0, 1, 2, 3}
    assert int((live & (mis_s != mis_d)).sum()) > 500
    short = eq & (mis_s == 1) & (n < 3)
    assert {1, 2} <= set(n[short].tolist())
    assert np.any((n[1:-1] == 0) & (n[:-2] > 0) & (n[2:] > 0))
    assert (m == 0).any() and (m < 0).any() and (m == np.diff(item_off.astype(np.int64))).any()


@pytest.mark.gpu
@pytest.mark.parametrize("n_users", SIZES)
def test_pack_offsets_and_copy(gpu_ctx, n_users):
    """Pins pack_offsets_kernel's `chunk` loop with the min(n_users, ...) clamps (1023, 1024: one
    user per thread, idle threads; 1025, 2500: chunks of 2 and 3 with the last threads clamped
    to empty ranges; 65586: chunks of 65), its max(m[u], 0), pack_copy_kernel's `u += gridDim.x`
    loop (65586 users on 65536 blocks) and its head / float4 / tail / unaligned copies.  The
    offsets-only call (d_packed null) comes first, then the full call into a NaN-filled buffer
    whose 64-float guard must stay NaN."""
    import torch

    item_off, m, evec_off, evecs, want_off, want_packed = pack_case(n_users)
    chunk = -(-n_users // SCAN_THREADS)
    assert (chunk > 1) == (n_users > SCAN_THREADS)
    assert n_users == SCAN_THREADS or chunk * SCAN_THREADS > n_users      # some thread's range is clamped
    total = int(want_off[-1])
    T = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to("cuda:0")          # noqa: E731
    d_off, d_m = T(item_off.view(np.int64)), T(m)
    d_eoff, d_ev = T(evec_off.view(np.int64)), T(evecs)
    d_poff = torch.full((n_users + 1,), -1, dtype=torch.int64, device="cuda:0")
    gpu_ctx.pack_eigen_run(n_users, d_off, d_m, None, None, d_poff)
    torch.cuda.synchronize()
    assert np.array_equal(d_poff.cpu().numpy().view(np.uint64), want_off)
    d_pk = torch.full((total + GUARD,), float("nan"), dtype=torch.float32, device="cuda:0")
    assert d_ev.data_ptr() % 16 == 0 and d_pk.data_ptr() % 16 == 0               # alignment_classes' premise
    d_poff.fill_(-1)
    gpu_ctx.pack_eigen_run(n_users, d_off, d_m, d_eoff, d_ev, d_poff, d_pk)
    torch.cuda.synchronize()
    assert np.array_equal(d_poff.cpu().numpy().view(np.uint64), want_off)
    pk = d_pk.cpu().numpy()
    assert np.array_equal(pk[:total].view(np.uint32), want_packed.view(np.uint32))
    assert np.all(np.isnan(pk[total:])) and len(pk) - total == GUARD
