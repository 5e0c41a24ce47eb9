"""Data prep: the k-fold split and the knn regroup.

CPU: the restatement of fold_cross_validation.py (oracle/cf_prep_oracle.py) reproduces the
files the reference script itself wrote (tests/golden/fold_cases.npz), and the product's
CPython-compatible shuffle (cf_pyrand.hpp via libcf_host.so) equals random.shuffle.
GPU: bin/fold_cross_validation writes byte-identical files; cf_knn_regroup matches the
restatement of knn.cpp's map semantics, including duplicates, both roles, users and movies
without ratings and the co-rated capacity contract."""
import ctypes
import os
import random
import subprocess

import numpy as np
import pytest

from oracle import cf_prep_oracle as prep
from prep_cases import assert_regroup_equal

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLD = np.load(os.path.join(ROOT, "tests", "golden", "fold_cases.npz"))
CASES = sorted({k.split("__")[0] for k in GOLD.files})


def golden(name):
    files = {k.split("__")[1]: GOLD[k].tobytes().decode() for k in GOLD.files
             if k.startswith(name + "__") and k.split("__")[1] not in ("input", "meta")}
    num_div, seed = (int(x) for x in GOLD[name + "__meta"])
    return GOLD[name + "__input"].tobytes().decode(), num_div, seed, files


@pytest.mark.parametrize("name", CASES)
def test_fold_restatement_matches_reference_output(name):
    text, num_div, seed, files = golden(name)
    assert prep.fold_split(text, num_div, seed) == files


def test_host_shuffle_is_cpython():
    L = ctypes.CDLL(os.path.join(ROOT, "collaborative_filtering_amd", "libcf_host.so"))
    L.cfh_py_shuffle.argtypes = [ctypes.c_uint64, ctypes.c_uint32, ctypes.c_void_p]
    for seed in (0, 1, 11, 2026, 2 ** 32 + 5, 123456789012345):
        for n in (1, 2, 3, 64, 943, 100_000):
            p = np.zeros(n, np.uint32)
            L.cfh_py_shuffle(seed, n, p.ctypes.data)
            x = list(range(n))
            random.Random(seed).shuffle(x)
            assert p.tolist() == x, (seed, n)


def test_regroup_cpu_baseline_matches_restatement():
    """The bench's data-prep CPU baseline (oracle cfo_knn_regroup_mt: the reference's containers
    on host threads) keeps the same entries as the Python restatement of knn.cpp's maps,
    duplicates (last read wins) and both roles included, for 1 and 3 threads."""
    lib = ctypes.CDLL(os.path.join(ROOT, "oracle", "libcf_oracle.so"))
    lib.cfo_knn_regroup_mt.argtypes = [ctypes.c_int64] + [ctypes.c_void_p] * 4 + [ctypes.c_int] * 3 + [ctypes.c_void_p]
    n_users, n_movies = 300, 120
    user, movie, rating, val = regroup_case(5, n_users, n_movies, 6000)
    tr, te, co = prep.knn_regroup(n_movies, user, movie, rating, val)
    want = [sum(len(x) for x in tr), sum(len(x) for x in te), sum(len(x) for x in co)]
    P = lambda a: np.ascontiguousarray(a).ctypes.data_as(ctypes.c_void_p)
    u32, m32 = np.ascontiguousarray(user, np.uint32), np.ascontiguousarray(movie, np.uint32)
    r32, v8 = np.ascontiguousarray(rating, np.float32), np.ascontiguousarray(val, np.uint8)
    for threads in (1, 3):
        cnt = np.zeros(3, np.uint64)
        lib.cfo_knn_regroup_mt(len(user), P(u32), P(m32), P(r32), P(v8), n_movies, n_users, threads, P(cnt))
        assert cnt.tolist() == want, (threads, cnt.tolist(), want)


@pytest.mark.gpu
@pytest.mark.parametrize("name", CASES)
def test_fold_binary_byte_identical(tmp_path, name):
    """bin/fold_cross_validation (CPython shuffle on the host, grouping by cf_fold_order on the
    GPU) writes exactly the files the reference script wrote under random.seed(seed)."""
    pytest.importorskip("torch").cuda.is_available() or pytest.skip("no GPU visible")
    text, num_div, seed, files = golden(name)
    (tmp_path / "u.data").write_text(text)
    p = subprocess.run([os.path.join(ROOT, "bin", "fold_cross_validation"), "u.data", str(num_div), "--seed",
                        str(seed)], cwd=tmp_path, capture_output=True, text=True, timeout=120)
    assert p.returncode == 0, p.stdout + p.stderr
    got = {f: (tmp_path / "cross_validation" / f).read_text() for f in os.listdir(tmp_path / "cross_validation")}
    assert got == files


@pytest.mark.gpu
def test_fold_order_matches_stable_rank_sort(gpu_ctx):
    rng = np.random.default_rng(3)
    n_users = 5000
    user = rng.integers(0, n_users, size=300_000).astype(np.uint32)
    rank = rng.permutation(n_users).astype(np.uint32)
    order = gpu_ctx.fold_order(user, rank)
    assert np.array_equal(order, np.argsort(rank[user], kind="stable"))


def regroup_case(seed, n_users, n_movies, n, dup_frac=0.1, val_frac=0.3):
    rng = np.random.default_rng(seed)
    p = 1.0 / np.arange(1, n_movies + 1)
    user = rng.integers(0, n_users, size=n)
    movie = rng.choice(n_movies, size=n, p=p / p.sum())
    dup = rng.random(n) < dup_frac            # repeat earlier (user, movie) pairs: last read wins
    src = rng.integers(0, np.maximum(np.arange(n), 1))
    user[dup] = user[src[dup]]
    movie[dup] = movie[src[dup]]
    rating = rng.integers(1, 6, size=n).astype(np.float32)
    validate = (rng.random(n) < val_frac).astype(np.uint8)
    return user.astype(np.uint32), movie.astype(np.uint32), rating, validate


@pytest.mark.gpu
@pytest.mark.parametrize("seed,n_users,n_movies,n", [(1, 300, 80, 4000), (2, 2000, 700, 60_000),
                                                     (3, 50, 2100, 3000), (4, 7, 5, 40)])
def test_knn_regroup_matches_restatement(gpu_ctx, seed, n_users, n_movies, n):
    user, movie, rating, validate = regroup_case(seed, n_users, n_movies, n)
    g = gpu_ctx.knn_regroup(n_users, n_movies, user, movie, rating, validate)
    assert_regroup_equal(g, prep.knn_regroup(n_movies, user, movie, rating, validate))


@pytest.mark.gpu
def test_knn_regroup_edge_cases(gpu_ctx):
    """No ratings; all-train input (validate NULL); a co-rated capacity that is too small:
    CF_ERANGE with complete offsets, then the exact capacity succeeds."""
    g = gpu_ctx.knn_regroup(3, 4, [], [], [])
    assert g["train_off"].tolist() == [0] * 5 and g["edg_off"].tolist() == [0] * 5
    user, movie, rating, _ = regroup_case(9, 40, 30, 900)
    g = gpu_ctx.knn_regroup(40, 30, user, movie, rating, None)
    train, test, corated = prep.knn_regroup(30, user, movie, rating, None)
    assert int(g["test_off"][-1]) == 0
    assert sum(len(t) for t in train) == int(g["train_off"][-1])
    need = sum(len(c) for c in corated)
    from collaborative_filtering_amd._native import NativeError
    with pytest.raises(NativeError):
        gpu_ctx.knn_regroup(40, 30, user, movie, rating, None, edg_cap=need - 1)
    g = gpu_ctx.knn_regroup(40, 30, user, movie, rating, None, edg_cap=need)
    assert [g["edg_movie"][g["edg_off"][m]:g["edg_off"][m + 1]].tolist() for m in range(30)] == corated
