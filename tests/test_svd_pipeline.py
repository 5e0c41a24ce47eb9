"""bin/svd, the drop-in for svd.cpp: its loader and writers on the CPU (through libcf_host.so),
and the binary itself on a written directory against Context.svd_fit on the same inputs."""
import ctypes
import os
import subprocess
from ctypes import c_char_p, c_int, c_int64, c_uint32, c_uint64, c_void_p

import numpy as np
import pytest

import pipeline_util as pu
import svd_ref as sr
from collaborative_filtering_amd._native import HOST_LIB_PATH, ptr

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BIN = os.path.join(ROOT, "bin", "svd")
HEADER = "%%GraphLab SVD Solver library. This file contains the singular values."


def host():
    L = ctypes.CDLL(HOST_LIB_PATH)
    L.cfh_svd_load.argtypes = [c_char_p, c_char_p, c_uint32, c_uint32, c_void_p, c_void_p, c_void_p, c_int64, c_char_p, c_int]
    L.cfh_svd_load.restype = c_int64
    L.cfh_svd_load_vector.argtypes = [c_char_p, c_uint32, c_void_p]
    L.cfh_svd_write_values.argtypes = [c_char_p, c_void_p, c_uint64]
    L.cfh_svd_write_vector.argtypes = [c_char_p, c_int, c_int, c_uint32, c_void_p, c_uint32]
    return L


def load(L, d, vecfile, rows, cols):
    err = ctypes.create_string_buffer(256)
    n = L.cfh_svd_load(d.encode(), vecfile.encode(), rows, cols, None, None, None, 0, err, 256)
    if n < 0:
        return None, err.value.decode()
    row, col, val = np.zeros(n, np.uint32), np.zeros(n, np.uint32), np.zeros(n, np.float32)
    assert L.cfh_svd_load(d.encode(), vecfile.encode(), rows, cols, ptr(row), ptr(col), ptr(val), n, err, 256) == n
    return (row, col, val), ""


def write_case(wd, name="A"):
    """The case's matrix as two files of "row col value" lines with 1-based ids, its start vector
    inside the same directory, and two files the loader has to skip."""
    row, col, val, rows, cols, v0, spec = sr.case_inputs(name)
    d = os.path.join(wd, "matrix")
    os.makedirs(d)
    os.makedirs(os.path.join(wd, "out"))
    lines = [f"{r + 1} {c + 1} {v:g}\n" for r, c, v in zip(row.tolist(), col.tolist(), val.tolist())]
    open(os.path.join(d, "part0"), "w").writelines(lines[::2])
    open(os.path.join(d, "part1"), "w").writelines(ln.replace(" ", "\t") for ln in lines[1::2])
    open(os.path.join(d, "start.vec"), "w").writelines(f"{x!r}\n" for x in v0.tolist())
    open(os.path.join(d, "old_singular_values"), "w").write(HEADER + "\n 1.5\n")
    open(os.path.join(d, "other_v0"), "w").write("0.25\n")
    return (row, col, val, rows, cols, v0, spec), d


def test_loader_and_writers_round_trip(tmp_path, monkeypatch):
    L = host()
    wd = str(tmp_path)
    monkeypatch.chdir(wd)
    (row, col, val, rows, cols, v0, _), _ = write_case(wd)
    got, msg = load(L, "matrix/", "matrix/start.vec", rows, cols)
    assert got is not None, msg
    # 1-based ids, every file but the skipped three, values through float
    want = sorted(zip(row.tolist(), col.tolist(), val.tolist()))
    assert sorted(zip(got[0].tolist(), got[1].tolist(), got[2].tolist())) == want
    bad, msg = load(L, "matrix/", "", rows, cols)   # the start vector read as a matrix file
    assert bad is None and "cannot parse" in msg
    bad, msg = load(L, "matrix/", "matrix/start.vec", int(row.max()), cols)   # row > rows is fatal
    assert bad is None and "row id" in msg
    back = np.zeros(rows)
    assert L.cfh_svd_load_vector(b"matrix/start.vec", rows, ptr(back)) == 0 and np.array_equal(back, v0)
    assert L.cfh_svd_load_vector(b"matrix/start.vec", rows + 1, ptr(np.zeros(rows + 1))) != 0   # too short
    sig = np.array([44.658940521234567, 19.0939924, 0.0, 1e-12])
    assert L.cfh_svd_write_values(b"out/p.singular_values", ptr(sig), len(sig)) == 0
    text = open("out/p.singular_values").read().split("\n")
    assert text[0] == HEADER and text[0].startswith("%%")   # the reference's double %
    assert text[1:5] == ["%10.13g" % s for s in sig] and text[5:] == [""]
    vec = np.array([0.1, -2.5e-7, 1.0 / 3.0, 4.0, 5.0])
    assert L.cfh_svd_write_vector(b"out/p.U.0", 2, 1, 1, ptr(vec), len(vec)) == 0
    assert L.cfh_svd_write_vector(b"out/p.V.0", 2, 1, 96, ptr(vec), len(vec)) == 0
    assert L.cfh_svd_write_vector(b"out/p.plain", 2, 0, 0, ptr(vec), len(vec)) == 0
    for prefix, first in (("out/p.U.0", 1), ("out/p.V.0", 96)):
        got = {int(a): float(b) for a, b in (ln.split() for ln in pu.read_shards(wd, prefix))}
        assert got == {first + i: x for i, x in enumerate(vec.tolist())}   # 17 digits: exact
    assert sorted(float(ln) for ln in pu.read_shards(wd, "out/p.plain")) == sorted(vec.tolist())


@pytest.mark.gpu
def test_binary_matches_the_library(tmp_path, gpu_ctx):
    wd = str(tmp_path)
    (row, col, val, rows, cols, v0, spec), _ = write_case(wd)
    nsv, nv = spec["nsv"], spec["nv"]
    p = subprocess.run([BIN, "--matrix", "matrix/", "--rows", str(rows), "--cols", str(cols), "--nsv", str(nsv), "--nv",
                        str(nv), "--max_iter", str(spec["max_iter"]), "--tol", str(spec["tol"]), "--initial_vector",
                        "matrix/start.vec", "--save_vectors", "1", "--id", "1", "--predictions", "out/p.", "--quiet", "1",
                        "--engine", "synchronous", "--no_edge_data", "1", "--nshards", "2"],
                       cwd=wd, capture_output=True, text=True, timeout=120)
    assert p.returncode == 0, p.stdout + p.stderr
    order = np.concatenate([np.arange(0, len(row), 2), np.arange(1, len(row), 2)])   # the loader's: part0, then part1
    row, col, val = row[order], col[order], val[order]
    r = gpu_ctx.svd_fit(row, col, val, rows, cols, nsv, nv, max_iter=spec["max_iter"], tol=spec["tol"], v0=v0)
    assert f" Number of computed signular values {r.nconv}\n" in p.stdout
    printed = [ln for ln in p.stdout.split("\n") if ln.startswith("Singular value ")]
    assert printed == ["Singular value %d \t%13.6g\tError estimate: %13.6g" % (i, r.sigma[i], r.err[i]) for i in range(nsv)]
    text = open(os.path.join(wd, "out", "p.singular_values")).read().split("\n")
    assert text[0] == HEADER and len(text) == 1 + nsv + nv + 1 + spec["max_iter"] + 1
    assert text[1:1 + nv] == ["%10.13g" % s for s in r.sigma]
    assert all(float(x) == 0.0 for x in text[1 + nv:-1])   # the slots of sigma no pass writes
    U, V = np.zeros((rows, nsv)), np.zeros((cols, nsv))
    for i in range(nsv):
        for M, side, first, n in ((U, "U", 1, rows), (V, "V", rows, cols)):
            got = {int(a): float(b) for a, b in (ln.split() for ln in pu.read_shards(wd, f"out/p.{side}.{i}_"))}
            assert sorted(got) == list(range(first, first + n))   # rows 1-based, columns by raw vertex id
            M[:, i] = [got[first + j] for j in range(n)]
    assert np.array_equal(U, r.U) and np.array_equal(V, r.V)   # 17 digits, the same inputs: the same bits
    A = sr.Matrix(row, col, val, rows, cols)
    resid, err = sr.residuals(A, U, V, r.sigma[:nsv], spec["tol"])
    want = sr.dense_sigma("A")[:nsv]
    assert np.all(err < spec["tol"])
    assert np.all(np.abs(r.sigma[:nsv] - want) <= sr.truth_bound(resid, want[0]))


@pytest.mark.gpu
def test_binary_refuses_what_the_reference_refuses(tmp_path):
    wd = str(tmp_path)
    (_, _, _, rows, cols, _, _), _ = write_case(wd)
    base = [BIN, "matrix/", "--rows", str(rows), "--cols", str(cols), "--initial_vector", "matrix/start.vec"]
    for extra, msg in ((["--nsv", "5", "--nv", "4"], "Please set the number of vectors"),
                       (["--nsv", "2", "--nv", "4", "--unittest", "1"], "--unittest"),
                       (["--nsv", "2", "--nv", "4", "--max_iter", "1", "--save_vectors", "1"], "No converged vectors")):
        p = subprocess.run(base + extra, cwd=wd, capture_output=True, text=True, timeout=120)
        assert p.returncode != 0 and msg in p.stderr, p.stdout + p.stderr
    p = subprocess.run([BIN, "matrix/", "--nsv", "2", "--nv", "4"], cwd=wd, capture_output=True, text=True, timeout=120)
    assert p.returncode != 0 and "Please specify number of rows/cols" in p.stderr
