"""The constructed data-prep cases (tests/prep_cases.py) reach the branches they are named for.

No GPU: every case is built, restated by oracle.cf_prep_oracle.knn_regroup, and checked by its
coverage assertion, before any device output exists.  tests/test_gpu_prep_edges.py then compares
cf_knn_regroup with the same restatement on the same cases."""
import numpy as np
import pytest

import prep_cases as pc


@pytest.mark.parametrize("name", pc.NAMES)
def test_case_reaches_its_branch(name):
    case = pc.case(name)
    n_users, n_movies, user, movie, rating, validate = case
    assert len(user) == len(movie) == len(rating) == len(validate) >= 1
    assert int(user.max()) < n_users and int(movie.max()) < n_movies
    ref = pc.reference(name)
    assert len(ref[0]) == len(ref[1]) == len(ref[2]) == n_movies
    pc.COVERAGE[name](case, ref)


def test_kernel_constants_mirrored():
    """The cuts the cases of this file, of test_gpu_graph_compact.py and of test_gpu_pack.py are
    placed at, as the kernels have them: a changed constant must move the cases with it."""
    import os
    import re

    import test_gpu_graph_compact as gc
    import test_gpu_pack as gp

    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    csrc = os.path.join(root, "collaborative_filtering_amd", "csrc")
    const = lambda src, name: int(re.search(rf"constexpr int {name} = (\d+);", src).group(1))   # noqa: E731
    prep_src = open(os.path.join(csrc, "cf_prep.hip")).read()
    assert const(prep_src, "kPrepThreads") == pc.PREP_THREADS
    assert f"b0 += {pc.WAVE}" in prep_src
    assert prep_src.count(f"{pc.GRID_CAP})), dim3(kPrepThreads)") == 2     # both grid caps
    assert pc.CHUNK_COLS == 8192
    graph_src = open(os.path.join(csrc, "cf_graph.hip")).read()
    assert const(graph_src, "kGT") == gc.GT and f"std::min({gc.ROW_THREADS}u, std::thread" in graph_src
    pack_src = open(os.path.join(csrc, "cf_pack.hip")).read()
    assert const(pack_src, "kScanThreads") == gp.SCAN_THREADS
    assert f"std::min<uint32_t>(n_users, {gp.GRID_CAP}u)" in pack_src


def test_reference_offsets_helper():
    ref = pc.reference("roles_mixed")
    tr, te, co = pc.reference_offsets(ref)
    assert int(tr[-1]) == sum(len(x) for x in ref[0]) and int(te[-1]) == sum(len(x) for x in ref[1])
    assert np.array_equal(np.diff(co.astype(np.int64)), [len(x) for x in ref[2]])
    assert len(pc.reference_corated_flat(ref)) == int(co[-1])
