"""Constructed inputs for the data prep (csrc/cf_prep.hip), built on the CPU only.

Every builder returns (n_users, n_movies, user, movie, rating, validate) in read order, compact
ids.  Each case is named for the branch of a kernel it is built to reach; COVERAGE[name] asserts
on the CPU, from the case and the restatement's output alone, that the branch is reached
(tests/test_prep_cases.py runs it without a GPU, tests/test_gpu_prep_edges.py before the device
call).  reference(name) is the restatement oracle.cf_prep_oracle.knn_regroup of the case, computed
once per process and shared; nobody may change what it returns.
"""
import functools

import numpy as np

from oracle import cf_prep_oracle as prep

# kernel constants the cases depend on (csrc/cf_prep.hip)
WAVE = 64               # lanes of corated_bits_kernel's b0 trip: `b0 += 64`
PREP_THREADS = 256      # kPrepThreads: words per w0 trip of row_write_kernel
WORD = 32               # columns per bitmap word
CHUNK_COLS = PREP_THREADS * WORD   # 8192: the first column of row_write_kernel's second trip
GRID_CAP = 65536        # the grid caps of corated_bits_kernel (users) and row_write_kernel (movies)


def _pack(n_users, n_movies, triples, rng=None, validate=None):
    """triples: list of (user, movie[, role]); ratings 1..5 by position, read order shuffled by rng."""
    t = [(x[0], x[1], x[2] if len(x) > 2 else 0) for x in triples]
    if rng is not None:
        t = [t[i] for i in rng.permutation(len(t))]
    user = np.array([x[0] for x in t], np.uint32)
    movie = np.array([x[1] for x in t], np.uint32)
    role = np.array([x[2] for x in t], np.uint8)
    rating = (1 + np.arange(len(t)) % 5).astype(np.float32)
    return n_users, n_movies, user, movie, rating, (role if validate is None else validate)


def user_sets(case):
    """{user: sorted unique movies} over both roles: the lists corated_bits_kernel walks."""
    sets = {}
    for u, m in zip(case[2].tolist(), case[3].tolist()):
        sets.setdefault(u, set()).add(m)
    return {u: sorted(s) for u, s in sets.items()}


def pairs_of(sets, users):
    """Ordered co-rated pairs (a, b), a != b, produced by the listed users."""
    out = set()
    for u in users:
        s = sets[u]
        out.update((a, b) for a in s for b in s if a != b)
    return out


# ---- wave_trips ----------------------------------------------------------------------------------
WAVE_TRIPS_LENGTHS = (0, 1, 2, 4, 5, 64, 65, 131)
WAVE_TRIPS_LONG_USER = 7


def wave_trips():
    """n_movies = 200 (7 words); users with set lengths 0, 1, 2, 4, 5, 64, 65 and 131.  The 131-set
    is movie 31, then every movie of words 1 and 2 (32..95), then 66 movies of 96..199: sorted,
    the two full 32-lane segments start at lanes 1 and 33, and the second runs to position 64,
    lane 0 of the second 64-lane trip of corated_bits_kernel's b0 loop (two atomics for one word)."""
    rng = np.random.default_rng(101)
    n_movies = 200
    tr = []
    for u, d in enumerate(WAVE_TRIPS_LENGTHS):
        if d == 131:
            ms = [31] + list(range(32, 96)) + sorted(rng.choice(np.arange(96, 200), size=66, replace=False).tolist())
        else:
            ms = rng.choice(n_movies, size=d, replace=False).tolist()
        tr += [(u, m, int(rng.random() < 0.3)) for m in ms]
    tr += [tr[i] for i in rng.integers(0, len(tr), size=40)]   # re-read pairs: sets stay sets
    return _pack(len(WAVE_TRIPS_LENGTHS), n_movies, tr, rng)


def full_segments(s):
    """(word, first sorted position) of every 32-column word the sorted set s holds whole."""
    out = []
    for w in sorted({m // WORD for m in s}):
        pos = [i for i, m in enumerate(s) if m // WORD == w]
        if len(pos) == WORD:
            out.append((w, pos[0]))
    return out


def cover_wave_trips(case, ref):
    sets = user_sets(case)
    lengths = sorted(len(sets.get(u, [])) for u in range(case[0]))
    assert lengths == sorted(WAVE_TRIPS_LENGTHS), lengths
    s = sets[WAVE_TRIPS_LONG_USER]
    assert len(s) == 131 > 2 * WAVE and {31, 32, 63, 64} <= set(s)
    assert s[0] == 31 and s[1:65] == list(range(32, 96))
    segs = full_segments(s)
    assert [p % WAVE for _, p in segs] == [1, 33]                          # odd starting lanes
    assert any(p // WAVE != (p + WORD - 1) // WAVE for _, p in segs)        # one straddles the trip
    assert s[WAVE - 1] // WORD == s[WAVE] // WORD                           # positions 63 and 64: one word
    assert any(len(v) > WAVE for v in sets.values()) and any(len(v) == WAVE for v in sets.values())


# ---- row_chunks ----------------------------------------------------------------------------------
ROW_CHUNKS_HIGH_PAIR = (8200, 8210)
ROW_CHUNKS_LOW_PAIR = (100, 5000)


def row_chunks():
    """n_movies = 8192 + 33 (258 words, the last with one valid bit): row_write_kernel's w0 loop
    takes a second trip and carries `base += s_run`.  A hub user rates about 600 movies over the
    whole range (0, 8191, 8192 and 8224 among them): its rows have entries on both sides of word
    256.  Movies 8200 and 8210 are co-rated only with each other (rows empty in the first chunk),
    movies 100 and 5000 likewise (rows empty in the second chunk)."""
    rng = np.random.default_rng(102)
    n_movies = CHUNK_COLS + 33
    reserved = set(ROW_CHUNKS_HIGH_PAIR + ROW_CHUNKS_LOW_PAIR)
    low = [m for m in rng.choice(CHUNK_COLS, size=600, replace=False).tolist() if m not in reserved][:588]
    high = [m for m in range(CHUNK_COLS, n_movies) if m not in reserved]
    hub = sorted(set(low) | {0, CHUNK_COLS - 1, CHUNK_COLS, n_movies - 1} |
                 set(rng.choice(high, size=8, replace=False).tolist()))
    tr = [(0, m, int(rng.random() < 0.2)) for m in hub]
    tr += [(1, m) for m in ROW_CHUNKS_HIGH_PAIR] + [(2, m) for m in ROW_CHUNKS_LOW_PAIR]
    free = np.array([m for m in range(n_movies) if m not in reserved])
    for u in range(3, 23):
        tr += [(u, int(m), int(rng.random() < 0.2)) for m in rng.choice(free, size=10, replace=False)]
    return _pack(24, n_movies, tr, rng)


def cover_row_chunks(case, ref):
    n_movies = case[1]
    assert n_movies > CHUNK_COLS and (n_movies + WORD - 1) // WORD == PREP_THREADS + 2
    assert n_movies - 1 == (PREP_THREADS + 1) * WORD                        # the last word holds one bit
    corated = ref[2]
    hub = user_sets(case)[0]
    assert 550 <= len(hub) <= 620 and {0, CHUNK_COLS - 1, CHUNK_COLS, n_movies - 1} <= set(hub)
    both = [a for a, c in enumerate(corated) if c and c[0] < CHUNK_COLS <= c[-1]]
    only_high = [a for a, c in enumerate(corated) if c and c[0] >= CHUNK_COLS]
    only_low = [a for a, c in enumerate(corated) if c and c[-1] < CHUNK_COLS]
    assert len(both) >= 500 and set(hub) <= set(both)
    assert set(ROW_CHUNKS_HIGH_PAIR) <= set(only_high) and set(ROW_CHUNKS_LOW_PAIR) <= set(only_low)
    assert corated[8200] == [8210] and corated[100] == [5000]
    assert n_movies - 1 in corated[0] and corated[n_movies - 1][0] == 0


# ---- many_users ----------------------------------------------------------------------------------
def many_users():
    """n_users = 65536 + 50: corated_bits_kernel's loop over u (grid capped at 65536 blocks) takes
    a second trip.  Movies 40..49 are rated by users >= 65536 only; users 0, 4 and 49 are active
    and so are 65536, 65540 and 65585, the second trips of blocks that worked in their first."""
    rng = np.random.default_rng(103)
    n_users, n_movies = GRID_CAP + 50, 50
    tr = [(GRID_CAP, 40), (GRID_CAP, 41), (GRID_CAP + 4, 42), (GRID_CAP + 4, 43), (GRID_CAP + 4, 44),
          (n_users - 1, 45), (n_users - 1, 46), (n_users - 1, 3)]
    lows = [0, 4, 49] + rng.choice(np.arange(50, GRID_CAP), size=60, replace=False).tolist()
    for u in lows:
        tr += [(int(u), int(m), int(rng.random() < 0.3)) for m in rng.choice(40, size=5, replace=False)]
    return _pack(n_users, n_movies, tr, rng)


def cover_many_users(case, ref):
    n_users = case[0]
    assert n_users > GRID_CAP and 100 <= len(case[2]) <= 1000
    sets = user_sets(case)
    hi = [u for u in sets if u >= GRID_CAP]
    lo = [u for u in sets if u < GRID_CAP]
    only_hi = pairs_of(sets, hi) - pairs_of(sets, lo)
    assert len({(a, b) for a, b in only_hi if a < b}) >= 3
    assert max(sets) == n_users - 1
    twice = [u for u in lo if u + GRID_CAP in sets and len(sets[u]) >= 2 and len(sets[u + GRID_CAP]) >= 2]
    assert len(twice) >= 1, twice
    assert ref[2][40] == [41] and ref[2][45] == [3, 46]


# ---- many_movies ---------------------------------------------------------------------------------
def many_movies():
    """n_movies = 65536 + 40: row_write_kernel's loop over a (grid capped at 65536 blocks) takes a
    second trip, in blocks whose first row is non-empty too.  The co-rated bitmap is
    n_movies x ceil(n_movies / 32) words = 65576 x 2050 x 4 B, about 0.54 GB of scratch."""
    rng = np.random.default_rng(104)
    n_users, n_movies = 300, GRID_CAP + 40
    tr = [(0, GRID_CAP), (0, GRID_CAP + 1), (0, n_movies - 1),
          (1, GRID_CAP + 3), (1, GRID_CAP + 10), (1, 3), (1, 500),
          (2, GRID_CAP + 39), (2, 39), (2, 70000 - GRID_CAP)]
    for u in range(3, n_users):
        tr += [(u, int(m), int(rng.random() < 0.3)) for m in rng.choice(n_movies, size=10, replace=False)]
    return _pack(n_users, n_movies, tr, rng)


def cover_many_movies(case, ref):
    n_movies = case[1]
    assert n_movies > GRID_CAP and 2000 <= len(case[2]) <= 5000
    corated = ref[2]
    high_pairs = [(a, b) for a in range(GRID_CAP, n_movies) for b in corated[a] if b > a]
    assert len(high_pairs) >= 4, high_pairs
    twice = [a for a in range(n_movies - GRID_CAP) if corated[a] and corated[a + GRID_CAP]]
    assert 3 in twice and 39 in twice


# ---- roles ---------------------------------------------------------------------------------------
def roles_all_validate():
    """Every rating VALIDATE: ntr == 0 in regroup_split_kernel, the train lists are empty and
    test_off is complete."""
    rng = np.random.default_rng(105)
    n_users, n_movies, n = 30, 40, 300
    tr = [(int(u), int(m)) for u, m in zip(rng.integers(0, n_users, n), rng.integers(0, n_movies, n))]
    return _pack(n_users, n_movies, tr, validate=np.ones(n, np.uint8))


def cover_roles_all_validate(case, ref):
    train, test, corated = ref
    assert case[5].all() and not any(train)
    assert sum(len(t) for t in test) == len(set(zip(case[2].tolist(), case[3].tolist()))) > 200
    assert sum(len(c) for c in corated) > 500


ROLES_BOTH = (3, 5)      # (user, movie) read in both roles
ROLES_TEST_ONLY = 7      # a movie rated as VALIDATE only


def roles_mixed():
    """(user 3, movie 5) read as TRAIN and as VALIDATE: in both lists, once in the co-rated sets.
    Movie 7 is rated as VALIDATE only and still joins its raters' co-rated sets."""
    rng = np.random.default_rng(106)
    n_users, n_movies = 12, 20
    tr = [(3, 5, 0), (3, 5, 1), (3, 9, 0), (3, 7, 1), (4, 7, 1), (4, 11, 0)]
    others = [m for m in range(n_movies) if m != ROLES_TEST_ONLY]
    for u in range(n_users):
        tr += [(u, int(m), int(rng.random() < 0.4)) for m in rng.choice(others, size=4, replace=False)]
    return _pack(n_users, n_movies, tr, rng)


def cover_roles_mixed(case, ref):
    train, test, corated = ref
    u, m = ROLES_BOTH
    assert u in train[m] and u in test[m]
    assert all(corated[b].count(m) == 1 for b in user_sets(case)[u] if b != m)
    assert not train[ROLES_TEST_ONLY] and len(test[ROLES_TEST_ONLY]) == 2
    assert {5, 9, 11} <= set(corated[ROLES_TEST_ONLY]) and ROLES_TEST_ONLY in corated[11]


# ---- one_run -------------------------------------------------------------------------------------
ONE_RUN = 200_000


def one_run():
    """200,000 reads of one (role, movie, user) key with distinct ratings, a handful of other
    ratings among them: the kept rating is the last read, so the stable merge sort has to keep
    read order through every merge level."""
    n_users, n_movies = 4, 3
    n = ONE_RUN + 6
    user = np.full(n, 2, np.uint32)
    movie = np.full(n, 1, np.uint32)
    validate = np.zeros(n, np.uint8)
    rating = np.arange(n, dtype=np.float32)          # distinct: n < 2^24
    for i, (u, m, v) in zip((0, 7, 1000, 65537, 131072, n - 2),
                            ((0, 0, 0), (3, 2, 1), (2, 1, 1), (1, 1, 0), (2, 0, 0), (3, 1, 0))):
        user[i], movie[i], validate[i] = u, m, v
    return n_users, n_movies, user, movie, rating, validate


def cover_one_run(case, ref):
    _, _, user, movie, rating, validate = case
    key = (user == 2) & (movie == 1) & (validate == 0)
    assert int(key.sum()) == ONE_RUN and len(np.unique(rating[key])) == ONE_RUN
    last = int(np.nonzero(key)[0][-1])
    assert last == len(user) - 1 and not key[last - 1]       # the run ends after an interruption
    assert ref[0][1][2] == float(rating[last])
    assert ref[1][1] == {2: 1000.0} and sorted(ref[0][1]) == [1, 2, 3]


# ---- bit_edges, tiny -----------------------------------------------------------------------------
BIT_EDGES = (1, 31, 32, 33, 64)


def bit_edges(n_movies):
    """One user rating every one of n_movies in {1, 31, 32, 33, 64}: every row holds every other
    movie, the self bit is the only one cleared (first and last bit of a word, a word boundary)."""
    return _pack(1, n_movies, [(0, m) for m in range(n_movies)])


def cover_bit_edges(case, ref):
    n_movies = case[1]
    assert n_movies in BIT_EDGES
    assert ref[2] == [[b for b in range(n_movies) if b != a] for a in range(n_movies)]


def tiny():
    """n = 1, n_users = 1, n_movies = 1."""
    return _pack(1, 1, [(0, 0)])


def cover_tiny(case, ref):
    assert (case[0], case[1], len(case[2])) == (1, 1, 1)
    assert ref[0] == [{0: 1.0}] and ref[1] == [{}] and ref[2] == [[]]


BUILDERS = {
    "wave_trips": wave_trips,
    "row_chunks": row_chunks,
    "many_users": many_users,
    "many_movies": many_movies,
    "roles_all_validate": roles_all_validate,
    "roles_mixed": roles_mixed,
    "one_run": one_run,
    **{f"bit_edges_{n}": functools.partial(bit_edges, n) for n in BIT_EDGES},
    "tiny": tiny,
}
COVERAGE = {
    "wave_trips": cover_wave_trips,
    "row_chunks": cover_row_chunks,
    "many_users": cover_many_users,
    "many_movies": cover_many_movies,
    "roles_all_validate": cover_roles_all_validate,
    "roles_mixed": cover_roles_mixed,
    "one_run": cover_one_run,
    **{f"bit_edges_{n}": cover_bit_edges for n in BIT_EDGES},
    "tiny": cover_tiny,
}
NAMES = list(BUILDERS)


@functools.lru_cache(maxsize=None)
def case(name):
    return BUILDERS[name]()


@functools.lru_cache(maxsize=None)
def reference(name):
    """(train, test, corated) of oracle.cf_prep_oracle.knn_regroup for the case."""
    _, n_movies, user, movie, rating, validate = case(name)
    return prep.knn_regroup(n_movies, user, movie, rating, validate)


def reference_offsets(ref):
    """The three offset arrays (train, test, co-rated) the restatement implies, uint64[n_movies + 1]."""
    out = []
    for lists in ref:
        off = np.zeros(len(lists) + 1, np.uint64)
        off[1:] = np.cumsum([len(x) for x in lists])
        out.append(off)
    return out


def reference_corated_flat(ref):
    c = [b for row in ref[2] for b in row]
    return np.array(c, np.uint32)


def assert_regroup_equal(g, ref):
    """The device regroup `g` (Context.knn_regroup's dict) against the restatement: the three
    offset arrays whole, then per movie the train and test lists (users ascending, the last rating
    read) and the sorted co-rated list.  Rows empty in all three are settled by the offsets."""
    train, test, corated = ref
    offs = reference_offsets(ref)
    for kind, off in zip(("train_off", "test_off", "edg_off"), offs):
        assert np.array_equal(g[kind], off), kind
    nonempty = np.nonzero(np.diff(offs[0].astype(np.int64)) + np.diff(offs[1].astype(np.int64)) +
                          np.diff(offs[2].astype(np.int64)))[0]
    for m in nonempty.tolist():
        for kind, r in (("train", train[m]), ("test", test[m])):
            off = g[kind + "_off"]
            us = g[kind + "_user"][off[m]:off[m + 1]].tolist()
            rs = g[kind + "_rating"][off[m]:off[m + 1]].tolist()
            assert us == sorted(r) and rs == [r[u] for u in sorted(r)], (kind, m)
        eo = g["edg_off"]
        assert g["edg_movie"][eo[m]:eo[m + 1]].tolist() == corated[m], m
