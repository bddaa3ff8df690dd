"""Shared inputs of tests/test_merge_cases_cpu.py and tests/test_topk_merge_gpu.py (not a
test module): candidate lists for di_topk_merge, its definition in numpy, and a restatement
of which kernel and which branch of it a given (n_lists, k, counts, keys) takes, so that the
CPU test can prove that the GPU cases between them reach every route of the merge."""
import functools

import numpy as np

# csrc/topk_merge.hip: the constants launch_merge and the merge kernels branch on
MS_LISTS = 64          # merge_sel_kernel: at most this many lists
MS_THREADS = 512       # ... with 8 or 16 candidates per thread
MG_SEL_MIN = 1024      # counting selection only above this many candidates
MG_SEL_KEYS = 2048     # ... and while the keys of the selected bins fit here
MG_SEL_CAP = 8192      # LDS key array past MG_LDS_KEYS candidates; histogram paths up to it
MG_LDS_KEYS = 16384    # every candidate fits in LDS
MG_SCAN_LISTS = 1024   # merge_topk_kernel: offset scan (fast_lists) up to this many lists
MG_SEL_BINS = 4096

U64 = np.uint64
KINDS = ("compact", "wide", "f32", "mixed", "one_score")
COUNT_MODES = ("full", "ragged", "empty", "short", "rejected")


def reference_merge(keys, counts, k, lists_major=False):
    """The definition of di_topk_merge.  keys [n_q, n_lists, k] and counts [n_q, n_lists]
    (lists_major: [n_lists, n_q, k] and [n_lists, n_q]).  Per query: any negative count ->
    n = -1; otherwise the union of each list's first min(count, k) keys, sorted descending
    as uint64, the first k kept.  Returns (out [n_q, k] uint64, zero past n; n [n_q] int32)."""
    keys = np.asarray(keys, U64)
    counts = np.asarray(counts, np.int32)
    if lists_major:
        keys, counts = keys.transpose(1, 0, 2), counts.T
    n_q, n_lists, kk = keys.shape
    assert kk == k and counts.shape == (n_q, n_lists)
    out = np.zeros((n_q, k), U64)
    n = np.zeros(n_q, np.int32)
    for q in range(n_q):
        if (counts[q] < 0).any():
            n[q] = -1
            continue
        parts = [keys[q, l, :min(int(counts[q, l]), k)] for l in range(n_lists)]
        top = np.sort(np.concatenate(parts))[::-1][:k]
        out[q, :top.size] = top
        n[q] = top.size
    return out, n


def _counts(rng, n_q, n_lists, k, mode):
    c = np.full((n_q, n_lists), k, np.int32)
    if mode == "ragged":  # 0..k per list, some lists empty, one full
        c = rng.integers(0, k + 1, (n_q, n_lists)).astype(np.int32)
        c[rng.random((n_q, n_lists)) < 0.2] = 0
        c[:, n_lists - 1] = k
        c[0, 0] = 0
    elif mode == "empty":
        c[:] = 0
    elif mode == "short":  # total <= MG_SEL_CAP although n_lists * k is not
        assert n_lists * k > MG_SEL_CAP
        base = MG_SEL_CAP // n_lists
        c = rng.integers(0, base + 1, (n_q, n_lists)).astype(np.int32)
        c[0] = base  # query 0: exactly MG_SEL_CAP candidates when n_lists divides it
        c[0, :MG_SEL_CAP - base * n_lists] += 1
        c = np.minimum(c, k)
    elif mode == "rejected":  # one list of one query; the other queries stay valid
        assert n_q > 1
        c[1, n_lists // 2] = -1
    else:
        assert mode == "full", mode
    return c


def _scores(rng, n, kind):
    """The bits above the tie fields of n keys of one query (not yet unique)."""
    if kind == "f32":  # float32 scores, multiples of 1/8 on both sides of 2.0 (many ties)
        s = (rng.integers(1, 40, n) / 8.0).astype(np.float32)
        return s.view(np.uint32).astype(U64) << U64(32)
    # ~256 keys per score value (the two-pass filter keeps more than MG_SEL_MIN keys at
    # k = 1000); 0 and 4095 (the last histogram bin) always among them
    vals = rng.choice(np.arange(1, MG_SEL_BINS - 1), size=max(2, n // 256), replace=False)
    vals = np.concatenate([vals, [0, MG_SEL_BINS - 1]])
    if kind == "one_score":
        vals = vals[:1]
    hi = rng.choice(vals, n).astype(U64) << U64(48)
    nib = np.zeros(n, U64)
    if kind == "wide":  # bit 60 or bit 63 set: unsigned order across the sign bit
        nib = rng.choice(np.array([1, 7, 8, 9, 15], U64), n)
    elif kind == "mixed":
        nib = rng.choice(np.array([0, 0, 0, 1, 8, 15], U64), n)
    return hi | (nib << U64(60))


@functools.lru_cache(maxsize=None)
def make_lists(n_q, n_lists, k, kind, counts_mode, seed=0):
    """(keys [n_q, n_lists, k] uint64, counts [n_q, n_lists] int32), query-major.  The keys of
    a query are unique; each list is sorted descending.  Entries past a list's count hold
    poison (keys larger than every real one) that a correct merge never reads.  Cached and
    read-only: the tests share one copy."""
    assert kind in KINDS and counts_mode in COUNT_MODES
    rng = np.random.default_rng([seed, n_q, n_lists, k, KINDS.index(kind),
                                 COUNT_MODES.index(counts_mode)])
    counts = _counts(rng, n_q, n_lists, k, counts_mode)
    n = n_lists * k
    keys = np.zeros((n_q, n_lists, k), U64)
    for q in range(n_q):
        hi = _scores(rng, n, kind)
        j = rng.integers(0, 256, n).astype(U64)  # first-touch term
        if kind == "f32":  # score bits << 32 | (255 - j) << 24 | (0xFFFFFF - doc)
            doc = (1 + rng.choice((1 << 24) - 2, n, replace=False)).astype(U64)
            doc[:2] = (0, 0xFFFFFF)  # both ends of the 24-bit doc field
            lo = ((U64(255) - j) << U64(24)) | (U64(0xFFFFFF) - doc)
        else:  # score << 48 | (255 - j) << 32 | (0xFFFFFFFF - doc)
            doc = (1 + rng.choice((1 << 32) - 2, n, replace=False)).astype(U64)
            doc[0] = 0
            lo = ((U64(255) - j) << U64(32)) | (U64(0xFFFFFFFF) - doc)
        allk = rng.permutation(hi | lo).reshape(n_lists, k)
        assert np.unique(allk).size == n and allk.min() > 0
        keys[q] = np.sort(allk, axis=1)[:, ::-1]
        for l in range(n_lists):
            c = max(int(counts[q, l]), 0)
            keys[q, l, c:] = U64(0xFFFFFFFFFFFFFFFF) - np.arange(k - c, dtype=U64)
    keys.setflags(write=False)
    counts.setflags(write=False)
    return keys, counts


def candidates(keys, counts, q):
    """The candidate keys of query q of a query-major case (empty for a rejected query)."""
    k = keys.shape[2]
    if (counts[q] < 0).any():
        return np.zeros(0, U64)
    return np.concatenate([keys[q, l, :min(int(c), k)] for l, c in enumerate(counts[q])])


def _in_bins_at_or_above_take(bins, take, total):
    """Keys in the histogram bins at or above the bin of the take-th largest key (sh.above);
    without the keys: as if no two keys shared a bin."""
    if bins is None:
        return take
    b = np.sort(np.asarray(bins))[::-1]
    assert b.size == total
    return int((b >= b[take - 1]).sum())


def expected_path(n_lists, k, counts_of_query, any_key_ge_2_60, bins=None):
    """The kernel and the branches one query takes, "kernel/load/selection", restating
    csrc/topk_merge.hip: launch_merge (the dispatch on n_lists, k and the LDS capacity `cap`,
    "few short lists" to the three launches), merge_sel_kernel (`counting`, `n_sel <=
    MG_SEL_KEYS`, `take < total`) and merge_topk_kernel (`fast_lists`, `total <= cap`, the
    two-pass filter's `big` and `n_keep <= cap`, `if (over)`, and the selection's condition
    and `n_sel <= MG_SEL_KEYS`).  bins: (key >> 48) & 4095 of the query's candidates, for
    the two data-dependent branches; the environment's A/B switches are left at default."""
    counts = np.asarray(counts_of_query, np.int64)
    assert counts.shape == (n_lists,)
    big = bool(any_key_ge_2_60)
    if n_lists <= MS_LISTS and n_lists * k <= 16 * MS_THREADS and k <= MG_SEL_KEYS:
        kern = "sel<8>" if n_lists * k <= 8 * MS_THREADS else "sel<16>"
        cap = None
    else:
        want = n_lists * k
        if n_lists > MG_SCAN_LISTS or want > MG_LDS_KEYS:
            want = max(k, MG_SEL_CAP)
        cap = 64
        while cap < want:
            cap <<= 1
        kern = ("topk<256>" if cap <= 256 else "topk<512>") + f"/cap{cap}"
    if (counts < 0).any():
        return kern + "/rejected"
    total = int(np.minimum(counts, k).sum())
    take = min(total, k)
    if cap is None:  # merge_sel_kernel: candidates in registers
        if not big and total > MG_SEL_MIN and take < total:
            if _in_bins_at_or_above_take(bins, take, total) <= MG_SEL_KEYS:
                return kern + "/registers/counting"
            return kern + "/registers/counting_overflow>radix_sort"
        return kern + ("/registers/radix_sort" if take < total else "/registers/sort")
    fast = n_lists <= MG_SCAN_LISTS
    n = total  # keys in LDS after the load
    if fast and total <= cap:
        load = "flatten"
    elif fast and MG_SEL_MIN < cap <= MG_SEL_CAP:
        if big:
            load, n = "two_pass_big>radix", take
        elif _in_bins_at_or_above_take(bins, take, total) <= cap:
            load, n = "two_pass", _in_bins_at_or_above_take(bins, take, total)
        else:
            load, n = "two_pass_overflow>radix", take
    else:
        load, n = ("radix" if fast else "noscan_radix"), take
    sel = "sort"
    if fast and n > MG_SEL_MIN and cap <= MG_SEL_CAP and take < n and not big:
        # (after the two-pass filter the kept keys are the bins >= T: the same count again)
        n_sel = _in_bins_at_or_above_take(bins, take, total)
        sel = "counting" if n_sel <= MG_SEL_KEYS else "counting_overflow>sort"
    return f"{kern}/{load}/{sel}"


def query_paths(n_lists, k, keys, counts):
    """expected_path of every query of a query-major case, from its data."""
    out = []
    for q in range(keys.shape[0]):
        cand = candidates(keys, counts, q)
        big = bool((cand >> U64(60)).any())
        bins = ((cand >> U64(48)) & U64(MG_SEL_BINS - 1)).astype(np.int64)
        out.append(expected_path(n_lists, k, counts[q], big, bins))
    return out


# Every route of the merge (the union over CASES must be exactly this set).
ROUTES = {
    "sel<8>/registers/sort",
    "sel<8>/registers/radix_sort",
    "sel<8>/registers/counting",
    "sel<8>/registers/counting_overflow>radix_sort",
    "sel<16>/registers/counting",
    "sel<16>/registers/radix_sort",
    "sel<16>/registers/counting_overflow>radix_sort",
    "topk<256>/cap256/flatten/sort",
    "topk<512>/cap4096/flatten/sort",
    "topk<512>/cap8192/flatten/counting",
    "topk<512>/cap8192/flatten/sort",
    "topk<512>/cap8192/flatten/counting_overflow>sort",
    "topk<512>/cap16384/flatten/sort",
    "topk<512>/cap8192/two_pass/counting",
    "topk<512>/cap8192/two_pass/counting_overflow>sort",
    "topk<512>/cap8192/two_pass/sort",
    "topk<512>/cap8192/two_pass_big>radix/sort",
    "topk<512>/cap8192/two_pass_overflow>radix/sort",
    "topk<512>/cap8192/noscan_radix/sort",
}

# (n_lists, k, kind, counts_mode, route): the route, or routes, that at least one query of
# the case takes (every query with `full` counts); None: an edge of the arguments, no route
# of its own.
CASES = [
    (1, 1, "compact", "full", "sel<8>/registers/sort"),
    (1, 1, "wide", "empty", None),
    (3, 64, "compact", "full", "sel<8>/registers/radix_sort"),
    (3, 64, "wide", "ragged", "sel<8>/registers/radix_sort"),
    (3, 64, "f32", "rejected", None),
    (4, 1000, "compact", "full", "sel<8>/registers/counting"),
    (4, 1000, "wide", "full", "sel<8>/registers/radix_sort"),
    (4, 1000, "one_score", "full", "sel<8>/registers/counting_overflow>radix_sort"),
    (4, 1000, "compact", "ragged", "sel<8>/registers/counting"),
    (4, 1000, "mixed", "ragged", "sel<8>/registers/radix_sort"),
    (4, 1000, "f32", "full", "sel<8>/registers/radix_sort"),
    (4, 1000, "compact", "rejected", None),
    (4, 1000, "compact", "empty", None),
    (8, 512, "compact", "full", "sel<8>/registers/counting"),
    (8, 512, "wide", "ragged", "sel<8>/registers/radix_sort"),
    (2, 2048, "compact", "full", "sel<8>/registers/counting_overflow>radix_sort"),
    (2, 2048, "mixed", "full", "sel<8>/registers/radix_sort"),
    (8, 1000, "compact", "full", "sel<16>/registers/counting"),
    (8, 1000, "wide", "full", "sel<16>/registers/radix_sort"),
    (8, 1000, "one_score", "full", "sel<16>/registers/counting_overflow>radix_sort"),
    (8, 1000, "compact", "ragged", "sel<16>/registers/counting"),
    (8, 1000, "mixed", "full", "sel<16>/registers/radix_sort"),
    (8, 1000, "f32", "ragged", "sel<16>/registers/radix_sort"),
    (8, 1000, "compact", "rejected", None),
    (100, 2, "compact", "full", "topk<256>/cap256/flatten/sort"),
    (100, 2, "wide", "ragged", "topk<256>/cap256/flatten/sort"),
    (100, 2, "compact", "rejected", None),
    (1, 4096, "compact", "full", "topk<512>/cap4096/flatten/sort"),
    (1, 4096, "wide", "ragged", "topk<512>/cap4096/flatten/sort"),
    (65, 100, "compact", "full", "topk<512>/cap8192/flatten/counting"),
    (65, 100, "wide", "full", "topk<512>/cap8192/flatten/sort"),
    (65, 100, "compact", "ragged", "topk<512>/cap8192/flatten/counting"),
    (65, 100, "f32", "full", "topk<512>/cap8192/flatten/sort"),
    (16, 1000, "compact", "full", "topk<512>/cap16384/flatten/sort"),
    (3, 4096, "compact", "full", "topk<512>/cap16384/flatten/sort"),
    (3, 4096, "mixed", "ragged", "topk<512>/cap16384/flatten/sort"),
    (1024, 16, "compact", "full", "topk<512>/cap16384/flatten/sort"),
    (1024, 16, "wide", "ragged", "topk<512>/cap16384/flatten/sort"),
    (1024, 16, "compact", "rejected", None),
    (32, 1000, "compact", "full", "topk<512>/cap8192/two_pass/counting"),
    (32, 1000, "wide", "full", "topk<512>/cap8192/two_pass_big>radix/sort"),
    (32, 1000, "one_score", "full", "topk<512>/cap8192/two_pass_overflow>radix/sort"),
    (32, 1000, "compact", "short", "topk<512>/cap8192/flatten/counting"),
    (32, 1000, "compact", "ragged", ("topk<512>/cap8192/two_pass/counting",
                                     "topk<512>/cap8192/two_pass/sort")),
    (32, 1000, "f32", "full", "topk<512>/cap8192/two_pass_big>radix/sort"),
    (32, 1000, "mixed", "full", "topk<512>/cap8192/two_pass_big>radix/sort"),
    (32, 1000, "compact", "rejected", None),
    (64, 4096, "compact", "full", "topk<512>/cap8192/two_pass/counting_overflow>sort"),
    (64, 4096, "wide", "full", "topk<512>/cap8192/two_pass_big>radix/sort"),
    (64, 4096, "compact", "short", ("topk<512>/cap8192/flatten/sort",
                                    "topk<512>/cap8192/flatten/counting_overflow>sort")),
    (1025, 4, "compact", "full", "topk<512>/cap8192/noscan_radix/sort"),
    (1025, 4, "wide", "ragged", "topk<512>/cap8192/noscan_radix/sort"),
    (1025, 4, "compact", "empty", None),
    (1025, 4, "compact", "rejected", None),
    (1100, 8, "compact", "ragged", "topk<512>/cap8192/noscan_radix/sort"),
    (1100, 8, "mixed", "full", "topk<512>/cap8192/noscan_radix/sort"),
]


def case_routes(case):
    r = case[4]
    return () if r is None else (r,) if isinstance(r, str) else tuple(r)


def n_queries(n_lists, k):
    """5 queries; 2 for the two largest shapes."""
    return 2 if n_lists * k >= 32000 else 5


def case_id(case):
    n_lists, k, kind, mode, _ = case
    return f"{n_lists}x{k}-{kind}-{mode}"


def case_lists(case):
    n_lists, k, kind, mode, _ = case
    return make_lists(n_queries(n_lists, k), n_lists, k, kind, mode)
