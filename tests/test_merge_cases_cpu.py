"""The cases of tests/test_topk_merge_gpu.py, checked without a GPU: every case takes the
route of di_topk_merge that its row names (merge_cases.expected_path restates the dispatch
of csrc/topk_merge.hip), the cases between them take every route, the numpy definition agrees
with Python's sorted(), and the data tells the two list layouts apart."""
import numpy as np
import pytest

import merge_cases as M


@pytest.mark.parametrize("case", M.CASES, ids=M.case_id)
def test_case_takes_its_route(case):
    n_lists, k, kind, mode, _ = case
    keys, counts = M.case_lists(case)
    assert keys.shape == (M.n_queries(n_lists, k), n_lists, k)
    paths = M.query_paths(n_lists, k, keys, counts)
    for r in M.case_routes(case):
        assert r in paths, (r, paths)
    if mode == "full":
        assert len(set(paths)) == 1, paths
    for p in paths:  # no query wanders onto a route the list does not know
        assert p in M.ROUTES or p.endswith("/rejected"), p
    if mode == "rejected":
        assert [p.endswith("/rejected") for p in paths] == [q == 1 for q in range(len(paths))]


def test_cases_cover_every_route():
    named = {r for c in M.CASES for r in M.case_routes(c)}
    assert named == M.ROUTES, (M.ROUTES - named, named - M.ROUTES)
    # every kind and every count mode is used, and the merge shapes of the worlds the
    # exchange test runs (8 x 1000, 64 x 4096) are among them
    assert {c[2] for c in M.CASES} == set(M.KINDS)
    assert {c[3] for c in M.CASES} == set(M.COUNT_MODES)
    assert {(8, 1000), (64, 4096)} <= {c[:2] for c in M.CASES}


def test_expected_path_thresholds():
    """The predicate at the constants' edges (keys unseen: no two in one bin)."""
    full = lambda n, k: np.full(n, k)  # noqa: E731
    assert M.expected_path(64, 64, full(64, 64), False) == "sel<8>/registers/counting"
    assert M.expected_path(64, 65, full(64, 65), False) == "sel<16>/registers/counting"
    assert M.expected_path(64, 128, full(64, 128), False) == "sel<16>/registers/counting"
    assert M.expected_path(65, 64, full(65, 64), False).startswith("topk<512>/cap8192/flatten")
    assert M.expected_path(4, 2049, full(4, 2049), False) == "topk<512>/cap16384/flatten/sort"
    assert M.expected_path(4, 256, full(4, 256), False) == "sel<8>/registers/radix_sort"  # 1024
    assert M.expected_path(5, 205, full(5, 205), False) == "sel<8>/registers/counting"    # 1025
    assert M.expected_path(128, 2, full(128, 2), False) == "topk<256>/cap256/flatten/sort"
    assert M.expected_path(129, 2, full(129, 2), False) == "topk<512>/cap512/flatten/sort"
    assert M.expected_path(1024, 16, full(1024, 16), False) == "topk<512>/cap16384/flatten/sort"
    assert M.expected_path(1024, 17, full(1024, 17), False) == "topk<512>/cap8192/two_pass/sort"
    assert M.expected_path(1025, 1, full(1025, 1), False) == "topk<512>/cap8192/noscan_radix/sort"
    c = full(32, 1000)
    assert M.expected_path(32, 1000, c, True) == "topk<512>/cap8192/two_pass_big>radix/sort"
    c[0] = -5
    assert M.expected_path(32, 1000, c, False) == "topk<512>/cap8192/rejected"


def test_reference_merge_is_sorted_union():
    rng = np.random.default_rng(0)
    n_q, n_lists, k = 4, 3, 7
    keys = rng.integers(0, 1 << 64, (n_q, n_lists, k), dtype=np.uint64)  # across the sign bit
    keys = np.sort(keys, axis=2)[:, :, ::-1]
    counts = rng.integers(0, k + 3, (n_q, n_lists)).astype(np.int32)  # some above k
    counts[2, 1] = -1
    for lists_major in (False, True):
        kk = np.ascontiguousarray(keys.transpose(1, 0, 2)) if lists_major else keys
        cc = np.ascontiguousarray(counts.T) if lists_major else counts
        out, n = M.reference_merge(kk, cc, k, lists_major)
        for q in range(n_q):
            if q == 2:
                assert n[q] == -1
                continue
            union = [int(x) for l in range(n_lists) for x in keys[q, l, :min(counts[q, l], k)]]
            want = sorted(union, reverse=True)[:k]
            assert n[q] == len(want) and [int(x) for x in out[q, :n[q]]] == want


@pytest.mark.parametrize("case", [c for c in M.CASES if c[0] > 1 and c[3] != "empty"],
                         ids=M.case_id)
def test_data_tells_the_layouts_apart(case):
    """Reading the lists-major buffer as query-major changes the definition's result, so a
    kernel that mixed up the strides could not pass.  (All-empty lists merge to nothing in
    either layout: that mode is exempt.)"""
    n_lists, k = case[:2]
    keys, counts = M.case_lists(case)
    n_q = keys.shape[0]
    assert n_q > 1
    want = M.reference_merge(keys, counts, k)
    lm_keys = np.ascontiguousarray(keys.transpose(1, 0, 2))
    lm_counts = np.ascontiguousarray(counts.T)
    same = M.reference_merge(lm_keys, lm_counts, k, lists_major=True)
    assert (same[0] == want[0]).all() and (same[1] == want[1]).all()
    misread = M.reference_merge(lm_keys.reshape(n_q, n_lists, k),
                                lm_counts.reshape(n_q, n_lists), k)
    assert not ((misread[0] == want[0]).all() and (misread[1] == want[1]).all())
