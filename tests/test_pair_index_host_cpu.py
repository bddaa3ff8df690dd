"""The host half of the pairwise index route without a GPU: di_term_table_rows_pairwise
numbers single and pair terms in sorted() order of their names (for 1 and 8 host threads),
refuses two kept entries with one name, and di_write_reference_index_pairwise writes the
oracle's files from the expected postings (pair_index_cases.py)."""
import os

import numpy as np
import pytest

import pair_index_cases as C


@pytest.fixture(scope="module")
def L():
    from improving_learned_index_amd import _lib

    return _lib


def _table(L, c):
    t = L.TermTable()
    assert t.intern_terms(c.terms).tolist() == list(range(len(c.terms)))
    return t


@pytest.mark.parametrize("name", C.OK_NAMES)
def test_rows_and_files_equal_the_text_route(L, name, tmp_path):
    c, e = C.case(name), C.expected(name)
    t = _table(L, c)
    for threads in ("1", "8"):
        os.environ["DI_HOST_THREADS"] = threads
        try:
            row, n_rows = t.rows_pairwise(e.term_count, e.pair_first, e.pair_second)
        finally:
            del os.environ["DI_HOST_THREADS"]
        assert n_rows == len(e.vocab) and np.array_equal(row, e.term_row), threads
    assert t.vocab(row, e.pair_first, e.pair_second) == {x: i for i, x in enumerate(e.vocab)}
    L.write_reference_index_pairwise(tmp_path, t, e.pair_first, e.pair_second, row, n_rows,
                                     e.term_off, e.pdoc, e.pval)
    for f, want in e.files.items():
        assert (tmp_path / f).read_bytes() == want, f


def test_no_pair_terms_is_rows(L):
    c, e = C.case("tiny"), C.expected("tiny")
    t = _table(L, c)
    none = np.zeros(0, np.uint32)
    row, n_rows = t.rows_pairwise(e.term_count, none, none)
    want, n_want = t.rows(e.term_count)
    assert n_rows == n_want and np.array_equal(row, want)


@pytest.mark.parametrize("name", ["collision_single", "collision_pair"])
def test_two_entries_with_one_name_are_refused(L, name):
    c = C.case(name)
    n = C.numpy_order(c)
    t = _table(L, c)
    with pytest.raises(L.DIError) as ei:
        t.rows_pairwise(n["term_count"], n["pair_first"], n["pair_second"])
    assert ei.value.code == L.DI_EFORMAT
    assert f"'{c.notes['name']}'" in str(ei.value) and "text route" in str(ei.value)


def test_a_pair_id_past_the_table_is_refused(L):
    c, e = C.case("tiny"), C.expected("tiny")
    t = _table(L, c)
    bad = e.pair_second.copy()
    bad[0] = len(c.terms)
    with pytest.raises(L.DIError) as ei:
        t.rows_pairwise(e.term_count, e.pair_first, bad)
    assert ei.value.code == L.DI_EINVAL
