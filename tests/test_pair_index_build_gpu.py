"""The pairwise route of the quantized index builder on the GPU
(di_index_builder_append_pairwise, the pair part of di_index_builder_quantize,
di_index_builder_pair_terms; csrc/index_build.hip) over the constructed cases of
pair_index_cases.py: maximum, counts, pair keys, rows and postings equal the text route's
answer (the oracle's restatements), the written files are byte-equal to oracle.write_index,
errors are where the header puts them, and an InvertedIndex made from the builder ranks
like InvertedIndex(path) over the oracle's files.  No tolerance: bytes and arrays."""
import numpy as np
import pytest
import torch

import oracle
import pair_index_cases as C

pytestmark = pytest.mark.gpu

ROUTES = ("host", "device")


@pytest.fixture(scope="module")
def L():
    from improving_learned_index_amd import _lib

    if _lib.device_count() < 1:
        pytest.fail("no HIP device visible (GPU test run without a GPU)")
    assert _lib.DI_INDEX_BUILD_TILE == C.T
    return _lib


def _dev(a, dt):
    a = a if a.size else np.zeros(1, dt)
    if a.dtype == np.uint32:
        a = a.view(np.int32)
    return torch.from_numpy(np.ascontiguousarray(a)).to(torch.device("cuda", 0))


def _append(b, a, route):
    if a[0] == "single":
        _, tid, imp, cu = a
        if route == "device":
            return b.append(_dev(tid, np.uint32), _dev(imp, np.float32), _dev(cu, np.int32))
        return b.append(tid, imp, cu)
    _, tid, single, pair, cu, cup = a
    if route == "device":
        return b.append_pairwise(_dev(tid, np.uint32), _dev(single, np.float32),
                                 _dev(pair, np.float32), _dev(cu, np.int32), _dev(cup, np.int64),
                                 timing=True)
    return b.append_pairwise(tid, single, pair, cu, cup, timing=True)


def _filled(L, c, route="host"):
    t = L.TermTable()
    assert t.intern_terms(c.terms).tolist() == list(range(len(c.terms)))
    b = L.IndexBuilder(0)
    first = 0
    for a in c.appends:
        assert _append(b, a, route) == first
        first = b.info()["n_docs"]
    assert first == c.n_docs
    return t, b


def _same(got, want, what):
    got = got.cpu().numpy() if hasattr(got, "cpu") else got
    assert got.shape == want.shape, what
    assert got.view(want.dtype).tobytes() == want.tobytes(), what


def _answer(L, t, b, c, max_val):
    used, term_count, n_kept = b.quantize(len(c.terms), max_val, timing=True)
    first, second, count = b.pair_terms()
    row, n_rows = t.rows_pairwise(term_count, first, second)
    post = b.postings(row, n_rows, timing=True)
    return used, term_count, n_kept, first, second, count, row, n_rows, post


def _check(L, t, b, c, e, max_val, tmp_path=None):
    used, term_count, n_kept, first, second, count, row, n_rows, post = \
        _answer(L, t, b, c, max_val)
    assert used == e.max_used
    assert n_kept == e.pdoc.size
    _same(term_count, e.term_count, "term_count")
    _same(first, e.pair_first, "pair_first")
    _same(second, e.pair_second, "pair_second")
    _same(count, e.pair_count, "pair_count")
    assert n_rows == len(e.vocab)
    _same(row, e.term_row, "term_row")
    _same(post[0], e.term_off, "term_off")
    _same(post[1], e.pdoc, "pdoc")
    _same(post[2], e.pval, "pval")
    if tmp_path is not None:
        L.write_reference_index_pairwise(tmp_path, t, first, second, row, n_rows, *post)
        for f, want in e.files.items():
            assert (tmp_path / f).read_bytes() == want, f
    return post


@pytest.mark.parametrize("route", ROUTES)
@pytest.mark.parametrize("name", C.OK_NAMES)
def test_case_equals_the_text_route(L, name, route, tmp_path):
    c, e = C.case(name), C.expected(name)
    t, b = _filled(L, c, route)
    post = _check(L, t, b, c, e, c.max_val, tmp_path)
    if any(a[0] == "pair" and a[5][-1] > 0 for a in c.appends):
        assert b.timing("ib_pair_append")[1] >= 1
    # a second run of the whole route gives identical bytes
    t2, b2 = _filled(L, c, route)
    again = _answer(L, t2, b2, c, c.max_val)[-1]
    for g, w in zip(again, post):
        assert g.tobytes() == w.tobytes()


def test_quantize_twice_on_split_appends(L, tmp_path):
    """One corpus in one call and in three: each quantize gives its max_val's bytes."""
    m = C.expected("split_appends_1").max_used
    for name in ("split_appends_1", "split_appends_3"):
        c = C.case(name)
        t, b = _filled(L, c)
        for mv in (None, 3 * m, None):
            e = C.expected("split_appends_1", mv)
            _check(L, t, b, c, e, mv, tmp_path / f"{name}_{mv}")
    assert C.expected("split_appends_1", 3 * m).files != C.expected("split_appends_1").files


@pytest.mark.parametrize("name", ["tiny", "name_order", "shared_pairs", "mixed"])
def test_search_from_builder_ranks_like_the_files(L, name, tmp_path):
    from improving_learned_index_amd.inverted_index import InvertedIndex

    c, e = C.case(name), C.expected(name)
    t, b = _filled(L, c)
    b.quantize(len(c.terms), c.max_val)
    ix = InvertedIndex.from_builder(b, t, index_path=tmp_path / "ix")
    assert ix.vocab == {x: i for i, x in enumerate(e.vocab)}
    for f, want in e.files.items():
        assert (tmp_path / "ix" / f).read_bytes() == want, f
    oracle.write_index(tmp_path / "want", e.vocab, e.term_off, e.pdoc, e.pval)
    ref = InvertedIndex(tmp_path / "want")
    qs = C.queries(e)
    assert any("|" in x for q in qs for x in q) and any("|" not in x for q in qs for x in q)
    pair_name = next(x for x in e.vocab if "|" in x and x not in c.terms)
    assert ix.term_ids([pair_name]) == [e.vocab.index(pair_name)]
    for k in (3, 100):
        assert ix.score_batch(qs, k) == ref.score_batch(qs, k)


def test_cu_pairs_off_by_one_changes_nothing(L):
    c = C.case("cu_pairs_off")
    _, tid, single, pair, cu, cup = c.appends[0]
    bad = cup.copy()
    bad[c.notes["doc"] + 1] += 1
    for route in ROUTES:
        t = L.TermTable()
        t.intern_terms(c.terms)
        b = L.IndexBuilder(0)
        before = b.info()
        with pytest.raises(L.DIError) as ei:
            _append(b, ("pair", tid, single, pair, cu, bad), route)
        assert ei.value.code == L.DI_EINVAL and f"document {c.notes['doc']} " in str(ei.value)
        assert b.info() == before
        not_zero, decreasing = cup.copy(), cup.copy()
        not_zero[0] = 1
        decreasing[2] = decreasing[1] - 1
        for wrong in (not_zero, decreasing):
            with pytest.raises(L.DIError) as ei:
                _append(b, ("pair", tid, single, pair, cu, wrong), route)
            assert ei.value.code == L.DI_EINVAL
        assert b.info() == before
        assert _append(b, c.appends[0], route) == 0
        _check(L, t, b, c, C.expected("cu_pairs_off"), None)


@pytest.mark.parametrize("name", ["bad_term_id", "nan_pair", "empty_doc"])
def test_quantize_errors(L, name):
    c = C.case(name)
    t, b = _filled(L, c)
    before = b.info()
    with pytest.raises(L.DIError) as ei:
        b.quantize(len(c.terms), c.max_val)
    assert ei.value.code == getattr(L, c.error)
    if name == "empty_doc":
        assert f"document {c.notes['doc']} " in str(ei.value)
    assert b.info() == before
    with pytest.raises(L.DIError):
        b.pair_terms()  # no quantize has succeeded


@pytest.mark.parametrize("name", ["collision_single", "collision_pair"])
def test_collisions_are_refused_at_the_rows(L, name):
    c = C.case(name)
    t, b = _filled(L, c)
    _, term_count, _ = b.quantize(len(c.terms), c.max_val)
    first, second, _ = b.pair_terms()
    with pytest.raises(L.DIError) as ei:
        t.rows_pairwise(term_count, first, second)
    assert ei.value.code == L.DI_EFORMAT and f"'{c.notes['name']}'" in str(ei.value)


def test_a_builder_without_pairs_is_as_before(L):
    """append_pairwise never called: no pair terms, no pair kernels timed."""
    import index_build_cases as S

    c, e = S.case("dropped"), S.expected("dropped")
    t = L.TermTable()
    t.intern_terms(c.terms)
    b = L.IndexBuilder(0)
    for a in c.appends:
        b.append(*a, timing=True)
    _, term_count, _ = b.quantize(len(c.terms), timing=True)
    first, second, count = b.pair_terms()
    assert first.size == 0 and second.size == 0 and count.size == 0
    assert np.array_equal(term_count, e.term_count)
    for k in ("ib_pair_append", "ib_pair_quantize", "ib_pair_compact", "ib_pair_scatter",
              "ib_pair_number"):
        assert b.timing(k)[1] == 0, k
