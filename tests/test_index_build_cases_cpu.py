"""The constructed cases of index_build_cases.py, checked without a GPU: a plain numpy
restatement of the expected order equals the oracle's text route, and every case reaches
the hazard it claims."""
import struct

import numpy as np
import pytest

import index_build_cases as C
import oracle

T = C.T


@pytest.mark.parametrize("name", C.OK_NAMES)
def test_numpy_restatement_equals_the_oracle(name):
    c, e = C.case(name), C.expected(name)
    m, kept, term_off, pdoc, pval, term_count, term_row = C.numpy_order(c, c.max_val)
    assert m == e.max_used
    assert kept == e.vocab
    assert np.array_equal(term_off, e.term_off)
    assert np.array_equal(pdoc, e.pdoc)
    assert np.array_equal(pval, e.pval)
    assert np.array_equal(term_count, e.term_count)
    assert np.array_equal(term_row, e.term_row)


@pytest.mark.parametrize("name", C.OK_NAMES)
def test_rows_are_sorted_kept_strings(name):
    c, e = C.case(name), C.expected(name)
    kept = [t for t, n in zip(c.terms, e.term_count.tolist()) if n > 0]
    assert e.vocab == sorted(kept)
    assert [c.terms[i] for i in np.argsort(np.where(e.term_row < 0, 1 << 30, e.term_row),
                                           kind="stable")[:len(kept)]] == e.vocab
    # bytes of the UTF-8 order the same way (what the native table compares)
    assert sorted(kept, key=lambda s: s.encode("utf-8")) == e.vocab


def test_impacts_are_what_round3_leaves():
    for name in C.CASE_NAMES:
        _, imp, _ = C.case(name).corpus()
        assert np.array_equal(oracle.round3(imp), imp), name


def test_ties_long_census():
    c, e = C.case("ties_long"), C.expected("ties_long")
    assert c.n_docs == 65537 and int(e.pdoc.max()) >= 65536
    r = e.vocab.index("common")
    a, b = int(e.term_off[r]), int(e.term_off[r + 1])
    assert b - a == 65537 > 16 * T
    assert sorted(set(e.pval[a:b].tolist())) == [85, 170, 255]
    # three runs of equal values, docs ascending inside each, each run longer than a tile
    for v in (85, 170, 255):
        docs = e.pdoc[a:b][e.pval[a:b] == v]
        assert docs.size > T and (np.diff(docs.astype(np.int64)) > 0).all()
    others = np.delete(np.diff(e.term_off), r)
    assert others.max() <= 2
    # in document order (the builder's buffer) the three values alternate: equal keys on
    # both sides of every tile boundary
    tid, _, _ = c.corpus()
    assert (tid == 0).sum() == 65537


@pytest.mark.parametrize("total", [T - 1, T, T + 1])
def test_tile_edges_census(total):
    e = C.expected(f"tile_edges_{total}")
    assert e.pdoc.size == total == C.case(f"tile_edges_{total}").notes["kept"]
    _, imp, _ = C.case(f"tile_edges_{total}").corpus()
    assert imp.size > total  # some pairs are dropped


def test_tile_owner_census():
    c, e = C.case("tile_owner"), C.expected("tile_owner")
    assert e.pdoc.size == c.notes["kept"] > 2 * T
    m, _, _, _, _, _, _ = C.numpy_order(c)
    tid, imp, _ = c.corpus()
    val = np.trunc(imp.astype(np.float64) * (255.0 / m)).astype(np.int64)
    first = np.flatnonzero(val > 0)[:T]  # the first tile of the kept records
    assert (tid[first] == 0).all() and np.unique(val[first]).size == 1


def test_all_values_census():
    e = C.expected("all_values")
    r = e.vocab.index("w0000")
    vals = e.pval[int(e.term_off[r]):int(e.term_off[r + 1])]
    assert sorted(set(vals.tolist())) == list(range(1, 256))
    docs = e.pdoc[int(e.term_off[r]):int(e.term_off[r + 1])].astype(np.int64)
    assert (np.diff(docs) < 0).any()  # value order is not document order
    assert e.max_used == 255.0


def test_max_254_census():
    c, e = C.case("max_254"), C.expected("max_254")
    assert int(e.pval.max()) == 254
    m = float(np.float32(c.notes["k_max"] / 1000.0))
    assert e.max_used == m and int(m * (255.0 / m)) == 254


def test_dropped_census():
    c, e = C.case("dropped"), C.expected("dropped")
    assert "gone" not in e.vocab and "relu" not in e.vocab
    assert e.term_count[c.terms.index("gone")] == 0 and e.term_row[c.terms.index("gone")] == -1
    assert c.notes["empty_after"] not in e.pdoc.tolist()
    _, imp, _ = c.corpus()
    assert (imp == 0.0).any()
    assert 0 < e.pdoc.size < imp.size and int(e.pval.min()) == 1


def test_many_terms_census():
    c, e = C.case("many_terms"), C.expected("many_terms")
    assert len(c.terms) > 65536 and len(e.vocab) == c.notes["kept_terms"] > 65536
    assert C.row_digits(len(e.vocab)) == 3
    assert (e.term_count == 0).sum() == len(c.terms) - len(e.vocab) > 0
    # ids in order of first appearance are far from the sorted order
    used = e.term_row[e.term_row >= 0]
    # (the multiplier 7919 wraps around the 70 001 strings 7 918 times)
    assert (np.diff(used.astype(np.int64)) < 0).sum() > 7000


def test_utf8_terms_census():
    c, e = C.case("utf8_terms"), C.expected("utf8_terms")
    a, b = c.notes["prefix"]
    assert b.startswith(a) and e.vocab.index(a) + 1 == e.vocab.index(b)
    assert {"a,b", "a:b", "x|y"} <= set(e.vocab)
    assert any(len(t.encode("utf-8")) > len(t) for t in e.vocab)
    assert e.files["vocab.txt"].decode("utf-8").splitlines() == e.vocab


def test_split_appends_census():
    c = C.case("split_appends")
    assert [len(a[2]) - 1 for a in c.appends] == c.notes["sizes"]
    assert c.reserve[1] < int(c.appends[2][2][-1])


def test_max_val_cases():
    above, below = C.case("max_val_above"), C.case("max_val_below")
    top = float(above.corpus()[1].max())
    assert above.max_val > top > below.max_val
    assert int(C.expected("max_val_above").pval.max()) < 255
    lines, _ = oracle.quantize_lines(below.impact_lines(), below.max_val)
    docs = [{t: float(v) for t, v in (p.split(": ") for p in l.split(", "))} for l in lines]
    with pytest.raises(struct.error):  # create.py:45
        oracle.build_index(docs)


def test_error_cases_are_the_text_routes_errors():
    c = C.case("empty_doc")
    assert c.impact_lines()[c.notes["doc"]] == ""
    with pytest.raises(ValueError):  # quantize.py:21-22 on the empty line
        oracle.quantize_lines(c.impact_lines())
    assert float(C.case("all_zero").corpus()[1].max()) == 0.0
    c = C.case("bad_term")
    assert any(", " in t for t in c.terms)
    c = C.case("bad_term_id")
    assert int(c.corpus()[0].max()) == len(c.terms)
    assert C.case("unassigned_row").stage == "postings"
    for name in C.ERROR_NAMES:
        assert C.case(name).error in ("DI_EFORMAT", "DI_EINVAL", "DI_ERANGE")
