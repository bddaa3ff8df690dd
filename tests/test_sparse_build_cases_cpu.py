"""The float index builder's constructed cases (sparse_build_cases.py) without a GPU: the
numpy restatement of the layout, read back term by term, is oracle.SparseIndex's
term_off / pdoc / pimp under the oracle's term renumbering, and a census shows that each
case reaches what it claims."""
import numpy as np
import pytest

import sparse_build_cases as C


@pytest.mark.parametrize("name", C.CASE_NAMES)
def test_expected_layout_is_the_oracles_index(name):
    c = C.case(name)
    ora = C.oracle_index(name)
    term_start, blk_off, pdoc, pimp = c.layout()
    nb = blk_off.shape[1] - 1
    assert nb == (c.n_docs + C.BLOCK - 1) // C.BLOCK
    assert blk_off.dtype == np.uint32 and pdoc.dtype == np.uint16 and pimp.dtype == np.float32
    assert np.array_equal(blk_off[:, 0], np.zeros(c.n_terms, np.uint32))
    # the rows tile the posting arrays, and the terms with a posting are the oracle's
    assert np.array_equal(term_start[1:], np.cumsum(blk_off[:-1, nb].astype(np.int64)))
    n_post = int(blk_off[:, nb].sum())
    assert n_post == pdoc.size == pimp.size
    kept_terms = np.flatnonzero(blk_off[:, nb]).tolist()
    assert sorted(ora.vocab) == kept_terms
    assert n_post == int(ora.term_off[-1])
    for t in kept_terms:
        s = int(term_start[t])
        docs = []
        for b in range(nb):
            lo, hi = int(blk_off[t, b]), int(blk_off[t, b + 1])
            local = pdoc[s + lo:s + hi].astype(np.int64)
            assert np.all(np.diff(local) > 0)  # ascending inside a segment, no repeat
            docs.append(local + b * C.BLOCK)
        docs = np.concatenate(docs)
        o = ora.vocab[t]
        a, e = int(ora.term_off[o]), int(ora.term_off[o + 1])
        assert np.array_equal(docs, ora.pdoc[a:e].astype(np.int64)), t
        assert np.array_equal(pimp[s:s + docs.size].view(np.uint32),
                              ora.pimp[a:e].view(np.uint32)), t


def test_term_major_arrays_hold_every_pair():
    """What the GPU test hands to di_sparse_create: every pair, dropped ones included, by
    term with documents in corpus order."""
    for name in ("dropped", "split_appends"):
        c = C.case(name)
        term_off, pdoc, pimp = c.term_major()
        tid, imp, cu = c.corpus()
        assert term_off[-1] == tid.size == pdoc.size
        for t in range(c.n_terms):
            d = pdoc[term_off[t]:term_off[t + 1]]
            assert np.all(np.diff(d.astype(np.int64)) > 0)
        with np.errstate(invalid="ignore"):
            assert int((pimp > 0).sum()) == c.layout()[2].size


def test_census_block_edges():
    for name in ("block_edges_16385", "block_edges_32769"):
        c = C.case(name)
        term_start, blk_off, pdoc, _ = c.layout()
        edges = c.notes["edges"]
        assert {0, 8191, 8192, 16383, 16384, c.n_docs - 1} == set(edges)
        # term 0's postings are exactly the edge documents
        got = []
        for b in range(blk_off.shape[1] - 1):
            seg = pdoc[term_start[0] + blk_off[0, b]:term_start[0] + blk_off[0, b + 1]]
            got += (seg.astype(np.int64) + b * C.BLOCK).tolist()
        assert got == edges
        assert blk_off[0, -1] == len(edges)
        assert c.n_docs % C.BLOCK == 1  # the last block holds one document
        sizes = C.segment_sizes(blk_off)
        assert sizes.min() <= 2 and sizes.max() > C.SHORT  # both ordering routes


def test_census_segment_sizes():
    c = C.case("segment_sizes")
    _, blk_off, _, _ = c.layout()
    sizes = set(C.segment_sizes(blk_off).tolist())
    assert {1, C.SHORT - 1, C.SHORT, C.SHORT + 1, C.BLOCK} <= sizes
    assert blk_off[0, 1] == C.BLOCK  # term 0 in every document of block 0: a full segment
    assert blk_off[5, 1] == 0 and blk_off[5, 2] == C.SHORT  # a segment that starts a row late


def test_census_split_appends():
    c = C.case("split_appends")
    assert len(c.appends) == 2
    first = len(c.appends[0][2]) - 1
    assert first == 16000 and c.n_docs > C.BLOCK > first
    tid, imp, cu = c.corpus()
    doc = np.repeat(np.arange(c.n_docs), np.diff(cu.astype(np.int64)))
    d0 = doc[tid == 0]
    assert d0.min() < first <= d0[d0 >= first].min() < C.BLOCK <= d0.max()
    assert np.any((d0 >= first) & (d0 < C.BLOCK))


def test_census_empty_and_dropped():
    c = C.case("empties")
    sizes = [len(a[2]) - 1 for a in c.appends]
    assert 0 in sizes  # an append of zero documents
    _, _, cu = c.corpus()
    n = np.diff(cu.astype(np.int64))
    assert n[0] == 0 and n[-1] > 0 and np.any(n[1:40] == 0)
    assert any(a[0].size == 0 and len(a[2]) > 1 for a in c.appends)  # only empty documents
    c = C.case("no_kept")
    term_start, blk_off, pdoc, pimp = c.layout()
    assert pdoc.size == 0 and not blk_off.any() and not term_start.any()
    assert not C.oracle_index("no_kept").vocab
    c = C.case("dropped")
    _, imp, _ = c.corpus()
    assert np.signbit(imp[imp == 0]).any() and not np.signbit(imp[imp == 0]).all()
    assert np.isnan(imp).any() and (imp < 0).any()
    _, blk_off, _, _ = c.layout()
    e = c.notes["empty_term"]
    assert not blk_off[e].any() and e not in C.oracle_index("dropped").vocab
    assert np.all(blk_off[[0, 1, 2, 4], -1] > 0)


def test_census_growth_and_scale():
    c = C.case("growth")
    assert c.reserve is not None and c.reserve[1] < c.appends[0][0].size
    assert len(c.appends) == 5 and c.layout()[2].size < c.corpus()[0].size
    c = C.case("many_blocks")
    _, blk_off, _, _ = c.layout()
    assert blk_off.shape[1] - 1 == c.notes["nb"] > 64 and c.n_terms > 256
    assert np.all(np.diff(blk_off[700].astype(np.int64)) > 0)  # a posting in every block
    assert len(c.appends) == 2
    c = C.case("many_terms")
    assert c.n_terms > 256 * 256
    assert c.layout()[1][c.n_terms - 1, -1] == 100
