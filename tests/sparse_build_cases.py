"""Constructed inputs of the float index builder (di_sparse_builder_*) and a numpy
restatement of the layout it must produce -- the bytes di_sparse_create uploads.

A case is a list of appends, each (term_ids uint32, impacts float32, cu_terms int32) as
di_sparse_builder_append takes them, the number of terms, and a few queries (term ids).
No GPU is needed here; test_sparse_build_cases_cpu.py checks the restatement against
oracle.SparseIndex (the reference's own loop) and that every case reaches what it claims.
"""
from dataclasses import dataclass, field
from functools import lru_cache
from typing import List, Optional, Tuple

import numpy as np

BLOCK = 16384  # documents of one block of the layout
SHORT = 64     # postings of a segment the builder orders with one wave


def expected_layout(term_ids, impacts, cu_terms, n_terms):
    """(term_start int64 [n_terms], blk_off uint32 [n_terms, nb + 1], pdoc uint16, pimp
    float32) of the corpus whose document d holds the pairs [cu_terms[d], cu_terms[d + 1]):
    pairs with impact > 0 only (nano_beir_evaluator.py:98), by term, then by document."""
    term_ids = np.asarray(term_ids, np.uint32)
    impacts = np.asarray(impacts, np.float32)
    cu = np.asarray(cu_terms, np.int64)
    n_docs = len(cu) - 1
    nb = (n_docs + BLOCK - 1) // BLOCK
    doc = np.repeat(np.arange(n_docs, dtype=np.int64), np.diff(cu))
    with np.errstate(invalid="ignore"):
        keep = impacts[:cu[-1]] > 0  # False for 0.0, -0.0, negatives and NaN
    t, d, x = term_ids[:cu[-1]][keep].astype(np.int64), doc[keep], impacts[:cu[-1]][keep]
    assert t.size == 0 or t.max() < n_terms
    order = np.lexsort((d, t))
    t, d, x = t[order], d[order], x[order]
    counts = np.bincount(t * nb + d // BLOCK, minlength=n_terms * nb).reshape(n_terms, nb)
    blk_off = np.zeros((n_terms, nb + 1), np.int64)
    blk_off[:, 1:] = np.cumsum(counts, axis=1)
    term_start = np.zeros(n_terms, np.int64)
    term_start[1:] = np.cumsum(blk_off[:-1, nb])
    return term_start, blk_off.astype(np.uint32), (d % BLOCK).astype(np.uint16), x


@dataclass
class Case:
    name: str
    appends: List[Tuple[np.ndarray, np.ndarray, np.ndarray]]
    n_terms: int
    queries: List[List[int]]
    reserve: Optional[Tuple[int, int]] = None  # a (small) reserve before the first append
    notes: dict = field(default_factory=dict)

    def corpus(self):
        """The appends joined: (term_ids, impacts, cu_terms) of the whole corpus."""
        tid = np.concatenate([a[0] for a in self.appends] or [np.zeros(0, np.uint32)])
        imp = np.concatenate([a[1] for a in self.appends] or [np.zeros(0, np.float32)])
        cu, base = [np.zeros(1, np.int64)], 0
        for a in self.appends:
            cu.append(a[2][1:].astype(np.int64) + base)
            base += int(a[2][-1])
        return tid.astype(np.uint32), imp.astype(np.float32), np.concatenate(cu).astype(np.int32)

    @property
    def n_docs(self):
        return sum(len(a[2]) - 1 for a in self.appends)

    def layout(self):
        return expected_layout(*self.corpus(), self.n_terms)

    def doc_lists(self):
        """Per document its [(term, np.float32 impact)] in input order: what the reference
        gets from get_impact_scores_batch."""
        tid, imp, cu = self.corpus()
        tl, il = tid.tolist(), [np.float32(v) for v in imp]
        return [list(zip(tl[a:b], il[a:b])) for a, b in zip(cu[:-1].tolist(), cu[1:].tolist())]

    def term_major(self):
        """(term_off, pdoc, pimp) for di_sparse_create from the same pairs, the dropped
        ones included: by term, documents in corpus order."""
        tid, imp, cu = self.corpus()
        doc = np.repeat(np.arange(len(cu) - 1, dtype=np.uint32), np.diff(cu.astype(np.int64)))
        order = np.argsort(tid, kind="stable")
        term_off = np.zeros(self.n_terms + 1, np.int64)
        term_off[1:] = np.cumsum(np.bincount(tid, minlength=self.n_terms))
        return term_off, doc[order], imp[order]


def _pack(n_docs, d, t, x):
    """Triplets (doc in [0, n_docs), term, impact), distinct (doc, term) -> one append."""
    d, t = np.asarray(d, np.int64), np.asarray(t, np.int64)
    assert np.unique(d * (1 << 32) + t).size == d.size, "a (doc, term) pair twice"
    order = np.argsort(d, kind="stable")
    cu = np.zeros(n_docs + 1, np.int32)
    cu[1:] = np.cumsum(np.bincount(d, minlength=n_docs))
    return (t[order].astype(np.uint32), np.asarray(x, np.float32)[order], cu)


def _background(rng, n_docs, terms, per_doc):
    """`per_doc` draws of `terms` for every document (repeats removed); impacts in eighths,
    so that sums tie exactly."""
    d = np.repeat(np.arange(n_docs, dtype=np.int64), per_doc)
    t = rng.choice(np.asarray(terms, np.int64), size=d.size)
    key = np.unique(d * (1 << 32) + t)
    d, t = key >> 32, key & 0xFFFFFFFF
    perm = rng.permutation(d.size)  # the pairs of a document in no particular term order
    d, t = d[perm], t[perm]
    return d, t, (rng.integers(1, 40, size=d.size) / 8.0).astype(np.float32)


def _split(n_docs, d, t, x, bounds):
    """One corpus cut into appends at the document numbers `bounds`."""
    out, lo = [], 0
    for hi in list(bounds) + [n_docs]:
        m = (d >= lo) & (d < hi)
        out.append(_pack(hi - lo, d[m] - lo, t[m], x[m]))
        lo = hi
    return out


def _join(*parts):
    return tuple(np.concatenate([np.asarray(p[i]) for p in parts]) for i in range(3))


def _ones(docs, term):
    docs = np.asarray(docs, np.int64)
    return docs, np.full(docs.size, term, np.int64), \
        (1.0 + (docs % 7) / 4.0).astype(np.float32)


def _block_edges(n_docs, seed):
    rng = np.random.default_rng(seed)
    edges = sorted({0, 8191, 8192, 16383, 16384, n_docs - 1})
    # term 0 at the edges only; terms 1-2 at the edges among other documents; a common
    # vocabulary 3-42 (long segments) and a rare one 43-2042 (short segments)
    d, t, x = _join(_ones(edges, 0),
                    _ones(sorted(set(edges) | set(range(5, n_docs, 97))), 1),
                    _ones(sorted(set(edges) | set(range(3, n_docs, 4001))), 2),
                    _background(rng, n_docs, range(3, 43), 2),
                    _background(rng, n_docs, range(43, 2043), 1))
    return Case(f"block_edges_{n_docs}", [_pack(n_docs, d, t, x)], 2043,
                [[0], [0, 1, 2], [5, 0, 44, 7], [2, 1500, 3, 43, 1]],
                notes={"edges": edges})


def _split_appends():
    rng = np.random.default_rng(11)
    n_docs = 17000
    # term 0: on both sides of the append boundary (16000) and of the block boundary (16384)
    d, t, x = _join(_ones(list(range(15990, 16010)) + list(range(16380, 16390)), 0),
                    _background(rng, n_docs, range(1, 30), 2),
                    _background(rng, n_docs, range(30, 900), 1))
    return Case("split_appends", _split(n_docs, d, t, x, [16000]), 900,
                [[0], [0, 3, 31], [29, 1, 0, 500]], notes={"bounds": [16000]})


def _segment_sizes():
    n_docs = BLOCK + 100
    rng = np.random.default_rng(5)
    parts = [_ones(np.arange(n_docs), 0)]  # every document: a full segment in block 0
    for term, size in ((1, 1), (2, 63), (3, 64), (4, 65)):
        parts.append(_ones(np.sort(rng.choice(BLOCK, size=size, replace=False)), term))
    parts.append(_ones(BLOCK + np.sort(rng.choice(100, size=64, replace=False)), 5))
    d, t, x = _join(*parts)
    perm = rng.permutation(d.size)
    return Case("segment_sizes", [_pack(n_docs, d[perm], t[perm], x[perm])], 6,
                [[0], [1, 2, 3, 4], [4, 0, 5], [3, 5]],
                notes={"sizes": [1, 63, 64, 65, BLOCK]})


def _empties():
    rng = np.random.default_rng(2)
    d, t, x = _background(rng, 40, range(0, 12), 3)
    m = (d != 0) & (d != 17) & (d != 39)  # empty documents: the first, one inside, the last
    a = _pack(40, d[m], t[m], x[m])
    none = (np.zeros(0, np.uint32), np.zeros(0, np.float32), np.zeros(1, np.int32))
    only_empty = (np.zeros(0, np.uint32), np.zeros(0, np.float32), np.zeros(4, np.int32))
    d2, t2, x2 = _background(rng, 25, range(5, 14), 2)
    return Case("empties", [none, a, none, only_empty, _pack(25, d2, t2, x2)], 14,
                [[0, 5, 13], [7], [11, 12, 1]])


def _no_kept():
    tid = np.array([0, 1, 2, 1, 0], np.uint32)
    imp = np.array([0.0, -0.0, -1.5, np.nan, -np.inf], np.float32)
    return Case("no_kept", [(tid, imp, np.array([0, 2, 2, 5], np.int32))], 3, [[0, 1, 2], [2]])


def _dropped():
    # term 3: every impact dropped (an empty row); the others lose some pairs
    tid = np.array([0, 3, 1, 2, 3, 0, 1, 3, 2, 0, 3, 4], np.uint32)
    imp = np.array([1.0, 0.0, -0.0, 2.5, -3.0, np.nan, 0.25, np.nan, -1e-30, 1e-30, -0.0, 7.0],
                   np.float32)
    return Case("dropped", [(tid, imp, np.array([0, 3, 5, 8, 12], np.int32))], 5,
                [[0, 1, 2, 3, 4], [3], [3, 4, 0]], notes={"empty_term": 3})


def _growth():
    rng = np.random.default_rng(8)
    sizes = [3, 50, 1, 700, 2000]
    bounds = np.cumsum(sizes)[:-1].tolist()
    n_docs = sum(sizes)
    d, t, x = _background(rng, n_docs, range(0, 300), 6)
    x[::5] = 0.0  # a fifth of the pairs dropped: the kept count is not the appended one
    return Case("growth", _split(n_docs, d, t, x, bounds), 300,
                [[0, 1, 2], [299, 150, 7, 8], [40]], reserve=(1, 4), notes={"bounds": bounds})


def _many_blocks():
    """More than 64 blocks (a row of blk_off longer than a wave) and more than 256 terms
    (term_start scanned over several chunks): mostly empty documents."""
    rng = np.random.default_rng(21)
    nb = 70
    n_docs = nb * BLOCK - 5
    docs = np.sort(rng.choice(n_docs, size=3000, replace=False))
    d = np.repeat(docs, 2)
    t = rng.integers(0, 700, size=d.size)
    key = np.unique(d * (1 << 32) + t)
    d, t = key >> 32, key & 0xFFFFFFFF
    x = (rng.integers(1, 40, size=d.size) / 8.0).astype(np.float32)
    every = _ones(np.arange(0, n_docs, BLOCK // 2 + 1), 700)  # a term in every block
    d, t, x = _join((d, t, x), every)
    return Case("many_blocks", _split(n_docs, d, t, x, [40 * BLOCK + 7]), 701,
                [[700], [700, 3, 650], [1, 2, 3, 4, 5, 6]], notes={"nb": nb})


def _many_terms():
    """More than 256 * 256 terms: the scan of the chunk sums carries over."""
    rng = np.random.default_rng(13)
    n_terms = 70000
    d, t, x = _background(rng, 300, rng.choice(n_terms, size=4000, replace=False), 12)
    d2, t2, x2 = _ones(np.arange(0, 300, 3), n_terms - 1)
    d, t, x = _join((d, t, x), (d2, t2, x2))
    qs = [[n_terms - 1], [int(t[0]), n_terms - 1, int(t[5])], [int(v) for v in t[10:16]]]
    return Case("many_terms", [_pack(300, d, t, x)], n_terms,
                [list(dict.fromkeys(q)) for q in qs])


_BUILDERS = {
    "block_edges_16385": lambda: _block_edges(16385, 1),
    "block_edges_32769": lambda: _block_edges(32769, 3),
    "split_appends": _split_appends,
    "segment_sizes": _segment_sizes,
    "empties": _empties,
    "no_kept": _no_kept,
    "dropped": _dropped,
    "growth": _growth,
    "many_blocks": _many_blocks,
    "many_terms": _many_terms,
}
CASE_NAMES = list(_BUILDERS)


@lru_cache(maxsize=None)
def case(name) -> Case:
    return _BUILDERS[name]()


@lru_cache(maxsize=None)
def oracle_index(name):
    """oracle.SparseIndex of the case (the reference's loop over every posting); its terms
    are the case's term ids, renumbered by the oracle in order of first kept posting."""
    import oracle

    c = case(name)
    return oracle.SparseIndex(list(range(c.n_docs)), c.doc_lists())


def segment_sizes(blk_off):
    """Posting counts of the non-empty (term, block) segments."""
    s = np.diff(blk_off.astype(np.int64), axis=1).ravel()
    return s[s > 0]
