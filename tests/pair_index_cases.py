"""Constructed inputs of the pairwise route of the quantized index builder
(di_index_builder_append_pairwise, di_index_builder_pair_terms, di_term_table_rows_pairwise)
and their expected answers.

A case is a list of term strings (term id = position) and a list of appends.  A pairwise
append is ("pair", term_ids uint32, single float32, pair float32, cu_terms int32, cu_pairs
int64) as di_index_builder_append_pairwise takes it: raw (unrounded) scores, the pairs of a
T-term document in itertools.combinations order.  A ("single", term_ids, impacts, cu_terms)
append is di_index_builder_append's.  The expected answer is the text route's, by the
oracle's restatements: per document the entries DeepPairwiseImpact.compute_term_impacts
keeps (pairwise_impact.py:98-129: every term, every pair whose round3 score is not zero,
named t_a + '|' + t_b) -> oracle.impact_line -> oracle.quantize_lines -> oracle.build_index
-> oracle.write_index.  No GPU is needed here; test_pair_index_cases_cpu.py checks a numpy
restatement against it and that every case reaches what it claims.
"""
import tempfile
from dataclasses import dataclass, field
from functools import lru_cache
from pathlib import Path
from typing import List, Optional

import numpy as np

from index_build_cases import T, f32k, find_max_254  # noqa: F401  (T: DI_INDEX_BUILD_TILE)


@dataclass
class Case:
    name: str
    terms: List[str]
    appends: List[tuple]
    max_val: Optional[float] = None
    error: Optional[str] = None   # the DIError code name the route must raise ...
    stage: Optional[str] = None   # ... in "append", "quantize" or "rows"
    notes: dict = field(default_factory=dict)

    @property
    def n_docs(self):
        return sum(len(a[-1 if a[0] == "single" else -2]) - 1 for a in self.appends)

    def documents(self):
        """Per document (term ids, single scores, pair scores or None for a document of a
        single-term append)."""
        out = []
        for a in self.appends:
            if a[0] == "single":
                _, tid, imp, cu = a
                for lo, hi in zip(cu[:-1].tolist(), cu[1:].tolist()):
                    out.append((tid[lo:hi], imp[lo:hi], None))
            else:
                _, tid, single, pair, cu, cup = a
                for d in range(len(cu) - 1):
                    out.append((tid[cu[d]:cu[d + 1]], single[cu[d]:cu[d + 1]],
                                pair[cup[d]:cup[d + 1]]))
        return out

    def entries(self):
        """The records the route keeps at append, flat over the collection: singles
        (term id, doc, round3 score) and pairs (id_a, id_b, doc, round3 score), a pair kept
        iff its round3 score is not zero (oracle.round3)."""
        import oracle

        s_t, s_d, s_v, p_a, p_b, p_d, p_v = [], [], [], [], [], [], []
        for d, (tid, single, pair) in enumerate(self.documents()):
            s_t.append(tid.astype(np.int64))
            s_d.append(np.full(tid.size, d, np.int64))
            s_v.append(oracle.round3(single))
            if pair is not None and pair.size:
                a, b = np.triu_indices(tid.size, 1)  # combinations order
                r = oracle.round3(pair)
                keep = r != 0  # -0.0 is dropped, NaN is kept: `if round(score, 3)`
                p_a.append(tid[a[keep]].astype(np.int64))
                p_b.append(tid[b[keep]].astype(np.int64))
                p_d.append(np.full(int(keep.sum()), d, np.int64))
                p_v.append(r[keep])
        cat = lambda x, dt: np.concatenate(x).astype(dt) if x else np.zeros(0, dt)  # noqa: E731
        return (cat(s_t, np.int64), cat(s_d, np.int64), cat(s_v, np.float32),
                cat(p_a, np.int64), cat(p_b, np.int64), cat(p_d, np.int64), cat(p_v, np.float32))

    def impact_lines(self):
        """The lines index --pairwise writes: per document its terms and kept pairs by raw
        score descending, equal scores by position (pairwise_impact.py:126-128)."""
        import oracle

        lines = []
        for tid, single, pair in self.documents():
            names = [self.terms[t] for t in tid.tolist()]
            scores = np.asarray(single, np.float32)
            if pair is not None and pair.size:
                a, b = np.triu_indices(tid.size, 1)
                keep = oracle.round3(pair) != 0
                names = names + [names[i] + "|" + names[j]
                                 for i, j in zip(a[keep].tolist(), b[keep].tolist())]
                scores = np.concatenate([scores, pair[keep]])
            order = np.argsort(-scores.astype(np.float64), kind="stable")
            lines.append(oracle.impact_line([names[i] for i in order.tolist()], scores[order]))
        return lines


@dataclass
class Expected:
    max_used: float
    vocab: List[str]
    term_off: np.ndarray
    pdoc: np.ndarray
    pval: np.ndarray
    term_count: np.ndarray   # per single term id
    pair_first: np.ndarray   # the distinct kept pair keys, ascending (first, second)
    pair_second: np.ndarray
    pair_count: np.ndarray
    term_row: np.ndarray     # per single term id, then per pair term; -1: not in the vocab
    files: dict              # name -> bytes of oracle.write_index


def numpy_order(c: Case, max_val=None):
    """The expected arrays restated in plain numpy: quantize in float64, drop the zeros,
    number the distinct kept pair keys, rows = sorted() of the kept names, lexsort by
    (row, -val, doc)."""
    s_t, s_d, s_v, p_a, p_b, p_d, p_v = c.entries()
    n_terms = len(c.terms)
    both = np.concatenate([s_v, p_v]).astype(np.float64)
    m = float(max_val) if max_val is not None else max(0.0, float(both.max(initial=0.0)))
    q = lambda v: np.trunc(v.astype(np.float64) * (255.0 / m)).astype(np.int64)  # noqa: E731
    sq, pq = q(s_v), q(p_v)
    ks, kp = sq > 0, pq > 0
    term_count = np.bincount(s_t[ks], minlength=n_terms).astype(np.int64)
    key = (p_a[kp] << 32) | p_b[kp]
    ukey, inv, pcount = np.unique(key, return_inverse=True, return_counts=True)
    first, second = (ukey >> 32).astype(np.uint32), (ukey & 0xFFFFFFFF).astype(np.uint32)
    names = [c.terms[t] for t in np.flatnonzero(term_count).tolist()]
    ids = np.flatnonzero(term_count).tolist()
    names += [c.terms[a] + "|" + c.terms[b] for a, b in zip(first.tolist(), second.tolist())]
    ids += list(range(n_terms, n_terms + ukey.size))
    order = sorted(range(len(names)), key=lambda i: names[i])
    term_row = np.full(n_terms + ukey.size, -1, np.int32)
    for r, i in enumerate(order):
        term_row[ids[i]] = r
    vocab = [names[i] for i in order]
    ent = np.concatenate([s_t[ks], n_terms + inv.reshape(-1)])
    doc = np.concatenate([s_d[ks], p_d[kp]])
    val = np.concatenate([sq[ks], pq[kp]])
    row = term_row[ent].astype(np.int64)
    o = np.lexsort((doc, -val, row))
    term_off = np.zeros(len(vocab) + 1, np.int64)
    term_off[1:] = np.cumsum(np.bincount(row, minlength=len(vocab)))
    return dict(max_used=m, vocab=vocab, term_off=term_off, pdoc=doc[o].astype(np.uint32),
                pval=val[o], term_count=term_count, pair_first=first, pair_second=second,
                pair_count=pcount.astype(np.int64), term_row=term_row)


def oracle_index(c: Case, max_val=None):
    """(max_used, vocab, term_off, pdoc, pval, files) of the text route, by the oracle."""
    import oracle

    qlines, used = oracle.quantize_lines(c.impact_lines(), max_val)
    with tempfile.TemporaryDirectory() as tmp:
        qf = Path(tmp) / "collection.quantized"
        qf.write_text("".join(l + "\n" for l in qlines), encoding="utf-8")
        vocab, term_off, pdoc, pval = oracle.build_index(oracle.collection_items(qf))
        oracle.write_index(Path(tmp) / "index", vocab, term_off, pdoc, pval)
        files = {p.name: p.read_bytes() for p in (Path(tmp) / "index").iterdir()}
    return used, vocab, term_off, pdoc, pval, files


@lru_cache(maxsize=None)
def expected(name, max_val=None) -> Expected:
    """The text route's answer for a case (max_val None: the case's own).  The postings and
    files are the oracle's; the pair keys and rows, which the text route never names, come
    from numpy_order, which test_pair_index_cases_cpu.py holds equal to the oracle."""
    c = case(name)
    assert c.error is None or c.stage in ("append", "rows")
    mv = c.max_val if max_val is None else max_val
    used, vocab, term_off, pdoc, pval, files = oracle_index(c, mv)
    n = numpy_order(c, mv)
    e = Expected(used, vocab, term_off, pdoc, pval, n["term_count"], n["pair_first"],
                 n["pair_second"], n["pair_count"], n["term_row"], files)
    for a in (e.term_off, e.pdoc, e.pval, e.term_count, e.pair_first, e.pair_second,
              e.pair_count, e.term_row):
        a.setflags(write=False)
    return e


# --------------------------------------------------------------------------- construction
def n_comb(t):
    return t * (t - 1) // 2


def pair_append(docs):
    """docs: (term ids, single scores, pair scores [T(T-1)/2]) per document -> one append."""
    tid = np.concatenate([np.asarray(d[0], np.uint32) for d in docs])
    single = np.concatenate([np.asarray(d[1], np.float32) for d in docs])
    pair = np.concatenate([np.asarray(d[2], np.float32).reshape(-1) for d in docs])
    cu = np.zeros(len(docs) + 1, np.int32)
    cu[1:] = np.cumsum([len(d[0]) for d in docs])
    cup = np.zeros(len(docs) + 1, np.int64)
    cup[1:] = np.cumsum([n_comb(len(d[0])) for d in docs])
    for d in docs:
        assert len(d[1]) == len(d[0]) and np.asarray(d[2]).size == n_comb(len(d[0]))
        assert len(set(np.asarray(d[0]).tolist())) == len(d[0]), "a term twice in a document"
    return ("pair", tid, single, pair, cu, cup)


def single_append(docs):
    """docs: (term ids, thousandths) per document -> one di_index_builder_append."""
    tid = np.concatenate([np.asarray(d[0], np.uint32) for d in docs])
    imp = np.concatenate([f32k(d[1]) for d in docs])
    cu = np.zeros(len(docs) + 1, np.int32)
    cu[1:] = np.cumsum([len(d[0]) for d in docs])
    return ("single", tid, imp, cu)


def _raw(rng, n, lo=100, hi=4000):
    """Raw scores: thousandths in [lo, hi) plus a fraction below the rounding step, so
    round3 has something to do."""
    k = rng.integers(lo, hi, size=n).astype(np.float64)
    return ((k + rng.uniform(-0.4, 0.4, size=n)) / 1000.0).astype(np.float32)


def _rand_doc(rng, term_ids, t, lo=100, hi=4000):
    ids = rng.choice(np.asarray(term_ids), size=t, replace=False)
    return (ids, _raw(rng, t, lo, hi), _raw(rng, n_comb(t), lo, hi))


def _words(n, prefix="w"):
    return [f"{prefix}{i:04d}" for i in range(n)]


def _tiny():
    docs = [([0], [1.25], []),
            ([1, 0], [0.5, 2.0], [0.75]),
            ([0, 2, 3], [1.0, 0.3, 0.9], [0.2, 1.5, 0.6])]
    return Case("tiny", ["a", "b", "c", "d"], [pair_append(docs)], notes={"T": [1, 2, 3]})


ROUND_EDGES = [0.0, -0.0, 0.0004, 0.0005, 0.00051, 0.0015]


def _round_edges():
    # the maximum is 0.2: a rounded 0.001 quantizes to int(1.275) = 1 and stays
    docs = [([0, 1, 2, 3], [0.2, 0.0, 0.05, 0.1], ROUND_EDGES),
            ([3, 2], [0.15, 0.02], [0.00051])]
    return Case("round_edges", ["p", "q", "r", "s"], [pair_append(docs)],
                notes={"zero_single": "q"})


def _shared_pairs():
    """(a, b) in 40 documents with three values and many ties, (b, a) in 15 others."""
    rng = np.random.default_rng(31)
    vals = [1.0, 2.0, 3.0]
    docs = []
    for d in range(55):  # of every 11 documents 8 hold (a, b) and 3 hold (b, a)
        ab = d % 11 not in (2, 5, 8)
        docs.append(([0, 1] if ab else [1, 0], _raw(rng, 2), [vals[(d * 7) % 3]]))
    return Case("shared_pairs", ["a", "b"], [pair_append(docs)], notes={"ab": 40, "ba": 15})


def _tile_edges(total):
    """Exactly `total` pairs kept: every pair of a T = 91 document (4095, the flat pair
    indices of one tile but one) and total - 4095 of a T = 92 document, whose pairs start
    at flat index 4095 and so straddle the tile boundary; its other pairs are 0.0."""
    rng = np.random.default_rng(total)
    d0 = _rand_doc(rng, np.arange(92), 91)
    d1 = _rand_doc(rng, np.arange(92), 92)
    pair1 = np.zeros(n_comb(92), np.float32)
    extra = total - n_comb(91)
    pair1[:extra] = d1[2][:extra]  # flat indices 4095 (tile 0), 4096 (tile 1)
    return Case(f"tile_edges_{total}", _words(92), [pair_append([d0, (d1[0], d1[1], pair1)])],
                notes={"kept_pairs": total})


def _max_from_pair():
    rng = np.random.default_rng(33)
    km = find_max_254()
    docs = [_rand_doc(rng, np.arange(12), 4, 100, km) for _ in range(10)]
    docs[4][2][2] = np.float32(km / 1000.0)
    docs[8][2][0] = np.float32(km / 1000.0)
    return Case("max_from_pair", _words(12), [pair_append(docs)], notes={"k_max": km})


def _quantized_to_zero():
    """Maximum 2.0: a score below 0.008 quantizes to 0.  (g, h) only ever scores 0.003 and
    0.005, so the term g|h is not in the vocabulary; (e, f) loses one posting of two."""
    docs = [([0, 1], [2.0, 1.0], [0.5]),
            ([2, 3], [0.7, 0.9], [0.003]),
            ([2, 3, 0], [0.6, 0.4, 0.3], [0.005, 0.8, 0.004]),
            ([0, 1], [1.1, 0.2], [0.006])]
    return Case("quantized_to_zero", ["e", "f", "g", "h"], [pair_append(docs)],
                notes={"gone": "g|h"})


def _wide_ids():
    rng = np.random.default_rng(35)
    docs = [_rand_doc(rng, np.arange(600), 92) for _ in range(20)]
    return Case("wide_ids", _words(600), [pair_append(docs)])


def _name_order():
    """'|' is 0x7C: 'az' < 'a|...' < 'a~' < 'a▁' in bytes, so pair names fall between
    single terms."""
    terms = ["a", "a|", "az", "a~", "a▁", "日本", "b", "{", "é"]
    rng = np.random.default_rng(36)
    docs = [_rand_doc(rng, np.arange(len(terms)), t) for t in (9, 5, 7, 9, 3)]
    return Case("name_order", terms, [pair_append(docs)])


def _split_docs():
    rng = np.random.default_rng(37)
    return [_rand_doc(rng, np.arange(40), int(t)) for t in rng.integers(1, 9, size=30)]


def _split_appends(cuts):
    docs = _split_docs()
    bounds = [0] + list(cuts) + [len(docs)]
    return Case(f"split_appends_{len(bounds) - 1}", _words(40),
                [pair_append(docs[a:b]) for a, b in zip(bounds[:-1], bounds[1:])])


def _mixed():
    rng = np.random.default_rng(38)
    s0 = single_append([(rng.choice(30, 4, replace=False), rng.integers(100, 4000, 4))
                        for _ in range(5)])
    p = pair_append([_rand_doc(rng, np.arange(30), int(t)) for t in (3, 1, 6, 2)])
    s1 = single_append([(rng.choice(30, 3, replace=False), rng.integers(100, 4000, 3))
                        for _ in range(3)])
    return Case("mixed", _words(30), [s0, p, s1])


def _small(name, seed=40, **kw):
    rng = np.random.default_rng(seed)
    docs = [_rand_doc(rng, np.arange(20), int(t)) for t in (3, 4, 2, 5, 3, 4)]
    return Case(name, _words(20), [pair_append(docs)], **kw)


def _cu_pairs_off():
    """The appends are right; the test appends a copy whose cu_pairs is off by one at
    document 2 first, which must change nothing."""
    return _small("cu_pairs_off", error="DI_EINVAL", stage="append", notes={"doc": 2})


def _bad_term_id():
    c = _small("bad_term_id", error="DI_EINVAL", stage="quantize")
    c.appends[0][1][6] = len(c.terms)
    return c


def _nan_pair():
    c = _small("nan_pair", error="DI_EFORMAT", stage="quantize")
    c.appends[0][3][5] = np.nan
    return c


def _empty_doc():
    rng = np.random.default_rng(41)
    docs = [_rand_doc(rng, np.arange(20), t) for t in (3, 2, 0, 4)]
    return Case("empty_doc", _words(20), [pair_append(docs)], error="DI_EFORMAT",
                stage="quantize", notes={"doc": 2})


def _collision_single(dropped):
    """The single term 'x|y' beside the pair ('x', 'y').  dropped: the pair's score rounds
    to 0.003 and quantizes to 0 under a maximum of 2.0, so nothing collides."""
    s = 0.003 if dropped else 0.8
    docs = [([0, 1, 2], [2.0, 1.0, 0.5], [s, 0.4, 0.6]), ([2, 0], [0.9, 0.7], [0.3])]
    kw = {} if dropped else dict(error="DI_EFORMAT", stage="rows")
    return Case("collision_dropped" if dropped else "collision_single", ["x", "y", "x|y"],
                [pair_append(docs)], notes={"name": "x|y"}, **kw)


def _collision_pair():
    docs = [([0, 1], [2.0, 1.0], [0.5]), ([2, 3], [0.9, 0.7], [0.3])]
    return Case("collision_pair", ["x|y", "z", "x", "y|z"], [pair_append(docs)],
                error="DI_EFORMAT", stage="rows", notes={"name": "x|y|z"})


_BUILDERS = {
    "tiny": _tiny,
    "round_edges": _round_edges,
    "shared_pairs": _shared_pairs,
    f"tile_edges_{T - 1}": lambda: _tile_edges(T - 1),
    f"tile_edges_{T}": lambda: _tile_edges(T),
    f"tile_edges_{T + 1}": lambda: _tile_edges(T + 1),
    "max_from_pair": _max_from_pair,
    "quantized_to_zero": _quantized_to_zero,
    "wide_ids": _wide_ids,
    "name_order": _name_order,
    "split_appends_1": lambda: _split_appends([]),
    "split_appends_3": lambda: _split_appends([1, 12]),
    "mixed": _mixed,
    "collision_dropped": lambda: _collision_single(True),
    # errors
    "cu_pairs_off": _cu_pairs_off,
    "bad_term_id": _bad_term_id,
    "nan_pair": _nan_pair,
    "empty_doc": _empty_doc,
    "collision_single": lambda: _collision_single(False),
    "collision_pair": _collision_pair,
}
CASE_NAMES = list(_BUILDERS)
ERROR_NAMES = ["cu_pairs_off", "bad_term_id", "nan_pair", "empty_doc", "collision_single",
               "collision_pair"]
OK_NAMES = [n for n in CASE_NAMES if n not in ERROR_NAMES]


@lru_cache(maxsize=None)
def case(name) -> Case:
    return _BUILDERS[name]()


def queries(e: Expected, n=6):
    """Queries over an expected vocabulary that mix single and 'a|b' terms."""
    pairs = [t for t in e.vocab if "|" in t]
    singles = [t for t in e.vocab if "|" not in t]
    out = []
    for i in range(n):
        q = singles[i::n][:3] + pairs[i::max(1, len(pairs) // 4)][:3]
        if q:
            out.append(q)
    return out
