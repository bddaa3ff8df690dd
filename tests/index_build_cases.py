"""Constructed inputs of the quantized index builder (di_term_table_*, di_index_builder_*)
and their expected answers.

A case is a list of term strings (term id = position, the order they are interned in), a
list of appends, each (term_ids uint32, impacts float32, cu_terms int32) as
di_index_builder_append takes them -- impacts in thousandths, the values DI_F_ROUND3
leaves -- and an optional max_val.  The expected answer is the text route's, computed by the
oracle's restatements: oracle.impact_line -> oracle.quantize_lines -> oracle.build_index ->
oracle.write_index.  No GPU is needed here; test_index_build_cases_cpu.py checks a numpy
restatement of the order against it and that every case reaches what it claims.
"""
import tempfile
from dataclasses import dataclass, field
from functools import lru_cache
from pathlib import Path
from typing import List, Optional, Tuple

import numpy as np

T = 4096  # DI_INDEX_BUILD_TILE: pairs / postings one workgroup counts and places


@dataclass
class Case:
    name: str
    terms: List[str]
    appends: List[Tuple[np.ndarray, np.ndarray, np.ndarray]]
    max_val: Optional[float] = None
    reserve: Optional[Tuple[int, int]] = None  # a (small) reserve before the first append
    error: Optional[str] = None   # the DIError code name the builder must raise ...
    stage: Optional[str] = None   # ... in "intern", "quantize" or "postings"
    queries: List[List[str]] = field(default_factory=list)
    notes: dict = field(default_factory=dict)

    def corpus(self):
        """The appends joined: (term_ids, impacts, cu_terms) of the whole collection."""
        tid = np.concatenate([a[0] for a in self.appends] or [np.zeros(0, np.uint32)])
        imp = np.concatenate([a[1] for a in self.appends] or [np.zeros(0, np.float32)])
        cu, base = [np.zeros(1, np.int64)], 0
        for a in self.appends:
            cu.append(a[2][1:].astype(np.int64) + base)
            base += int(a[2][-1])
        return tid.astype(np.uint32), imp.astype(np.float32), np.concatenate(cu)

    @property
    def n_docs(self):
        return sum(len(a[2]) - 1 for a in self.appends)

    def impact_lines(self):
        """The lines of the impact TSV (indexer.py:62-68)."""
        import oracle

        tid, imp, cu = self.corpus()
        names = [self.terms[t] for t in tid.tolist()]
        return [oracle.impact_line(names[a:b], imp[a:b])
                for a, b in zip(cu[:-1].tolist(), cu[1:].tolist())]


@dataclass
class Expected:
    max_used: float
    vocab: List[str]
    term_off: np.ndarray
    pdoc: np.ndarray
    pval: np.ndarray
    term_count: np.ndarray  # per term id
    term_row: np.ndarray    # per term id, -1: not in the vocab
    files: dict             # name -> bytes of oracle.write_index


@lru_cache(maxsize=None)
def expected(name) -> Expected:
    """The text route's answer for a case without an error, by the oracle."""
    import oracle

    c = case(name)
    assert c.error is None or c.stage == "postings"
    qlines, used = oracle.quantize_lines(c.impact_lines(), c.max_val)
    with tempfile.TemporaryDirectory() as tmp:
        q = Path(tmp) / "collection.quantized"
        q.write_text("".join(l + "\n" for l in qlines), encoding="utf-8")
        vocab, term_off, pdoc, pval = oracle.build_index(oracle.collection_items(q))
        oracle.write_index(Path(tmp) / "index", vocab, term_off, pdoc, pval)
        files = {p.name: p.read_bytes() for p in (Path(tmp) / "index").iterdir()}
    row_of = {t: r for r, t in enumerate(vocab)}
    term_row = np.array([row_of.get(t, -1) for t in c.terms], np.int32)
    counts = np.diff(term_off)
    term_count = np.where(term_row >= 0, counts[np.maximum(term_row, 0)] if len(vocab) else 0,
                          0).astype(np.int64)
    for a in (term_off, pdoc, pval, term_count, term_row):
        a.setflags(write=False)
    return Expected(used, vocab, term_off, pdoc, pval, term_count, term_row, files)


def numpy_order(c: Case, max_val=None):
    """The expected arrays restated in plain numpy: quantize in float64, drop the zeros,
    rows = sorted() of the kept strings, lexsort by (row, -val, doc)."""
    tid, imp, cu = c.corpus()
    doc = np.repeat(np.arange(len(cu) - 1, dtype=np.int64), np.diff(cu))
    v = imp.astype(np.float64)
    m = float(max_val) if max_val is not None else max(0.0, float(v.max(initial=0.0)))
    val = np.trunc(v * (255.0 / m)).astype(np.int64)
    keep = val > 0
    tid, doc, val = tid[keep].astype(np.int64), doc[keep], val[keep]
    term_count = np.bincount(tid, minlength=len(c.terms)).astype(np.int64)
    kept = sorted(c.terms[t] for t in np.flatnonzero(term_count).tolist())
    row_of = {t: r for r, t in enumerate(kept)}
    term_row = np.array([row_of[t] if n > 0 else -1 for t, n in zip(c.terms, term_count.tolist())],
                        np.int32)
    row = term_row[tid].astype(np.int64)
    order = np.lexsort((doc, -val, row))
    term_off = np.zeros(len(kept) + 1, np.int64)
    term_off[1:] = np.cumsum(np.bincount(row, minlength=len(kept)))
    return (m, kept, term_off, doc[order].astype(np.uint32), val[order], term_count, term_row)


def row_digits(n_rows):
    """8-bit digits of the largest row: the sort's passes on the row."""
    d, top = 0, n_rows - 1
    while top > 0:
        d, top = d + 1, top >> 8
    return d


# --------------------------------------------------------------------------- construction
def f32k(k):
    """Thousandths as float32: the values round(impact, 3) leaves."""
    return (np.asarray(k, np.float64) / 1000.0).astype(np.float32)


def _pack(n_docs, d, t, k):
    """Triplets (doc, term id, thousandths), distinct (doc, term), in the order given inside
    a document -> one append."""
    d, t = np.asarray(d, np.int64), np.asarray(t, np.int64)
    assert np.unique(d * (1 << 32) + t).size == d.size, "a (doc, term) pair twice"
    order = np.argsort(d, kind="stable")
    cu = np.zeros(n_docs + 1, np.int32)
    cu[1:] = np.cumsum(np.bincount(d, minlength=n_docs))
    return (t[order].astype(np.uint32), f32k(np.asarray(k)[order]), cu)


def _split(n_docs, d, t, k, bounds):
    """One collection cut into appends at the document numbers `bounds`."""
    d, t, k = np.asarray(d, np.int64), np.asarray(t, np.int64), np.asarray(k)
    out, lo = [], 0
    for hi in list(bounds) + [n_docs]:
        m = (d >= lo) & (d < hi)
        out.append(_pack(hi - lo, d[m] - lo, t[m], k[m]))
        lo = hi
    return out


def _random(rng, n_docs, term_ids, per_doc, k_lo=100, k_hi=4000):
    """`per_doc` distinct terms of `term_ids` for every document, in no particular order,
    thousandths in [k_lo, k_hi)."""
    term_ids = np.asarray(term_ids, np.int64)
    d = np.repeat(np.arange(n_docs, dtype=np.int64), per_doc)
    t = np.concatenate([rng.choice(term_ids, size=per_doc, replace=False)
                        for _ in range(n_docs)]) if n_docs else np.zeros(0, np.int64)
    return d, t, rng.integers(k_lo, k_hi, size=d.size)


def _join(*parts):
    return tuple(np.concatenate([np.asarray(p[i], np.int64) for p in parts]) for i in range(3))


def _words(n, prefix="w"):
    return [f"{prefix}{i:04d}" for i in range(n)]


def _ties_long():
    """Term 0 in every one of 65 537 documents (docs >= 65 536, a run of 17 tiles), its
    values cycling over three classes, so equal (row, value) keys cross every tile
    boundary; 40 more terms in two documents each."""
    rng = np.random.default_rng(3)
    n_docs = 65537
    d0 = np.arange(n_docs, dtype=np.int64)
    k0 = np.array([1000, 2000, 3000])[d0 % 3]
    rare_d = rng.choice(n_docs, size=80, replace=False)
    rare_t = np.repeat(np.arange(1, 41), 2)
    rare_k = rng.integers(200, 3000, size=80)
    d, t, k = _join((d0, np.zeros(n_docs, np.int64), k0), (rare_d, rare_t, rare_k))
    terms = ["common"] + _words(40, "rare")
    return Case("ties_long", terms, [_pack(n_docs, d, t, k)],
                queries=[["common"], ["common", "rare0003"], ["rare0007", "common", "rare0020"],
                         ["rare0001", "rare0002"]],
                notes={"n_docs": n_docs, "classes": 3})


def _tile_edges(total):
    """Exactly `total` kept postings (and a few dropped ones between them)."""
    rng = np.random.default_rng(total)
    per = 5
    n_docs = total // per
    d, t, k = _random(rng, n_docs, np.arange(60), per)
    rest = total - n_docs * per  # one more document with the remainder
    if rest:
        d = np.concatenate([d, np.full(rest, n_docs)])
        t = np.concatenate([t, np.arange(rest)])
        k = np.concatenate([k, rng.integers(100, 4000, size=rest)])
        n_docs += 1
    k[0] = 4000  # the maximum: every k >= 100 keeps a value >= 6
    # dropped pairs (value 0) on term 60, every 7th document
    dz = np.arange(0, n_docs, 7)
    d, t, k = _join((d, t, k), (dz, np.full(dz.size, 60), np.ones(dz.size)))
    return Case(f"tile_edges_{total}", _words(61), [_pack(n_docs, d, t, k)],
                notes={"kept": total})


def _tile_owner():
    """The first T kept postings are one term with one value: in the value pass and in the
    row pass one digit owns the whole first tile; then a mixed tail into a third tile."""
    rng = np.random.default_rng(9)
    n_docs = T + 400
    d0 = np.arange(T, dtype=np.int64)
    d1, t1, k1 = _random(rng, 400, np.arange(1, 50), 11)
    d, t, k = _join((d0, np.zeros(T), np.full(T, 2500)), (d1 + T, t1, k1))
    k[-1] = 4000
    return Case("tile_owner", _words(50), [_pack(n_docs, d, t, k)], notes={"kept": T + 4400})


def _all_values():
    """Term 0 with every value 1..255 (maximum 255.0: the scale is 1) and some zeros, three
    documents a value, documents in an order unrelated to the value."""
    rng = np.random.default_rng(4)
    vals = np.concatenate([np.repeat(np.arange(1, 256), 3), np.zeros(20, np.int64)])
    n_docs = vals.size
    perm = rng.permutation(n_docs)
    k0 = vals[perm] * 1000 + np.where(vals[perm] == 0, 3, 0)  # zeros as 0.003
    d1, t1, k1 = _random(rng, n_docs, np.arange(1, 9), 2, 500, 200000)
    d, t, k = _join((np.arange(n_docs), np.zeros(n_docs), k0), (d1, t1, k1))
    return Case("all_values", _words(9), [_pack(n_docs, d, t, k)])


def find_max_254():
    """The smallest maximum m (thousandths, from 1.000 up) with
    int(float(m) * (255 / float(m))) == 254: the top value of a collection need not be 255."""
    for k in range(1000, 200000):
        m = float(np.float32(k / 1000.0))
        if int(m * (255.0 / m)) == 254:
            return k
    raise AssertionError("no such maximum")


def _max_254():
    rng = np.random.default_rng(6)
    km = find_max_254()
    d, t, k = _random(rng, 30, np.arange(1, 12), 4, 100, km)
    d, t, k = _join((d, t, k), ([0, 7, 29], [0, 0, 0], [km, km // 2, km]))
    return Case("max_254", _words(12), [_pack(30, d, t, k)], notes={"k_max": km})


def _dropped():
    """Postings that quantize to 0 (maximum 2.0: below 0.008); 'gone' loses all its postings
    and is absent from the vocab; document 2 loses all its postings; 'relu' has impact 0.0."""
    terms = ["keep", "some", "gone", "relu", "late"]
    docs = [[(0, 2000), (1, 1)], [(2, 3), (0, 1000)], [(2, 1), (1, 2)], [(3, 0), (0, 500)],
            [(1, 1500), (2, 7)], [(4, 8), (3, 0)]]
    d = [i for i, x in enumerate(docs) for _ in x]
    t = [p[0] for x in docs for p in x]
    k = [p[1] for x in docs for p in x]
    return Case("dropped", terms, [_pack(len(docs), d, t, k)],
                notes={"gone": "gone", "empty_after": 2})


def _many_terms():
    """70 001 term ids, 66 000 of them with one kept posting each (three row digits), the
    others never used; id i is the string w<(i * 7919) % 70001>, far from sorted order."""
    rng = np.random.default_rng(12)
    n_terms, used, per = 70001, 66000, 60
    terms = [f"w{(i * 7919) % n_terms:05d}" for i in range(n_terms)]
    ids = rng.permutation(n_terms)[:used]
    n_docs = used // per
    d = np.repeat(np.arange(n_docs, dtype=np.int64), per)
    k = rng.integers(100, 4000, size=used)
    k[5] = 4000
    return Case("many_terms", terms, [_pack(n_docs, d, ids, k)], notes={"kept_terms": used})


def _utf8_terms():
    terms = ["▁hello", "▁hell", "▁", "naïve", "日本語", "a,b", "a:b", "x|y", "é", "e", "z",
             "Ω:,|", "▁日本", "\U0001F600", "~"]
    rng = np.random.default_rng(15)
    d, t, k = _random(rng, 40, np.arange(len(terms)), 6)
    return Case("utf8_terms", terms, [_pack(40, d, t, k)],
                notes={"prefix": ("▁hell", "▁hello")})


def _split_appends():
    """Appends of 0, 1 and many documents, past a reserve of 4 pairs."""
    rng = np.random.default_rng(17)
    n_docs = 3000
    d, t, k = _random(rng, n_docs, np.arange(200), 5)
    none = (np.zeros(0, np.uint32), np.zeros(0, np.float32), np.zeros(1, np.int32))
    a = _split(n_docs, d, t, k, [1, 51])
    return Case("split_appends", _words(200), [none, a[0], a[1], none, a[2]], reserve=(1, 4),
                notes={"sizes": [0, 1, 50, 0, 2949]})


def _small(name, seed=20, **kw):
    rng = np.random.default_rng(seed)
    d, t, k = _random(rng, 50, np.arange(30), 4)
    k[3] = 4000
    return Case(name, _words(30), [_pack(50, d, t, k)], **kw)


def _empty_doc():
    rng = np.random.default_rng(22)
    d, t, k = _random(rng, 20, np.arange(10), 3)
    m = d != 11
    return Case("empty_doc", _words(10), [_pack(20, d[m], t[m], k[m])], error="DI_EFORMAT",
                stage="quantize", notes={"doc": 11})


def _all_zero():
    d, t, k = _random(np.random.default_rng(23), 10, np.arange(6), 2, 0, 1)
    return Case("all_zero", _words(6), [_pack(10, d, t, k)], error="DI_EINVAL", stage="quantize")


def _bad_term_id():
    c = _small("bad_term_id", error="DI_EINVAL", stage="quantize")
    c.appends[0][0][17] = len(c.terms)
    return c


_BUILDERS = {
    "ties_long": _ties_long,
    f"tile_edges_{T - 1}": lambda: _tile_edges(T - 1),
    f"tile_edges_{T}": lambda: _tile_edges(T),
    f"tile_edges_{T + 1}": lambda: _tile_edges(T + 1),
    "tile_owner": _tile_owner,
    "all_values": _all_values,
    "max_254": _max_254,
    "dropped": _dropped,
    "many_terms": _many_terms,
    "utf8_terms": _utf8_terms,
    "split_appends": _split_appends,
    "max_val_above": lambda: _small("max_val_above", max_val=9.5),
    # errors
    "max_val_below": lambda: _small("max_val_below", max_val=2.0, error="DI_ERANGE",
                                    stage="quantize"),
    "empty_doc": _empty_doc,
    "all_zero": _all_zero,
    "bad_term": lambda: _small("bad_term", error="DI_EFORMAT", stage="intern"),
    "bad_term_id": _bad_term_id,
    "unassigned_row": lambda: _small("unassigned_row", error="DI_EINVAL", stage="postings"),
}
CASE_NAMES = list(_BUILDERS)
OK_NAMES = [n for n in CASE_NAMES if n in (
    "ties_long", f"tile_edges_{T - 1}", f"tile_edges_{T}", f"tile_edges_{T + 1}", "tile_owner",
    "all_values", "max_254", "dropped", "many_terms", "utf8_terms", "split_appends",
    "max_val_above")]
ERROR_NAMES = [n for n in CASE_NAMES if n not in OK_NAMES]


@lru_cache(maxsize=None)
def case(name) -> Case:
    c = _BUILDERS[name]()
    if name == "bad_term":
        c.terms[5] = "two, words"
    return c
