"""Shared inputs of tests/test_scorer_cases_cpu.py and tests/test_scorer_edges_gpu.py (not a
test module): constructed collections and queries for the quantized-index scorer
(score_blocks_kernel / score_long_kernel / item_setup_kernel of csrc/index_score.hip), the numpy
definition of its accumulator words and of the exact top-k, and a restatement of which
selection route and which scatter rounds a (query, block) item takes, so that the CPU test
can prove that the GPU cases between them reach every route and every round shape.

Nothing here draws a random number where a count matters: every sublist length, tie count
and score is placed."""
import functools

import numpy as np

# csrc/index_score.h / index_score.hip: the constants the scorer branches on
MAX_BLOCK_DOCS = 32768        # docs per block (one workgroup's LDS accumulators)
SC_THREADS = 1024             # threads per workgroup; all-wave rounds are multiples of it
WSEG = 16                     # wave segments per block (SC_THREADS / 64)
WLONG_MIN = 128               # sublists from this many postings get the per-wave layout
WTERMS = 64                   # queries up to this many terms: the per-wave form
FAST_TERMS = 16               # ... up to this many: the score-histogram selection
HIST_BINS = 4096              # bins of that histogram
TIE_CAP = HIST_BINS           # ties at the k-th score the fast path lists; more: radix
QH_BINS = 4096                # the shared per-query histogram; the last bin saturates
LH_DOCS = 16384               # long queries: docs per half block
DI_SHORT_QUERY_TERMS = 256    # compact word / compact key up to this many terms
DI_MAX_QUERY_TERMS = 4096     # more: the query is rejected (out_n = -1)
AUTO_THRESHOLD_BLOCKS = 8     # di_index::shared_thr = -1: the shared histogram from 8 blocks
TQ_EVERY, TQ_FIRST = 8, 4     # refresh schedule: blocks b < 4 and b % 8 == 0 read the histogram

U64 = np.uint64


def few_blocks(nb, k, shared_thr=-1):
    """di_index::few_blocks: the emit-above selection (list capacity 2 k) of shards of
    2..7 blocks, unless DI_SCORE_THRESHOLD=1 forces the shared histogram."""
    return 2 <= nb < 8 and shared_thr != 1 and 2 * k <= 2048


def shared_threshold(nb, shared_thr=-1):
    """di_index_search's `thr`: the per-query histogram (qhist) is in use."""
    return nb > 1 and (nb >= AUTO_THRESHOLD_BLOCKS if shared_thr < 0 else shared_thr == 1)


def reads_histogram(b, every=TQ_EVERY, first=TQ_FIRST):
    """score_item's qpre under the schedule: this block's items copy the histogram; the
    others take the running word."""
    return every <= 1 or b < first or b % every == 0


def layout(n_docs):
    """build_index: (nb, block_docs, wave_seg) of a shard of n_docs docs."""
    nb = -(-n_docs // MAX_BLOCK_DOCS)
    if nb == 0:
        return 0, MAX_BLOCK_DOCS, MAX_BLOCK_DOCS // WSEG
    bd = min(MAX_BLOCK_DOCS, -(-(-(-n_docs // nb)) // 64) * 64)
    return nb, bd, -(-bd // WSEG)


def tail_fits(n_local, k):
    """score_item: 2 k words of staging fit behind the block's accumulators."""
    return 2 * k <= MAX_BLOCK_DOCS - 4 * (-(-n_local // 4))


def hist_fits(k):
    """... or, for a one-sweep selection, k keys fit in the histogram area."""
    return 8 * k <= 4 * HIST_BINS


# ---------------------------------------------------------------------------------------
# collections
# ---------------------------------------------------------------------------------------
class Coll:
    """A shard [doc_lo, doc_lo + n_docs) given by explicit posting lists (local doc ids)."""

    def __init__(self, n_docs, doc_lo=0):
        self.n_docs, self.doc_lo = int(n_docs), int(doc_lo)
        self.terms = []
        self.nb, self.block_docs, self.wave_seg = layout(self.n_docs)

    def term(self, docs, vals):
        docs = np.asarray(docs, np.int64).reshape(-1)
        vals = np.broadcast_to(np.asarray(vals, np.int64), docs.shape).copy()
        assert np.unique(docs).size == docs.size, "a doc occurs once per term"
        assert docs.size == 0 or (0 <= docs.min() and docs.max() < self.n_docs)
        assert vals.size == 0 or (1 <= vals.min() and vals.max() <= 255)
        order = np.lexsort((docs, -vals))  # the reference file order: value desc, doc asc
        self.terms.append((docs[order], vals[order]))
        return len(self.terms) - 1

    def arrays(self):
        """(term_off int64, pdoc uint32 (global ids), pval uint8)."""
        off = np.zeros(len(self.terms) + 1, np.int64)
        off[1:] = np.cumsum([d.size for d, _ in self.terms])
        pdoc = np.concatenate([d for d, _ in self.terms] + [np.zeros(0, np.int64)])
        pval = np.concatenate([v for _, v in self.terms] + [np.zeros(0, np.int64)])
        return off, (pdoc + self.doc_lo).astype(np.uint32), pval.astype(np.uint8)

    def sublist_len(self, t, b):
        d = self.terms[t][0]
        return int(((d // self.block_docs) == b).sum())

    def run_lengths(self, t, b):
        """Postings of term t in each wave segment of block b (build pass 3)."""
        d = self.terms[t][0]
        d = d[(d // self.block_docs) == b] % self.block_docs
        return np.bincount(np.minimum(d // self.wave_seg, WSEG - 1), minlength=WSEG).tolist()

    def n_local(self, b):
        return min(self.block_docs, self.n_docs - b * self.block_docs)


def accumulate(coll, query, drop=None, min_value=1):
    """(score, first-touch term, value there) per local doc; first = -1: untouched.
    drop = (term, local doc): that posting is left out; min_value: impact pruning."""
    n = coll.n_docs
    sc, first, v0 = np.zeros(n, np.int64), np.full(n, -1, np.int64), np.zeros(n, np.int64)
    for j, t in enumerate(query):
        d, v = coll.terms[t]
        keep = v >= min_value
        if drop is not None and drop[0] == t:
            keep = keep & (d != drop[1])
        d, v = d[keep], v[keep]
        new = first[d] < 0
        first[d[new]] = j
        v0[d[new]] = v[new]
        sc[d] += v
    return sc, first, v0


def words_of(sc, first, v0, nt):
    """The accumulator words: score << 16 | (255 - j) << 8 | v_j, or for more than 256
    query terms the 40-bit word score << 20 | (4095 - j) << 8 | v_j; 0: untouched."""
    if nt > DI_SHORT_QUERY_TERMS:
        w = (sc << 20) | ((4095 - first) << 8) | v0
    else:
        assert sc.max(initial=0) < 65536
        w = (sc << 16) | ((255 - first) << 8) | v0
    return np.where(first >= 0, w, 0)


def all_block_words(coll, query, **kw):
    """block_words of every block, from one accumulation."""
    w = words_of(*accumulate(coll, query, **kw), len(query))
    return [w[b * coll.block_docs:b * coll.block_docs + coll.n_local(b)] for b in range(coll.nb)]


def block_words(coll, query, b, **kw):
    """The words of block b (n_local of them) for this query."""
    w = words_of(*accumulate(coll, query, **kw), len(query))
    return w[b * coll.block_docs:b * coll.block_docs + coll.n_local(b)]


def ranked_keys(coll, query, tie="first_touch", drop=None, min_value=1):
    """Every touched doc as its merge key, best first: word << 32 | ~doc (compact) or
    word << 24 | ~doc24 (more than 256 terms), doc global.  tie = "doc" ranks equal scores
    by doc alone (a mutation of the CPU test); drop leaves one posting out."""
    nt = len(query)
    sc, first, v0 = accumulate(coll, query, drop=drop, min_value=min_value)
    w = words_of(sc, first, v0, nt)
    idx = np.nonzero(w)[0]
    g = (idx + coll.doc_lo).astype(U64)
    if nt > DI_SHORT_QUERY_TERMS:
        keys = (w[idx].astype(U64) << U64(24)) | (U64(0xFFFFFF) - g)
    else:
        keys = (w[idx].astype(U64) << U64(32)) | (U64(0xFFFFFFFF) - g)
    order = np.lexsort((g, -sc[idx])) if tie == "doc" else np.argsort(keys)[::-1]
    return keys[order]


def cut_at(ranked, k, off_by_one=False):
    """The first k keys; off_by_one (a mutation): the k-th entry replaced by the k+1-th,
    or dropped where there is none."""
    if off_by_one:
        return np.concatenate([ranked[:k - 1], ranked[k:k + 1]])
    return ranked[:k]


def reference_topk(coll, query, k, **kw):
    """The exact top-k of the shard as merge keys, descending."""
    return cut_at(ranked_keys(coll, query, **kw), k)


# ---------------------------------------------------------------------------------------
# routes
# ---------------------------------------------------------------------------------------
SHORT_ROUTES = (
    "empty",
    "fast/all_touched",                    # total <= k
    "fast/all_ties",                       # ties == need
    "fast/ties_wave",                      # <= 64 ties ranked by one wave
    "fast/ties_radix",                     # 65..TIE_CAP ties: radix over the tie list
    "fast/ties_overflow>radix/no_cut",     # > TIE_CAP ties: the general path from shift 8
    "fast/ties_overflow>radix/doc_cut",
    "radix/all_touched",                   # > 16 terms, rs.total <= k
    "radix/no_cut",
    "radix/doc_cut",                       # doc-order radix among equal words
)
LONG_ROUTES = ("long/empty", "long/all", "long/select", "long/all+held", "long/select+held")


def _word_cut(w, need):
    """general path: the need-th largest word, then doc order among its equals or not."""
    s = np.sort(w)[::-1]
    t = s[need - 1]
    return "no_cut" if int((s == t).sum()) == need - int((s > t).sum()) else "doc_cut"


def expected_route(words, nt, k):
    """The selection route of a score_item that runs the full selection (no threshold
    read, a threshold of 0, or a sweep that overflowed), nt <= 256 terms."""
    assert nt <= DI_SHORT_QUERY_TERMS
    w = words[words != 0]
    if w.size == 0:
        return "empty"
    if nt > FAST_TERMS:
        return "radix/all_touched" if w.size <= k else "radix/" + _word_cut(w, k)
    if w.size <= k:
        return "fast/all_touched"
    s = np.sort(w >> 16)[::-1]
    t = s[k - 1]
    ties, need = int((s == t).sum()), k - int((s > t).sum())
    if ties == need:
        return "fast/all_ties"
    if ties <= 64:
        return "fast/ties_wave"
    if ties <= TIE_CAP:
        return "fast/ties_radix"
    return "fast/ties_overflow>radix/" + _word_cut(w[(w >> 16) == t], need)


def expected_long_routes(words, k):
    """score_long_item, per half block: every key is a candidate (total <= k) or the radix
    selects, and whether the first half's keys are held for the second selection."""
    out, held = [], 0
    for hb in range(0, len(words), LH_DOCS):
        total = int((words[hb:hb + LH_DOCS] != 0).sum()) + held
        r = "long/empty" if total == 0 else "long/all" if total <= k else "long/select"
        out.append(r + ("+held" if held else ""))
        held = min(total, k)
    return out


THRESHOLD_ROUTES = ("T=0>full", "sweep_emits", "sweep_overflows>full")


def threshold_route(words, T, cap):
    """An item that reads the threshold T: cap = k for the shared histogram, 2 k for the
    emit-above selection of few blocks."""
    if T == 0:
        return "T=0>full"
    n = int(((words >> 16) >= T).sum())
    return "sweep_emits" if n <= cap else "sweep_overflows>full"


def kth_score(words, k):
    """The k-th largest score of a block (what its full selection publishes), or None when
    fewer than k docs are touched (it publishes nothing)."""
    s = np.sort(words[words != 0] >> 16)[::-1]
    return int(s[k - 1]) if s.size >= k else None


def admissible_thresholds(blocks_words, b, k, saturate=None):
    """Every nonzero T that blocks 0..b-1 can have published when block b starts: [lo, hi]
    (None: none).  A published value is a k-th score of counted candidates, each an emitted
    doc of an earlier block with its full score: at most the k-th largest score of the
    earlier blocks' union (hi), at least the smallest score any of them can emit (lo: its
    own k-th score, or its smallest when it holds fewer than k docs; by induction a block
    that swept against an earlier T emits nothing below that T).  The histogram may be read
    with any part of the counts still in flight: every value between is possible.
    saturate: QH_BINS - 1 for the shared histogram (its last bin counts that and above)."""
    if b == 0:
        return None
    earlier = np.concatenate([w[w != 0] >> 16 for w in blocks_words[:b]])
    if earlier.size < k:
        return None
    hi = int(np.sort(earlier)[::-1][k - 1])
    lo = hi
    for w in blocks_words[:b]:
        s = w[w != 0] >> 16
        if s.size:
            kth = kth_score(w, k)
            lo = min(lo, kth if kth is not None else int(s.min()))
    if saturate is not None:
        lo, hi = min(lo, saturate), min(hi, saturate)
    return lo, hi


# ---------------------------------------------------------------------------------------
# scatter rounds
# ---------------------------------------------------------------------------------------
def _wave_rounds(n):
    out, rem = [], n
    while rem > 0:
        if rem > 8 * 64:
            out.append("16x64")
            rem -= 16 * 64
        else:
            out.append("8x64" if rem > 4 * 64 else "4x64" if rem > 64 else "1x64")
            rem = 0
    return out


def scatter_rounds(lengths, form):
    """The rounds score_item's scatter takes.
    form "wave_run": lengths = one long term's run per wave segment -> a list of round
    shapes per run.  form "wave_short": lengths = [the sublist's length], read whole by
    every wave -> the same.  form "all_wave": lengths = the sublist lengths of the query's
    terms in query order -> per term a list of (shape, rem, prefetch): rem as the loop saw
    it ("pre4x1024": the postings the previous term's last round loaded ahead), prefetch:
    this round also loads the next term's first 4096."""
    if form in ("wave_run", "wave_short"):
        return [_wave_rounds(n) for n in lengths]
    assert form == "all_wave"
    out, have_pre = [], False
    for j, n in enumerate(lengths):
        rounds, pos = [], 0
        if have_pre:
            rounds.append(("pre4x1024", n, False))
            pos, have_pre = min(n, 4 * SC_THREADS), False
        nxt = j + 1 < len(lengths) and lengths[j + 1] > 0
        while pos < n:
            rem = n - pos
            if rem >= 16 * SC_THREADS:
                pf = nxt and rem == 16 * SC_THREADS
                rounds.append(("16x1024", rem, pf))
                pos += 16 * SC_THREADS
            elif rem > SC_THREADS:
                pf = nxt and rem <= 4 * SC_THREADS
                rounds.append(("4x1024", rem, pf))
                pos += 4 * SC_THREADS
            else:
                pf = nxt
                rounds.append(("1x1024", rem, pf))
                pos = n
            have_pre = have_pre or pf
        out.append(rounds)
    return out


def scattered_postings(coll, query, b, min_value=1):
    """Postings an item scatters under impact pruning (values >= min_value): the count
    the EXT_BM instantiation compares with k (at most k: every touched doc is a candidate,
    one append sweep), for queries of at most FAST_TERMS terms."""
    n = 0
    for t in query:
        d, v = coll.terms[t]
        n += int((((d // coll.block_docs) == b) & (v >= min_value)).sum())
    return n


def query_form(nt):
    if nt > DI_MAX_QUERY_TERMS:
        return "rejected"
    return "wave" if nt <= WTERMS else "all_wave" if nt <= DI_SHORT_QUERY_TERMS else "long"


# ---------------------------------------------------------------------------------------
# cases
# ---------------------------------------------------------------------------------------
class Case:
    """name, group, the collection, the queries, the k values it runs at, the boundary
    postings [(term, local doc)] whose loss must show, and for threshold cases the route
    designed for the blocks after the first."""

    def __init__(self, name, group, coll, queries, ks, boundary=(), designed=None, note=""):
        self.name, self.group, self.coll = name, group, coll
        self.queries, self.ks = [list(q) for q in queries], tuple(ks)
        self.boundary, self.designed, self.note = list(boundary), designed, note

    def inputs(self, k=None):
        """(term_off, pdoc, pval, n_docs, queries, k, note); n_docs counts from doc 0."""
        off, pdoc, pval = self.coll.arrays()
        return (off, pdoc, pval, self.coll.doc_lo + self.coll.n_docs, self.queries,
                self.ks[0] if k is None else k, self.note)


def _spread(n, count, off=0, step=37):
    """count distinct docs spread over [0, n): multiples of a step coprime to n (the next
    odd number that is, from the one given)."""
    assert count <= n and step % 2 == 1
    while np.gcd(step, n) != 1:
        step += 2
    return (off + step * np.arange(count, dtype=np.int64)) % n


@functools.lru_cache(maxsize=None)
def selection_cases(n):
    """One block of n docs (the plain kernel, no threshold: every route a pure function of
    the data), k = 1000 unless the case says otherwise.  One collection holds the terms of
    every case, so that one device-pointer call can batch them."""
    c = Coll(n)
    cases = []

    def add(name, queries, ks=(1000,), boundary=(), note=""):
        cases.append(Case(f"sel{n}/{name}", "selection", c, queries, ks, boundary, note=note))

    # equal scores 7 that arise as 7 via term 0 (word low bits (255, 7)), as 3 + 4 ((255, 3))
    # and as 7 via term 1 ((254, 7)): rank order G7a > G34 > G7b whatever their docs; the
    # groups' docs descend (G7b lowest), so doc order alone ranks them the other way round.
    def tie_groups(n7a, n34, n7b, n_above, off):
        ids = _spread(n, n7a + n34 + n7b + n_above, off)
        g7b, g34, g7a, above = np.split(np.sort(ids), np.cumsum([n7b, n34, n7a]))
        t0 = c.term(np.concatenate([g7a, g34]), np.concatenate([np.full(n7a, 7), np.full(n34, 3)]))
        t1 = c.term(np.concatenate([g34, g7b]), np.concatenate([np.full(n34, 4), np.full(n7b, 7)]))
        t2 = c.term(above, 20 + np.arange(n_above) % 200)
        return [t0, t1, t2], (t0, int(g34[0]))

    # ties == need: 600 docs above, 400 tied, all taken
    q, bd = tie_groups(100, 200, 100, 600, 1)
    add("ties_equal_need", [q], boundary=[bd], note="fast/all_ties")
    # <= 64 ties, the cut inside the 3 + 4 group
    q, bd = tie_groups(20, 20, 20, 970, 3)
    add("ties_jv_60", [q, q[:2], [q[1], q[0], q[2]]], ks=(1000, 30), boundary=[bd],
        note="fast/ties_wave; two terms at k = 30: the 60 tied docs alone")
    q, bd = tie_groups(20, 24, 20, 970, 5)
    add("ties_64", [q], boundary=[bd], note="fast/ties_wave at its limit")
    q, bd = tie_groups(20, 25, 20, 970, 7)
    add("ties_65", [q], boundary=[bd], note="fast/ties_radix, its first size")
    q, bd = tie_groups(50, 4000, 46, 900, 9)
    add("ties_4096", [q], boundary=[bd], note="fast/ties_radix at TIE_CAP")
    q, bd = tie_groups(50, 4000, 47, 900, 11)
    add("ties_4097", [q], boundary=[bd], note="> TIE_CAP: general path from shift 8, doc cut")
    # 900 above, 5000 docs tied on one word: the doc-order radix over > 256 equal words
    ids = np.sort(_spread(n, 5900, 13))
    ta = c.term(ids[5000:], 9)
    tb = c.term(ids[:5000], 7)
    add("900_above_5000_tied", [[ta, tb], [tb, ta]], boundary=[(tb, int(ids[99]))],
        note="> TIE_CAP ties, doc cut at rank 100 of the tied docs")
    # ... and 100 of the 5000 tied docs first touched by an earlier term: no doc cut
    t7a = c.term(ids[4900:5000], 7)
    t7b = c.term(ids[:4900], 7)
    add("5000_tied_cut_between_words", [[t7a, t7b, ta]], boundary=[(t7a, int(ids[4900]))],
        note="> TIE_CAP ties, the cut falls between two words")
    # a term in every doc with one value: the answer is docs 0..k-1
    tall = c.term(np.arange(n), 1)
    add("one_value_everywhere", [[tall]], ks=(1000, 1, 4096), boundary=[(tall, 0), (tall, 999)],
        note="> TIE_CAP ties; docs 0..999")
    # every touched doc: total <= k, and total == k
    t700 = c.term(_spread(n, 700, 17), 1 + np.arange(700) % 255)
    t1000 = c.term(_spread(n, 1000, 19), 1 + np.arange(1000) % 3)
    add("all_touched", [[t700], [t1000]], boundary=[(t700, int(_spread(n, 700, 17)[-1]))],
        note="fast/all_touched at 700 and at exactly k docs")
    tnone, tnone2 = c.term([], []), c.term([], [])
    add("empty", [[tnone], [tnone, tnone2]], note="no posting in the block")
    # 17-term queries: the block-wide radix; 15 filler terms of one posting each
    fill = [c.term([int(d)], 1 + i) for i, d in enumerate(_spread(n, 15, 23, step=1201))]
    ids = _spread(n, 1500, 29)
    i = np.arange(1500)
    ra = c.term(ids, 1 + i % 50)   # (score, first value) = (a + b, a): all words distinct
    rb = c.term(ids, 1 + i // 50)
    add("radix_distinct_words", [[ra, rb] + fill, fill + [rb, ra]],
        boundary=[(ra, int(ids[1499])), (rb, int(ids[1449]))], note="radix/no_cut")
    r800 = c.term(_spread(n, 800, 31), 1 + np.arange(800) % 255)
    add("radix_all_touched", [[r800] + fill, fill[:8] + [r800] + fill[8:]],
        boundary=[(r800, int(_spread(n, 800, 31)[5]))], note="radix/all_touched")
    ids = np.sort(_spread(n, 1300, 37, step=3))  # 1300 docs over 3900 doc ids
    rhi = c.term(ids[:850], 200)
    rlo = c.term(ids[850:], 100)  # 450 docs share one word; the cut takes 150 of them, their
    add("radix_doc_cut", [[rhi, rlo] + fill],   # docs span more than 256 ids: both digits
        boundary=[(rlo, int(ids[850 + 149]))], note="radix/doc_cut inside 450 equal words")
    # k edges on a plain pattern
    tk = c.term(_spread(n, min(n, 9000), 41), 1 + (np.arange(min(n, 9000)) * 7) % 255)
    tk2 = c.term(_spread(n, 3000, 43), 1 + np.arange(3000) % 11)
    add("k_edges", [[tk, tk2], [tk2, tk]], ks=(1, 2048, 2049, 4096),
        boundary=[(tk, int(_spread(n, 9000, 41)[253]))], note="k = 1, 2048, 2049, 4096")
    return cases


@functools.lru_cache(maxsize=None)
def small_collection_cases():
    """n_docs 1, 2, 3, 5, 63, 64, 65, 32767, 32768 (n_local % 4 and % 64 nonzero) and both
    sides of tail_fits at k = 1000 (30768 / 30769 docs)."""
    cases = []
    for n in (1, 2, 3, 5, 63, 64, 65, 30768, 30769, 32767, 32768):
        c = Coll(n)
        d = np.arange(n)
        ta = c.term(d, 1 + d % 7)
        tb = c.term(d[1::2], 1 + d[1::2] % 5)
        tl = c.term([n - 1], 200)
        cases.append(Case(f"small/{n}", "k_edges", c, [[ta], [tb, ta], [tl, ta, tb]], (1, 1000),
                          boundary=[(ta, n - 1)], note=f"tail_fits(k=1000) = {tail_fits(n, 1000)}"))
    return cases


RUN_LENGTHS = (0, 1, 63, 64, 65, 255, 256, 257, 511, 512, 513, 1023, 1024, 1025, 2047, 2048)


def _stripes(c, docs, width=4000, val=255):
    """Boost terms over consecutive stripes of docs: with k = 4096 every doc of a stripe is
    in that query's top-k, so the loss of any one posting of the striped term shows."""
    docs = np.sort(np.asarray(docs))
    return [c.term(docs[s:s + width], val) for s in range(0, docs.size, width)]


def _values(docs):
    """1..255 by doc, both sides of every power of two from one doc to the next."""
    return 1 + (np.asarray(docs, np.int64) * 101) % 255


@functools.lru_cache(maxsize=None)
def wave_scatter_cases(n=MAX_BLOCK_DOCS):
    """Queries of at most 64 terms: every term per wave segment (S = block_docs / 16)."""
    c = Coll(n)
    S = c.wave_seg
    cases = []

    def add(name, queries, ks, boundary, note=""):
        cases.append(Case(f"wave{n}/{name}", "scatter_wave", c, queries, ks, boundary, note=note))

    if n == MAX_BLOCK_DOCS:
        # one long term whose 16 runs have the lengths RUN_LENGTHS; the boundary postings
        # (first and last doc of a run) carry 1 and 255: both sides of any pruning cut
        docs = np.concatenate([w * S + np.arange(m) for w, m in enumerate(RUN_LENGTHS)])
        vals = _values(docs)
        for w, m in enumerate(RUN_LENGTHS):
            if m >= 2:
                vals[docs == w * S] = 1
                vals[docs == w * S + m - 1] = 255
        tr = c.term(docs, vals)
        st = _stripes(c, docs)
        add("run_lengths", [[tr, s] for s in st] + [[st[0], tr]], (4096,),
            [(tr, w * S + m - 1) for w, m in enumerate(RUN_LENGTHS) if m], note="runs " + str(RUN_LENGTHS))
    # postings at docs w S - 1 and w S for every wave: long (with 100 more docs) and short
    edge = np.array(sorted({d for w in range(1, WSEG) for d in (w * S - 1, w * S)} | {0, n - 1}))
    edge = edge[edge < n]
    more = np.setdiff1d(_spread(n, 140, 5), edge)[:100]
    te_long = c.term(np.concatenate([edge, more]), np.concatenate([_values(edge), _values(more)]))
    te_short = c.term(edge, 256 - _values(edge))
    add("segment_edges", [[te_long], [te_short], [te_short, te_long], [te_long, te_short]],
        (1000,), [(te_long, int(d)) for d in edge[:4]] + [(te_short, int(edge[-1]))],
        note="docs w S - 1 and w S of every wave, long and short sublist")
    # short sublists of 1, 64, 65, 127 postings and the first long one, 128
    lens = (1, 64, 65, 127, 128)
    ts = [c.term(_spread(n, m, 7 + i), _values(_spread(n, m, 7 + i))) for i, m in enumerate(lens)]
    add("short_lengths", [[t] for t in ts] + [ts, ts[::-1]], (1000,),
        [(t, int(c.terms[t][0][-1])) for t in ts], note="sublists of " + str(lens))
    # a term in every doc, first and second in the query
    d = np.arange(n)
    tev = c.term(d, _values(d))
    tx = c.term(_spread(n, 90, 11), 3)
    st = _stripes(c, d)
    add("every_doc", [[tev, s] for s in st] + [[s, tev] for s in st[:2]] + [[tev, tx], [tx, tev]],
        (4096,), [(tev, 0), (tev, n - 1), (tev, S), (tev, S - 1)],
        note="first-touch bits from either term")
    return cases


ALL_WAVE_LENGTHS = (1024, 1025, 4096, 4097, 16384, 16385, 20480, 32768)


@functools.lru_cache(maxsize=None)
def all_wave_cases():
    """Queries of 65..256 terms: whole sublists, a barrier per term, the next term's first
    4096 postings loaded ahead by a term's last round."""
    n = MAX_BLOCK_DOCS
    c = Coll(n)
    fill = [c.term([int(d)], 1 + i % 7) for i, d in enumerate(_spread(n, 70, 3, step=467))]
    cases = []
    for m in ALL_WAVE_LENGTHS:
        docs = np.sort(_spread(n, m, m % 97))
        big = c.term(docs, _values(docs))
        qs = []
        for s in _stripes(c, docs):
            qs += [[big, s] + fill,      # first term: no postings loaded ahead, rem = m
                   fill + [big, s],      # after a one-posting term: rem = m - 4096
                   fill + [s, big]]      # the last term: nothing to load ahead
        cases.append(Case(f"allwave/{m}", "scatter_all_wave", c, qs, (4096,),
                          [(big, int(docs[0])), (big, int(docs[-1])), (big, int(docs[m // 2]))],
                          note=f"a sublist of {m} postings"))
    # the tie rule through the all-wave scatter and the block-wide radix: equal scores 7
    # as 7 via one term ((j, 7)), as 3 + 4 ((j, 3)) and as 7 via the next term ((j + 1, 7)),
    # docs descending from group to group, 970 docs above, the cut (k = 1000) inside the
    # 3 + 4 group -- with the fillers (ten of them score 7 too, none more) behind, in front
    # and around
    taken = np.concatenate([c.terms[t][0] for t in fill])
    ids = np.sort(np.setdiff1d(_spread(n, 1200, 11), taken)[:1030])
    g7b, g34, g7a, above = np.split(ids, np.cumsum([20, 30, 10]))
    t0 = c.term(np.concatenate([g7a, g34]), np.concatenate([np.full(10, 7), np.full(30, 3)]))
    t1 = c.term(np.concatenate([g34, g7b]), np.concatenate([np.full(30, 4), np.full(20, 7)]))
    t2 = c.term(above, 20 + np.arange(970) % 200)
    cases.append(Case("allwave/ties_jv", "scatter_all_wave", c,
                      [[t0, t1, t2] + fill, fill + [t0, t1, t2], fill[:35] + [t1, t0] + fill[35:] + [t2]],
                      (1000,), [(t0, int(g34[0]))],
                      note="radix/doc_cut inside equal scores ordered by (j, v_j)"))
    # 256 terms: one doc holds every term at 255 (score 65 280); term 255 alone touches
    # another doc ((255 - j) == 0)
    c2 = Coll(n)
    H, E = 12345, n - 1
    ts = []
    for j in range(256):
        own = _spread(n, 3, 100 + 7 * j, step=1009)
        own = own[(own != H) & (own != E)]
        d = np.concatenate([[H], own] + ([[E]] if j == 255 else []))
        ts.append(c2.term(d, np.concatenate([[255], 1 + (own + j) % 255] + ([[77]] if j == 255 else []))))
    cases.append(Case("allwave/256_terms", "scatter_all_wave", c2, [ts, ts[:65], ts[191:]],
                      (1000, 1), [(ts[255], E), (ts[100], H)],
                      note="score 65 280; first touch by term 255"))
    return cases


@functools.lru_cache(maxsize=None)
def long_query_cases(n):
    """Queries of more than 256 terms (score_long_kernel) over one block of n docs: 16384
    (one half), 16385 (a second half of one doc), 32768 (two full halves)."""
    c = Coll(n)
    H, F = 5, 16001
    n1 = min(n, LH_DOCS)
    base = []
    for j in range(DI_MAX_QUERY_TERMS):
        a = (3 * j + 7) % n1
        a = a if a not in (H, F) else 6
        d, v = [H, a], [255, 1 + j % 255]
        if j == DI_MAX_QUERY_TERMS - 1:
            d, v = d + [F], v + [9]
        base.append(c.term(d, v))
    cases = []

    def add(name, queries, ks, boundary, note=""):
        cases.append(Case(f"long{n}/{name}", "long", c, queries, ks, boundary, note=note))

    add("257_4095_4096", [base[:257], base[:4095], base], (1, 1000, 4096),
        [(base[4095], F), (base[256], H)],
        note="score 1 044 480 at doc 5; doc 16001 first touched by term 4095")
    if n > LH_DOCS:
        # candidates only in the second half; more than k in both halves
        n2 = n - LH_DOCS
        xs = [c.term(np.unique(LH_DOCS + np.array([0, (5 * j) % n2, n2 - 1])), 1 + j % 200)
              for j in range(300)]
        b1 = c.term(_spread(LH_DOCS, 3000, 1), _values(np.arange(3000)))
        b2 = c.term(LH_DOCS + (_spread(n2, min(n2, 3000), 2) if n2 > 1 else np.zeros(1, np.int64)),
                    _values(np.arange(min(n2, 3000))) if n2 > 1 else 50)
        add("second_half_only", [xs, xs[:257]], (1, 1000), [(xs[0], n - 1), (xs[299], LH_DOCS)],
            note="the first half is empty")
        add("both_halves", [[b1, b2] + base[:255], base[:255] + [b2, b1]], (1, 1000, 4096),
            [(b2, int(c.terms[b2][0][0])), (b1, int(c.terms[b1][0][0]))],
            note="held keys take part in the second selection")
    return cases


def _banded(c, order, per_block, handful):
    """One term whose docs of block b carry values in a band of 20: ascending, every block
    strictly above the earlier ones; descending, below -- but for `handful` docs per later
    block at 250.  Docs at the first and last index of every block.  Returns the term and
    a doc of the last block that is in the shard's top-k."""
    nb, bd = c.nb, c.block_docs
    docs, vals = [], []
    for b in range(nb):
        nl = c.n_local(b)
        idx = np.unique(np.concatenate([[0, nl - 1], _spread(nl, per_block - 2, 5 + b, step=11)]))
        band = b if order == "ascending" else nb - 1 - b
        v = 20 * band + 2 + np.arange(idx.size) % 18
        if order == "descending" and b > 0:
            v[1:1 + handful] = 250
        docs.append(b * bd + idx)
        vals.append(v)
    top = docs[-1][1] if order == "descending" and nb > 1 else docs[-1][-1]
    return c.term(np.concatenate(docs), np.concatenate(vals)), int(top)


@functools.lru_cache(maxsize=None)
def block_count_cases(nb, full=False, doc_lo=1000):
    """The same pattern over a shard of nb blocks (few_blocks at 2..7, the automatic shared
    threshold from 8), doc_lo nonzero.  Blocks that leave an accumulator tail for 2 k keys
    (at most 29 376 docs), or full 32 768-doc blocks (keys stage in the histogram area).
    Every block holds 2100 docs of the main term: more than 2 k at k = 1000."""
    n = nb * MAX_BLOCK_DOCS if full else (nb - 1) * MAX_BLOCK_DOCS + 2000 if nb > 1 else 20000
    c = Coll(n, doc_lo)
    assert c.nb == nb
    tag = f"nb{nb}" + ("full" if full else "")
    cases = []
    few = [c.term(np.unique(np.concatenate([[0, n - 1], _spread(n, 40 * nb, 9, step=7001)])), 1)]
    for order in ("ascending", "descending"):
        t, last = _banded(c, order, 2100, 5)
        cases.append(Case(f"blocks/{tag}/{order}", "blocks", c, [[t], few + [t], [t] + few],
                          (1000, 2048, 2049) if full and nb >= 8 else (100, 1000), [(t, last)],
                          designed="sweep_overflows>full" if order == "ascending" else "sweep_emits",
                          note=f"{order} bands over {nb} blocks"))
    if nb > 1:
        # a plateau: 2100 docs of block 0 and 50 docs of the last block all score 5, the
        # late ones first touched by the earlier term, so they rank first.  Block 0
        # publishes 5; the last block's sweep must emit docs scoring exactly the threshold.
        nl = c.n_local(nb - 1)
        late = (nb - 1) * c.block_docs + np.unique(np.concatenate([[0, nl - 1], _spread(nl, 48, 7, step=211)]))
        ta = c.term(late, 5)
        tb = c.term(np.unique(np.concatenate([[0, c.block_docs - 1], _spread(c.block_docs, 2098, 3, step=11)])), 5)
        cases.append(Case(f"blocks/{tag}/plateau", "blocks", c, [[ta, tb]], (100, 1000),
                          [(ta, int(late[-1]))], designed="sweep_emits",
                          note="docs scoring exactly the published threshold are in the top-k"))
    if nb >= AUTO_THRESHOLD_BLOCKS:
        # 17 terms in the same 150 docs of every block at 241..255: every score >= 4097,
        # the shared histogram's last bin takes them all
        q = []
        for j in range(17):
            docs = np.concatenate([b * c.block_docs + _spread(c.n_local(b), 150, 3, step=131)
                                   for b in range(nb)])
            q.append(c.term(docs, 241 + (docs + j) % 15))
        best = int(np.argmax(accumulate(c, q)[0]))
        cases.append(Case(f"blocks/{tag}/saturate", "blocks", c, [q], (100,), [(q[16], best)],
                          designed="sweep_overflows>full", note="QH_BINS saturation: k-th score >= 4095"))
    return cases


def all_cases():
    out = []
    for n in (MAX_BLOCK_DOCS, 20000):
        out += selection_cases(n)
    out += small_collection_cases()
    out += wave_scatter_cases(MAX_BLOCK_DOCS) + wave_scatter_cases(20000)
    out += all_wave_cases()
    for n in (16384, 16385, 32768):
        out += long_query_cases(n)
    for nb in (1, 2, 7, 8, 9):
        out += block_count_cases(nb)
    out += block_count_cases(3) + block_count_cases(3, full=True)
    out += block_count_cases(8, full=True)  # hist_fits on both sides of k = 2048
    return out


# ---------------------------------------------------------------------------------------
# census of a random batch (tests/test_index_gpu.py::test_synthetic_matches_oracle)
# ---------------------------------------------------------------------------------------
def census(term_off, pdoc, pval, queries, k):
    """Items (query, block) per full-selection route of expected_route, for reference-
    order postings from doc 0."""
    import collections

    n_docs = int(pdoc.max()) + 1
    nb, bd, _ = layout(n_docs)
    count = collections.Counter()
    for q in queries:
        if not q or len(q) > DI_SHORT_QUERY_TERMS:
            continue
        sc, first, v0 = np.zeros(n_docs, np.int64), np.full(n_docs, -1, np.int64), np.zeros(n_docs, np.int64)
        for j, t in enumerate(q):
            d = pdoc[term_off[t]:term_off[t + 1]].astype(np.int64)
            v = pval[term_off[t]:term_off[t + 1]].astype(np.int64)
            new = first[d] < 0
            first[d[new]], v0[d[new]] = j, v[new]
            sc[d] += v
        w = words_of(sc, first, v0, len(q))
        for b in range(nb):
            count[expected_route(w[b * bd:(b + 1) * bd], len(q), k)] += 1
    return count
