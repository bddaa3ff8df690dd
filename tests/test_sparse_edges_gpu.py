"""The float index (csrc/sparse.hip) at its edges, bit-exact against the CPU oracle's float
scorer (oracle.SparseIndex; the reference: src/deep_impact/evaluation/
nano_beir_evaluator.py:78-133): the 16384-doc block and 8192-doc half-block boundaries, what
di_sparse_create keeps and drops, the documented key layout, the tie rule past 255 query
terms, the query-chunk loop with the merge past its LDS capacity, device pointers with a
rejected query, the host-side argument errors, and the rejection of a repeated
(term, doc) posting."""
import ctypes
import time

import numpy as np
import pytest
import torch

import merge_cases as M
import oracle

pytestmark = pytest.mark.gpu

DI_EINVAL, DI_ERANGE = -1, -4
SP_DOCS = 16384  # docs per block (sparse.hip); the f64 scorer works on halves of it
ACCS = ("f32", "f64")


@pytest.fixture(scope="module")
def L():
    from improving_learned_index_amd import _lib

    if _lib.device_count() < 1:
        pytest.fail("no HIP device visible (GPU test run without a GPU)")
    return _lib


class Index:
    """Postings term -> (docs ascending, float32 impacts), as the device index (everything
    handed to di_sparse_create) and as the oracle (impacts > 0 only: its C scorer does not
    filter)."""

    def __init__(self, L, terms, n_docs, device=True):
        self.terms, self.n_docs = terms, n_docs
        self.term_off = np.zeros(len(terms) + 1, np.int64)
        self.term_off[1:] = np.cumsum([len(d) for d, _ in terms])
        cat = lambda i, dt: (np.concatenate([np.asarray(t[i], dt) for t in terms])  # noqa: E731
                             if terms else np.zeros(0, dt))
        self.pdoc, self.pimp = cat(0, np.uint32), cat(1, np.float32)
        self.dev = L.DeviceSparseIndex(self.term_off, self.pdoc, self.pimp, n_docs) \
            if device else None
        keep = self.pimp > 0
        kept = [int(keep[a:b].sum()) for a, b in zip(self.term_off[:-1], self.term_off[1:])]
        self.n_kept = int(keep.sum())
        ora = oracle.SparseIndex.__new__(oracle.SparseIndex)
        ora.corpus_ids = range(n_docs)
        ora.vocab = {t: t for t in range(len(terms))}
        ora.term_off = np.concatenate([[0], np.cumsum(kept)]).astype(np.int64)
        ora.pdoc = np.ascontiguousarray(self.pdoc[keep]) if self.n_kept else np.zeros(1, np.uint32)
        ora.pimp = np.ascontiguousarray(self.pimp[keep]) if self.n_kept else np.zeros(1, np.float32)
        self.ora = ora

    def info(self, L):
        nt, npost = ctypes.c_int64(), ctypes.c_int64()
        nd, nb = ctypes.c_uint32(), ctypes.c_int32()
        L.check(L.lib().di_sparse_info(self.dev._h, ctypes.byref(nt), ctypes.byref(npost),
                                       ctypes.byref(nd), ctypes.byref(nb)))
        return nt.value, npost.value, nd.value, nb.value

    def check(self, qs, k, acc):
        got = self.dev.search(qs, k, accumulation=acc)
        want = self.ora.search(qs, k, use_f64=acc == "f64")
        for i, (g, w) in enumerate(zip(got, want)):
            assert [(d, float(s)) for d, s in g] == w, (i, qs[i], k, acc)
        return want

    def oracle_arrays(self, flat, cu, k, acc):
        """The oracle's C scorer on CSR queries, as arrays (docs, f64 scores, n)."""
        o, n_q = self.ora, len(cu) - 1
        od, osc = np.zeros((n_q, k), np.uint32), np.zeros((n_q, k), np.float64)
        on = np.zeros(n_q, np.int32)
        oracle.lib().or_sparse_search(oracle._p(o.term_off), oracle._p(o.pdoc), oracle._p(o.pimp),
                                      self.n_docs, oracle._p(flat), oracle._p(cu), n_q, k,
                                      int(acc == "f64"), oracle._p(od), oracle._p(osc),
                                      oracle._p(on))
        return od, osc, on

    def sums(self, q):
        """(touched docs ascending, their exact sums) of one query: every impact used with
        this is a small dyadic rational, so float64 sums are the float32 sums."""
        if not q:
            return np.zeros(0, np.int64), np.zeros(0)
        d = np.concatenate([np.asarray(self.terms[t][0], np.int64) for t in q])
        w = np.concatenate([np.asarray(self.terms[t][1], np.float64) for t in q])
        u, inv = np.unique(d, return_inverse=True)
        return u, np.bincount(inv, weights=w)


# ---------------------------------------------------------------------------
# block and half-block edges
# ---------------------------------------------------------------------------
EDGE_DOCS = (0, 8191, 8192, 16383, 16384)


def _edge_index(L, n_docs, seed=0):
    rng = np.random.default_rng([seed, n_docs])
    edges = np.array(sorted({d for d in EDGE_DOCS + (n_docs - 1,) if d < n_docs}))
    terms = []
    for t in range(40):
        m = min(n_docs, int(rng.integers(1, 1500)))
        docs = rng.choice(n_docs, size=m, replace=False)
        take = edges if t == 0 else edges[rng.random(edges.size) < 0.5]
        docs = np.unique(np.concatenate([docs, take]))
        terms.append((docs, (rng.integers(1, 9, docs.size) / 8.0).astype(np.float32)))
    qs = [[], [0], [0, 0], [3, 1, 3], [5, 0, 7, 7, 5]]
    qs += [rng.integers(0, 40, int(n)).tolist() for n in (1, 2, 3, 4, 6, 8, 8)]
    return Index(L, terms, n_docs), qs


@pytest.mark.parametrize("n_docs", [1, 8191, 8192, 8193, 16383, 16384, 16385, 32768, 32769])
def test_block_edges(L, n_docs):
    ix, qs = _edge_index(L, n_docs)
    for d in EDGE_DOCS + (n_docs - 1,):  # postings on both sides of every boundary
        assert d >= n_docs or any(d in docs for docs, _ in ix.terms)
    assert ix.info(L) == (40, ix.n_kept, n_docs, -(-n_docs // SP_DOCS))
    # k = the touched docs of a block (the all-in branch at its edge) and k = the docs of
    # block 0 at or above 2.0 -- every key of the first radix digit's bin is taken
    # (`in_bin == need`: 2.0 starts a new top byte of the f32 and of the f64 bits)
    u, s = ix.sums(qs[4])
    ks = {1, 10, min(n_docs, 4096), 4096, int((u < SP_DOCS).sum()),
          int(((u < SP_DOCS) & (s >= 2.0)).sum()), int(((u < SP_DOCS // 2) & (s >= 2.0)).sum())}
    for k in sorted(x for x in ks if 1 <= x <= 4096):
        for acc in ACCS:
            want = ix.check(qs, k, acc)
            assert want[2] == [(d, 2 * s) for d, s in want[1]]  # the repeated term counts twice
            assert len(want[0]) == 0 and len(want[4]) == min(k, u.size)


# ---------------------------------------------------------------------------
# what create drops and keeps
# ---------------------------------------------------------------------------
def test_create_drops_and_keeps(L):
    f = np.float32
    sub1, sub2 = f(1e-45), f(1e-39)  # subnormals
    assert 0 < sub1 < sub2 < np.finfo(f).tiny
    n_docs = 20000
    terms = [
        # dropped: 0.0, -0.0, negative, NaN, -inf; kept: +inf, subnormals, 0.5
        (np.array([1, 2, 3, 4, 5, 6, 7, 8, 9, 16384, 16390]),
         np.array([0.0, -0.0, -1.0, np.nan, -np.inf, np.inf, sub1, sub2, 0.5, sub1, -2.0], f)),
        (np.array([1, 6, 7, 8, 10, 16384]), np.array([sub1, 1.0, sub1, sub2, sub1, sub1], f)),
        (np.array([2, 7, 10, 11, 19999]), np.array([0.25, sub1, sub2, np.inf, 0.0], f)),
        (np.array([3, 4]), np.array([-0.0, np.nan], f)),  # nothing kept
    ]
    ix = Index(L, terms, n_docs)
    assert ix.n_kept == 5 + 6 + 4 + 0
    assert ix.info(L) == (4, ix.n_kept, n_docs, 2)
    qs = [[0], [1], [2], [3], [0, 1], [1, 0], [2, 1, 0], [0, 2, 1, 1], [3, 0]]
    flat, cu = L.csr(qs)
    for k in (1, 3, 100):
        want = ix.check(qs, k, "f64")
        docs, scores, n, _ = ix.dev.search_csr(flat, cu, k)
        od, osc, on = ix.oracle_arrays(flat, cu, k, "f32")
        assert (n == on).all()
        for i in range(len(qs)):  # the oracle's bits (a subnormal sum is a score, not "untouched")
            assert (docs[i, :n[i]] == od[i, :n[i]]).all(), (i, k)
            assert (scores[i, :n[i]].view(np.uint32) ==
                    osc[i, :n[i]].astype(f).view(np.uint32)).all(), (i, k)
        assert want[3] == []
    # the subnormal sums really occur: doc 7 under [0, 1] is 2 * 1e-45, doc 16384 too
    got = dict(ix.dev.search([[0, 1]], 100)[0])
    assert got[7] == float(f(sub1 + sub1)) and got[16384] == float(f(sub1 + sub1)) and got[7] > 0
    assert got[6] == float("inf")
    assert [d for d, _ in ix.dev.search([[0]], 100)[0]] == [6, 9, 8, 7, 16384]


# ---------------------------------------------------------------------------
# keys
# ---------------------------------------------------------------------------
def test_keys_follow_the_documented_layout(L):
    """out_key = score bits << 32 | (255 - first term) << 24 | (0xFFFFFF - doc)
    (include/deepimpact.h, di_sparse_search), the first term computed here."""
    ix, qs = _edge_index(L, 32769, seed=1)
    flat, cu = L.csr(qs)
    for k in (10, 4096):
        docs, scores, n, keys = ix.dev.search_csr(flat, cu, k, with_keys=True)
        for i, q in enumerate(qs):
            first = np.full(ix.n_docs, 255, np.uint64)
            for j in reversed(range(len(q))):
                first[ix.terms[q[j]][0]] = j
            d = docs[i, :n[i]].astype(np.uint64)
            want = (scores[i, :n[i]].view(np.uint32).astype(np.uint64) << np.uint64(32)) | \
                ((np.uint64(255) - first[d]) << np.uint64(24)) | (np.uint64(0xFFFFFF) - d)
            assert (keys[i, :n[i]] == want).all(), (i, k)
            assert (np.diff(keys[i, :n[i]].astype(object)) < 0).all()  # strictly descending


# ---------------------------------------------------------------------------
# ties past 255 terms
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("acc", ACCS)
def test_ties_past_255_terms_follow_the_documented_rule(L, acc):
    """300 terms with impact 1.0 on 3 docs each, all disjoint, over two blocks; one query of
    all of them: every touched doc scores 1.0.  The order is (score desc, min(j, 255) asc,
    doc asc) (sparse.hip's header, DESIGN.md §5 deviation 2): the reference's first-touch
    order for the docs of terms 0..254, corpus order among those of terms 255..299."""
    rng = np.random.default_rng(5)
    n_docs, n_terms, per = 30000, 300, 3
    owned = rng.permutation(n_docs)[:n_terms * per].reshape(n_terms, per)
    terms = [(np.sort(owned[t]), np.ones(per, np.float32)) for t in range(n_terms)]
    ix = Index(L, terms, n_docs)
    q = list(range(n_terms))
    j_of = np.repeat(np.arange(n_terms), per)
    docs = np.concatenate([t[0] for t in terms])
    order = np.lexsort((docs, np.minimum(j_of, 255)))
    rule = docs[order].tolist()
    true_first_touch = [d for d, _ in ix.ora.search([q], 4096, use_f64=acc == "f64")[0]]
    assert true_first_touch == docs.tolist()
    n_exact = 255 * per
    assert rule[:n_exact] == true_first_touch[:n_exact]
    assert rule[n_exact:] != true_first_touch[n_exact:]  # the rule shows past the prefix
    for k in (10, 1000):
        got = ix.dev.search([q], k, accumulation=acc)[0]
        assert got == [(d, 1.0) for d in rule[:k]], k
    assert k > n_exact


# ---------------------------------------------------------------------------
# query chunks and the merge past its LDS capacity (DECODE_SPARSE)
# ---------------------------------------------------------------------------
BIG_DOCS = (1 << 20) + 1  # 65 blocks, the last holding one doc


def _big_terms(scale=1.0):
    rng = np.random.default_rng(21)
    terms = []
    for t in range(48):
        docs = rng.choice(BIG_DOCS, size=6000, replace=False)
        if t % 8 == 0:
            docs[:2] = (0, BIG_DOCS - 1)
        docs = np.unique(docs)
        imp = (rng.integers(1, 5, docs.size) / 32.0 if t < 24
               else rng.integers(1, 12, docs.size) / 8.0)
        if t % 8 == 0:  # the first and the last doc of the index, with the term's top impact
            imp[[0, -1]] = imp.max()
        terms.append((docs, (imp * scale).astype(np.float32)))
    return terms


def _big_queries(n_q):
    rng = np.random.default_rng(22)
    qs = []
    for i in range(n_q):
        n = 1 + (i // 3) % 6
        pool = (np.arange(24), np.arange(24, 48), np.arange(48))[i % 3]
        qs.append(rng.choice(pool, size=n, replace=False).tolist())
    return qs


def _query_classes(ix, qs, k, scale=1.0):
    """Per query: (touched docs, largest score / scale, the route its merge takes by
    merge_cases.expected_path from the candidates' f32 key bits).  Asserts that no block
    holds more than k touched docs, so the candidates are all the touched docs."""
    nb = -(-ix.n_docs // SP_DOCS)
    out = []
    for q in qs:
        u, s = ix.sums(q)
        per_block = np.bincount(u // SP_DOCS, minlength=nb)
        assert per_block.max() <= k
        bits = s.astype(np.float32).view(np.uint32)
        assert (bits.view(np.float32).astype(np.float64) == s).all()  # the sums are exact
        route = M.expected_path(nb, k, per_block, bool((bits >> 28).any()),
                                ((bits >> 16) & 4095).astype(np.int64))
        out.append((u.size, s.max() / scale, route))
    return out


@pytest.fixture(scope="module")
def big(L):
    return Index(L, _big_terms(), BIG_DOCS)


def _check_arrays(ix, L, qs, k, acc):
    flat, cu = L.csr(qs)
    t0 = time.perf_counter()
    docs, scores, n, _ = ix.dev.search_csr(flat, cu, k, accumulation=acc)
    t1 = time.perf_counter()
    od, osc, on = ix.oracle_arrays(flat, cu, k, acc)
    print(f"{acc} k={k} n_q={len(qs)}: device {1e3 * (t1 - t0):.1f} ms, "
          f"oracle {1e3 * (time.perf_counter() - t1):.1f} ms")
    assert (n == on).all()
    live = np.arange(k)[None, :] < on[:, None]
    assert (docs[live] == od[live]).all()
    assert (scores[live].astype(np.float64) == osc[live]).all()
    return od, on


@pytest.mark.parametrize("acc,n_q", [("f32", 520), ("f64", 140)])
def test_query_chunks_and_overfull_merge(L, big, acc, n_q):
    """k = 4096 over 65 blocks: the candidate workspace (1 GiB) holds 504 f32 queries or 126
    f64 ones, so the query-chunk loop of di_sparse_search / di_sparse_search_f64 runs twice;
    most queries touch more than 8192 docs, past the LDS capacity of the f32 merge.
    (An f32 score from 2^-95 up sets one of the key's top four bits, so merge_topk_kernel's
    histogram paths stand aside for every query of this index, below 2.0 or not: the route
    printed is the radix select.  test_tiny_scores_take_the_histogram_merge runs the
    histogram paths in this decode mode.)"""
    k = 4096
    nb = -(-BIG_DOCS // SP_DOCS)
    assert big.info(L)[3] == nb == 65
    per_q = nb * k * 8 if acc == "f32" else 2 * nb * k * 16
    chunk = (1 << 30) // per_q
    assert chunk == (504 if acc == "f32" else 126) and chunk < n_q <= 2 * chunk
    qs = _big_queries(n_q)
    assert all(1 <= len(q) == len(set(q)) <= 6 for q in qs)
    cls = _query_classes(big, qs, k)
    below = [c for c in cls if c[0] > 8192 and c[1] < 2.0]
    above = [c for c in cls if c[0] > 8192 and c[1] >= 2.0]
    single = [c for q, c in zip(qs, cls) if len(q) == 1 and c[0] <= 8192]
    print(f"{acc}: {len(below)} queries > 8192 touched docs, all scores < 2.0; {len(above)} with "
          f"a score >= 2.0; {len(single)} single-term <= 8192; routes "
          f"{sorted({c[2] for c in cls})}")
    assert below and above and single
    # both sides of the chunk boundary hold every class
    for part in (cls[:chunk], cls[chunk:]):
        assert any(c[0] > 8192 for c in part) and any(c[0] <= 8192 for c in part)
    od, on = _check_arrays(big, L, qs, k, acc)
    assert (on == np.minimum([c[0] for c in cls], k)).all()
    # k = 1000 in one chunk
    _check_arrays(big, L, qs[:60], 1000, acc)


def test_last_block_of_one_doc(L, big):
    """Doc 2^20 alone in block 64, doc 0 first in block 0: both are found with their sums."""
    for acc in ACCS:
        got = big.dev.search([[0], [24, 0], [8, 16, 24, 32, 40]], 4096, accumulation=acc)
        want = big.ora.search([[0], [24, 0], [8, 16, 24, 32, 40]], 4096, use_f64=acc == "f64")
        assert [[(d, float(s)) for d, s in g] for g in got] == want
        for w in want:
            assert {0, BIG_DOCS - 1} <= {d for d, _ in w}


def test_tiny_scores_take_the_histogram_merge(L):
    """The same index with every impact scaled by 2^-100 (exact: the sums scale with it).
    The f32 keys then stay below 2^60, and by merge_cases.expected_path the over-capacity
    queries take the two-pass histogram filter with the counting selection, or its overflow
    into the sort -- in DECODE_SPARSE mode, which the quantized index never uses."""
    scale = 2.0 ** -100
    ix = Index(L, _big_terms(scale), BIG_DOCS)
    qs = _big_queries(60)
    k = 1000
    cls = _query_classes(ix, qs, k, scale)
    routes = {c[2] for c in cls}
    print("routes:", sorted(routes))
    assert {"topk<512>/cap8192/two_pass/counting",
            "topk<512>/cap8192/two_pass/counting_overflow>sort",
            "topk<512>/cap8192/flatten/counting"} <= routes
    _check_arrays(ix, L, qs, k, "f32")


# ---------------------------------------------------------------------------
# device pointers, a rejected query
# ---------------------------------------------------------------------------
def test_device_pointers_with_a_rejected_query(L):
    ix, qs = _edge_index(L, 32769, seed=2)
    bad = 5
    qs_dev = [list(q) for q in qs]
    qs_dev[bad] = qs_dev[bad] + [40]  # term id == n_terms
    flat, cu = L.csr(qs_dev)
    n_q, k = len(qs), 100
    dev = torch.device("cuda", 0)
    tq, tcu = torch.from_numpy(flat.view(np.int32)).to(dev), torch.from_numpy(cu).to(dev)
    od = torch.zeros(n_q * k, dtype=torch.int32, device=dev)
    osc = torch.zeros(n_q * k, dtype=torch.float32, device=dev)
    on = torch.full((n_q,), -7, dtype=torch.int32, device=dev)
    ok = torch.zeros(n_q * k, dtype=torch.int64, device=dev)
    torch.cuda.synchronize()
    P = L.ptr
    L.check(L.lib().di_sparse_search(ix.dev._h, P(tq), P(tcu), n_q, k, P(od), P(osc), P(on),
                                     P(ok), L.DI_F_DEVICE_PTRS))
    n = on.cpu().numpy()
    docs = od.cpu().numpy().view(np.uint32).reshape(n_q, k)
    scores = osc.cpu().numpy().reshape(n_q, k)
    keys = ok.cpu().numpy().view(np.uint64).reshape(n_q, k)
    want = ix.ora.search(qs, k)
    hd, hs, hn, hk = ix.dev.search_csr(*L.csr(qs), k, with_keys=True)
    for i in range(n_q):
        if i == bad:
            assert n[i] == -1
            continue
        assert list(zip(docs[i, :n[i]].tolist(), scores[i, :n[i]].tolist())) == want[i], i
        assert n[i] == hn[i] and (keys[i, :n[i]] == hk[i, :n[i]]).all(), i
    # the same batch on host pointers is refused as a whole
    with pytest.raises(L.DIError) as e:
        ix.dev.search(qs_dev, k)
    assert e.value.code == DI_EINVAL


# ---------------------------------------------------------------------------
# host errors, empty indexes
# ---------------------------------------------------------------------------
def test_host_errors(L):
    ix, qs = _edge_index(L, 8193, seed=3)
    for acc in ACCS:
        for k in (0, 4097):
            with pytest.raises(L.DIError) as e:
                ix.dev.search(qs, k, accumulation=acc)
            assert e.value.code == DI_ERANGE
        with pytest.raises(L.DIError) as e:
            ix.dev.search([[1], [0] * 4097], 10, accumulation=acc)
        assert e.value.code == DI_ERANGE
        assert len(ix.dev.search([[0] * 4096], 1, accumulation=acc)[0]) == 1  # the limit itself
        with pytest.raises(L.DIError) as e:
            ix.dev.search([[1], [2, 40]], 10, accumulation=acc)
        assert e.value.code == DI_EINVAL
    with pytest.raises(L.DIError) as e:
        L.DeviceSparseIndex(np.array([0, 2]), np.array([3, 8193]), np.array([1.0, 1.0]), 8193)
    assert e.value.code == DI_EINVAL
    with pytest.raises(L.DIError) as e:  # even where the impact would be dropped
        L.DeviceSparseIndex(np.array([0, 2]), np.array([3, 9000]), np.array([1.0, 0.0]), 8193)
    assert e.value.code == DI_EINVAL


@pytest.mark.parametrize("acc", ACCS)
def test_empty_indexes(L, acc):
    no_docs = L.DeviceSparseIndex(np.zeros(4, np.int64), np.zeros(0, np.uint32),
                                  np.zeros(0, np.float32), 0)
    assert no_docs.search([[], [0, 2], []], 10, accumulation=acc) == [[], [], []]
    no_terms = L.DeviceSparseIndex(np.zeros(1, np.int64), np.zeros(0, np.uint32),
                                   np.zeros(0, np.float32), 100)
    assert no_terms.search([[], []], 10, accumulation=acc) == [[], []]
    with pytest.raises(L.DIError) as e:
        no_terms.search([[0]], 10, accumulation=acc)
    assert e.value.code == DI_EINVAL


# ---------------------------------------------------------------------------
# a repeated (term, doc) posting
# ---------------------------------------------------------------------------
def test_repeated_posting_is_rejected(L):
    """The score kernels apply one term's postings in parallel with a plain read-modify-write:
    a doc named twice by one term would lose an update.  di_sparse_create refuses it."""
    rng = np.random.default_rng(8)
    n_docs = 20000
    terms = []
    for t in range(5):
        docs = np.sort(rng.choice(n_docs, 800, replace=False))
        terms.append((docs, (rng.integers(1, 9, 800) / 8.0).astype(np.float32)))
    clean = Index(L, terms, n_docs)
    qs = [[2], [2, 2, 0], [4, 3, 2, 1, 0]]
    for acc in ACCS:
        clean.check(qs, 1000, acc)
    d2, i2 = terms[2]
    dup = d2[400]

    def with_extra(impact, at):
        t2 = (np.insert(d2, at, dup), np.insert(i2, at, np.float32(impact)))
        return terms[:2] + [t2] + terms[3:]

    for at in (401, 800):  # next to the first posting, and at the term's end
        with pytest.raises(L.DIError) as e:
            Index(L, with_extra(0.5, at), n_docs)
        assert e.value.code == DI_EINVAL
        assert "term 2" in str(e.value) and f"doc {dup}" in str(e.value)
    # a second posting that is dropped (impact 0) before the check is no duplicate
    for impact in (0.0, -1.0, np.nan):
        ok = Index(L, with_extra(impact, 401), n_docs)
        assert ok.info(L)[1] == clean.n_kept
        for acc in ACCS:
            assert ok.check(qs, 1000, acc) == clean.ora.search(qs, 1000, use_f64=acc == "f64")
