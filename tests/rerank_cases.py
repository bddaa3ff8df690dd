"""Seeded cases of the re-ranker's device store and scorer (csrc/rerank.hip), and the
restatement of the reference they are checked against: ReRanker.score
(src/deep_impact/evaluation/reranker.py:52-53) and the order of line 91.

A store is a list of passages, each a list of (term id, np.float32 impact) pairs in the
order they are handed over.  Impacts: lognormal(0, 2) times a sign that is negative with
probability 0.2, cast to float32 -- magnitudes spread over many binades, so float32 sums
depend on the order of the adds -- with a seeded share of exact +0.0 and of -0.0.
"""
from __future__ import annotations

import functools

import numpy as np

ZERO_SHARE, NEG_ZERO_SHARE = 0.04, 0.03
CUT = 1000  # reranker.py:91


def draw_impacts(rng, n):
    v = (rng.lognormal(0.0, 2.0, n) * np.where(rng.random(n) < 0.2, -1.0, 1.0)).astype(np.float32)
    u = rng.random(n)
    v[u < ZERO_SHARE] = np.float32(0.0)
    v[(u >= ZERO_SHARE) & (u < ZERO_SHARE + NEG_ZERO_SHARE)] = np.float32(-0.0)
    return v


# ------------------------------------------------------------------ the restatement
def reference_score(cache_pid: dict, query_terms):
    """reranker.py:52-53, literally: the int 0 when nothing matched, else an np.float32
    (numpy >= 2: int + np.float32 is an np.float32)."""
    return sum(cache_pid.get(term, 0) for term in query_terms)


def reference_scores(passages, queries, cands):
    """passages: the store; queries: per query its term ids in iteration order; cands: per
    query its candidate store indices.  -> per query (scores: what reference_score gives,
    bits uint32 of the float32 sums, match int32: the terms that matched)."""
    cache = [dict(p) for p in passages]  # ReRanker.save, reranker.py:48-50
    out = []
    for q, cs in zip(queries, cands):
        scores = [reference_score(cache[c], q) for c in cs]
        bits = np.array([np.float32(s).view(np.uint32) for s in scores], np.uint32)
        match = np.array([sum(t in cache[c] for t in q) for c in cs], np.int32)
        for s, m in zip(scores, match):
            assert isinstance(s, int) == (m == 0) and (m == 0 or isinstance(s, np.float32))
        out.append((scores, bits, match))
    return out


def reference_ranking(pids, scores):
    """reranker.py:91."""
    return sorted(zip(pids, scores), key=lambda x: x[1], reverse=True)[:CUT]


# ------------------------------------------------------------------ packing for the ABI
def pack_passages(passages):
    """-> (term_ids uint32, impacts float32, cu_terms int32) of di_term_store_append."""
    cu = np.zeros(len(passages) + 1, np.int32)
    cu[1:] = np.cumsum([len(p) for p in passages])
    ids = np.array([t for p in passages for t, _ in p], np.uint32)
    imp = np.array([v for p in passages for _, v in p], np.float32)
    return ids, imp, cu


def pack_queries(queries, cands):
    """-> (q_terms uint32, cu_q int32, cand_doc int32, cu_cand int32) of di_term_store_score."""
    cu_q = np.zeros(len(queries) + 1, np.int32)
    cu_q[1:] = np.cumsum([len(q) for q in queries])
    cu_c = np.zeros(len(cands) + 1, np.int32)
    cu_c[1:] = np.cumsum([len(c) for c in cands])
    return (np.array([t for q in queries for t in q], np.uint32), cu_q,
            np.array([c for cs in cands for c in cs], np.int32), cu_c)


# ------------------------------------------------------------------ the ABI case
PASSAGE_SIZES = (0, 1, 2, 63, 64, 65, 255, 256, 257, 2047, 2048)
QUERY_SIZES = (0, 1, 6, 63, 64, 65, 300)
# term ids of the passages: small ones, and two with the top bit set (the sort key holds
# the id in its upper half)
VOCAB = np.concatenate([np.arange(2398, dtype=np.uint32),
                        np.array([0x80000000, 0xFFFFFFFF], np.uint32)])
ABSENT = np.arange(5000, 5040, dtype=np.uint32)  # ids no passage holds
APPEND_SPLITS = (0, 8, 15, 22)  # the three append calls (host, device, host pointers)


@functools.lru_cache(maxsize=None)
def abi_case(seed=11):
    """22 passages (every size of PASSAGE_SIZES with its ids descending, then in random
    order) and 8 queries (QUERY_SIZES; ids no passage holds; a repeated id; the last query
    has no candidates; query 2 names passage 5 twice).  -> (passages, queries, cands, ref),
    ref = reference_scores(...), computed once."""
    rng = np.random.default_rng(seed)
    passages = []
    for order in ("descending", "random"):
        for T in PASSAGE_SIZES:
            ids = rng.choice(VOCAB, T, replace=False)
            ids = np.sort(ids)[::-1] if order == "descending" else ids
            passages.append(list(zip(ids.tolist(), draw_impacts(rng, T))))
    queries = []
    for Q in QUERY_SIZES:
        q = rng.choice(VOCAB, Q, replace=True)  # (300 draws of 2400 ids repeat some)
        if Q >= 6:
            q[rng.choice(Q, max(1, Q // 6), replace=False)] = rng.choice(ABSENT, max(1, Q // 6))
            q[Q - 1] = q[1] = passages[10][7][0]  # a repeated id that passage 10 (2048) holds
            q[2], q[3] = 0xFFFFFFFF, ABSENT[0]
        queries.append(q.tolist())
    queries.append(rng.choice(VOCAB, 6, replace=False).tolist())
    n = len(passages)
    cands = [list(range(n)) for _ in QUERY_SIZES] + [[]]
    cands[1] = [3, 21, 10]
    cands[2] = list(range(n)) + [5, 5]
    cands[4] = list(rng.permutation(n))
    return passages, queries, cands, reference_scores(passages, queries, cands)


# ------------------------------------------------------------------ the ranking case
@functools.lru_cache(maxsize=None)
def ranking_case(seed=5, n_cand=1001, n_queries=3):
    """Passages of 1 to 40 pairs over a 60-id vocabulary and n_queries queries of 3 to 8 distinct ids
    with n_cand candidates each, so the cut at 1000 drops one.  Planted per query: passages
    with ids outside the vocabulary (no match: the int 0), passages whose only matching
    pair has impact 0.0 (a matched 0.0, equal to the int 0), copies of other candidates'
    passages (equal sums), and the lowest sum twice (a tie across rank 1000).
    -> (passages, queries, cands, ref)."""
    rng = np.random.default_rng(seed)
    vocab = np.arange(100, 160, dtype=np.uint32)
    queries = [rng.choice(vocab, int(rng.integers(3, 9)), replace=False).tolist()
               for _ in range(n_queries)]
    passages, cands = [], []
    for q in queries:
        mine = []
        for i in range(n_cand):
            kind = i % 25
            if kind == 3:  # no match
                ids = rng.choice(np.arange(900, 960, dtype=np.uint32), 4, replace=False)
                p = list(zip(ids.tolist(), draw_impacts(rng, 4)))
            elif kind == 7:  # a matched 0.0
                p = [(q[0], np.float32(0.0)), (950, np.float32(2.5))]
            elif kind == 11 and mine:  # a copy of an earlier candidate
                p = list(passages[mine[int(rng.integers(0, len(mine)))]])
            else:
                T = int(rng.integers(1, 41))
                ids = rng.choice(vocab, T, replace=False)
                p = list(zip(ids.tolist(), draw_impacts(rng, T)))
            mine.append(len(passages))
            passages.append(p)
        # the lowest sum twice, far apart in the list: one of the two is cut
        passages[mine[40]] = [(q[0], np.float32(-1e6))]
        passages[mine[900]] = [(q[0], np.float32(-1e6))]
        cands.append(mine)
    return passages, queries, cands, reference_scores(passages, queries, cands)


def sum_bits(values, reverse=False):
    """float32 bits of Python's sum() of np.float32 values in the given (or reverse) order."""
    vs = list(values)[::-1] if reverse else list(values)
    return np.float32(sum(vs)).view(np.uint32)


def matched_values(passages, query, cand):
    d = dict(passages[cand])
    return [d[t] for t in query if t in d]
