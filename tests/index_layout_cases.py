"""Shared inputs of tests/test_index_layout_cases_cpu.py and tests/test_index_layout_gpu.py
(not a test module): constructed CSR collections for the scorer's blocked device layout, and
a plain Python / numpy restatement of build_index() (csrc/index.hip) -- the kept postings,
the (term, block) entries, the per-group class order and the sequential greedy bank deal --
whose output both layout routes (di_index_create on host threads, di_index_create_device on
the GPU) must equal byte for byte.  The restatement also counts which branches of the deal a
case reaches (census), so that the CPU test can prove each case hits what it was built for.

Every length that matters is placed; random numbers only fill values and filler terms."""
import functools

import numpy as np

MAX_BLOCK_DOCS = 32768   # csrc/index_score.h
WSEG = 16
WLONG_MIN = 128
POST_X = MAX_BLOCK_DOCS << 10
NO = 0xFFFFFFFF

ENVS = {  # (f): read at create time
    "default": {},
    "wlong1": {"DI_WLONG_MIN": "1"},
    "wlong64": {"DI_WLONG_MIN": "64"},
    "x4off": {"DI_DEAL_X4": "0"},
    "classes": {"DI_DEAL_CLASSES": "1"},
}
ENV_NAMES = ("DI_WLONG_MIN", "DI_DEAL_X4", "DI_DEAL_CLASSES")


def blocks_of(nd):
    """build_index: (nb, block_docs) of a shard of nd docs."""
    nb = -(-nd // MAX_BLOCK_DOCS)
    if nb == 0:
        return 0, MAX_BLOCK_DOCS
    return nb, min(MAX_BLOCK_DOCS, -(-(-(-nd // nb)) // 64) * 64)


class Case:
    """A CSR (term_off, pdoc, pval) plus the shard range."""

    def __init__(self, name, terms, doc_lo=0, doc_hi=0, lead=0):
        self.name, self.doc_lo, self.doc_hi = name, int(doc_lo), int(doc_hi)
        docs = [np.full(lead, 7, np.uint32)]   # postings before term_off[0]: never read
        vals = [np.full(lead, 9, np.uint8)]
        off = [lead]
        for d, v in terms:
            d, v = np.asarray(d, np.uint32), np.asarray(v, np.uint8)
            assert d.shape == v.shape and d.ndim == 1
            docs.append(d)
            vals.append(v)
            off.append(off[-1] + d.size)
        self.term_off = np.array(off, np.int64)
        self.pdoc = np.concatenate(docs)
        self.pval = np.concatenate(vals)
        self.n_terms = len(terms)

    def kept(self):
        """Per term the kept (doc - doc_lo, value) pairs in input order, and the resolved
        doc_hi -- the three rules of build_index, stated on their own."""
        a, b = int(self.term_off[0]), int(self.term_off[-1])
        hi = self.doc_hi
        if hi == 0:
            hi = int(self.pdoc[a:b].max()) + 1 if b > a else self.doc_lo
        out = []
        for t in range(self.n_terms):
            s, e = int(self.term_off[t]), int(self.term_off[t + 1])
            d, v = self.pdoc[s:e].astype(np.int64), self.pval[s:e].astype(np.int64)
            z = np.flatnonzero(v == 0)
            if z.size:
                d, v = d[:z[0]], v[:z[0]]
            m = (d >= self.doc_lo) & (d < hi)
            out.append((d[m] - self.doc_lo, v[m]))
        return out, hi


def _ctz(x):
    return (x & -x).bit_length() - 1


def _cls(w):
    return 7 - ((w & 255).bit_length() - 1)


def emit_group(words, one_class, deal_x4, census):
    """emit_group of build_index: classes in order (stable), each bucketed stably by bank
    and dealt by the sequential greedy -> (the words in output order, the 8 class ends)."""
    by_cls = [[] for _ in range(8)]
    for w in words:
        by_cls[0 if one_class else _cls(w)].append(w)
    out, cum = [], []
    usedq, cursor = [0, 0, 0, 0], 0
    reset = 127 if deal_x4 else 31
    for c in range(8):
        cw = by_cls[c]
        buckets = [[] for _ in range(32)]
        for w in cw:
            buckets[(w >> 8) & 31].append(w)
        head = [0] * 32
        avail = sum(1 << k for k in range(32) if buckets[k])
        if cw and out and cursor:
            census["cursor_carry"] += 1
        for i in range(len(cw)):
            rp = len(out)
            if rp & reset == 0:
                usedq = [0, 0, 0, 0]
                if i > 0:
                    census["reset_in_class"] += 1
            s = rp & 3 if deal_x4 else 0
            cand = avail & ~usedq[s]
            if not cand:
                cand = avail
                census["fallback"] += 1
            rot = ((cand >> cursor) | (cand << (32 - cursor))) & 0xFFFFFFFF if cursor else cand
            k = (_ctz(rot) + cursor) & 31
            out.append(buckets[k][head[k]])
            head[k] += 1
            if head[k] == len(buckets[k]):
                avail &= ~(1 << k)
            usedq[s] |= 1 << k
            cursor = (k + 1) & 31
        cum.append(len(out))
    return out, cum


def _encode(words):
    w = np.asarray(words, np.uint32)
    return (((w >> 8) << 10) | (w & 255)) ^ np.uint32(POST_X)


def decode(post):
    """device word -> (doc_in_block, value)"""
    w = np.asarray(post, np.uint32) ^ np.uint32(POST_X)
    return (w >> 10).astype(np.int64), (w & 255).astype(np.int64)


def layout_ref(case, env=None):
    """build_index() restated -> (dict of the ten arrays and the scalars, census)."""
    env = env or {}
    wlong_min = max(1, int(env.get("DI_WLONG_MIN", WLONG_MIN)))
    deal_x4 = int(env.get("DI_DEAL_X4", 1)) != 0
    flat_runs = int(env.get("DI_DEAL_CLASSES", 0)) == 0
    census = {"fallback": 0, "reset_in_class": 0, "cursor_carry": 0, "entry_lens": set(),
              "direct_terms": 0, "search_terms": 0}
    kept, hi = case.kept()
    nd = hi - case.doc_lo
    nb, bd = blocks_of(nd)
    S = -(-bd // WSEG)
    post, flat, tb_start, eblk, epos, seg, lid, wmeta, emax, wmax = ([] for _ in range(10))
    for rel, val in kept:
        tb_start.append(len(eblk))
        blk = rel // bd
        order = np.argsort(blk, kind="stable")
        words = (((rel % bd) << 8) | val)[order].tolist()
        blk = blk[order].tolist()
        n_ent_t, i = 0, 0
        while i < len(words):
            j = i
            while j < len(words) and blk[j] == blk[i]:
                j += 1
            grp = words[i:j]
            n_ent_t += 1
            census["entry_lens"].add(len(grp))
            eblk.append(blk[i])
            epos.append(len(post))
            emax.append(max(w & 255 for w in grp))
            if len(grp) < wlong_min:
                lid.append(NO)
                out, cum = emit_group(grp, False, deal_x4, census)
                post += out
                flat += out
                seg += cum
            else:
                lid.append(len(wmax) // WSEG)
                cc = [0] * 8
                for w in grp:
                    cc[_cls(w)] += 1
                seg += np.cumsum(cc).tolist()
                s0 = len(post)
                for ws in range(WSEG):
                    seg_in = [w for w in grp if min((w >> 8) // S, WSEG - 1) == ws]
                    wmax.append(max([w & 255 for w in seg_in], default=0))
                    out, cum = emit_group(seg_in, False, deal_x4, census)
                    wmeta += [len(post) - s0 + c for c in cum]
                    post += out
                    if flat_runs:
                        flat += emit_group(seg_in, True, deal_x4, census)[0]
            i = j
        if nb > 1 and n_ent_t == nb:
            census["direct_terms"] += 1
        elif nb > 1 and n_ent_t >= 2:
            census["search_terms"] += 1
    tb_start.append(len(eblk))
    epos.append(len(post))
    lay = {
        "post": _encode(post), "post_flat": _encode(flat) if flat_runs else None,
        "tb_start": np.array(tb_start, np.uint32), "eblk": np.array(eblk, np.uint16),
        "epos": np.array(epos, np.uint32),
        "seg": (np.array(seg, np.int64) & 0xFFFF).astype(np.uint16),
        "lid": np.array(lid, np.uint32),
        "wmeta": (np.array(wmeta, np.int64) & 0xFFFF).astype(np.uint16),
        "emax": np.array(emax, np.uint8), "wmax": np.array(wmax, np.uint8),
        "n_post": len(post), "n_ent": len(eblk), "n_long": len(wmax) // WSEG, "nb": nb,
        "block_docs": bd, "n_docs": nd, "has_flat": flat_runs, "wlong_min": wlong_min,
    }
    return lay, census


@functools.lru_cache(maxsize=None)
def reference(name, env_name="default"):
    """The restatement of a case under an environment, computed once per session."""
    return layout_ref(CASES[name], ENVS[env_name])


ARRAYS = ("post", "post_flat", "tb_start", "eblk", "epos", "seg", "lid", "wmeta", "emax", "wmax")


# ---------------------------------------------------------------------------------------
# the cases
# ---------------------------------------------------------------------------------------
def _vals(rng, n, lo=1, hi=255):
    return rng.integers(lo, hi + 1, n).astype(np.uint8)


def _filler(rng, n_terms, doc_a, doc_b, n_max=40):
    """Small terms of distinct docs in [doc_a, doc_b), value-descending: the other terms of a
    17-term query."""
    out = []
    for _ in range(n_terms):
        n = int(rng.integers(1, n_max + 1))
        d = np.sort(rng.choice(np.arange(doc_a, doc_b), n, replace=False))
        v = np.sort(_vals(rng, n))[::-1]
        out.append((d, v))
    return out


def _case_a():
    """One block: short sublists of 1, 31, 32, 33 and 127 postings."""
    rng = np.random.default_rng(11)
    pat8 = np.array([255, 128, 100, 64, 33, 17, 9, 5, 3, 2, 1, 1], np.uint8)
    terms = [
        ([7], [255]),                                                       # 1 posting
        (np.arange(31) * 32, _vals(rng, 31)),                               # one bank: fallback
        (np.arange(32) * 3 + 1, np.resize(pat8, 32)),                       # all eight classes
        (np.arange(33) * 5 + 2, np.ones(33, np.uint8)),                     # a single class
        (np.arange(127) * 37 % 4099, np.resize([255, 130, 17, 1], 127)),    # empty classes between
        (np.arange(64) * 32 + 5, np.resize([200, 3], 64)),                  # one bank, two classes
    ]
    return Case("a", terms)


def _case_b():
    """One full 32768-doc block: long sublists of exactly 128 and 129 postings, a full wave
    segment, the full block, a long sublist with empty segments, and 127 (short)."""
    rng = np.random.default_rng(12)
    alld = np.arange(MAX_BLOCK_DOCS)
    some = np.concatenate([np.arange(100) * 3, 5 * 2048 + np.arange(60) * 7,
                           15 * 2048 + np.arange(40) * 32])
    terms = [
        (np.arange(127) * 257 % MAX_BLOCK_DOCS, _vals(rng, 127)),
        (np.arange(128) * 251 % MAX_BLOCK_DOCS, _vals(rng, 128)),
        (np.arange(129) * 241 % MAX_BLOCK_DOCS, _vals(rng, 129)),
        (3 * 2048 + np.arange(2048), _vals(rng, 2048)),                # all of wave segment 3
        (alld, (1 + alld * 7 % 255).astype(np.uint8)),                 # class end 32768
        (some, _vals(rng, some.size, 1, 40)),                          # segments 0, 5, 15 only
    ]
    return Case("b", terms, doc_hi=MAX_BLOCK_DOCS)


def _case_c():
    """Two blocks, nd = 32769 (bd = 16448, S = 1028)."""
    rng = np.random.default_rng(13)
    both = np.sort(np.concatenate([rng.choice(32768, 299, replace=False), [32768]]))
    hi_only = 16448 + np.sort(rng.choice(32769 - 16448, 150, replace=False))
    terms = [
        (both, np.sort(_vals(rng, 300))[::-1]),
        (hi_only, np.sort(_vals(rng, 150))[::-1]),
        ([], []),
        ([3, 16447, 16448, 20000, 32768], [9, 9, 8, 2, 1]),
    ] + _filler(rng, 14, 0, 32769)
    return Case("c", terms, doc_hi=32769)


def _case_d():
    """Nine blocks, nd = 8 * 32768 + 1."""
    rng = np.random.default_rng(14)
    nd = 8 * MAX_BLOCK_DOCS + 1
    nb, bd = blocks_of(nd)
    assert nb == 9

    def in_blocks(blocks, per):
        d = np.concatenate([b * bd + rng.choice(min(bd, nd - b * bd), per, replace=False)
                            for b in blocks])
        return np.sort(d)
    every = in_blocks(range(9), 25)
    big = np.sort(np.concatenate([1 * bd + rng.choice(bd, 3000, replace=False),
                                  6 * bd + rng.choice(bd, 2000, replace=False)]))
    terms = [
        (every, np.sort(_vals(rng, every.size))[::-1]),       # find_entry's direct index
        (in_blocks([0, 4, 8], 1), [200, 100, 50]),            # binary search
        (in_blocks([2, 7], 40), np.sort(_vals(rng, 80))[::-1]),
        (in_blocks([3, 5, 6], 130), np.sort(_vals(rng, 390))[::-1]),
        (big, np.sort(_vals(rng, big.size))[::-1]),
    ] + _filler(rng, 13, 0, nd)
    return Case("d", terms, doc_hi=nd)


def _case_e_range():
    """doc_lo > 0, postings on both sides of the range, a CSR that starts at posting 3."""
    rng = np.random.default_rng(15)
    d = np.sort(rng.choice(60000, 400, replace=False))
    terms = [
        (d, np.sort(_vals(rng, 400))[::-1]),
        ([10, 999, 1000, 39999, 40000, 59999], [6, 5, 4, 3, 2, 1]),
        ([500, 45000], [3, 3]),                                # nothing in range
    ] + _filler(rng, 15, 0, 60000)
    return Case("e_range", terms, doc_lo=1000, doc_hi=40000, lead=3)


def _case_e_hi0():
    """doc_hi = 0 with the largest doc behind a zero value; a zero in mid-term; input not
    value-descending."""
    rng = np.random.default_rng(16)
    terms = [
        ([10, 99999, 20, 30], [5, 0, 9, 7]),                   # the zero holds the largest doc
        (np.arange(50) * 1999, np.arange(1, 51)),              # ascending values
        (np.arange(200) * 311, np.r_[_vals(rng, 120), 0, _vals(rng, 79)]),   # cut at 120
        ([0], [0]),                                            # starts with the zero: empty
    ] + _filler(rng, 14, 0, 90000)
    return Case("e_hi0", terms)


def _case_e_out():
    """All postings out of the range: nb comes from the range, no entries."""
    return Case("e_out", [([1, 2, 49999], [3, 2, 1]), ([], []), ([17], [1])],
                doc_lo=50000, doc_hi=120000)


CASES = {c.name: c for c in (
    _case_a(), _case_b(), _case_c(), _case_d(), _case_e_range(), _case_e_hi0(), _case_e_out(),
    Case("e_empty", []),
)}
ENV_CASES = ("a", "b", "c")        # (f): these again under every other environment
SEARCH_CASES = ("c", "d", "e_range", "e_hi0")
ALL = [(n, "default") for n in CASES] + [(n, e) for n in ENV_CASES for e in ENVS if e != "default"]


def queries(case, n=36, seed=5):
    """A few dozen seeded queries (distinct terms each), a 17-term one among them -> (flat
    term ids, cu)."""
    rng = np.random.default_rng(seed)
    nt = case.n_terms
    assert nt >= 17
    qs = [rng.choice(nt, int(rng.integers(1, 7)), replace=False) for _ in range(n - 3)]
    qs += [rng.choice(nt, 17, replace=False), np.arange(min(nt, 5)), np.array([0])]
    cu = np.cumsum([0] + [len(q) for q in qs]).astype(np.int32)
    return np.concatenate(qs).astype(np.uint32), cu
