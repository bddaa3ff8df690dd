"""The cases of tests/test_exchange_world_gpu.py and the exchange's definition in numpy.

A case is (world, k, g, n_q, mode): `world` ranks each hold, per query, up to k unique u64
merge keys sorted descending (test_exchange_cpu._lists), sampled every g keys.  DIRECT
cases (g free) call the di_xchg_* kernels one by one; PRODUCTION cases go through
parallel.exchange_topk on device tensors with g from its own formula.  What each case is
there to reach (the sample count against the 1024 registers of xchg_count_kernel, the
queries per thread of xchg_offsets_kernel, T_q = 0, emax = 0, padding, clamped and
rejected counts) is asserted without a GPU by test_exchange_cases_cpu.py.

definition() restates parallel.exchange_topk's docstring, vectorised over ranks and
queries: samples at positions g-1, 2g-1, ...; T_q = the ceil(k/g)-th largest sample of the
union (0 when the union holds fewer than that many nonzero samples: every key passes);
e = each rank's valid keys >= T_q; offsets, totals and the padded size emax of round 2;
each rank's packed buffer; the prefixes every rank ends up with and their counts.
"""
from types import SimpleNamespace

import numpy as np

from test_exchange_cpu import _lists, _merge  # noqa: F401  (_merge: for the tests)

XR_SAMPLES = 1024  # 64 lanes x XR = 16 sample registers (exchange.hip: xchg_count_kernel)
XS_T = 1024        # threads of xchg_offsets_kernel
SIGN = np.uint64(1 << 63)

MODES = ("iid", "ragged", "short", "empty", "rank1_empty", "clamped")

# (world, k, g, n_q, mode)
DIRECT = [
    (16, 256, 4, 6, "iid"),         # 1024 samples: register route, last row full
    (17, 256, 4, 6, "iid"),         # 1088 samples: re-read route
    (25, 82, 2, 6, "iid"),          # 1025 samples: first size on the re-read route
    (8, 250, 2, 6, "iid"),          # 1000 samples: last register row partly filled
    (1, 10, 3, 7, "iid"),           # 3 samples < need 4: T_q = 0, every key passes
    (4, 64, 8, 9, "short"),         # every count < g: enough samples, all zero, T_q = 0
    (3, 40, 3, 1029, "ragged"),     # per = 2, last thread ragged, n_q % 4 == 1
    (4, 16, 2, 2051, "iid"),        # per = 3; threads past q0 == n_q
    (2, 32, 4, 1024, "iid"),        # per = 1 with every thread busy
    (2, 100, 25, 5, "empty"),       # every list empty: emax == 0, gathered == NULL
    (3, 100, 8, 24, "rank1_empty"),  # padding behind tot[r]; a zero total between others
    (2, 50, 5, 24, "clamped"),      # counts k + 5 and one -1; keys past the sign bit
]


def production_g(world, k):
    """parallel.exchange_topk's sample stride."""
    return max(1, min(64, k // (4 * world)))


# (world, k, n_q, mode, pruned): exchange_topk(..., pruned=pruned), g = production_g
PRODUCTION = [
    (2, 200, 24, "iid", True),
    (8, 1000, 24, "ragged", True),
    (3, 40, 1029, "ragged", True),
    (4, 64, 2051, "iid", None),      # the automatic choice must pick pruned
    (8, 16, 5, "iid", True),         # g = 1: the plain path, on device tensors
    (2, 100, 5, "empty", True),
    (3, 100, 24, "rank1_empty", True),
    (2, 100, 0, "iid", True),        # no queries
]


def case_id(case):
    return "w{}-k{}-g{}-q{}-{}".format(*case)


def production_case(p):
    world, k, n_q, mode, _ = p
    return (world, k, production_g(world, k), n_q, mode)


def _lists_many(world, nq, k, seed, mode):
    """test_exchange_cpu._lists with the docs drawn from 4 k world ids, not 2^20: the same
    lists in kind (unique keys, few scores -> ties, sorted descending, ragged counts, keys
    past the sign bit, one rejected query) at a cost that allows thousands of queries."""
    rng = np.random.default_rng(seed)
    keys = np.zeros((world, nq, k), np.uint64)
    cnt = np.zeros((world, nq), np.int32)
    n_docs = 4 * k * world
    for q in range(nq):
        n_all = int(rng.integers(0, 3 * k * world)) if mode == "ragged" else n_docs
        score = rng.integers(1, 40, n_all).astype(np.uint64)
        if mode == "ragged" and q % 3 == 0:
            score |= np.uint64(1 << 31)
        doc = rng.permutation(n_docs)[:n_all].astype(np.uint64)
        allk = (score << np.uint64(32)) | (np.uint64(0xFFFFFFFF) - doc)
        owner = rng.integers(0, world, n_all)
        for r in range(world):
            mine = np.sort(allk[owner == r])[::-1][:k]
            keys[r, q, :mine.size] = mine
            cnt[r, q] = mine.size
    if mode == "ragged":
        cnt[0, 1 % nq] = -1
    return keys, cnt


_CACHE = {}


def case_lists(case):
    """(keys [world, n_q, k] uint64, counts [world, n_q] int32) of a case; computed once
    and shared (read-only)."""
    if case in _CACHE:
        return _CACHE[case]
    world, k, g, nq, mode = case
    assert mode in MODES
    seed = 1000 + 31 * world + 7 * k + nq
    base = "ragged" if mode == "ragged" else "iid"
    if nq == 0:
        keys, cnt = np.zeros((world, 0, k), np.uint64), np.zeros((world, 0), np.int32)
    elif nq <= 64:
        keys, cnt = _lists(world, nq, k, seed, base)
    else:
        keys, cnt = _lists_many(world, nq, k, seed, base)
    rng = np.random.default_rng(seed + 1)
    if mode == "short":  # fewer than g keys everywhere: no list reaches its first sample
        cnt = np.minimum(cnt, rng.integers(0, g, cnt.shape)).astype(np.int32)
        cnt[0, 0], cnt[1, 0] = g - 1, 0
        keys[np.arange(k)[None, None, :] >= cnt[:, :, None]] = 0
    elif mode == "empty":
        keys[:], cnt[:] = 0, 0
    elif mode == "rank1_empty":
        assert (cnt == k).all()  # (the others full)
        keys[1], cnt[1] = 0, 0
    elif mode == "clamped":
        assert (cnt == k).all()
        keys[:, ::3, :] |= SIGN  # order kept: every key of these queries moves past the sign
        cnt[0, 0] = cnt[1, 3] = cnt[0, 7] = k + 5
        cnt[0, 1] = -1
    keys.setflags(write=False)
    cnt.setflags(write=False)
    _CACHE[case] = (keys, cnt)
    return keys, cnt


def definition(keys, cnt, k, g):
    """The pruned exchange of [world, n_q, k] lists, every quantity the device steps
    produce (see the module docstring)."""
    world, nq, _ = keys.shape
    c = np.clip(cnt.astype(np.int64), 0, k)
    s_n, need = k // g, -(-k // g)
    pos = np.arange(1, s_n + 1) * g - 1
    samples = np.where(pos[None, None, :] < c[:, :, None], keys[:, :, pos], np.uint64(0))
    union = samples.transpose(1, 0, 2).reshape(nq, world * s_n)
    n_samples = world * s_n
    if n_samples >= need:
        T = np.sort(union, axis=1)[:, ::-1][:, need - 1].copy()
    else:
        T = np.zeros(nq, np.uint64)
    valid = np.arange(k)[None, None, :] < c[:, :, None]
    sel = valid & (keys >= T[None, :, None])  # (a prefix of each list: lists are sorted)
    e = sel.sum(2).astype(np.int64)
    assert (sel == (np.arange(k)[None, None, :] < e[:, :, None])).all()
    off = np.cumsum(e, 1) - e
    tot = e.sum(1)
    emax = int(tot.max()) if nq else 0
    packed = np.zeros((world, emax), np.uint64)
    for r in range(world):
        packed[r, :tot[r]] = keys[r][sel[r]]
    g_n = np.where(cnt < 0, cnt, e).astype(np.int32)
    return SimpleNamespace(
        world=world, n_q=nq, k=k, g=g, s_n=s_n, need=need, n_samples=n_samples,
        samples=samples, T=T, nonzero_samples=(union != 0).sum(1), e=e,
        ec=np.stack([e.astype(np.int32), cnt.astype(np.int32)], 1),  # [world, 2, n_q]
        off=off, tot=tot, emax=emax, packed=packed, prefix=sel, g_n=g_n)


def definition_plain(keys, cnt, k):
    """A plain all_gather: every list whole, the scorer's counts."""
    world, nq, _ = keys.shape
    sel = np.arange(k)[None, None, :] < np.clip(cnt, 0, k)[:, :, None]
    return SimpleNamespace(world=world, n_q=nq, k=k, prefix=sel, g_n=cnt.astype(np.int32))


def case_definition(case):
    key = ("def",) + case
    if key not in _CACHE:
        keys, cnt = case_lists(case)
        _CACHE[key] = definition(keys, cnt, case[1], case[2])
    return _CACHE[key]


def count_route(d):
    """The branch of xchg_count_kernel a definition's sample count takes."""
    if d.n_samples < d.need:
        return "too_few_samples"
    return "registers" if d.n_samples <= XR_SAMPLES else "reread"


def offsets_threads(n_q):
    """xchg_offsets_kernel's split of n_q queries over its threads -> (per, working
    threads, queries of the last working thread)."""
    per = -(-n_q // XS_T)
    if per == 0:
        return 0, 0, 0
    working = -(-n_q // per)
    return per, working, n_q - (working - 1) * per


def zero_T(d):
    """(queries with T_q == 0 because the union is too small, ... because it holds enough
    samples but fewer than need nonzero ones)."""
    if d.n_samples < d.need:
        assert (d.T == 0).all()
        return d.n_q, 0
    few = d.nonzero_samples < d.need
    assert ((d.T == 0) == few).all()
    return 0, int(few.sum())
