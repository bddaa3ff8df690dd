"""di_pairwise_order on the GPU, on constructed arrays (no encoder): the entry order of
DeepPairwiseImpact.compute_term_impacts (reference pairwise_impact.py:98-129) against
models.pairwise_entries -- offsets, single / pair flags, indices and score bits all equal --
and, on the small cases, against the plain loops of pairwise_cases.restated_term_impacts.

The cases cover ties, the round-to-0.000 filter's boundary, map positions that are a
permutation, degenerate documents, every route of the ordering at its boundaries (one
workgroup up to DI_PAIR_ORDER_LDS_KEYS entries, sorted runs and merge passes above), batch
invariance and the calling forms.  Everything is exact equality."""
import ctypes
import functools

import numpy as np
import pytest
import torch

import pairwise_cases as P

pytestmark = pytest.mark.gpu

U1 = np.float32(0.0005)  # fl32(0.0005) * 1000 is exactly 0.5: rint gives 0, dropped


def _lib():
    from improving_learned_index_amd import _lib as L

    if L.device_count() < 1:
        pytest.fail("no HIP device visible (GPU test run without a GPU)")
    return L


K = 16384  # DI_PAIR_ORDER_LDS_KEYS (test_entry_lines_cpu checks the header's value)


def make(Ts, seed, values=None, perm=False):
    """A batch of documents with Ts terms each: singles and pairs drawn from `values`
    (default: distinct-ish floats in [0.001, 8), all kept), positions a random permutation
    per document when perm."""
    rng = np.random.default_rng(seed)
    Ts = np.asarray(Ts, np.int64)
    ct = np.zeros(len(Ts) + 1, np.int32)
    ct[1:] = np.cumsum(Ts)
    cp = np.zeros(len(Ts) + 1, np.int64)
    cp[1:] = np.cumsum(Ts * (Ts - 1) // 2)

    def draw(n):
        if values is None:
            x = rng.random(n, np.float32) * np.float32(7.9) + np.float32(0.001)
            return x.astype(np.float32)
        return np.asarray(values, np.float32)[rng.integers(0, len(values), n)]

    pos = None
    if perm:
        pos = np.concatenate([rng.permutation(int(t)) for t in Ts] + [np.zeros(0, np.int64)])
        pos = pos.astype(np.int32)
    return {"single": draw(int(ct[-1])), "pair": draw(int(cp[-1])), "ct": ct, "cp": cp, "pos": pos}


def trim(c, d, entries, seed=0):
    """Zero random pairs of document d until it has exactly `entries` entries."""
    T = int(c["ct"][d + 1] - c["ct"][d])
    seg = c["pair"][c["cp"][d]:c["cp"][d + 1]]
    assert (P_round3(seg) != 0).all() and T <= entries <= T + len(seg)
    drop = np.random.default_rng(seed).choice(len(seg), T + len(seg) - entries, replace=False)
    seg[drop] = 0
    return c


def P_round3(x):
    from improving_learned_index_amd.models import round3

    return round3(x)


def sub(c, d):
    """Document d of batch c alone."""
    t0, t1, p0, p1 = c["ct"][d], c["ct"][d + 1], c["cp"][d], c["cp"][d + 1]
    return {"single": c["single"][t0:t1], "pair": c["pair"][p0:p1],
            "ct": np.array([0, t1 - t0], np.int32), "cp": np.array([0, p1 - p0], np.int64),
            "pos": None if c["pos"] is None else c["pos"][t0:t1]}


def by_tok(c):
    """Global sorted-term index -> global map index."""
    n = int(c["ct"][-1])
    doc0 = np.repeat(c["ct"][:-1].astype(np.int64), np.diff(c["ct"]))
    return doc0 + (np.arange(n) - doc0 if c["pos"] is None else c["pos"].astype(np.int64))


def reference(c):
    """models.pairwise_entries on the batch in map order: the term at map position
    pos[r] has token index r."""
    from improving_learned_index_amd.models import pairwise_entries

    n = int(c["ct"][-1])
    bt = by_tok(c)
    doc0 = np.repeat(c["ct"][:-1].astype(np.int64), np.diff(c["ct"]))
    tt = np.empty(n, np.int64)
    single = np.empty(n, np.float32)
    tt[bt] = np.arange(n) - doc0
    single[bt] = c["single"]
    return pairwise_entries(tt, c["ct"], single, c["pair"], c["cp"])


def run(c, round3=False, device=False):
    L = _lib()
    if not device:
        return L.pairwise_order(c["single"], c["pair"], c["ct"], c["cp"], c["pos"], round3=round3)
    t = {k: (None if v is None else torch.from_numpy(np.ascontiguousarray(v)).cuda())
         for k, v in c.items()}
    out = L.pairwise_order(t["single"], t["pair"], t["ct"], t["cp"], t["pos"], round3=round3)
    torch.cuda.synchronize()
    return tuple(x.cpu().numpy() for x in out)


def check(c, got=None, round3=False, device=False):
    cu, first, second, score = run(c, round3, device) if got is None else got
    wcu, wpair, wfirst, wsecond, wscore = reference(c)
    bt = by_tok(c)
    assert cu.dtype == np.int64 and first.dtype == second.dtype == np.int32
    assert cu.tolist() == wcu.tolist()
    assert len(first) == len(second) == len(score) == wcu[-1]
    assert ((second >= 0) == wpair).all()
    assert (bt[first] == wfirst).all()
    assert (bt[second[wpair]] == wsecond[wpair]).all() and (second[~wpair] == -1).all()
    if round3:
        wscore = P_round3(wscore)
    assert score.view(np.uint32).tolist() == wscore.view(np.uint32).tolist()
    return cu, first, second, score


def check_restated(c, got):
    """The same entries from the plain loops of the test helpers, by name."""
    cu, first, second, score = got
    bt = by_tok(c)
    ct, cp = c["ct"], c["cp"]
    maps, tok, pairs = [], [], []
    for d in range(len(ct) - 1):
        T = ct[d + 1] - ct[d]
        rank = np.empty(T, np.int64)  # map position -> token index (the sorted rank)
        rank[bt[ct[d]:ct[d + 1]] - ct[d]] = np.arange(T)
        maps.append({f"t{ct[d] + k}": int(rank[k]) for k in range(T)})
        tok.append({r: c["single"][ct[d] + r] for r in range(T)})
        pairs.append(c["pair"][cp[d]:cp[d + 1]])
    want = P.restated_term_impacts(maps, tok, pairs)
    for d in range(len(ct) - 1):
        names = [f"t{bt[f]}" if s < 0 else f"t{bt[f]}|t{bt[s]}"
                 for f, s in zip(first[cu[d]:cu[d + 1]], second[cu[d]:cu[d + 1]])]
        assert names == [n for n, _ in want[d]]
        assert score[cu[d]:cu[d + 1]].tobytes() == np.array([v for _, v in want[d]],
                                                              np.float32).tobytes()


# ----------------------------------------------------------------------------- ties
def test_all_scores_equal():
    c = make([1, 9, 40, 0, 64], 1, values=[0.25])
    check_restated(c, check(c))
    c = make([30, 7], 2, values=[0.25], perm=True)
    check_restated(c, check(c))


def test_singles_equal_to_pairs_come_first_then_combination_order():
    c = make([6], 3, values=[0.5])
    cu, first, second, _ = check(c)
    assert second[:6].tolist() == [-1] * 6 and first[:6].tolist() == list(range(6))
    from itertools import combinations
    assert list(zip(first[6:].tolist(), second[6:].tolist())) == list(combinations(range(6), 2))


def test_eight_distinct_values_at_a_large_size():
    vals = [0.001, 0.0015, 0.25, 0.5, 1.0, 1.0000001, 3.0, 7.5]
    c = make([300, 20, 181], 4, values=vals, perm=True)  # 45150 entries: three runs, merged
    check(c)
    check(c, round3=True)


# ----------------------------------------------------------------------------- filter
def boundary_values():
    b = U1.view(np.uint32)
    return (np.arange(-8, 9) + int(b)).astype(np.uint32).view(np.float32)


def test_filter_boundary_and_special_values():
    v = boundary_values()
    kept = P_round3(v) != 0
    assert not kept[8] and kept[9] and kept.any() and (~kept).any()  # fl32(0.0005) itself: dropped
    special = np.array([0.0, -0.0, 1e-40, -1e-40, 1.4e-45, -0.0004, -0.002, 0.0004999, 0.002,
                        1e-3, 1.5], np.float32)
    vals = np.concatenate([v, special])
    c = make([12, 40, 3, 25], 5, values=vals, perm=True)
    # negative singles, signed zeros and denormals among the singles too (drawn from vals);
    # document 2: every pair dropped
    c["pair"][c["cp"][2]:c["cp"][3]] = [0.0, -0.0, U1]
    c["single"][c["ct"][2]:c["ct"][3]] = [-1.5, -0.0, 0.0]
    got = check(c)
    assert got[0][3] - got[0][2] == 3
    assert 0 < (got[0][2] - got[0][1]) - 40 < 40 * 39 // 2  # some kept, some dropped
    check_restated(c, got)
    check(c, round3=True)
    check(c, device=True)


# ----------------------------------------------------------------------------- positions
def test_single_pos_permutation():
    c = make([17, 1, 2, 64, 33], 6, values=[0.1, 0.2, 0.2, 0.3, 0.0004], perm=True)
    assert (c["pos"][:17] != np.arange(17)).any()
    check_restated(c, check(c))
    check(c, device=True)


# ----------------------------------------------------------------------------- degenerate
def test_degenerate_documents():
    c = make([0, 1, 2, 0, 0, 2, 1, 0], 7, values=[0.3, 0.0001, 0.3])
    check_restated(c, check(c))
    c = make([0, 0], 7)
    cu, first, second, score = check(c)
    assert cu.tolist() == [0, 0, 0] and len(first) == 0
    c = make([], 7)
    assert run(c)[0].tolist() == [0]


def test_three_thousand_small_documents():
    rng = np.random.default_rng(8)
    c = make(rng.integers(0, 13, 3000), 8, values=[0.0, 0.0004, 0.001, 0.5, 0.5, 2.0], perm=True)
    check(c)


# ----------------------------------------------------------------------------- routes
@functools.lru_cache(maxsize=None)
def route_case(name):
    if name in ("lds-1", "lds", "lds+1"):  # 181 terms: 16471 entries before trimming
        return trim(make([181], 10), 0, K + {"lds-1": -1, "lds": 0, "lds+1": 1}[name])
    if name == "small-edge":  # the 256-thread kernel's last size and the next
        c = make([64, 64, 3], 11)  # 2080 entries each before trimming
        return trim(trim(c, 0, 2048), 1, 2049)
    if name == "two-runs+1":
        return trim(make([256], 12, perm=True), 0, 2 * K + 1)
    if name == "three-runs":
        return trim(make([314], 13), 0, 3 * K)
    if name == "nine-runs":  # 8 K + 200 entries: 9 runs, 4 merge passes, the last run short
        return trim(make([512], 14), 0, 8 * K + 200)
    if name == "t1232":  # everything kept: 759528 entries, 47 runs
        return make([1232], 15, values=[0.001, 0.5, 0.75, 1.0, 1.25, 2.0, 4.0, 6.5])
    if name == "mixed":
        c = make([5, 181, 256, 0, 60, 70, 400, 1, 200], 16, perm=True)
        return trim(trim(c, 1, K), 6, 4 * K + 7)
    raise KeyError(name)


ROUTES = ["lds-1", "lds", "lds+1", "small-edge", "two-runs+1", "three-runs", "nine-runs", "t1232",
          "mixed"]


@pytest.mark.parametrize("name", ROUTES)
def test_route_boundaries(name):
    c = route_case(name)
    cu, *_ = check(c)
    n = np.diff(cu)
    want = {"lds-1": [K - 1], "lds": [K], "lds+1": [K + 1], "small-edge": [2048, 2049, 6],
            "two-runs+1": [2 * K + 1], "three-runs": [3 * K], "nine-runs": [8 * K + 200],
            "t1232": [759528],
            "mixed": [15, K, 256 * 257 // 2, 0, 1830, 2485, 4 * K + 7, 1, 20100]}[name]
    assert n.tolist() == want


def test_batch_invariance_across_routes():
    c = route_case("mixed")
    cu, first, second, score = run(c, round3=True)
    for d in range(len(c["ct"]) - 1):
        one = sub(c, d)
        cu1, f1, s1, sc1 = check(one, round3=True)
        sl = slice(cu[d], cu[d + 1])
        assert cu1[-1] == cu[d + 1] - cu[d]
        assert (f1 + c["ct"][d] == first[sl]).all()
        assert (np.where(s1 >= 0, s1 + c["ct"][d], -1) == second[sl]).all()
        assert sc1.tobytes() == score[sl].tobytes()


# ----------------------------------------------------------------------------- calling forms
def test_device_pointer_form_equals_host_form():
    c = route_case("mixed")
    host = run(c)
    dev = run(c, device=True)
    for a, b in zip(host, dev):
        assert a.dtype == b.dtype and a.tobytes() == b.tobytes()
    c2 = make([9, 0, 30], 17)  # identity positions
    for a, b in zip(run(c2, round3=True), run(c2, round3=True, device=True)):
        assert a.tobytes() == b.tobytes()


def _raw(L, c, cap, guard, device):
    """di_pairwise_order with entry arrays of cap + guard elements filled with a sentinel;
    returns (rc, n_out, cu_out, first, second, score bits) as numpy arrays."""
    n_docs = len(c["ct"]) - 1
    n = ctypes.c_int64(-1)
    size = cap + guard
    if device:
        t = {k: (None if v is None else torch.from_numpy(np.ascontiguousarray(v)).cuda())
             for k, v in c.items()}
        cu = torch.full((n_docs + 1,), -7, dtype=torch.int64, device="cuda")
        first = torch.full((size,), -77, dtype=torch.int32, device="cuda")
        second = torch.full((size,), -77, dtype=torch.int32, device="cuda")
        score = torch.full((size,), -77.0, dtype=torch.float32, device="cuda")
        flags = L.DI_F_DEVICE_PTRS
    else:
        t = c
        cu = np.full(n_docs + 1, -7, np.int64)
        first, second = np.full(size, -77, np.int32), np.full(size, -77, np.int32)
        score = np.full(size, -77.0, np.float32)
        flags = 0
    rc = L.lib().di_pairwise_order(L.ptr(t["single"]), L.ptr(t["pair"]), L.ptr(t["ct"]),
                                   L.ptr(t["cp"]), L.ptr(t["pos"]), n_docs, len(c["single"]),
                                   len(c["pair"]), L.ptr(cu), L.ptr(first), L.ptr(second),
                                   L.ptr(score), cap, ctypes.byref(n), 0, None, flags)
    if device:
        torch.cuda.synchronize()
        cu, first, second, score = (x.cpu().numpy() for x in (cu, first, second, score))
    return rc, n.value, cu, first, second, score


@pytest.mark.parametrize("device", [False, True])
def test_out_cap_and_guard_region(device):
    L = _lib()
    c = route_case("mixed")
    want = run(c)
    total = len(want[1])
    # too small: DI_ERANGE, the size needed, the offsets, and no entry written anywhere
    for cap in (0, 100, total - 1):
        rc, n, cu, first, second, score = _raw(L, c, cap, 64, device)
        assert rc == L.DI_ERANGE and n == total
        assert cu.tolist() == want[0].tolist()
        assert (first == -77).all() and (second == -77).all() and (score == -77.0).all()
    # exactly enough: the entries, and the guard behind them untouched
    rc, n, cu, first, second, score = _raw(L, c, total, 64, device)
    assert rc == 0 and n == total
    assert first[:n].tobytes() == want[1].tobytes() and second[:n].tobytes() == want[2].tobytes()
    assert score[:n].tobytes() == want[3].tobytes()
    assert (first[n:] == -77).all() and (second[n:] == -77).all() and (score[n:] == -77.0).all()
    with pytest.raises(L.DIError) as e:
        L.pairwise_order(c["single"], c["pair"], c["ct"], c["cp"], c["pos"], out_cap=10)
    assert e.value.code == L.DI_ERANGE and e.value.needed == total


@pytest.mark.parametrize("device", [False, True])
def test_inconsistent_offsets_are_refused(device):
    L = _lib()
    good = make([9, 4, 30], 18, perm=True)
    for change in ("cp_mid", "cp_end", "ct_end", "pos"):
        c = {k: (None if v is None else v.copy()) for k, v in good.items()}
        if change == "cp_mid":
            c["cp"][1] += 1
        elif change == "cp_end":
            c["cp"][-1] -= 1
        elif change == "ct_end":
            c["ct"][-1] -= 1
        else:
            c["pos"][10] = 4  # outside document 1's four terms
        rc, n, cu, first, second, score = _raw(L, c, 1000, 8, device)
        assert rc == -1, change  # DI_EINVAL
        assert (first == -77).all() and (score == -77.0).all()
    check(good, device=device)  # and the next call is right
    if not device:  # more terms than a key holds: a documented limit
        big = make([L.DI_PAIR_ORDER_MAX_TERMS + 1], 19, values=[0.0])
        with pytest.raises(L.DIError) as e:
            run(big)
        assert e.value.code == L.DI_ERANGE
