"""The constructed cases of tests/index_layout_cases.py, checked on the CPU: the restatement
of build_index() gives a consistent layout (every run a permutation of its group, class
prefixes, seg / wmeta / emax / wmax agree with the postings), and each case reaches the
branch of the layout code it was built for (the census).  The GPU test
(test_index_layout_gpu.py) then only has to compare bytes."""
import numpy as np
import pytest

import index_layout_cases as C


def _groups(case, lay):
    """(term, block) -> sorted (doc_in_block, value) pairs, straight from the kept postings."""
    kept, _ = case.kept()
    bd = lay["block_docs"]
    out = {}
    for t, (rel, val) in enumerate(kept):
        for r, v in zip(rel.tolist(), val.tolist()):
            out.setdefault((t, r // bd), []).append((r % bd, v))
    return {k: sorted(v) for k, v in out.items()}


def _classes(val):
    return 7 - np.floor(np.log2(val)).astype(np.int64)


@pytest.mark.parametrize("name, env", C.ALL)
def test_restatement_is_a_consistent_layout(name, env):
    case = C.CASES[name]
    lay, _ = C.reference(name, env)
    groups = _groups(case, lay)
    nb, bd = lay["nb"], lay["block_docs"]
    S = -(-bd // C.WSEG)
    assert lay["n_ent"] == len(groups) and lay["n_post"] == sum(map(len, groups.values()))
    assert lay["tb_start"].size == case.n_terms + 1 and lay["tb_start"][-1] == lay["n_ent"]
    assert lay["epos"][-1] == lay["n_post"]
    doc, val = C.decode(lay["post"])
    fdoc, fval = C.decode(lay["post_flat"]) if lay["has_flat"] else (doc, val)
    e = 0
    for t in range(case.n_terms):
        blocks = sorted(b for (tt, b) in groups if tt == t)
        assert lay["tb_start"][t] == e
        for b in blocks:
            assert lay["eblk"][e] == b and b < nb
            s0, s1 = int(lay["epos"][e]), int(lay["epos"][e + 1])
            want = groups[(t, b)]
            assert sorted(zip(doc[s0:s1].tolist(), val[s0:s1].tolist())) == want
            assert lay["emax"][e] == max(v for _, v in want)
            cls = _classes(val[s0:s1])
            counts = np.cumsum(np.bincount(cls, minlength=8)) & 0xFFFF
            assert lay["seg"][8 * e:8 * e + 8].tolist() == counts.tolist()
            if s1 - s0 < lay["wlong_min"]:
                assert lay["lid"][e] == C.NO
                assert np.all(np.diff(cls) >= 0)              # classes in order
                assert np.array_equal(fdoc[s0:s1], doc[s0:s1])  # flat = a copy
                assert np.array_equal(fval[s0:s1], val[s0:s1])
            else:
                i = int(lay["lid"][e])
                assert i != C.NO
                a = 0
                for w in range(C.WSEG):
                    m = lay["wmeta"][i * 128 + 8 * w:i * 128 + 8 * w + 8].astype(np.int64)
                    z = int(m[7])
                    z += 65536 if z < a else 0                 # (32768 fits; kept general)
                    run = slice(s0 + a, s0 + z)
                    assert np.all(np.minimum(doc[run] // S, C.WSEG - 1) == w)
                    rc = _classes(val[run])
                    assert np.all(np.diff(rc) >= 0)
                    ends = a + np.cumsum(np.bincount(rc, minlength=8))
                    assert (ends & 0xFFFF).tolist() == m.tolist()
                    assert lay["wmax"][i * 16 + w] == (val[run].max() if z > a else 0)
                    assert sorted(zip(fdoc[run].tolist(), fval[run].tolist())) == \
                        sorted(zip(doc[run].tolist(), val[run].tolist()))
                    a = z
                assert a == s1 - s0
            e += 1
    assert e == lay["n_ent"]
    assert lay["n_long"] == int(np.sum(lay["lid"] != C.NO))
    assert np.array_equal(lay["lid"][lay["lid"] != C.NO], np.arange(lay["n_long"]))


def test_census_each_case_hits_its_branch():
    a, b, c, d = (C.reference(n)[1] for n in "abcd")
    # (a): the one-bank sublists fall back on every pick after a set's first; a cursor goes
    # over a class boundary; short sublists of exactly these lengths
    assert a["fallback"] >= 30 and a["cursor_carry"] >= 1
    assert {1, 31, 32, 33, 127} <= a["entry_lens"] and max(a["entry_lens"]) < C.WLONG_MIN
    assert C.reference("a")[0]["n_long"] == 0 and C.reference("a")[0]["nb"] == 1
    # (b): entries at 127, 128 and 129; a full segment, the full block; used sets reset
    # inside a class (a run of more than 128 postings of one class)
    assert {127, 128, 129, 2048, 32768} <= b["entry_lens"]
    assert b["reset_in_class"] >= 1 and b["cursor_carry"] >= 1
    lay_b = C.reference("b")[0]
    assert lay_b["n_long"] == 5 and lay_b["nb"] == 1 and lay_b["block_docs"] == 32768
    assert 32768 in lay_b["seg"].tolist()                       # a class end of 2^15
    some = lay_b["wmeta"][4 * 128:5 * 128].reshape(16, 8)[:, 7].astype(np.int64)
    assert np.sum(np.diff(np.r_[0, some]) == 0) == 13           # empty segments
    # (c): two blocks of 16448 docs; a term in both, one in block 1 only, one without postings
    lay_c = C.reference("c")[0]
    assert (lay_c["nb"], lay_c["block_docs"]) == (2, 16448)
    ts = lay_c["tb_start"].astype(np.int64)
    assert ts[1] - ts[0] == 2 and ts[2] - ts[1] == 1 and lay_c["eblk"][ts[1]] == 1
    assert ts[3] - ts[2] == 0 and lay_c["n_long"] >= 2
    # (d): nine blocks; a direct-index term and binary-search terms
    lay_d = C.reference("d")[0]
    assert lay_d["nb"] == 9 and d["direct_terms"] >= 1 and d["search_terms"] >= 3
    td = lay_d["tb_start"].astype(np.int64)
    assert td[1] - td[0] == 9 and lay_d["eblk"][td[1]:td[2]].tolist() == [0, 4, 8]
    # (f): with 4-byte deal sets the used set resets inside the classes of short sublists
    assert C.reference("a", "x4off")[1]["reset_in_class"] >= 1
    assert C.reference("a", "wlong1")[0]["n_long"] == C.reference("a")[0]["n_ent"]
    assert 0 < C.reference("a", "wlong64")[0]["n_long"] < C.reference("a")[0]["n_ent"]
    assert C.reference("b", "classes")[0]["post_flat"] is None


def test_edge_cases_are_what_they_say():
    r = C.reference("e_range")[0]
    case = C.CASES["e_range"]
    assert case.term_off[0] == 3 and (r["n_docs"], r["nb"]) == (39000, 2)
    kept, _ = case.kept()
    assert kept[1][0].tolist() == [0, 38999] and kept[2][0].size == 0
    h = C.reference("e_hi0")[0]
    k0, hi = C.CASES["e_hi0"].kept()
    assert hi == 100000 and h["nb"] == 4                        # the doc behind the zero counts
    assert k0[0][0].tolist() == [10] and k0[2][0].size == 120 and k0[3][0].size == 0
    assert np.any(np.diff(k0[1][1]) > 0)                        # not value-descending
    o = C.reference("e_out")[0]
    assert (o["nb"], o["n_ent"], o["n_post"]) == (3, 0, 0)
    z = C.reference("e_empty")[0]
    assert (z["nb"], z["n_ent"], z["tb_start"].tolist()) == (0, 0, [0])
    for name in C.SEARCH_CASES:
        q, cu = C.queries(C.CASES[name])
        assert 17 in np.diff(cu).tolist() and q.max() < C.CASES[name].n_terms
