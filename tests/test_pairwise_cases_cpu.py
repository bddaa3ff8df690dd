"""What the inputs of tests/test_pairwise_gpu.py can see, from the float64 oracle alone
(conditions on the inputs, not measurements of the device), and the host logic of the
pairwise model: the combination index and compute_term_impacts, exact.

Shares found with these inputs (3601 pairs; the oracle's attn spans 1.3e-5 .. 0.71):
pairs scoring above 1e-3: 0.29; exactly 0: 0.71; of the positive pairs, moved by more than
1e-2 relative when attn is replaced by zero: 0.88, taken from one direction only: 0.40,
from the last layer only: 0.42, from head 0 instead of the mean over heads: 0.88.

The second half holds the same conditions, case by case, for the route cases of
tests/test_pairwise_routes_gpu.py (pairwise_cases.ROUTE_CASES): the shape facts each launch
route needs, the shares above, which layer holds the maximum (layers4), that the positions
show (bert), the tolerances, and the oracle's cost.  The figures found are in each test's
docstring."""
from itertools import combinations

import numpy as np
import pytest

import pairwise_cases as P


def test_inputs_have_the_stated_shape():
    tt, ct = P.terms(P.LENS)
    assert np.diff(ct).tolist() == [48, 17, 65, 16, 0, 17, 2, 1]
    assert P.n_pairs(ct) == 3601
    assert tt[0] == 0 and tt[47] == 511
    for d in range(len(P.LENS)):
        seg = tt[ct[d]:ct[d + 1]]
        assert (np.diff(seg) > 0).all() and (seg < P.LENS[d]).all()


def test_oracle_can_show_a_wrong_kernel():
    o = P.oracle(variants=True)
    _, attn, pre, score = o["full"]
    print(f"attn spans {attn.min():.3g} .. {attn.max():.3g}")
    pos = score > 1e-3
    shares = {"positive": pos.mean(), "exactly_zero": (score == 0).mean()}
    for v in P.VARIANTS:
        shares[v] = (np.abs(o[v][3][pos] - score[pos]) > 1e-2 * score[pos]).mean()
    print({k: round(float(x), 3) for k, x in shares.items()})
    assert shares["positive"] >= 1 / 4
    assert shares["exactly_zero"] >= 1 / 10
    assert shares["exactly_zero"] == pytest.approx((pre <= 0).mean())
    assert shares["zero"] >= 1 / 2            # attn replaced by zero
    assert shares["one_direction"] >= 1 / 4
    assert shares["last_layer"] >= 1 / 4
    assert shares["head0"] >= 1 / 2


def test_pair_atol_is_below_half_a_printed_step():
    for kind in ("fp32", "bf16x3"):
        a = P.pair_atol(kind)
        print(kind, "atol", a)
        assert 0 < a < 5e-4


@pytest.mark.parametrize("T", [2, 3, 4, 17, 65, 91, 512])
def test_combination_index_is_itertools_order(T):
    from improving_learned_index_amd.models import pair_ab, pair_index

    want = np.array(list(combinations(range(T), 2)), np.int64)
    j = np.arange(len(want))
    assert (pair_index(want[:, 0], want[:, 1], T) == j).all()
    a, b = pair_ab(j, T)
    assert (a == want[:, 0]).all() and (b == want[:, 1]).all()


def test_combination_index_inverse_at_large_T():
    from improving_learned_index_amd.models import pair_ab, pair_index

    T = 100_003  # the float root is inexact here: the fix-up steps run
    rng = np.random.default_rng(0)
    a = rng.integers(0, T - 1, 20000)
    a[:3] = [0, T - 2, T - 3]
    b = a + 1 + rng.integers(0, T - 1 - a)
    ga, gb = pair_ab(pair_index(a, b, T), T)
    assert (ga == a).all() and (gb == b).all()


def test_compute_term_impacts_is_the_reference_loop():
    """Filter, names and the stable descending order on made-up float32 scores with ties,
    exact zeros, values that round to 0.000 (and one just above), a negative zero, maps
    that are not in token order, a document without terms and one with a single term."""
    from improving_learned_index_amd.models import DeepPairwiseImpact

    f = np.float32
    maps = [{"b": 5, "a": 2, "c": 9, "d": 7},          # not in token order
            {},
            {"x": 0},
            {"p": 1, "q": 2, "r": 3, "s": 4, "t": 6}]
    S = 10
    tok = np.zeros((4, S, 1), np.float32)
    tok[0, [2, 5, 7, 9], 0] = [0.25, 0.25, 0.0, 1.5]      # a tie between a and b
    tok[2, 0, 0] = 0.0004
    tok[3, [1, 2, 3, 4, 6], 0] = [0.5, 0.125, 0.5, 0.0, 0.125]
    pairs = [np.array([0.25, 0.00049, 0.0, 0.0005, 0.00051, 2.0], np.float32),
             np.zeros(0, np.float32),
             np.zeros(0, np.float32),
             np.array([0.5, 0.5, -0.0, 0.125, 0.0004, 0.125, 0.0, 0.5, 1e-9, 0.001],
                      np.float32)]
    want = P.restated_term_impacts(maps, tok[..., 0], pairs)
    got = DeepPairwiseImpact.compute_term_impacts(maps, (tok, [p.reshape(-1, 1) for p in pairs],
                                                        None))
    assert [[t for t, _ in d] for d in got] == [[t for t, _ in d] for d in want]
    for g, w in zip(got, want):
        assert [f(v).tobytes() for _, v in g] == [f(v).tobytes() for _, v in w]
    # the cases are in there: a kept pair, a dropped one, pair names in token order
    names = [t for t, _ in got[0]]
    assert "a|b" in names and "b|a" not in names and len(names) < 4 + 6
    assert got[1] == [] and [t for t, _ in got[2]] == ["x"]
    # and the lines go through the native formatter as the reference prints them
    from improving_learned_index_amd import _lib
    from improving_learned_index_amd.models import round3

    text = _lib.format_impact_lines([[t for t, _ in d] for d in got],
                                    [round3(np.array([v for _, v in d], np.float32)) for d in got])
    assert text == P.restated_lines(want)


# ---- the route cases of tests/test_pairwise_routes_gpu.py ----

ROUTES = list(P.ROUTE_CASES)


def _T(name):
    return np.diff(np.array(P.ROUTE_CASES[name].terms[1], np.int64))


def _lds_bytes(n, T):
    """pair_attn_kernel's LDS, restated: a [16][ceil16(n) + 4] score panel, [16][T] head
    sums and [T] term columns, 4 bytes each."""
    return (16 * ((n + 15) // 16 * 16 + 4) + 16 * T + T) * 4


@pytest.mark.parametrize("name", ROUTES)
def test_route_terms_are_valid(name):
    c = P.ROUTE_CASES[name]
    tt, ct = (np.array(t) for t in c.terms)
    assert len(ct) == len(c.lens) + 1 and ct[0] == 0 and ct[-1] == len(tt)
    for d, n in enumerate(c.lens):
        seg = tt[ct[d]:ct[d + 1]]
        assert (np.diff(seg) > 0).all() and (seg >= 0).all() and (seg < n).all()


def test_route_shapes_reach_their_routes():
    """Sum of T^2 per case (the size of Mx): many_docs 33963, many_docs_x3 2250, wide
    157425, heads 18500, layers4 5607, bert 2085, long 865."""
    R = P.ROUTE_CASES
    sq = {n: int((_T(n) ** 2).sum()) for n in R}
    print(sq)
    assert sq == {"many_docs": 33963, "many_docs_x3": 2250, "wide": 157425, "heads64": 18500,
                  "heads832": 18500, "layers4": 5607, "bert": 2085, "long": 865}
    # many_docs: a second group of 8, a partial last group, two documents per prep thread
    for name, n_docs in (("many_docs", 300), ("many_docs_x3", 19)):
        c = R[name]
        assert len(c.lens) == n_docs and n_docs % 8 != 0 and set(c.lens) <= set(P.ROUTE_LENS)
        T, n = _T(name), np.array(c.lens)
        rules = np.array(c.rules)
        assert (T[rules == "none"] == 0).all() and (T[rules == "one"] == 1).all()
        assert (T[rules == "all"] == n[rules == "all"]).all() and (T >= 0).all() and (T <= n).all()
        # every rule from the ninth document on and, where they exist, past 256: "all"
        # with pairs, and a subset that is neither one token nor all of them
        for lo, hi in ((8, 16), (256, n_docs)):
            if lo < n_docs:
                r, t, m = rules[lo:hi], T[lo:hi], n[lo:hi]
                assert set(r) == set(P.RULES), (name, lo)
                assert (t[r == "all"] >= 2).any(), (name, lo)
                assert ((t[r == "subset"] >= 2) & (t[r == "subset"] < m[r == "subset"])).any()
    assert len(R["many_docs"].lens) > 256 and set(R["many_docs"].lens) == set(P.ROUTE_LENS)
    # every thread of pair_prep_kernel's 256 owns [300 t / 256, 300 (t + 1) / 256): some own two
    own = np.diff(300 * np.arange(257) // 256)
    assert own.max() == 2 and (own == 2).sum() == 44
    # wide: many 16-row tiles, partial last tiles, T past the square root's exact range
    assert _T("wide").tolist() == [300, 256, 40, 17]
    assert (_T("wide") % 16).tolist() == [12, 0, 8, 1]
    assert R["wide"].lens == (300, 257, 40, 17) and 100 not in R["wide"].terms[0][300:556]
    assert 75000 < P.n_pairs(np.array(R["wide"].terms[1])) < 85000
    assert R["heads64"].hidden // 64 == 1 and R["heads832"].hidden // 64 == 13
    assert R["layers4"].layers == 4 and R["bert"].variant == "bert"
    # long: the largest document the 160 KiB LDS panel admits (T <= n)
    assert _lds_bytes(1232, 1232) <= 160 * 1024 < _lds_bytes(1233, 1233)
    lt = R["long"].terms
    assert R["long"].lens == (1232, 17) and lt[1] == (0, 24, 41)
    assert lt[0][0] == 0 and lt[0][23] == 1231 and R["long"].max_positions == 1240


@pytest.mark.parametrize("name", ROUTES)
def test_route_oracle_can_show_a_wrong_kernel(name):
    """Shares found (positive; exactly zero; then, of the positive pairs, moved by more
    than 1e-2 relative by: attn zero, one direction, last layer only, head 0):
    many_docs    0.741 0.258 | 0.987 0.452 0.478 0.977
    many_docs_x3 0.698 0.300 | 1.000 0.474 0.486 0.996
    wide         0.701 0.299 | 0.790 0.350 0.327 0.779
    heads64      0.492 0.506 | 0.677 0.341 0.357 0 (one head: head 0 is the mean)
    heads832     0.796 0.203 | 0.912 0.425 0.404 0.895
    layers4      0.874 0.126 | 0.980 0.453 0.729 0.960
    bert         0.744 0.256 | 0.997 0.483 0.505 0.992
    long         0.774 0.226 | 0.558 0.266 0.273 0.567
    and the float64 oracle's CPU time on one thread (the minimum of three runs after a
    first one): many_docs 0.18 to 0.25 s, many_docs_x3 0.30, wide 0.45, long 0.24, bert
    0.15, the others under 0.1."""
    import time

    c = P.ROUTE_CASES[name]
    P.oracle(c)  # (the tests' shared copy; it also warms up what torch sets up once)
    cost = np.inf
    for _ in range(3):  # the cost of computing it, whichever test computed it first
        t0 = time.process_time()
        P._oracle.__wrapped__(c, False, None)
        cost = min(cost, time.process_time() - t0)
    o = P.oracle(c, variants=True)
    _, attn, pre, score = o["full"]
    pos = score > 1e-3
    shares = {"positive": pos.mean(), "exactly_zero": (score == 0).mean()}
    for v in P.VARIANTS:
        shares[v] = (np.abs(o[v][3][pos] - score[pos]) > 1e-2 * score[pos]).mean()
    print(name, f"oracle {cost:.2f} s; attn spans {attn.min():.3g} .. {attn.max():.3g}",
          {k: round(float(x), 3) for k, x in shares.items()})
    assert cost < 1.0
    assert shares["positive"] >= 1 / 4
    assert shares["exactly_zero"] >= 1 / 10
    assert shares["exactly_zero"] == pytest.approx((pre <= 0).mean())
    assert shares["zero"] >= 1 / 2
    assert shares["one_direction"] >= 1 / 4
    assert shares["last_layer"] >= 1 / 4
    if c.hidden == 64:
        assert (o["head0"][3] == score).all()
    else:
        assert shares["head0"] >= 1 / 2


def test_layers4_every_layer_holds_maxima():
    """Shares found: layers 0..3 hold the pair maximum for 0.252, 0.265, 0.248, 0.235 of
    the pairs."""
    c = P.ROUTE_CASES["layers4"]
    la = P.layer_attn(c)
    assert la.shape[0] == 4 and (la.max(0) == P.oracle(c)["full"][1]).all()
    share = np.bincount(la.argmax(0), minlength=4) / la.shape[1]
    print(share.round(3))
    assert (share >= 1 / 20).all()


def test_bert_positions_show_in_the_scores():
    """Found: 0.996 of the positive pair scores move by more than 1e-2 relative when the
    positions are XLM-R's (pad id + 1 onwards) instead of BERT's."""
    c = P.ROUTE_CASES["bert"]
    score = P.oracle(c)["full"][3]
    other = P.oracle(c, positions="xlmr")["full"][3]
    pos = score > 1e-3
    share = (np.abs(other[pos] - score[pos]) > 1e-2 * score[pos]).mean()
    print(round(float(share), 3))
    assert share >= 1 / 2
    cfg, sd, *_ = P.inputs(c)
    assert cfg["layer_norm_eps"] == 1e-12 and cfg["type_vocab_size"] == 2
    assert sd["bert.embeddings.token_type_embeddings.weight"].shape[0] == 2


@pytest.mark.parametrize("name", ROUTES)
def test_route_tolerances_hold_for_a_right_device(name):
    """pair_atol (4 x the storage emulation's largest pair-score error) below half a
    printed step, and the emulation's largest relative attn error at most 4e-4: the device
    measures 1.8 x its emulation on the 768 inputs (4.6e-4 against 2.6e-4), so an emulation
    above 5.5e-4 would put a right device at the 1e-3 bound.  Found, atol / attn error:
    many_docs fp32 1.9e-5 / 1.6e-5; many_docs_x3 bf16x3 2.0e-4 / 1.3e-4; wide fp32 2.7e-5 /
    3.3e-5, bf16x3 3.6e-4 / 3.6e-4; heads64 3.2e-5 / 9.7e-6; heads832 1.8e-5 / 2.7e-5;
    layers4 2.3e-5 / 1.5e-5; bert fp32 1.5e-5 / 1.5e-5, bf16x3 1.7e-4 / 1.9e-4; long 1.3e-5 /
    1.6e-5."""
    c = P.ROUTE_CASES[name]
    want = P.oracle(c)["full"][1]
    for kind in sorted({p.split("-")[0] for p in P.ROUTE_PRECS[name]}):
        a = P.pair_atol(kind, c)
        rel = float((np.abs(P.emulation(kind, c)[1] - want) / np.abs(want)).max())
        print(name, kind, f"atol {a:.3g} emulated attn error {rel:.3g}")
        assert 0 < a < 5e-4
        assert rel <= 4e-4
