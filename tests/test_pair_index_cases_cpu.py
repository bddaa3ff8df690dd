"""pair_index_cases.py without a GPU: the plain-numpy restatement of the pairwise route
equals the oracle's text route on every case, and every case reaches the edge it is there
for, so the GPU tests cannot pass by missing it."""
import itertools

import numpy as np
import pytest

import oracle
import pair_index_cases as C


@pytest.mark.parametrize("name", C.OK_NAMES)
def test_numpy_restatement_equals_the_oracle(name):
    c, e = C.case(name), C.expected(name)
    n = C.numpy_order(c, c.max_val)
    assert n["max_used"] == e.max_used
    assert n["vocab"] == e.vocab
    assert np.array_equal(n["term_off"], e.term_off)
    assert np.array_equal(n["pdoc"], e.pdoc)
    assert np.array_equal(n["pval"], e.pval)
    # rows and counts agree with the oracle's lists
    counts = np.diff(e.term_off)
    all_count = np.concatenate([e.term_count, e.pair_count])
    assert (e.term_row >= 0).sum() == len(e.vocab)
    assert np.array_equal(counts[e.term_row[e.term_row >= 0]], all_count[e.term_row >= 0])
    assert (all_count[e.term_row < 0] == 0).all()
    assert (e.pair_count > 0).all()
    key = (e.pair_first.astype(np.int64) << 32) | e.pair_second
    assert (np.diff(key) > 0).all()


def test_tiny():
    c = C.case("tiny")
    assert [len(d[0]) for d in c.documents()] == [1, 2, 3]
    assert sorted(t for t in C.expected("tiny").vocab if "|" in t) == ["a|c", "a|d", "b|a", "c|d"]


def test_round_edges():
    c, e = C.case("round_edges"), C.expected("round_edges")
    r = oracle.round3(np.array(C.ROUND_EDGES, np.float32))
    step = oracle.round3(np.array([0.001], np.float32))[0]
    raw = np.array(C.ROUND_EDGES, np.float32)
    assert ((r == 0) & (raw != 0)).any(), "no non-zero pair dropped by round3"
    assert (r == step).any() and step > 0, "no pair kept with rounded value 0.001"
    assert np.signbit(raw[1]) and r[1] == 0  # -0.0 stays falsy
    p_v = c.entries()[6]
    assert (p_v == step).any() and p_v.size == int((r != 0).sum()) + 1
    assert "q: 0.0" in c.impact_lines()[0] and "q" not in e.vocab
    # a rounded 0.001 survives the quantizer here, so the edge reaches the files
    kept_names = [t for t in e.vocab if "|" in t]
    assert "s|r" in kept_names


def test_shared_pairs():
    c, e = C.case("shared_pairs"), C.expected("shared_pairs")
    assert "a|b" in e.vocab and "b|a" in e.vocab
    got = dict(zip(zip(e.pair_first.tolist(), e.pair_second.tolist()), e.pair_count.tolist()))
    assert got == {(0, 1): 40, (1, 0): 15}
    r = e.vocab.index("a|b")
    v = e.pval[e.term_off[r]:e.term_off[r + 1]]
    d = e.pdoc[e.term_off[r]:e.term_off[r + 1]].astype(np.int64)
    assert len(set(v.tolist())) == 3
    assert (np.diff(v.astype(np.int64)) <= 0).all()
    assert (np.diff(d)[np.diff(v.astype(np.int64)) == 0] > 0).all()  # doc ascending in a tie


@pytest.mark.parametrize("total", [C.T - 1, C.T, C.T + 1])
def test_tile_edges(total):
    c, e = C.case(f"tile_edges_{total}"), C.expected(f"tile_edges_{total}")
    assert [len(d[0]) for d in c.documents()] == [91, 92]
    assert C.n_comb(91) == 4095 and C.n_comb(92) == 4186
    assert c.entries()[3].size == total      # kept by round3 at the append
    assert int(e.pair_count.sum()) == total  # and by the quantizer
    cup = c.appends[0][5]
    assert cup[1] < C.T < cup[2]  # document 1's pairs straddle the tile boundary


def test_max_from_pair():
    c, e = C.case("max_from_pair"), C.expected("max_from_pair")
    s_v, p_v = c.entries()[2], c.entries()[6]
    assert e.max_used == float(p_v.max()) > float(s_v.max())
    assert e.max_used == float(np.float32(c.notes["k_max"] / 1000.0))
    assert int(e.max_used * (255.0 / e.max_used)) == 254 and int(e.pval.max()) == 254


def test_quantized_to_zero():
    c, e = C.case("quantized_to_zero"), C.expected("quantized_to_zero")
    _, _, _, p_a, p_b, _, p_v = c.entries()
    appended = {(a, b) for a, b in zip(p_a.tolist(), p_b.tolist())}
    assert (p_v != 0).all()
    assert c.notes["gone"] not in e.vocab and (2, 3) in appended
    assert e.pair_first.size < len(appended)
    assert e.max_used == 2.0


def test_wide_ids():
    c, e = C.case("wide_ids"), C.expected("wide_ids")
    assert int(e.pair_first.max()) > 255 and int(e.pair_second.max()) > 255
    assert len(e.vocab) > 65536  # three digits of the row
    assert [len(d[0]) for d in c.documents()] == [92] * 20


def test_name_order():
    e = C.expected("name_order")
    kinds = ["|" in t and t not in C.case("name_order").terms for t in e.vocab]
    runs = "".join(k for k, _ in itertools.groupby("p" if k else "s" for k in kinds))
    assert "sps" in runs and "psp" in runs  # pair names between singles, and the reverse
    assert e.vocab == sorted(e.vocab, key=lambda t: t.encode("utf-8"))
    assert any(len(t.encode("utf-8")) > len(t) for t in e.vocab)
    assert len(set(e.vocab)) == len(e.vocab)


def test_split_appends():
    one, three = C.case("split_appends_1"), C.case("split_appends_3")
    assert len(one.appends) == 1 and len(three.appends) == 3
    assert C.expected("split_appends_1").files == C.expected("split_appends_3").files
    m = C.expected("split_appends_1").max_used
    other = C.expected("split_appends_1", 3 * m)
    assert other.max_used == 3 * m and other.files != C.expected("split_appends_1").files


def test_mixed():
    c = C.case("mixed")
    assert [a[0] for a in c.appends] == ["single", "pair", "single"]
    assert any("|" in t for t in C.expected("mixed").vocab)


def test_error_cases():
    for name in C.ERROR_NAMES:
        assert C.case(name).error in ("DI_EINVAL", "DI_EFORMAT")
    c = C.case("cu_pairs_off")
    d = c.notes["doc"]
    cup = c.appends[0][5].copy()
    cup[d + 1] += 1
    assert (np.diff(cup) >= 0).all() and cup[0] == 0 and cup[-1] == c.appends[0][5][-1]
    c = C.case("bad_term_id")
    assert int(c.appends[0][1].max()) == len(c.terms)
    assert np.isnan(C.case("nan_pair").appends[0][3]).sum() == 1
    c = C.case("empty_doc")
    assert len(c.documents()[c.notes["doc"]][0]) == 0


@pytest.mark.parametrize("name", ["collision_single", "collision_pair"])
def test_collisions_collide(name):
    """Two kept entries share a name: the text route would merge them into one line."""
    c = C.case(name)
    n = C.numpy_order(c)
    assert len(set(n["vocab"])) == len(n["vocab"]) - 1
    assert n["vocab"].count(c.notes["name"]) == 2


def test_collision_dropped_does_not_collide():
    c, e = C.case("collision_dropped"), C.expected("collision_dropped")
    _, _, _, p_a, p_b, _, p_v = c.entries()
    assert (0, 1) in set(zip(p_a.tolist(), p_b.tolist()))  # appended, rounded non-zero
    assert (0, 1) not in set(zip(e.pair_first.tolist(), e.pair_second.tolist()))
    assert e.vocab.count("x|y") == 1
