"""di_format_entry_lines on the host: the impact-TSV lines of DeepPairwiseImpact's entries
(reference indexer.py:62-68 over the names of pairwise_impact.py:98-129) from term indices,
byte-equal to di_format_impact_lines fed the names Python builds; the DI_ERANGE contract;
and the LDS capacity constant against the header."""
import ctypes
import re

import numpy as np
import pytest

from conftest import ROOT

SCORES = np.array([0.0, 0.001, 12.345, 1e-05, 1.5e-05, 123456.789, 3.4e38, 1e10, 0.1, 2.0, -0.0,
                   -1.25, 7e-4, 1e16, 0.999], np.float32)


def _blob(terms):
    enc = [t.encode("utf-8") for t in terms]
    off = np.zeros(len(enc) + 1, np.int64)
    if enc:
        off[1:] = np.cumsum([len(b) for b in enc])
    return b"".join(enc), off


def _case(n_docs, seed, n_terms=40, max_entries=30):
    """Terms (some multibyte), and per document a random list of entries; document 0 is
    empty, document 1 holds single terms only."""
    rng = np.random.default_rng(seed)
    terms = [("▁" if i % 3 else "") + f"t{i}" + ("é" if i % 5 == 0 else "")
             for i in range(n_terms)]
    n = rng.integers(0, max_entries + 1, n_docs)
    n[:1] = 0
    if n_docs > 1:
        n[1] = 5
    if n_docs > 3:
        n[3] = 0
    cu = np.zeros(n_docs + 1, np.int64)
    cu[1:] = np.cumsum(n)
    ne = int(cu[-1])
    first = rng.integers(0, n_terms, ne).astype(np.int32)
    second = np.where(rng.random(ne) < 0.6, rng.integers(0, n_terms, ne), -1).astype(np.int32)
    if n_docs > 1:
        second[cu[1]:cu[2]] = -1
    score = SCORES[rng.integers(0, len(SCORES), ne)]
    return terms, first, second, score, cu


def _want(terms, first, second, score, cu):
    """di_format_impact_lines over the names a Python loop builds (the host path)."""
    from improving_learned_index_amd import _lib

    names = [terms[f] if s < 0 else f"{terms[f]}|{terms[s]}"
             for f, s in zip(first.tolist(), second.tolist())]
    blob, off = _blob(names)
    return _lib.format_impact_lines_packed(blob, off, score, cu)


@pytest.mark.parametrize("n_docs,seed", [(0, 0), (1, 1), (2, 2), (7, 3), (5000, 4)])
def test_entry_lines_equal_impact_lines_over_built_names(n_docs, seed, monkeypatch):
    """5000 documents: more chunks than threads, so several threads format (8 are asked for)."""
    from improving_learned_index_amd import _lib

    monkeypatch.setenv("DI_HOST_THREADS", "8")
    terms, first, second, score, cu = _case(n_docs, seed)
    blob, off = _blob(terms)
    got = _lib.format_entry_lines(blob, off, first, second, score, cu)
    want = _want(terms, first, second, score, cu)
    assert got == want
    assert got.count("\n") == n_docs
    if n_docs >= 2:
        lines = got.split("\n")
        assert lines[0] == "" and "|" not in lines[1] and lines[1].count(", ") == 4
    if n_docs >= 5000:  # (float32(1.5e-05) prints as 1.4999999621068127e-05)
        assert "▁t1|" in got and "é|" in got and "e-05, " in got and ": 0.0, " in got
    monkeypatch.setenv("DI_HOST_THREADS", "1")
    assert _lib.format_entry_lines(blob, off, first, second, score, cu) == want


def test_the_scores_print_as_python_reprs():
    from improving_learned_index_amd import _lib

    blob, off = _blob(["a", "▁b"])
    n = len(SCORES)
    first = np.zeros(n, np.int32)
    second = np.where(np.arange(n) % 2, 1, -1).astype(np.int32)
    got = _lib.format_entry_lines(blob, off, first, second, SCORES, np.array([0, n], np.int64))
    want = ", ".join(f"{'a|▁b' if i % 2 else 'a'}: {float(v)!r}" for i, v in enumerate(SCORES))
    assert got == want + "\n"
    assert "a: 0.0, a|▁b: 0.0010000000474974513" in got


def test_small_buffer_reports_the_length_needed():
    from improving_learned_index_amd import _lib

    terms, first, second, score, cu = _case(50, 9)
    blob, off = _blob(terms)
    want = _want(terms, first, second, score, cu).encode("utf-8")
    L = _lib.lib()
    tb = ctypes.create_string_buffer(blob, len(blob) + 1)
    for cap in (0, 1, len(want) - 1):
        buf = ctypes.create_string_buffer(b"\xAA" * (len(want) + 8), len(want) + 8)
        n = ctypes.c_int64(-1)
        rc = L.di_format_entry_lines(tb, _lib.ptr(off), len(terms), _lib.ptr(first),
                                     _lib.ptr(second), _lib.ptr(score), _lib.ptr(cu), len(cu) - 1,
                                     buf, cap, ctypes.byref(n))
        assert rc == _lib.DI_ERANGE and n.value == len(want)
        assert buf.raw == b"\xAA" * (len(want) + 8)  # nothing written
    buf = ctypes.create_string_buffer(len(want))
    n = ctypes.c_int64(-1)
    rc = L.di_format_entry_lines(tb, _lib.ptr(off), len(terms), _lib.ptr(first), _lib.ptr(second),
                                 _lib.ptr(score), _lib.ptr(cu), len(cu) - 1, buf, len(want),
                                 ctypes.byref(n))
    assert rc == 0 and buf.raw[:n.value] == want
    with pytest.raises(_lib.DIError) as e:
        _lib.format_entry_lines(blob, off, first, second, score, cu, out_cap=10)
    assert e.value.code == _lib.DI_ERANGE


def test_a_term_index_outside_the_batch_is_refused():
    from improving_learned_index_amd import _lib

    blob, off = _blob(["a", "b"])
    cu = np.array([0, 1], np.int64)
    for f, s in ((2, -1), (0, 2), (-1, -1)):
        with pytest.raises(_lib.DIError) as e:
            _lib.format_entry_lines(blob, off, np.array([f], np.int32), np.array([s], np.int32),
                                    np.ones(1, np.float32), cu)
        assert e.value.code == -1


def test_lds_capacity_constant_is_the_headers():
    from improving_learned_index_amd import _lib

    text = (ROOT / "include" / "deepimpact.h").read_text()
    m = re.search(r"^#define\s+DI_PAIR_ORDER_LDS_KEYS\s+(\d+)", text, re.M)
    assert m and int(m.group(1)) == _lib.DI_PAIR_ORDER_LDS_KEYS
    m = re.search(r"^#define\s+DI_PAIR_ORDER_MAX_TERMS\s+(\d+)", text, re.M)
    assert m and int(m.group(1)) == _lib.DI_PAIR_ORDER_MAX_TERMS
    # one LDS sort fits the 160 KiB of a workgroup, as a power of two (bitonic)
    k = _lib.DI_PAIR_ORDER_LDS_KEYS
    assert k & (k - 1) == 0 and k * 8 <= 160 * 1024
    # every document di_encode_pairwise accepts fits the key's position and rank bits
    T = _lib.DI_PAIR_ORDER_MAX_TERMS
    assert T >= 1232 and T < 2 ** 11 and T * (T + 1) // 2 < 2 ** 21
