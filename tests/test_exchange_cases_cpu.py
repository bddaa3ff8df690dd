"""The cases of tests/test_exchange_world_gpu.py, checked without a GPU: every case reaches
what its row in exchange_cases names (proved from the numpy definition, so a case that
stops reaching its route fails here and not silently on the GPU); the replayed-collective
harness (virtual_ranks) gives what real gloo ranks give; and the unsharded rank driver
raises on a query the scorer rejected before it writes a line."""
import multiprocessing as mp
import traceback

import numpy as np
import pytest
import torch

import exchange_cases as X
from test_exchange_cpu import _lists, _run
from virtual_ranks import run_world

from improving_learned_index_amd import parallel

# what each DIRECT row must reach: (sample count, route, per, last thread ragged,
# T_q == 0 for too few samples / too few nonzero, emax == 0, a rank below emax,
# a clamped count, a rejected query)
ALL, SOME, NONE = "all", "some", "none"
WANT = {
    (16, 256, 4, 6, "iid"): (1024, "registers", 1, False, NONE, NONE, False, None, False, False),
    (17, 256, 4, 6, "iid"): (1088, "reread", 1, False, NONE, NONE, False, None, False, False),
    (25, 82, 2, 6, "iid"): (1025, "reread", 1, False, NONE, NONE, False, None, False, False),
    (8, 250, 2, 6, "iid"): (1000, "registers", 1, False, NONE, NONE, False, None, False, False),
    (1, 10, 3, 7, "iid"): (3, "too_few_samples", 1, False, ALL, NONE, False, False, False, False),
    (4, 64, 8, 9, "short"): (32, "registers", 1, False, NONE, ALL, False, None, False, False),
    (3, 40, 3, 1029, "ragged"): (39, "registers", 2, True, NONE, SOME, False, None, False, True),
    (4, 16, 2, 2051, "iid"): (32, "registers", 3, True, NONE, NONE, False, None, False, False),
    (2, 32, 4, 1024, "iid"): (16, "registers", 1, False, NONE, NONE, False, None, False, False),
    (2, 100, 25, 5, "empty"): (8, "registers", 1, False, NONE, ALL, True, False, False, False),
    (3, 100, 8, 24, "rank1_empty"): (36, "registers", 1, False, NONE, NONE, False, True, False,
                                     False),
    (2, 50, 5, 24, "clamped"): (20, "registers", 1, False, NONE, NONE, False, None, True, True),
}


def _amount(n, n_q):
    return NONE if n == 0 else (ALL if n == n_q else SOME)


def _census(case, capsys):
    keys, cnt = X.case_lists(case)
    d = X.case_definition(case)
    per, working, last = X.offsets_threads(d.n_q)
    few_samples, few_nonzero = X.zero_T(d)
    with capsys.disabled():
        print(f"\n  {X.case_id(case)}: {d.n_samples} samples ({X.count_route(d)}, need {d.need}), "
              f"per {per} ({working} threads, last {last}), T_q == 0: {few_samples} too few "
              f"samples + {few_nonzero} too few nonzero of {d.n_q}, emax {d.emax}, "
              f"tot {d.tot.min()}..{d.tot.max()}")
    return keys, cnt, d, per, working, last, few_samples, few_nonzero


def test_direct_table_is_the_issue_table():
    assert set(X.DIRECT) == set(WANT) and len(X.DIRECT) == len(WANT)
    for world, k, g, nq, _ in X.DIRECT:  # a case takes a second or two
        assert nq * k * world < (1 << 20) and 0 < g <= k


@pytest.mark.parametrize("case", X.DIRECT, ids=X.case_id)
def test_direct_case_reaches_its_row(case, capsys):
    world, k, g, nq, mode = case
    keys, cnt, d, per, working, last, few_samples, few_nonzero = _census(case, capsys)
    (n_samples, route, want_per, ragged, w_few_s, w_few_nz, emax0, below, clamped,
     rejected) = WANT[case]
    assert keys.shape == (world, nq, k) and cnt.shape == (world, nq)
    # lists as the scorer emits them: valid prefix strictly descending (unique keys)
    c = np.clip(cnt, 0, k)
    inside = np.arange(k - 1)[None, None, :] < (c[:, :, None] - 1)
    assert (keys[:, :, :-1] > keys[:, :, 1:])[inside].all()
    assert d.n_samples == n_samples and X.count_route(d) == route
    assert (d.n_samples <= X.XR_SAMPLES) == (route != "reread")
    if route == "registers" and n_samples >= 960:  # the last register row: full or partly
        assert (n_samples % 64 == 0) == (n_samples == 1024)
    assert per == want_per and (last < per) == ragged
    if per == 1:
        assert working == nq and (working == X.XS_T) == (nq == 1024)
    if case[3] == 2051:  # threads past the last query: q0 == n_q
        assert working < X.XS_T and working * per >= nq
    assert _amount(few_samples, nq) == w_few_s and _amount(few_nonzero, nq) == w_few_nz
    if mode == "short":  # enough samples, every one of them zero
        assert d.n_samples >= d.need and (d.samples == 0).all() and (cnt < g).all()
        assert cnt.max() > 0 and (d.e == c).all()
    if w_few_s == ALL:
        assert (d.e == c).all()  # every key passes
    assert (d.emax == 0) == emax0
    if emax0:
        assert (cnt == 0).all()
    if below is not None:
        assert (d.tot < d.emax).any() == below
    if mode == "rank1_empty":  # a zero total between non-zero ones
        assert d.tot[1] == 0 and d.tot[0] > 0 and d.tot[2] > 0
    assert (cnt > k).any() == clamped and (cnt < 0).any() == rejected
    if clamped:
        assert (d.e[cnt > k] <= k).all() and (d.e[cnt > k] > 0).all()
        assert (keys >= X.SIGN).any() and (keys[cnt[:, :] > 0] < X.SIGN).any()
    if ragged and per == 2:  # ... and a wave tail in the 4-queries-per-workgroup grids
        assert nq % 4 == 1
    if mode == "iid" and world >= 2:  # doc-id-sharded lists: well under k keys per rank
        assert d.tot.max() / nq < 0.6 * k + d.s_n


@pytest.mark.parametrize("p", X.PRODUCTION, ids=lambda p: "w{}-k{}-q{}-{}-{}".format(*p))
def test_production_case_reaches_its_row(p, capsys):
    world, k, nq, mode, pruned = p
    case = X.production_case(p)
    assert nq * k * world < (1 << 20)
    takes_pruned = parallel.exchange_pruned(world, nq, k, pruned)
    if nq == 0:
        assert X.case_lists(case)[0].shape == (world, 0, k)
        return
    keys, cnt, d, per, working, last, few_samples, few_nonzero = _census(case, capsys)
    assert takes_pruned == (p != (8, 16, 5, "iid", True))
    if pruned is None:  # the automatic choice
        assert nq * k >= parallel.PLAIN_MAX_KEYS and world > 1
    if not takes_pruned:
        assert case[2] == 1  # g = 1: sampling every key is the plain gather
    want = {(2, 200, 24): (25, 1, False), (8, 1000, 24): (31, 1, False),
            (3, 40, 1029): (3, 2, True), (4, 64, 2051): (4, 3, True), (8, 16, 5): (1, 1, False),
            (2, 100, 5): (12, 1, False), (3, 100, 24): (8, 1, False)}[(world, k, nq)]
    assert (case[2], per, last < per) == want
    assert (d.emax == 0) == (mode == "empty")
    if mode == "rank1_empty":
        assert d.tot[1] == 0 and d.tot[0] > 0 and d.tot[2] > 0
    if mode == "ragged":
        assert (cnt < 0).any() and (keys >= X.SIGN).any()
    if mode == "iid" and world >= 2:
        assert d.tot.max() / nq < 0.6 * k + d.s_n


def test_definition_equals_a_per_query_restatement():
    """The vectorised definition against the loop test_exchange_gpu.py writes out."""
    for case in [(3, 40, 3, 24, "ragged"), (2, 50, 5, 24, "clamped"), (4, 64, 8, 9, "short"),
                 (1, 10, 3, 7, "iid")]:
        world, k, g, nq, _ = case
        keys, cnt = X.case_lists(case)
        d = X.definition(keys, cnt, k, g)
        s_n, need = k // g, -(-k // g)
        for q in range(nq):
            allS = []
            for r in range(world):
                c = min(max(int(cnt[r, q]), 0), k)
                sr = [keys[r, q, (j + 1) * g - 1] if (j + 1) * g - 1 < c else 0 for j in range(s_n)]
                assert d.samples[r, q].tolist() == sr
                allS += sr
            allS = sorted(allS, reverse=True)
            T = allS[need - 1] if len(allS) >= need else 0
            assert int(d.T[q]) == int(T)
            for r in range(world):
                c = min(max(int(cnt[r, q]), 0), k)
                e = sum(1 for x in keys[r, q, :c].tolist() if x >= int(T))
                assert d.e[r, q] == e and d.off[r, q] == d.e[r, :q].sum()
                assert d.packed[r, d.off[r, q]:d.off[r, q] + e].tolist() == keys[r, q, :e].tolist()
                assert d.g_n[r, q] == (cnt[r, q] if cnt[r, q] < 0 else e)
        # the merge of the prefixes is the merge of the full lists
        pre = np.where(d.prefix, keys, np.uint64(0))
        assert X._merge(pre, d.g_n, k) == X._merge(keys, cnt, k)


def _host_exchange(world, keys, cnt, k, pruned, backend="gloo"):
    def body(rank):
        st = {}
        kt = torch.from_numpy(keys[rank].reshape(-1).view(np.int64).copy())
        gk, gn = parallel.exchange_topk(kt, torch.from_numpy(cnt[rank].copy()), k, stats=st,
                                        pruned=pruned)
        nq = cnt.shape[1]
        return gk.numpy().view(np.uint64).reshape(world, nq, k), gn.numpy().reshape(world, nq), st

    return body


def _play_in_child(q, world, keys, cnt, k, pruned):
    try:
        with pytest.MonkeyPatch.context() as m:
            q.put(run_world(m, world, _host_exchange(world, keys, cnt, k, pruned), "gloo"))
    except BaseException:
        q.put(traceback.format_exc())


def _played(world, keys, cnt, k, pruned):
    """run_world in a forked child, as the gloo ranks of test_exchange_cpu._run are: torch's
    tensor operations start its thread pool, and a process that has done so must not fork
    ranks afterwards (their first parallel operation would wait for threads that the fork
    did not copy) -- the pytest process forks them in test_exchange_cpu.py after this."""
    ctx = mp.get_context("fork")
    q = ctx.Queue()
    p = ctx.Process(target=_play_in_child, args=(q, world, keys, cnt, k, pruned))
    p.start()
    res = q.get(timeout=120)
    p.join(timeout=60)
    assert not isinstance(res, str), res
    assert p.exitcode == 0
    return res


@pytest.mark.parametrize("pruned", [True, False])
def test_replayed_collectives_equal_gloo(pruned):
    """exchange_topk on CPU tensors at world 3: played rank by rank under run_world it
    returns what three real gloo processes return for the same lists."""
    world, k, nq = 3, 40, 24
    keys, cnt = _lists(world, nq, k, seed=5, mode="ragged")
    real = _run(world, keys, cnt, k, pruned)
    played = _played(world, keys, cnt, k, pruned)
    assert len(played) == world
    for r in range(world):
        gk, gn, st = played[r]
        rk, rn, rst = real[r]
        assert st == rst and st["path"] == ("pruned" if pruned else "plain")
        assert (gn == rn).all()
        valid = np.arange(k)[None, None, :] < np.maximum(gn, 0)[:, :, None]
        assert (gk[valid] == rk[valid]).all()  # (slots past a prefix are torch.empty)
        assert X._merge(gk, gn, k) == X._merge(keys, cnt, k)


def test_harness_refuses_what_a_collective_hangs_on(monkeypatch):
    import torch.distributed as dist

    real, real_rank = dist.all_gather_into_tensor, dist.get_rank

    def uneven(rank):  # rank 1 skips the collective
        if rank != 1:
            out = torch.empty(4, dtype=torch.int64)
            dist.all_gather_into_tensor(out, torch.full((2,), rank, dtype=torch.int64))
        return rank

    with pytest.raises(AssertionError, match="disagree"):
        run_world(monkeypatch, 2, uneven)

    def shapes(rank):
        n = 2 + rank
        dist.all_gather_into_tensor(torch.empty(2 * n), torch.zeros(n))

    with pytest.raises(AssertionError, match="disagree"):
        run_world(monkeypatch, 2, shapes)

    def short_out(rank):
        dist.all_gather_into_tensor(torch.empty(3), torch.zeros(2))

    with pytest.raises(AssertionError):
        run_world(monkeypatch, 2, short_out)

    calls = []

    def fickle(rank):  # not deterministic: the re-played input differs
        calls.append(rank)
        dist.all_gather_into_tensor(torch.empty(2), torch.full((1,), float(len(calls))))

    with pytest.raises(AssertionError, match="re-played differently"):
        run_world(monkeypatch, 2, fickle)

    def ok(rank):
        assert dist.get_rank() == rank and dist.get_world_size() == 3
        assert dist.get_backend() == "nccl"
        a = torch.empty(3, dtype=torch.int32)
        dist.all_gather_into_tensor(a, torch.tensor([rank * 10], dtype=torch.int32))
        b = torch.empty(3, dtype=torch.int32)
        dist.all_gather_into_tensor(b, (a.sum() + rank).to(torch.int32).reshape(1))
        return a.tolist(), b.tolist()

    assert run_world(monkeypatch, 3, ok) == [([0, 10, 20], [30, 31, 32])] * 3
    # ... and torch.distributed is itself again
    assert dist.all_gather_into_tensor is real and dist.get_rank is real_rank


class _RejectingIndex:
    """An index whose scorer rejected query 1 of 3 (count -1; its row is garbage)."""

    def term_ids(self, terms):
        return [1, 2]

    def search_ids(self, queries_ids, top_k=1000, with_keys=False):
        n_q = len(queries_ids)
        docs = np.arange(n_q * top_k, dtype=np.uint32).reshape(n_q, top_k)
        scores = np.full((n_q, top_k), 9, np.uint32)
        return docs, scores, np.array([2, -1, 3], np.int32)[:n_q], None


@pytest.mark.parametrize("py_writes", [None, "1"])
def test_unsharded_rank_raises_on_a_rejected_query(tmp_path, monkeypatch, py_writes):
    """ranker.Ranker.run without shards: a count of -1 raises decode_quant_keys' error
    before either write path runs (docs[i, :-1] would be k - 1 garbage lines), and the
    run file gains no line for the chunk."""
    from improving_learned_index_amd.datasets import RunFile
    from improving_learned_index_amd.ranker import Ranker

    if py_writes is None:
        monkeypatch.delenv("DI_RANK_PY_WRITES", raising=False)
    else:
        monkeypatch.setenv("DI_RANK_PY_WRITES", py_writes)
    run = tmp_path / "run.tsv"
    run.write_text("q0\t5\t1\t7\n")  # (an earlier chunk's line)
    rk = Ranker.__new__(Ranker)
    rk.query_iterator, rk.batch_queries, rk.dist, rk.top_k = ["a", "b", "c"], 8, False, 4
    rk.index, rk.run_file, rk.pairwise = _RejectingIndex(), RunFile(run), False
    monkeypatch.setattr(Ranker, "get_query_terms", lambda self, qid: {"x"})
    with pytest.raises(RuntimeError, match="rejected a query") as e:
        rk.run()
    with pytest.raises(RuntimeError) as same:
        parallel.decode_quant_keys(np.zeros(4, np.uint64), -1)
    assert str(e.value) == str(same.value)
    assert run.read_text() == "q0\t5\t1\t7\n"


def test_key_layout_uses_the_library_constant():
    from improving_learned_index_amd import _lib

    t = _lib.DI_SHORT_QUERY_TERMS
    keys = np.array([[(7 << 48) | (0xFFFFFFFF - 5)], [(7 << 44) | (0xFFFFFF - 5)]], np.uint64)
    docs, scores = parallel.decode_quant_key_arrays(keys, np.array([1, 1]), [t, t + 1])
    assert docs.tolist() == [[5], [5]] and scores.tolist() == [[7], [7]]
    assert parallel.decode_quant_keys(keys[0], 1, t) == [(5, 7)]
    assert parallel.decode_quant_keys(keys[1], 1, t + 1) == [(5, 7)]
