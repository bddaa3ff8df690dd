"""The device exchange between doc-id shards at world > 1, on one GPU.

* The di_xchg_* kernels (exchange.hip) one by one on the cases of exchange_cases.DIRECT:
  every output against the numpy definition (samples, both rows of ec, offsets, totals,
  emax, each rank's packed buffer, the unpacked prefixes, g_n), then the lists-major
  di_topk_merge of the result against the merge of the full lists.
* The production function: parallel.exchange_topk on device tensors, every rank played in
  turn under replayed all_gathers (virtual_ranks.run_world, backend "nccl") -- the call
  that reaches _exchange_pruned_hip with me > 0, several ranks' offset rows and padding --
  against the same call on CPU tensors (the tensor-operation form) and the definition.
* The whole retrieve step: parallel.exchange_merge_device over DeviceIndex shards of one
  synthetic collection against the unsharded index's keys.
* Bad arguments to every di_xchg_* entry point: DI_EINVAL before any launch.

Every comparison is integer equality.  test_exchange_cases_cpu.py proves without a GPU
that each case reaches what it is here for.  (pack / unpack trust their offsets and
counts: they only ever get the ones the earlier steps produced and this file has checked.)
"""
import numpy as np
import pytest
import torch

import exchange_cases as X
from virtual_ranks import run_world

from improving_learned_index_amd import parallel

pytestmark = pytest.mark.gpu

SENTINEL = -6148914691236517206  # 0xAAAA...: a slot no kernel may have written


@pytest.fixture(scope="module")
def L():
    from improving_learned_index_amd import _lib

    if _lib.device_count() < 1:
        pytest.fail("no HIP device visible (GPU test run without a GPU)")
    return _lib


def _dev_lists(keys, cnt, dev):
    W = keys.shape[0]
    Ks = [torch.from_numpy(keys[r].reshape(-1).view(np.int64).copy()).to(dev) for r in range(W)]
    Cs = [torch.from_numpy(cnt[r].copy()).to(dev) for r in range(W)]
    return Ks, Cs


def _u64(t, *shape):
    return t.cpu().numpy().view(np.uint64).reshape(shape)


def _device_steps_equal_definition(L, keys, cnt, k, g, d):
    """The five kernels as parallel._exchange_pruned_hip chains them, over every rank of
    the case, each output checked before the next step consumes it."""
    lib, P = L.lib(), L.ptr
    W, nq, _ = keys.shape
    dev = torch.device("cuda", 0)
    st = torch.cuda.current_stream(dev).cuda_stream
    Ks, Cs = _dev_lists(keys, cnt, dev)
    s_n = k // g
    smp = []
    for r in range(W):
        s = torch.full((nq * s_n,), SENTINEL, dtype=torch.int64, device=dev)
        L.check(lib.di_xchg_sample(P(Ks[r]), P(Cs[r]), nq, k, g, P(s), 0, st))
        smp.append(s)
    gs = torch.cat(smp)
    assert (_u64(gs, W, nq, s_n) == d.samples).all()
    ecs = []
    for r in range(W):
        ec = torch.full((2 * nq,), -77, dtype=torch.int32, device=dev)
        L.check(lib.di_xchg_count(P(gs), W, P(Ks[r]), P(Cs[r]), nq, k, g, P(ec), 0, st))
        ecs.append(ec)
    gec = torch.cat(ecs)
    got_ec = gec.cpu().numpy().reshape(W, 2, nq)
    assert (got_ec[:, 0] == d.ec[:, 0]).all(), np.argwhere(got_ec[:, 0] != d.ec[:, 0])[:8]
    assert (got_ec[:, 1] == d.ec[:, 1]).all()
    off = torch.full((W * nq,), -1, dtype=torch.int64, device=dev)
    tot = torch.full((W,), -1, dtype=torch.int64, device=dev)
    L.check(lib.di_xchg_offsets(P(gec), W, nq, P(off), P(tot), 0, st))
    assert (off.cpu().numpy().reshape(W, nq) == d.off).all()
    assert (tot.cpu().numpy() == d.tot).all()
    emax = int(tot.max().item())
    assert emax == d.emax
    g2 = None
    if emax:
        g2 = torch.zeros(W * emax, dtype=torch.int64, device=dev)
        for r in range(W):
            buf = g2[r * emax:(r + 1) * emax]
            L.check(lib.di_xchg_pack(P(Ks[r]), P(ecs[r]), P(off[r * nq:]), nq, k, P(buf), 0, st))
        assert (_u64(g2, W, emax) == d.packed).all()
    out = torch.full((W * nq * k,), SENTINEL, dtype=torch.int64, device=dev)
    g_n = torch.full((W * nq,), -77, dtype=torch.int32, device=dev)
    L.check(lib.di_xchg_unpack(P(g2), emax, P(gec), P(off), W, nq, k, P(out), P(g_n), 0, st))
    assert (g_n.cpu().numpy().reshape(W, nq) == d.g_n).all()
    # the prefixes, and nothing written past them
    want = np.where(d.prefix, keys, np.int64(SENTINEL).astype(np.uint64))
    assert (_u64(out, W, nq, k) == want).all()
    # the production chain's last step (parallel._exchange_merge): di_topk_merge over the
    # gathered [world][nq][k] lists where they lie, lists-major on device pointers
    mk = torch.full((nq * k,), -1, dtype=torch.int64, device=dev)
    mn = torch.full((nq,), -7, dtype=torch.int32, device=dev)
    L.topk_merge_device(out, g_n, nq, W, k, mk, mn, device=0, stream=st,
                        flags=L.DI_F_DEVICE_PTRS | L.DI_F_LISTS_MAJOR)
    torch.cuda.synchronize()
    return _u64(mk, nq, k), mn.cpu().numpy()


def _merge_equals_full_lists(mk, mn, keys, cnt, k):
    want = X._merge(keys, cnt, k)
    for q, w in enumerate(want):
        if w is None:
            assert mn[q] == -1, q  # (a rejected query)
        else:
            assert mn[q] == len(w) and mk[q, :mn[q]].tolist() == w, q


@pytest.mark.parametrize("case", X.DIRECT, ids=X.case_id)
def test_kernels_equal_definition(L, case):
    world, k, g, nq, mode = case
    keys, cnt = X.case_lists(case)
    mk, mn = _device_steps_equal_definition(L, keys, cnt, k, g, X.case_definition(case))
    _merge_equals_full_lists(mk, mn, keys, cnt, k)


def _exchange_body(world, keys, cnt, k, pruned, dev):
    nq = cnt.shape[1]

    def body(rank):
        st = {}
        kt = torch.from_numpy(keys[rank].reshape(-1).view(np.int64).copy()).to(dev)
        ct = torch.from_numpy(cnt[rank].copy()).to(dev)
        gk, gn = parallel.exchange_topk(kt, ct, k, stats=st, pruned=pruned)
        assert gk.device.type == dev.type and gn.device.type == dev.type
        assert gk.dtype == torch.int64 and gn.dtype == torch.int32
        return _u64(gk, world, nq, k), gn.cpu().numpy().reshape(world, nq), st

    return body


@pytest.mark.parametrize("p", X.PRODUCTION, ids=lambda p: "w{}-k{}-q{}-{}-{}".format(*p))
def test_exchange_topk_on_device_tensors(L, monkeypatch, p):
    world, k, nq, mode, pruned = p
    case = X.production_case(p)
    keys, cnt = X.case_lists(case)
    takes_pruned = parallel.exchange_pruned(world, nq, k, pruned)
    assert takes_pruned == (case[2] > 1)
    d = X.definition(keys, cnt, k, case[2]) if takes_pruned else X.definition_plain(keys, cnt, k)
    on_dev = run_world(monkeypatch, world,
                       _exchange_body(world, keys, cnt, k, pruned, torch.device("cuda", 0)), "nccl")
    on_cpu = run_world(monkeypatch, world,
                       _exchange_body(world, keys, cnt, k, pruned, torch.device("cpu")), "nccl")
    assert len(on_dev) == len(on_cpu) == world
    for r in range(world):
        gk, gn, st = on_dev[r]
        ck, cn, cst = on_cpu[r]
        assert st == cst, (r, st, cst)  # path, gathered_keys_per_query, bytes_sent
        assert st["path"] == ("pruned" if takes_pruned else "plain")
        assert (gn == cn).all() and (gn == d.g_n).all(), r
        valid = np.arange(k)[None, None, :] < np.maximum(gn, 0)[:, :, None]
        assert (valid == d.prefix).all(), r
        # (slots past a prefix are torch.empty in the device form: not compared)
        assert (gk[valid] == ck[valid]).all(), r
        assert (gk[d.prefix] == keys[d.prefix]).all(), r
        g0k, g0n, _ = on_dev[0]
        assert (gn == g0n).all() and (gk[valid] == g0k[valid]).all(), r
        if takes_pruned and nq:
            assert st["bytes_sent"] == 8 * (nq * d.s_n + d.emax) + 8 * nq
    if nq:
        # the merge of what the last rank received is the merge of the full lists
        assert X._merge(on_dev[-1][0], on_dev[-1][1], k) == X._merge(keys, cnt, k)


@pytest.fixture(scope="module")
def collection(L):
    """A small synthetic quantized collection, whole, and ~40 queries: short ones, an empty
    one, one of more than DI_SHORT_QUERY_TERMS terms (wide keys) and one of more than
    DI_MAX_QUERY_TERMS (rejected).  The whole index's keys are the reference (the host
    entry point refuses the rejected query outright, so it is left out of that call)."""
    from improving_learned_index_amd import synthetic as S

    n_docs, v_terms, k = 4000, 5000, 128
    cu, term, imp = S.msmarco_like_docs(n_docs, v_terms, 23, max_terms=60)
    q, _ = S.quantize_like_reference(imp)
    term_off, pdoc, pval = S.postings_reference_order(cu, term, q, v_terms)
    rng = np.random.default_rng(29)
    qs = []
    for _ in range(37):
        z = np.minimum(rng.zipf(1.25, int(rng.integers(1, 9))), v_terms) - 1
        qs.append(list(dict.fromkeys(int(x) for x in z)))
    qs.insert(5, [])
    qs.insert(11, [int(x) for x in rng.permutation(v_terms)[:L.DI_SHORT_QUERY_TERMS + 44]])
    rejected = 20
    qs.insert(rejected, list(range(L.DI_MAX_QUERY_TERMS + 1)))
    assert len(qs) == 40
    accepted = [i for i in range(len(qs)) if i != rejected]
    whole = L.DeviceIndex.from_postings(term_off, pdoc, pval)
    _, _, n, key = whole.search_csr(*L.csr([qs[i] for i in accepted]), k, with_keys=True)
    assert n.min() >= 0 and n.max() == k and (n < k).any()
    return dict(postings=(term_off, pdoc, pval), n_docs=int(pdoc.max()) + 1, k=k, queries=qs,
                rejected=rejected, accepted=accepted, keys=key, counts=n)


@pytest.mark.parametrize("world", [2, 5])
def test_retrieve_step_over_shards_equals_whole_index(L, monkeypatch, collection, world):
    c = collection
    k, qs = c["k"], c["queries"]
    assert parallel.exchange_pruned(world, len(qs), k)  # (the default choice: pruned)
    shards = [L.DeviceIndex.from_postings(*c["postings"], *parallel.shard_range(c["n_docs"], world, r))
              for r in range(world)]
    res = run_world(monkeypatch, world,
                    lambda rank: parallel.exchange_merge_device(shards[rank], qs, k, 0), "nccl")
    n_terms = [len(q) for q in qs]
    for r, (keys, n) in enumerate(res):
        assert keys.shape == (len(qs), k) and keys.dtype == np.uint64 and n.shape == (len(qs),)
        assert n[c["rejected"]] < 0, r  # the rejected query keeps its negative count
        assert (n[c["accepted"]] == c["counts"]).all(), r
        valid = np.arange(k)[None, :] < c["counts"][:, None]
        assert (keys[c["accepted"]][valid] == c["keys"][valid]).all(), r
        with pytest.raises(RuntimeError, match="rejected a query"):
            parallel.decode_quant_key_arrays(keys, n, n_terms)
        docs, _ = parallel.decode_quant_key_arrays(keys[c["accepted"]], n[c["accepted"]],
                                                   [n_terms[i] for i in c["accepted"]])
        assert int(docs[valid].max()) < c["n_docs"]  # (wide and compact keys both decode)


def test_bad_arguments_are_refused_before_any_launch(L):
    """Every di_xchg_* entry point returns DI_EINVAL for a zero or oversized stride, an
    empty world, a negative query count, a null required pointer and an impossible emax;
    a correct chain on the same stream afterwards still equals the definition."""
    lib, P = L.lib(), L.ptr
    case = (2, 50, 5, 24, "clamped")
    W, k, g, nq, _ = case
    keys, cnt = X.case_lists(case)
    d = X.case_definition(case)
    dev = torch.device("cuda", 0)
    st = torch.cuda.current_stream(dev).cuda_stream
    (K, _), (C, _) = _dev_lists(keys, cnt, dev)
    i64 = lambda n: torch.zeros(max(n, 1), dtype=torch.int64, device=dev)  # noqa: E731
    i32 = lambda n: torch.zeros(max(n, 1), dtype=torch.int32, device=dev)  # noqa: E731
    smp, gs, ec, gec = i64(nq * (k // g)), i64(W * nq * (k // g)), i32(2 * nq), i32(W * 2 * nq)
    off, tot, buf, g2 = i64(W * nq), i64(W), i64(nq * k), i64(W * nq * k)
    out, g_n = i64(W * nq * k), i32(W * nq)
    emax = nq * k

    def sample(keys=K, counts=C, n_q=nq, k=k, g=g, samples=smp):
        return lib.di_xchg_sample(P(keys), P(counts), n_q, k, g, P(samples), 0, st)

    def count(gs=gs, world=W, keys=K, counts=C, n_q=nq, k=k, g=g, ec=ec):
        return lib.di_xchg_count(P(gs), world, P(keys), P(counts), n_q, k, g, P(ec), 0, st)

    def offsets(gec=gec, world=W, n_q=nq, off=off, tot=tot):
        return lib.di_xchg_offsets(P(gec), world, n_q, P(off), P(tot), 0, st)

    def pack(keys=K, ec=ec, off=off, n_q=nq, k=k, buf=buf):
        return lib.di_xchg_pack(P(keys), P(ec), P(off), n_q, k, P(buf), 0, st)

    def unpack(g2=g2, emax=emax, gec=gec, off=off, world=W, n_q=nq, k=k, out=out, g_n=g_n):
        return lib.di_xchg_unpack(P(g2), emax, P(gec), P(off), world, n_q, k, P(out), P(g_n), 0,
                                  st)

    bad = [
        (sample, dict(g=0)), (sample, dict(g=k + 1)), (sample, dict(k=0)), (sample, dict(k=0, g=0)),
        (sample, dict(n_q=-1)), (sample, dict(keys=None)), (sample, dict(counts=None)),
        (sample, dict(samples=None)),
        (count, dict(g=0)), (count, dict(g=k + 1)), (count, dict(k=0)), (count, dict(k=0, g=0)),
        (count, dict(world=0)), (count, dict(n_q=-1)), (count, dict(gs=None)),
        (count, dict(keys=None)), (count, dict(counts=None)), (count, dict(ec=None)),
        (offsets, dict(world=0)), (offsets, dict(n_q=-1)), (offsets, dict(gec=None)),
        (offsets, dict(off=None)), (offsets, dict(tot=None)),
        (pack, dict(k=0)), (pack, dict(n_q=-1)), (pack, dict(keys=None)), (pack, dict(ec=None)),
        (pack, dict(off=None)), (pack, dict(buf=None)),
        (unpack, dict(k=0)), (unpack, dict(world=0)), (unpack, dict(n_q=-1)),
        (unpack, dict(gec=None)), (unpack, dict(off=None)), (unpack, dict(out=None)),
        (unpack, dict(g_n=None)), (unpack, dict(g2=None)), (unpack, dict(emax=-1)),
        (unpack, dict(emax=-1, g2=None)),
    ]
    for fn, kw in bad:
        assert fn(**kw) == L.DI_EINVAL, (fn.__name__, kw)
        assert lib.di_last_error()  # (a message is left for check())
    torch.cuda.synchronize()
    # nothing was launched: every output buffer is as it was
    for t in (smp, ec, off, tot, buf, out, g_n):
        assert not t.any()
    mk, mn = _device_steps_equal_definition(L, keys, cnt, k, g, d)
    _merge_equals_full_lists(mk, mn, keys, cnt, k)
