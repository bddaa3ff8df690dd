"""di_topk_merge called directly on every route of launch_merge (csrc/topk_merge.hip): the cases
of tests/merge_cases.py (tests/test_merge_cases_cpu.py proves that they reach every kernel
and branch), each in the query-major and the lists-major layout, on host pointers and on
device pointers with DI_F_ASYNC on a torch stream -- the call parallel._exchange_merge
makes.  The output is defined by merge_cases.reference_merge alone (the keys are unique
and totally ordered): counts and keys must match bit for bit."""
import numpy as np
import pytest
import torch

import merge_cases as M

pytestmark = pytest.mark.gpu

DI_EINVAL, DI_ERANGE = -1, -4


@pytest.fixture(scope="module")
def L():
    from improving_learned_index_amd import _lib

    if _lib.device_count() < 1:
        pytest.fail("no HIP device visible (GPU test run without a GPU)")
    return _lib


def _check(got_key, got_n, want_key, want_n, what):
    assert (got_n == want_n).all(), (what, got_n.tolist(), want_n.tolist())
    for q in range(len(want_n)):
        n = max(int(want_n[q]), 0)
        assert (got_key[q, :n] == want_key[q, :n]).all(), (what, q)


def _device(L, buf_keys, buf_counts, n_q, n_lists, k, flags, stream):
    dev = torch.device("cuda", 0)
    tk = torch.from_numpy(buf_keys.reshape(-1).view(np.int64).copy()).to(dev)
    tc = torch.from_numpy(buf_counts.reshape(-1).copy()).to(dev)
    out = torch.full((n_q * k,), -1, dtype=torch.int64, device=dev)
    on = torch.full((n_q,), -7, dtype=torch.int32, device=dev)
    stream.wait_stream(torch.cuda.current_stream(dev))
    L.topk_merge_device(tk, tc, n_q, n_lists, k, out, on, device=0, stream=stream.cuda_stream,
                        flags=L.DI_F_DEVICE_PTRS | L.DI_F_ASYNC | flags)
    stream.synchronize()
    return out.cpu().numpy().view(np.uint64).reshape(n_q, k), on.cpu().numpy()


@pytest.mark.parametrize("case", M.CASES, ids=M.case_id)
def test_merge_equals_definition(L, case):
    n_lists, k, _, mode, _ = case
    keys, counts = M.case_lists(case)
    n_q = keys.shape[0]
    want_key, want_n = M.reference_merge(keys, counts, k)
    if mode == "rejected":  # the rejected query and only it
        assert (want_n < 0).tolist() == [q == 1 for q in range(n_q)]
    # the same data, lists-major: [n_lists][n_q][k] (the shape below is only how
    # _lib.topk_merge reads n_q and n_lists)
    lm_keys = np.ascontiguousarray(keys.transpose(1, 0, 2)).reshape(n_q, n_lists, k)
    lm_counts = np.ascontiguousarray(counts.T).reshape(n_q, n_lists)
    _check(*L.topk_merge(keys, counts, k), want_key, want_n, "query-major, host")
    _check(*L.topk_merge(lm_keys, lm_counts, k, flags=L.DI_F_LISTS_MAJOR), want_key, want_n,
           "lists-major, host")
    stream = torch.cuda.Stream(torch.device("cuda", 0))
    _check(*_device(L, keys, counts, n_q, n_lists, k, 0, stream), want_key, want_n,
           "query-major, device")
    _check(*_device(L, lm_keys, lm_counts, n_q, n_lists, k, L.DI_F_LISTS_MAJOR, stream),
           want_key, want_n, "lists-major, device")


def test_merge_argument_errors(L):
    keys = np.full((2, 3, 8), 5, np.uint64)
    counts = np.zeros((2, 3), np.int32)
    out, n = np.zeros((2, 4097), np.uint64), np.zeros(2, np.int32)
    lib, P = L.lib(), L.ptr
    for k in (0, 4097):
        assert lib.di_topk_merge(P(keys), P(counts), 2, 3, k, P(out), P(n), 0, None, 0) == DI_ERANGE
        with pytest.raises(L.DIError) as e:
            L.topk_merge(np.zeros((2, 3, k), np.uint64), counts, k)
        assert e.value.code == DI_ERANGE
    assert lib.di_topk_merge(P(keys), P(counts), 2, 0, 8, P(out), P(n), 0, None, 0) == DI_EINVAL
    assert lib.di_topk_merge(P(keys), P(counts), -1, 3, 8, P(out), P(n), 0, None, 0) == DI_EINVAL
    # no queries: returns cleanly and writes nothing
    out[:], n[:] = 9, 9
    assert lib.di_topk_merge(P(keys), P(counts), 0, 3, 8, P(out), P(n), 0, None, 0) == 0
    assert (out == 9).all() and (n == 9).all()
    mk, mn = L.topk_merge(np.zeros((0, 3, 8), np.uint64), np.zeros((0, 3), np.int32), 8)
    assert mk.shape == (0, 8) and mn.shape == (0,)
