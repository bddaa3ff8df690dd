"""Several ranks of a torch.distributed program played in one process, one after another.

Every collective in the retrieve exchange (parallel.exchange_topk and what calls it) is an
all_gather_into_tensor of data each rank computes deterministically from its own inputs
and from earlier collectives.  That lets the ranks run in turn, with no threads, no
subprocesses and one process holding the GPU: run_world patches torch.distributed so that
an all_gather is answered from a log of every rank's contribution once the log holds all
of them, and otherwise records this rank's contribution and unwinds the rank (_Suspend).
Rounds repeat -- every rank re-run from the start, re-playing its earlier collectives from
the log -- until every rank returns: c collectives cost c + 1 runs per rank.

What a real collective would hang or corrupt memory on is asserted instead: in a round
every rank stops at the same call with the same input shape and dtype, the output holds
world inputs, and a re-played input equals the logged one bit for bit (the rank bodies
must be deterministic).  Rounds are capped, so a disagreement fails and cannot spin.
"""
import torch

MAX_ROUNDS = 8


class _Suspend(BaseException):
    """Unwinds a rank at a collective whose other contributions are not logged yet.
    (BaseException: an `except Exception` in the code played must not swallow it.)"""

    def __init__(self, call, shape, dtype):
        super().__init__(call)
        self.call, self.shape, self.dtype = call, shape, dtype


def _bits(t):
    return t.detach().contiguous().reshape(-1).view(torch.uint8)


def run_world(monkeypatch, world, body, backend="nccl"):
    """body(rank) for rank 0 .. world-1 under replayed collectives -> [result per rank]."""
    import torch.distributed as dist

    log = []  # log[i][rank] = the rank's input to its i-th collective
    now = {"rank": None, "call": 0}

    def all_gather_into_tensor(out, inp, group=None, async_op=False):
        assert not async_op
        rank, i = now["rank"], now["call"]
        now["call"] += 1
        assert out.numel() == world * inp.numel(), (rank, i, out.shape, inp.shape)
        assert out.dtype == inp.dtype and out.device == inp.device, (rank, i)
        assert out.is_contiguous() and inp.is_contiguous(), (rank, i)
        if i == len(log):
            log.append({})
        assert i < len(log), (rank, i, len(log))
        entry = log[i]
        if rank in entry:
            was = entry[rank]
            assert was.shape == inp.shape and was.dtype == inp.dtype, (rank, i)
            assert torch.equal(_bits(was), _bits(inp)), f"rank {rank}: call {i} re-played differently"
        if len(entry) == world:
            out.reshape(-1).copy_(torch.cat([entry[r].reshape(-1) for r in range(world)]))
            return None
        if rank not in entry:
            entry[rank] = inp.detach().clone()
            if inp.is_cuda:  # (ranks may run on streams of their own: the log is complete data)
                torch.cuda.synchronize(inp.device)
        raise _Suspend(i, tuple(inp.shape), inp.dtype)

    with monkeypatch.context() as m:
        m.setattr(dist, "get_world_size", lambda group=None: world)
        m.setattr(dist, "get_rank", lambda group=None: now["rank"])
        m.setattr(dist, "get_backend", lambda group=None: backend)
        m.setattr(dist, "all_gather_into_tensor", all_gather_into_tensor)
        for _ in range(MAX_ROUNDS):
            results, stops = [], []
            for rank in range(world):
                now["rank"], now["call"] = rank, 0
                try:
                    results.append(body(rank))
                    stops.append(None)
                except _Suspend as s:
                    results.append(None)
                    stops.append((s.call, s.shape, s.dtype))
            # every rank at the same collective with the same input, or every rank done
            assert all(s == stops[0] for s in stops), f"the ranks disagree: {stops}"
            if stops[0] is None:
                return results
        raise AssertionError(f"no end after {MAX_ROUNDS} rounds ({len(log)} collectives logged)")
