"""Encode loop: documents -> impact TSV (reference src/deep_impact/indexing/indexer.py
and src/deep_impact/index.py).

Indexer.index(batch, file) writes exactly the reference's bytes: one line per
document, ', '.join(f'{term}: {round(impact, 3)}'), terms in first-occurrence
order.  The forward, head, gather and 3-decimal rounding run on the GPU (di_encode
with DI_F_ROUND3); the text is produced by the native formatter
(di_format_impact_lines).

Tokenization and term extraction (A3, host hot loop #1) run either in-process (the
Rust tokenizer's batched call) or, like the reference's 8-process Pool
(indexer.py:29, :41), in a TokenizerPool of worker processes: the batch goes out in
chunks, and the GPU encodes chunk i while the workers tokenize the chunks after it.
Chunking never changes the output bytes.
"""
from __future__ import annotations

import multiprocessing as mp
from pathlib import Path
from typing import List, Optional, Sequence

from . import _lib
from .models import DeepImpact

# --------------------------------------------------------------------------- workers
_W = {}


def _tok_init(tok_json: str, max_length: int, term_mapping: str,
              rayon_threads: Optional[int] = None) -> None:
    import os

    if rayon_threads and "RAYON_NUM_THREADS" not in os.environ:
        # before the first batched call starts the tokenizers' thread pool
        os.environ["RAYON_NUM_THREADS"] = str(rayon_threads)
    from tokenizers import Tokenizer

    DeepImpact.tokenizer = Tokenizer.from_str(tok_json)
    DeepImpact.term_mapping = term_mapping
    _W["max_length"] = max_length


def _tok_chunk(docs: Sequence[str]):
    # packed numpy arrays + the terms as one UTF-8 blob: cheap to pickle back to the
    # parent, and the parent formats the lines without per-term Python objects
    return DeepImpact.pack_processed_blob(DeepImpact.process_documents(docs, _W["max_length"]))


def _tok_rate(docs: Sequence[str]) -> float:
    """One worker's tokenize + term-extraction rate (docs/s) over `docs` (the bench's
    host budget of the index CLI: indexer.py:28-33 is the reference loop it replaces)."""
    import time

    t0 = time.perf_counter()
    _tok_chunk(docs)
    return len(docs) / max(time.perf_counter() - t0, 1e-9)


def pool_supported() -> bool:
    """Spawned workers re-import the parent's __main__: impossible when it is not a
    file or module (stdin, -c); callers then tokenize in-process."""
    import os
    import sys

    main = sys.modules.get("__main__")
    if getattr(main, "__spec__", None) is not None:
        return True
    f = getattr(main, "__file__", None)
    return f is None or os.path.isfile(f)


def worker_threads(num_processes: int) -> int:
    """Threads of each worker's batched tokenizer call.  The tokenizers' pool defaults
    to every CPU the process may run on: on a share of a large machine (OMP_NUM_THREADS
    names the share) N workers would each start that many.  Measured with 16 workers on
    the GPU box (16 of 256 CPUs): default 7.7 k, 1-4 threads 9.8-9.9 k docs/s end to end;
    8 workers on 8 CPUs here: 2-4 threads 4.3-4.4 k, default 4.0 k docs/s."""
    import os

    share = len(os.sched_getaffinity(0)) if hasattr(os, "sched_getaffinity") else (os.cpu_count() or 1)
    omp = os.environ.get("OMP_NUM_THREADS", "")
    if omp.isdigit() and int(omp) > 0:
        share = min(share, int(omp))
    return max(2, min(4, share // max(1, num_processes)))


class TokenizerPool:
    """Worker processes running DeepImpact.process_documents (xlmr_original.py:120-189)
    with the parent's tokenizer, max_length and term mapping.

    Start it BEFORE the GPU is initialised (index.run does): the workers are spawned
    interpreters that never touch the GPU."""

    def __init__(self, num_processes: int, tokenizer, max_length: int,
                 term_mapping: str = "word_ids"):
        from .models import load_tokenizer

        tok = load_tokenizer(tokenizer)
        ctx = mp.get_context("spawn")
        self.n = num_processes
        self.pool = ctx.Pool(num_processes, initializer=_tok_init,
                             initargs=(tok.to_str(), max_length, term_mapping,
                                       worker_threads(num_processes)))

    def imap(self, chunks):
        return self.pool.imap(_tok_chunk, chunks)

    def worker_rate(self, docs: Sequence[str]) -> float:
        """docs/s of one worker over `docs` (the pool otherwise idle)."""
        return self.pool.apply(_tok_rate, (list(docs),))

    def close(self) -> None:
        self.pool.close()
        self.pool.join()

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()


DEVICE_DOCS = 4096  # documents per device call when tokenizer chunks are merged
PAIR_STEP_T2 = 1 << 32  # di_encode_pairwise: the sum of T_d^2 over the documents of a call


def _slice_packed_blob(packed, lo, hi):
    """Documents [lo, hi) of a pack_processed_blob batch, as such a batch."""
    ids, cu, blob, term_off, tt, ct = packed
    t0, t1 = int(ct[lo]), int(ct[hi])
    return (ids[cu[lo]:cu[hi]], (cu[lo:hi + 1] - cu[lo]).astype(cu.dtype),
            blob[int(term_off[t0]):int(term_off[t1])],
            (term_off[t0:t1 + 1] - term_off[t0]).astype(term_off.dtype), tt[t0:t1],
            (ct[lo:hi + 1] - ct[lo]).astype(ct.dtype))


def _pair_step_ranges(ct, budget):
    """[lo, hi) document ranges of a batch whose sums of T_d^2 stay within `budget` (a
    document over it alone gets a range of its own: the library refuses it)."""
    import numpy as np

    t2 = np.diff(np.asarray(ct, np.int64)) ** 2
    out, lo, run = [], 0, 0
    for d, x in enumerate(t2.tolist()):
        if d > lo and run + x > budget:
            out.append((lo, d))
            lo, run = d, 0
        run += x
    if len(t2) > lo:
        out.append((lo, len(t2)))
    return out


class _Writer:
    """One background thread that formats and writes batches in submission order, so
    that a batch's formatting (native, the GIL released) and its file write overlap the
    next batch's device encode.  An exception in a job is raised at the next put /
    drain."""

    def __init__(self):
        import queue
        import threading

        self.q = queue.Queue(maxsize=4)
        self.err = None
        self.t = threading.Thread(target=self._run, name="di-index-writer", daemon=True)
        self.t.start()

    def _run(self):
        while True:
            job = self.q.get()
            try:
                if job is None:
                    return
                if self.err is None:
                    job()
            except BaseException as e:  # (re-raised in the caller's thread)
                self.err = e
            finally:
                self.q.task_done()

    def _check(self):
        if self.err is not None:
            err, self.err = self.err, None
            raise err

    def put(self, job):
        self._check()
        self.q.put(job)

    def drain(self):
        self.q.join()
        self._check()

    def close(self):
        self.q.put(None)
        self.t.join()
        self._check()


class Indexer:
    def __init__(self, model: DeepImpact, model_batch_size: int = 32, num_processes: int = 8,
                 pool: Optional[TokenizerPool] = None):
        self.model = model
        # the GPU takes far bigger batches than the reference's DataParallel default;
        # batch sizes never change the output bytes
        self.batch_size = max(model_batch_size, 256)
        self.num_processes = num_processes
        self.pool = pool  # None: tokenize in this process
        self._writer = None  # (pool path: formatting + writes behind the next encode)

    def _chunks(self, batch: Sequence[str]):
        # with a pool: enough chunks to keep every worker busy (down to 64 docs each)
        step = self.batch_size
        if self.pool is not None and batch:
            step = max(64, min(step, -(-len(batch) // self.pool.n)))
        return [batch[s:s + step] for s in range(0, len(batch), step)]

    def encode(self, batch: Sequence[str]):
        out: List = []
        if self.pool is not None:
            for ids, cu, blob, term_off, tt, ct in self.pool.imap(self._chunks(batch)):
                terms = [blob[term_off[i]:term_off[i + 1]].decode("utf-8")
                         for i in range(len(term_off) - 1)]
                out += self.model.encode_packed_terms((ids, cu, terms, tt, ct), round3=True)
        else:
            for c in self._chunks(batch):
                out += self.model.encode_processed(
                    self.model.process_documents(c, self.model.max_length), round3=True)
        return out

    def submit(self, batch: Sequence[str]):
        """Start tokenizing `batch` in the pool (returns at once); finish() encodes and
        writes it.  One submitted batch ahead keeps the workers busy while the GPU
        encodes the current one."""
        if self.pool is None:
            return (batch, None)
        return (batch, self.pool.imap(self._chunks(batch)))

    def finish(self, handle, file, wait: bool = True) -> None:
        """indexer.py:31-68: file.write('\\n'.join(lines) + '\\n').  wait=False (the
        pool path): return once the batch is encoded; its formatting and write run on
        the writer thread, in order, while the caller encodes the next batch --
        drain() (or a later finish with wait=True) completes them."""
        batch, it = handle
        if it is None:
            impacts = self.encode(batch)
            text = _lib.format_impact_lines([[t for t, _ in d] for d in impacts],
                                            [[v for _, v in d] for d in impacts])
            self.drain()  # (earlier deferred writes first)
            file.write(text if batch else "\n")
            file.flush()
            return
        # the workers' chunks are merged into device batches of up to DEVICE_DOCS
        # documents (a 100-doc chunk leaves most of the GPU idle), in order
        enc = getattr(self.model, "encode_packed_impacts", None)
        parts, n, jobs = [], 0, []

        def encode(parts):
            packed = DeepImpact.merge_packed_blobs(parts)
            if enc is not None:
                jobs.append(enc(packed))
            else:
                text = self.model.encode_packed_text(packed)
                jobs.append(lambda: text)

        for p in it:
            parts.append(p)
            n += len(p[1]) - 1
            if n >= DEVICE_DOCS:
                encode(parts)
                parts, n = [], 0
        if parts:
            encode(parts)

        def write():
            text = "".join(j() for j in jobs)
            # '\\n'.join(lines) + '\\n' == every line + '\\n', except for an empty batch
            file.write(text if batch else "\n")
            file.flush()

        if self._writer is None:
            self._writer = _Writer()
        self._writer.put(write)
        if wait:
            self._writer.drain()

    def drain(self) -> None:
        """Wait for the deferred formatting and writes (re-raises their errors)."""
        if self._writer is not None:
            self._writer.drain()

    def index(self, batch: Sequence[str], file) -> None:
        """indexer.py:31-68: file.write('\\n'.join(lines) + '\\n')."""
        self.finish(self.submit(batch), file)

    def build_index(self, documents_or_batches, max_val=None, index_path=None, file=None,
                    layout="device"):
        """Index these documents and search them, in one process: the InvertedIndex the text
        route (index -> quantize -> inverted_index -> InvertedIndex(path)) gives for the
        same collection, without its files.  The round3 impacts of every device step stay
        on the GPU and go to an IndexBuilder; the terms are numbered by a TermTable from
        the tokenizer's blob.  documents_or_batches: a sequence of passages, or an iterable
        of such batches (document ids count on across them).  A DeepPairwiseImpact model
        gives the index of index --pairwise -> quantize -> inverted_index, 't1|t2' terms
        included.  max_val: quantize's -m.
        index_path: also write vocab.txt / inverted_index.idx / inverted_index.dat there.
        file: also write the impact TSV there, from the same encode.
        layout: "host" or "device", where the scorer's blocked layout is built
        (InvertedIndex.from_builder); the index is the same."""
        docs = documents_or_batches
        batches = [docs] if isinstance(docs, (list, tuple)) and (not docs or isinstance(docs[0], str)) \
            else docs
        build = IndexBuild(self, write_tsv=file is not None)
        pending = None
        for batch in batches:  # tokenized one batch ahead, as index.py's loop
            handle = build.submit(batch)
            if pending is not None:
                build.finish(pending, file)
            pending = handle
        if pending is not None:
            build.finish(pending, file)
        ix = build.inverted_index(max_val, index_path, layout=layout)
        self.build_ms, self.last_build = build.ms, build
        return ix


class IndexBuild:
    """The device route from documents to the quantized index, one batch at a time: the
    submit / finish protocol of Indexer (so index.py's loop drives either), the impacts
    appended to an IndexBuilder instead of formatted -- and formatted as well when the
    impact TSV is wanted (write_tsv: the bytes of Indexer.index).  With a
    DeepPairwiseImpact the pair scores stay on the device as well (_pair_step) and the
    index holds the 't1|t2' terms; its bf16 precision is refused, as in the encoder."""

    def __init__(self, indexer: "Indexer", write_tsv: bool = True):
        from .models import DeepPairwiseImpact

        model = indexer.model
        if not hasattr(model, "encoder"):
            raise ValueError("the device index route needs a DeepImpact or DeepPairwiseImpact "
                             "model on a DeviceEncoder")
        self.pairwise = isinstance(model, DeepPairwiseImpact)
        if self.pairwise and getattr(model.encoder, "precision", None) == "bf16":
            raise ValueError("DeepPairwiseImpact runs at fp32 or bf16x3")
        self.indexer, self.model, self.write_tsv = indexer, model, write_tsv
        self.device = getattr(model.encoder, "device", 0) or 0
        self.table = _lib.TermTable()
        self.builder = _lib.IndexBuilder(self.device)
        self.ms = {"tokenize": 0.0, "encode": 0.0, "build": 0.0}

    def submit(self, batch: Sequence[str]):
        return self.indexer.submit(batch)

    def _packed_steps(self, handle):
        """The batch as pack_processed_blob device steps of up to DEVICE_DOCS documents."""
        import time

        batch, it = handle
        if it is None:
            def chunks():
                for c in self.indexer._chunks(batch):
                    yield DeepImpact.pack_processed_blob(
                        self.model.process_documents(c, self.model.max_length))
            it = chunks()
        parts, n = [], 0
        while True:
            t0 = time.perf_counter()
            p = next(it, None)
            self.ms["tokenize"] += (time.perf_counter() - t0) * 1e3
            if p is None:
                break
            parts.append(p)
            n += len(p[1]) - 1
            if n >= DEVICE_DOCS:
                yield DeepImpact.merge_packed_blobs(parts)
                parts, n = [], 0
        if parts:
            yield DeepImpact.merge_packed_blobs(parts)

    def _step(self, packed) -> str:
        import time

        import numpy as np
        import torch

        if self.pairwise:
            return "".join(self._pair_step(_slice_packed_blob(packed, lo, hi))
                           for lo, hi in _pair_step_ranges(packed[5], PAIR_STEP_T2))
        ids, cu, blob, term_off, tt, ct = packed
        t0 = time.perf_counter()
        dev = torch.device("cuda", self.device)
        n_docs, n_terms = len(cu) - 1, int(ct[-1])
        tid = self.table.intern(blob, term_off).view(np.int32)
        pad = lambda a: a if a.size else np.zeros(1, np.int32)  # noqa: E731
        d_ids = torch.from_numpy(pad(np.ascontiguousarray(ids, np.int32))).to(dev)
        d_cu = torch.from_numpy(np.ascontiguousarray(cu, np.int32)).to(dev)
        d_tt = torch.from_numpy(pad(np.ascontiguousarray(tt, np.int32))).to(dev)
        d_ct = torch.from_numpy(np.ascontiguousarray(ct, np.int32)).to(dev)
        d_tid = torch.from_numpy(pad(tid)).to(dev)
        d_imp = torch.empty(max(1, n_terms), dtype=torch.float32, device=dev)
        t1 = time.perf_counter()
        # synchronous at return (no DI_F_ASYNC): the builder's stream may read d_imp
        self.model.encoder.encode_device(d_ids, d_cu, n_docs, int(cu[-1]),
                                         int(np.diff(cu).max(initial=0)), d_tt, d_ct, n_terms,
                                         d_imp, flags=_lib.DI_F_DEVICE_PTRS | _lib.DI_F_ROUND3)
        t2 = time.perf_counter()
        self.builder.append(d_tid, d_imp, d_ct, timing=True)
        text = ""
        if self.write_tsv:
            text = _lib.format_impact_lines_packed(blob, term_off, d_imp[:n_terms].cpu().numpy(), ct)
        t3 = time.perf_counter()
        self.ms["encode"] += (t2 - t1) * 1e3
        self.ms["build"] += (t1 - t0 + t3 - t2) * 1e3
        return text

    def _pair_step(self, packed) -> str:
        """One device step of the pairwise model: the unrounded single and pair scores of
        encode_pairwise stay in torch buffers and go to the builder (which rounds them);
        for the TSV the same buffers are ordered on the device (di_pairwise_order, round3)
        and only the entries come to the host."""
        import time

        import numpy as np
        import torch

        ids, cu, blob, term_off, tt, ct = packed
        t0 = time.perf_counter()
        dev = torch.device("cuda", self.device)
        n_docs, n_terms = len(cu) - 1, int(ct[-1])
        tid = self.table.intern(blob, term_off).view(np.int32)
        tt, ct = np.asarray(tt, np.int32)[:n_terms], np.ascontiguousarray(ct, np.int32)
        T = np.diff(ct.astype(np.int64))
        cu_pairs = np.zeros(n_docs + 1, np.int64)
        cu_pairs[1:] = np.cumsum(T * (T - 1) // 2)
        n_pairs = int(cu_pairs[-1])
        # the encoder and the builder take a document's terms in token order; the
        # bert_legacy maps can differ from it (models._encode_entries_device)
        asc = np.ones(n_terms, bool)
        asc[1:] = tt[1:] > tt[:-1]
        asc[ct[:-1][ct[:-1] < n_terms]] = True
        by_tok = pos = None
        if not asc.all():
            tdoc = np.repeat(np.arange(n_docs), T)
            by_tok = np.lexsort((tt, tdoc))
            pos = (by_tok - ct[tdoc]).astype(np.int32)
            tt, tid = tt[by_tok], tid[by_tok]
        pad = lambda a, dt=np.int32: a if a.size else np.zeros(1, dt)  # noqa: E731
        up = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)  # noqa: E731
        d_ids, d_cu = up(pad(np.ascontiguousarray(ids, np.int32))), up(np.asarray(cu, np.int32))
        d_tt, d_ct, d_tid, d_cup = up(pad(tt)), up(ct), up(pad(tid)), up(cu_pairs)
        d_single = torch.empty(max(1, n_terms), dtype=torch.float32, device=dev)[:n_terms]
        d_pair = torch.empty(max(1, n_pairs), dtype=torch.float32, device=dev)[:n_pairs]
        t1 = time.perf_counter()
        # synchronous at return (no DI_F_ASYNC): the builder's stream may read the buffers
        self.model.encoder.encode_pairwise_device(
            d_ids, d_cu, n_docs, int(cu[-1]), int(np.diff(cu).max(initial=0)), d_tt, d_ct,
            n_terms, d_cup, n_pairs, d_single, d_pair, None, flags=_lib.DI_F_DEVICE_PTRS)
        t2 = time.perf_counter()
        self.builder.append_pairwise(d_tid, d_single, d_pair, d_ct, d_cup, timing=True)
        text = ""
        if self.write_tsv:
            d_pos = up(pos) if pos is not None else None
            cu_out, first, second, score = _lib.pairwise_order(
                d_single, d_pair, d_ct, d_cup, d_pos, round3=True, device=self.device)
            cu_out, first = cu_out.cpu().numpy(), first.cpu().numpy()
            second, score = second.cpu().numpy(), score.cpu().numpy()
            if by_tok is not None:  # sorted-term indices back to the blob's (map) order
                by32 = by_tok.astype(np.int32)
                first, second = by32[first], np.where(second >= 0, by32[np.maximum(second, 0)],
                                                      np.int32(-1)).astype(np.int32)
            text = _lib.format_entry_lines(blob, term_off, first, second, score, cu_out)
        t3 = time.perf_counter()
        self.ms["encode"] += (t2 - t1) * 1e3
        self.ms["build"] += (t1 - t0 + t3 - t2) * 1e3
        return text

    def finish(self, handle, file, wait: bool = True) -> None:
        import numpy as np

        batch = handle[0]
        if not batch:
            # the reference writes an empty line for an empty batch (indexer.py:68): a
            # document without terms, which quantize refuses on either route
            self.builder.append(np.zeros(0, np.uint32), np.zeros(0, np.float32),
                                np.zeros(2, np.int32))
            text = "\n"
        else:
            text = "".join(self._step(p) for p in self._packed_steps(handle))
        if self.write_tsv and file is not None:
            file.write(text)
            file.flush()

    def index(self, batch: Sequence[str], file) -> None:
        self.finish(self.submit(batch), file)

    def drain(self) -> None:
        pass

    def inverted_index(self, max_val=None, index_path=None, layout="device"):
        """Quantize, number the terms, fetch the postings (sorted on the GPU) and create the
        device index -> InvertedIndex."""
        import time

        from .inverted_index import InvertedIndex

        if max_val is not None and max_val == 0:
            raise ZeroDivisionError("float division by zero")  # quantize.py:37
        if max_val is not None and max_val < 0:
            raise ValueError("a negative max_val empties every line: use the text route")
        t0 = time.perf_counter()
        self.max_used, _, _ = self.builder.quantize(len(self.table), max_val, timing=True)
        ix = InvertedIndex.from_builder(self.builder, self.table, device=self.device,
                                        index_path=index_path, timing=True, layout=layout)
        self.ms["build"] += (time.perf_counter() - t0) * 1e3
        return ix


def resolve_tokenizer(model_checkpoint_path, tokenizer_path):
    """The tokenizer DeepImpact.load would pick (explicit path, else the checkpoint
    directory's tokenizer.json)."""
    if tokenizer_path is not None:
        return tokenizer_path
    p = Path(model_checkpoint_path) if model_checkpoint_path is not None else None
    if p is not None and p.is_dir() and (p / "tokenizer.json").exists():
        return p / "tokenizer.json"
    return None
