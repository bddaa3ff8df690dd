"""ctypes binding of libdeepimpact_hip.so (the C ABI in include/deepimpact.h).

The HIP library is the product path: there is no CPU fallback.  If the shared
object is missing or cannot be loaded this module raises ImportError-like
errors at first use, loudly.
"""
from __future__ import annotations

import ctypes
import os
from pathlib import Path

import numpy as np

_HERE = Path(__file__).resolve().parent
LIB_PATH = Path(os.environ.get("DEEPIMPACT_HIP_LIB", _HERE / "libdeepimpact_hip.so"))

DI_OK = 0
DI_F_DEVICE_PTRS = 0x1
DI_F_ASYNC = 0x2
DI_F_TIMING = 0x4
DI_F_LISTS_MAJOR = 0x8
DI_SHORT_QUERY_TERMS = 256  # longer queries: wide merge keys (include/deepimpact.h)
DI_MAX_QUERY_TERMS = 4096
DI_MAX_TOPK = 4096
DI_PAIR_ORDER_LDS_KEYS = 16384  # entries one workgroup orders in LDS (include/deepimpact.h)
DI_PAIR_ORDER_MAX_TERMS = 2047
DI_TERM_STORE_MAX_TERMS = 2048  # pairs of one passage of a TermStore (include/deepimpact.h)
DI_F_ROUND3 = 0x10
DI_ERANGE = -4
DI_EINVAL = -1
DI_EFORMAT = -7
DI_INDEX_BUILD_TILE = 4096  # postings one workgroup of the index builder's sort places
DI_MAX_SPARSE_DOCS = 16777215  # documents of a float index (include/deepimpact.h)
SPARSE_BLOCK_DOCS = 16384  # documents of one block of the float index's layout

_ERRNAMES = {-1: "DI_EINVAL", -2: "DI_ENOMEM", -3: "DI_EHIP", -4: "DI_ERANGE",
             -5: "DI_ENODEV", -6: "DI_EIO", -7: "DI_EFORMAT"}


class DIError(RuntimeError):
    def __init__(self, code, msg):
        super().__init__(f"{_ERRNAMES.get(code, code)}: {msg}")
        self.code = code


class di_timing(ctypes.Structure):
    _fields_ = [("ms", ctypes.c_double), ("launches", ctypes.c_int64)]


class di_synth_skew(ctypes.Structure):
    _fields_ = [("term_rank0", ctypes.c_double), ("term_exp", ctypes.c_double),
                ("cluster_docs", ctypes.c_int32), ("cluster_sigma", ctypes.c_double),
                ("doc_sigma", ctypes.c_double), ("mass_max", ctypes.c_double)]


DI_MAX_PAIR_SPECIALS = 4


class di_pair_format(ctypes.Structure):
    _fields_ = [("prefix", ctypes.c_int32 * DI_MAX_PAIR_SPECIALS), ("n_prefix", ctypes.c_int32),
                ("suffix", ctypes.c_int32 * DI_MAX_PAIR_SPECIALS), ("n_suffix", ctypes.c_int32),
                ("max_length", ctypes.c_int32)]


def pair_format(prefix, suffix, max_length) -> di_pair_format:
    """di_pair_format of a single-sequence template (prefix / suffix special ids)."""
    if len(prefix) > DI_MAX_PAIR_SPECIALS or len(suffix) > DI_MAX_PAIR_SPECIALS:
        raise ValueError(f"at most {DI_MAX_PAIR_SPECIALS} prefix and suffix ids")
    f = di_pair_format()
    for i, t in enumerate(prefix):
        f.prefix[i] = int(t)
    for i, t in enumerate(suffix):
        f.suffix[i] = int(t)
    f.n_prefix, f.n_suffix, f.max_length = len(prefix), len(suffix), int(max_length)
    return f


P = ctypes.c_void_p
I32, I64, U32, U64 = ctypes.c_int32, ctypes.c_int64, ctypes.c_uint32, ctypes.c_uint64

# name -> (restype, argtypes); every symbol include/deepimpact.h declares
SIGNATURES = {
    "di_last_error": (ctypes.c_char_p, []),
    "di_version": (ctypes.c_int, []),
    "di_device_count": (ctypes.c_int, [P]),
    "di_index_create": (ctypes.c_int, [P, I64, P, P, U32, U32, ctypes.c_int, P]),
    "di_index_create_device": (ctypes.c_int, [P, I64, P, P, U32, U32, ctypes.c_int, P, U32, P]),
    "di_index_layout": (ctypes.c_int, [P, P, P, P, P]),
    "di_index_export": (ctypes.c_int, [P, P, P, P, P, P, P, P, P, P, P]),
    "di_index_load_reference": (ctypes.c_int, [ctypes.c_char_p, U32, U32, ctypes.c_int, P]),
    "di_build_reference_index": (ctypes.c_int, [ctypes.c_char_p, ctypes.c_char_p]),
    "di_index_search": (ctypes.c_int, [P, P, P, I32, I32, P, P, P, P, U32]),
    "di_index_reserve": (ctypes.c_int, [P, I32, I32]),
    "di_index_info": (ctypes.c_int, [P, P, P, P, P]),
    "di_index_set_min_impact": (ctypes.c_int, [P, I32]),
    "di_index_set_block_max": (ctypes.c_int, [P, ctypes.c_float]),
    "di_index_set_packed": (ctypes.c_int, [P, I32, P]),
    "di_index_set_stream": (ctypes.c_int, [P, P]),
    "di_index_sync": (ctypes.c_int, [P]),
    "di_index_timing": (ctypes.c_int, [P, ctypes.c_char_p, P, ctypes.c_int]),
    "di_index_destroy": (ctypes.c_int, [P]),
    "di_topk_merge": (ctypes.c_int, [P, P, I32, I32, I32, P, P, ctypes.c_int, P, U32]),
    "di_xchg_sample": (ctypes.c_int, [P, P, I32, I32, I32, P, ctypes.c_int, P]),
    "di_xchg_count": (ctypes.c_int, [P, I32, P, P, I32, I32, I32, P, ctypes.c_int, P]),
    "di_xchg_offsets": (ctypes.c_int, [P, I32, I32, P, P, ctypes.c_int, P]),
    "di_xchg_pack": (ctypes.c_int, [P, P, P, I32, I32, P, ctypes.c_int, P]),
    "di_xchg_unpack": (ctypes.c_int, [P, I64, P, P, I32, I32, I32, P, P, ctypes.c_int, P]),
    "di_encoder_create": (ctypes.c_int, [P, P, I32, ctypes.c_int, P]),
    "di_encode": (ctypes.c_int, [P, P, P, I32, I64, I32, P, P, I64, P, U32]),
    "di_encode_pairwise": (ctypes.c_int, [P, P, P, I32, I64, I32, P, P, I64, P, I64, P, P, P,
                                          U32]),
    "di_pairwise_order": (ctypes.c_int, [P, P, P, P, P, I32, I64, I64, P, P, P, P, I64, P,
                                         ctypes.c_int, P, U32]),
    "di_encode_pairwise_entries": (ctypes.c_int, [P, P, P, I32, I64, I32, P, P, I64, P, I64, P,
                                                  P, P, P, P, I64, P, U32]),
    "di_encoder_reserve": (ctypes.c_int, [P, I64, I32, I64]),
    "di_encoder_set_stream": (ctypes.c_int, [P, P]),
    "di_encoder_sync": (ctypes.c_int, [P]),
    "di_encoder_timing": (ctypes.c_int, [P, ctypes.c_char_p, P, ctypes.c_int]),
    "di_encoder_destroy": (ctypes.c_int, [P]),
    "di_pairs_pack": (ctypes.c_int, [P, P, I32, P, P, I32, P, P, I32, P, P, I64, P, P, P,
                                     ctypes.c_int, P, U32]),
    "di_encode_pairs": (ctypes.c_int, [P, P, P, I32, P, P, I32, P, P, I32, P, P, U32]),
    "di_segment_order": (ctypes.c_int, [P, P, I32, P, ctypes.c_int, P, U32]),
    "di_term_store_create": (ctypes.c_int, [ctypes.c_int, P]),
    "di_term_store_reserve": (ctypes.c_int, [P, I64, I64]),
    "di_term_store_append": (ctypes.c_int, [P, P, P, P, I32, P, P, U32]),
    "di_term_store_info": (ctypes.c_int, [P, P, P, P]),
    "di_term_store_score": (ctypes.c_int, [P, P, P, I32, P, P, P, P, P, U32]),
    "di_term_store_timing": (ctypes.c_int, [P, ctypes.c_char_p, P, ctypes.c_int]),
    "di_term_store_destroy": (ctypes.c_int, [P]),
    "di_quantize": (ctypes.c_int, [P, I64, ctypes.c_double, I32, P, P, ctypes.c_int, P, U32]),
    "di_quantize_file": (ctypes.c_int, [ctypes.c_char_p, ctypes.c_char_p, ctypes.c_double, I32,
                                        ctypes.c_int, P]),
    "di_format_impact_lines": (ctypes.c_int, [P, P, P, P, I32, P, I64, P]),
    "di_format_entry_lines": (ctypes.c_int, [P, P, I64, P, P, P, P, I32, P, I64, P]),
    "di_append_run_lines": (ctypes.c_int, [ctypes.c_char_p, P, P, I32, P, P, P, I32]),
    "di_sparse_create": (ctypes.c_int, [P, I64, P, P, U32, ctypes.c_int, P]),
    "di_sparse_search": (ctypes.c_int, [P, P, P, I32, I32, P, P, P, P, U32]),
    "di_sparse_search_f64": (ctypes.c_int, [P, P, P, I32, I32, P, P, P, U32]),
    "di_sparse_info": (ctypes.c_int, [P, P, P, P, P]),
    "di_sparse_timing": (ctypes.c_int, [P, ctypes.c_char_p, P, ctypes.c_int]),
    "di_sparse_destroy": (ctypes.c_int, [P]),
    "di_sparse_builder_create": (ctypes.c_int, [ctypes.c_int, P]),
    "di_sparse_builder_reserve": (ctypes.c_int, [P, I64, I64]),
    "di_sparse_builder_append": (ctypes.c_int, [P, P, P, P, I32, P, P, U32]),
    "di_sparse_builder_info": (ctypes.c_int, [P, P, P]),
    "di_sparse_builder_finish": (ctypes.c_int, [P, I64, P, U32, P]),
    "di_sparse_builder_destroy": (ctypes.c_int, [P]),
    "di_sparse_export": (ctypes.c_int, [P, P, P, P, P]),
    "di_term_table_create": (ctypes.c_int, [P]),
    "di_term_table_intern": (ctypes.c_int, [P, P, P, I64, P]),
    "di_term_table_info": (ctypes.c_int, [P, P, P]),
    "di_term_table_export": (ctypes.c_int, [P, P, P]),
    "di_term_table_rows": (ctypes.c_int, [P, P, P, P]),
    "di_term_table_rows_pairwise": (ctypes.c_int, [P, P, I64, P, P, P, P]),
    "di_term_table_destroy": (ctypes.c_int, [P]),
    "di_index_builder_create": (ctypes.c_int, [ctypes.c_int, P]),
    "di_index_builder_reserve": (ctypes.c_int, [P, I64, I64]),
    "di_index_builder_append": (ctypes.c_int, [P, P, P, P, I32, P, P, U32]),
    "di_index_builder_append_pairwise": (ctypes.c_int, [P, P, P, P, P, P, I32, I64, P, P, U32]),
    "di_index_builder_pair_terms": (ctypes.c_int, [P, P, P, P, P]),
    "di_index_builder_info": (ctypes.c_int, [P, P, P]),
    "di_index_builder_quantize": (ctypes.c_int, [P, I64, ctypes.c_double, P, U32, P, P, P]),
    "di_index_builder_postings": (ctypes.c_int, [P, P, I64, P, U32, P, P, P]),
    "di_index_builder_timing": (ctypes.c_int, [P, ctypes.c_char_p, P, ctypes.c_int]),
    "di_index_builder_destroy": (ctypes.c_int, [P]),
    "di_write_reference_index": (ctypes.c_int, [ctypes.c_char_p, P, P, I64, P, P, P]),
    "di_write_reference_index_pairwise": (ctypes.c_int, [ctypes.c_char_p, P, I64, P, P, P, I64,
                                                         P, P, P]),
    "di_synth_postings": (ctypes.c_int, [I64, I32, U64, I32, I32, ctypes.c_double, P, P, P, I64,
                                         P, P]),
    "di_synth_postings_skewed": (ctypes.c_int, [I64, I32, U64, I32, I32, ctypes.c_double, P, P,
                                                P, P, I64, P, P]),
    "di_synth_postings_shard": (ctypes.c_int, [I64, I64, I32, U64, I32, I32, ctypes.c_double,
                                               P, ctypes.c_double, P, P, P, I64, P, P]),
    "di_synth_impact_tsv": (ctypes.c_int, [ctypes.c_char_p, I64, I32, U64, I32, I32,
                                           ctypes.c_double, P]),
}

_LIB = None


def hip_runtimes_mapped():
    """Real paths of every libamdhip64 mapped into this process (/proc/self/maps)."""
    found = set()
    try:
        with open("/proc/self/maps") as f:
            for line in f:
                p = line.split(maxsplit=5)
                if len(p) == 6 and "libamdhip64.so" in p[5]:
                    found.add(os.path.realpath(p[5].strip()))
    except OSError:
        pass
    return found


def _torch_lib_dir():
    import importlib.util

    spec = importlib.util.find_spec("torch")
    if spec is None or not spec.origin:
        return None
    return os.path.realpath(os.path.join(os.path.dirname(spec.origin), "lib"))


def _guard_hip_runtime():
    """torch bundles its own libamdhip64.so (SONAME libamdhip64.so.7, like
    /opt/rocm's this library links), and whichever loads first serves both.  So
    when torch is importable, torch's runtime must be the one mapped: import torch
    before loading the library, and refuse if a different HIP runtime is already in
    the process (an embedder that loaded /opt/rocm's first would break torch)."""
    import sys

    tdir = _torch_lib_dir()
    if tdir is None:
        return  # no torch: the library's own runtime (RUNPATH /opt/rocm) serves alone
    if "torch" not in sys.modules:
        foreign = [p for p in hip_runtimes_mapped() if not p.startswith(tdir + os.sep)]
        if foreign:
            raise RuntimeError(
                f"a HIP runtime other than torch's is already loaded ({', '.join(foreign)}); "
                f"torch ({tdir}) would bind to it. Import torch before loading any HIP "
                f"library, or before importing improving_learned_index_amd")
        import torch  # noqa: F401  (maps torch's libamdhip64 first)


def _check_one_runtime():
    rts = hip_runtimes_mapped()
    if len(rts) > 1:
        raise RuntimeError(f"two HIP runtimes are mapped into this process: {sorted(rts)}")


def lib():
    """Load the HIP library (raises if it is missing -- no fallback)."""
    global _LIB
    if _LIB is None:
        if not LIB_PATH.exists():
            raise RuntimeError(
                f"{LIB_PATH} is missing: the HIP extension must be built "
                f"(python -c 'import __graft_entry__; __graft_entry__.build()')")
        _guard_hip_runtime()
        L = ctypes.CDLL(str(LIB_PATH))
        _check_one_runtime()
        # (DI_LIB_ALLOW_MISSING=1: an older build for an A/B run, tools/ab_scorer.sh)
        allow_missing = os.environ.get("DI_LIB_ALLOW_MISSING") == "1"
        for name, (res, args) in SIGNATURES.items():
            if allow_missing and not hasattr(L, name):
                continue
            fn = getattr(L, name)
            fn.restype = res
            fn.argtypes = args
        _LIB = L
    return _LIB


def check(rc):
    if rc != DI_OK:
        raise DIError(rc, lib().di_last_error().decode("utf-8", "replace"))
    return rc


def ptr(a):
    """ctypes pointer of a numpy array or a torch tensor (host or device)."""
    if a is None:
        return None
    if isinstance(a, np.ndarray):
        return ctypes.c_void_p(a.ctypes.data)
    if hasattr(a, "data_ptr"):
        return ctypes.c_void_p(a.data_ptr())
    if isinstance(a, int):
        return ctypes.c_void_p(a)
    raise TypeError(type(a))


def device_count():
    n = ctypes.c_int(0)
    check(lib().di_device_count(ctypes.byref(n)))
    return n.value


def version():
    v = lib().di_version()
    return (v >> 16, v & 0xFFFF)


def csr(queries):
    """list of term-id lists -> (uint32 terms, int32 cu)."""
    cu = np.zeros(len(queries) + 1, np.int32)
    for i, q in enumerate(queries):
        cu[i + 1] = cu[i] + len(q)
    flat = np.fromiter((t for q in queries for t in q), np.uint32, count=int(cu[-1]))
    return flat, cu


class _Handle:
    """A native handle in _h, destroyed once by the <_family>_destroy call."""

    _family = ""

    def close(self):
        if getattr(self, "_h", None):
            getattr(lib(), self._family + "_destroy")(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


class _TimedHandle(_Handle):
    """A handle whose family reads its DI_F_TIMING regions with <_family>_timing."""

    def timing(self, name, reset=False):
        t = di_timing()
        check(getattr(lib(), self._family + "_timing")(self._h, name.encode(), ctypes.byref(t),
                                                       int(reset)))
        return t.ms, t.launches


def _query_arrays(q_terms, cu_q, k, score_dtype, with_keys):
    """The inputs and the zeroed outputs of a host search_csr, as the ABI takes them ->
    (q_terms, cu_q, n_q, docs, scores, n, keys)."""
    q_terms = np.ascontiguousarray(q_terms, np.uint32)
    if q_terms.size == 0:
        q_terms = np.zeros(1, np.uint32)
    cu_q = np.ascontiguousarray(cu_q, np.int32)
    n_q = len(cu_q) - 1
    docs = np.zeros((max(n_q, 1), k), np.uint32)
    scores = np.zeros((max(n_q, 1), k), score_dtype)
    n = np.zeros(max(n_q, 1), np.int32)
    keys = np.zeros((max(n_q, 1), k), np.uint64) if with_keys else None
    return q_terms, cu_q, n_q, docs, scores, n, keys


def _append_arrays(term_ids, impacts, cu_terms, timing):
    """The (term id, impact) pairs of an append, as the ABI takes them: host numpy arrays
    made contiguous and checked against cu_terms, torch device tensors as they are ->
    (term_ids, impacts, cu_terms, n_docs, flags)."""
    n_docs = len(cu_terms) - 1
    flags = DI_F_TIMING if timing else 0
    if _is_device(cu_terms):
        return term_ids, impacts, cu_terms, n_docs, flags | DI_F_DEVICE_PTRS
    term_ids = np.ascontiguousarray(term_ids, np.uint32)
    impacts = np.ascontiguousarray(impacts, np.float32)
    cu_terms = np.ascontiguousarray(cu_terms, np.int32)
    if term_ids.size != impacts.size or (n_docs > 0 and term_ids.size < cu_terms[-1]):
        raise ValueError("term_ids and impacts: one entry per pair of cu_terms")
    if term_ids.size == 0:
        term_ids, impacts = np.zeros(1, np.uint32), np.zeros(1, np.float32)
    return term_ids, impacts, cu_terms, n_docs, flags


class DeviceIndex(_TimedHandle):
    """Device-resident quantized index (one shard [doc_lo, doc_hi) of doc ids)."""

    _family = "di_index"

    def __init__(self, handle):
        self._h = handle

    @classmethod
    def from_postings(cls, term_off, pdoc, pval, doc_lo=0, doc_hi=0, device=0, layout="host",
                      stream=0, timing=False):
        """layout="host": di_index_create (the blocked layout built on host threads and
        uploaded); "device": di_index_create_device (built on the GPU, the same bytes), which
        also takes torch device tensors (IndexBuilder.postings(device=True)) as they are."""
        if layout not in ("host", "device"):
            raise ValueError(f"layout must be 'host' or 'device', not {layout!r}")
        h = ctypes.c_void_p()
        if _is_device(term_off):
            if layout != "device":
                raise ValueError("device tensors need layout='device'")
            flags = DI_F_DEVICE_PTRS | (DI_F_TIMING if timing else 0)
            check(lib().di_index_create_device(ptr(term_off), len(term_off) - 1, ptr(pdoc),
                                               ptr(pval), doc_lo, doc_hi, device,
                                               ctypes.c_void_p(stream or 0), flags,
                                               ctypes.byref(h)))
            return cls(h)
        term_off = np.ascontiguousarray(term_off, np.int64)
        pdoc = np.ascontiguousarray(pdoc, np.uint32)
        pval = np.ascontiguousarray(pval, np.uint8)
        if pdoc.size == 0:
            pdoc = np.zeros(1, np.uint32)
            pval = np.zeros(1, np.uint8)
        if layout == "device":
            check(lib().di_index_create_device(ptr(term_off), len(term_off) - 1, ptr(pdoc),
                                               ptr(pval), doc_lo, doc_hi, device,
                                               ctypes.c_void_p(stream or 0),
                                               DI_F_TIMING if timing else 0, ctypes.byref(h)))
        else:
            check(lib().di_index_create(ptr(term_off), len(term_off) - 1, ptr(pdoc), ptr(pval),
                                        doc_lo, doc_hi, device, ctypes.byref(h)))
        return cls(h)

    @classmethod
    def from_reference_dir(cls, path, doc_lo=0, doc_hi=0, device=0):
        h = ctypes.c_void_p()
        check(lib().di_index_load_reference(str(path).encode(), doc_lo, doc_hi, device,
                                            ctypes.byref(h)))
        return cls(h)

    def info(self):
        nt, npo, nd, nb = I64(), I64(), U32(), I32()
        check(lib().di_index_info(self._h, ctypes.byref(nt), ctypes.byref(npo),
                                  ctypes.byref(nd), ctypes.byref(nb)))
        return {"n_terms": nt.value, "n_postings": npo.value, "n_docs": nd.value,
                "n_blocks": nb.value}

    def layout(self):
        ne, nl, bd, hf = I64(), I64(), I32(), I32()
        check(lib().di_index_layout(self._h, ctypes.byref(ne), ctypes.byref(nl),
                                    ctypes.byref(bd), ctypes.byref(hf)))
        return {"n_ent": ne.value, "n_long": nl.value, "block_docs": bd.value,
                "has_flat": bool(hf.value)}

    def export(self):
        """di_index_export: the device layout on the host, a dict of numpy arrays (post,
        post_flat -- None without the flat array --, tb_start, eblk, epos, seg, lid, wmeta,
        emax, wmax), of an index from either layout route."""
        i, lay = self.info(), self.layout()
        np_, ne, nl = i["n_postings"], lay["n_ent"], lay["n_long"]
        a = {"post": np.zeros(np_, np.uint32),
             "post_flat": np.zeros(np_, np.uint32) if lay["has_flat"] else None,
             "tb_start": np.zeros(i["n_terms"] + 1, np.uint32),
             "eblk": np.zeros(ne, np.uint16), "epos": np.zeros(ne + 1, np.uint32),
             "seg": np.zeros(8 * ne, np.uint16), "lid": np.zeros(ne, np.uint32),
             "wmeta": np.zeros(128 * nl, np.uint16), "emax": np.zeros(ne, np.uint8),
             "wmax": np.zeros(16 * nl, np.uint8)}
        check(lib().di_index_export(self._h, *[ptr(a[k]) for k in (
            "post", "post_flat", "tb_start", "eblk", "epos", "seg", "lid", "wmeta", "emax",
            "wmax")]))
        return a

    def search_csr(self, q_terms, cu_q, k, with_keys=False, timing=False):
        q_terms, cu_q, n_q, docs, scores, n, keys = _query_arrays(q_terms, cu_q, k, np.uint32,
                                                                  with_keys)
        flags = DI_F_TIMING if timing else 0
        check(lib().di_index_search(self._h, ptr(q_terms), ptr(cu_q), n_q, k, ptr(docs),
                                    ptr(scores), ptr(n), ptr(keys), flags))
        return docs[:n_q], scores[:n_q], n[:n_q], (keys[:n_q] if with_keys else None)

    def search(self, queries, k=1000):
        """queries: list of term-id lists (iteration order = tie order)."""
        flat, cu = csr(queries)
        docs, scores, n, _ = self.search_csr(flat, cu, k)
        return [list(zip(docs[i, :n[i]].tolist(), scores[i, :n[i]].tolist()))
                for i in range(len(queries))]

    def search_device(self, q_terms, cu_q, n_q, k, out_doc, out_score, out_n, out_key=None,
                      flags=DI_F_DEVICE_PTRS):
        """All pointers are device pointers (torch tensors or ints)."""
        check(lib().di_index_search(self._h, ptr(q_terms), ptr(cu_q), n_q, k, ptr(out_doc),
                                    ptr(out_score), ptr(out_n), ptr(out_key), flags))

    def reserve(self, max_q, k):
        check(lib().di_index_reserve(self._h, max_q, k))

    def set_min_impact(self, min_impact=1):
        """Score only postings with value >= 2^floor(log2 min_impact) (1 = exact)."""
        check(lib().di_index_set_min_impact(self._h, int(min_impact)))

    def set_block_max(self, factor=0.0):
        """Block-max skipping: 0 off, 1 exact, > 1 approximate (di_index_set_block_max)."""
        check(lib().di_index_set_block_max(self._h, float(factor)))

    def set_packed(self, on=True):
        """Block-compressed postings (di_index_set_packed, configs[4]); returns the packed
        size in bytes."""
        b = I64(0)
        check(lib().di_index_set_packed(self._h, int(bool(on)), ctypes.byref(b)))
        return b.value

    def set_stream(self, stream_ptr):
        check(lib().di_index_set_stream(self._h, ctypes.c_void_p(stream_ptr)))

    def sync(self):
        check(lib().di_index_sync(self._h))


class TermStore(_TimedHandle):
    """Device-resident (term id, impact) lists per passage (di_term_store_*): the
    re-ranker's per-pid cache (reranker.py:39,48-53) on the GPU."""

    _family = "di_term_store"

    def __init__(self, device=0, n_docs=0, n_terms=0):
        h = ctypes.c_void_p()
        check(lib().di_term_store_create(device, ctypes.byref(h)))
        self._h = h
        self.device = device
        if n_docs or n_terms:
            self.reserve(n_docs, n_terms)

    def reserve(self, n_docs, n_terms):
        check(lib().di_term_store_reserve(self._h, int(n_docs), int(n_terms)))

    def append(self, term_ids, impacts, cu_terms, stream=0, timing=False):
        """Appends len(cu_terms) - 1 passages; passage d holds (term_ids[i], impacts[i]) for
        i in [cu_terms[d], cu_terms[d + 1]).  Host numpy arrays, or torch device tensors
        (all three; term ids as int32 bit patterns).  Returns the store index of the first
        appended passage."""
        term_ids, impacts, cu_terms, n_docs, flags = _append_arrays(term_ids, impacts, cu_terms,
                                                                    timing)
        first = I64(0)
        check(lib().di_term_store_append(self._h, ptr(term_ids), ptr(impacts), ptr(cu_terms),
                                         n_docs, ctypes.byref(first),
                                         ctypes.c_void_p(stream or 0), flags))
        return first.value

    def score(self, q_terms, cu_q, cand_doc, cu_cand, stream=0, timing=False):
        """di_term_store_score: for every candidate cand_doc[c] of every query, the float32
        sum of the impacts of the query's terms the passage holds, added in the query's
        order, and the number of terms that matched.  Host numpy arrays in -> (scores
        float32, match int32) numpy; torch device tensors in (all four) -> torch device
        tensors."""
        n_q = len(cu_q) - 1
        flags = DI_F_TIMING if timing else 0
        if _is_device(cand_doc):
            import torch

            n_c = int(cand_doc.numel())
            scores = torch.empty(max(1, n_c), dtype=torch.float32, device=cand_doc.device)
            match = torch.empty(max(1, n_c), dtype=torch.int32, device=cand_doc.device)
            flags |= DI_F_DEVICE_PTRS
        else:
            q_terms = np.ascontiguousarray(q_terms, np.uint32)
            cu_q = np.ascontiguousarray(cu_q, np.int32)
            cand_doc = np.ascontiguousarray(cand_doc, np.int32)
            cu_cand = np.ascontiguousarray(cu_cand, np.int32)
            n_c = cand_doc.size
            if n_q > 0 and (cu_cand[-1] > n_c or cu_q[-1] > q_terms.size):
                raise ValueError("cu_cand / cu_q name more entries than the arrays hold")
            if q_terms.size == 0:
                q_terms = np.zeros(1, np.uint32)
            if n_c == 0:
                cand_doc = np.zeros(1, np.int32)
            scores = np.zeros(max(1, n_c), np.float32)
            match = np.zeros(max(1, n_c), np.int32)
        check(lib().di_term_store_score(self._h, ptr(q_terms), ptr(cu_q), n_q, ptr(cand_doc),
                                        ptr(cu_cand), ptr(scores), ptr(match),
                                        ctypes.c_void_p(stream or 0), flags))
        return scores[:n_c], match[:n_c]

    def info(self):
        nd, nt, nb = I64(), I64(), I64()
        check(lib().di_term_store_info(self._h, ctypes.byref(nd), ctypes.byref(nt),
                                       ctypes.byref(nb)))
        return {"n_docs": nd.value, "n_terms": nt.value, "device_bytes": nb.value}


def topk_merge(keys, counts, k, device=0, stream=None, flags=0):
    """keys: [n_q, n_lists, k] uint64, counts: [n_q, n_lists] int32 (host numpy, or device
    tensors with DI_F_DEVICE_PTRS).  Returns (keys [n_q,k], n [n_q]) for host inputs."""
    if flags & DI_F_DEVICE_PTRS:
        raise ValueError("use topk_merge_device for device pointers")
    keys = np.ascontiguousarray(keys, np.uint64)
    counts = np.ascontiguousarray(counts, np.int32)
    n_q, n_lists = counts.shape
    assert keys.shape == (n_q, n_lists, k)
    out = np.zeros((max(n_q, 1), k), np.uint64)
    n = np.zeros(max(n_q, 1), np.int32)
    check(lib().di_topk_merge(ptr(keys), ptr(counts), n_q, n_lists, k, ptr(out), ptr(n),
                              device, ctypes.c_void_p(stream or 0), flags))
    return out[:n_q], n[:n_q]


def topk_merge_device(keys, counts, n_q, n_lists, k, out_key, out_n, device=0, stream=0,
                      flags=DI_F_DEVICE_PTRS):
    check(lib().di_topk_merge(ptr(keys), ptr(counts), n_q, n_lists, k, ptr(out_key),
                              ptr(out_n), device, ctypes.c_void_p(stream), flags))


def _is_device(a) -> bool:
    return hasattr(a, "data_ptr") and getattr(a, "is_cuda", False)


def pairs_pack(doc_tok, doc_off, qry_tok, qry_off, pair_doc, pair_qry, fmt, device=0,
               stream=0):
    """di_pairs_pack.  Host numpy arrays in -> (tok_ids, cu_seqlens) numpy out; torch
    device tensors in (all of them) -> torch device tensors out.  Also returns
    (n_tokens, max_len)."""
    n_docs, n_q, n_pairs = len(doc_off) - 1, len(qry_off) - 1, len(pair_doc)
    cap = max(1, n_pairs * fmt.max_length)
    nt, ml = I64(0), I32(0)
    if _is_device(pair_doc):
        import torch

        ids = torch.empty(cap, dtype=torch.int32, device=pair_doc.device)
        cu = torch.empty(n_pairs + 1, dtype=torch.int32, device=pair_doc.device)
        flags = DI_F_DEVICE_PTRS
    else:
        doc_tok = np.ascontiguousarray(doc_tok, np.int32)
        qry_tok = np.ascontiguousarray(qry_tok, np.int32)
        doc_off = np.ascontiguousarray(doc_off, np.int64)
        qry_off = np.ascontiguousarray(qry_off, np.int64)
        pair_doc = np.ascontiguousarray(pair_doc, np.int32)
        pair_qry = np.ascontiguousarray(pair_qry, np.int32)
        ids = np.zeros(cap, np.int32)
        cu = np.zeros(n_pairs + 1, np.int32)
        flags = 0
    check(lib().di_pairs_pack(ptr(doc_tok), ptr(doc_off), n_docs, ptr(qry_tok), ptr(qry_off),
                              n_q, ptr(pair_doc), ptr(pair_qry), n_pairs, ctypes.byref(fmt),
                              ptr(ids), cap, ptr(cu), ctypes.byref(nt), ctypes.byref(ml),
                              device, ctypes.c_void_p(stream or 0), flags))
    return ids[:nt.value], cu, nt.value, ml.value


def segment_order(scores, cu_seg, device=0, stream=0):
    """di_segment_order: per segment the positions in the order of Python's
    sorted(..., key=score, reverse=True).  numpy in -> numpy out, torch device tensors in
    -> a torch device tensor out."""
    n_seg = len(cu_seg) - 1
    if _is_device(scores):
        import torch

        out = torch.empty(max(1, scores.numel()), dtype=torch.int32, device=scores.device)
        check(lib().di_segment_order(ptr(scores), ptr(cu_seg), n_seg, ptr(out), device,
                                     ctypes.c_void_p(stream or 0), DI_F_DEVICE_PTRS))
        return out[:scores.numel()]
    scores = np.ascontiguousarray(scores, np.float32)
    cu_seg = np.ascontiguousarray(cu_seg, np.int32)
    out = np.zeros(max(1, scores.size), np.int32)
    check(lib().di_segment_order(ptr(scores if scores.size else np.zeros(1, np.float32)),
                                 ptr(cu_seg), n_seg, ptr(out), device,
                                 ctypes.c_void_p(stream or 0), 0))
    return out[:scores.size]


def _check_entries(rc, needed):
    """check() for the calls that report the entries needed with DI_ERANGE: the DIError
    carries them as .needed."""
    if rc == DI_ERANGE:
        e = DIError(rc, lib().di_last_error().decode("utf-8", "replace"))
        e.needed = needed
        raise e
    check(rc)


def pairwise_order(single, pair, cu_terms, cu_pairs, single_pos=None, round3=False, out_cap=None,
                   device=0, stream=0):
    """di_pairwise_order: the entries of DeepPairwiseImpact.compute_term_impacts
    (pairwise_impact.py:98-129) in their order.  single / pair: di_encode_pairwise's
    arrays (terms sorted by token index, pairs in combination order); single_pos: the
    position in the document's map of every sorted term (None: the identity).
    numpy in -> (cu_out int64 [n_docs + 1], first int32, second int32 (-1: a single term),
    score float32); torch device tensors in (all of them) -> torch device tensors out.
    first / second index the sorted terms globally.  out_cap: capacity of the entry
    arrays (default: every pair kept); too small raises DIError DI_ERANGE."""
    n_docs = len(cu_terms) - 1
    n = I64(0)
    flags = DI_F_ROUND3 if round3 else 0
    if _is_device(single) or _is_device(cu_terms):
        import torch

        n_terms, n_pairs = int(single.numel()), int(pair.numel())
        cap = n_terms + n_pairs if out_cap is None else int(out_cap)
        dev = cu_terms.device
        cu_out = torch.empty(n_docs + 1, dtype=torch.int64, device=dev)
        first = torch.empty(max(1, cap), dtype=torch.int32, device=dev)
        second = torch.empty(max(1, cap), dtype=torch.int32, device=dev)
        score = torch.empty(max(1, cap), dtype=torch.float32, device=dev)
        flags |= DI_F_DEVICE_PTRS
    else:
        single = np.ascontiguousarray(single, np.float32)
        pair = np.ascontiguousarray(pair, np.float32)
        cu_terms = np.ascontiguousarray(cu_terms, np.int32)
        cu_pairs = np.ascontiguousarray(cu_pairs, np.int64)
        if single_pos is not None:
            single_pos = np.ascontiguousarray(single_pos, np.int32)
        n_terms, n_pairs = single.size, pair.size
        cap = n_terms + n_pairs if out_cap is None else int(out_cap)
        if single.size == 0:
            single = np.zeros(1, np.float32)
        if pair.size == 0:
            pair = np.zeros(1, np.float32)
        cu_out = np.zeros(n_docs + 1, np.int64)
        first = np.zeros(max(1, cap), np.int32)
        second = np.zeros(max(1, cap), np.int32)
        score = np.zeros(max(1, cap), np.float32)
    rc = lib().di_pairwise_order(ptr(single), ptr(pair), ptr(cu_terms), ptr(cu_pairs),
                                 ptr(single_pos), n_docs, n_terms, n_pairs, ptr(cu_out),
                                 ptr(first), ptr(second), ptr(score), cap, ctypes.byref(n),
                                 device, ctypes.c_void_p(stream or 0), flags)
    _check_entries(rc, n.value)
    return cu_out, first[:n.value], second[:n.value], score[:n.value]


def key_doc(keys, wide=False):
    """Doc of quantized-index merge keys (di_key_doc / di_key_doc_wide); wide: the
    keys of a query of more than DI_SHORT_QUERY_TERMS known terms."""
    if wide:
        return (np.uint64(0xFFFFFF) - (keys & np.uint64(0xFFFFFF))).astype(np.uint32)
    return (np.uint64(0xFFFFFFFF) - (keys & np.uint64(0xFFFFFFFF))).astype(np.uint32)


def key_score(keys, wide=False):
    return (keys >> np.uint64(44 if wide else 48)).astype(np.uint32)


def is_wide(n_terms: int) -> bool:
    """Does a query of n_terms known terms get wide merge keys?"""
    return n_terms > DI_SHORT_QUERY_TERMS


def append_run_lines(path, qids, docs, scores, counts) -> None:
    """Native RunFile.writelines over a batch (di_append_run_lines): qids (str list),
    docs / scores uint32 [n_q, k], counts [n_q] -> those queries' lines appended to path."""
    n_q = len(qids)
    if n_q == 0:
        open(path, "ab").close()
        return
    enc = [str(q).encode("utf-8") for q in qids]
    blob = b"".join(enc) + b"\0"
    off = np.zeros(n_q + 1, np.int64)
    off[1:] = np.cumsum([len(b) for b in enc])
    docs = np.ascontiguousarray(docs, np.uint32).reshape(n_q, -1)
    scores = np.ascontiguousarray(scores, np.uint32).reshape(docs.shape)
    cnt = np.ascontiguousarray(counts, np.int32)
    check(lib().di_append_run_lines(str(path).encode("utf-8"), blob, ptr(off), n_q, ptr(docs),
                                    ptr(scores), ptr(cnt), docs.shape[1]))


def format_impact_lines_packed(blob: bytes, term_off, impacts, cu_terms) -> str:
    """format_impact_lines on the packed form: the terms' UTF-8 bytes back to back
    (term_off [T+1] int64 byte offsets), their float32 impacts and the per-document
    term offsets cu_terms [n_docs+1]."""
    n_docs = len(cu_terms) - 1
    term_off = np.ascontiguousarray(term_off, np.int64)
    imp = np.ascontiguousarray(impacts, np.float32)
    if imp.size == 0:
        imp = np.zeros(1, np.float32)
    cu = np.ascontiguousarray(cu_terms, np.int64)
    n_terms = len(term_off) - 1
    cap = len(blob) + 30 * (n_terms + 1) + n_docs + 16
    out = ctypes.create_string_buffer(cap)
    n = ctypes.c_int64(0)
    tb = ctypes.create_string_buffer(blob, len(blob) + 1)
    check(lib().di_format_impact_lines(tb, ptr(term_off), ptr(imp), ptr(cu), n_docs, out, cap,
                                       ctypes.byref(n)))
    return out.raw[:n.value].decode("utf-8")


def format_entry_lines(blob: bytes, term_off, first, second, score, cu_out, out_cap=None) -> str:
    """di_format_entry_lines: the impact-TSV lines of di_pairwise_order's entries.  blob /
    term_off: the batch's terms as in format_impact_lines_packed; entry e is term first[e],
    or 'term first[e]|term second[e]' when second[e] >= 0, with score[e]; document d holds
    the entries cu_out[d] .. cu_out[d + 1]."""
    n_docs = len(cu_out) - 1
    term_off = np.ascontiguousarray(term_off, np.int64)
    cu = np.ascontiguousarray(cu_out, np.int64)
    first = np.ascontiguousarray(first, np.int32)
    second = np.ascontiguousarray(second, np.int32)
    score = np.ascontiguousarray(score, np.float32)
    n_terms, n_ent = len(term_off) - 1, int(cu[-1])
    if first.size < n_ent or second.size < n_ent or score.size < n_ent:
        raise ValueError("cu_out names more entries than the arrays hold")
    if n_ent == 0:
        first, second, score = np.zeros(1, np.int32), np.zeros(1, np.int32), np.zeros(1, np.float32)
    if out_cap is None:
        # an entry: at most its two terms, '|', ': ', a float32's repr (<= 24) and ', '
        # (indices clipped for the estimate only: the library rejects a bad one)
        lens = np.diff(term_off) if n_terms else np.zeros(1, np.int64)
        f, s = first[:n_ent].clip(0, max(n_terms - 1, 0)), second[:n_ent]
        names = int(lens[f].sum()) + int((lens[s.clip(0, max(n_terms - 1, 0))] + 1)[s >= 0].sum())
        out_cap = names + 28 * n_ent + n_docs + 16
    out = ctypes.create_string_buffer(max(1, int(out_cap)))
    n = ctypes.c_int64(0)
    tb = ctypes.create_string_buffer(blob, len(blob) + 1)
    check(lib().di_format_entry_lines(tb, ptr(term_off), n_terms, ptr(first), ptr(second),
                                      ptr(score), ptr(cu), n_docs, out, int(out_cap),
                                      ctypes.byref(n)))
    return out.raw[:n.value].decode("utf-8")


def format_impact_lines(doc_terms, doc_impacts):
    """Native A9 formatter: list (per doc) of term lists + float32 impact arrays
    (already rounded) -> the impact-TSV text of those docs (one line each)."""
    n_docs = len(doc_terms)
    enc = [t.encode("utf-8") for terms in doc_terms for t in terms]
    blob = b"".join(enc)
    term_off = np.zeros(len(enc) + 1, np.int64)
    if enc:
        term_off[1:] = np.cumsum([len(b) for b in enc])
    cu = np.zeros(n_docs + 1, np.int64)
    cu[1:] = np.cumsum([len(t) for t in doc_terms])
    imp = np.ascontiguousarray(np.concatenate([np.asarray(x, np.float32) for x in doc_impacts])
                               if n_docs else np.zeros(0, np.float32), np.float32)
    if imp.size == 0:
        imp = np.zeros(1, np.float32)
    cap = len(blob) + 30 * (len(enc) + 1) + n_docs + 16
    out = ctypes.create_string_buffer(cap)
    n = ctypes.c_int64(0)
    tb = ctypes.create_string_buffer(blob, len(blob) + 1)
    check(lib().di_format_impact_lines(tb, ptr(term_off), ptr(imp), ptr(cu), n_docs, out, cap,
                                       ctypes.byref(n)))
    return out.raw[:n.value].decode("utf-8")


class DeviceSparseIndex(_TimedHandle):
    """Device-resident float index (di_sparse_*), NanoBEIR's SparseSearch path."""

    _family = "di_sparse"

    def __init__(self, term_off, pdoc, pimp, n_docs, device=0):
        term_off = np.ascontiguousarray(term_off, np.int64)
        pdoc = np.ascontiguousarray(pdoc, np.uint32)
        pimp = np.ascontiguousarray(pimp, np.float32)
        if pdoc.size == 0:
            pdoc, pimp = np.zeros(1, np.uint32), np.zeros(1, np.float32)
        h = ctypes.c_void_p()
        check(lib().di_sparse_create(ptr(term_off), len(term_off) - 1, ptr(pdoc), ptr(pimp),
                                     n_docs, device, ctypes.byref(h)))
        self._h = h

    @classmethod
    def _from_handle(cls, h):
        self = cls.__new__(cls)
        self._h = h
        return self

    def info(self):
        nt, npost, nd, nb = I64(), I64(), U32(), I32()
        check(lib().di_sparse_info(self._h, ctypes.byref(nt), ctypes.byref(npost),
                                   ctypes.byref(nd), ctypes.byref(nb)))
        return {"n_terms": nt.value, "n_postings": npost.value, "n_docs": nd.value,
                "n_blocks": nb.value}

    def export(self):
        """di_sparse_export: the device layout on the host, (term_start int64 [n_terms],
        blk_off uint32 [n_terms, n_blocks + 1], pdoc uint16 [n_postings] (doc % 16384),
        pimp float32 [n_postings]).  Term t's postings of block b are
        [term_start[t] + blk_off[t, b], term_start[t] + blk_off[t, b + 1]), docs ascending;
        blk_off[t, n_blocks] is its posting count."""
        i = self.info()
        term_start = np.zeros(i["n_terms"], np.int64)
        blk_off = np.zeros((i["n_terms"], i["n_blocks"] + 1), np.uint32)
        pdoc = np.zeros(i["n_postings"], np.uint16)
        pimp = np.zeros(i["n_postings"], np.float32)
        check(lib().di_sparse_export(self._h, ptr(term_start), ptr(blk_off), ptr(pdoc),
                                     ptr(pimp)))
        return term_start, blk_off, pdoc, pimp

    def search_csr(self, q_terms, cu_q, k, with_keys=False, accumulation="f32"):
        """accumulation "f32" (numpy >= 2) or "f64" (the reference's pinned numpy 1.25:
        f64 scores; no keys)."""
        if accumulation not in ("f32", "f64"):
            raise ValueError(f"accumulation must be 'f32' or 'f64', not {accumulation!r}")
        if accumulation == "f64" and with_keys:
            raise ValueError("f64 search has no 64-bit merge keys")
        q_terms, cu_q, n_q, docs, scores, n, keys = _query_arrays(
            q_terms, cu_q, k, np.float64 if accumulation == "f64" else np.float32, with_keys)
        if accumulation == "f64":
            check(lib().di_sparse_search_f64(self._h, ptr(q_terms), ptr(cu_q), n_q, k, ptr(docs),
                                             ptr(scores), ptr(n), 0))
            return docs[:n_q], scores[:n_q], n[:n_q], None
        check(lib().di_sparse_search(self._h, ptr(q_terms), ptr(cu_q), n_q, k, ptr(docs),
                                     ptr(scores), ptr(n), ptr(keys), 0))
        return docs[:n_q], scores[:n_q], n[:n_q], (keys[:n_q] if with_keys else None)

    def search(self, queries, k, accumulation="f32"):
        flat, cu = csr(queries)
        docs, scores, n, _ = self.search_csr(flat, cu, k, accumulation=accumulation)
        return [list(zip(docs[i, :n[i]].tolist(), scores[i, :n[i]].tolist()))
                for i in range(len(queries))]


class SparseBuilder(_Handle):
    """Device builder of the float index (di_sparse_builder_*): documents appended as
    (term id, impact) pairs -- host arrays, or the device buffers of an encode step --
    and assembled into a DeviceSparseIndex on the GPU."""

    _family = "di_sparse_builder"

    def __init__(self, device=0, n_docs=0, n_pairs=0):
        h = ctypes.c_void_p()
        check(lib().di_sparse_builder_create(device, ctypes.byref(h)))
        self._h = h
        self.device = device
        if n_docs or n_pairs:
            self.reserve(n_docs, n_pairs)

    def reserve(self, n_docs, n_pairs):
        check(lib().di_sparse_builder_reserve(self._h, int(n_docs), int(n_pairs)))

    def append(self, term_ids, impacts, cu_terms, stream=0, timing=False):
        """Appends len(cu_terms) - 1 documents; document d holds (term_ids[i], impacts[i])
        for i in [cu_terms[d], cu_terms[d + 1]); pairs whose impact is not > 0 are dropped.
        Host numpy arrays, or torch device tensors (all three; term ids as int32 bit
        patterns).  Returns the corpus position of the first appended document."""
        term_ids, impacts, cu_terms, n_docs, flags = _append_arrays(term_ids, impacts, cu_terms,
                                                                    timing)
        first = I64(0)
        check(lib().di_sparse_builder_append(self._h, ptr(term_ids), ptr(impacts),
                                             ptr(cu_terms), n_docs, ctypes.byref(first),
                                             ctypes.c_void_p(stream or 0), flags))
        return first.value

    def info(self):
        nd, npairs = I64(), I64()
        check(lib().di_sparse_builder_info(self._h, ctypes.byref(nd), ctypes.byref(npairs)))
        return {"n_docs": nd.value, "n_pairs": npairs.value}

    def finish(self, n_terms, stream=0, timing=False) -> DeviceSparseIndex:
        """The index of everything appended over terms 0 .. n_terms - 1 (the builder stays
        as it is).  A term id >= n_terms, or a term twice in one document: DI_EINVAL."""
        h = ctypes.c_void_p()
        check(lib().di_sparse_builder_finish(self._h, int(n_terms), ctypes.c_void_p(stream or 0),
                                             DI_F_TIMING if timing else 0, ctypes.byref(h)))
        return DeviceSparseIndex._from_handle(h)


class TermTable(_Handle):
    """Term strings numbered in order of first appearance (di_term_table_*): the host side
    of IndexBuilder.  Terms go in as the tokenizer workers' packed form -- one UTF-8 blob
    and byte offsets -- so no Python str is made per term."""

    _family = "di_term_table"

    def __init__(self):
        h = ctypes.c_void_p()
        check(lib().di_term_table_create(ctypes.byref(h)))
        self._h = h

    def intern(self, blob: bytes, term_off) -> np.ndarray:
        """uint32 ids of the terms blob[term_off[i]:term_off[i + 1]]; a term the impact TSV
        would not parse back to (empty, whitespace at an end, ', ' or ': ' inside) raises
        DIError DI_EFORMAT and leaves the table as it was."""
        term_off = np.ascontiguousarray(term_off, np.int64)
        n = len(term_off) - 1
        ids = np.zeros(max(n, 1), np.uint32)
        if n > 0 and int(term_off[-1]) > len(blob):
            raise ValueError("term_off names more bytes than the blob holds")
        check(lib().di_term_table_intern(self._h, blob, ptr(term_off), n, ptr(ids)))
        return ids[:max(n, 0)]

    def intern_terms(self, terms) -> np.ndarray:
        enc = [t.encode("utf-8") for t in terms]
        off = np.zeros(len(enc) + 1, np.int64)
        if enc:
            off[1:] = np.cumsum([len(b) for b in enc])
        return self.intern(b"".join(enc), off)

    def __len__(self):
        n = I64(0)
        check(lib().di_term_table_info(self._h, ctypes.byref(n), None))
        return n.value

    def export(self):
        """(blob, term_off int64 [n_terms + 1]): every term in id order."""
        n, nb = I64(0), I64(0)
        check(lib().di_term_table_info(self._h, ctypes.byref(n), ctypes.byref(nb)))
        blob = ctypes.create_string_buffer(max(1, nb.value))
        off = np.zeros(n.value + 1, np.int64)
        check(lib().di_term_table_export(self._h, blob, ptr(off)))
        return blob.raw[:nb.value], off

    def rows(self, term_count):
        """(term_row int32 [n_terms], n_rows): the terms with term_count > 0 numbered in
        sorted() order of their strings -- the lines of vocab.txt -- every other term -1."""
        term_count = np.ascontiguousarray(term_count, np.int64)
        if term_count.size != len(self):
            raise ValueError("term_count: one entry per term of the table")
        row = np.full(max(term_count.size, 1), -1, np.int32)
        n = I64(0)
        check(lib().di_term_table_rows(self._h, ptr(term_count if term_count.size else
                                                    np.zeros(1, np.int64)), ptr(row),
                                       ctypes.byref(n)))
        return row[:term_count.size], n.value

    def rows_pairwise(self, term_count, first_id, second_id):
        """rows() over the single terms and the pair terms of IndexBuilder.pair_terms ->
        (term_row int32 [n_terms + n_pair_terms], n_rows): pair u, named term[first_id[u]] +
        '|' + term[second_id[u]], is entry n_terms + u.  Two entries with one name: DIError
        DI_EFORMAT naming it (the text route merges them: build that collection there)."""
        term_count = np.ascontiguousarray(term_count, np.int64)
        first_id = np.ascontiguousarray(first_id, np.uint32)
        second_id = np.ascontiguousarray(second_id, np.uint32)
        if term_count.size != len(self) or first_id.size != second_id.size:
            raise ValueError("term_count: one entry per term of the table; one id pair per pair term")
        n_pt = first_id.size
        row = np.full(max(term_count.size + n_pt, 1), -1, np.int32)
        n = I64(0)
        one = np.zeros(1, np.uint32)
        check(lib().di_term_table_rows_pairwise(
            self._h, ptr(term_count if term_count.size else np.zeros(1, np.int64)), n_pt,
            ptr(first_id if n_pt else one), ptr(second_id if n_pt else one), ptr(row),
            ctypes.byref(n)))
        return row[:term_count.size + n_pt], n.value

    def vocab(self, term_row, first_id=None, second_id=None) -> dict:
        """{term: row} of the terms that have a row (InvertedIndex.vocab); with the pair
        terms' ids, term_row holds their rows after the single terms' and the pairs are
        named 'a|b'."""
        blob, off = self.export()
        ol = off.tolist()
        names = [blob[ol[i]:ol[i + 1]].decode("utf-8") for i in range(len(ol) - 1)]
        rows = np.asarray(term_row).tolist()
        v = {names[i]: r for i, r in enumerate(rows[:len(names)]) if r >= 0}
        if first_id is not None:
            for a, b, r in zip(np.asarray(first_id).tolist(), np.asarray(second_id).tolist(),
                               rows[len(names):]):
                if r >= 0:
                    v[names[a] + "|" + names[b]] = r
        return v


class IndexBuilder(_TimedHandle):
    """Device builder of the quantized inverted index (di_index_builder_*): documents
    appended as (term id, round3 impact) pairs -- host arrays, or the device buffers of an
    encode step -- quantized, and returned as the postings di_index_create takes, in the
    order of the reference's files."""

    _family = "di_index_builder"

    def __init__(self, device=0, n_docs=0, n_pairs=0):
        h = ctypes.c_void_p()
        check(lib().di_index_builder_create(device, ctypes.byref(h)))
        self._h = h
        self.device = device
        self.n_kept, self.term_count = None, None  # of the last quantize
        if n_docs or n_pairs:
            self.reserve(n_docs, n_pairs)

    def reserve(self, n_docs, n_pairs):
        check(lib().di_index_builder_reserve(self._h, int(n_docs), int(n_pairs)))

    def append(self, term_ids, impacts, cu_terms, stream=0, timing=False):
        """Appends len(cu_terms) - 1 documents; document d holds (term_ids[i], impacts[i])
        for i in [cu_terms[d], cu_terms[d + 1]), every pair kept.  Host numpy arrays, or
        torch device tensors (all three; term ids as int32 bit patterns).  Returns the doc
        id of the first appended document."""
        term_ids, impacts, cu_terms, n_docs, flags = _append_arrays(term_ids, impacts, cu_terms,
                                                                    timing)
        first = I64(0)
        check(lib().di_index_builder_append(self._h, ptr(term_ids), ptr(impacts), ptr(cu_terms),
                                            n_docs, ctypes.byref(first),
                                            ctypes.c_void_p(stream or 0), flags))
        if n_docs > 0:
            self.n_kept, self.term_count = None, None
        return first.value

    def append_pairwise(self, term_ids, single, pair, cu_terms, cu_pairs, stream=0, timing=False):
        """Appends len(cu_terms) - 1 documents of the pairwise model from encode_pairwise's
        unrounded outputs (round3 is applied here): the singles as append() takes them, the
        terms in token order; pair / cu_pairs (int64) the scores of every document's
        T(T-1)/2 combinations, kept iff they do not round to zero, each the posting of the
        term 'a|b'.  Host numpy arrays, or torch device tensors (all five).  Returns the doc
        id of the first appended document."""
        n_docs = len(cu_terms) - 1
        if len(cu_pairs) != n_docs + 1:
            raise ValueError("cu_terms and cu_pairs: one entry per document + 1")
        if _is_device(cu_terms):
            if not all(_is_device(x) for x in (term_ids, single, pair, cu_pairs)):
                raise ValueError("append_pairwise: all five arrays on the device, or none")
            if cu_pairs.element_size() != 8 or cu_terms.element_size() != 4:
                raise ValueError("cu_terms is int32 and cu_pairs int64")
            n_pairs = int(cu_pairs[-1]) if n_docs > 0 else 0
            flags = (DI_F_TIMING if timing else 0) | DI_F_DEVICE_PTRS
        else:
            term_ids, single, cu_terms, n_docs, flags = _append_arrays(term_ids, single,
                                                                      cu_terms, timing)
            pair = np.ascontiguousarray(pair, np.float32)
            cu_pairs = np.ascontiguousarray(cu_pairs, np.int64)
            n_pairs = int(cu_pairs[-1]) if n_docs > 0 else 0
            if pair.size < n_pairs:
                raise ValueError("pair: one entry per pair of cu_pairs")
            if pair.size == 0:
                pair = np.zeros(1, np.float32)
        first = I64(0)
        check(lib().di_index_builder_append_pairwise(
            self._h, ptr(term_ids), ptr(single), ptr(pair), ptr(cu_terms), ptr(cu_pairs), n_docs,
            n_pairs, ctypes.byref(first), ctypes.c_void_p(stream or 0), flags))
        if n_docs > 0:
            self.n_kept, self.term_count = None, None
        return first.value

    def pair_terms(self):
        """The distinct pair keys that kept a posting in the last quantize, in ascending
        (first id, second id) order -> (first_id uint32, second_id uint32, count int64)."""
        n = I64(0)
        check(lib().di_index_builder_pair_terms(self._h, ctypes.byref(n), None, None, None))
        first = np.zeros(max(n.value, 1), np.uint32)
        second = np.zeros(max(n.value, 1), np.uint32)
        count = np.zeros(max(n.value, 1), np.int64)
        check(lib().di_index_builder_pair_terms(self._h, ctypes.byref(n), ptr(first), ptr(second),
                                                ptr(count)))
        return first[:n.value], second[:n.value], count[:n.value]

    def info(self):
        nd, npairs = I64(), I64()
        check(lib().di_index_builder_info(self._h, ctypes.byref(nd), ctypes.byref(npairs)))
        return {"n_docs": nd.value, "n_pairs": npairs.value}

    def quantize(self, n_terms, max_val=None, stream=0, timing=False):
        """quantize.py:13-47 on everything appended -> (max_used, term_count int64
        [n_terms], n_kept).  max_val None: the maximum over all pairs."""
        tc = np.zeros(max(int(n_terms), 1), np.int64)
        used, kept = ctypes.c_double(0.0), I64(0)
        check(lib().di_index_builder_quantize(
            self._h, int(n_terms), float(max_val) if max_val is not None else -1.0,
            ctypes.c_void_p(stream or 0), DI_F_TIMING if timing else 0, ctypes.byref(used),
            ptr(tc), ctypes.byref(kept)))
        self.n_kept, self.term_count = kept.value, tc[:int(n_terms)]
        return used.value, self.term_count, kept.value

    def postings(self, term_row, n_rows, stream=0, timing=False, device=False):
        """The kept postings in the reference file order -> (term_off int64 [n_rows + 1],
        pdoc uint32 [n_kept], pval uint8 [n_kept]): numpy arrays, or torch tensors on the
        builder's device (device=True)."""
        term_row = np.ascontiguousarray(term_row, np.int32)
        if self.n_kept is None:
            raise ValueError("IndexBuilder.quantize comes first")
        n = self.n_kept
        flags = DI_F_TIMING if timing else 0
        if device:
            import torch

            dev = torch.device("cuda", self.device)
            term_off = torch.empty(n_rows + 1, dtype=torch.int64, device=dev)
            pdoc = torch.empty(max(n, 1), dtype=torch.int32, device=dev)
            pval = torch.empty(max(n, 1), dtype=torch.uint8, device=dev)
            flags |= DI_F_DEVICE_PTRS
        else:
            term_off = np.zeros(n_rows + 1, np.int64)
            pdoc = np.zeros(max(n, 1), np.uint32)
            pval = np.zeros(max(n, 1), np.uint8)
        check(lib().di_index_builder_postings(
            self._h, ptr(term_row if term_row.size else np.zeros(1, np.int32)), int(n_rows),
            ctypes.c_void_p(stream or 0), flags, ptr(term_off), ptr(pdoc), ptr(pval)))
        return term_off, pdoc[:n], pval[:n]


def write_reference_index(out_dir, table: TermTable, term_row, n_rows, term_off, pdoc, pval):
    """di_write_reference_index: vocab.txt / inverted_index.idx / inverted_index.dat of
    IndexBuilder.postings' host arrays, the bytes create_index writes."""
    Path(out_dir).mkdir(parents=True, exist_ok=True)
    term_row = np.ascontiguousarray(term_row, np.int32)
    term_off = np.ascontiguousarray(term_off, np.int64)
    pdoc = np.ascontiguousarray(pdoc, np.uint32)
    pval = np.ascontiguousarray(pval, np.uint8)
    one = np.zeros(1, np.int32)
    check(lib().di_write_reference_index(str(out_dir).encode("utf-8"), table._h,
                                         ptr(term_row if term_row.size else one), int(n_rows),
                                         ptr(term_off), ptr(pdoc if pdoc.size else one),
                                         ptr(pval if pval.size else one)))


def write_reference_index_pairwise(out_dir, table: TermTable, first_id, second_id, term_row,
                                   n_rows, term_off, pdoc, pval):
    """di_write_reference_index_pairwise: write_reference_index with the pair terms of
    IndexBuilder.pair_terms, term_row as TermTable.rows_pairwise numbers them."""
    Path(out_dir).mkdir(parents=True, exist_ok=True)
    first_id = np.ascontiguousarray(first_id, np.uint32)
    second_id = np.ascontiguousarray(second_id, np.uint32)
    term_row = np.ascontiguousarray(term_row, np.int32)
    term_off = np.ascontiguousarray(term_off, np.int64)
    pdoc = np.ascontiguousarray(pdoc, np.uint32)
    pval = np.ascontiguousarray(pval, np.uint8)
    one = np.zeros(1, np.int32)
    check(lib().di_write_reference_index_pairwise(
        str(out_dir).encode("utf-8"), table._h, first_id.size,
        ptr(first_id if first_id.size else one), ptr(second_id if second_id.size else one),
        ptr(term_row if term_row.size else one), int(n_rows), ptr(term_off),
        ptr(pdoc if pdoc.size else one), ptr(pval if pval.size else one)))
