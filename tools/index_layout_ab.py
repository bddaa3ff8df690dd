"""The scorer's blocked device layout, host route against device route, on di_synth_postings
collections (the bench's shards: seed 4321, V = 2 N):

  host         di_index_create: build_index() on host threads, ten arrays uploaded
  device_h2d   di_index_create_device from host arrays (staging included)
  device       di_index_create_device from device-resident arrays (DI_F_DEVICE_PTRS)

The three routes alternate in one process over the same arrays, each warmed once at the
first size; a run is the wall time of the create call, which ends synchronised (the index is
destroyed outside the timed window).  Reports per size and route the runs, their median,
fastest and spread, the device route's il_* regions (HIP events, a run of their own with
DI_F_TIMING), host_cpus (the threads build_index() uses), whether the exports are byte-equal
(sizes up to --check_docs), and the verdict of DESIGN.md §3's rule: the device route counts
as faster only if its median is below the host route's fastest run.
    python tools/index_layout_ab.py [--docs 100000,1100000] [--skewed_docs 0] [--runs 3]
                                    [--out profiles/index_layout_ab.json]
"""
import argparse
import json
import os
import statistics
import sys
import time
from pathlib import Path

import numpy as np
import torch

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT))
from improving_learned_index_amd import synthetic as S  # noqa: E402
from improving_learned_index_amd._lib import DeviceIndex  # noqa: E402

REGIONS = ("il_check", "il_input", "il_count", "il_scan", "il_compact", "il_hist", "il_scatter",
           "il_heads", "il_entries", "il_long", "il_segment", "il_deal")
ARRAYS = ("post", "post_flat", "tb_start", "eblk", "epos", "seg", "lid", "wmeta", "emax", "wmax")
ROUTES = ("host", "device_h2d", "device")


def host_cpus():
    """di::host_threads()"""
    e = os.environ.get("DI_HOST_THREADS") or os.environ.get("OMP_NUM_THREADS")
    t = int(e) if e else (os.cpu_count() or 1)
    return max(1, min(t, 64))


def measure(n_docs, skew, runs, check, warm):
    v_terms = 2 * n_docs  # (bench.v_terms)
    term_off, pdoc, pval, _ = S.synth_postings(n_docs, v_terms, seed=4321, skew=skew)
    dev = torch.device("cuda", 0)
    d_off = torch.from_numpy(term_off).to(dev)
    d_doc = torch.from_numpy(pdoc.view(np.int32)).to(dev)
    d_val = torch.from_numpy(pval).to(dev)
    torch.cuda.synchronize()

    def create(route, timing=False):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        if route == "host":
            ix = DeviceIndex.from_postings(term_off, pdoc, pval, 0, n_docs)
        elif route == "device_h2d":
            ix = DeviceIndex.from_postings(term_off, pdoc, pval, 0, n_docs, layout="device",
                                           timing=timing)
        else:
            ix = DeviceIndex.from_postings(d_off, d_doc, d_val, 0, n_docs, layout="device",
                                           timing=timing)
        return time.perf_counter() - t0, ix

    if warm:
        for r in ROUTES:
            create(r)[1].close()
    times = {r: [] for r in ROUTES}
    for _ in range(runs):
        for r in ROUTES:
            dt, ix = create(r)
            times[r].append(dt)
            ix.close()
    _, ix = create("device", timing=True)
    regions = {r: round(ix.timing(r)[0], 3) for r in REGIONS}
    info, lay = ix.info(), ix.layout()
    equal = None
    if check:
        want = create("host")[1].export()
        equal = all((want[k] is None and g[k] is None) or want[k].tobytes() == g[k].tobytes()
                    for g in (ix.export(), create("device_h2d")[1].export()) for k in ARRAYS)
    ix.close()

    def summary(t):
        med = statistics.median(t)
        return {"run_s": [round(x, 4) for x in t], "median_s": med, "fastest_s": min(t),
                "spread": (max(t) - min(t)) / med}
    out = {"docs": n_docs, "v_terms": v_terms, "skewed": skew is not None, "postings": info["n_postings"],
           "blocks": info["n_blocks"], "entries": lay["n_ent"], "long_sublists": lay["n_long"],
           **{r: summary(times[r]) for r in ROUTES}, "il_regions_ms": regions,
           "exports_equal": equal}
    out["device_is_faster"] = out["device"]["median_s"] < out["host"]["fastest_s"]
    out["device_h2d_is_faster"] = out["device_h2d"]["median_s"] < out["host"]["fastest_s"]
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--docs", default="100000,1100000", help="i.i.d. collections of these sizes")
    ap.add_argument("--skewed_docs", type=int, default=0,
                    help="also the skewed collection (SKEW_CONFIG4) of this many docs")
    ap.add_argument("--runs", type=int, default=3)
    ap.add_argument("--check_docs", type=int, default=100000,
                    help="compare the exports of the routes up to this size")
    ap.add_argument("--out", default=None, help="also write the JSON result here")
    a = ap.parse_args()
    torch.cuda.init()
    sizes = [(int(x), None) for x in a.docs.split(",") if x]
    if a.skewed_docs:
        sizes.append((a.skewed_docs, S.SKEW_CONFIG4))
    rows = []
    for i, (n, skew) in enumerate(sizes):
        rows.append(measure(n, skew, a.runs, n <= a.check_docs, warm=i == 0))
        print(json.dumps(rows[-1]), file=sys.stderr, flush=True)
    out = {"tool": "index_layout_ab", "runs": a.runs, "host_cpus": host_cpus(), "sizes": rows}
    line = json.dumps(out)
    print(line)
    if a.out:
        Path(a.out).parent.mkdir(parents=True, exist_ok=True)
        Path(a.out).write_text(line + "\n")


if __name__ == "__main__":
    main()
