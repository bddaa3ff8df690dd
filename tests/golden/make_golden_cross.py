"""Golden vectors for the cross-encoder reranker's TopKDataset loader: writes the seeded
fixture tests/golden/topk_fixture.tsv (qid \t pid \t query \t passage) and runs the
reference's own TopKDataset (src/utils/datasets.py:181-222) on it, in this container where
/root/reference is mounted, to produce tests/golden/topk_dataset.json.  Re-run:
    python tests/golden/make_golden_cross.py
"""
import json
import random
import sys
import tempfile
from pathlib import Path

HERE = Path(__file__).resolve().parent
REF = Path("/root/reference")
sys.dont_write_bytecode = True
sys.path.insert(0, str(REF))
sys.path.insert(0, str(HERE))

import local_tokenizer  # noqa: E402


def write_fixture(path):
    rng = random.Random(11)
    words = local_tokenizer.WORDS
    # string ids (the reference keeps them as str), queries out of numeric order, a passage
    # shared by two queries, a query with one candidate, 21 lines
    queries = {"7": "what is a sparse index", "q2": "neural ranking model", "10": "water",
               "3": "how do people search the world"}
    cands = {"7": ["p1", "12", "5", "p9", "40", "41"], "q2": ["5", "13", "p1", "14", "15", "16",
                                                              "17"],
             "10": ["18"], "3": ["19", "20", "12", "21", "22", "23", "24"]}
    passages = {}
    lines = []
    for qid, pids in cands.items():
        for pid in pids:
            if pid not in passages:
                passages[pid] = " ".join(rng.choice(words) for _ in range(rng.randint(4, 30)))
            lines.append(f"{qid}\t{pid}\t{queries[qid]}\t{passages[pid]}\n")
    path.write_text("".join(lines), encoding="utf-8")


def main():
    import src.utils.defaults as ref_defaults

    ref_defaults.LOG_DIR = Path(tempfile.mkdtemp(prefix="ref_logs_"))
    from src.utils.datasets import TopKDataset

    fx = HERE / "topk_fixture.tsv"
    write_fixture(fx)
    ds = TopKDataset(top_k_path=fx)
    out = {"queries": ds.queries, "passages": ds.passages, "top_k": ds.top_k,
           "keys": list(ds.keys()), "len": len(ds), "min_len": ds.min_len,
           "max_len": ds.max_len, "avg_len": ds.avg_len,
           "getitem": {qid: ds[qid] for qid in ds.keys()}}
    (HERE / "topk_dataset.json").write_text(json.dumps(out, indent=1) + "\n", encoding="utf-8")


if __name__ == "__main__":
    main()
