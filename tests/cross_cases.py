"""Shared inputs of tests/test_cross_cpu.py and tests/test_cross_gpu.py (not a test
module): the hand-written pack-rule cases, the seeded text pairs of the split-vs-joined
tokenization check, and a local WordPiece tokenizer."""
import random
import string

import numpy as np

import local_tokenizer

PREFIX, SUFFIX, MAX_LENGTH = [0], [2], 16  # "<s> $A </s>", budget 14


def _doc(d, n):
    return [1000 * (d + 1) + j for j in range(n)]


def _qry(q, n):
    return [500000 + 1000 * q + j for j in range(n)]


# passages 0..7 of 10, 10, 20, 14, 5, 0, 4, 0 tokens; query parts 0..6 of 4, 5, 3, 3, 12, 3, 0
DOC_LENS = [10, 10, 20, 14, 5, 0, 4, 0]
QRY_LENS = [4, 5, 3, 3, 12, 3, 0]
DOCS = [_doc(d, n) for d, n in enumerate(DOC_LENS)]
QRYS = [_qry(q, n) for q, n in enumerate(QRY_LENS)]

# (name, passage, query part, expected sequence written out by hand)
PACK_CASES = [
    ("content of exactly 14", 0, 0,
     [0, 1000, 1001, 1002, 1003, 1004, 1005, 1006, 1007, 1008, 1009,
      500000, 500001, 500002, 500003, 2]),
    ("content of 15: the last query token is cut", 1, 1,
     [0, 2000, 2001, 2002, 2003, 2004, 2005, 2006, 2007, 2008, 2009,
      501000, 501001, 501002, 501003, 2]),
    ("cut inside the passage", 2, 2,
     [0, 3000, 3001, 3002, 3003, 3004, 3005, 3006, 3007, 3008, 3009, 3010, 3011, 3012, 3013,
      2]),
    ("cut at the passage / query boundary", 3, 3,
     [0, 4000, 4001, 4002, 4003, 4004, 4005, 4006, 4007, 4008, 4009, 4010, 4011, 4012, 4013,
      2]),
    ("cut inside the query", 4, 4,
     [0, 5000, 5001, 5002, 5003, 5004,
      504000, 504001, 504002, 504003, 504004, 504005, 504006, 504007, 504008, 2]),
    ("empty passage", 5, 5, [0, 505000, 505001, 505002, 2]),
    ("empty query part", 6, 6, [0, 7000, 7001, 7002, 7003, 2]),
    ("both empty", 7, 6, [0, 2]),
]


def store(seqs):
    off = np.zeros(len(seqs) + 1, np.int64)
    off[1:] = np.cumsum([len(s) for s in seqs])
    tok = np.array([t for s in seqs for t in s], np.int32)
    return tok, off


def seeded_text_pairs(n=2000, seed=5):
    """(passage, query) strings with trailing, leading and doubled spaces, punctuation,
    words outside the vocabulary, empty queries and a few empty passages."""
    rng = random.Random(seed)
    words = local_tokenizer.WORDS + ["zyxq", "Hello", "re-ranking", "don't", "3.14", "(index)",
                                     "[SEP]", "a,b", "UPPER", "x" * 12]

    def text(lo, hi):
        out = []
        for _ in range(rng.randint(lo, hi)):
            out.append(rng.choice(words))
            out.append(rng.choice([" ", " ", " ", "  ", " , ", ". ", "? "]))
        s = "".join(out)
        r = rng.random()
        if r < 0.25:
            s = s.rstrip()
        elif r < 0.4:
            s = " " + s
        elif r < 0.5:
            s = s.rstrip() + rng.choice(string.punctuation)
        return s

    pairs = []
    for _ in range(n):
        passage = "" if rng.random() < 0.02 else text(1, 40)
        query = "" if rng.random() < 0.05 else text(1, 8)
        pairs.append((passage, query))
    return pairs


def build_wordpiece_tokenizer():
    """bert-base-uncased's pipeline shape over the local word list: BertNormalizer,
    BertPreTokenizer, WordPiece, "[CLS] $A [SEP]", with [SEP] a special token that is
    matched in the raw text (as in the reference's joined string)."""
    from tokenizers import Tokenizer, models, normalizers, pre_tokenizers, processors

    vocab = ["[PAD]", "[UNK]", "[CLS]", "[SEP]", "[MASK]"]
    seen = set(vocab)

    def add(p):
        if p not in seen:
            seen.add(p)
            vocab.append(p)

    for w in local_tokenizer.WORDS:
        add(w)
    for s in local_tokenizer.SUBWORDS:
        add("##" + s)
        add(s)
    for c in string.ascii_lowercase + string.digits + string.punctuation:
        add(c)
        add("##" + c)
    tok = Tokenizer(models.WordPiece({p: i for i, p in enumerate(vocab)}, unk_token="[UNK]"))
    tok.normalizer = normalizers.BertNormalizer(lowercase=True)
    tok.pre_tokenizer = pre_tokenizers.BertPreTokenizer()
    tok.post_processor = processors.TemplateProcessing(
        single="[CLS] $A [SEP]", pair="[CLS] $A [SEP] $B:1 [SEP]:1",
        special_tokens=[("[CLS]", 2), ("[SEP]", 3)])
    tok.add_special_tokens(["[PAD]", "[UNK]", "[CLS]", "[SEP]", "[MASK]"])
    return tok
