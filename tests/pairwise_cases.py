"""Shared inputs of tests/test_pairwise_cases_cpu.py and tests/test_pairwise_gpu.py (not a
test module): the peaked encoder of encoder_cases with a ReLU head and the pair head of
DeepPairwiseImpact (reference src/deep_impact/models/pairwise_impact.py), the terms of
every document, the forward restated once more so that it hands out the last hidden state
and every layer's softmax probabilities, the float64 oracle of (single, attn, pair score)
with the variants that say what the inputs can see, and the CPU storage emulations from
which the pair-score tolerance is derived."""
import functools
from itertools import combinations

import numpy as np
import torch

import encoder_cases as C
import encoder_ref

LENS = (512, 257, 65, 33, 32, 17, 2, 1)
SMALL = (192, 320, (65, 33, 2))  # 3 heads, a shape outside the 256-tile path
PAIR_SEED, TERM_SEED = 5, 21


def pair_head(hidden):
    """pairwise_impact_score_encoder: ([2H + 1] float32 weight, bias).  Element 0 (the
    attention's weight) is 4 so that the attention moves the score."""
    w = np.random.default_rng(PAIR_SEED).standard_normal(2 * hidden + 1) * 0.02
    w[0] = 4.0
    return w.astype(np.float32), np.float32(0.0)


def terms(lens):
    """(term_tok int32, cu_terms int32): per document its kept terms' token index,
    ascending.  Drawn in document order from one generator."""
    rng = np.random.default_rng(TERM_SEED)
    tt, ct = [], [0]
    for n in lens:
        if n == 512:  # both ends plus 46 inner positions
            pos = np.concatenate([[0, 511], rng.choice(np.arange(1, 511), 46, replace=False)])
        elif n == 257:
            pos = rng.choice(n, 17, replace=False)
        elif n == 33:
            pos = rng.choice(n, 16, replace=False)
        elif n == 32:
            pos = np.zeros(0, np.int64)
        else:  # 65 (crosses the 16-row tile and the 64-key chunk), 17, 2, 1: every token
            pos = np.arange(n)
        tt += sorted(int(p) for p in pos)
        ct.append(len(tt))
    return np.array(tt, np.int32), np.array(ct, np.int32)


def n_pairs(ct):
    T = np.diff(ct.astype(np.int64))
    return int((T * (T - 1) // 2).sum())


@functools.lru_cache(maxsize=None)
def inputs(hidden=768, intermediate=3072, lens=LENS):
    """(cfg, state dict with the pair head, pad, mask, term_tok, cu_terms)."""
    _, cfg, sd, pad, mask = C.case(hidden, intermediate, list(lens))
    w, b = pair_head(hidden)
    sd = dict(sd)
    sd["pairwise_impact_score_encoder.0.weight"] = torch.from_numpy(w.reshape(1, -1).copy())
    sd["pairwise_impact_score_encoder.0.bias"] = torch.from_numpy(np.array([b], np.float32))
    tt, ct = terms(lens)
    return cfg, sd, pad, mask, tt, ct


def device_config(E, cfg):
    c = C.device_config(E, cfg)
    c.activation = "relu"
    return c


def restated_forward(sd, cfg, ids, m, dtype, rnd):
    """encoder_cases._restated_forward once more (XLM-R positions), returning the last
    hidden state [B, S, H] and every layer's softmax probabilities [B, heads, S, S].
    `rnd` is applied to what is stored between operations, as there: tables and weights,
    LayerNorm outputs, Q | K | V, the probabilities that multiply V, the attention
    output, the GELU output and the pre-LayerNorm sums.  The probabilities handed out are
    the softmax of the stored Q and K, not rounded again: the device computes them anew
    from those and keeps them in registers."""
    p = "bert."
    H, nh, eps = cfg["hidden_size"], cfg["num_attention_heads"], cfg["layer_norm_eps"]
    w = {k: (v if k.endswith(("bias", "LayerNorm.weight")) else rnd(v)) for k, v in sd.items()}
    pos = encoder_ref.position_ids(ids, "xlmr", cfg["pad_token_id"])
    x = (w[p + "embeddings.word_embeddings.weight"][ids]
         + w[p + "embeddings.position_embeddings.weight"][pos]
         + w[p + "embeddings.token_type_embeddings.weight"][0])
    x = rnd(encoder_ref.layer_norm(x, w[p + "embeddings.LayerNorm.weight"],
                                   w[p + "embeddings.LayerNorm.bias"], eps))
    B, S, _ = x.shape
    neg = ((1.0 - m[:, None, None, :].float()) * torch.finfo(torch.float32).min).to(dtype)
    probs = []
    for i in range(cfg["num_hidden_layers"]):
        L = f"{p}encoder.layer.{i}."

        def lin(t, name):
            return t @ w[L + name + ".weight"].T + w[L + name + ".bias"]

        def heads(t):
            return rnd(t).view(B, S, nh, 64).transpose(1, 2)

        s = heads(lin(x, "attention.self.query")) @ heads(
            lin(x, "attention.self.key")).transpose(-1, -2) / 8.0 + neg
        pr = torch.softmax(s, -1)
        probs.append(pr)
        ctx = rnd((rnd(pr) @ heads(lin(x, "attention.self.value"))).transpose(
            1, 2).reshape(B, S, H))
        x = rnd(encoder_ref.layer_norm(rnd(x + lin(ctx, "attention.output.dense")),
                                       w[L + "attention.output.LayerNorm.weight"],
                                       w[L + "attention.output.LayerNorm.bias"], eps))
        h = rnd(torch.nn.functional.gelu(lin(x, "intermediate.dense")))
        x = encoder_ref.layer_norm(rnd(x + lin(h, "output.dense")),
                                   w[L + "output.LayerNorm.weight"],
                                   w[L + "output.LayerNorm.bias"], eps)
        if i + 1 < cfg["num_hidden_layers"]:
            x = rnd(x)
    return x, probs


def pair_outputs(x, probs, tok, sd, attn_mode="full"):
    """One document's (single [T], attn [P], pre-activation [P], score [P]) in float64 from
    its last hidden state x [S, H] and probabilities (per layer [heads, S, S]); tok: the
    terms' token index, ascending; pairs in itertools.combinations order
    (pairwise_impact.py:59-87).  attn_mode: "full", or what a wrong kernel would compute:
    "zero", "one_direction" (P[a, b] only), "last_layer", "head0" (no mean over heads)."""
    x = x.double()
    hw = sd["impact_score_encoder.0.weight"][0].double()
    hb = sd["impact_score_encoder.0.bias"][0].double()
    pw = sd["pairwise_impact_score_encoder.0.weight"][0].double()
    pb = sd["pairwise_impact_score_encoder.0.bias"][0].double()
    H = x.shape[1]
    tok = torch.as_tensor(np.asarray(tok, np.int64))
    single = torch.relu(x[tok] @ hw + hb)
    T = len(tok)
    iu = torch.triu_indices(T, T, 1)  # row-major: the combinations order
    a, b = iu[0], iu[1]
    layers = probs[-1:] if attn_mode == "last_layer" else probs
    best = None
    for pr in layers:
        pr = pr.double()
        mean = pr[0] if attn_mode == "head0" else pr.mean(0)
        sub = mean[tok][:, tok]
        m = sub if attn_mode == "one_direction" else torch.maximum(sub, sub.T)
        best = m if best is None else torch.maximum(best, m)
    attn = best[a, b] if T > 1 else torch.zeros(0, dtype=torch.float64)
    if attn_mode == "zero":
        attn = torch.zeros_like(attn)
    u, v = x[tok] @ pw[1:H + 1], x[tok] @ pw[H + 1:]
    pre = pw[0] * attn + u[a] + v[b] + pb
    return (single.numpy(), attn.numpy(), pre.numpy(), torch.relu(pre).numpy())


def _run(hidden, intermediate, lens, dtype, rnd, modes=("full",)):
    """{mode: (single, attn, pre, score)} packed over the documents, each document one
    forward on its own unpadded row (as encoder_cases.oracle)."""
    cfg, sd, pad, mask, tt, ct = inputs(hidden, intermediate, lens)
    parts = {m: [] for m in modes}
    with torch.no_grad(), C._one_torch_thread():
        sdc = C._cast(sd, dtype)
        for d, n in enumerate(mask.sum(1)):
            x, probs = restated_forward(sdc, cfg, torch.from_numpy(pad[d:d + 1, :n]),
                                        torch.from_numpy(mask[d:d + 1, :n]), dtype, rnd)
            for m in modes:
                parts[m].append(pair_outputs(x[0], [p[0] for p in probs],
                                             tt[ct[d]:ct[d + 1]], sdc, m))
    out = {}
    for m in modes:
        cat = tuple(np.concatenate([p[i] for p in parts[m]]) for i in range(4))
        for a in cat:
            a.setflags(write=False)
        out[m] = cat
    return out


VARIANTS = ("zero", "one_direction", "last_layer", "head0")


@functools.lru_cache(maxsize=None)
def oracle(hidden=768, intermediate=3072, lens=LENS, variants=False):
    """The float64 oracle, computed once per process (read only)."""
    return _run(hidden, intermediate, lens, torch.float64, lambda t: t,
                ("full",) + (VARIANTS if variants else ()))


def _split16(t):
    """hi + lo with hi = bf16(v), lo = bf16(v - hi): the bf16x3 mode's storage."""
    f = t.to(torch.float32)
    hi = f.to(torch.bfloat16).to(torch.float32)
    lo = (f - hi).to(torch.bfloat16).to(torch.float32)
    return (hi + lo).to(t.dtype)


@functools.lru_cache(maxsize=None)
def emulation(kind, hidden=768, intermediate=3072, lens=LENS):
    """The CPU storage emulation of a precision: "bf16x3" = float64 arithmetic with every
    stored tensor rounded to the split's 16 significant bits; "fp32" = the torch float32
    forward.  The head on top runs in float64 either way."""
    if kind == "fp32":
        return _run(hidden, intermediate, lens, torch.float32, lambda t: t)["full"]
    return _run(hidden, intermediate, lens, torch.float64, _split16)["full"]


def pair_atol(kind, hidden=768, intermediate=3072, lens=LENS):
    """The absolute part of the pair-score criterion: 4 x the largest absolute pair-score
    error of the precision's storage emulation against float64 on these inputs.  The
    factor covers what the emulation leaves in float64 and the device does not (f32
    accumulation order, the exp2 form, the LayerNorm in f32) on an extreme over thousands
    of values, where the project's factor 2 is for medians.  It must stay below 5e-4, half
    the 3-decimal step the scores are written in: if it does not, the inputs are wrong,
    not the bound."""
    emu = emulation(kind, hidden, intermediate, lens)
    want = oracle(hidden, intermediate, lens)["full"]
    atol = 4.0 * float(np.abs(emu[3] - want[3]).max())
    assert atol < 5e-4, atol
    return atol


def restated_term_impacts(maps, token_impacts, pair_scores):
    """What DeepPairwiseImpact.compute_term_impacts defines (pairwise_impact.py:98-129),
    written as plain loops: per document its terms in map order, then every 2-combination
    of its terms sorted by token index whose score does not round to 0.000, named
    't1|t2', and the list sorted by score, descending and stable."""
    out = []
    for d, m in enumerate(maps):
        entries = [(t, token_impacts[d][i]) for t, i in m.items()]
        by_token = sorted(m.items(), key=lambda kv: kv[1])
        for j, (p, q) in enumerate(combinations(by_token, 2)):
            s = pair_scores[d][j]
            if round(s, 3) != 0:
                entries.append((p[0] + "|" + q[0], s))
        out.append(sorted(entries, key=lambda e: e[1], reverse=True))
    return out


def restated_lines(docs):
    """The impact-TSV text of indexer.py:62-67: 'term: round(impact, 3)' joined by ', ',
    one line per document."""
    return "".join(", ".join(f"{t}: {round(v, 3)}" for t, v in doc) + "\n" for doc in docs)
