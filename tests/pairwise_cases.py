"""Shared inputs of tests/test_pairwise_cases_cpu.py, tests/test_pairwise_gpu.py and
tests/test_pairwise_routes_gpu.py (not a test module): the peaked encoder of encoder_cases
with a ReLU head and the pair head of DeepPairwiseImpact (reference
src/deep_impact/models/pairwise_impact.py), the terms of
every document, the forward restated once more so that it hands out the last hidden state
and every layer's softmax probabilities, the float64 oracle of (single, attn, pair score)
with the variants that say what the inputs can see, and the CPU storage emulations from
which the pair-score tolerance is derived; and ROUTE_CASES, the seeded cases that reach
the launch routes the one batch LENS does not."""
import functools
from itertools import combinations
from typing import NamedTuple, Optional

import numpy as np
import torch

import encoder_cases as C
import encoder_ref

LENS = (512, 257, 65, 33, 32, 17, 2, 1)
SMALL = (192, 320, (65, 33, 2))  # 3 heads, a shape outside the 256-tile path
PAIR_SEED, TERM_SEED = 5, 21


def pair_head(hidden, bias=0.0):
    """pairwise_impact_score_encoder: ([2H + 1] float32 weight, bias).  Element 0 (the
    attention's weight) is 4 so that the attention moves the score."""
    w = np.random.default_rng(PAIR_SEED).standard_normal(2 * hidden + 1) * 0.02
    w[0] = 4.0
    return w.astype(np.float32), np.float32(bias)


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


class Case(NamedTuple):
    """One test configuration; the defaults are the inputs of tests/test_pairwise_gpu.py.
    variant "bert": absolute positions, a 2-row type table, LayerNorm eps 1e-12
    (original.DeepImpact, which DeepPairwiseImpact extends).  terms: (term_tok, cu_terms)
    as tuples, None for terms(lens).  pair_bias: the pair head's bias.  rules: the rule
    each document's terms were drawn by (rule_terms), where the case records it."""
    hidden: int = 768
    intermediate: int = 3072
    lens: tuple = LENS
    variant: str = "xlmr"
    layers: int = 2
    max_positions: Optional[int] = None
    terms: Optional[tuple] = None
    logit_std: float = 6.0
    seed: int = C.SEED
    pair_bias: float = 0.0
    rules: Optional[tuple] = None


def _case(*a, **kw):
    """A Case from a Case or from Case's fields (the functions below take either)."""
    if a and isinstance(a[0], Case):
        if len(a) > 1 or kw:
            raise TypeError("a Case takes no further fields")
        return a[0]
    return Case(*a, **kw)


def inputs(*a, **kw):
    """(cfg, state dict with the pair head, pad, mask, term_tok, cu_terms)."""
    return _inputs(_case(*a, **kw))


@functools.lru_cache(maxsize=None)
def _inputs(c):
    bert = c.variant == "bert"
    shp, cfg = C.shapes(c.hidden, c.intermediate, 1024, c.layers, c.max_positions,
                        2 if bert else None)
    if bert:
        cfg["layer_norm_eps"] = 1e-12
    sd = C.peaked_state_dict(shp, c.seed, c.logit_std)
    pad, mask = C.batch(np.random.default_rng(c.seed + c.hidden + c.intermediate), list(c.lens),
                        1024)
    w, b = pair_head(c.hidden, c.pair_bias)
    sd["pairwise_impact_score_encoder.0.weight"] = torch.from_numpy(w.reshape(1, -1).copy())
    sd["pairwise_impact_score_encoder.0.bias"] = torch.from_numpy(np.array([b], np.float32))
    if c.terms is None:
        tt, ct = terms(c.lens)
    else:
        tt, ct = (np.array(t, np.int32) for t in c.terms)
    return cfg, sd, pad, mask, tt, ct


def device_config(E, cfg, variant="xlmr"):
    c = C.device_config(E, cfg)
    c.activation = "relu"
    c.variant = variant
    return c


def restated_forward(sd, cfg, ids, m, dtype, rnd, variant="xlmr"):
    """encoder_cases._restated_forward once more, returning the last hidden state
    [B, S, H] and every layer's softmax probabilities [B, heads, S, S].  variant: XLM-R
    positions (pad id + 1 onwards) or "bert" (from 0); type row 0 and cfg's eps either way.
    `rnd` is applied to what is stored between operations, as there: tables and weights,
    LayerNorm outputs, Q | K | V, the probabilities that multiply V, the attention
    output, the GELU output and the pre-LayerNorm sums.  The probabilities handed out are
    the softmax of the stored Q and K, not rounded again: the device computes them anew
    from those and keeps them in registers."""
    p = "bert."
    H, nh, eps = cfg["hidden_size"], cfg["num_attention_heads"], cfg["layer_norm_eps"]
    w = {k: (v if k.endswith(("bias", "LayerNorm.weight")) else rnd(v)) for k, v in sd.items()}
    pos = encoder_ref.position_ids(ids, variant, cfg["pad_token_id"])
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
    "zero", "one_direction" (P[a, b] only), "last_layer", "head0" (no mean over heads);
    "layer<i>": layer i alone (which layer holds a pair's maximum)."""
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
    if attn_mode.startswith("layer"):
        layers = [probs[int(attn_mode[5:])]]
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


def _run(c, dtype, rnd, modes=("full",), positions=None):
    """{mode: (single, attn, pre, score)} packed over the documents, each document one
    forward on its own unpadded row (as encoder_cases.oracle; rows of equal length share
    a call).  positions: the position
    rule, the case's variant unless given."""
    cfg, sd, pad, mask, tt, ct = _inputs(c)
    lens = mask.sum(1)
    docs = [None] * len(lens)
    with torch.no_grad(), C._one_torch_thread():
        sdc = C._cast(sd, dtype)
        # documents of one length run as one batch without padding: each row is still its
        # own document's forward, and 300 short documents cost 8 forwards instead of 300
        for n in sorted(set(lens.tolist())):
            rows = np.flatnonzero(lens == n)
            x, probs = restated_forward(sdc, cfg, torch.from_numpy(pad[rows, :n]),
                                        torch.from_numpy(mask[rows, :n]), dtype, rnd,
                                        positions or c.variant)
            for i, d in enumerate(rows):
                docs[d] = {m: pair_outputs(x[i], [p[i] for p in probs], tt[ct[d]:ct[d + 1]],
                                           sdc, m) for m in modes}
    parts = {m: [doc[m] for doc in docs] for m in modes}
    out = {}
    for m in modes:
        cat = tuple(np.concatenate([p[i] for p in parts[m]]) for i in range(4))
        for a in cat:
            a.setflags(write=False)
        out[m] = cat
    return out


VARIANTS = ("zero", "one_direction", "last_layer", "head0")


def oracle(*a, variants=False, positions=None, **kw):
    """The float64 oracle, computed once per process (read only)."""
    return _oracle(_case(*a, **kw), variants, positions)


@functools.lru_cache(maxsize=None)
def _oracle(c, variants, positions):
    return _run(c, torch.float64, lambda t: t, ("full",) + (VARIANTS if variants else ()),
                positions)


def layer_attn(c):
    """[layers, n_pairs]: every pair's attention from one layer alone (float64); the
    oracle's attn is the maximum over axis 0."""
    modes = tuple(f"layer{i}" for i in range(c.layers))
    out = _run(c, torch.float64, lambda t: t, modes)
    return np.stack([out[m][1] for m in modes])


def _split16(t):
    """hi + lo with hi = bf16(v), lo = bf16(v - hi): the bf16x3 mode's storage."""
    f = t.to(torch.float32)
    hi = f.to(torch.bfloat16).to(torch.float32)
    lo = (f - hi).to(torch.bfloat16).to(torch.float32)
    return (hi + lo).to(t.dtype)


def emulation(kind, *a, **kw):
    """The CPU storage emulation of a precision: "bf16x3" = float64 arithmetic with every
    stored tensor rounded to the split's 16 significant bits; "fp32" = the torch float32
    forward.  The head on top runs in float64 either way."""
    return _emulation(kind, _case(*a, **kw))


@functools.lru_cache(maxsize=None)
def _emulation(kind, c):
    if kind == "fp32":
        return _run(c, torch.float32, lambda t: t)["full"]
    return _run(c, torch.float64, _split16)["full"]


def pair_atol(kind, *a, **kw):
    """The absolute part of the pair-score criterion: 4 x the largest absolute pair-score
    error of the precision's storage emulation against float64 on these inputs.  The
    factor covers what the emulation leaves in float64 and the device does not (f32
    accumulation order, the exp2 form, the LayerNorm in f32) on an extreme over thousands
    of values, where the project's factor 2 is for medians.  It must stay below 5e-4, half
    the 3-decimal step the scores are written in: if it does not, the inputs are wrong,
    not the bound."""
    emu = emulation(kind, *a, **kw)
    want = oracle(*a, **kw)["full"]
    atol = 4.0 * float(np.abs(emu[3] - want[3]).max())
    assert atol < 5e-4, atol
    return atol


# ---- the launch routes that LENS does not reach (tests/test_pairwise_routes_gpu.py) ----

ROUTE_LENS = (1, 2, 3, 5, 16, 17, 31, 33)
RULES = ("none", "one", "all", "subset")


def rule_terms(lens, rules, seed):
    """(term_tok, cu_terms) as tuples: document d keeps no term, one token, every token,
    a random non-empty subset of its tokens or (rules[d] an int) a random subset of that
    size, ascending."""
    rng = np.random.default_rng(seed)
    tt, ct = [], [0]
    for n, r in zip(lens, rules):
        if r == "none":
            pos = []
        elif r == "one":
            pos = [int(rng.integers(n))]
        elif r == "all":
            pos = range(n)
        else:
            k = int(rng.integers(1, n + 1)) if r == "subset" else r
            pos = sorted(rng.choice(n, k, replace=False).tolist())
        tt += [int(p) for p in pos]
        ct.append(len(tt))
    return tuple(tt), tuple(ct)


def all_terms(lens):
    return rule_terms(lens, ["all"] * len(lens), 0)


def many_docs(n_docs, seed):
    """(lens, rules) of n_docs documents: lengths drawn from ROUTE_LENS, each document's
    rule drawn from RULES; documents 8..11 and, where there are that many, 256..259 take
    the four rules in order, "all" at 17 tokens and "subset" at 33, so that every rule
    occurs with pairs in a second group of 8 and past document 256 whatever the seed."""
    rng = np.random.default_rng(seed)
    lens = [int(n) for n in rng.choice(ROUTE_LENS, n_docs)]
    rules = [RULES[int(r)] for r in rng.integers(0, 4, n_docs)]
    for d0 in (8, 256):
        if d0 + 3 < n_docs:
            rules[d0:d0 + 4] = RULES
            lens[d0 + 2:d0 + 4] = 17, 33
    return tuple(lens), tuple(rules)


def _route_cases():
    out = {}
    # pair_bias: with bias 0 these short documents (attn ~ 1 / n, weighted by 4) leave
    # 0.04 of the pair scores at exactly 0, under the 1/10 that the ReLU's zero side needs
    lens, rules = many_docs(300, 31)
    out["many_docs"] = Case(192, 320, lens, terms=rule_terms(lens, rules, 32), pair_bias=-0.4,
                            rules=rules)
    lens, rules = many_docs(19, 33)
    out["many_docs_x3"] = Case(768, 3072, lens, terms=rule_terms(lens, rules, 34), rules=rules)
    # wide: all 300 tokens, 256 of the 257 (token 100 dropped), all 40, all 17
    wl = (300, 257, 40, 17)
    tt, ct = all_terms(wl)
    tt = tt[:300 + 100] + tt[300 + 101:]
    ct = (ct[0], ct[1]) + tuple(c - 1 for c in ct[2:])
    out["wide"] = Case(1024, 1280, wl, terms=(tt, ct))
    out["heads64"] = Case(64, 64, (130, 40), terms=all_terms((130, 40)))
    out["heads832"] = Case(832, 448, (130, 40), terms=all_terms((130, 40)))
    ll = (65, 33, 17, 2)
    out["layers4"] = Case(192, 320, ll, layers=4, terms=all_terms(ll))
    # pair_bias: this seed's u_a + v_b has mean +0.7 and bias 0 leaves 0.01 of the scores at 0
    out["bert"] = Case(768, 3072, ll, variant="bert",
                       terms=rule_terms(ll, [40, 20, 9, 2], 35), pair_bias=-0.6)
    # long: the largest document the LDS panel admits; 24 of its tokens, both ends among them
    rng = np.random.default_rng(36)
    t24 = sorted([0, 1231] + rng.choice(np.arange(1, 1231), 22, replace=False).tolist())
    out["long"] = Case(192, 320, (1232, 17), max_positions=1240,
                       terms=(tuple(int(t) for t in t24) + tuple(range(17)), (0, 24, 41)))
    return out


ROUTE_CASES = _route_cases()
# the device precisions each case runs in ("-nofold": DI_NO_LN_FOLD=1)
ROUTE_PRECS = {"many_docs": ("fp32",), "many_docs_x3": ("bf16x3", "bf16x3-nofold"),
               "wide": ("fp32", "bf16x3", "bf16x3-nofold"), "heads64": ("fp32",),
               "heads832": ("fp32",), "layers4": ("fp32",), "bert": ("fp32", "bf16x3"),
               "long": ("fp32",)}


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
