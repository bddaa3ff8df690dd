"""Shared inputs of tests/test_encoder_cases_cpu.py, tests/test_encoder_peaked_gpu.py and
tests/test_encoder_shapes_gpu.py (not a test module): encoder shapes derived from the
xlm-roberta-base fixture, weights with peaked attention, the CPU oracle on one torch
thread, the oracle's attention logits and the two measures that say what an input can
see -- how many softmax rows force the device's running maximum to move after its first
key block, and how far the output moves when the heads of one projection are shifted."""
import contextlib
import functools
import json
import math

import numpy as np
import torch

import encoder_ref
from conftest import GOLDEN

LN2_8 = 8.0 * math.log(2.0)  # the device rescales when a score passes its reference by 8 (base 2)

# the shape family of test_encoder_shapes_gpu.py: (hidden, intermediate); heads = hidden / 64
SHAPES = [(64, 64), (192, 320), (256, 512), (384, 1536), (512, 1024), (832, 448), (1024, 4096),
          (1024, 1280)]
# intermediate < hidden on the folded bf16 path: the pruned last layer packs its gathered
# rows (hidden wide) into the FFN buffer (intermediate wide)
NARROW_FFN = (512, 256)
SHAPE_LENS = [385, 200, 130, 97, 65, 33, 32, 2, 1]
PEAKED_LENS = [512, 385, 384, 257, 256, 65, 64, 33, 32, 17, 1]
SEED = 7


def shapes(hidden, intermediate, vocab=1024, layers=2, max_positions=None, type_vocab=None):
    """(state_dict_shapes, config) of the xlm-roberta-base fixture with 768 -> hidden,
    3072 -> intermediate, 250002 -> vocab, layers >= `layers` dropped and
    num_attention_heads = hidden // 64; max_positions / type_vocab: the rows of the
    position and token-type tables (the fixture's 514 and 1 unless given)."""
    fx = json.loads((GOLDEN / "encoder_xlmr_base.json").read_text())
    sub = {768: hidden, 3072: intermediate, 250002: vocab}
    rows = {"bert.embeddings.position_embeddings.weight": max_positions,
            "bert.embeddings.token_type_embeddings.weight": type_vocab}
    out = []
    for k, shape, dtype in fx["state_dict_shapes"]:
        if ".layer." in k and int(k.split(".layer.")[1].split(".")[0]) >= layers:
            continue
        shape = [sub.get(d, d) for d in shape]
        if rows.get(k) is not None:
            shape[0] = rows[k]
        out.append((k, shape, dtype))
    cfg = dict(fx["config"])
    cfg.update(hidden_size=hidden, intermediate_size=intermediate, vocab_size=vocab,
               num_hidden_layers=layers, num_attention_heads=hidden // 64)
    if max_positions is not None:
        cfg["max_position_embeddings"] = max_positions
    if type_vocab is not None:
        cfg["type_vocab_size"] = type_vocab
    return out, cfg


def peaked_state_dict(shapes, seed, logit_std=6.0, vo_scale=2.0):
    """seeded_state_dict(std 0.02) with the query and key weights scaled so that the
    scaled logits q k^T / 8 have standard deviation ~ logit_std (the LayerNorm output has
    unit variance, so q and k have variance hidden * std_w^2 = logit_std each), and the
    value and attention-output weights scaled by vo_scale so that the attention output
    weighs against the residual."""
    sd = encoder_ref.seeded_state_dict(shapes, seed, 0.02)
    hidden = sd["bert.embeddings.LayerNorm.weight"].shape[0]
    qk = math.sqrt(logit_std / hidden) / 0.02
    with _one_torch_thread():
        for k in sd:
            if k.endswith(("attention.self.query.weight", "attention.self.key.weight")):
                sd[k] = sd[k] * qk
            elif k.endswith(("attention.self.value.weight", "attention.output.dense.weight")):
                sd[k] = sd[k] * vo_scale
    return sd


def batch(rng, lens, vocab):
    """Padded ids / mask [B, max(lens)]: token 0 first, ids in [5, vocab), pad id 1."""
    ids = [rng.integers(5, vocab, n).astype(np.int64) for n in lens]
    for a in ids:
        a[0] = 0
    pad = np.ones((len(lens), max(lens)), np.int64)
    mask = np.zeros_like(pad)
    for i, a in enumerate(ids):
        pad[i, :len(a)] = a
        mask[i, :len(a)] = 1
    return pad, mask


def pack(pad, mask):
    lens = mask.sum(1)
    ids = np.concatenate([pad[i, :n] for i, n in enumerate(lens)]).astype(np.int32)
    cu = np.zeros(len(lens) + 1, np.int32)
    cu[1:] = np.cumsum(lens)
    return ids, cu


@contextlib.contextmanager
def _one_torch_thread():
    """The CPU oracle on one thread: a torch thread pool started in this process would
    deadlock the workers that tests/test_distributed_cpu.py forks from it later.  Every
    torch operation of this module runs under it (casts and weight scaling included)."""
    n = torch.get_num_threads()
    torch.set_num_threads(1)
    try:
        yield
    finally:
        torch.set_num_threads(n)


def _cast(sd, dtype):
    return {k: v.to(dtype) for k, v in sd.items()}


def oracle(sd, cfg, pad, mask, act="softplus", dtype=torch.float64):
    """encoder_ref.forward on the state dict cast to `dtype` -> the impacts of the real
    tokens, packed in document order (numpy float64).  Each document is one call on its
    own unpadded row: a masked key contributes exp(-huge) = 0 exactly, so this is the
    padded batch's result without the padded rows' arithmetic."""
    out = []
    with torch.no_grad(), _one_torch_thread():
        sd = _cast(sd, dtype)
        for i, n in enumerate(mask.sum(1)):
            row = encoder_ref.forward(sd, cfg, torch.from_numpy(pad[i:i + 1, :n]),
                                      torch.from_numpy(mask[i:i + 1, :n]), "xlmr", act)
            out.append(row[0].double().numpy())
    return np.concatenate(out)


def _restated_forward(sd, cfg, ids, m, dtype, rnd, logits=None):
    """encoder_ref.forward written out again (XLM-R, softplus) so that it can hand out
    the attention logits and round what is stored between operations: `rnd` is applied to
    the embedding tables and weights, to every LayerNorm output, to Q | K | V, to the
    probabilities, the attention output, the GELU output and the pre-LayerNorm sums."""
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
    for i in range(cfg["num_hidden_layers"]):
        L = f"{p}encoder.layer.{i}."

        def lin(t, name):
            return t @ w[L + name + ".weight"].T + w[L + name + ".bias"]

        def heads(t):
            return rnd(t).view(B, S, nh, 64).transpose(1, 2)

        s = heads(lin(x, "attention.self.query")) @ heads(
            lin(x, "attention.self.key")).transpose(-1, -2) / 8.0 + neg
        if logits is not None:
            logits.append(s)
        ctx = rnd((rnd(torch.softmax(s, -1)) @ heads(lin(x, "attention.self.value"))).transpose(
            1, 2).reshape(B, S, H))
        x = rnd(encoder_ref.layer_norm(rnd(x + lin(ctx, "attention.output.dense")),
                                       w[L + "attention.output.LayerNorm.weight"],
                                       w[L + "attention.output.LayerNorm.bias"], eps))
        h = rnd(torch.nn.functional.gelu(lin(x, "intermediate.dense")))
        x = encoder_ref.layer_norm(rnd(x + lin(h, "output.dense")),
                                   w[L + "output.LayerNorm.weight"],
                                   w[L + "output.LayerNorm.bias"], eps)
        if i + 1 < cfg["num_hidden_layers"]:
            x = rnd(x)  # (the last LayerNorm feeds the f32 impact head only)
    z = x @ sd["impact_score_encoder.0.weight"][0] + sd["impact_score_encoder.0.bias"][0]
    return torch.nn.functional.softplus(z)


def layer_logits(sd, cfg, pad, mask, dtype=torch.float32):
    """The masked scaled scores q k^T / 8 of every layer, [B, heads, S, S] each, from a
    restatement of encoder_ref.forward on the padded batch; also returns that forward's
    packed impacts, which test_encoder_cases_cpu.py holds against encoder_ref.forward."""
    logits = []
    with torch.no_grad(), _one_torch_thread():
        imp = _restated_forward(_cast(sd, dtype), cfg, torch.from_numpy(pad),
                                torch.from_numpy(mask), dtype, lambda t: t, logits)
    return logits, imp.double().numpy()[mask.astype(bool)]


def oracle_bf16_storage(sd, cfg, pad, mask):
    """What the bf16 number format alone costs: the restated forward in float32 with
    every tensor the bf16 mode keeps in memory rounded to bf16 (tables and weights,
    activations between operations; sums, softmax, LayerNorm and GELU in float32).
    Packed impacts, document by document as oracle()."""
    def rnd(t):
        return t.to(torch.bfloat16).to(torch.float32)

    out = []
    with torch.no_grad(), _one_torch_thread():
        sd = _cast(sd, torch.float32)
        for i, n in enumerate(mask.sum(1)):
            row = _restated_forward(sd, cfg, torch.from_numpy(pad[i:i + 1, :n]),
                                    torch.from_numpy(mask[i:i + 1, :n]), torch.float32, rnd)
            out.append(row[0].double().numpy())
    return np.concatenate(out)


def rescale_rows(logits, lens, block):
    """One layer's logits [B, heads, S, S] -> the fraction of (document, head, query)
    rows in which some key block b >= 1 (keys in order, `block` keys per block) has a
    maximum more than 8 ln 2 above the maximum of all earlier blocks; documents longer
    than `block` only.  A lower bound on the rows in which the device must rescale: its
    stale reference maximum is never above the running maximum."""
    hit = rows = 0
    with _one_torch_thread():
        for d, n in enumerate(lens):
            if n <= block:
                continue
            s = logits[d, :, :n, :n]
            nb = -(-n // block)
            s = torch.nn.functional.pad(s, (0, nb * block - n), value=-math.inf)
            bm = s.reshape(s.shape[0], n, nb, block).amax(-1)
            before = torch.cummax(bm, -1).values[..., :-1]
            hit += int((bm[..., 1:] > before + LN2_8).any(-1).sum())
            rows += s.shape[0] * n
    return hit / rows if rows else 0.0


def roll_heads(sd, which):
    """Every layer's `which` ("query" | "key" | "value") projection moved by one head:
    weight and bias rolled by 64 rows, so head h computes with head h-1's projection."""
    sd = dict(sd)
    with _one_torch_thread():
        for k in sd:
            if f"attention.self.{which}." in k:
                sd[k] = torch.roll(sd[k], 64, 0)
    return sd


def sensitive_fraction(a, b, rel=1e-2):
    """Fraction of tokens at which b differs from a by more than `rel` relative."""
    return float(np.mean(np.abs(b - a) > rel * np.abs(a)))


def device_config(E, cfg):
    return E.EncoderConfig(variant="xlmr", activation="softplus", vocab_size=cfg["vocab_size"],
                           hidden=cfg["hidden_size"], layers=cfg["num_hidden_layers"],
                           heads=cfg["num_attention_heads"],
                           intermediate=cfg["intermediate_size"],
                           max_positions=cfg["max_position_embeddings"],
                           type_vocab=cfg["type_vocab_size"], pad_id=cfg["pad_token_id"],
                           layer_norm_eps=cfg["layer_norm_eps"])


def case(hidden, intermediate, lens, seed=SEED, vocab=1024):
    """(shapes, cfg, peaked weights, pad, mask) of one test configuration."""
    shp, cfg = shapes(hidden, intermediate, vocab)
    sd = peaked_state_dict(shp, seed)
    pad, mask = batch(np.random.default_rng(seed + hidden + intermediate), lens, vocab)
    return shp, cfg, sd, pad, mask


@functools.lru_cache(maxsize=None)
def want(hidden, intermediate, lens):
    """The float64 oracle's packed impacts of case(hidden, intermediate, lens) (lens a
    tuple), computed once per process and shared by every test that needs it (read only)."""
    _, cfg, sd, pad, mask = case(hidden, intermediate, list(lens))
    w = oracle(sd, cfg, pad, mask)
    w.setflags(write=False)
    return w


@functools.lru_cache(maxsize=None)
def bf16_format_error(hidden, intermediate, lens):
    """Median relative error of oracle_bf16_storage against the float64 oracle."""
    _, cfg, sd, pad, mask = case(hidden, intermediate, list(lens))
    return float(np.median(rel_err(oracle_bf16_storage(sd, cfg, pad, mask),
                                   want(hidden, intermediate, lens))))


def rel_err(got, w):
    return np.abs(got - w) / np.maximum(np.abs(w), 1e-3)


def assert_fp32_bound(got, w):
    """The project's north-star bound (fp32 and bf16x3): 1e-3 relative."""
    np.testing.assert_allclose(got, w, rtol=1e-3, atol=1e-6)


def assert_bf16_bound(got, w):
    """The project's bf16 bound (tests/test_encoder_gpu.py): |d| <= 0.05 + 0.05 |x| per
    token and median relative error < 1e-2."""
    err = np.abs(got - w)
    assert (err <= 0.05 + 0.05 * np.abs(w)).all(), float((err - 0.05 * np.abs(w)).max())
    assert float(np.median(rel_err(got, w))) < 1e-2


def assert_bf16_format_bound(got, w, format_error):
    """The bf16 bound above is one figure for every shape and lets a small model be
    wrong by twenty times its own rounding error.  This one follows the number format:
    the median relative error is at most twice that of oracle_bf16_storage on the same
    input (bf16_format_error), which rounds to bf16 exactly the tensors the bf16 mode
    keeps in memory.  The factor 2 is for what the emulation leaves in float32 and the
    device does not: bf16 MFMA operands of folded weights (W gamma rounded once more),
    the tanh-form GELU and the exp2-based softmax -- at most one further rounding of the
    size of those it already counts per stored tensor."""
    med = float(np.median(rel_err(got, w)))
    assert med <= 2.0 * format_error, (med, format_error)


def random_terms(rng, lens, none=2, whole=0, repeat=3):
    """Term rows for the pruned-last-layer check: document `none` without terms, all
    tokens of document `whole`, two positions of document `repeat` twice, every
    document's positions unsorted."""
    tt, ct = [], [0]
    for d, n in enumerate(lens):
        k = 0 if d == none else (n if d == whole else int(rng.integers(1, n + 1)))
        pos = rng.choice(n, size=k, replace=False)
        if d == repeat:
            pos = np.concatenate([pos, pos[:2]])
        tt += pos.tolist()
        ct.append(len(tt))
    return np.array(tt, np.int32), np.array(ct, np.int32)
