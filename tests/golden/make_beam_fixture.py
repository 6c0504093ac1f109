#!/usr/bin/env python3
"""Generate tests/golden/beam_search.npz: what the installed `transformers` beam search (GenerationMixin._beam_search, do_sample=False)
does on the tiny config in fp32, case by case -- the per-step logits it ranked, and the sequences, sequences_scores and beam_indices
it returned.  Run by hand where `transformers` is installed (`python tests/golden/make_beam_fixture.py`); tests read only the .npz.

The tiny random weights almost never rank an EOS id inside the top beams, so a forward hook on lm_head adds a per-case bias to the
EOS logits -- and rounds every logit to an fp16-exact value, so that the file stores in two bytes exactly the numbers HF ranked.
Rows of `logits_<case>` are [step, beam, vocab] in HF's beam order."""
from __future__ import annotations

import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, ROOT)
sys.path.insert(0, HERE)

from oracle import qwen25vl  # noqa: E402

# (name, num_beams, early_stopping, length_penalty, repetition_penalty, max_new_tokens, prompt seed, EOS bias)
CASES = [
    ("b2_false_lp1", 2, False, 1.0, 1.0, 8, 11, 1.2),
    ("b2_true_lp0", 2, True, 0.0, 1.3, 8, 12, 1.6),
    ("b2_never_lp2", 2, "never", 2.0, 1.0, 8, 23, 2.0),
    ("b4_false_lp2", 4, False, 2.0, 1.3, 6, 24, 1.2),
    ("b4_true_lp1", 4, True, 1.0, 1.0, 6, 15, 1.6),
    ("b4_never_lp0", 4, "never", 0.0, 1.3, 6, 16, 0.0),
]
WEIGHTS = dict(seed=1, std=0.02, matrix_gain=4.0, bias_std=0.02, norm_jitter=0.1)
PROMPT_LEN = 9


def main():
    from hf_bridge import hf_model

    cfg = qwen25vl.tiny_config()
    model = hf_model(cfg, qwen25vl.synthetic_weights(cfg, **WEIGHTS), torch.float32)
    bias = torch.zeros(cfg.text.vocab_size)
    model.lm_head.register_forward_hook(lambda m, i, o: (o + bias).to(torch.float16).to(torch.float32))
    out = {"eos_token_ids": np.asarray(cfg.eos_token_ids, np.int32), "pad_token_id": np.int32(cfg.pad_token_id)}
    names = []
    for name, B, early, lp, pen, max_new, seed, eos_bias in CASES:
        rng = np.random.default_rng(seed)
        prompt = rng.integers(20, 2000, size=PROMPT_LEN)
        bias.zero_()
        bias[list(cfg.eos_token_ids)] = eos_bias
        ids = torch.from_numpy(prompt)[None]
        with torch.no_grad():
            g = model.generate(input_ids=ids, attention_mask=torch.ones_like(ids), max_new_tokens=max_new, do_sample=False, num_beams=B,
                               num_return_sequences=B, early_stopping=early, length_penalty=lp, repetition_penalty=pen,
                               return_dict_in_generate=True, output_scores=True, output_logits=True)
        logits = torch.stack(g.logits).numpy()   # [steps, B, vocab]
        assert np.array_equal(logits, logits.astype(np.float16).astype(np.float32))
        seqs = g.sequences.numpy()
        n_eos = int(np.isin(seqs[:, PROMPT_LEN:], cfg.eos_token_ids).any(axis=1).sum())
        print(f"{name}: steps {logits.shape[0]}, sequences {seqs.shape}, rows ending in EOS {n_eos}, scores {g.sequences_scores.numpy()}")
        names.append(name)
        out[f"prompt_{name}"] = prompt.astype(np.int32)
        out[f"params_{name}"] = np.asarray([B, {False: 0, True: 1, "never": 2}[early], max_new], np.int32)
        out[f"floats_{name}"] = np.asarray([lp, pen], np.float64)
        out[f"logits_{name}"] = logits.astype(np.float16)
        out[f"sequences_{name}"] = seqs.astype(np.int32)
        out[f"scores_{name}"] = g.sequences_scores.numpy().astype(np.float32)
        out[f"beam_indices_{name}"] = g.beam_indices.numpy().astype(np.int32)
    out["cases"] = np.asarray(names)
    path = os.path.join(HERE, "beam_search.npz")
    np.savez_compressed(path, **out)
    print(path, os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()
