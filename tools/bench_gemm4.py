"""Times the projections of the 2 .. 64-chain decode step (decode family 0, the fragment kernels) for three weight forms in ONE process
on one box: the dequantised bf16 fragments of an MXFP4 engine (ze_tune knob 24 = 1, the form before the W4 kernels), the FP8 fragment
stream and the MXFP4 fragment stream (knob 24 = 0).  Per projection (qkv, o, gate/up, down, lm_head) at 16 and 64 rows through
ze_profile_batch_kernel, which launches the step's own functions over the layers in rotation (the weights are not L2-resident); the
down projection has no fragment kernel and reads the dequantised arena in every form -- it is the control.  Then the whole step: ms
per step of a 64-chain greedy burst (captured graphs) on the MXFP4 engine, knob 0 against knob 1 in alternating runs.  Every figure
is the median of `--repeats` measurements with the spread (min .. max).  Synthetic weights; needs the GPU; nothing is read from disk.

    python tools/bench_gemm4.py [--model 3b|7b|both] [--out profiles/mxfp4_batched.txt]"""
import argparse
import os
import statistics
import sys
import time

import torch

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))

from zoomearth_amd.config import ModelConfig   # noqa: E402
from zoomearth_amd.engine import Engine        # noqa: E402

KINDS = ("qkv", "o", "gate_up", "down", "lm_head")
FORMS = (("bf16(dq)", "mxfp4", 1), ("fp8", "fp8", 0), ("mxfp4", "mxfp4", 0))   # label, weight format, knob 24


def step_ms(e, seqs, tokens):
    """ms per step of one greedy burst of `tokens` tokens for the prefilled chains `seqs`"""
    ids = list(range(100, 132))
    for s in seqs:
        e.seq_reset(s)
        e.prefill(s, ids, None, *e.rope_index(ids, []), want_logits=False)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    toks = e.generate_batch(seqs, tokens, ignore_eos=True)
    torch.cuda.synchronize()
    assert all(len(t) == tokens for t in toks)
    return (time.perf_counter() - t0) * 1e3 / (tokens - 1)   # (the first token comes from the prefill's logits)


def run(model, args, lines):
    cfg = ModelConfig.zoomearth_3b() if model == "3b" else ModelConfig.qwen25vl_7b()
    e = Engine(cfg, device=0, max_seqs=64, max_ctx=512, max_patches=64, max_tile_side=64)
    e.set_decode_regime(0)
    t = cfg.text
    lines.append(f"batched decode weight forms, {model} shape (hidden {t.hidden_size}, intermediate {t.intermediate_size}, "
                 f"{t.num_hidden_layers} layers, lm_head {'tied: bf16 in every form' if t.tie_word_embeddings else 'untied'}); "
                 f"median of {args.repeats} x {args.iters} launches (min .. max)")
    seqs = list(range(64))
    ids = list(range(100, 132))
    try:
        for label, fmt, knob in FORMS:
            e.fill_synthetic(seed=0, std=0.02)        # (a weight write returns the engine to bf16)
            e.set_weight_format(fmt)
            e.lib.ze_tune(24, knob)
            for s in seqs:
                e.seq_reset(s)
                e.prefill(s, ids, None, *e.rope_index(ids, []), want_logits=False)
            for n in (16, 64):
                for which, kind in enumerate(KINDS):
                    if kind == "lm_head" and t.tie_word_embeddings:
                        continue
                    e.profile_batch_kernel(which, n, 36)  # warm-up: instruction cache, clocks
                    us = [e.profile_batch_kernel(which, n, args.iters)[0] for _ in range(args.repeats)]
                    lines.append(f"{model} {label:<9} {kind:<8} {n:3d} rows {statistics.median(us):8.2f} us ({min(us):.2f} .. {max(us):.2f})")
            lines.append(f"{model} {label:<9} fragment copies: {e.fragment_bytes() / 2 ** 20:9.1f} MiB")
        # the whole step, MXFP4 engine (the last form): knob 0 against knob 1, alternating
        ms = {0: [], 1: []}
        for rep in range(args.repeats):
            for knob in (0, 1):
                e.lib.ze_tune(24, knob)
                step_ms(e, seqs, 8)                    # the switch rebuilds the copies and re-captures the step
                ms[knob].append(step_ms(e, seqs, args.tokens))
        for knob, name in ((1, "bf16(dq) fragments (knob 24 = 1)"), (0, "mxfp4 fragments (knob 24 = 0)")):
            v = ms[knob]
            lines.append(f"{model} 64-chain burst, {args.tokens} tokens, {name}: {statistics.median(v):7.3f} ms/step ({min(v):.3f} .. {max(v):.3f}), "
                         f"{64e3 / statistics.median(v):8.0f} tokens/s")
    finally:
        e.lib.ze_tune(24, 0)
        e.close()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--model", default="both", choices=["3b", "7b", "both"])
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--iters", type=int, default=144)
    ap.add_argument("--tokens", type=int, default=64)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    lines = []
    for model in (("3b", "7b") if args.model == "both" else (args.model,)):
        run(model, args, lines)
    text = "\n".join(lines)
    print(text)
    if args.out:
        with open(args.out, "a", encoding="utf-8") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
