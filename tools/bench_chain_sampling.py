"""Cost of the per-chain sampling requests (ze_seq_set_sampling; the per-chain kernels of zoomearth_amd/csrc/ze_sample.hip) on one engine.

The batched decode step of a two-layer engine (3B head structure) with the full vocabulary, HIP-event time per step of
ze_decode_burst under a captured graph, same chains, same process, in four settings:

  uniform_sampled   no request anywhere, the call's params sampled: the scalar kernels -- what the step launched before this entry
  no_request        no request anywhere, the call's params greedy (the scalar arg-max alone)
  all_sampled       the call's params greedy, every chain with a sampled request of its own (temperature 0.7, its own seed)
  half_half         the call's params greedy, even chains sampled, odd chains with a greedy request

The steps differ in their sampling stage alone; its kernels' own times come from
`rocprofv3 --kernel-trace --stats -- python tools/bench_chain_sampling.py ...` (k_argmax_partial_batch / _chain,
k_softmax_partial / _chain, k_multinomial_pick / _chain, k_argmax_final_batch).

One JSON line per measurement.
"""
import argparse
import dataclasses
import json
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from zoomearth_amd.config import ModelConfig  # noqa: E402
from zoomearth_amd.engine import Engine  # noqa: E402

VOCAB = 151936
T = 0.7
VARIANTS = ("uniform_sampled", "no_request", "all_sampled", "half_half", "uniform_sampled_again")


def bench_step(chains, steps, repeats):
    cfg = ModelConfig.heads()   # the 3B model's head structure at depth 2, with the full vocabulary
    cfg = dataclasses.replace(cfg, text=dataclasses.replace(cfg.text, vocab_size=VOCAB))
    e = Engine(cfg, device=0, max_seqs=chains, max_ctx=max(256, chains), max_patches=1024, max_tile_side=1024)
    try:
        e.fill_synthetic(seed=1, std=0.02, matrix_gain=4.0, bias_std=0.02, norm_jitter=0.1)
        ids = list(range(10, 42))
        pos, delta = e.rope_index(ids, [])
        slots = list(range(chains))
        for label in VARIANTS:
            for s in slots:
                e.seq_reset(s)
                e.prefill(s, ids, None, pos, delta, want_logits=False)
                if label == "all_sampled" or (label == "half_half" and s % 2 == 0):
                    e.set_sampling(s, do_sample=True, temperature=T, seed=100 + s)
                elif label == "half_half":
                    e.set_sampling(s, do_sample=False)
            sampled = label.startswith("uniform_sampled")
            params = e.gen_params(ignore_eos=True, do_sample=sampled, temperature=T, seed=3, use_graph=True)
            for i, s in enumerate(slots):
                e.chain_begin(s, params, i)
            e.decode_burst(slots, 4, params)   # capture + warm
            times = []
            for _ in range(repeats):
                a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                a.record()
                e.decode_burst_begin(slots, steps, params)
                b.record()
                e.decode_burst_end(slots)
                times.append(round(a.elapsed_time(b) * 1e3 / steps, 1))
            print(json.dumps(dict(what="step", chains=chains, variant=label, us_per_step=times)), flush=True)
    finally:
        e.close()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--chains", type=int, nargs="+", default=[64, 512])
    ap.add_argument("--steps", type=int, default=16)
    ap.add_argument("--repeats", type=int, default=3)
    args = ap.parse_args()
    for n in args.chains:
        bench_step(n, args.steps, args.repeats)


if __name__ == "__main__":
    main()
