"""Cost of the entropy filters (typical / epsilon / eta; zoomearth_amd/csrc/ze_sample_band.hip) on one engine.

  --kernel   the two selections through Engine.sample_band on `--chains` rows of 151,936 fp32 logits: each stage alone, all
             three on, every one behind top_p = 0.95 so k_sample_filter runs next to k_sample_band (run under `rocprofv3
             --kernel-trace --stats -- python tools/bench_entropy_filters.py --kernel` for the per-launch figures; the wall
             time printed here includes the op's table upload and its wait)
  --plain    a chain-sampling burst on the tiny decoder with no filter of any kind set: under `rocprofv3 --kernel-trace --stats`
             its kernel-call table is the parent's
  (default)  the sampled batched decode step of the tiny decoder, `--chains` chains, with and without the filters on its chains:
             HIP-event time per step of ze_decode_burst, same chains, same process

One JSON line per measurement.
"""
import argparse
import json
import os
import sys
import time

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from zoomearth_amd.config import ModelConfig  # noqa: E402
from zoomearth_amd.engine import Engine  # noqa: E402

VOCAB = 151936
STAGES = [("typical", dict(typical_p=0.9)), ("epsilon", dict(epsilon_cutoff=3e-4)), ("eta", dict(eta_cutoff=2e-3)),
          ("all", dict(typical_p=0.9, epsilon_cutoff=3e-4, eta_cutoff=2e-3)), ("none", dict())]


def bench_kernel(e, chains, iters, only=None):
    lg = (torch.randn((chains, VOCAB), device="cuda") * 3.0).float()
    for name, kw in STAGES:
        if only not in (None, name):
            continue
        e.sample_band(lg, 1.0, top_p=0.95, **kw)
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for _ in range(iters):
            cut, ceil, kept = e.sample_band(lg, 1.0, top_p=0.95, **kw)
        torch.cuda.synchronize()
        print(json.dumps(dict(what="kernel", chains=chains, stage=name, iters=iters,
                              wall_us_per_call=round((time.perf_counter() - t0) / iters * 1e6, 1), kept_mean=float(kept.float().mean()))))


def bench_step(chains, steps, plain_only=False):
    e = Engine(ModelConfig.tiny(), device=0, max_seqs=chains, max_ctx=256, max_patches=1024, max_tile_side=1024)
    try:
        e.fill_synthetic(seed=1, std=0.02, matrix_gain=4.0, bias_std=0.02, norm_jitter=0.1)
        ids = list(range(10, 42))
        pos, delta = e.rope_index(ids, [])
        slots = list(range(chains))
        variants = [("no_filter", None)] if plain_only else [("no_filter", None)] + [(n, kw) for n, kw in STAGES[:4]] + [("no_filter_again", None)]
        for label, kw in variants:
            for s in slots:
                e.seq_reset(s)
                e.prefill(s, ids, None, pos, delta, want_logits=False)
                if kw:
                    e.set_entropy_filter(s, **kw)
            params = e.gen_params(ignore_eos=True, do_sample=True, temperature=0.9, seed=3, use_graph=True)
            for i, s in enumerate(slots):
                e.chain_begin(s, params, i)
            e.decode_burst(slots, 4, params)   # capture + warm
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            e.decode_burst_begin(slots, steps, params)
            b.record()
            e.decode_burst_end(slots)
            print(json.dumps(dict(what="step", chains=chains, variant=label, us_per_step=round(a.elapsed_time(b) * 1e3 / steps, 1))))
    finally:
        e.close()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--kernel", action="store_true")
    ap.add_argument("--plain", action="store_true")
    ap.add_argument("--stage", choices=[n for n, _ in STAGES], default=None, help="--kernel: this stage only (one profiler run each)")
    ap.add_argument("--chains", type=int, default=64)
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--steps", type=int, default=32)
    args = ap.parse_args()
    if args.kernel:
        e = Engine(ModelConfig.tiny(), device=0, max_seqs=1, max_ctx=64, max_patches=1024, max_tile_side=1024)
        try:
            bench_kernel(e, args.chains, args.iters, args.stage)
        finally:
            e.close()
    else:
        bench_step(args.chains, args.steps, plain_only=args.plain)


if __name__ == "__main__":
    main()
