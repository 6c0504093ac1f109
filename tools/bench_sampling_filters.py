"""Cost of the sampling filters (top-k / top-p / min-p; zoomearth_amd/csrc/ze_sample_filter.hip) on one engine.

  --kernel   the selection kernel alone through Engine.sample_filter on `--chains` rows of 151,936 fp32 logits
             (run under `rocprofv3 --kernel-trace --stats -- python tools/bench_sampling_filters.py --kernel ...` for the
             per-launch figure; the wall time printed here includes the op's table upload and its wait)
  (default)  the sampled batched decode step of a two-layer engine (3B head structure) with the full vocabulary, with and without a filter
             on its chains: HIP-event time per step of ze_decode_burst, same chains, same process

One JSON line per measurement.
"""
import argparse
import dataclasses
import json
import os
import sys
import time

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from zoomearth_amd.config import ModelConfig  # noqa: E402
from zoomearth_amd.engine import Engine  # noqa: E402

VOCAB = 151936
HBM_BYTES_PER_S = 8.0e12   # MI355X HBM3E peak


def bench_kernel(e, chains, iters, setting):
    t, k, p, m = setting
    lg = (torch.randn((chains, VOCAB), device="cuda") * 3.0).float()
    e.sample_filter(lg, t, k, p, m)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(iters):
        cut, kept = e.sample_filter(lg, t, k, p, m)
    torch.cuda.synchronize()
    wall_us = (time.perf_counter() - t0) / iters * 1e6
    passes = 2 + (k > 0 or p < 1.0) + 2 * (k > 0) + 2 * (p < 1.0)   # max, level 1, two per select, survivors
    print(json.dumps(dict(what="kernel", chains=chains, setting=setting, wall_us_per_call=round(wall_us, 1), passes=passes,
                          one_pass_floor_us=round(chains * VOCAB * 4 / HBM_BYTES_PER_S * 1e6, 1),
                          kept_mean=float(kept.float().mean()))))


def bench_step(chains, steps, setting):
    cfg = ModelConfig.heads()   # the 3B model's head structure at depth 2, with the full vocabulary
    cfg = dataclasses.replace(cfg, text=dataclasses.replace(cfg.text, vocab_size=VOCAB))
    e = Engine(cfg, device=0, max_seqs=chains, max_ctx=max(256, chains), max_patches=1024, max_tile_side=1024)
    try:
        e.fill_synthetic(seed=1, std=0.02, matrix_gain=4.0, bias_std=0.02, norm_jitter=0.1)
        ids = list(range(10, 42))
        pos, delta = e.rope_index(ids, [])
        slots = list(range(chains))
        t, k, p, m = setting
        for label, filt in (("no_filter", None), ("filter", (k, p, m)), ("no_filter_again", None)):
            for s in slots:
                e.seq_reset(s)
                e.prefill(s, ids, None, pos, delta, want_logits=False)
                if filt:
                    e.set_sampling_filter(s, *filt)
            params = e.gen_params(ignore_eos=True, do_sample=True, temperature=t, seed=3, use_graph=True)
            for i, s in enumerate(slots):
                e.chain_begin(s, params, i)
            e.decode_burst(slots, 4, params)   # capture + warm
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            e.decode_burst_begin(slots, steps, params)
            b.record()
            e.decode_burst_end(slots)
            print(json.dumps(dict(what="step", chains=chains, setting=setting, variant=label,
                                  us_per_step=round(a.elapsed_time(b) * 1e3 / steps, 1))))
    finally:
        e.close()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--kernel", action="store_true")
    ap.add_argument("--chains", type=int, nargs="+", default=[64, 490])
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--steps", type=int, default=32)
    ap.add_argument("--setting", type=float, nargs=4, default=[0.7, 50, 0.95, 0.0], metavar=("T", "K", "P", "MINP"))
    args = ap.parse_args()
    setting = (args.setting[0], int(args.setting[1]), args.setting[2], args.setting[3])
    if args.kernel:
        e = Engine(ModelConfig.tiny(), device=0, max_seqs=1, max_ctx=64, max_patches=1024, max_tile_side=1024)
        try:
            for n in args.chains:
                for s in (setting, (1.0, 50, 1.0, 0.0), (1.0, 0, 0.9, 0.0), (1.0, 0, 1.0, 0.05)):
                    bench_kernel(e, n, args.iters, s)
        finally:
            e.close()
    else:
        for n in args.chains:
            bench_step(n, args.steps, setting)


if __name__ == "__main__":
    main()
