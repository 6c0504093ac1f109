"""Cost of the log-probabilities of generated tokens (zoomearth_amd/csrc/ze_logprobs.hip) on one engine.

  --kernel   k_token_logprobs alone through Engine.op_token_logprobs on `--chains` rows of 151,936 fp32 logits, top_n 0 / 5 / 20,
             on `randn x 4` rows and on stream-like rows (the logits of a real batched decode step of a two-layer engine with the
             3B head structure and the full vocabulary, repeated to the row count): HIP-event time per call (which includes
             the gaps the host leaves between launches); run the same command under
             `rocprofv3 --kernel-trace --stats -- python tools/bench_logprobs.py --kernel ...` for the per-launch figure
  (default)  the batched decode step of that engine with nobody asking, every chain asking for top_n, nobody again:
             HIP-event time per step of ze_decode_burst, same chains, same process

One JSON line per measurement; "floor" = rows x vocab x 4 B at the 8 TB/s HBM peak (one pass over the rows).
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
HBM_BYTES_PER_S = 8.0e12   # MI355X HBM3E peak


def heads_engine(chains):
    cfg = ModelConfig.heads()   # the 3B model's head structure at depth 2, with the full vocabulary
    cfg = dataclasses.replace(cfg, text=dataclasses.replace(cfg.text, vocab_size=VOCAB))
    e = Engine(cfg, device=0, max_seqs=chains, max_ctx=max(256, chains), max_patches=1024, max_tile_side=1024)
    e.fill_synthetic(seed=1, std=0.02, matrix_gain=4.0, bias_std=0.02, norm_jitter=0.1)
    return e


def prefill_all(e, slots):
    ids = list(range(10, 42))
    pos, delta = e.rope_index(ids, [])
    for s in slots:
        e.seq_reset(s)
        e.prefill(s, [i + s % 7 for i in ids], None, pos, delta, want_logits=False)


def bench_kernel(e, kind, lg, iters):
    rows = lg.shape[0]
    tg = torch.randint(0, VOCAB, (rows,), dtype=torch.int32, device="cuda")
    floor = rows * VOCAB * 4 / HBM_BYTES_PER_S * 1e6
    for n in (0, 5, 20):
        for _ in range(3):
            e.op_token_logprobs(lg, tg, n)
        torch.cuda.synchronize()
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        for _ in range(iters):
            e.op_token_logprobs(lg, tg, n)
        b.record()
        torch.cuda.synchronize()
        us = a.elapsed_time(b) * 1e3 / iters
        print(json.dumps(dict(what="kernel", rows=rows, logits=kind, top_n=n, event_us_per_call=round(us, 1),
                              floor_us=round(floor, 1), floor_fraction=round(floor / us, 3))), flush=True)


def bench_step(chains, steps, top_n):
    e = heads_engine(chains)
    try:
        slots = list(range(chains))
        for label, n in (("nobody", None), (f"all_top_{top_n}", top_n), ("nobody_again", None)):
            prefill_all(e, slots)
            if n is not None:
                for s in slots:
                    e.set_logprobs(s, n)
            params = e.gen_params(ignore_eos=True, use_graph=True)
            for i, s in enumerate(slots):
                e.chain_begin(s, params, i)
            e.decode_burst(slots, 4, params)   # capture + warm
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            e.decode_burst_begin(slots, steps, params)
            b.record()
            e.decode_burst_end(slots)
            print(json.dumps(dict(what="step", chains=chains, variant=label, us_per_step=round(a.elapsed_time(b) * 1e3 / steps, 1))),
                  flush=True)
    finally:
        e.close()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--kernel", action="store_true")
    ap.add_argument("--chains", type=int, nargs="+", default=[64, 490])
    ap.add_argument("--iters", type=int, default=50)
    ap.add_argument("--steps", type=int, default=32)
    ap.add_argument("--top-n", type=int, default=20)
    args = ap.parse_args()
    if args.kernel:
        e = heads_engine(64)
        try:
            slots = list(range(64))
            prefill_all(e, slots)
            e.decode_batch(slots, [11 + s for s in slots], want_logits=False)
            real = e.decode_batch(slots, [50 + 3 * s for s in slots])   # one real step's rows: [64, vocab] fp32
            for n in args.chains:
                stream_like = real.repeat((n + 63) // 64, 1)[:n].contiguous()
                bench_kernel(e, "decode_step", stream_like, args.iters)
                bench_kernel(e, "randn_x4", (torch.randn((n, VOCAB), device="cuda") * 4.0).float(), args.iters)
        finally:
            e.close()
    else:
        for n in args.chains:
            bench_step(n, args.steps, args.top_n)


if __name__ == "__main__":
    main()
