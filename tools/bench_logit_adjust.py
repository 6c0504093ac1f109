"""Cost of the per-chain logit adjustments (zoomearth_amd/csrc/ze_logit_adjust.hip) on one engine.

  --kernel   k_logit_adjust alone through ze_op_logit_adjust on `--chains` rows of 151,936 fp32 logits (randn x 4), its arguments
             prepared on the device once, in three variants: a 1-entry bias and no penalties (rows + copy), penalties over a
             count table, a 300-entry bias per row.  HIP-event time per call (which includes the gaps the host leaves between
             launches); run the same command under `rocprofv3 --kernel-trace --stats -- python tools/bench_logit_adjust.py
             --kernel ...` for the per-launch figure
  (default)  the batched decode step of a two-layer engine with the 3B head structure and the full vocabulary with nobody
             asking, every chain carrying a request (penalties + 5 biases), nobody again: HIP-event time per step of
             ze_decode_burst, same chains, same process

One JSON line per measurement; "floor" = bytes read + bytes written (4 + 4 B per element, + 2 B with counts) at the 8 TB/s
HBM peak.
"""
import argparse
import ctypes as C
import dataclasses
import json
import os
import sys

import numpy as np
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


def ptr(t):
    return C.c_void_p(t.data_ptr()) if t is not None else None


def bench_kernel(e, rows, iters):
    rng = np.random.default_rng(rows)
    lg = (torch.randn((rows, VOCAB), device="cuda") * 4.0).float()
    out = torch.empty_like(lg)
    counts = torch.from_numpy(rng.integers(0, 4, size=(rows, VOCAB), dtype=np.int16)).cuda()
    zeros_f = torch.zeros(rows, dtype=torch.float32, device="cuda")
    zeros_i = torch.zeros(rows, dtype=torch.int32, device="cuda")

    def lists(n):
        ids = np.stack([rng.choice(VOCAB, size=n, replace=False) for _ in range(rows)]).astype(np.int32)
        return (torch.arange(0, (rows + 1) * n, n, dtype=torch.int32, device="cuda"), torch.from_numpy(ids.reshape(-1)).cuda(),
                torch.from_numpy(rng.uniform(-5, 5, size=rows * n).astype(np.float32)).cuda())

    variants = (("no_penalties", None, zeros_f, zeros_f, lists(1), 8),
                ("penalties", counts, zeros_f + 0.5, zeros_f + 0.7, lists(1), 10),
                ("bias_300", None, zeros_f, zeros_f, lists(300), 8))
    for name, cnt, pr, fr, (off, ids, vals), bytes_per in variants:
        floor = rows * VOCAB * bytes_per / HBM_BYTES_PER_S * 1e6

        def call():
            e._check(e.lib.ze_op_logit_adjust(e.h, ptr(lg), rows, VOCAB, VOCAB, ptr(cnt), ptr(pr), ptr(fr), ptr(zeros_i), ptr(off),
                                              ptr(ids), ptr(vals), ptr(out), e._stream()))
        for _ in range(3):
            call()
        torch.cuda.synchronize()
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        for _ in range(iters):
            call()
        b.record()
        torch.cuda.synchronize()
        us = a.elapsed_time(b) * 1e3 / iters
        print(json.dumps(dict(what="kernel", rows=rows, variant=name, event_us_per_call=round(us, 1), floor_us=round(floor, 1),
                              floor_fraction=round(floor / us, 3))), flush=True)


def bench_step(chains, steps):
    e = heads_engine(chains)
    try:
        slots = list(range(chains))
        for label, on in (("nobody", False), ("all_chains", True), ("nobody_again", False)):
            prefill_all(e, slots)
            if on:
                for s in slots:
                    e.seq_set_logit_adjust(s, 0.5, 0.7, 0, {20 + s: 3.0, 700: -4.0, 1500: float("-inf"), 0: 1.5, 2047: -2.5})
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
    args = ap.parse_args()
    if args.kernel:
        e = Engine(ModelConfig.tiny(), device=0, max_seqs=1, max_ctx=256, max_patches=1024, max_tile_side=1024)
        try:
            for n in args.chains:
                bench_kernel(e, n, args.iters)
        finally:
            e.close()
    else:
        for n in args.chains:
            bench_step(n, args.steps)


if __name__ == "__main__":
    main()
