"""Times the batch-1 decode projections for the three weight streams -- bf16, FP8 and MXFP4 -- in ONE process on one box: per
projection (qkv, o, gate/up, down, lm_head) through ze_profile_decode_kernel, which launches the step's own kernels with the step's own
arguments over the layers in rotation, and a whole-path figure: tokens/s of a 128-token batch-1 greedy run (captured decode graph) on
synthetic weights.  Every figure is the median of `--repeats` measurements with the spread (min .. max) beside it; us per launch and
TB/s of the stream's OWN bytes (bf16 2 B, FP8 1 B + 4 B per row, MXFP4 0.5 B + 1 B per 32 weights).  `--knob 1=2` style settings pass
ze_tune knobs through for A/B runs (knob 1 = 2: one row pair per wave in the many-row FP8 / MXFP4 kernels).  Reduced-precision modes
are opt-in and never the headline configuration.  Needs the GPU; nothing is read from disk.

    python tools/bench_gemv4.py [--model 3b|7b] [--out profiles/mxfp4_gemv.txt]"""
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


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--model", default="3b", choices=["3b", "7b"])
    ap.add_argument("--repeats", type=int, default=7)
    ap.add_argument("--iters", type=int, default=144)
    ap.add_argument("--tokens", type=int, default=128)
    ap.add_argument("--knob", action="append", default=[], help="K=V: ze_tune(K, V) before measuring")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    cfg = ModelConfig.zoomearth_3b() if args.model == "3b" else ModelConfig.qwen25vl_7b()
    e = Engine(cfg, device=0, max_seqs=1, max_ctx=1024, max_patches=1024, max_tile_side=1024)
    for kv in args.knob:
        k, v = kv.split("=")
        e.lib.ze_tune(int(k), int(v))
    t = cfg.text
    lines = [f"decode weight streams, {args.model} shape (hidden {t.hidden_size}, intermediate {t.intermediate_size}, {t.num_hidden_layers} layers), "
             f"knobs {args.knob or 'default'}; median of {args.repeats} x {args.iters} launches (min .. max)"]
    ids = list(range(100, 164))
    for fmt in ("bf16", "fp8", "mxfp4"):
        e.fill_synthetic(seed=0, std=0.02)        # (a weight write returns the engine to bf16)
        e.set_weight_format(fmt)
        assert e.weight_format == fmt
        for which, kind in enumerate(KINDS):
            e.profile_decode_kernel(which, 36)      # warm-up: instruction cache, clocks
            us, by = zip(*[e.profile_decode_kernel(which, args.iters) for _ in range(args.repeats)])
            med = statistics.median(us)
            lines.append(f"{fmt:<6} {kind:<8} {med:8.2f} us ({min(us):.2f} .. {max(us):.2f})  {by[0] / 1e6:8.2f} MB  {by[0] / med / 1e6:6.3f} TB/s "
                         f"= {by[0] / med / 1e6 / 8 * 100:5.1f} % of 8 TB/s")
        rates = []
        for rep in range(args.repeats + 1):
            e.seq_reset(0)
            e.prefill(0, ids, None, *e.rope_index(ids, []), want_logits=True)
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            toks = e.generate(0, args.tokens, ignore_eos=True)
            torch.cuda.synchronize()
            dt = time.perf_counter() - t0
            if rep:                                 # (the first run captures the graph)
                rates.append(len(toks) / dt)
        lines.append(f"{fmt:<6} greedy {args.tokens} tokens, batch 1: {statistics.median(rates):8.1f} tokens/s ({min(rates):.1f} .. {max(rates):.1f})")
    e.close()
    text = "\n".join(lines)
    print(text)
    if args.out:
        with open(args.out, "a", encoding="utf-8") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
