"""Cost of a beam-search step (zoomearth_amd/csrc/ze_beam.hip) at the 3B shape, vocabulary 151,936, on one engine.

Per shape -- `--beams` B (default 4) beams, `--groups` in {1, 8, 16} prompts -- HIP-event microseconds per launch of k_beam_rows, k_beam_select and
k_beam_reorder (ze_profile_beam_kernel; the reorder at its widest: every slot but a group's first takes 96 generated K/V rows of every
layer from the group's first slot), the bytes each launch moves, and next to them the time of a plain greedy batched decode step of the
same row count on the same engine (HIP events around a captured burst, as tools/bench_entropy_filters.py times its steps).

One JSON line per measurement; `--out FILE` also writes them there."""
import argparse
import ctypes as C
import json
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from zoomearth_amd.config import ModelConfig  # noqa: E402
from zoomearth_amd.engine import Engine  # noqa: E402

GEN_ROWS = 96
KERNELS = ("k_beam_rows", "k_beam_select", "k_beam_reorder")


def kernel_us(e, which, groups, B, logits, iters):
    out = C.c_float()
    e._check(e.lib.ze_profile_beam_kernel(e.h, which, groups, B, GEN_ROWS, C.c_void_p(logits.data_ptr()), iters, C.byref(out), e._stream()))
    return float(out.value)


def bytes_moved(cfg, groups, B):
    t = cfg.text
    n, vocab = groups * B, t.vocab_size
    row_kv = t.num_hidden_layers * t.num_key_value_heads * 2 * (t.hidden_size // t.num_attention_heads) * 2   # K and V, bf16
    moving = groups * (B - 1)
    return {"k_beam_rows": n * vocab * 4,                                  # the fp32 logits row, streamed from HBM once (later passes: L2)
            "k_beam_select": n * (B + len(cfg.eos_token_ids)) * 8,        # the candidate table
            # read + write: K/V rows and the seen-set (the measured call has run one step: no ids or beam indices to move yet)
            "k_beam_reorder": moving * 2 * (GEN_ROWS * row_kv + vocab)}


def greedy_step_us(e, rows, steps):
    ids = list(range(10, 42))
    pos, delta = e.rope_index(ids, [])
    slots = list(range(rows))
    for s in slots:
        e.seq_reset(s)
        e.prefill(s, ids, None, pos, delta, want_logits=False)
    params = e.gen_params(ignore_eos=True, use_graph=True)
    for i, s in enumerate(slots):
        e.chain_begin(s, params, i)
    e.decode_burst(slots, 4, params)   # capture + warm
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    e.decode_burst_begin(slots, steps, params)
    b.record()
    e.decode_burst_end(slots)
    return a.elapsed_time(b) * 1e3 / steps


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--groups", type=int, nargs="*", default=[1, 8, 16])
    ap.add_argument("--beams", type=int, nargs="*", default=[4], help="beam widths; groups * beams <= 64 (decode family 0)")
    ap.add_argument("--iters", type=int, default=50)
    ap.add_argument("--steps", type=int, default=32)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    cfg = ModelConfig()
    shapes = [(g, B) for B in args.beams for g in args.groups if g * B <= 64]
    e = Engine(cfg, device=0, max_seqs=max(g * B for g, B in shapes), max_ctx=512, max_patches=1024, max_tile_side=1024)
    lines = []
    try:
        e.fill_synthetic(seed=1, std=0.02, matrix_gain=4.0, bias_std=0.02, norm_jitter=0.1)
        e.set_decode_regime(0)
        for groups, B in shapes:
            n = groups * B
            logits = (torch.randn((n, cfg.text.vocab_size), device="cuda") * 3.0).to(torch.bfloat16).float().contiguous()
            greedy = greedy_step_us(e, n, args.steps)
            moved = bytes_moved(cfg, groups, B)
            for which, name in enumerate(KERNELS):
                us = kernel_us(e, which, groups, B, logits, args.iters)
                lines.append(dict(what="beam_kernel", kernel=name, num_beams=B, groups=groups, rows=n, generated_rows=GEN_ROWS,
                                  us_per_launch=round(us, 2), bytes_moved=moved[name], gb_per_s=round(moved[name] / us / 1e3, 1),
                                  greedy_step_us_same_rows=round(greedy, 1)))
                print(json.dumps(lines[-1]), flush=True)
    finally:
        e.close()
    if args.out:
        with open(args.out, "w", encoding="utf-8") as f:
            for ln in lines:
                f.write(json.dumps(ln) + "\n")


if __name__ == "__main__":
    main()
