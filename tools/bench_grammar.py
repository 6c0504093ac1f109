"""Cost of guided decoding (zoomearth_amd/csrc/ze_grammar.hip) on one engine, at the real vocabulary (151,936).

ze_op_grammar_mask and ze_op_grammar_advance on 1, 64 and 512 rows under a grammar whose states allow about 1 % of the ids each
(the realistic case, and the worst case for the mask's stores), and ze_op_logit_adjust -- k_logit_adjust, the kernel the mask
pass follows in a step -- on the same rows in the same process.  The HIP-event time of the mask op covers the row copy the op
makes in front of the pass (it is not part of the pass: in a decode step the adjusted copy exists already); run the same command
under `rocprofv3 --kernel-trace --stats -- python tools/bench_grammar.py ...` for the per-launch figures of k_grammar_mask,
k_grammar_advance and k_logit_adjust, which are the ones to compare.  Then the step time of a 64-chain decode burst (a tiny
decoder under the real vocabulary, so that the lm_head and the sampler have their real width) with every chain guided and with
none.

One JSON line per measurement; "floor" = the bytes a pass must touch at the 8 TB/s HBM peak: the mask stores a row and loads its
bits (4 B + 1/8 B per id), the adjust kernel loads and stores a row (8 B per id).
"""
import argparse
import ctypes as C
import copy
import json
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from zoomearth_amd.config import ModelConfig  # noqa: E402
from zoomearth_amd.engine import Engine  # noqa: E402
from zoomearth_amd.grammar import TokenAutomaton  # noqa: E402

VOCAB, EOS = 151936, (151645, 151643)
N_STATES, N_CLASSES = 64, 100    # one class in a hundred allowed per state: about 1 % of the ids
HBM_BYTES_PER_S = 8.0e12         # MI355X HBM3E peak


def ptr(t):
    return C.c_void_p(t.data_ptr())


def automaton(seed=0) -> TokenAutomaton:
    rng = np.random.default_rng(seed)
    tc = rng.integers(0, N_CLASSES, VOCAB).astype(np.uint16)
    trans = np.full((N_STATES, N_CLASSES), -1, np.int16)
    for s in range(N_STATES):
        trans[s, rng.integers(0, N_CLASSES)] = (s + 1) % N_STATES
    return TokenAutomaton(tc, trans, (np.arange(N_STATES) % 8 == 0).astype(np.uint8))


def timed(call, iters):
    for _ in range(5):
        call()
    torch.cuda.synchronize()
    t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    t0.record()
    for _ in range(iters):
        call()
    t1.record()
    torch.cuda.synchronize()
    return t0.elapsed_time(t1) * 1e3 / iters


def bench_ops(e, gid, rows, iters):
    rng = np.random.default_rng(rows)
    lg = torch.randn((rows, VOCAB), device="cuda").float()
    out = torch.empty_like(lg)
    states = torch.from_numpy(rng.integers(0, N_STATES, rows).astype(np.int32)).cuda()
    tokens = torch.from_numpy(rng.integers(0, VOCAB, rows).astype(np.int32)).cuda()
    nxt = torch.empty(rows, dtype=torch.int32, device="cuda")
    zf = torch.zeros(rows, dtype=torch.float32, device="cuda")
    pres = torch.full((rows,), 0.5, dtype=torch.float32, device="cuda")   # a request: the kernel computes, it does not just copy
    zi = torch.zeros(rows + 1, dtype=torch.int32, device="cuda")
    s = e._stream()

    def mask():
        e._check(e.lib.ze_op_grammar_mask(e.h, gid, ptr(lg), rows, VOCAB, VOCAB, ptr(states), ptr(out), s))

    def advance():
        e._check(e.lib.ze_op_grammar_advance(e.h, gid, ptr(states), ptr(tokens), rows, ptr(nxt), s))

    def adjust():
        e._check(e.lib.ze_op_logit_adjust(e.h, ptr(lg), rows, VOCAB, VOCAB, None, ptr(pres), ptr(zf), ptr(zi), ptr(zi), ptr(zi), ptr(zf),
                                          ptr(out), s))

    floors = dict(grammar_mask_with_row_copy=rows * VOCAB * (4 + 1 / 8), grammar_advance=rows * 16, logit_adjust=rows * VOCAB * 8)
    for name, call in (("grammar_mask_with_row_copy", mask), ("grammar_advance", advance), ("logit_adjust", adjust)):
        us = timed(call, iters)
        print(json.dumps(dict(op=name, rows=rows, vocab=VOCAB, us_per_call=round(us, 2),
                              floor_us=round(floors[name] / HBM_BYTES_PER_S * 1e6, 3))), flush=True)
    mask()
    torch.cuda.synchronize()
    print(json.dumps(dict(op="allowed_share", rows=rows, share=round(float(torch.isfinite(out).float().mean().item()), 4))), flush=True)


def bench_burst(e, gid, chains, steps):
    params = e.gen_params(ignore_eos=True)
    ids = list(range(10, 26))
    pos, delta = e.rope_index(ids, [])
    slots = list(range(chains))
    for guided in (False, True, False, True):
        for s in slots:
            e.seq_reset(s)
            e.prefill(s, ids, None, pos, delta, want_logits=True)
            if guided:
                e.set_grammar(s, gid, s % N_STATES)
            e.chain_begin(s, params)
        e.decode_burst(slots, 4, params)   # (captures the step on first use)
        torch.cuda.synchronize()
        t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        t0.record()
        e.decode_burst(slots, steps, params)
        t1.record()
        torch.cuda.synchronize()
        print(json.dumps(dict(op="burst_step", chains=chains, guided=guided, us_per_step=round(t0.elapsed_time(t1) * 1e3 / steps, 2))),
              flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", type=int, nargs="*", default=[1, 64, 512])
    ap.add_argument("--iters", type=int, default=50)
    ap.add_argument("--burst-chains", type=int, default=64)
    ap.add_argument("--burst-steps", type=int, default=64)
    a = ap.parse_args()
    cfg = copy.deepcopy(ModelConfig.tiny())
    cfg.text.vocab_size, cfg.eos_token_ids, cfg.pad_token_id = VOCAB, EOS, EOS[1]
    e = Engine(cfg, device=0, max_seqs=max(a.burst_chains, 1), max_ctx=256, max_patches=1024, max_tile_side=1024)
    try:
        e.fill_synthetic(seed=1, std=0.02, matrix_gain=4.0)
        gid = e.grammar_create(automaton())
        for rows in a.rows:
            bench_ops(e, gid, rows, a.iters)
        if a.burst_chains > 0:
            bench_burst(e, gid, a.burst_chains, a.burst_steps)
    finally:
        e.close()


if __name__ == "__main__":
    main()
