"""Cost of the per-chain token rules (zoomearth_amd/csrc/ze_token_rules.hip) on one engine.

ze_op_token_rules on 64 and 490 rows with a 1500-id history each (the stream's prompt plus generation; the last 300 ids count as
generated), its arguments prepared on the device once, in three variants: no_repeat_ngram_size = 3 alone, 8 ban records alone,
and n-gram + ban records + 4 stop records.  The logits are 4096 columns wide, so the row copy the op makes in front of the ban
pass (it is not part of the pass: in a decode step the adjusted copy exists already) stays small against the passes; the
HIP-event time per call covers copy + ban pass + stop pass and the gaps the host leaves between the three launches.  Run the same
command under `rocprofv3 --kernel-trace --stats -- python tools/bench_token_rules.py ...` for the per-launch figures of
k_token_ban and k_token_stop.

One JSON line per measurement; "floor" = the bytes the passes must touch (4 B per history id, the packed records, one flag)
at the 8 TB/s HBM peak -- microseconds of launch latency stand against nanoseconds of traffic, so the figure says how far a
latency-bound pass is from mattering, not how well it streams.
"""
import argparse
import ctypes as C
import json
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from zoomearth_amd.config import ModelConfig  # noqa: E402
from zoomearth_amd.engine import Engine, pack_records  # noqa: E402

VOCAB, HIST, GENERATED = 4096, 1500, 300
HBM_BYTES_PER_S = 8.0e12   # MI355X HBM3E peak


def ptr(t):
    return C.c_void_p(t.data_ptr())


def flat(lists, rows):
    off = np.zeros(rows + 1, dtype=np.int32)
    off[1:] = np.cumsum([len(x) for x in lists])
    return torch.from_numpy(np.concatenate(list(lists) + [np.zeros(4, np.int32)]).astype(np.int32)).cuda(), torch.from_numpy(off).cuda()


def bench(e, rows, iters):
    rng = np.random.default_rng(rows)
    lg = (torch.randn((rows, VOCAB), device="cuda") * 4.0).float()
    out = torch.empty_like(lg)
    hit = torch.zeros(rows, dtype=torch.int32, device="cuda")
    hists = [rng.integers(0, VOCAB, size=HIST).astype(np.int32) for _ in range(rows)]
    hist, hoff = flat(hists, rows)
    nctx = torch.full((rows,), HIST - GENERATED, dtype=torch.int32, device="cuda")
    zeros = torch.zeros(rows, dtype=torch.int32, device="cuda")
    none = [np.zeros(0, np.int32)] * rows
    bans = [pack_records([list(h[-3:]) + [7], [11]] + [rng.integers(0, VOCAB, size=4).tolist() for _ in range(6)]) for h in hists]
    stops = [pack_records([rng.integers(0, VOCAB, size=3).tolist() for _ in range(4)]) for _ in range(rows)]
    variants = (("ngram_3", zeros + 3, none, none), ("bans_8", zeros, bans, none), ("ngram_bans_stops", zeros + 3, bans, stops))
    for name, ngram, ban, stop in variants:
        bd, boff = flat(ban, rows)
        sd, soff = flat(stop, rows)
        touched = rows * (HIST * 4 * (2 if int(ngram[0]) else 0) / 2 + 4) + int(boff[-1]) * 4 + int(soff[-1]) * 4
        floor = touched / HBM_BYTES_PER_S * 1e6

        def call():
            e._check(e.lib.ze_op_token_rules(e.h, ptr(lg), rows, VOCAB, VOCAB, ptr(hist), ptr(hoff), ptr(nctx), ptr(ngram), ptr(bd),
                                             ptr(boff), ptr(sd), ptr(soff), ptr(zeros), ptr(out), ptr(hit), e._stream()))

        for _ in range(5):
            call()
        torch.cuda.synchronize()
        t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        t0.record()
        for _ in range(iters):
            call()
        t1.record()
        torch.cuda.synchronize()
        us = t0.elapsed_time(t1) * 1e3 / iters
        print(json.dumps(dict(op="token_rules", rows=rows, history=HIST, variant=name, us_per_call=round(us, 2),
                              floor_us=round(floor, 4), banned_per_row=int(torch.isinf(out).sum().item()) // rows)), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--chains", type=int, nargs="*", default=[64, 490])
    ap.add_argument("--iters", type=int, default=50)
    a = ap.parse_args()
    e = Engine(ModelConfig.tiny(), device=0, max_seqs=1, max_ctx=512, max_patches=1024, max_tile_side=1024)
    try:
        for rows in a.chains:
            bench(e, rows, a.iters)
    finally:
        e.close()


if __name__ == "__main__":
    main()
