"""Admission of G identical prompts on one engine: the shared-prefix way against the fork (zoomearth_amd/csrc/ze_fork.hip).

The 3B layer shape with synthetic weights, text prompts of 802 and 1320 rows (a stage-1 and a stage-2 prompt of the zoom chain),
G in {4, 8, 16} completions:

  (a) "shared prefix": what a scheduler does for G requests of one prompt without the fork -- one whole prefill, then G - 1 times
      ze_seq_copy_prefix of all rows but one, then ONE batched pass of the G - 1 one-row tails.  Written against calls every commit
      since the shared prefixes has, so the same tool measures a tree without ze_seq_fork (it then prints (a) alone).
  (b) "fork": one whole prefill, then one ze_seq_fork to G - 1 slots.
  and the copies alone: the G - 1 ze_seq_copy_prefix calls, and the one ze_seq_fork call, without the prefill or the tails.

HIP events on the stream, --warmup untimed repeats, then --repeats timed ones each between its own pair of events; min and median
are printed (the measuring guide: a minimum for what the GPU can do, a median for what a caller sees).  One JSON line per
measurement.  "copy_rate_TBps" of a copy = bytes read + written / its minimum time: the fork reads the rows once and writes them to
its G - 1 destinations ((1 + G - 1) x the chain's bytes), the prefix copies read and write them G - 1 times each; next to it the
rate a float4 copy streams at on an MI355X, 6.29 TB/s (measured; 79 % of the 8 TB/s HBM3E peak).
"""
import argparse
import json
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from zoomearth_amd.config import ModelConfig  # noqa: E402
from zoomearth_amd.engine import Engine  # noqa: E402

MEASURED_COPY_TBPS = 6.29


def timed(fn, setup, warmup, repeats):
    """ms per call of fn(), each call behind an untimed setup() and between its own pair of events"""
    out = []
    for i in range(warmup + repeats):
        setup()
        torch.cuda.synchronize()
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        torch.cuda.synchronize()
        if i >= warmup:
            out.append(a.elapsed_time(b))
    return min(out), statistics.median(out)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", type=int, nargs="*", default=[802, 1320])
    ap.add_argument("--G", type=int, nargs="*", default=[4, 8, 16])
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--repeats", type=int, default=10)
    ap.add_argument("--tiny", action="store_true", help="the parity-fixture shape instead of the 3B one (a smoke run)")
    a = ap.parse_args()
    cfg = ModelConfig.tiny() if a.tiny else ModelConfig.zoomearth_3b()
    e = Engine(cfg, device=0, max_seqs=max(a.G) + 1, max_ctx=max(a.rows) + 8, max_patches=1024, max_tile_side=1024)
    e.fill_synthetic(seed=1, std=0.02)
    t = cfg.text
    has_fork = hasattr(e, "seq_fork")
    row_bytes = t.num_hidden_layers * t.num_key_value_heads * 2 * (t.hidden_size // t.num_attention_heads) * 2   # K and V, bf16
    g = torch.Generator().manual_seed(7)
    try:
        for L in a.rows:
            ids = torch.randint(10, min(t.vocab_size, 100000), (L,), generator=g).tolist()
            pos, delta = e.rope_index(ids, [])

            def whole():
                e.seq_reset(0)
                e.prefill(0, ids, None, pos, delta, want_logits=False)

            for G in a.G:
                dsts = list(range(1, G))

                def copies():
                    for d in dsts:
                        e.seq_copy_prefix(d, 0, L - 1)

                def tails():
                    e.prefill_batch(dsts, [ids[-1:]] * (G - 1), [None] * (G - 1), [pos[:, -1:]] * (G - 1), [delta] * (G - 1))

                def shared():
                    whole()
                    copies()
                    tails()

                def fork():
                    e.seq_fork(0, dsts)

                def forked():
                    whole()
                    fork()

                def say(what, ms, moved=None):
                    rec = dict(op=what, rows=L, G=G, ms_min=round(ms[0], 4), ms_median=round(ms[1], 4))
                    if moved is not None:
                        rec.update(copy_rate_TBps=round(moved / (ms[0] * 1e-3) / 1e12, 3), measured_float4_copy_TBps=MEASURED_COPY_TBPS)
                    print(json.dumps(rec), flush=True)

                say("a_shared_prefix_admission", timed(shared, lambda: None, a.warmup, a.repeats))
                say("a_copy_prefix_calls_alone", timed(copies, whole, a.warmup, a.repeats), 2 * (G - 1) * (L - 1) * row_bytes)
                if has_fork:
                    say("b_fork_admission", timed(forked, lambda: None, a.warmup, a.repeats))
                    extra = (t.vocab_size * 5) * G                       # the logits row (f32) and the seen-set (u8), read once, written G - 1 times
                    say("b_fork_call_alone", timed(fork, whole, a.warmup, a.repeats), G * L * row_bytes + extra)
    finally:
        e.close()


if __name__ == "__main__":
    main()
