"""The prefix cache measured: its two kernels against the copies they stand beside, and a server-style request stream with and
without the pool (zoomearth_amd/csrc/ze_prefix.hip, zoomearth_amd/prefix_cache.py).

Kernels (3B layer shape, synthetic weights; 347 rows = the system turn and a view's image tokens, 1053 = a stage-1 prompt with its
reply): `ze_prefix_save`, `ze_prefix_load` to 1 and to 10 slots, next to `ze_seq_copy_prefix` (1 slot) and `ze_seq_fork` (1 and 10
slots) of the same rows.  HIP events, --warmup untimed calls, --repeats timed ones each between its own pair of events, and the
whole series --series times over (the run-to-run noise); one JSON line per measurement and series.  A load to one slot moves the
bytes ze_seq_copy_prefix moves; the fork also copies a logits row and a seen-set (vocab * 5 bytes per slot).

Flow: --tiles tiles of --questions questions each; the questions of a tile share their first --shared ids (of --prompt).  Every
question is TWO requests, as an HTTP client sends them -- stage 1, then stage 2 = stage-1 prompt + its reply + a tail, submitted only
once stage 1 has finished -- and the questions of a tile follow one another, never together.  The same stream runs through
`ChainScheduler(prefix_cache_rows=0)` and through one with a pool; questions/s, prefill rows and hit rows of both are printed.  Text
prompts with ids as words, so the reply's re-tokenisation is the identity (the upper bound for generated-row reuse).
"""
import argparse
import json
import os
import statistics
import sys
import time

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from zoomearth_amd.config import ModelConfig  # noqa: E402
from zoomearth_amd.engine import Engine  # noqa: E402


def timed(fn, setup, warmup, repeats):
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


def kernels(a, cfg):
    t = cfg.text
    block = a.block_rows
    e = Engine(cfg, device=0, max_seqs=12, max_ctx=max(a.rows) + 2 * block, max_patches=1024, max_tile_side=1024)
    e.fill_synthetic(seed=1, std=0.02)
    row_bytes = t.num_hidden_layers * t.num_key_value_heads * 2 * (t.hidden_size // t.num_attention_heads) * 2
    g = torch.Generator().manual_seed(7)
    e.prefix_pool_create((max(a.rows) + block - 1) // block + 1, block)
    try:
        for L in a.rows:
            nb = (L + block - 1) // block
            ids = torch.randint(10, min(t.vocab_size, 100000), (nb * block,), generator=g).tolist()
            pos, delta = e.rope_index(ids, [])
            e.seq_reset(0)
            e.prefill(0, ids, None, pos, delta, want_logits=False)
            blocks = list(range(nb))[::-1]
            e.prefix_save(0, 0, blocks)
            ten = list(range(1, 11))
            ops = [("copy_prefix_1", lambda: e.seq_copy_prefix(1, 0, L), 2 * L * row_bytes),
                   ("fork_1", lambda: e.seq_fork(0, [1]), 2 * nb * block * row_bytes),
                   ("fork_10", lambda: e.seq_fork(0, ten), 11 * nb * block * row_bytes),
                   ("prefix_save", lambda: e.prefix_save(0, 0, blocks), 2 * nb * block * row_bytes),
                   ("prefix_load_1", lambda: e.prefix_load(blocks, L, 0, [1]), 2 * L * row_bytes),
                   ("prefix_load_10", lambda: e.prefix_load(blocks, L, 0, ten), 11 * L * row_bytes)]
            for series in range(a.series):
                for name, fn, moved in ops:
                    lo, med = timed(fn, lambda: None, a.warmup, a.repeats)
                    print(json.dumps(dict(part="kernels", op=name, rows=L if "fork" not in name and name != "prefix_save" else nb * block,
                                          series=series, ms_min=round(lo, 4), ms_median=round(med, 4),
                                          rate_TBps=round(moved / (lo * 1e-3) / 1e12, 3))), flush=True)
    finally:
        e.close()


class IdTokenizer:
    def __init__(self, banned):
        self.banned = banned

    def decode(self, ids, skip_special_tokens=True):
        return " ".join(str(11 if int(i) in self.banned else int(i)) for i in ids)   # (no image block may appear in a text prompt)


class IdProcessor:
    """text -> ids: one id per whitespace word (text prompts only)"""

    def __init__(self, banned):
        self.tokenizer = IdTokenizer(banned)

    def __call__(self, text, images=None, return_tensors="pt", **kw):
        return dict(input_ids=torch.tensor([[int(w) for w in text[0].split()]]))


def flow(a, cfg):
    from zoomearth_amd.modeling import ZoomEarthForConditionalGeneration
    from zoomearth_amd.scheduler import ChainScheduler, Request
    ctx = a.prompt + 2 * a.new_tokens + 64
    model = ZoomEarthForConditionalGeneration.from_synthetic(cfg, seed=1, std=0.02, max_seqs=4, max_ctx=ctx, max_patches=1024,
                                                            max_tile_side=1024)
    g = torch.Generator().manual_seed(11)
    hi = min(cfg.text.vocab_size, 100000)
    banned = {cfg.image_token_id, cfg.vision_start_token_id, cfg.vision_end_token_id}
    rnd = lambda n: [int(v) for v in torch.randint(10, hi, (n,), generator=g) if int(v) not in banned]   # noqa: E731
    stream = []
    for _ in range(a.tiles):
        shared = rnd(a.shared)
        stream += [" ".join(map(str, shared + rnd(a.prompt - a.shared))) for _ in range(a.questions)]
    tail = " ".join(map(str, rnd(40)))
    try:
        for rows in (0, a.pool_rows):
            sched = ChainScheduler(model, IdProcessor(banned), do_sample=False, burst=8, ignore_eos=True, prefix_cache_rows=rows,
                                   prefix_cache_block_rows=a.block_rows)
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            for p1 in stream:
                r1 = Request(prompt=p1, images=[], max_new_tokens=a.new_tokens)
                sched.submit(r1)
                sched.run()
                sched.submit(Request(prompt=p1 + " " + r1.text + " " + tail, images=[], max_new_tokens=a.new_tokens))
                sched.run()
            torch.cuda.synchronize()
            dt = time.perf_counter() - t0
            print(json.dumps(dict(part="flow", prefix_cache_rows=rows, questions=len(stream), seconds=round(dt, 3),
                                  questions_per_s=round(len(stream) / dt, 3), prefill_rows=sched.stats["prefill_rows"],
                                  hit_rows=sched.stats.get("prefix_cache_hit_rows", 0),
                                  saved_rows=sched.stats.get("prefix_cache_saved_rows", 0),
                                  evicted_blocks=sched.stats.get("prefix_cache_evicted_blocks", 0))), flush=True)
            sched.close()
    finally:
        model.engine.close()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--part", choices=["kernels", "flow", "both"], default="both")
    ap.add_argument("--rows", type=int, nargs="*", default=[347, 1053])
    ap.add_argument("--block-rows", type=int, default=32)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--repeats", type=int, default=10)
    ap.add_argument("--series", type=int, default=3)
    ap.add_argument("--tiles", type=int, default=3)
    ap.add_argument("--questions", type=int, default=10)
    ap.add_argument("--prompt", type=int, default=802)
    ap.add_argument("--shared", type=int, default=347)
    ap.add_argument("--new-tokens", type=int, default=48)
    ap.add_argument("--pool-rows", type=int, default=65536)
    ap.add_argument("--tiny", action="store_true", help="the parity-fixture shape instead of the 3B one (a smoke run)")
    a = ap.parse_args()
    cfg = ModelConfig.tiny() if a.tiny else ModelConfig.zoomearth_3b()
    if a.part in ("kernels", "both"):
        kernels(a, cfg)
    if a.part in ("flow", "both"):
        flow(a, cfg)


if __name__ == "__main__":
    main()
