"""Rollout scoring of a GRPO step on the 3B shape (synthetic weights): 8 samples x G = 8 sequences of about 1 500 tokens whose
first ~800 are the sample's prompt with one image, scored from the prompt's end, three ways in one process:
  (a) the per-chain loop: one `Engine.score` per sequence through slot 0, then the slice from the prompt's end
  (b) `model.score_sequences(items, share_prefix=False)`: many sequences per `ze_score_batch` pass, scored rows only
  (c) `model.score_sequences(items, share_prefix=True)`: the G generations of a sample also share their prompt's rows
Five timed repetitions each after one warm-up; medians, spreads (min .. max), rows per pass and rows saved by sharing go to
stdout and, with --out, to a file.  --loop-only times (a) alone (it needs nothing but `Engine.score`)."""
import argparse
import os
import statistics
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch  # noqa: E402

from zoomearth_amd.config import ModelConfig  # noqa: E402
from zoomearth_amd.engine import Engine  # noqa: E402
from zoomearth_amd.synth import uniform_ints  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--samples", type=int, default=8)
ap.add_argument("--generations", type=int, default=8)
ap.add_argument("--reps", type=int, default=5)
ap.add_argument("--max-seqs", type=int, default=16)
ap.add_argument("--max-prefill-rows", type=int, default=12800)
ap.add_argument("--loop-only", action="store_true")
ap.add_argument("--out", default=None)
args = ap.parse_args()

cfg = ModelConfig.zoomearth_3b()
e = Engine(cfg, max_seqs=args.max_seqs, max_ctx=2048, max_patches=2048, max_tile_side=1024, max_prefill_rows=args.max_prefill_rows)
e.fill_synthetic(0)
grid = [1, 52, 52]                                   # 676 merged rows: a 728 x 728 view
n_img = grid[1] * grid[2] // 4
seqs = []                                            # (ids, features, key, prompt length)
gen = torch.Generator().manual_seed(0)
for s in range(args.samples):
    feat = (torch.randn(n_img, cfg.text.hidden_size, generator=gen) * 0.5).to(torch.bfloat16).to(e.device)
    prompt = (uniform_ints(100 + s, 60, 1000, 150000).tolist() + [cfg.vision_start_token_id] + [cfg.image_token_id] * n_img +
              [cfg.vision_end_token_id] + uniform_ints(200 + s, 62, 1000, 150000).tolist())
    for g in range(args.generations):
        tail = uniform_ints(1000 + 16 * s + g, 650 + 13 * ((3 * g + s) % 8), 1000, 150000).tolist()
        seqs.append((prompt + tail, feat, ("view", s), len(prompt)))
rows_total = sum(len(q[0]) for q in seqs)
scored_total = sum(len(q[0]) - q[3] for q in seqs)


def loop():
    out = []
    for ids, feat, _, n_prompt in seqs:
        pos, delta = e.rope_index(ids, [grid])
        e.seq_reset(0)
        out.append(e.score(0, ids, feat, pos, delta)[n_prompt - 1:])
    return out


def timed(fn):
    fn()
    torch.cuda.synchronize()
    ts, res = [], None
    for _ in range(args.reps):
        t0 = time.perf_counter()
        res = fn()
        torch.cuda.synchronize()
        ts.append(1e3 * (time.perf_counter() - t0))
    return ts, res


def line(name, ts, extra=""):
    return (f"{name}: median {statistics.median(ts):.1f} ms, spread {min(ts):.1f} .. {max(ts):.1f} ms over {len(ts)} repetitions"
            f" ({1e3 * rows_total / statistics.median(ts):.0f} sequence rows/s){extra}")


lines = [f"3B shape, synthetic weights: {args.samples} samples x G = {args.generations} = {len(seqs)} sequences, {rows_total} rows "
         f"({min(len(q[0]) for q in seqs)} .. {max(len(q[0]) for q in seqs)} per sequence), prompt {seqs[0][3]} rows with one image of {n_img} rows, "
         f"{scored_total} scored rows; max_seqs {args.max_seqs}, max_prefill_rows {args.max_prefill_rows}"]
ta, ra = timed(loop)
lines.append(line("(a) per-chain Engine.score loop", ta, f"; {len(seqs)} passes of about {rows_total // len(seqs)} rows, "
                                                         f"{rows_total - len(seqs)} rows through the lm_head"))
if not args.loop_only:
    from zoomearth_amd.modeling import ScoreItem, ZoomEarthForConditionalGeneration

    model = ZoomEarthForConditionalGeneration(cfg, e)
    items = [ScoreItem(ids, [grid], [feat], [key], n_prompt - 1) for ids, feat, key, n_prompt in seqs]
    for name, share in (("(b) score_sequences, no sharing", False), ("(c) score_sequences, shared prefixes", True)):
        ts, res = timed(lambda: model.score_sequences(items, share_prefix=share))
        st = model.last_score_stats
        same = all(torch.equal(x, y) for x, y in zip(res, ra))
        lines.append(line(name, ts, f"; {st['passes']} passes of {st['rows_per_pass']} rows, {st['scored_rows']} rows through the "
                                    f"lm_head, {st['shared_rows']} rows copied instead of prefilled; bit-equal to (a): {same}"))
        lines.append(f"    speed-up over (a): {statistics.median(ta) / statistics.median(ts):.2f}x "
                     f"(spread of (a): {max(ta) - min(ta):.1f} ms; gain {statistics.median(ta) - statistics.median(ts):.1f} ms)")
e.close()
print("\n".join(lines))
if args.out:
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w", encoding="utf-8") as f:
        f.write("\n".join(lines) + "\n")
