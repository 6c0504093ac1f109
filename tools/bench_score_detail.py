"""Cost of what a scored position reports beyond its log-probability (zoomearth_amd/csrc/ze_score_detail.hip) on one engine.
  kernel   k_score_detail per launch (Engine.op_score_detail) at 1 / 64 / 512 rows of 151,936 bf16 logits with top_n 0 and 20, beside
           k_token_logprob (Engine.op_token_logprob) on the same rows: median and spread (min .. max) of the event times of --reps
           launches after a warm-up, one CSV row each (--csv), with the worst entropy error against float64 over the first rows
  pass     a whole scoring call on the 3B shape with the workload of tools/bench_score_batch.py (8 samples x G = 8 sequences, scored
           from the prompt's end): model.score_sequences(items) against score_sequences(items, top_n=20, entropy=True, rank=True),
           medians and spreads to stdout and --out."""
import argparse
import os
import statistics
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np  # noqa: E402
import torch  # noqa: E402

from zoomearth_amd.config import ModelConfig  # noqa: E402
from zoomearth_amd.engine import Engine  # noqa: E402
from zoomearth_amd.synth import uniform_ints  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--reps", type=int, default=20)
ap.add_argument("--pass-reps", type=int, default=5)
ap.add_argument("--samples", type=int, default=8)
ap.add_argument("--generations", type=int, default=8)
ap.add_argument("--skip-pass", action="store_true")
ap.add_argument("--csv", default=None)
ap.add_argument("--out", default=None)
args = ap.parse_args()

VOCAB = 151936
cfg = ModelConfig.zoomearth_3b()
e = Engine(cfg, max_seqs=16, max_ctx=2048, max_patches=2048, max_tile_side=1024, max_prefill_rows=12800)
e.fill_synthetic(0)


def event_times(fn, reps):
    fn()
    torch.cuda.synchronize()
    ts = []
    for _ in range(reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        b.synchronize()
        ts.append(1e3 * a.elapsed_time(b))
    return ts


rows_csv = ["kernel,rows,top_n,median_us,min_us,max_us,us_per_row,reps"]
lines = []
gen = torch.Generator(device="cuda").manual_seed(0)
for rows in (1, 64, 512):
    lg = (torch.randn((rows, VOCAB), generator=gen, device="cuda") * 2.5).to(torch.bfloat16)
    tg = torch.randint(0, VOCAB, (rows,), generator=gen, device="cuda", dtype=torch.int32)
    for name, n, fn in (("k_token_logprob", 0, lambda: e.op_token_logprob(lg, tg)),
                        ("k_score_detail", 0, lambda: e.op_score_detail(lg, tg, 0)),
                        ("k_score_detail", 20, lambda: e.op_score_detail(lg, tg, 20))):
        ts = event_times(fn, args.reps)
        med = statistics.median(ts)
        rows_csv.append(f"{name},{rows},{n},{med:.1f},{min(ts):.1f},{max(ts):.1f},{med / rows:.2f},{len(ts)}")
        lines.append(f"{name} rows {rows} top_n {n}: median {med:.1f} us, spread {min(ts):.1f} .. {max(ts):.1f} us ({med / rows:.2f} us/row)")
    if rows == 64:   # the entropy against float64 on the same bf16 rows
        d = e.op_score_detail(lg, tg, 0)
        z = lg[:8].double().cpu().numpy()
        z = z - z.max(1, keepdims=True)
        logp = z - np.log(np.exp(z).sum(1, keepdims=True))
        ent = -(np.exp(logp) * logp).sum(1)
        err = float(np.abs(d.entropy[:8].cpu().numpy() - ent).max())
        rows_csv.append(f"# max |entropy - float64| over 8 rows of {VOCAB} logits (entropies {ent.min():.3f} .. {ent.max():.3f}): {err:.3e}")
        lines.append(rows_csv[-1][2:])

if not args.skip_pass:
    from zoomearth_amd.modeling import ScoreItem, ZoomEarthForConditionalGeneration

    grid = [1, 52, 52]
    n_img = grid[1] * grid[2] // 4
    seqs = []
    cgen = torch.Generator().manual_seed(0)
    for s in range(args.samples):
        feat = (torch.randn(n_img, cfg.text.hidden_size, generator=cgen) * 0.5).to(torch.bfloat16).to(e.device)
        prompt = (uniform_ints(100 + s, 60, 1000, 150000).tolist() + [cfg.vision_start_token_id] + [cfg.image_token_id] * n_img +
                  [cfg.vision_end_token_id] + uniform_ints(200 + s, 62, 1000, 150000).tolist())
        for g in range(args.generations):
            tail = uniform_ints(1000 + 16 * s + g, 650 + 13 * ((3 * g + s) % 8), 1000, 150000).tolist()
            seqs.append((prompt + tail, feat, ("view", s), len(prompt)))
    model = ZoomEarthForConditionalGeneration(cfg, e)
    items = [ScoreItem(ids, [grid], [feat], [key], n_prompt - 1) for ids, feat, key, n_prompt in seqs]

    def timed(fn):
        fn()
        torch.cuda.synchronize()
        ts, res = [], None
        for _ in range(args.pass_reps):
            t0 = time.perf_counter()
            res = fn()
            torch.cuda.synchronize()
            ts.append(1e3 * (time.perf_counter() - t0))
        return ts, res

    ta, ra = timed(lambda: model.score_sequences(items))
    scored = model.last_score_stats["scored_rows"]
    tb, rb = timed(lambda: model.score_sequences(items, top_n=20, entropy=True, rank=True))
    same = all(torch.equal(x, y.logps) for x, y in zip(ra, rb))
    lines.append(f"3B shape, {len(seqs)} sequences, {scored} scored rows, shared prefixes:")
    lines.append(f"  score_sequences (k_token_logprob): median {statistics.median(ta):.1f} ms, spread {min(ta):.1f} .. {max(ta):.1f} ms over {len(ta)} repetitions")
    lines.append(f"  score_sequences(top_n=20, entropy, rank) (k_score_detail): median {statistics.median(tb):.1f} ms, spread {min(tb):.1f} .. "
                 f"{max(tb):.1f} ms; +{statistics.median(tb) - statistics.median(ta):.1f} ms = {statistics.median(tb) / statistics.median(ta):.3f}x; "
                 f"logps bit-equal: {same}")
e.close()
print("\n".join(lines))
for path, content in ((args.csv, rows_csv), (args.out, lines)):
    if path:
        os.makedirs(os.path.dirname(os.path.abspath(path)), exist_ok=True)
        with open(path, "w", encoding="utf-8") as f:
            f.write("\n".join(content) + "\n")
