"""Speculative decoding by prompt lookup at batch 1 on the 3B shape (synthetic weights): tokens/s of a greedy run of `--tokens` tokens
  (a) on the single-chain GEMV family (Engine.generate, captured decode graph), as today;
  (b) through family-0 bursts without speculation (one row per step);
  (c) family 0 with k = 2 and (d) with k = 4, each on two scripted id streams: HIGH -- the lookup text handed to set_speculation
      holds the run's own continuation, so every draft hits (what a stage-2 prompt that restates stage 1's text looks like to the
      drafter) -- and ZERO -- an empty lookup text and 8-grams only, so nothing is ever drafted and every step pays k + 1 rows for one
      token;
with the mean accepted draft ids per step, the family-0 step time at 1, 3, 5 and 9 rows (k = 0, 2, 4, 8 on the HIGH stream: wall time
of the bursts / steps taken) and the break-even: (step time at k + 1 rows) / (GEMV step time) tokens per step are needed for the
speculative form to draw level with (a).  Every figure is the median of `--repeats` runs with the spread beside it.  Needs the GPU.

    python tools/bench_speculative.py [--tokens 128] [--repeats 5] [--out profiles/speculative.txt]

With `--temperature T` (> 0; `--top-p P` optional) the run measures the SAMPLED mode instead (set_speculation(sampled=True)): the plain
sampled family-0 step at 1 row, the sampled-mode step at k + 1 rows on the HIGH and ZERO streams for k = 2, 4, 8, the greedy-mode step
(k_spec_accept, the code of the commit before the sampled mode) at the same k on a greedy chain, what the sampled accept pass costs
over it, and the break-even accepted ids per step against the plain sampled step.

    python tools/bench_speculative.py --temperature 0.7 --top-p 0.9 [--out profiles/speculative_sampled.txt]"""
import argparse
import os
import statistics
import sys
import time

import torch

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))

from zoomearth_amd.config import ModelConfig   # noqa: E402
from zoomearth_amd.engine import Engine        # noqa: E402


def sampled_report(e, cfg, args, ids, n, timed):
    """The sampled mode at batch 1: see the module docstring."""
    T, top_p, seed = args.temperature, args.top_p, 11

    def bursts(k, lookup, sampled, temperature, gmin=1, gmax=3):
        def run():
            if top_p < 1.0 and temperature > 0:
                e.set_sampling_filter(0, top_p=top_p)
            if k:
                e.set_speculation(0, k, lookup, gmin, gmax, sampled=sampled)
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            toks = e.generate_speculative([0], n, ignore_eos=True, burst=16, do_sample=temperature > 0, temperature=temperature or 1.0, seed=seed)[0]
            dt = time.perf_counter() - t0
            st = e.spec_stats(0)
            return toks, dt, st[0] if k else n - 1, st
        return run

    def step_ms(runs):
        return statistics.median(r[1] / max(r[2], 1) * 1e3 for r in runs)

    def spread(runs):
        v = [r[1] / max(r[2], 1) * 1e3 for r in runs]
        return f"{statistics.median(v):6.3f} ms / step ({min(v):.3f} .. {max(v):.3f})"

    t = cfg.text
    lines = [f"speculative decoding by prompt lookup, SAMPLED mode, batch 1, 3B shape (hidden {t.hidden_size}, {t.num_hidden_layers} layers), bf16 "
             f"weights, T = {T}, top_p = {top_p}, {n} tokens after a {len(ids)}-id prompt; median of {args.repeats} runs (min .. max); wall time of "
             "the bursts / steps taken, host loop included"]
    plain = timed(bursts(0, [], False, T))
    ref = plain[0][0]
    plain_ms = step_ms(plain)
    lines.append(f"plain sampled family-0 step, 1 row            {spread(plain)}")
    gplain = timed(bursts(0, [], False, 0.0))
    gref = gplain[0][0]
    lines.append(f"plain greedy family-0 step, 1 row             {spread(gplain)}")
    for k in (2, 4, 8):
        hi = timed(bursts(k, ids + ref, True, T))
        zero = timed(bursts(k, [], True, T, 8, 8))
        ghi = timed(bursts(k, ids + gref, False, 0.0))
        same = all(r[0] == ref for r in hi + zero) and all(r[0] == gref for r in ghi)
        st = hi[-1][3]
        cost = step_ms(hi) - step_ms(ghi)
        lines.append(f"k = {k} ({k + 1} rows): sampled mode HIGH {spread(hi)}  accepted / step {st[2] / max(st[0], 1):.2f};  ZERO {spread(zero)};  "
                     f"greedy mode HIGH {spread(ghi)};  sampled accept over greedy accept {cost * 1e3:+.0f} us "
                     f"({100 * cost / step_ms(hi):+.1f} % of the step);  break-even accepted ids / step against the plain sampled step "
                     f"{step_ms(hi) / plain_ms - 1:.2f};  {'ids == the plain runs' if same else 'IDS DIFFER FROM THE PLAIN RUNS'}")
    return "\n".join(lines)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--tokens", type=int, default=128)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--out", default=None)
    ap.add_argument("--temperature", type=float, default=0.0, help="> 0: measure the sampled mode at this temperature")
    ap.add_argument("--top-p", type=float, default=1.0, help="with --temperature: the chain's top-p filter (1 = none)")
    ap.add_argument("--append", action="store_true", help="append to --out instead of replacing it")
    args = ap.parse_args()
    cfg = ModelConfig.zoomearth_3b()
    e = Engine(cfg, device=0, max_seqs=1, max_ctx=1024, max_patches=1024, max_tile_side=1024)
    e.fill_synthetic(seed=0, std=0.02)
    e.set_decode_regime(0)
    ids = list(range(100, 164))
    n = args.tokens

    def prefill():
        e.seq_reset(0)
        e.prefill(0, ids, None, *e.rope_index(ids, []), want_logits=False)

    def timed(run):
        out = []
        for rep in range(args.repeats + 1):
            prefill()
            res = run()
            if rep:   # (the first run warms up: graph capture, instruction cache, clocks)
                out.append(res)
        return out

    def gemv():
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        toks = e.generate(0, n, ignore_eos=True)
        return toks, time.perf_counter() - t0, n - 1, (0, 0, 0)

    def bursts(k, lookup, gmin=1, gmax=3):
        def run():
            if k:
                e.set_speculation(0, k, lookup, gmin, gmax)
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            toks = e.generate_speculative([0], n, ignore_eos=True, burst=16)[0]
            dt = time.perf_counter() - t0
            st = e.spec_stats(0)
            return toks, dt, st[0] if k else n - 1, st
        return run

    def line(name, runs, ref=None):
        rate = [len(r[0]) / r[1] for r in runs]
        step_ms = statistics.median(r[1] / max(r[2], 1) * 1e3 for r in runs)
        st = runs[-1][3]
        same = "" if ref is None else ("  ids == (b)" if all(r[0] == ref for r in runs) else "  IDS DIFFER FROM (b)")
        acc = f"  steps {st[0]} drafted {st[1]} accepted {st[2]}  mean accepted / step {st[2] / max(st[0], 1):.2f}" if st[0] else ""
        return (f"{name:<34} {statistics.median(rate):8.1f} tokens/s ({min(rate):.1f} .. {max(rate):.1f})  {step_ms:6.3f} ms / step{acc}{same}",
                statistics.median(rate), step_ms)

    if args.temperature > 0:
        text = sampled_report(e, cfg, args, ids, n, timed)
        print(text)
        if args.out:
            with open(args.out, "a" if args.append else "w") as f:
                f.write(text + "\n")
        e.close()
        return

    t = cfg.text
    lines = [f"speculative decoding by prompt lookup, batch 1, 3B shape (hidden {t.hidden_size}, {t.num_hidden_layers} layers), bf16 weights, "
             f"{n} tokens after a {len(ids)}-id prompt; median of {args.repeats} runs (min .. max); wall time, host loop included"]
    a_runs = timed(gemv)
    la, a_rate, a_step = line("(a) GEMV family, as today", a_runs)
    b_runs = timed(bursts(0, []))
    ref = b_runs[0][0]
    lb, b_rate, b_step = line("(b) family 0, no speculation", b_runs)
    lines += [la, lb, f"    (a) and (b) emit the same ids for the first {next((i for i, (x, y) in enumerate(zip(a_runs[0][0], ref)) if x != y), n)} of {n} tokens "
                      "(the two families agree within bf16 rounding, not bit for bit)"]
    rates, steps = {}, {1: b_step}
    for k in (2, 4, 8):
        hi = timed(bursts(k, ids + ref))
        lh, r_hi, s_hi = line(f"({'c' if k == 2 else 'd' if k == 4 else '-'}) family 0, k = {k}, HIGH hit stream", hi, ref)
        steps[k + 1] = s_hi
        lines.append(lh)
        rates[(k, "high")] = r_hi
        if k != 8:
            zero = timed(bursts(k, [], 8, 8))
            lz, r_z, _ = line(f"({'c' if k == 2 else 'd'}) family 0, k = {k}, ZERO hit stream", zero, ref)
            lines.append(lz)
            rates[(k, "zero")] = r_z
    lines.append("family-0 step time by rows (bursts' wall time / steps): " + ", ".join(f"{r} rows {steps[r]:.3f} ms" for r in sorted(steps)))
    lines.append(f"GEMV step {a_step:.3f} ms; break-even tokens per step = step(k + 1 rows) / GEMV step: " +
                 ", ".join(f"k = {r - 1}: {steps[r] / a_step:.2f}" for r in sorted(steps) if r > 1))
    lines.append(f"(d) on the HIGH stream {'beats' if rates[(4, 'high')] > a_rate else 'does not beat'} (a): {rates[(4, 'high')]:.1f} against {a_rate:.1f} tokens/s; "
                 f"on the ZERO stream {rates[(4, 'zero')]:.1f}")
    text = "\n".join(lines)
    print(text)
    if args.out:
        with open(args.out, "w") as f:
            f.write(text + "\n")
    e.close()


if __name__ == "__main__":
    main()
