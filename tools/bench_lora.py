"""Times LoRA adapter switches at the 3B shape (ze_lora_activate): base -> adapter, adapter -> adapter, adapter -> base, for an r = 8 and
an r = 64 adapter over the seven decoder projections of every layer, and the achieved bytes/s of the merge pass against the 8 TB/s HBM
figure; beside it, the refresh without adapters: ze_load_weight of the same tensors from host memory (a LOWER bound on a
load_state_dict of the merged checkpoint, which loads every other tensor too).  Needs the GPU; synthetic weights, nothing read from disk.

    python tools/bench_lora.py [--out profiles/lora_merge.txt]"""
import argparse
import os
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))

from zoomearth_amd.config import ModelConfig   # noqa: E402
from zoomearth_amd.engine import Engine        # noqa: E402

PROJ = ("self_attn.q_proj", "self_attn.k_proj", "self_attn.v_proj", "self_attn.o_proj", "mlp.gate_proj", "mlp.up_proj", "mlp.down_proj")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    cfg = ModelConfig.zoomearth_3b()
    e = Engine(cfg, device=0, max_seqs=1, max_ctx=512, max_patches=1024, max_tile_side=1024)
    e.fill_synthetic(seed=0, std=0.02)
    names = [f"model.language_model.layers.{i}.{p}.weight" for i in range(cfg.text.num_hidden_layers) for p in PROJ]
    shapes = {n: e.weight_shape(n)[:2] for n in names}
    elems = sum(r * c for r, c in shapes.values())
    g = np.random.default_rng(0)
    ids = {}
    for tag, r in (("r8", 8), ("r64", 64), ("r8b", 8)):
        a = e.lora_create()
        for n, (rows, cols) in shapes.items():
            e.lora_add(a, n, (g.standard_normal((r, cols)) * 0.05).astype(np.float32),
                       (g.standard_normal((rows, r)) * 0.05).astype(np.float32), 16.0 / r)
        ids[tag] = a
    lines = [f"LoRA switches, 3B shape: {len(names)} tensors, {elems / 1e9:.3f} G elements; one pass reads {elems * 2 / 1e9:.2f} GB of base store "
             f"and writes {elems * 2 / 1e9:.2f} GB of arena"]

    def timed(label, target, stream_bytes):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        e.lora_activate(target)
        dt = time.perf_counter() - t0
        lines.append(f"{label:<34} {dt * 1e3:9.2f} ms   {stream_bytes / dt / 1e12:6.3f} TB/s = {stream_bytes / dt / 8e12 * 100:5.1f} % of 8 TB/s")

    timed("first activation (snapshot + r8)", ids["r8"], elems * 8)   # snapshot: read + write, merge: read + write
    e.lora_activate(None)
    for rep in range(3):
        timed(f"base -> r8 (run {rep})", ids["r8"], elems * 4)
        timed(f"r8 -> r8b (run {rep})", ids["r8b"], elems * 4)
        timed(f"r8b -> r64 (run {rep})", ids["r64"], elems * 4)
        timed(f"r64 -> base (run {rep})", None, elems * 4)
    lines.append(f"base store: {e.lora_info()[2] / 1e9:.2f} GB")
    host = {n: (np.zeros(s, np.uint16), "bf16") for n, s in shapes.items()}
    for rep in range(2):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for n, arr in host.items():
            e.load_weight(n, arr)
        torch.cuda.synchronize()
        dt = time.perf_counter() - t0
        lines.append(f"ze_load_weight of the same {len(names)} tensors from host memory, bf16 (run {rep}): {dt * 1e3:9.2f} ms")
    e.close()
    text = "\n".join(lines) + "\n"
    print(text, end="")
    if args.out:
        with open(args.out, "w", encoding="utf-8") as f:
            f.write(text)


if __name__ == "__main__":
    main()
