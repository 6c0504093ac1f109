"""GPU: the one-line JSON contract of bench.py (what the driver parses): keys, types, the roofline and cpu_baseline
objects, and internal consistency (value = questions / time, frac = achieved / peak)."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def run_bench(*args, timeout=1500, **env):
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), *args], capture_output=True, text=True,
                       timeout=timeout, cwd=ROOT, env=dict(os.environ, **env))
    assert r.returncode == 0, r.stderr[-2000:]
    lines = [ln for ln in r.stdout.strip().splitlines() if ln.startswith("{")]
    assert len(lines) == 1, r.stdout[-2000:]
    return json.loads(lines[0])


def check_roofline(r, lo=0.05):
    for k in ("bound", "achieved", "peak", "unit", "frac", "traffic"):
        assert k in r, k
    assert r["bound"] == "hbm" and r["unit"] == "GB/s" and r["peak"] == 8000.0
    assert abs(r["frac"] - r["achieved"] / r["peak"]) < 1e-9 and lo < r["frac"] < 1.0
    # counter traffic against algorithmic bytes: above 1 where a kernel re-reads, down to ~0.85 where the chains of a tile read their
    # shared prefix from one cache (the stream line's attention: 0.856 x in round 4's PMC passes)
    assert r["traffic"] is None or 0.8 < r["traffic"] / r["bytes_per_launch"] < 1.6
    if r.get("traffic_source") and "DIFFERENT" in r["traffic_source"]:   # (stale counter figures are named, not hidden)
        import warnings
        warnings.warn("profiles/traffic_latest.json was collected on other kernel sources than this tree's: " + r["traffic_source"][-160:])
    if r["traffic"] is not None and "hbm_interface_frac" in r:
        # (avg_us is printed with two decimals)
        assert abs(r["hbm_interface_frac"] - r["traffic"] / (r["avg_us"] * 1e-6) / 1e9 / r["peak"]) < 1e-3 and 0 < r["hbm_interface_frac"] < 1


def test_bench_line_contract():
    """The default workload: BASELINE configs[3], the question stream (here 12 timed steps of 64 questions: enough live chains for
    the decode attention to be the step's dominant kernel, so that the line takes the branch the driver's line takes -- the
    shared-prefix measurement), with the configs[1] / configs[2] / cpu_baseline sub-objects of an N = 1 `--full` run."""
    d = run_bench("--gpus", "1", "--steps", "12", "--warmup", "1", "--full")
    for k in ("metric", "value", "unit", "n_gpus", "steps", "warmup", "ms_per_step", "higher_is_better", "scaling",
              "vs_baseline", "dtype", "data", "config", "roofline", "cpu_baseline", "per_rank"):
        assert k in d, k
    assert d["unit"] == "questions/s" and d["n_gpus"] == 1 and d["steps"] == 12 and d["warmup"] == 1
    assert d["higher_is_better"] is True and d["scaling"] == "weak" and d["vs_baseline"] is None
    assert d["dtype"] == "bf16" and d["data"] == "synthetic" and "workload" in d["config"] and "model" not in d["config"]
    assert "configs[3]" in d["config"]["workload"] and d["config"]["questions_per_step_per_gpu"] == 64
    assert abs(d["value"] - 64 * 1000.0 / d["ms_per_step"]) < 1e-6 * d["value"]     # 64 questions per step per GPU
    assert d["per_rank"]["questions"] == [768] and d["scheduler"]["admitted"] == 1536  # two stages per question
    assert 32 < d["mean_chains_per_step"] <= 768
    assert d["value"] > 10.0
    check_roofline(d["roofline"])
    assert d["roofline"]["chains"] >= 1 and "decode" in d["roofline"]["kernel"]
    # the branch the driver's line takes: the attention timed with the stream's sharing (ten chains per tile read their prefix from
    # one cache) -- fewer bytes cross the HBM interface than the algorithmic ones -- next to the same launch on independent chains
    r = d["roofline"]
    assert "attention" in r["kernel"] and "sharing" in r and "independent_chains" in r, r.get("kernel")
    ind = r["independent_chains"]
    assert r["avg_us"] < ind["avg_us"] and r["frac"] > ind["frac"] and r["traffic"] < ind["traffic"]
    assert r["hbm_interface_frac"] is not None and r["hbm_interface_frac"] < r["frac"]
    # the stream's largest consumer of GPU time is named next to it, with its own fraction measured alone
    tk = r["top_kernel_by_gpu_time"]
    assert tk is not None and "error" not in tk, tk
    assert 0.05 < tk["share_of_gpu_time"] < 0.6 and tk["share_source"].startswith("profiles/r") and tk["kernel"]
    if "frac" in tk:
        assert tk["bound"] == "mfma" and 0.2 < tk["frac"] < 1.0 and abs(tk["frac"] - tk["achieved_TFLOPs"] / 2500.0) < 1e-3
        # round 6: per pass size, both launch forms, the four projections in pass order -- never a mean over two sizes
        assert tk["form_in_stream"] in ("tile_granular", "persistent") and len(tk["by_rows"]) >= 2
        for rows_p, ent in tk["by_rows"].items():
            for form in ("persistent", "tile_granular"):
                assert set(ent[form]["layer_us"]) == {"qkv", "o", "gate_up", "down"} and 0.2 < ent[form]["frac"] < 1.0, (rows_p, form, ent[form])
        big = tk["by_rows"][max(tk["by_rows"], key=int)]
        assert tk["frac"] == big[tk["form_in_stream"]]["frac"]
    # round 6: what a row pays for a layer's projections in a decode step and in a prefill pass; what the line
    # owes to the synthetic tokenizer's identity round trip
    dec = d["roofline_phases"]["decode"]
    assert 0.05 < dec["projections_us_per_row_per_layer"] < 1.0
    assert all(0.02 < v < dec["projections_us_per_row_per_layer"] for v in dec["prefill_pass_projections_us_per_row_per_layer"].values())
    rs = d["reuse_sensitivity"]
    assert 0.5 < rs["ratio"] <= 1.02 and abs(d["value_without_generated_row_reuse"] - d["value"] * rs["ratio"]) < 0.01
    assert rs["generated_rows_kept_per_question"][1] == 0.0 < rs["generated_rows_kept_per_question"][0] and 0 < d["generated_rows_kept_fraction"] <= 1
    # tile uploads are INSIDE the timed region (pinned host -> HBM by each lane's TileFeeder, ahead of the first question)
    assert "INSIDE the timed region" in d["tile_upload_note"] and d["tile_upload_ms"] > 0.3
    # the stream's own whole-question roofline (isolated kernel-time accounting; SURVEY 8d's formula at the measured batch)
    rp = d["roofline_phases"]
    assert "error" not in rp, rp
    assert rp["decode"]["bound"] == "hbm" and rp["vit"]["bound"] == "mfma" and rp["prefill"]["bound"] == "mfma"
    for k in ("vit", "prefill", "decode"):
        assert 0 < rp[k]["frac"] < 1 and rp[k]["ms_per_question"] > 0, (k, rp[k])
    assert 0 < rp["question"]["frac"] < 1 and rp["question"]["measured_ms"] > rp["question"]["roofline_ms"] > 0
    assert abs(rp["question"]["measured_ms"] - 1000.0 / d["value"]) < 0.02 * rp["question"]["measured_ms"]
    assert abs(rp["isolated_ms_per_question"] - sum(rp[k]["ms_per_question"] for k in ("vit", "prefill", "decode"))) < 0.01
    # the decode phase is the histogram-weighted sum of the step timed alone in every live-chain bucket the stream visited
    hist = rp["decode"]["steps_by_live_chains"]
    assert hist and sum(b["steps"] for b in hist) == d["scheduler"]["steps"]
    assert all(b["step_us"] > 0 and b["timed_at"] >= 65 for b in hist)
    want_ms = sum(b["steps"] * b["step_us"] for b in hist) / 1000.0 / d["per_rank"]["questions"][0]
    assert abs(want_ms - rp["decode"]["ms_per_question"]) < 0.01 * want_ms + 0.002
    assert sum(v for k, v in d["scheduler"].items() if k.startswith("steps_le_") or k == "steps_gt_768") == d["scheduler"]["steps"]
    assert d["per_rank"]["filled_own_weights"] == [True]
    c = d["cpu_baseline"]
    for k in ("value", "unit", "cores", "threads", "kind", "sample"):
        assert k in c, k
    assert c["kind"] in ("reference", "port") and c["unit"] == "questions/s" and c["cores"] >= 1
    assert c["cores"] == os.cpu_count() and (c["threads"] is None or 1 <= c["threads"] <= c["cores"])
    assert c["value"] is None or 0 < c["value"] < d["value"]
    assert d["tile_upload_ms"] > 0 and d["weight_broadcast_s"] == 0
    # BASELINE configs[1] in the same line: the single-chain path with its own roofline (the decode gate/up GEMV)
    s = d["configs1"]
    assert s["steps"] == 4 and abs(s["value"] - 1000.0 / s["ms_per_question"]) < 1e-6 * s["value"] and 0.5 < s["value"] < 10.0
    assert (s["L1"], s["N1"], s["N2"]) == (802, 192, 96)
    check_roofline(s["roofline"], lo=0.3)
    ph = s["roofline_phases"]
    assert ph["decode"]["bound"] == "hbm" and ph["vit"]["bound"] == "mfma" and 0 < ph["question"]["frac"] < 1
    # BASELINE configs[2] in the same line: 256 questions about 6 tiles through 64 chain slots
    b = d["batch64"]
    assert b["questions"] == 256 and b["chain_slots"] == 64 and b["steps"] == 4
    assert abs(b["value"] - 64000.0 / b["ms_per_step"]) < 1e-6 * b["value"]
    assert b["value"] > 5 * s["value"]
    assert 0.75 * 192 <= b["mean_N1"] <= 1.25 * 192 and 0.75 * 96 <= b["mean_N2"] <= 1.25 * 96 and b["mean_L1"] == 802
    assert b["scheduler"]["admitted"] == 512 and b["scheduler"]["chain_steps"] > 40 * b["scheduler"]["steps"]
    check_roofline(b["roofline"])
    assert b["roofline"]["chains"] == 64 and "batched decode" in b["roofline"]["kernel"]


def test_bench_batch1_is_configs1():
    """`--batch 1`: BASELINE configs[1] as the line's own value (one question per step), no sub-objects."""
    d = run_bench("--gpus", "1", "--steps", "2", "--warmup", "1", "--batch", "1", "--no-cpu-baseline", "--full")
    assert "configs[1]" in d["config"]["workload"] and d["config"]["questions_per_step_per_gpu"] == 1
    assert abs(d["value"] - 1000.0 / d["ms_per_step"]) < 1e-6 * d["value"] and 0.5 < d["value"] < 10.0
    check_roofline(d["roofline"], lo=0.3)
    assert "batch64" not in d and "configs1" not in d and "cpu_baseline" not in d


def test_bench_plain_run_is_the_headline_only_and_dumps_its_outputs(tmp_path):
    """A plain run (no --full) times the stream and prints the headline line without the annexes; --dump-outputs writes the token ids
    and lengths of the last timed step's questions, and a second run with the same arguments gets the same inputs (same questions,
    same prompt lengths)."""
    runs = []
    for k in range(2):
        out = tmp_path / f"run{k}"
        d = run_bench("--gpus", "1", "--steps", "2", "--warmup", "1", "--dump-outputs", str(out))
        for key in ("metric", "value", "unit", "higher_is_better", "dtype", "ms_per_step"):
            assert key in d, key
        assert d["steps"] == 2 and d["warmup"] == 1 and d["dtype"] == "bf16" and d["higher_is_better"] is True
        assert abs(d["value"] - 64 * 1000.0 / d["ms_per_step"]) < 1e-6 * d["value"]
        for key in ("roofline", "roofline_phases", "reuse_sensitivity", "configs1", "batch64", "cpu_baseline"):
            assert key not in d, key
        arrays = {n: np.load(out / f"{n}.npy") for n in ("question", "stage1_tokens", "stage2_tokens", "lengths")}
        q, t1, t2, ln = arrays["question"], arrays["stage1_tokens"], arrays["stage2_tokens"], arrays["lengths"]
        assert q.dtype == np.float64 and t1.dtype == t2.dtype == ln.dtype == np.float32
        assert q.tolist() == [1_000_000 + i for i in range(64, 128)] and ln.shape == (64, 4) and len(t1) == len(t2) == 64
        assert (ln[:, 0] == 802).all() and ((t1 >= 0).sum(axis=1) == ln[:, 1]).all() and ((t2 >= 0).sum(axis=1) == ln[:, 3]).all()
        assert 0.75 * 192 - 1 <= ln[:, 1].min() and ln[:, 1].max() <= 1.25 * 192 + 1
        runs.append(arrays)
    assert np.array_equal(runs[0]["question"], runs[1]["question"]) and np.array_equal(runs[0]["lengths"][:, 1], runs[1]["lengths"][:, 1])


def test_bench_runs_the_collective_path_on_one_rank():
    """ZE_BENCH_FORCE_DIST=1: a one-rank RCCL communicator -- init, the weight broadcast (accel.broadcast_engine_weights), the
    barriers and the max-over-ranks reductions of the N > 1 path, on this box's one GPU."""
    d = run_bench("--gpus", "1", "--steps", "1", "--warmup", "1", "--no-cpu-baseline", "--no-batch64", "--no-configs1",
                  ZE_BENCH_FORCE_DIST="1", MASTER_PORT="29577")
    assert d["n_gpus"] == 1 and d["weight_broadcast_s"] > 0 and d["per_rank"]["questions"] == [64]
    assert d["value"] > 5.0
    # the xGMI-shaped form of the broadcast (scatter + in-place all-gather + tail broadcast) on the same one-rank RCCL
    # communicator: no peer to scatter to, but ncclAllGather in place on the 7.5-GB arena and the tail broadcast run on RCCL
    d = run_bench("--gpus", "1", "--steps", "1", "--warmup", "1", "--no-cpu-baseline", "--no-batch64", "--no-configs1",
                  ZE_BENCH_FORCE_DIST="1", MASTER_PORT="29578", ZE_BCAST="scatter_allgather")
    assert d["weight_broadcast_s"] > 0 and d["per_rank"]["questions"] == [64] and d["value"] > 5.0


def test_bench_two_ranks_share_the_gpu_over_gloo():
    """the N > 1 branch of bench.py had never executed anywhere (RCCL wants one rank per GPU and no multi-GPU box
    has been available).  `ZE_DIST_BACKEND=gloo` runs the same code with both ranks on this box's one GPU: `--gpus 2` spawns the
    ranks itself (before anything touches the GPU), the question table of 2 x 64 questions is sharded by tile, rank 1 never
    fills its weights and receives the packed arena by broadcast, the report is reduced over the ranks (MAX of the times, SUM of
    the per-rank rows) and rank 0 alone prints the line."""
    d = run_bench("--gpus", "2", "--steps", "1", "--warmup", "1", "--lanes", "1", "--slots", "96", "--no-cpu-baseline",
                  "--no-batch64", "--no-configs1", ZE_DIST_BACKEND="gloo")
    assert d["n_gpus"] == 2 and d["per_rank"]["dist_backend"] == "gloo"
    assert len(d["per_rank"]["questions"]) == 2 and sum(d["per_rank"]["questions"]) == 128
    assert min(d["per_rank"]["questions"]) >= 40                      # tile-level LPT: close to 64 / 64
    assert d["per_rank"]["filled_own_weights"] == [True, False] and d["weight_broadcast_s"] > 0
    assert d["config"]["parallelism"] == "dp2" and d["scaling"] == "weak"
    assert abs(d["value"] - 128 * 1000.0 / (d["ms_per_step"] * 1)) < 1e-6 * d["value"]   # all questions / the slowest rank's time
    assert d["ms_per_step"] >= 1000.0 * max(d["per_rank"]["seconds"]) * 0.999 and d["value"] > 3.0


@pytest.mark.parametrize("bcast", ["broadcast"])   # (the scatter + all-gather form with eight ranks: tests/test_hostlayer_cpu.py, world = 8 --
def test_bench_eight_ranks_share_the_gpu_over_gloo(bcast):   #  on the 7.5-GB arena over gloo it takes five minutes and proves nothing more)
    """the 8-rank shape of everything -- the LPT packing over 8, seven receivers of the weight broadcast, the
    port / LOCAL_RANK mapping of `--gpus 8` -- had never executed.  No 8-GPU node exists for this build, so the eight ranks share
    this box's one GPU over gloo (children spawned before any GPU call): 8 x 64 questions sharded by tile, rank 0 alone fills its
    weights, the others receive the packed arena by broadcast, times reduced with MAX, rows with SUM.  What this does NOT give is a scaling curve: one GPU runs all eight ranks."""
    d = run_bench("--gpus", "8", "--steps", "1", "--warmup", "0", "--lanes", "1", "--slots", "48", "--no-cpu-baseline", "--no-batch64",
                  "--no-configs1", timeout=2400, ZE_DIST_BACKEND="gloo", **({"ZE_BCAST": "scatter_allgather"} if bcast != "broadcast" else {}))
    pr = d["per_rank"]
    assert d["n_gpus"] == 8 and pr["dist_backend"] == "gloo" and d["config"]["parallelism"] == "dp8" and d["scaling"] == "weak"
    assert len(pr["questions"]) == 8 and sum(pr["questions"]) == 512
    assert max(pr["questions"]) / (sum(pr["questions"]) / 8.0) <= 1.15          # tile-level LPT over eight ranks
    assert pr["filled_own_weights"] == [True] + [False] * 7 and d["weight_broadcast_s"] > 0
    assert abs(d["value"] - 512 * 1000.0 / d["ms_per_step"]) < 1e-6 * d["value"] and d["value"] > 1.0
    assert d["ms_per_step"] >= 1000.0 * max(pr["seconds"]) * 0.999
