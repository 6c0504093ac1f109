"""numpy restatement of ONE row of the per-chain sampling kernels (zoomearth_amd/csrc/ze_sample.hip, ze_seq_set_sampling /
ze_op_sample_rows): a row with temperature > 0 is the oracle's draw (oracle.qwen25vl.sample_temperature: the kernel's fp32
summation order and inverse-CDF rule) with the row's own temperature, seed and random stream; a greedy row (temperature 0) is the
repetition-penalised arg-max with the lowest index on ties and 0 for a row without a comparable logit (every one NaN), as
torch.argmax gives it."""
import numpy as np

from oracle import qwen25vl as Q

f32 = np.float32
GAP = 1e-5   # tests/test_gpu_sampling.py: draws closer than this to a CDF boundary may differ where expf differs in the last bit


def scores_of(logits, seen_ids, penalty):
    lg = np.asarray(logits, dtype=f32)
    return Q.apply_repetition_penalty(lg, list(seen_ids), penalty) if penalty != 1.0 and len(seen_ids) else lg


def greedy_token(scores) -> int:
    sc = np.asarray(scores, dtype=f32)
    ok = ~np.isnan(sc)
    if not ok.any():
        return 0
    return int(np.nonzero(ok & (sc == sc[ok].max()))[0][0])


def sample_row(logits, seen_ids, temperature, penalty, seed, stream, index):
    """(token, gap) of one row; gap = inf for a greedy row (an exact rule), else the oracle's CDF gap"""
    if not temperature > 0.0:
        return greedy_token(scores_of(logits, seen_ids, penalty)), float("inf")
    tok, gap = Q.sample_temperature(np.asarray(logits, dtype=f32), list(seen_ids), float(penalty), float(temperature), seed=int(seed),
                                    slot=int(stream), index=int(index))
    return int(tok), float(gap)


# ---- the cases of the unit-op test (tests/test_gpu_chain_sampling.py), shared with the CPU self-check
SHAPES = ((257, 257, 1), (2000, 2000, 3), (2049, 2056, 65))   # vocab, ld, rows
INDICES = (0, 1, 7, 300)


def case_row(r, vocab):
    """row r: (logits, seen ids, temperature, penalty, seed, stream); every fifth row greedy"""
    logits = (np.random.default_rng(1000 + r).normal(size=vocab) * 3).astype(f32)
    temperature = 0.0 if r % 5 == 4 else (0.7, 1.0, 0.01)[r % 3]
    seen = [(7 * r + 3) % vocab, (13 * r + 100) % vocab, int(np.argmax(logits))]   # (the arg-max among them: the penalty moves it)
    return logits, seen, temperature, (1.0, 1.3)[r % 2], 1234 + r, r % 5
