"""CPU: the sampling filters' definition against HF's own warpers, ties, and the host layers (scheduler, server, model
wrapper) on stubs."""
from types import SimpleNamespace

import numpy as np
import pytest
import torch

import sampling_filters_ref as R
from zoomearth_amd.scheduler import ChainScheduler, Request


def hf_keep(z_scores, temperature, top_k, top_p, min_p):
    from transformers.generation.logits_process import (MinPLogitsWarper, TemperatureLogitsWarper, TopKLogitsWarper,
                                                        TopPLogitsWarper)
    s = torch.from_numpy(np.asarray(z_scores, dtype=np.float32))[None]
    ids = torch.zeros((1, 1), dtype=torch.long)
    if temperature != 1.0:
        s = TemperatureLogitsWarper(float(temperature))(ids, s)
    if top_k:
        s = TopKLogitsWarper(int(top_k))(ids, s)
    if top_p < 1.0:
        s = TopPLogitsWarper(float(top_p))(ids, s)
    if min_p > 0.0:
        s = MinPLogitsWarper(float(min_p))(ids, s)
    return torch.isfinite(s[0]).numpy()


@pytest.mark.parametrize("vocab", [2048, 151936])
@pytest.mark.parametrize("scale", [3.0, 1.0, 0.3])
def test_restatement_equals_hf_warpers_outside_the_margins(vocab, scale):
    differ = 0
    for seed in range(20):
        lg = R.rand_logits(1000 * seed + int(scale * 10), vocab, scale)
        for T, k, p, m in R.SETTINGS:
            want = hf_keep(lg, T, k, p, m)
            got, cut, kept = R.filter_ref(lg, T, k, p, m)
            k64, near = R.filter_f64(lg, T, k, p, m)
            what = f"vocab {vocab} scale {scale} seed {seed} setting {(T, k, p, m)}"
            only_k = p >= 1.0 and m <= 0.0
            differ += R.assert_same_keep(got, want, near, vocab, only_k, what + " (restatement vs HF)")
            R.assert_same_keep(got, k64, near, vocab, only_k, what + " (fixed point vs float64)")
            assert kept == int(got.sum()) and got[int(lg.argmax())]
            assert np.array_equal(got, R.scaled(lg, T) >= cut)   # the keep-set IS one cut
    print(f"vocab {vocab} scale {scale}: {differ} tokens differ from HF, all inside the margins")


def test_ties_are_kept_or_dropped_together():
    lg = R.rand_logits(3, 2048, 2.0)
    order = np.argsort(-lg)
    lg[order[9:14]] = lg[order[9]]          # the 10th value five times
    keep, cut, kept = R.filter_ref(lg, 1.0, top_k=10)
    assert kept == 14 and keep[order[:14]].all() and cut == lg[order[9]]
    flat = np.full(2048, 0.25, dtype=np.float32)
    for p in (1e-6, 0.1, 0.5, 0.9, 0.999999):
        keep, cut, kept = R.filter_ref(flat, 0.7, top_p=p)
        assert kept == 2048 and keep.all()
    keep, _, kept = R.filter_ref(flat, 1.0, top_k=5, top_p=0.3, min_p=1.0)
    assert kept == 2048


def test_masked_logits_are_never_kept_before_the_finite_ones():
    lg = R.rand_logits(4, 2048, 1.0)
    lg[100:2040] = -np.inf
    keep, cut, kept = R.filter_ref(lg, 1.0, top_k=50, top_p=0.999)
    assert np.isfinite(cut) and not keep[100:2040].any() and kept <= 50


# ---------------------------------------------------------------- host layers on stubs
EOS, PAD = 3, 0


class FilterStubEngine:
    """Just enough engine for ChainScheduler: records the order of the calls that matter here."""

    def __init__(self, max_seqs=2):
        self.max_seqs, self.max_ctx, self.max_prefill_rows, self.max_patches = max_seqs, 64, 256, 64
        self.log, self.chains = [], {}

    def gen_params(self, **kw):
        return kw

    def rope_index(self, ids, grids):
        return np.zeros((3, len(ids)), np.int32), 0

    def seq_reset(self, slot):
        self.log.append(("reset", slot))
        self.chains[slot] = dict(ids=[], out=[])

    def seq_len(self, slot):
        c = self.chains.get(slot)
        return 0 if c is None else len(c["ids"]) + max(len(c["out"]) - 1, 0)

    def seq_truncate(self, slot, keep):
        self.log.append(("truncate", slot))
        c = self.chains[slot]
        c["ids"], c["out"] = (c["ids"] + c["out"][:-1])[:keep], []

    def seq_copy_prefix(self, dst, src, n):
        self.log.append(("copy", dst))
        self.chains[dst] = dict(ids=list(self.chains[src]["ids"][:n]), out=[])

    def set_sampling_filter(self, slot, top_k=0, top_p=1.0, min_p=0.0):
        self.log.append(("filter", slot, top_k, top_p, min_p))

    def prefill_batch(self, slots, ids_l, emb_l, pos_l, dl):
        for s, ids in zip(slots, ids_l):
            self.chains[s]["ids"] += list(ids)

    def mark_seen(self, slot, ids):
        pass

    def chain_begin(self, slot, params, stream):
        self.log.append(("begin", slot, self.chains[slot]["ids"][0]))
        self.chains[slot]["out"].append(100)

    def decode_burst(self, slots, steps, params):
        for s in slots:
            self.chains[s]["out"] += [100] * steps
        return steps, [len(self.chains[s]["out"]) for s in slots], [False for _ in slots]

    def chain_tokens(self, slot, cap=0):
        return self.chains[slot]["out"][: cap or None]


class Proc:
    tokenizer = SimpleNamespace(decode=lambda ids, skip_special_tokens=True: " ".join(map(str, ids)))

    def __call__(self, text, images=None, return_tensors="pt", **kw):
        return dict(input_ids=torch.tensor([[int(w) for w in text[0].split()]]))


def make_model(**kw):
    cfg = SimpleNamespace(image_token_id=7, eos_token_ids=(EOS,), pad_token_id=PAD, vision=SimpleNamespace(spatial_merge_size=2))
    return SimpleNamespace(engine=FilterStubEngine(**kw), config=cfg, _chains={}, device="cpu",
                           generation_config=SimpleNamespace(repetition_penalty=1.0, temperature=None))


def run_requests(do_sample, **sched_kw):
    model = make_model(max_seqs=2)
    sched = ChainScheduler(model, Proc(), do_sample=do_sample, temperature=1.0, burst=2, share_prefix=False, **sched_kw)
    reqs = [Request(prompt="11 50 51", images=[], max_new_tokens=3, top_k=50),
            Request(prompt="12 50 51", images=[], max_new_tokens=3, top_p=0.9, min_p=0.05),
            Request(prompt="13 50 51", images=[], max_new_tokens=3),                    # the scheduler's default
            Request(prompt="14 50 51", images=[], max_new_tokens=3, top_k=0, top_p=1.0, min_p=0.0)]   # explicitly off
    for r in reqs:
        sched.submit(r)
    sched.run()
    return model.engine.log


def test_scheduler_sets_each_requests_own_filter_before_its_first_draw():
    log = run_requests(True, top_k=20)
    by_first = {}
    for i, ev in enumerate(log):
        if ev[0] == "begin":
            slot = ev[1]
            # what happened to the slot since its last reset / truncate / copy
            j = max(k for k in range(i) if log[k][0] in ("reset", "truncate", "copy") and log[k][1] == slot)
            by_first[ev[2]] = [x for x in log[j + 1:i] if x[0] == "filter" and x[1] == slot]
    assert [f[2:] for f in by_first[11]] == [(50, 1.0, 0.0)]
    assert [f[2:] for f in by_first[12]] == [(20, 0.9, 0.05)]     # top_k from the scheduler's default
    assert [f[2:] for f in by_first[13]] == [(20, 1.0, 0.0)]
    assert by_first[14] == []                                      # off: the reset already cleared the slot
    assert len(by_first) == 4


def test_greedy_scheduler_never_touches_the_filter_table():
    assert not [x for x in run_requests(False, top_k=20) if x[0] == "filter"]


def test_server_parses_and_rejects_the_filter_fields():
    from zoomearth_amd.serve import BadRequest, ChatServer

    srv = ChatServer(make_model(), Proc())
    msg = [{"role": "user", "content": "hi"}]
    p = srv._parse(dict(messages=msg, temperature=1.0, top_p=0.9, top_k=40, min_p=0.05))
    assert (p.top_k, p.top_p, p.min_p) == (40, 0.9, 0.05) and p.sample
    p = srv._parse(dict(messages=msg, temperature=0.7))
    assert (p.top_k, p.top_p, p.min_p) == (0, 1.0, 0.0)
    assert srv._parse(dict(messages=msg, temperature=0.7, top_k=-1)).top_k == 0     # vLLM's "off"
    for bad in (dict(top_p=2), dict(top_p=0), dict(top_p=-0.1), dict(top_k=-2), dict(min_p=1.5), dict(min_p=-1), dict(top_p="x")):
        with pytest.raises(BadRequest):
            srv._parse(dict(messages=msg, temperature=1.0, **bad))


class GenStubEngine:
    max_seqs, max_ctx, max_prefill_rows = 2, 64, 64

    def __init__(self):
        self.calls = []

    def rope_index(self, ids, grids):
        return np.zeros((3, len(ids)), np.int32), 0

    def seq_reset(self, slot):
        pass

    def seq_len(self, slot):
        return 0

    def prefill(self, *a, **kw):
        pass

    def mark_seen(self, *a):
        pass

    def generate(self, slot, max_new_tokens, **kw):
        self.calls.append(kw)
        return [5] * max_new_tokens


def wrapper(**gen_cfg):
    from zoomearth_amd.modeling import ZoomEarthForConditionalGeneration as M

    m = M.__new__(M)
    m.engine = GenStubEngine()
    m.config = SimpleNamespace(image_token_id=7, eos_token_ids=(EOS,), pad_token_id=PAD)
    m.generation_config = SimpleNamespace(temperature=None, top_p=None, top_k=None, repetition_penalty=1.0, **gen_cfg)
    from collections import OrderedDict
    m._vit_cache, m._chains, m._next_slot, m.reuse_prefix = OrderedDict(), OrderedDict(), 0, False
    return m


def test_model_generate_forwards_the_filters_and_raises_hf_errors():
    ids = torch.tensor([[11, 12, 13]])
    m = wrapper()
    out = m.generate(input_ids=ids, max_new_tokens=2, do_sample=True, top_p=0.9, top_k=50)
    assert out.shape == (1, 5)
    kw = m.engine.calls[-1]
    assert kw["do_sample"] and (kw["top_k"], kw["top_p"], kw["min_p"]) == (50, 0.9, 0.0)
    m.generate(input_ids=ids, max_new_tokens=2, do_sample=True, min_p=0.1)
    assert (m.engine.calls[-1]["top_k"], m.engine.calls[-1]["top_p"], m.engine.calls[-1]["min_p"]) == (0, 1.0, 0.1)
    for bad in (dict(top_p=1.5), dict(top_p=-0.5), dict(top_k=-3), dict(min_p=2.0)):
        with pytest.raises(ValueError):
            m.generate(input_ids=ids, max_new_tokens=2, do_sample=True, **bad)
    with pytest.raises(NotImplementedError):
        m.generate(input_ids=ids, max_new_tokens=2, num_beams=2)
    # a stock generation_config (top_p and top_k present) no longer fails; top_k = 1 stays the greedy shortcut
    m = wrapper(min_p=None)
    m.generation_config.top_p, m.generation_config.top_k, m.generation_config.temperature = 0.001, 1, 0.1
    m.generate(input_ids=ids, max_new_tokens=2, do_sample=True)
    assert not m.engine.calls[-1]["do_sample"] and "top_k" not in m.engine.calls[-1]
    m.generation_config.top_k = 20
    m.generate(input_ids=ids, max_new_tokens=2, do_sample=True)
    assert (m.engine.calls[-1]["top_k"], m.engine.calls[-1]["top_p"]) == (20, 0.001)
    # greedy ignores the filters altogether
    m.generate(input_ids=ids, max_new_tokens=2, do_sample=False, top_p=0.5)
    assert "top_p" not in m.engine.calls[-1]
