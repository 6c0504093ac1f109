"""CPU: the entropy filters' definition (tests/entropy_filters_ref.py) against HF's own warpers, analytic cases, and the host
layers (ChainRequest, scheduler, server, model wrapper) on the stubs of tests/test_sampling_filters_cpu.py."""
import math

import numpy as np
import pytest
import torch

import entropy_filters_ref as E
from test_sampling_filters_cpu import FilterStubEngine, Proc, make_model, wrapper
from zoomearth_amd.chain_request import ChainRequest
from zoomearth_amd.scheduler import ChainScheduler, Request


def hf_keep(scores, temperature, top_k, top_p, min_p, typical_p, eps, eta):
    from transformers.generation.logits_process import (EpsilonLogitsWarper, EtaLogitsWarper, MinPLogitsWarper, TemperatureLogitsWarper,
                                                        TopKLogitsWarper, TopPLogitsWarper, TypicalLogitsWarper)
    # (in float64: over 151,936 tokens the fp32 cumsum of HF's own typical warper drifts by more than the 1e-5 mass margin)
    s = torch.from_numpy(np.asarray(scores, dtype=np.float32).astype(np.float64))[None]
    ids = torch.zeros((1, 1), dtype=torch.long)
    if temperature != 1.0:
        s = TemperatureLogitsWarper(float(temperature))(ids, s)
    if top_k:
        s = TopKLogitsWarper(int(top_k))(ids, s)
    if top_p < 1.0:
        s = TopPLogitsWarper(float(top_p))(ids, s)
    if min_p > 0.0:
        s = MinPLogitsWarper(float(min_p))(ids, s)
    if typical_p < 1.0:
        s = TypicalLogitsWarper(mass=float(typical_p))(ids, s)
    if eps > 0.0:
        s = EpsilonLogitsWarper(epsilon=float(eps))(ids, s)
    if eta > 0.0:
        s = EtaLogitsWarper(epsilon=float(eta))(ids, s)
    return torch.isfinite(s[0]).numpy()


@pytest.mark.parametrize("vocab", E.VOCABS)
def test_restatement_equals_hf_warpers_outside_the_margins_on_every_row_the_tests_use(vocab):
    differ = 0
    for name, lg in E.case_rows(vocab):
        for st in E.SETTINGS:
            what = f"vocab {vocab} row '{name}' setting {st}"
            got, cut, ceil, kept = E.band_ref(lg, *st)
            k64, near = E.band_f64(lg, *st)
            # the condition of every check that uses these rows: the float64 reference alone stays within the cap
            assert int(near.sum()) <= E.cap_for(vocab), f"{what}: {int(near.sum())} tokens inside the margins"
            differ += E.assert_same_keep(got, hf_keep(lg, *st), near, vocab, what + " (restatement vs HF)")
            E.assert_same_keep(got, k64, near, vocab, what + " (fixed point vs float64)")
            assert kept == int(got.sum()) >= 1
            assert np.array_equal(got, E.in_band(lg, st[0], cut, ceil))   # the keep-set IS one band
            assert (ceil == np.inf) == (st[4] >= 1.0)
    print(f"vocab {vocab}: {differ} tokens differ from HF, all inside the margins")


def test_typical_drops_the_arg_max_on_a_peaked_plus_flat_row():
    # one token with 40 % of the mass over a flat tail: H is about the tail's -log p, far from the peak's
    vocab = 1000
    lg = np.zeros(vocab, dtype=np.float32)
    lg[17] = np.float32(math.log(0.4 / (0.6 / (vocab - 1))))
    keep, cut, ceil, kept = E.band_ref(lg, 1.0, typical_p=0.5)
    assert not keep[17] and kept == vocab - 1 and cut == 0.0 and ceil == 0.0   # the flat tokens tie: together
    assert np.array_equal(keep, hf_keep(lg, 1.0, 0, 1.0, 0.0, 0.5, 0.0, 0.0))
    keep, _, _, _ = E.band_ref(lg, 1.0, typical_p=0.7)   # the tail alone holds 60 %: the peak comes back
    assert keep.all()


def test_every_stage_off_is_no_band():
    lg = E.row_for(1, 2048, 2.0)
    keep, cut, ceil, kept = E.band_ref(lg, 0.9)
    assert keep.all() and cut == -np.inf and ceil == np.inf and kept == 2048


def test_ties_live_or_die_together():
    lg = E.row_for(2, 2048, 2.0)
    order = np.argsort(-lg)
    lg[order[5:9]] = lg[order[5]]
    for st in E.SETTINGS:
        keep = E.band_ref(lg, *st)[0]
        assert len(set(keep[order[5:9]].tolist())) == 1, st
    flat = np.full(2048, 0.25, dtype=np.float32)
    for kw in (dict(typical_p=0.01), dict(typical_p=0.99), dict(epsilon_cutoff=1e-4), dict(eta_cutoff=1e-4)):
        assert E.band_ref(flat, 1.0, **kw)[3] == 2048, kw


def test_each_stage_keeps_at_least_one_token():
    lg = E.row_for(3, 2048, 1.0)
    for kw in (dict(typical_p=1e-6), dict(epsilon_cutoff=0.999), dict(eta_cutoff=0.999),
               dict(typical_p=1e-6, epsilon_cutoff=0.999, eta_cutoff=0.999)):
        keep, cut, ceil, kept = E.band_ref(lg, 1.0, **kw)
        assert kept >= 1 and keep.sum() == kept, kw
    flat = np.full(2048, 0.25, dtype=np.float32)   # nobody reaches the threshold: the largest z -- all of them -- stays
    assert E.band_ref(flat, 1.0, epsilon_cutoff=0.5)[3] == 2048
    assert E.band_ref(lg, 1.0, epsilon_cutoff=0.999)[3] == 1 and E.band_ref(lg, 1.0, epsilon_cutoff=0.999)[0][int(lg.argmax())]


def test_eta_over_a_uniform_row_uses_exp_of_minus_log_n():
    # n equal tokens over a far lower rest: H = log n, thr = min(eta, sqrt(eta) / n); the n tokens have p = 1 / n each
    n, vocab = 64, 2048
    lg = np.full(vocab, -40.0, dtype=np.float32)
    lg[:n] = 0.0
    eta = 0.5                                  # sqrt(eta) / n < 1 / n < eta: the uniform tokens pass only through exp(-H)
    keep, cut, ceil, kept = E.band_ref(lg, 1.0, eta_cutoff=eta)
    assert kept == n and keep[:n].all() and cut == 0.0 and ceil == np.inf
    assert math.sqrt(eta) * math.exp(-math.log(n)) < 1.0 / n < eta
    assert np.array_equal(keep, hf_keep(lg, 1.0, 0, 1.0, 0.0, 1.0, 0.0, eta))
    # epsilon at the same value has no entropy to lean on: nobody reaches it, the largest z (all n, tied) stays
    assert E.band_ref(lg, 1.0, epsilon_cutoff=eta)[3] == n


# ---------------------------------------------------------------- host layers on stubs
class EntropyStubEngine(FilterStubEngine):
    def set_entropy_filter(self, slot, typical_p=1.0, epsilon_cutoff=0.0, eta_cutoff=0.0):
        self.log.append(("entropy", slot, typical_p, epsilon_cutoff, eta_cutoff))

    def set_sampling(self, slot, **kw):
        self.log.append(("sampling", slot, kw))


def run_requests(do_sample, **sched_kw):
    model = make_model(max_seqs=2)
    model.engine = EntropyStubEngine(max_seqs=2)
    sched = ChainScheduler(model, Proc(), do_sample=do_sample, temperature=1.0, burst=2, share_prefix=False, **sched_kw)
    reqs = [Request(prompt="11 50 51", images=[], max_new_tokens=3, typical_p=0.3),
            Request(prompt="12 50 51", images=[], max_new_tokens=3, epsilon_cutoff=3e-4, top_p=0.9),
            Request(prompt="13 50 51", images=[], max_new_tokens=3),                                   # the scheduler's default
            Request(prompt="14 50 51", images=[], max_new_tokens=3, typical_p=1.0, epsilon_cutoff=0.0, eta_cutoff=0.0),   # off
            Request(prompt="15 50 51", images=[], max_new_tokens=3, do_sample=False, typical_p=0.2)]   # a greedy request
    for r in reqs:
        sched.submit(r)
    sched.run()
    return model.engine.log


def per_chain(log, kind):
    out = {}
    for i, ev in enumerate(log):
        if ev[0] == "begin":
            slot = ev[1]
            j = max(k for k in range(i) if log[k][0] in ("reset", "truncate", "copy") and log[k][1] == slot)
            out[ev[2]] = [x[2:] for x in log[j + 1:i] if x[0] == kind and x[1] == slot]
    return out


def test_scheduler_sets_each_requests_own_entropy_filter_before_its_first_draw():
    log = run_requests(True, eta_cutoff=2e-3)
    ent, filt = per_chain(log, "entropy"), per_chain(log, "filter")
    assert ent[11] == [(0.3, 0.0, 2e-3)]           # eta from the scheduler's default
    assert ent[12] == [(1.0, 3e-4, 2e-3)] and filt[12] == [(0, 0.9, 0.0)]
    assert ent[13] == [(1.0, 0.0, 2e-3)]
    assert ent[14] == []                           # explicitly off: the reset already cleared the slot
    assert ent[15] == []                           # greedy ignores the settings
    assert len(ent) == 5


def test_greedy_scheduler_never_touches_the_entropy_table():
    assert not [x for x in run_requests(False, typical_p=0.5) if x[0] == "entropy"]


def test_scheduler_refuses_values_outside_the_unit_interval():
    model = make_model(max_seqs=2)
    model.engine = EntropyStubEngine(max_seqs=2)
    sched = ChainScheduler(model, Proc(), do_sample=True, temperature=1.0, burst=2, share_prefix=False)
    for bad in (dict(typical_p=0.0), dict(typical_p=1.5), dict(epsilon_cutoff=1.0), dict(epsilon_cutoff=-0.1), dict(eta_cutoff=2.0)):
        with pytest.raises(ValueError):
            sched._resolve(Request(prompt="11 50 51", images=[], max_new_tokens=3, **bad))


def test_chain_request_installs_the_entropy_filter_for_a_sampled_chain_only():
    e = EntropyStubEngine()
    ChainRequest(sampled=True, typical_p=0.4, eta_cutoff=1e-3).install(e, 1, [5, 6])
    assert e.log == [("entropy", 1, 0.4, 0.0, 1e-3)]
    e.log.clear()
    ChainRequest(sampled=False, typical_p=0.4).install(e, 1, [5, 6])
    ChainRequest(sampled=True).install(e, 1, [5, 6])
    assert e.log == []
    assert ChainRequest(sampled=True, typical_p=0.4).speculation_conflict() == "sampling"


def test_server_parses_and_rejects_the_entropy_fields():
    from zoomearth_amd.serve import BadRequest, ChatServer

    srv = ChatServer(make_model(), Proc())
    msg = [{"role": "user", "content": "hi"}]
    p = srv._parse(dict(messages=msg, temperature=1.0, typical_p=0.3, epsilon_cutoff=3e-4, eta_cutoff=2e-3))
    assert (p.typical_p, p.epsilon_cutoff, p.eta_cutoff) == (0.3, 3e-4, 2e-3) and p.sample
    assert p.entropy_kw() == dict(typical_p=0.3, epsilon_cutoff=3e-4, eta_cutoff=2e-3)
    p = srv._parse(dict(messages=msg, temperature=0.7, typical_p=1.0, epsilon_cutoff=0.0))
    assert (p.typical_p, p.epsilon_cutoff, p.eta_cutoff) == (1.0, 0.0, 0.0) and p.entropy_kw() == {}
    for bad in (dict(typical_p=0), dict(typical_p=1.5), dict(typical_p="x"), dict(epsilon_cutoff=1.0), dict(epsilon_cutoff=-1),
                dict(eta_cutoff=3), dict(eta_cutoff=True)):
        with pytest.raises(BadRequest):
            srv._parse(dict(messages=msg, temperature=1.0, **bad))


def test_model_generate_forwards_the_entropy_filters_and_raises_hf_errors():
    ids = torch.tensor([[11, 12, 13]])
    m = wrapper()
    m.generate(input_ids=ids, max_new_tokens=2, do_sample=True, typical_p=0.2, eta_cutoff=2e-3)
    kw = m.engine.calls[-1]
    assert kw["do_sample"] and kw["typical_p"] == 0.2 and kw["eta_cutoff"] == 2e-3 and "epsilon_cutoff" not in kw
    m.generate(input_ids=ids, max_new_tokens=2, do_sample=True, typical_p=1.0, epsilon_cutoff=0.0)    # HF's off values
    assert not {"typical_p", "epsilon_cutoff", "eta_cutoff"} & set(m.engine.calls[-1])
    for name in ("typical_p", "epsilon_cutoff", "eta_cutoff"):
        for bad in (1.5, -0.2):
            with pytest.raises(ValueError, match=f"`{name}` has to be a float > 0 and < 1, but is"):
                m.generate(input_ids=ids, max_new_tokens=2, do_sample=True, **{name: bad})
    # the generation_config is the fall-back, a keyword wins
    m = wrapper(typical_p=0.9, epsilon_cutoff=0.0, eta_cutoff=None)
    m.generate(input_ids=ids, max_new_tokens=2, do_sample=True)
    assert m.engine.calls[-1]["typical_p"] == 0.9 and "epsilon_cutoff" not in m.engine.calls[-1]
    m.generate(input_ids=ids, max_new_tokens=2, do_sample=True, typical_p=0.5)
    assert m.engine.calls[-1]["typical_p"] == 0.5
    # greedy ignores them, as HF ignores its warpers
    m.generate(input_ids=ids, max_new_tokens=2, do_sample=False, typical_p=0.5)
    assert "typical_p" not in m.engine.calls[-1]
    # speculation by prompt lookup is greedy only: refused together
    with pytest.raises(ValueError, match="prompt_lookup_num_tokens"):
        m.generate(input_ids=ids, max_new_tokens=2, prompt_lookup_num_tokens=2, typical_p=0.5)
