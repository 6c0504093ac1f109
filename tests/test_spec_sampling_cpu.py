"""CPU: speculative decoding for sampled chains (ze_seq_set_speculation_mode mode 1) -- the restatement of the sampled accept pass
(tests/spec_sample_ref.py) on the cases the GPU unit test runs, the conditions that let that test skip nothing, the ABI, and the host
layers (ChainRequest, generate(), the scheduler, the server, the inference entry) on recording stub engines."""
import numpy as np
import pytest
import torch

import chain_sampling_ref as C
import spec_ref as S
import spec_sample_ref as R
from test_chain_request_cpu import Calls
from test_sampling_filters_cpu import wrapper
from test_scheduler_cpu import Proc, make_model
from test_speculative_host_cpu import SpecGenStub, SpecStub
from zoomearth_amd.chain_request import ChainRequest
from zoomearth_amd.scheduler import ChainScheduler, Request

NAMES = [c[0] for c in R.CHAINS]


# ---------------------------------------------------------------- the restatement on the unit cases
@pytest.fixture(scope="module", params=[(v, k) for v, _ in R.SHAPES for k in R.KS], ids=lambda p: f"vocab{p[0]}-k{p[1]}")
def case(request):
    vocab, k = request.param
    return vocab, k, R.unit_case(vocab, k)


def test_the_cases_are_what_their_names_say(case):
    vocab, k, u = case
    n = dict(zip(NAMES, map(len, u["want"])))
    assert len(u["want"]) >= 6
    assert n["all accepted"] == k + 1 and u["want"][0][:k] == u["drafts"][0]
    assert n["none accepted"] == 1 and u["want"][1][0] != u["drafts"][1][0]
    assert n["middle stop"] == k // 2 + 1 and u["want"][2][:k // 2] == u["drafts"][2][:k // 2]
    assert n["room ends mid-draft"] == u["room"][4] == min(2, k) and u["want"][4] == u["drafts"][4][:min(2, k)]   # drafts hit: the room stops it
    assert n["greedy row"] == k + 1 and n["filtered"] == k + 1
    if u["eos"]:    # the EOS id is drawn AND drafted: an accepted id that still ends the walk, nothing behind it is emitted
        at = min(1, k - 1)
        assert u["fins"][3] and u["want"][3][-1] == u["eos"][0] == u["drafts"][3][at] and n["eos inside the draft"] == at + 1
    assert [f for i, f in enumerate(u["fins"]) if i != 3] == [False] * (len(NAMES) - 1)
    for c, ids in enumerate(u["want"]):     # every emitted id is marked, nothing else is
        extra = np.flatnonzero(u["seen_after"][c] != u["seen0"][c])
        assert set(extra) <= set(ids) and all(u["seen_after"][c][t] for t in ids)


def test_marking_an_accepted_id_seen_changes_the_next_rows_draw(case):
    vocab, k, u = case
    c = NAMES.index("seen flips a later row")
    rows = u["logits"][c * (k + 1):(c + 1) * (k + 1)]
    assert u["want"][c] == [11, 200] and u["penalty"][c] == 1.3
    # the same row under the seen-set BEFORE row 0's token was marked draws the draft id: the walk would have gone on
    tok, _ = R.draw(rows[1], u["seen0"][c], u["temperature"][c], 1.3, u["seed"][c], u["stream"][c], u["index0"][c] + 1)
    assert tok == 11


def test_no_draw_of_the_cases_sits_on_a_cdf_boundary_or_a_filter_margin(case):
    """The GPU unit test compares every token and skips none, so the cases must be decided: every draw at least chain_sampling_ref.GAP
    from a CDF boundary, no token inside the filter's float64 decision margins."""
    vocab, k, u = case
    assert min(u["gaps"]) >= C.GAP, min(u["gaps"])
    assert u["near"] and not any(u["near"])


def test_a_greedy_chain_is_the_greedy_accept_pass():
    rng = np.random.default_rng(2)
    rows = (rng.standard_normal((5, 300)) * 3).astype(np.float32)
    seen = (rng.random(300) < 0.1).astype(np.uint8)
    first = S.argmax(S.penalised(rows[0], seen, 1.3))
    for draft in ([first, 1, 2, 3], [299, 1, 2, 3], []):
        a, b = seen.copy(), seen.copy()
        want = S.accept(rows[:len(draft) + 1], draft, a, 1.3, (first,) if draft == [] else ())
        got = R.accept_sampled(rows[:len(draft) + 1], draft, b, 0.0, 1.3, eos_ids=(first,) if draft == [] else ())
        assert got[:2] == want and np.array_equal(a, b) and got[2] == [float("inf")] * len(want[0])


def test_the_draw_index_and_the_stream_are_the_rows_own():
    rng = np.random.default_rng(4)
    rows = (rng.standard_normal((3, 257)) * 2).astype(np.float32)
    seen = np.zeros(257, np.uint8)
    t0, _ = C.sample_row(rows[0], [], 1.0, 1.0, 9, 2, 5)
    ids, _, _ = R.accept_sampled(rows, [t0, 0], seen.copy(), 1.0, 1.0, 9, 2, 5)
    assert ids[0] == t0 and ids[1] == C.sample_row(rows[1], [t0], 1.0, 1.0, 9, 2, 6)[0]


# ---------------------------------------------------------------- the ABI
def test_the_abi_declares_the_two_entries():
    import os
    from zoomearth_amd import _lib
    header = open(os.path.join(os.path.dirname(__file__), "..", "include", "zoomearth.h")).read()
    for name in ("ze_seq_set_speculation_mode", "ze_op_spec_accept_sampled"):
        assert name in _lib._SIGS and f"int {name}(" in header, name
    res, args = _lib._SIGS["ze_seq_set_speculation_mode"]
    assert len(args) == len(_lib._SIGS["ze_seq_set_speculation"][1]) + 1          # ... plus the mode
    assert len(_lib._SIGS["ze_op_spec_accept_sampled"][1]) == len(_lib._SIGS["ze_op_spec_accept"][1]) + 7


# ---------------------------------------------------------------- ChainRequest
PROMPT = [11, 12, 13]


def test_install_order_and_the_switch():
    engine = Calls()
    ChainRequest(sampling=(True, 0.7, 3, 1.3), sampled=True, effective_penalty=1.3, top_k=5, top_p=0.9, speculative_tokens=4,
                 speculative_sampling=True).install(engine, 2, tuple(PROMPT))
    assert [c[0] for c in engine.log] == ["set_sampling", "set_sampling_filter", "set_speculation"]      # speculation last
    assert engine.log[-1] == ("set_speculation", (2, 4, PROMPT, 1, 3), dict(sampled=True))
    engine = Calls()
    ChainRequest(speculative_tokens=4).install(engine, 2, tuple(PROMPT))                                     # off: today's call
    assert engine.log == [("set_speculation", (2, 4, PROMPT, 1, 3), {})]


def test_the_conflicts_with_the_switch_on():
    on = dict(speculative_tokens=4, speculative_sampling=True)
    assert ChainRequest(sampled=True, top_k=5, top_p=0.9, min_p=0.1, **on).speculation_conflict() is None
    assert ChainRequest(sampled=True, speculative_tokens=4).speculation_conflict() == "sampling"
    assert ChainRequest(sampled=True, typical_p=0.9, **on).speculation_conflict() == "entropy filters"
    assert ChainRequest(sampled=True, logprobs=0, **on).speculation_conflict() == "logprobs"
    assert ChainRequest(sampled=True, presence_penalty=0.5, **on).speculation_conflict() == "logit adjustments"
    assert ChainRequest(sampled=True, stop_ids=[[5]], **on).speculation_conflict() == "token rules"
    assert ChainRequest(sampled=True, **on).speculation_conflict(grammar=True) == "guided decoding"


# ---------------------------------------------------------------- generate()
class SampledGenStub(SpecGenStub):
    def set_speculation(self, slot, k, prompt_ids=(), ngram_min=1, ngram_max=3, sampled=False):
        self.log.append(("speculation", slot, k, list(prompt_ids), ngram_min, ngram_max, sampled))

    def _apply_filter(self, slots, top_k, top_p, min_p):
        self.log.append(("filter", list(slots), top_k, top_p, min_p))

    def seq_fork(self, slot, into):
        self.log.append(("fork", slot, list(into)))


def gen(rows, max_seqs=2, **kw):
    m = wrapper()
    m.engine = SampledGenStub(max_seqs=max_seqs)
    out = m.generate(input_ids=torch.tensor(rows), max_new_tokens=3, **kw)
    return m.engine.log, out


def test_generate_with_the_keyword_samples_through_the_bursts():
    log, out = gen([[11, 50, 51]], prompt_lookup_num_tokens=4, prompt_lookup_sampling=True, do_sample=True, temperature=0.7, seed=5, top_k=5,
                   top_p=0.9)
    assert [c for c in log if c[0] == "speculation"] == [("speculation", 0, 4, [11, 50, 51], 1, 3, True)]
    (call,) = [c for c in log if c[0] == "generate_speculative"]
    assert call[3]["do_sample"] is True and call[3]["temperature"] == 0.7 and call[3]["seed"] == 5
    assert [c for c in log if c[0] == "filter"] == [("filter", [0], 5, 0.9, 0.0)]
    assert not [c for c in log if c[0] == "generate"] and out.shape == (1, 6)
    # greedy with the keyword: the sampled mode's setter, nothing of the call's sampling
    log, _ = gen([[11, 50, 51]], prompt_lookup_num_tokens=4, prompt_lookup_sampling=True)
    (call,) = [c for c in log if c[0] == "generate_speculative"]
    assert "do_sample" not in call[3] and [c[6] for c in log if c[0] == "speculation"] == [True]
    # without the keyword a greedy call is today's call
    log, _ = gen([[11, 50, 51]], prompt_lookup_num_tokens=4)
    assert [c for c in log if c[0] == "speculation"] == [("speculation", 0, 4, [11, 50, 51], 1, 3, False)]


def test_generate_num_return_sequences_inside_the_row_budget():
    log, out = gen([[11, 50, 51]], max_seqs=4, prompt_lookup_num_tokens=4, prompt_lookup_sampling=True, do_sample=True, num_return_sequences=3)
    assert out.shape == (3, 6) and [c[1] for c in log if c[0] == "speculation"] == [0, 1, 2]
    (call,) = [c for c in log if c[0] == "generate_speculative"]
    assert call[1] == [0, 1, 2] and call[3]["do_sample"] is True
    with pytest.raises(ValueError, match="num_return_sequences"):      # 33 completions need 66 rows: today's error
        gen([[11, 50, 51]], max_seqs=64, prompt_lookup_num_tokens=4, prompt_lookup_sampling=True, do_sample=True, num_return_sequences=33)


@pytest.mark.parametrize("kw", [dict(do_sample=True), dict(do_sample=True, num_return_sequences=2)])
def test_generate_without_the_keyword_refuses_as_before(kw):
    with pytest.raises(ValueError, match="greedy speculative decoding"):
        gen([[11, 50, 51]], prompt_lookup_num_tokens=4, **kw)


@pytest.mark.parametrize("kw", [dict(logprobs=0), dict(no_repeat_ngram_size=2), dict(presence_penalty=0.5), dict(stop_token_ids=[5]),
                                dict(typical_p=0.9), dict(epsilon_cutoff=0.01), dict(eta_cutoff=0.01), dict(bad_words_ids=[[4]])])
def test_generate_with_the_keyword_still_refuses_what_stays_excluded(kw):
    with pytest.raises(ValueError):
        gen([[11, 50, 51]], prompt_lookup_num_tokens=4, prompt_lookup_sampling=True, do_sample=True, **kw)


# ---------------------------------------------------------------- the scheduler, the server, the inference entry
class SampledSpecStub(SpecStub):
    def set_speculation(self, slot, k, prompt_ids=(), ngram_min=1, ngram_max=3, sampled=False):
        super().set_speculation(slot, k, prompt_ids, ngram_min, ngram_max)
        self.log.append(("sampled", slot, sampled))

    def set_sampling(self, slot, **kw):
        self.log.append(("set_sampling", slot, kw))


def test_resolve_with_the_switch_on_and_off():
    model = make_model()
    model.engine = SampledSpecStub(max_seqs=4)
    sampled = dict(prompt="1 2", images=[], do_sample=True, temperature=0.5)
    off = ChainScheduler(model, Proc(), burst=4, share_prefix=False, speculative_tokens=4)
    assert off._resolve(Request(**sampled)).speculative_tokens == 0                       # as today: rides with one row
    assert off._resolve(Request(speculative_sampling=True, **sampled)).speculative_tokens == 4
    with pytest.raises(ValueError):
        off._resolve(Request(speculative_tokens=4, **sampled))
    on = ChainScheduler(model, Proc(), burst=4, share_prefix=False, speculative_tokens=4, speculative_sampling=True)
    got = on._resolve(Request(top_p=0.9, **sampled))
    assert got.speculative_tokens == 4 and got.speculative_sampling and got.sampled
    assert on._resolve(Request(speculative_sampling=False, **sampled)).speculative_tokens == 0
    assert on._resolve(Request(typical_p=0.9, **sampled)).speculative_tokens == 0         # an entropy filter stays excluded
    assert on._resolve(Request(stop_ids=[[5]], **sampled)).speculative_tokens == 0
    assert on._resolve(Request(prompt="1 2", images=[])).speculative_tokens == 4


def test_the_scheduler_installs_the_sampled_mode_and_keeps_the_row_budget():
    model = make_model(max_seqs=10)
    model.engine = SampledSpecStub(max_seqs=10)
    sched = ChainScheduler(model, Proc(), burst=4, share_prefix=False, speculative_tokens=8, speculative_sampling=True)
    for i in range(10):
        sched.submit(Request(prompt=f"{2 * i + 11} 60 61", images=[], max_new_tokens=12, do_sample=True, temperature=0.5, tag=i))
    sched.run()
    eng = model.engine
    assert [c[2] for c in eng.log if c[0] == "speculation"] == [8, 8, 8, 8, 8, 8, 6]          # the budget of test_speculative_host_cpu
    assert all(c[2] for c in eng.log if c[0] == "sampled") and max(eng.rows_seen) == 64


def test_the_server_flag():
    from zoomearth_amd import serve
    srv = serve.ChatServer(make_model(), Proc(), "stub", speculative_ngram=4, speculative_sampling=True)
    assert srv.speculative_sampling is True
    assert serve.ChatServer(make_model(), Proc(), "stub", speculative_ngram=4).speculative_sampling is False


def test_the_inference_entry_refuses_the_row_streaming_family_at_start():
    import importlib.util
    import os
    spec = importlib.util.spec_from_file_location("ze_infer_entry", os.path.join(os.path.dirname(__file__), "..", "src", "eval", "infer.py"))
    infer = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(infer)
    assert infer.speculative_kwargs(0, 256) == {}
    assert infer.speculative_kwargs(4, 64) == dict(speculative_tokens=4, speculative_sampling=True)
    with pytest.raises(ValueError, match="row-streaming"):
        infer.speculative_kwargs(4, 65)
    with pytest.raises(ValueError):
        infer.speculative_kwargs(9, 16)
