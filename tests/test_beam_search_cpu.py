"""CPU: the float64 restatement of beam search (tests/beam_ref.py) reproduces the installed transformers on the recorded cases
(tests/golden/beam_search.npz, made by tests/golden/make_beam_fixture.py), the decision margin TAU is derived from HF's own fp32
error, and the rules that are this project's own -- slot assignment, tie rule, "best B non-EOS" -- hold on random inputs."""
import os

import numpy as np
import pytest

import beam_ref as R

HERE = os.path.dirname(os.path.abspath(__file__))
EARLY = {0: False, 1: True, 2: "never"}


@pytest.fixture(scope="module")
def fx():
    return np.load(os.path.join(HERE, "golden", "beam_search.npz"))


def replay(fx, name):
    """The restatement driven by the logits HF ranked; returns (group, per-step outputs)."""
    B, early, max_new = (int(x) for x in fx[f"params_{name}"])
    lp, pen = (float(x) for x in fx[f"floats_{name}"])
    logits = fx[f"logits_{name}"].astype(np.float32)
    g = R.BeamGroup(B, logits.shape[2], list(fx["eos_token_ids"]), max_new, lp, EARLY[early], pen, prompt_ids=fx[f"prompt_{name}"])
    steps = []
    for t in range(logits.shape[0]):
        assert not g.done, f"{name}: the restatement stopped before HF did (step {t})"
        by_slot = logits[t][np.asarray(g.rank)]   # HF's rows are in beam order, the restatement's by slot
        steps.append(g.step(by_slot))
    assert g.done, f"{name}: HF stopped after {logits.shape[0]} steps, the restatement goes on"
    return g, steps


def test_fixture_covers_the_cases(fx):
    names = list(fx["cases"])
    par = np.array([fx[f"params_{n}"] for n in names])
    fl = np.array([fx[f"floats_{n}"] for n in names])
    assert set(par[:, 0]) == {2, 4} and set(par[:, 1]) == {0, 1, 2}
    assert set(fl[:, 0]) == {0.0, 1.0, 2.0} and set(fl[:, 1]) == {1.0, 1.3}
    assert all(fx[f"logits_{n}"].shape[0] <= 12 for n in names)
    eos = list(fx["eos_token_ids"])
    with_eos = sum(bool(np.isin(fx[f"sequences_{n}"][:, len(fx[f"prompt_{n}"]):], eos).any()) for n in names)
    assert with_eos >= 2, "an EOS hypothesis must finish in at least two cases"
    assert os.path.getsize(os.path.join(HERE, "golden", "beam_search.npz")) < 512 * 1024


def test_restatement_reproduces_hf(fx):
    pad = int(fx["pad_token_id"])
    for name in fx["cases"]:
        g, _ = replay(fx, name)
        B = g.B
        want_seq, want_sc, want_bi = fx[f"sequences_{name}"], fx[f"scores_{name}"], fx[f"beam_indices_{name}"]
        P = len(fx[f"prompt_{name}"])
        res = g.results(B)
        width = want_seq.shape[1] - P
        assert max(len(r["tokens"]) for r in res) == width, name
        for r, (ws, wsc, wbi) in zip(res, zip(want_seq, want_sc, want_bi)):
            n = len(r["tokens"])
            assert list(ws[P:P + n]) == r["tokens"] and all(ws[P + n:] == pad), name
            assert list(wbi[:n]) == r["bidx"] and all(wbi[n:] == -1), name
            assert abs(r["score"] - float(wsc)) <= R.MEASURED_HF_FP32_VS_F64, (name, r["score"], float(wsc))


def test_tau_is_derived_from_hf_fp32(fx):
    """TAU = 16 x the largest |HF fp32 score - float64 restatement| seen on the fixture; the constant in beam_ref.py is that value
    (rounded up, by less than a factor 2), and every step of every case is decided under it."""
    worst = 0.0
    for name in fx["cases"]:
        g, steps = replay(fx, name)
        for r, wsc in zip(g.results(g.B), fx[f"scores_{name}"]):
            worst = max(worst, abs(r["score"] - float(wsc)))
        for t, s in enumerate(steps):
            assert s["decided"], f"{name} step {t}: margin {s['margin']:.3g} <= TAU {R.TAU:.3g}"
    print(f"max |HF fp32 - float64| = {worst:.3e}, TAU = {R.TAU:.3e}")
    assert worst <= R.MEASURED_HF_FP32_VS_F64 <= 2.0 * worst + 1e-12
    assert R.TAU == 16 * R.MEASURED_HF_FP32_VS_F64


def test_slot_assignment_is_hazard_free():
    rng = np.random.default_rng(7)
    for _ in range(10000):
        B = int(rng.integers(1, 17))
        parents = [int(x) for x in rng.integers(0, B, size=B)]
        if rng.random() < 0.1:
            parents = list(range(B))
        slot_of = R.assign_slots(parents)
        assert sorted(slot_of) == list(range(B))   # every surviving hypothesis ends in exactly one slot
        sources = {pj for k, pj in enumerate(parents) if slot_of[k] != pj}   # slots read by a copy
        dests = {slot_of[k] for k, pj in enumerate(parents) if slot_of[k] != pj}   # slots written by one
        assert not (sources & dests)
        for pj in set(parents):   # a parent with children keeps its first child
            first = parents.index(pj)
            assert slot_of[first] == pj
        moved = [k for k, pj in enumerate(parents) if slot_of[k] != pj]
        assert [slot_of[k] for k in moved] == sorted(slot_of[k] for k in moved)   # free slots ascending, children in order


def test_planted_tie_follows_the_flat_index():
    V, B = 64, 3
    rng = np.random.default_rng(3)
    logits = rng.normal(size=(B, V)).astype(np.float32)
    g = R.BeamGroup(B, V, [], 4)
    logits[0, [40, 7, 23]] = 9.0   # three equal logits in the one row that counts at the first step
    out = g.step(logits)
    by_rank = [out["token"][out["rank"].index(k)] for k in range(B)]
    assert by_rank == [7, 23, 40]
    # second step: the same value in two rows whose running scores are bit-equal -- the lower beam index comes first
    assert g.score[0] == g.score[1] == g.score[2]
    logits = np.full((B, V), -3.0, np.float32)
    for j in range(B):
        logits[j, 11] = 5.0
    out = g.step(logits)
    assert sorted(out["token"]) == [11, 11, 11]
    # each beam extended itself: beam k's child is beam k again (flat index beam * V + 11 ascending)
    assert all(g.bidx[j][-1] == g.rank[j] for j in range(B))


def test_best_non_eos_equals_hf_masking():
    rng = np.random.default_rng(5)
    for _ in range(300):
        B, V = int(rng.integers(1, 9)), int(rng.integers(24, 80))
        n_eos = int(rng.integers(0, 4))
        eos = [int(x) for x in rng.choice(V, size=n_eos, replace=False)]
        sc = rng.normal(size=B * V)
        if eos and rng.random() < 0.7:   # push EOS candidates to the top: the case the (1 + n_eos) * B bound is about
            for b in range(B):
                sc[b * V + np.asarray(eos)] += 6.0
        if rng.random() < 0.3:
            sc = np.round(sc, 1)   # ties
        assert R.best_non_eos(sc, V, eos, B) == R.hf_equivalent_top(sc, V, eos, B)


def test_model_beam_search_argument_errors():
    """HF's argument errors, raised before the engine is touched."""
    from zoomearth_amd.config import ModelConfig
    from zoomearth_amd.modeling import ZoomEarthForConditionalGeneration
    m = ZoomEarthForConditionalGeneration(ModelConfig.tiny(), None)
    for bad in (dict(num_beams=1), dict(num_beams=True), dict(num_beams=2, num_return_sequences=3), dict(num_beams=2, num_return_sequences=0),
                dict(num_beams=17), dict(num_beams=2, do_sample=True), dict(num_beams=2, top_k=5), dict(num_beams=2, guided_regex="a+")):
        with pytest.raises(ValueError):
            m.beam_search(input_ids=None, max_new_tokens=4, **bad)
    with pytest.raises(NotImplementedError):
        m.generate(input_ids=None, num_beams=2)


def test_beam_host_checks_under_asan_ubsan(tmp_path):
    """The host-only part of beam search (zoomearth_amd/csrc/ze_index.cpp: argument and table checks, divisor table, live groups),
    built with -fsanitize=address,undefined into a stand-alone program with its own main and run: any report aborts it."""
    import shutil
    import subprocess
    root = os.path.dirname(HERE)
    cxx = shutil.which("g++") or shutil.which("clang++")
    assert cxx, "a host C++ compiler is needed for the sanitizer build"
    exe = str(tmp_path / "ze_beam_host_san")
    r = subprocess.run([cxx, "-O1", "-g", "-std=c++17", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                        "-I", os.path.join(root, "zoomearth_amd", "csrc"), os.path.join(root, "zoomearth_amd", "csrc", "ze_index.cpp"),
                        os.path.join(HERE, "cabi_san", "ze_beam_host_san.cpp"), "-o", exe], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-4000:]
    r = subprocess.run([exe], capture_output=True, text=True, timeout=120,
                       env=dict(os.environ, ASAN_OPTIONS="detect_leaks=1:halt_on_error=1:abort_on_error=1", UBSAN_OPTIONS="halt_on_error=1"))
    assert r.returncode == 0 and "sanitized beam host checks ok" in r.stdout, (r.stdout[-2000:], r.stderr[-4000:])
