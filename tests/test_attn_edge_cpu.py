"""CPU: the planted attention inputs (tests/attn_edge_ref.py) prove their own power.  For every case tests/test_gpu_attention_edges.py
runs, every mutant that applies to it -- the float64 result over a WRONG set of rows -- and every probed (query, head) the mutant
affects: max |mutant - reference| >= 16 x the bound the GPU test applies to that row.  A case without an affected row for an
applicable mutant FAILS (it is not skipped): the GPU test would be blind to that fault there.  One more test documents the gap
these inputs close: on the N(0, 1) inputs of the existing float64 tests a dropped key moves the reference by less than their bound."""
import numpy as np
import pytest

import attn_edge_ref as R


def _check(case_name, probes, mutants_of, result, bound_of):
    """-> {mutant: smallest move / bound over its affected probes}; asserts the 16 x condition and the cap"""
    power = {}
    for p in probes:
        ref = result(p)
        for name, mut in mutants_of(p).items():
            power.setdefault(name, [])
            if not p.affected(mut):
                continue
            move = float(np.abs(result(p, mut) - ref).max())
            power[name].append(move / bound_of(p))
            assert move >= R.POWER * bound_of(p), (case_name, name, p.where, p.head, p.pair, p.mode, move, bound_of(p))
    for name, moves in power.items():
        assert moves, f"{case_name}: no probed row is affected by the mutant '{name}'"
    return {name: min(moves) for name, moves in power.items()}


@pytest.mark.parametrize("D,causal,ci,kvh", R.flash_cases())
def test_flash_inputs_tell_every_mutant_apart(D, causal, ci, kvh):
    c = R.flash_case(D, causal, ci, kvh)
    assert c.bound <= 2.0 ** -6 * R.VMAX and len(c.probes) >= 4 * 2 * (len(c.cu) - 1) - 8
    power = _check((D, causal, ci, kvh), c.probes, c.mutants, c.result, lambda p: c.bound)
    want = {"drop the last visible key", "add the first invisible key", "drop the first key", "add the previous segment's last key",
            "drop the last key of a key tile", "read the last key of a key tile twice", "drop the first key of the next key tile",
            "read the first key of the next key tile twice", "another kv head"}
    assert set(power) == want, want ^ set(power)
    print(f"flash D {D} causal {causal} cu {ci} kv heads {kvh}: smallest move / bound {min(power.values()):.1f} "
          f"({min(power, key=power.get)})")


def test_decode_inputs_tell_every_mutant_apart():
    worst = {}
    for c in R.decode_chains():
        probes = [p for r in range(c.passes) for p in c.probes(r)]
        power = _check(("decode", c.ctx, c.split), probes, lambda p: c.mutants(), c.result, lambda p: c.bound[p.kvh])
        assert {"drop the last key", "read the dead rows behind ctx", "drop row 0", "another kv head"} <= set(power)
        for part in (64, 192, 384):                                       # every partition that cuts this context has its four mutants
            assert (c.ctx >= part) == (f"{part}-key parts: drop the last key of a part" in power), (c.ctx, part)
        assert ("split row: read the last key of a part twice" in power) == (c.split > 0)
        for name, v in power.items():
            worst[name] = min(worst.get(name, np.inf), v)
        assert max(c.bound) <= 2.0 ** -7 * R.VMAX and c.dead and c.dead[0] == c.ctx + 1
    assert any(c.split and "split parts: drop the first key of the next part" in c.mutants() for c in R.decode_chains())
    print("decode: smallest move / bound per mutant:", {k: round(v, 1) for k, v in sorted(worst.items())})


def test_prefix_hint_inputs_tell_every_mutant_apart():
    for a, b in R.prefix_pairs():
        power = _check(("prefix", b.own_from), b.probes(0), lambda p: b.mutants(), b.result, lambda p: b.bound[p.kvh])
        assert {"prefix rows from the chain's own slot", "the first own row from the holder's slot",
                "prefix end: drop the last key of a part", "read the dead rows behind ctx"} <= set(power)
        # the premise of the hint does NOT hold on purpose: the chain's own rows below `rows` differ from the holder's
        assert not np.array_equal(b.k[:, :b.own_from], a.k[:, :b.own_from]) and np.array_equal(b.kt[:, :b.own_from], a.k[:, :b.own_from])
        assert np.array_equal(b.kt[:, b.own_from:b.ctx + 1], b.k[:, b.own_from:b.ctx + 1])
        print(f"prefix rows {b.own_from}: smallest move / bound {min(power.values()):.1f}")


def test_diffuse_inputs_cannot_see_a_dropped_key():
    """The gap: on the very inputs of tests/test_gpu_ops.py::test_attention's ViT case (80, 16, 16, [0, 1296]) -- q, k, v ~ N(0, 1) in
    bf16, one full segment of 1296 rows -- the float64 result WITHOUT the segment's last key differs from the reference by less than
    the bound that test applies, on each of 40 (query, head) rows spread over the segment: a kernel one key short at the segment end
    passes it."""
    L, d, heads = 1296, 80, 16
    q, k, v = R.rnd(6, (L, heads, d)), R.rnd(7, (L, heads, d)), R.rnd(8, (L, heads, d))
    rows = [(i * 33 % L, i % heads) for i in range(40)]
    want = np.stack([R.attend(q[i, h], k[:, h], v[:, h], range(L)) for i, h in rows])
    short = np.stack([R.attend(q[i, h], k[:, h], v[:, h], range(L - 1)) for i, h in rows])
    bound = 2.0 ** -6 * max(1.0, float(np.abs(want).max()))
    move = float(np.abs(short - want).max())
    print(f"d {d}, L {L}: dropping the last key moves the float64 result by {move:.4f}; the existing bound is {bound:.4f}")
    assert move < bound
