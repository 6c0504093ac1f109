"""CPU: the exact GEMM operands (tests/gemm_operand_ref.py) prove their own power.  For every case tests/test_gpu_gemm_operands.py runs
and every mutant that applies to it -- the buffer a kernel with ONE indexing or rounding fault would leave -- the mutant differs from
the truth: in at least 5 % of the written elements' count where the GPU test compares bits, by at least 16 x the GPU test's bound
somewhere where it compares within a bound (GELU, SWIGLU).  A case whose applicable mutant changes nothing FAILS (it is not skipped):
the GPU test would be blind to that fault there.  One more test documents the gap these inputs close."""
import numpy as np
import pytest

import gemm_operand_ref as R
from oracle import prng
from oracle.qwen25vl import bf16_round

# one CPU case per distinct set of operands and mutants: the launcher, the form and the knobs do not change what is expected
_SEEN = {}
for _c in R.cases() + R.misaligned_cases():
    _SEEN.setdefault((_c.epi, _c.M, _c.N, _c.K, _c.plain, _c.ksplit, _c.ldr_odd), _c)
CPU_CASES = list(_SEEN.values())


def _powers(c):
    names = R.mutants(c)
    assert {"A read with lda := K", "W read with ldw := K", "the last K-tile dropped", "C written with ldc := N"} <= set(names)
    if c.epi == R.RESIDUAL:
        assert {"R taken from row r + 1", "residual added before the first rounding", "R read with ldr := N", "R read with ldr := ldc",
                "residual added before the bias rounding, bias dropped"} <= set(names)
    if c.plain == "rows":
        assert "c_rows ignored" in names and (c.epi != R.RESIDUAL or "R taken at the output row c_rows[r]" in names)
    if c.ksplit > 1:
        assert "split-K: slice 0 added twice, the last slice dropped" in names
    return {n: R.power(c, n) for n in names}


@pytest.mark.parametrize("c", CPU_CASES, ids=lambda c: c.id)
def test_inputs_tell_every_mutant_apart(c):
    p = _powers(c)
    worst = min(p, key=p.get)
    print(f"{c.id}: smallest {'share' if c.exact else 'move / bound'} {p[worst]:.3f} ({worst})")
    need = R.POWER_SHARE if c.exact else R.POWER_TOL
    for name, v in p.items():
        assert v >= need, (c.id, name, v)


def test_gaussian_operands_cannot_see_the_order_of_the_residual_roundings():
    """The gap: on the N(0, 1) x N(0, 0.05) operands of tests/test_gpu_ops.py::test_linear at (130, 200, 96), with a residual of the
    sum's own scale.  The right result bf16(R + bf16(v)) rounds twice, so the tightest bound a tolerance test can put on it is
    test_linear's bound on v (1.5 bf16 ulp of max(|v|, scale)) plus the output rounding (2^-8 of the result at most) -- test_linear's
    own bound taken on R + v alone is broken by the RIGHT result wherever R cancels v (asserted and printed below).  Inside that bound lies
    bf16(R + v) as well, everywhere: a kernel that adds the residual before the first rounding passes any tolerance test."""
    m, n, k = 130, 200, 96

    def rnd(seed, shape, std=1.0):
        return bf16_round(prng.normal_ih4(seed, int(np.prod(shape)), std)).reshape(shape).astype(np.float64)

    a, w, b = rnd(1, (m, k)), rnd(2, (n, k), 0.05), rnd(3, (n,), 0.5)
    r = rnd(4, (m, n), 0.5)
    v = a @ w.T + b
    want = r + v
    bound = (1.5 * 2.0 ** -8 + 1e-6) * np.maximum(np.abs(v), 0.05 * np.sqrt(k) * 0.05) + 2.0 ** -8 * np.abs(want)
    two, one = R.bf16r(r + R.bf16r(v)), R.bf16r(r + v)
    e2, e1 = np.abs(two - want) / bound, np.abs(one - want) / bound
    own = np.abs(two - want) / np.maximum(np.abs(want), 0.05 * np.sqrt(k) * 0.05) / 2.0 ** -8   # test_linear's measure, in its ulps
    print(f"test_linear's bound on R + v alone: the right result reaches {own.max():.1f} ulp (allowed 1.5), {(own > 1.5).sum()} elements outside")
    assert own.max() > 1.5
    print(f"bf16(R + bf16(v)): {e2.max():.2f} of the bound, bf16(R + v): {e1.max():.2f} of the bound; "
          f"{(two != one).mean():.1%} of the outputs differ between them")
    assert e2.max() <= 1.0 and e1.max() <= 1.0 and (two != one).mean() > 0.05
