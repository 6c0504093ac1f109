"""GPU: every public GEMM launcher through ze_op_gemm with the operands the engine gives them -- leading dimensions larger than the
extent, the residual epilogue out of place and in place, the output row table, the fp32 epilogue, both tails (wide-store and plain) of
the ring and eight-phase kernels -- on the exact operands of tests/gemm_operand_ref.py, whose expected output is ONE bit pattern
whatever the accumulation order.  NONE / RESIDUAL / F32: the whole C buffer, sentinels included, equals the expected bits
(torch.equal); GELU / SWIGLU: the bounds of tests/test_gpu_ops.py on the written elements and untouched sentinel bits everywhere else.
Every case runs twice (same bits); every RESIDUAL case has its in-place twin (r and c the same tensor: the same bits).
tests/test_gemm_operands_cpu.py shows that these inputs tell every indexing and rounding fault apart.  Which kernel each case id names
was read from the launch rules of ze_gemm.hip; profiles/gemm_operands_kernel_stats.csv records what this file launched."""
import functools

import numpy as np
import pytest
import torch

import gemm_operand_ref as R
from gpu_util import tiny_engine  # noqa: F401

pytestmark = pytest.mark.gpu
ZE_ERR_INVALID = -1


def _dev_bf16(values):
    """bf16-exact float64 values -> a bf16 device tensor of those bits"""
    return torch.from_numpy(R.bf16_bits(values).view(np.int16)).cuda().view(torch.bfloat16)


@functools.lru_cache(maxsize=2)
def _dev_w(c_key):
    return _dev_bf16(R.operands(c_key).Wbuf)


def _w_key(c):  # the cases that share a W buffer (same N, K, scale): the largest upload of a case
    return R.Case("w", 0, R.NONE if c.exact else R.GELU, 8, c.N, c.K)


def _sentinel_c(c, extra=0):
    if c.epi == R.F32:
        flat = torch.full(((c.MC + R.GUARD) * c.ldc + extra,), R.SENTINEL_BITS << 16, dtype=torch.int32, device="cuda").view(torch.float32)
    else:
        flat = torch.full(((c.MC + R.GUARD) * c.ldc + extra,), R.SENTINEL_BITS, dtype=torch.int16, device="cuda").view(torch.bfloat16)
    return flat


def _ints(t):
    return t.view(torch.int32 if t.dtype == torch.float32 else torch.int16)


def _run(e, c, o, da, dw, db, dr, rows, inplace=False):
    """one call on a fresh sentinel-filled C -> the whole C buffer [MC + GUARD, ldc] (a view c_off elements into its allocation)"""
    flat = _sentinel_c(c, c.c_off)
    cbuf = flat[c.c_off:]
    ldr = c.ldr
    if inplace:   # r and c the same tensor: the residual sits in the output rows, ldr = ldc
        cbuf.view(c.MC + R.GUARD, c.ldc)[:c.M, :c.N] = dr.view(-1, c.ldr)[:c.M, :c.N]
        dr, ldr = cbuf, c.ldc
    try:
        for k, v in c.knobs:
            e.lib.ze_tune(k, v)
        st = e.op_gemm(c.launcher, c.epi, da, c.lda, dw, c.ldw, db, dr if c.epi == R.RESIDUAL else None, ldr, cbuf, c.ldc, rows,
                       c.M, c.N, c.K)
    finally:
        for k, _ in c.knobs:
            e.lib.ze_tune(k, 0)
    assert st == 0, (st, e.lib.ze_last_error(e.h))
    torch.cuda.synchronize()
    if c.c_off:
        assert (_ints(flat[:c.c_off]) == _ints(_sentinel_c(c)[:1])).all(), "the elements in front of C were written"
    return cbuf.view(c.MC + R.GUARD, c.ldc)


def _check(e, c):
    o = R.operands(c)
    want, tol = R.result(c)
    da, db = _dev_bf16(o.Abuf), _dev_bf16(o.biasbuf) if c.bias else None
    dw = _dev_w(_w_key(c)) if c.N * c.K >= 1 << 22 else _dev_bf16(o.Wbuf)
    dr = _dev_bf16(o.Rbuf) if c.epi == R.RESIDUAL else None
    rows = torch.from_numpy(o.c_rows).cuda() if o.c_rows is not None else None
    got = _run(e, c, o, da, dw, db, dr, rows)
    again = _run(e, c, o, da, dw, db, dr, rows)
    assert torch.equal(_ints(got), _ints(again)), "two runs of the same call differ"
    if tol is None:
        want_t = torch.from_numpy(R.c_bits(c, want)).cuda()
        if not torch.equal(_ints(got), want_t):
            bad = (_ints(got) != want_t).nonzero()
            i, j = (int(x) for x in bad[0])
            pytest.fail(f"{len(bad)} of {want_t.numel()} elements of the C buffer differ; first at buffer row {i}, column {j} "
                        f"(M {c.M}, N {c.N}, ldc {c.ldc}): got {float(got[i, j])}, expected {want[i, j]}")
    else:
        g = got.float().cpu().numpy().astype(np.float64)
        written = tol > 0
        err = np.abs(g - want)
        print(f"{c.id}: max error / bound {float((err[written] / tol[written]).max()):.3f}")
        assert (err[written] <= tol[written]).all(), float((err[written] / tol[written]).max())
        sent = torch.from_numpy(~written).cuda()
        assert (_ints(got)[sent] == R.SENTINEL_BITS).all(), "a sentinel of C was overwritten"
    if c.epi == R.RESIDUAL and c.plain != "rows":   # (with a row table the output rows are other rows than the residual's)
        twin = _run(e, c, o, da, dw, db, dr, rows, inplace=True)
        assert torch.equal(_ints(twin), _ints(got)), "the in-place run (r == c) differs from the out-of-place run"
    return got


@pytest.mark.parametrize("c", R.cases(), ids=lambda c: c.id)
def test_gemm_operands(tiny_engine, c):
    _check(tiny_engine, c)


@pytest.mark.parametrize("c", R.misaligned_cases(), ids=lambda c: c.id)
def test_gemm_misaligned_output_and_residual(tiny_engine, c):
    """ldc = N + 3 (N = 130), C one element into its allocation, ldr odd: the plain tail, held to the expected bits like every case.
    The N = 136 cases (C offset, ldr odd) must also give the bits of the run with ldc = N + 16, ldr = N + 8 and C on a 16-byte boundary,
    which takes the wide-store tail where the form has one; at N = 130 every run is plain (N % 8), so there is no such twin."""
    got = _check(tiny_engine, c)
    if c.N % 8 == 0:
        ref = _check(tiny_engine, R.Case(c.form, c.launcher, c.epi, c.M, c.N, c.K, c.knobs))
        assert torch.equal(_ints(got)[:c.M, :c.N], _ints(ref)[:c.M, :c.N])


def test_gemm_refusals(tiny_engine):
    """everything a launcher does not take: ZE_ERR_INVALID, and the sentinel-filled C unchanged"""
    e = tiny_engine
    M, N, K = 16, 64, 64
    a = torch.zeros((M + 8) * (K + 8), dtype=torch.bfloat16, device="cuda")
    w = torch.zeros((N + 8) * (K + 24), dtype=torch.bfloat16, device="cuda")
    b = torch.zeros(N + 24, dtype=torch.bfloat16, device="cuda")
    r = torch.zeros((M + 8) * (N + 8), dtype=torch.bfloat16, device="cuda")
    rows = torch.arange(M, dtype=torch.int32, device="cuda")
    big_k = torch.zeros(24 * (4128 + 24), dtype=torch.bfloat16, device="cuda")
    ok = dict(launcher=0, epi=R.NONE, a=a, lda=K + 8, w=w, ldw=K + 24, bias=b, r=r, ldr=N + 8, ldc=N + 16, c_rows=None, m=M, n=N, k=K)
    refused = {
        "a null": dict(a=None), "w null": dict(w=None), "c null": dict(c=None), "r null under RESIDUAL": dict(epi=R.RESIDUAL, r=None),
        "lda below K": dict(lda=K - 8), "ldw below K": dict(ldw=K - 8), "ldc below N": dict(ldc=N - 1),
        "ldc below N / 2 (SWIGLU)": dict(epi=R.SWIGLU, ldc=N // 2 - 1), "ldr below N": dict(epi=R.RESIDUAL, ldr=N - 1),
        "K % 8": dict(k=60), "p8: K % 64": dict(launcher=2, k=32), "unknown launcher": dict(launcher=7), "unknown epilogue": dict(epi=5),
        "SWIGLU with N % 32": dict(epi=R.SWIGLU, n=48),
        "frag: N % 16": dict(launcher=5, n=56), "frag: K % 32": dict(launcher=5, k=48), "frag: M > 64": dict(launcher=5, m=65),
        "frag: K > 4096": dict(launcher=5, m=8, n=16, k=4128, a=big_k, lda=4128 + 8, w=big_k, ldw=4128 + 24),
        "frag: GELU": dict(launcher=5, epi=R.GELU), "oneshot: N % 16": dict(launcher=6, n=56), "oneshot: M > 64": dict(launcher=6, m=65),
        "oneshot: K % 32": dict(launcher=6, k=48), "oneshot: GELU": dict(launcher=6, epi=R.GELU),
        "oneshot: SWIGLU": dict(launcher=6, epi=R.SWIGLU), "oneshot: F32": dict(launcher=6, epi=R.F32),
    }
    for L in (3, 4, 5, 6):
        refused[f"c_rows on launcher {L}"] = dict(launcher=L, c_rows=rows)
    for name, change in refused.items():
        c = torch.full((128 * 128,), R.SENTINEL_BITS, dtype=torch.int16, device="cuda")
        args = dict(ok, c=c.view(torch.bfloat16))
        args.update(change)
        st = e.op_gemm(**args)
        torch.cuda.synchronize()
        assert st == ZE_ERR_INVALID, (name, st)
        assert (c == R.SENTINEL_BITS).all(), name
    c = torch.full((128 * 128,), R.SENTINEL_BITS, dtype=torch.int16, device="cuda")   # and the unchanged arguments are taken
    assert e.op_gemm(**dict(ok, c=c.view(torch.bfloat16))) == 0
    torch.cuda.synchronize()
    assert not (c == R.SENTINEL_BITS).all()
