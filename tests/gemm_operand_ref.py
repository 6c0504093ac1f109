"""Inputs, expected bits and mutants for tests/test_gpu_gemm_operands.py (ze_op_gemm: the public GEMM launchers with strided operands,
the residual epilogue and the output row table).  numpy only.

Exact operands.  A and W hold integers in [-15, 15] (oracle.prng); W is times 2^wexp.  Every partial sum is an integer multiple of
2^wexp below 2^24 of them (|sum| <= 225 K), so EVERY fp32 accumulation order -- MFMA grouping, K-tile order, split-K slab sums -- gives
the same exact value, and the expected output of the NONE / RESIDUAL / F32 epilogues is one fixed bit pattern:
    NONE      bf16(acc + bias)
    RESIDUAL  bf16(R + bf16(acc + bias))
    F32       the fp32 copy of bf16(acc + bias)
bias and R hold 8-bit integers times `unit` = 2^(floor(log2 s) - 6), s = 80 sqrt(K) 2^wexp the nominal deviation of a sum (a product of
two such integers has variance 80^2): 8 at K = 64 with W unscaled.  The module asserts in float64 that |acc| < 2^24 units of 2^wexp and
that acc + bias and R + bf16(acc + bias) are exact in fp32 (`operands`).  GELU / SWIGLU take the same operands with wexp chosen for an
O(1) pre-activation (exact, again) and the bounds of tests/test_gpu_ops.py, because silu_f / erff are approximations.

Poison and sentinels.  Every device buffer is larger than its logical operand: the columns behind K (A, W) and N (R), 8 whole rows
behind the last one, and the bias entries behind N hold the finite bf16 value 2^60 -- a masked lane that multiplies it by zero stays
right, a kernel that takes it for data is off by tens of orders of magnitude.  C is pre-filled with a sentinel bit pattern, and the
expected buffer holds it wherever the call must not write: the columns behind the output width, the rows behind M (or not in c_rows)
and the 8 guard rows -- so one comparison of the WHOLE buffer checks values and sentinels.

Mutants (tests/test_gemm_operands_cpu.py): `mutants(case)` names every plausible indexing or rounding fault that applies to a case;
`result(case, fault=name)` is what a kernel with that fault would leave in C.
"""
import functools
import math
from dataclasses import dataclass

import numpy as np

from oracle import prng

NONE, GELU, RESIDUAL, SWIGLU, F32 = 0, 1, 2, 3, 4
EPI_NAME = {NONE: "none", GELU: "gelu", RESIDUAL: "residual", SWIGLU: "swiglu", F32: "f32"}
POISON = 2.0 ** 60
SENTINEL_BITS = 0x7B7B                                          # bf16; the fp32 sentinel is the same value (0x7B7B0000)
SENTINEL = float(np.array([SENTINEL_BITS << 16], dtype=np.uint32).view(np.float32)[0])
GUARD = 8
POWER_SHARE, POWER_TOL = 0.05, 16.0


def bf16r(x):
    """float64 -> the nearest bf16 value (ties to even), as float64"""
    u = np.ascontiguousarray(x, dtype=np.float32).view(np.uint32).astype(np.uint64)
    u = (u + 0x7FFF + ((u >> 16) & 1)) & 0xFFFF0000
    return u.astype(np.uint32).view(np.float32).astype(np.float64).reshape(np.shape(x))


def bf16_bits(x):
    """bf16-exact float64 values -> uint16 bit patterns"""
    f = np.ascontiguousarray(x, dtype=np.float32)
    assert np.array_equal(f.astype(np.float64), x), "value is not fp32-exact"
    u = f.view(np.uint32)
    assert not (u & 0xFFFF).any(), "value is not bf16-exact"
    return (u >> 16).astype(np.uint16).reshape(np.shape(x))


@dataclass(frozen=True)
class Case:
    form: str                 # the kernel form the (launcher, shape, knobs) reaches, read from the launch rules of ze_gemm.hip
    launcher: int
    epi: int
    M: int
    N: int
    K: int
    knobs: tuple = ()         # ((ze_tune knob, value), ...), restored to 0 after the call
    plain: str = ""           # which way the plain (two-byte) epilogue is reached: "" (wide-store form), "ldc" (ldc % 8 != 0), "rows" (c_rows)
    ksplit: int = 1           # K slices the form adds (for the split-K mutant)
    bias: bool = True
    ldr_odd: bool = False     # the misalignment cases
    c_off: int = 0            # C starts c_off elements into its allocation

    @property
    def exact(self):
        return self.epi in (NONE, RESIDUAL, F32)

    @property
    def wexp(self):           # W = integers * 2^wexp: 0 where the bits are fixed, an O(1) pre-activation for the approximated epilogues
        return 0 if self.exact else -int(round(math.log2(80.0 * math.sqrt(self.K))))

    @property
    def unit(self):
        return 2.0 ** (math.floor(math.log2(80.0 * math.sqrt(self.K))) + self.wexp - 6)

    @property
    def NO(self):             # output columns
        return self.N // 2 if self.epi == SWIGLU else self.N

    @property
    def lda(self):
        return self.K + 8

    @property
    def ldw(self):
        return self.K + 24

    @property
    def ldr(self):
        return self.N + (5 if self.ldr_odd else 8)

    @property
    def ldc(self):
        return self.N + (3 if self.plain == "ldc" else 16)

    @property
    def MC(self):             # rows of C that may be written: M, or the range of the row table
        return self.M + 5 if self.plain == "rows" else self.M

    @property
    def id(self):
        knobs = "".join(f"-k{k}={v}" for k, v in self.knobs)
        extra = ("-ldr_odd" if self.ldr_odd else "") + (f"-c+{self.c_off}" if self.c_off else "") + ("" if self.bias else "-nobias")
        return f"{self.form}-L{self.launcher}-{EPI_NAME[self.epi]}-{self.M}x{self.N}x{self.K}-{self.plain or 'aligned'}{knobs}{extra}"


@functools.lru_cache(maxsize=2)
def _w_ints(N, K):
    return prng.uniform_ints(0xB0B + N * 13 + K, N * K, 0, 31).reshape(N, K).astype(np.float64) - 15.0


@functools.lru_cache(maxsize=2)
def _ints(M, N, K):
    a = prng.uniform_ints(0xA11CE + M * 7 + K, M * K, 0, 31).reshape(M, K).astype(np.float64) - 15.0
    w = _w_ints(N, K)
    return a, w, a @ w.T


class Operands:
    """Logical operands (float64, exact) and the padded device buffers (float64 values; bf16_bits() of them is what is uploaded)."""

    def __init__(self, c: Case):
        M, N, K = c.M, c.N, c.K
        a, w, acc = _ints(M, N, K)
        s = 2.0 ** c.wexp
        self.A, self.W, self.acc = a, w * s, acc * s
        self.bias = (prng.uniform_ints(0xB1A5 + N, N, 0, 255).astype(np.float64) - 127.0) * c.unit if c.bias else np.zeros(N)
        self.R = (prng.uniform_ints(0x4E5 + M * 3 + N, M * N, 0, 255).reshape(M, N).astype(np.float64) - 127.0) * c.unit
        self.c_rows = None
        if c.plain == "rows":  # an injective table into MC rows, out of order
            order = np.argsort(prng.stream64(0xC0 + M, 0, c.MC), kind="stable")
            self.c_rows = order[:M].astype(np.int32)
        # ---- the three conditions the fixed bit patterns rest on
        assert np.abs(acc).max() < 2 ** 24 and 225 * K < 2 ** 24
        v = self.acc + self.bias
        assert np.array_equal(v.astype(np.float32).astype(np.float64), v), "acc + bias is not exact in fp32"
        if c.epi == RESIDUAL:
            t = self.R + bf16r(v)
            assert np.array_equal(t.astype(np.float32).astype(np.float64), t), "R + bf16(acc + bias) is not exact in fp32"
        # ---- padded buffers
        self.Abuf = np.full((M + GUARD, c.lda), POISON)
        self.Abuf[:M, :K] = self.A
        self.Wbuf = np.full((N + GUARD, c.ldw), POISON)
        self.Wbuf[:N, :K] = self.W
        self.biasbuf = np.full(N + 24, POISON)
        self.biasbuf[:N] = self.bias
        self.Rbuf = np.full((c.MC + GUARD, c.ldr), POISON)
        self.Rbuf[:M, :N] = self.R


@functools.lru_cache(maxsize=2)
def operands(c: Case) -> Operands:
    return Operands(c)


def _strided(buf, rows, cols, ld, row0=0):
    flat = buf.reshape(-1)
    idx = (np.arange(rows)[:, None] + row0) * ld + np.arange(cols)[None, :]
    return flat[np.minimum(idx, flat.size - 1)]   # (a read behind the allocation: poison, like the guard rows)


def mutants(c: Case):
    """the faults that apply to this case"""
    m = ["A read with lda := K", "W read with ldw := K", "the last K-tile dropped"]
    if c.ldc != c.NO:
        m.append("C written with ldc := N")
    if c.epi == RESIDUAL:
        m += ["R taken from row r + 1", "residual added before the first rounding"]
        if c.ldr != c.N:
            m.append("R read with ldr := N")
        if c.ldr != c.ldc:
            m.append("R read with ldr := ldc")
        if c.bias:
            m.append("residual added before the bias rounding, bias dropped")
        if c.plain == "rows":
            m.append("R taken at the output row c_rows[r]")
    if c.plain == "rows":
        m.append("c_rows ignored")
    if c.bias and c.epi != SWIGLU:
        m.append("bias column col + 16")
    if c.ksplit > 1:
        m.append("split-K: slice 0 added twice, the last slice dropped")
    return m


def result(c: Case, fault: str = ""):
    """-> (C buffer [MC + GUARD, ldc] as float64 values, tolerance buffer or None).  Bit-exact cases: the buffer IS the expected
    content (bits: `c_bits`).  GELU / SWIGLU: the float64 value of the epilogue on the exact bf16 pre-activation and the bound of
    tests/test_gpu_ops.py per element (0 where the sentinel must stay)."""
    assert not fault or fault in mutants(c), fault
    o = operands(c)
    M, N, K = c.M, c.N, c.K
    A, W, acc = o.A, o.W, o.acc
    if fault == "A read with lda := K":
        acc = _strided(o.Abuf, M, K, K) @ W.T
    elif fault == "W read with ldw := K":
        acc = A @ _strided(o.Wbuf, N, K, K).T
    elif fault == "the last K-tile dropped":
        k0 = (-(-K // 64) - 1) * 64
        acc = acc - A[:, k0:] @ W[:, k0:].T
    elif fault.startswith("split-K"):
        per = -(-(-(-K // 64)) // c.ksplit) * 64          # ceil(K-tiles / slices) tiles per slice, as every kernel cuts them
        last = per * (c.ksplit - 1)
        assert last < K
        acc = acc + A[:, :per] @ W[:, :per].T - A[:, last:] @ W[:, last:].T
    b = o.biasbuf[16:16 + N] if fault == "bias column col + 16" else o.biasbuf[:N]
    v = acc + b
    x = bf16r(v)
    tol = None
    if c.epi == RESIDUAL:
        Rm = o.R
        if fault == "R read with ldr := N":
            Rm = _strided(o.Rbuf, M, N, N)
        elif fault == "R read with ldr := ldc":
            Rm = _strided(o.Rbuf, M, N, c.ldc)
        elif fault == "R taken from row r + 1":
            Rm = o.Rbuf[1:M + 1, :N]
        elif fault == "R taken at the output row c_rows[r]":
            Rm = o.Rbuf[o.c_rows, :N]
        if fault == "residual added before the first rounding":
            out = bf16r(Rm + v)
        elif fault.startswith("residual added before the bias rounding"):
            out = bf16r(Rm + acc)
        else:
            out = bf16r(Rm + x)
    elif c.epi == GELU:    # tests/test_gpu_ops.py::test_linear, unchanged: x is the bf16 pre-activation
        ux, inv = np.unique(x, return_inverse=True)   # (x is bf16: a few thousand distinct values)
        erf = np.array([math.erf(t / math.sqrt(2.0)) for t in ux])[inv].reshape(x.shape)
        out = 0.5 * x * (1.0 + erf)
        tol = 2.0 ** -8 * (1.2 * np.maximum(np.abs(x), 0.05) + 1.5 * np.maximum(np.abs(out), 0.05))
    elif c.epi == SWIGLU:  # tests/test_gpu_ops.py::test_linear_3b_shapes, unchanged; sc = 0.05 x the nominal deviation of a sum there and here
        blk = v.reshape(M, N // 32, 2, 16)
        g, u = blk[:, :, 0, :].reshape(M, -1), blk[:, :, 1, :].reshape(M, -1)
        with np.errstate(over="ignore"):   # (a mutant's poisoned gate: exp overflows to inf, the quotient is 0 or the gate)
            out = g / (1.0 + np.exp(-g)) * u
        sc = 0.05 * 80.0 * math.sqrt(K) * 2.0 ** c.wexp
        tol = 2.0 ** -8 * (3.0 * np.abs(out) + 1.2 * np.maximum(np.abs(g), sc) * np.abs(u) + sc * sc)
    else:
        out = x
    buf = np.full((c.MC + GUARD, c.ldc), SENTINEL)
    rows = np.arange(M) if (o.c_rows is None or fault == "c_rows ignored") else o.c_rows.astype(np.int64)
    ld = c.NO if fault == "C written with ldc := N" else c.ldc
    idx = rows[:, None] * ld + np.arange(c.NO)[None, :]
    buf.reshape(-1)[idx] = out
    if tol is None:
        return buf, None
    tbuf = np.zeros_like(buf)
    tbuf.reshape(-1)[idx] = tol
    return buf, tbuf


def c_bits(c: Case, buf):
    """the expected C buffer of a bit-exact case as the integers the GPU test compares: int16 (bf16) or int32 (F32)"""
    if c.epi == F32:
        f = buf.astype(np.float32)
        assert np.array_equal(f.astype(np.float64), buf)
        return f.view(np.int32)
    return bf16_bits(buf).view(np.int16)


def power(c: Case, fault: str):
    """how clearly the case's inputs tell the fault from the truth: bit-exact cases -> the share of the written elements' count whose
    bits differ anywhere in the buffer; tolerance cases -> the largest |mutant - truth| / bound (inf where a sentinel moved)."""
    ref, tol = result(c)
    mut, _ = result(c, fault)
    if tol is None:
        return float((c_bits(c, ref) != c_bits(c, mut)).sum()) / (c.M * c.NO)
    d = np.abs(mut - ref)
    with np.errstate(divide="ignore", invalid="ignore"):
        ratio = np.where(d > 0, d / tol, 0.0)
    return float(ratio.max())


# ------------------------------------------------------------------------------------------------------------------ the cases
# The form each (launcher, shape, knobs) reaches is read from launch_policy / launch_cfg / launch_stream / ze_launch_gemm_wide /
# launch_tall / launch_splitk_two (ze_gemm.hip) for 256 CUs; tests/test_gpu_gemm_operands.py's kernel record
# (profiles/gemm_operands_kernel_stats.csv) is the check that they are reached.
def _epis(form, L, M, N, K, knobs=(), epis=(NONE, RESIDUAL), plains=("",), ksplit=1):
    return [Case(form, L, e, M, N, K, tuple(knobs), p, ksplit) for p in plains for e in epis]


def cases():
    cs = []
    all_plain = ("", "ldc", "rows")
    # ---- k_gemm_tn (register-staged): knob 6 = 1, and K = 40 / 1176 (not ring-able)
    cs += _epis("tn64x64", 0, 130, 200, 40, epis=(NONE, RESIDUAL, GELU), plains=("", "rows"))
    cs += _epis("tn64x64", 1, 70, 136, 1176, epis=(NONE, RESIDUAL, GELU), plains=("", "rows"))
    cs += _epis("tn64x64", 0, 130, 200, 256, [(6, 1)], epis=(NONE, RESIDUAL))
    cs += _epis("tn64x128", 0, 1030, 1000, 256, [(6, 1)], epis=(NONE, RESIDUAL, GELU), plains=("", "rows"))
    cs += _epis("tn128x128", 0, 1800, 1736, 256, [(6, 1)], epis=(NONE, RESIDUAL, GELU), plains=("", "rows"))
    # ---- k_gemm_ring, wide-store and plain (knob 7 = 10 / ldc % 8 / c_rows); K-tiles 4, 5 and 7
    for K in (256, 320, 448):
        cs += _epis("ring64x64", 0, 130, 200, K, plains=all_plain)
        cs += _epis("ring64x64-plain", 0, 130, 200, K, [(7, 10)])
    cs += _epis("ring64x64", 1, 130, 192, 320, epis=(SWIGLU, F32), plains=("", "ldc"))
    cs += _epis("ring64x64-plain", 1, 130, 192, 320, [(7, 10)], epis=(SWIGLU, F32))
    cs += _epis("ring64x128", 0, 1030, 1000, 256, plains=all_plain)
    cs += _epis("ring64x128", 0, 1030, 992, 320, epis=(SWIGLU, F32), plains=("", "ldc"))
    cs += _epis("ring64x128-plain", 0, 1030, 1000, 448, [(7, 10)])
    for K in (256, 448):
        cs += _epis("ring128x128spread", 0, 1410, 1496, K, plains=all_plain)
    cs += _epis("ring128x128spread-plain", 0, 1410, 1496, 320, [(7, 10)])
    cs += _epis("ring128x128spread", 1, 1410, 1504, 320, epis=(SWIGLU, F32), plains=("", "ldc"))
    cs += _epis("ring128x256", 0, 1800, 1736, 256, [(7, 6)], plains=all_plain)
    cs += _epis("ring128x256", 0, 1800, 1728, 320, [(7, 6)], epis=(SWIGLU, F32), plains=("", "ldc"))
    cs += _epis("ring256x256", 0, 1800, 1736, 256, [(7, 4)])     # (four K-tiles: the two-stage ring's minimum)
    cs += _epis("ring256x256", 0, 1800, 1736, 320, [(7, 4)], plains=all_plain)
    cs += _epis("ring256x256", 0, 1800, 1728, 448, [(7, 4)], epis=(SWIGLU, F32), plains=("", "ldc"))
    # ---- k_gemm_p8, direct: wide and plain tails, persistent and one tile per workgroup (knob 4)
    for M, N, K in ((300, 520, 128), (513, 2056, 320), (5, 16, 256)):
        cs += _epis("p8", 2, M, N, K, plains=all_plain)
        cs += _epis("p8-plain", 2, M, N, K, [(7, 10)])
    cs += _epis("p8-tilewise", 2, 300, 520, 128, [(4, 1)], plains=("", "rows"))
    cs += _epis("p8", 2, 300, 544, 128, epis=(SWIGLU, F32), plains=("", "ldc"))
    cs += _epis("p8-plain", 2, 513, 2048, 320, [(7, 10)], epis=(SWIGLU, F32))
    # Three K slices (knob 20 = 3).  The eight-phase kernel takes them through launcher 2 here, not through launcher 0: ze_launch_gemm
    # picks it only from 200 tiles of 128 x 128 on, and three slabs of such a grid do not fit the prefill workspace of the test engine
    # (3 x rows x hidden floats of the tiny model).  Launcher 0 at this K runs the 64 x 64 tiles: the ring while tiles x 3 slices fit
    # one round of 256 workgroups (600 rows: 10 x 8 x 3 = 240), the register-staged kernel beyond (700 rows: 264).
    cs += _epis("p8-3slices", 2, 700, 512, 4160, [(20, 3)], ksplit=3)
    cs += _epis("ring64x64-3slices", 0, 600, 512, 4160, [(20, 3)], ksplit=3)
    cs += _epis("tn64x64-3slices", 0, 700, 512, 4160, [(20, 3)], ksplit=3)
    # ---- the weight-streaming launcher: the row-major skinny kernel (MT 1 / 2 / 4), the 64 x 64 ring with eight ticketed K slices
    for M in (3, 17, 33):
        cs += _epis("skinny", 3, M, 208, 352, plains=("", "ldc"))
    cs += _epis("ring64x64-8tickets", 3, 70, 512, 4160, plains=("", "ldc"), ksplit=8)
    # ---- the row-streaming launcher: two-launch split K (k_splitk_reduce), tall tiles, k_gemm_wstream, the 192-column SwiGLU tiles
    for M, tile in ((65, "64x128"), (129, "128x128"), (257, "192x128"), (385, "128x256"), (513, "320x128"), (641, "384x128")):
        cs += _epis(f"splitk2-{tile}", 4, M, 512, 4160, ksplit=8)
    for M, bm in ((65, 64), (257, 80), (321, 96), (385, 112), (449, 128)):
        cs += _epis(f"tall{bm}x64-6stage", 4, M, 4088, 256)
    cs += _epis("tall80x64-4stage", 4, 257, 4088, 320)
    # (k_gemm_wstream is instantiated for the 32 K-steps of K = 2048 alone: launch_wstream)
    for M, form in ((96, "policy-ring64x128"), (97, "wstream128x96"), (128, "wstream128x96"), (129, "wstream256x96"), (256, "wstream256x96")):
        cs += _epis(form, 4, M, 8192, 2048, epis=(SWIGLU,))
    cs += _epis("wstream256x96+128x96", 4, 257, 8192, 2048, [(15, 5)], epis=(SWIGLU,))   # (knob 15 = 5: blocks of 256 rows)
    for M, form in ((128, "wstream128x96"), (129, "wstream256x96"), (160, "wstream256x96"), (161, "policy-ring64x128")):
        cs += _epis(form, 4, M, 8192, 2048, epis=(F32,))
    cs += _epis("ring192x192", 4, 257, 8192, 2048, epis=(SWIGLU,))
    cs += _epis("ring192x192", 4, 384, 8192, 2048, epis=(SWIGLU,))
    cs += _epis("ring256x192", 4, 385, 8192, 256, epis=(SWIGLU,))
    cs += _epis("ring320x192", 4, 513, 8192, 256, epis=(SWIGLU,))
    cs += _epis("ring384x192", 4, 641, 8192, 256, epis=(SWIGLU,))
    cs += _epis("wstream384x96", 4, 300, 8192, 2048, [(15, 4)], epis=(SWIGLU,))
    cs += _epis("wstream512x96", 4, 400, 8192, 2048, [(15, 4)], epis=(SWIGLU,))
    cs += _epis("policy", 4, 769, 512, 256, epis=(NONE, RESIDUAL, SWIGLU))
    # ---- fragment-major skinny and one-shot
    for L, form in ((5, "frag"), (6, "oneshot")):
        for M, N, K in ((3, 16, 32), (17, 208, 128), (64, 2560, 2048)):
            cs += _epis(form, L, M, N, K)
    ids = [c.id for c in cs]
    assert len(set(ids)) == len(ids), [i for i in ids if ids.count(i) > 1]
    return cs


def misaligned_cases():
    """C and R off the 16-byte grid: ldc = N + 3 with N = 130, C one element into its allocation, ldr odd -- each takes the plain tail.
    The expected bits do not know about alignment; the N = 136 cases are also compared with the wide-store run of the same operands
    (at N = 130 no run can be wide: N % 8)."""
    cs = []
    for L, form, M, K, knobs in ((0, "ring64x64", 130, 256, ()), (0, "tn64x64", 130, 40, ()), (2, "p8", 300, 128, ()),
                                 (3, "skinny", 33, 352, ()), (4, "tall64x64", 65, 256, ())):
        for e in (NONE, RESIDUAL):
            cs.append(Case(form, L, e, M, 130, K, knobs, "ldc"))
            cs.append(Case(form, L, e, M, 136, K, knobs, "", c_off=1))
            if e == RESIDUAL:
                cs.append(Case(form, L, e, M, 136, K, knobs, "", ldr_odd=True))
    return cs
