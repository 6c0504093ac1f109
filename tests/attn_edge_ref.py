"""Planted inputs for the attention kernels, their float64 reference and the MUTANTS a test on them has to tell apart (numpy only).

On N(0, 1) queries one key carries about 1 / L of the softmax mass, so a kernel that reads one key too many or too few at a
mask edge, a segment end, a key-tile edge or a part boundary moves the result by less than the parity bounds
(tests/test_attn_edge_cpu.py::test_diffuse_inputs_cannot_see_a_dropped_key measures it).  Here a probed (query, head) is a NEEDLE:

  * one needle    q = bf16(2 K[t]) (flash: scaled so that q . K[t] = 2 d exactly): the target's score is about 2 sqrt(d), every
                  other key's is N(0, 4) -- the target holds nearly all of the mass;
  * two needles   q = alpha K[a] + beta K[b] with q . K[a] = q . K[b] = 2 d, a and b on either side of a boundary: the mass splits
                  in halves, which makes the result depend on the merge weights of the online softmax / of the part merge (and
                  on a key that is read TWICE, which a single needle cannot see);
  * poison        an INVISIBLE key next to the visible set that would take the mass if it were read.  Decode: the dead rows
                  x behind ctx hold K[x] = bf16(1.5 (K[a] + K[b])) and |V| = 8.  Flash: a poison row of one query is a visible
                  row of the next, so the pull sits in the query instead -- q gets a component along K[x] of the row x just outside
                  ITS visible set with q . K[x] = 3 d (score 3 sqrt(d) against the needle's 2 sqrt(d), as 1.5 K[t] would give) --
                  and K stays free of dependencies between rows;
  * V             N(0, 1) clipped to +-4; the two targets of a pair hold +4 / -4 in one column, so that the halves of a two-needle
                  result differ by 8 where the bound is a fraction of max |V| = 4.

The reference is always the exact float64 softmax over the true visible set (`attend`); nothing assumes a one-hot result.  A mutant
is the same function over a WRONG set of rows (a row dropped, added, read twice; another kv head; a prefix read from the wrong
slot).  A probed row is AFFECTED by a mutant when the row the mutant touches is one of its needles (a doubled row: one of its two
needles) or its poison; tests/test_attn_edge_cpu.py asserts that every affected row moves by at least 16 x the bound of the GPU
test, and that every case has an affected row for every mutant that applies to it."""
import os
import re

import numpy as np

from oracle import prng
from oracle.qwen25vl import bf16_round

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "zoomearth_amd", "csrc")
VMAX, VPOISON = 4.0, 8.0
POWER = 16.0                        # a mutant moves an affected row by at least POWER x the bound


def _define(path, name):
    with open(os.path.join(CSRC, path), encoding="utf-8") as f:
        m = re.search(r"^#define\s+%s\s+(\d+)\s*(?://.*)?$" % name, f.read(), flags=re.M)
    assert m, (path, name)
    return int(m.group(1))


def flash_geometry():
    """(keys per tile non-causal, keys per tile causal, query rows per short tile, per long tile) of k_flash_attn, from its source"""
    return (_define("ze_attention.hip", "FA_BK"), _define("ze_attention.hip", "ZE_FA_CAUSAL_BKV"), _define("ze_attention.hip", "FA_BQ"),
            _define("ze_kernels.h", "ZE_FA_BQ_LONG"))


def rnd(seed, shape, std=1.0):
    return bf16_round(prng.normal_ih4(seed, int(np.prod(shape)), std)).reshape(shape)


def attend(q, K, V, idx):
    """float64 softmax(q . K[idx] / sqrt(d)) V[idx]; a row named twice is a key read twice"""
    idx = np.asarray(idx, dtype=np.int64)
    if idx.size == 0:                                   # no visible key: the kernels' l = 0 -> a row of zeros
        return np.zeros(V.shape[-1])
    s = K[idx].astype(np.float64) @ q.astype(np.float64) / np.sqrt(float(q.shape[-1]))
    p = np.exp(s - s.max())
    return (p / p.sum()) @ V[idx].astype(np.float64)


def one_needle(kt):
    return bf16_round((2.0 * kt.astype(np.float64)).astype(np.float32))


def needles(keys, pull=None):
    """the combination of `keys` (one or two target rows) and of the invisible row `pull` whose product with every target is 2 d and
    with `pull` 3 d: two targets share the mass in halves; the invisible row, if read, outweighs them by exp(sqrt(d))"""
    vecs = [k.astype(np.float64) for k in keys] + ([pull.astype(np.float64)] if pull is not None else [])
    d = len(vecs[0])
    gram = np.array([[a @ b for b in vecs] for a in vecs])
    rhs = np.array([2.0 * d] * len(keys) + ([3.0 * d] if pull is not None else []))
    coef = np.linalg.solve(gram, rhs)
    return bf16_round(sum(c * v for c, v in zip(coef, vecs)).astype(np.float32))


def _sign_rows(n, d, mag, first=0):
    """rows first .. first + n - 1 of +-mag, a different pattern per row: far from any N(0, 1) row and from each other"""
    r = np.arange(first, first + n, dtype=np.uint64)[:, None]
    c = np.arange(d, dtype=np.uint64)[None, :]
    h = ((r + 1) * 0x9E3779B1 + (c + 1) * 0x85EBCA6B) & 0xFFFFFFFF      # a 32-bit integer hash of (row, column): its bit 5 is the sign
    h ^= h >> 15
    h = (h * 0x2C1B3C6D) & 0xFFFFFFFF
    h ^= h >> 12
    return np.where((h >> 5) & 1 == 0, mag, -mag).astype(np.float32)


def _plant_pair_column(V, row, a, b, d):
    """the two targets of a pair differ by 2 VMAX in one column (`row(r)`: the view of V that is row r of the kv head)"""
    if a == b:
        return
    col = (a * 7 + b * 13) % d
    row(a)[col] = VMAX
    row(b)[col] = -VMAX


class Probe:
    """one needle row: `idx` the truly visible rows, (a, b) its pair of targets, mode 0 / 1 / 2 = needle on a / on b / on both,
    x the poison rows that serve it"""

    def __init__(self, where, head, kvh, idx, pair, mode, poison, q):
        self.where, self.head, self.kvh, self.idx, self.pair, self.poison, self.q = where, head, kvh, idx, pair, tuple(poison), q
        self.mode = 0 if pair[0] == pair[1] else mode
        self.needles = {0: {pair[0]}, 1: {pair[1]}, 2: set(pair)}[self.mode]

    def affected(self, mut):
        kind, rows = mut[0], mut[1]
        if kind == "drop":
            return bool(self.needles & set(rows))
        if kind == "twice":
            return self.mode == 2 and bool(self.needles & set(rows))
        if kind == "add":
            return bool(set(self.poison) & set(rows))
        return True                                             # another kv head / another slot: every needle is somewhere else

    def rows_under(self, mut):
        kind, rows = mut[0], mut[1]
        if kind == "drop":
            return [r for r in self.idx if r not in set(rows)]
        if kind in ("twice", "add"):
            return list(self.idx) + list(rows)
        return list(self.idx)


# ------------------------------------------------------------------------------------------------------------------ flash
FLASH_CU = ([0, 1, 64, 65, 128, 192, 193, 321, 449, 450, 705], [0, 4, 68, 100, 356, 1296 + 356])
FLASH_PAD = 64


class FlashCase:
    """q [T + 64, heads, D], k / v [T + 64, kvh, D] (the 64 rows behind T: poison, never visible), the probes and their float64
    results.  Probed queries: the first and last row of every segment, rows 63, 64, 127, 128 of the segments that have them (the
    edges of the 64- and 128-row query tiles; the last row of T is the last segment's).  Targets cycle over the first key of the
    visible set, the last one, and the first key of the last key tile with the key before it."""

    def __init__(self, D, causal, cu, heads, kvh, seed=0):
        bk, bk_causal, _, _ = flash_geometry()
        bkv = bk_causal if causal else bk
        T, g = cu[-1], heads // kvh
        self.D, self.causal, self.cu, self.heads, self.kvh, self.T = D, causal, list(cu), heads, kvh, T
        n = T + FLASH_PAD
        self.k = rnd(1000 + seed, (n, kvh, D))
        self.v = np.clip(rnd(2000 + seed, (n, kvh, D)), -VMAX, VMAX)
        self.q = rnd(3000 + seed, (n, heads, D))
        self.v[T:] = _sign_rows(FLASH_PAD * kvh, D, VPOISON).reshape(FLASH_PAD, kvh, D)
        plan, count = [], 0
        for s0, s1 in zip(cu[:-1], cu[1:]):
            rel = sorted({0, s1 - s0 - 1} | {r for r in (63, 64, 127, 128) if r < s1 - s0})
            for i in (s0 + r for r in rel):
                lo, hi = s0, (i + 1 if causal else s1)
                edge = lo + (hi - 1 - lo) // bkv * bkv
                pairs = [(lo, min(lo + 1, hi - 1)), (max(hi - 2, lo), hi - 1)] + ([(edge - 1, edge)] if edge > lo else [])
                for kh in range(kvh):
                    pair = pairs[(count + kh) % len(pairs)]
                    for j in range(g):
                        h = kh * g + j
                        x = s0 - 1 if (s0 > 0 and (count + h) % 2) else hi   # the previous segment's last row, or the row behind the visible set
                        plan.append((i, h, kh, lo, hi, pair, (count // len(pairs) + kh + j) % 3, x, edge if edge > lo else None))
                count += 1
        for (i, h, kh, lo, hi, pair, mode, x, edge) in plan:       # in-segment poison rows first, then the pair columns on top
            if x < T:
                self.v[x, kh] = _sign_rows(1, D, VMAX, first=x * kvh + kh)[0]
        for (i, h, kh, lo, hi, pair, mode, x, edge) in plan:
            _plant_pair_column(self.v, lambda r, kh=kh: self.v[r, kh], pair[0], pair[1], D)
        self.probes = []
        for (i, h, kh, lo, hi, pair, mode, x, edge) in plan:
            ka, kb = self.k[pair[0], kh], self.k[pair[1], kh]
            mode = 0 if pair[0] == pair[1] else mode
            qv = needles([ka, kb] if mode == 2 else [kb if mode == 1 else ka], self.k[x, kh])
            self.q[i, h] = qv
            p = Probe(i, h, kh, range(lo, hi), pair, mode, [x], qv)
            p.lo, p.hi, p.seg0, p.edge = lo, hi, self.cu[np.searchsorted(self.cu, i, side="right") - 1], edge
            self.probes.append(p)
        self.want = np.stack([self.result(p) for p in self.probes])
        self.bound = 2.0 ** -6 * max(1.0, float(np.abs(self.want).max()))          # the bound of tests/test_gpu_ops.py::test_attention

    def result(self, p, mut=None):
        kh = p.kvh if mut is None or mut[0] != "kvh" else (p.kvh + 1) % self.kvh
        return attend(p.q, self.k[:, kh], self.v[:, kh], p.idx if mut is None or mut[0] == "kvh" else p.rows_under(mut))

    def mutants(self, p):
        """name -> (kind, rows) for one probe: what a kernel with that fault would compute"""
        m = {"drop the last visible key": ("drop", [p.hi - 1]),
             "add the first invisible key": ("add", [p.hi]),                 # causal: key i + 1; else the next segment's first row / a row behind T
             "drop the first key": ("drop", [p.lo])}
        if p.seg0 > 0:
            m["add the previous segment's last key"] = ("add", [p.seg0 - 1])
        if p.edge is not None:
            m["drop the last key of a key tile"] = ("drop", [p.edge - 1])
            m["read the last key of a key tile twice"] = ("twice", [p.edge - 1])
            m["drop the first key of the next key tile"] = ("drop", [p.edge])
            m["read the first key of the next key tile twice"] = ("twice", [p.edge])
        if self.kvh > 1:
            m["another kv head"] = ("kvh", [])
        return m


def flash_cases():
    """D x causal x the two segment lists x (GQA 4 on 2, MHA 4 on 4)"""
    out = []
    for D in (80, 128):
        for causal in (False, True):
            for ci in range(len(FLASH_CU)):
                for kvh in (2, 4):
                    out.append((D, causal, ci, kvh))
    return out


_FLASH = {}


def flash_case(D, causal, ci, kvh):
    key = (D, causal, ci, kvh)
    if key not in _FLASH:
        _FLASH[key] = FlashCase(D, causal, FLASH_CU[ci], 4, kvh, seed=D + 400 * int(causal) + 20 * ci + kvh)
    return _FLASH[key]


# ------------------------------------------------------------------------------------------------------------------ decode
DECODE_LENS = [5, 62, 63, 64, 190, 191, 192, 254, 255, 256, 382, 383, 384, 500, 766, 767, 768, 1000]
DECODE_SPLIT = [(731, 347), (384, 347)]           # (ctx, split row) of the split-row form: a last own part of one row, a short one
DECODE_PARTS = (64, 192, 384)                     # k_attn_decode_split, k_attn_decode_wave, k_attn_decode_wave_long
HEADS, KV_HEADS, HD, MAX_CTX = 16, 2, 128, 1024


def stream_part(n):
    """keys per part of k_attn_decode_stream over n visible rows (ze_attn_batch.hip: a sixth .. an eighth of the context, 192 at least)"""
    return max(192, ((n + 7) // 8 + 31) // 32 * 32)


class DecodeChain:
    """One chain of `ctx` cached rows whose decode step attends rows 0 .. ctx (the step's own row included): K / V [kv, MAX_CTX,
    128] to plant in rows 0 .. ctx, the dead rows ctx + 1 .. to the end of that 64-key tile (poison), and per PASS one qkv row of
    needles.  A pass gives each kv head one pair of targets; heads j of a kv head take mode j % 3.  Pairs: (ctx - 1, ctx), (0, 1) and
    (B - 1, B) for the start B of the last part under every partition (64, 192, 384, the stream kernel's, the split row's)."""

    def __init__(self, ctx, seed, split=0, own_from=0, holder=None):
        self.ctx, self.split, self._memo = ctx, split, {}
        n = ctx + 1
        self.k = rnd(5000 + seed, (KV_HEADS, MAX_CTX, HD))
        self.v = np.clip(rnd(6000 + seed, (KV_HEADS, MAX_CTX, HD)), -VMAX, VMAX)
        self.dead = list(range(ctx + 1, min(MAX_CTX, (ctx + 1) // 64 * 64 + 64)))
        self.v[:, self.dead] = _sign_rows(len(self.dead), HD, VPOISON)[None]
        self.bounds = {}
        for name, part in [("64-key parts", 64), ("192-key parts", 192), ("384-key parts", 384), ("stream parts", stream_part(n))]:
            if ctx // part >= 1:
                self.bounds[name] = ctx // part * part
        if split:
            self.bounds["split row"] = split
            if (ctx - split) // 384 >= 1:
                self.bounds["split parts"] = split + (ctx - split) // 384 * 384
        if own_from:
            self.bounds = {"prefix end": own_from}
        pairs = [(ctx - 1, ctx), (0, 1)] + [(b - 1, b) for b in sorted(set(self.bounds.values()))]
        self.pairs = [p for i, p in enumerate(pairs) if p not in pairs[:i]]
        if own_from:
            self.pairs = [(own_from - 1, own_from)]
        self.passes = (len(self.pairs) + KV_HEADS - 1) // KV_HEADS
        # the rows a correct kernel reads: this chain's, or below `own_from` the holder's (prefix hint)
        self.own_from, self.holder = own_from, holder
        self.kt, self.vt = self.k.copy(), self.v.copy()
        if holder is not None:
            self.kt[:, :own_from], self.vt[:, :own_from] = holder.k[:, :own_from], holder.v[:, :own_from]
            self.v[:, :own_from] = _sign_rows(own_from, HD, VPOISON)[None]           # its own rows below: never read
        for a, b in self.pairs:
            for kh in range(KV_HEADS):
                _plant_pair_column(self.vt, lambda r, kh=kh: self.vt[kh, r], a, b, HD)
                if holder is None:
                    _plant_pair_column(self.v, lambda r, kh=kh: self.v[kh, r], a, b, HD)
        if holder is not None:                                                        # (the planted columns land in the slot that holds the row)
            holder.v[:, :own_from] = self.vt[:, :own_from]
            self.v[:, own_from:] = self.vt[:, own_from:]
            for kh in range(KV_HEADS):   # the two wrong reads: row own_from - 1 from this slot, row own_from from the holder's
                pull = bf16_round((1.5 * (self.kt[kh, own_from - 1].astype(np.float64) + self.kt[kh, own_from])).astype(np.float32))
                self.k[kh, own_from - 1] = pull
                holder.k[kh, own_from] = pull
                holder.v[kh, own_from] = _sign_rows(1, HD, VPOISON)[0]
        self.bound = [2.0 ** -7 * float(np.abs(self.vt[kh, :n]).max()) for kh in range(KV_HEADS)]   # max |V| over VISIBLE rows

    def pair_of(self, r, kh):
        return self.pairs[(r * KV_HEADS + kh) % len(self.pairs)]

    def dead_k(self, r):
        """K of every dead row in pass r: [kv, 128] = bf16(1.5 (K[a] + K[b])) of the kv head's pair"""
        out = np.zeros((KV_HEADS, HD), np.float32)
        for kh in range(KV_HEADS):
            a, b = self.pair_of(r, kh)
            out[kh] = bf16_round((1.5 * (self.kt[kh, a].astype(np.float64) + self.kt[kh, b])).astype(np.float32))
        return out

    def probes(self, r):
        g = HEADS // KV_HEADS
        out = []
        for h in range(HEADS):
            kh, j = h // g, h % g
            a, b = self.pair_of(r, kh)
            mode = 0 if a == b else j % 3
            ka, kb = self.kt[kh, a], self.kt[kh, b]
            qv = needles([ka, kb]) if mode == 2 else one_needle(kb if mode == 1 else ka)
            out.append(Probe(r, h, kh, range(0, self.ctx + 1), (a, b), mode, self.dead, qv))
        return out

    def _true_rows(self, r):
        if r not in self._memo:
            k = self.kt.copy()
            k[:, self.dead] = self.dead_k(r)[:, None, :]
            self._memo[r] = k
        return self._memo[r], self.vt

    def result(self, p, mut=None):
        """float64 result of probe p (pass p.where), or what the kernel with fault `mut` would give"""
        k, v = self._true_rows(p.where)
        kh, rows = p.kvh, list(p.idx)
        if mut is not None:
            if mut[0] == "kvh":
                kh = (p.kvh + 1) % KV_HEADS
            elif mut[0] == "own slot":                   # rows [0, own_from) from the chain's own slot instead of the holder's
                k, v = k.copy(), v.copy()
                k[:, :self.own_from], v[:, :self.own_from] = self.k[:, :self.own_from], self.v[:, :self.own_from]
            elif mut[0] == "holder row":                 # row own_from from the holder's slot instead of the chain's own
                k, v = k.copy(), v.copy()
                k[:, self.own_from], v[:, self.own_from] = self.holder.k[:, self.own_from], self.holder.v[:, self.own_from]
            else:
                rows = p.rows_under(mut)
        return attend(p.q, k[kh], v[kh], rows)

    def mutants(self):
        m = {"read the dead rows behind ctx": ("add", self.dead), "another kv head": ("kvh", [])}
        if self.holder is None:
            m.update({"drop the last key": ("drop", [self.ctx]), "drop row 0": ("drop", [0])})
        for name, b in self.bounds.items():
            m[f"{name}: drop the last key of a part"] = ("drop", [b - 1])
            m[f"{name}: read the last key of a part twice"] = ("twice", [b - 1])
            m[f"{name}: drop the first key of the next part"] = ("drop", [b])
            m[f"{name}: read the first key of the next part twice"] = ("twice", [b])
        if self.holder is not None:
            m["prefix rows from the chain's own slot"] = ("own slot", [])
            m["the first own row from the holder's slot"] = ("holder row", [])
        return m

    def qkv_row(self, r):
        """the row ze_op_attn_decode takes in pass r: the needles, then k / v of the chain's newest row (row ctx)"""
        q = np.concatenate([p.q for p in self.probes(r)])
        return np.concatenate([q, self.kt[:, self.ctx].reshape(-1), self.vt[:, self.ctx].reshape(-1)])

    def cache_rows(self, r):
        """[rows, (heads + 2 kv) x 128] to plant at row 0 of the chain's OWN slot in pass r: rows 0 .. ctx and the dead rows (q part zero)"""
        k, v = self.k.copy(), self.v.copy()
        k[:, self.dead] = self.dead_k(r)[:, None, :]
        n = self.ctx + 1 + len(self.dead)
        out = np.zeros((n, (HEADS + 2 * KV_HEADS) * HD), np.float32)
        out[:, HEADS * HD: (HEADS + KV_HEADS) * HD] = k[:, :n].transpose(1, 0, 2).reshape(n, -1)
        out[:, (HEADS + KV_HEADS) * HD:] = v[:, :n].transpose(1, 0, 2).reshape(n, -1)
        return out


_DECODE = {}


def decode_chains():
    """the chains of the planted decode test: the lengths of the existing float64 test, then the two split-row chains"""
    if "chains" not in _DECODE:
        _DECODE["chains"] = [DecodeChain(L, i) for i, L in enumerate(DECODE_LENS)] + \
            [DecodeChain(c, 100 + i, split=s) for i, (c, s) in enumerate(DECODE_SPLIT)]
    return _DECODE["chains"]


PREFIX_ROWS = (347, 383, 384)
PREFIX_CTX = 500


def prefix_pairs():
    """(holder A, reader B) per prefix length: B reads rows [0, rows) from A's slot and rows rows .. ctx from its own"""
    if "prefix" not in _DECODE:
        out = []
        for i, rows in enumerate(PREFIX_ROWS):
            a = DecodeChain(PREFIX_CTX, 200 + 2 * i)
            out.append((a, DecodeChain(PREFIX_CTX, 201 + 2 * i, own_from=rows, holder=a)))
        _DECODE["prefix"] = out
    return _DECODE["prefix"]
