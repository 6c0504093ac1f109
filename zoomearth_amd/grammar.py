"""Guided decoding, the compiler: a regular expression (or a list of choices) and a vocabulary become the token automaton that
ze_grammar_create takes (include/zoomearth.h) -- vLLM's `guided_regex` / `guided_choice`.

    pattern --parse--> AST --Thompson--> NFA --subset construction--> DFA over bytes --minimise-->
    --walk every token through every state, one byte position at a time--> token automaton
    --drop what cannot reach an accepting state BY TOKENS OF THIS VOCABULARY--> --group identical columns--> classes

The pattern has full-match semantics over BYTES (a non-ASCII literal stands for its UTF-8 bytes).  Supported: literals, the escapes
\\d \\w \\s \\n \\t \\r \\\\ and escaped punctuation, `.` (any byte but \\n), `[...]` with ranges and negation, groups `(...)` / `(?:...)`,
`|`, and the quantifiers `* + ? {m} {m,} {m,n}`.  Anything else raises ValueError naming the construct.  Pure Python + numpy.
"""
from __future__ import annotations

from typing import NamedTuple, Optional, Sequence

import numpy as np

MAX_GRAMMAR_STATES = 2048    # ZE_MAX_GRAMMAR_STATES
MAX_GRAMMAR_CLASSES = 4096   # ZE_MAX_GRAMMAR_CLASSES

# The stage-1 reply (hostloop.stage1_prompt asks for it): one <think> block holding exactly one "bbox_2d": [n,n,n,n] with 1-4-digit
# integers, then <answer>...</answer> on one line.  No entry point uses it by default.
_FREE = r'(?:[^<"\n]|\n)'   # free text of the think block: no tag, no quote (so no second "bbox_2d")
STAGE1_BBOX = (r'<think>' + _FREE + r'*"bbox_2d": ?\[\d{1,4}, ?\d{1,4}, ?\d{1,4}, ?\d{1,4}\]' + _FREE + r'*</think>\n?'
               r'<answer>[^<"\n]+</answer>')


class TokenAutomaton(NamedTuple):
    token_class: np.ndarray   # uint16 [vocab]
    trans: np.ndarray         # int16 [n_states, n_classes], -1 = not allowed; state 0 is the start
    accepting: np.ndarray     # uint8 [n_states]

    def step(self, state: int, token: int) -> int:
        return int(self.trans[state, self.token_class[token]])

    def allowed(self, state: int) -> np.ndarray:
        """ids allowed in `state` (EOS handling is the engine's: it follows `accepting`)"""
        return np.nonzero(self.trans[state][self.token_class] >= 0)[0]


# ----------------------------------------------------------------------------- parser: pattern -> AST
# AST nodes: ("set", mask) one byte of a 256-bit mask | ("cat", [nodes]) | ("alt", [nodes]) | ("rep", node, lo, hi or None)
_ALL = (1 << 256) - 1


def _mask(chars) -> int:
    m = 0
    for c in chars:
        m |= 1 << c
    return m


_DIGIT = _mask(range(0x30, 0x3a))
_WORD = _DIGIT | _mask(range(0x41, 0x5b)) | _mask(range(0x61, 0x7b)) | (1 << 0x5f)
_SPACE = _mask(b" \t\n\r\f\v")
_CLASS_ESC = {"d": _DIGIT, "w": _WORD, "s": _SPACE}
_CHAR_ESC = {"n": 0x0a, "t": 0x09, "r": 0x0d}
_PUNCT = set("\\.^$*+?{}[]()|/-\"'<>:,;=!#%&~`@_ ")


class _Parser:
    def __init__(self, pattern: str):
        self.p, self.i = pattern, 0

    def fail(self, what: str):
        raise ValueError(f"unsupported regular expression construct: {what} (at offset {self.i} of {self.p!r})")

    def peek(self) -> Optional[str]:
        return self.p[self.i] if self.i < len(self.p) else None

    def parse(self):
        node = self.alt()
        if self.i < len(self.p):
            self.fail("unbalanced ')'")
        return node

    def alt(self):
        branches = [self.cat()]
        while self.peek() == "|":
            self.i += 1
            branches.append(self.cat())
        return branches[0] if len(branches) == 1 else ("alt", branches)

    def cat(self):
        items = []
        while self.peek() is not None and self.peek() not in "|)":
            items.append(self.quantified())
        return ("cat", items)

    def quantified(self):
        node = self.atom()
        c = self.peek()
        lo = hi = None
        if c == "*":
            lo, hi = 0, None
        elif c == "+":
            lo, hi = 1, None
        elif c == "?":
            lo, hi = 0, 1
        elif c == "{":
            j = self.p.find("}", self.i)
            body = self.p[self.i + 1:j] if j > 0 else ""
            parts = body.split(",")
            if j < 0 or len(parts) > 2 or not parts[0].isdigit() or (len(parts) == 2 and parts[1] and not parts[1].isdigit()):
                self.fail("'{' that is no {m}, {m,} or {m,n} quantifier (escape a literal brace)")
            lo = int(parts[0])
            hi = lo if len(parts) == 1 else (int(parts[1]) if parts[1] else None)
            if hi is not None and hi < lo:
                self.fail("{m,n} with n < m")
            self.i = j
        if lo is None:
            return node
        self.i += 1
        if self.peek() == "?":
            self.fail("lazy quantifier")
        if self.peek() == "+":
            self.fail("possessive quantifier")
        if self.peek() in ("*", "{"):
            self.fail("multiple repeat")
        return ("rep", node, lo, hi)

    def atom(self):
        c = self.p[self.i]
        if c == "(":
            self.i += 1
            if self.peek() == "?":
                if self.p[self.i:self.i + 2] == "?:":
                    self.i += 2
                else:
                    nxt = self.p[self.i + 1:self.i + 3]
                    self.fail("look-around" if nxt[:1] in ("=", "!") or nxt in ("<=", "<!") else
                              "named group / back-reference" if nxt[:1] == "P" or nxt[:1] == "<" else "inline flag")
            node = self.alt()
            if self.peek() != ")":
                self.fail("unbalanced '('")
            self.i += 1
            return node
        if c == "[":
            return self.char_class()
        if c == ".":
            self.i += 1
            return ("set", _ALL & ~(1 << 0x0a))
        if c in "^$":
            self.fail(f"anchor '{c}' (the pattern is matched in full)")
        if c in "*+?{":
            self.fail(f"quantifier '{c}' with nothing to repeat")
        if c == "\\":
            kind, val = self.escape()
            return ("set", val if kind == "set" else 1 << val)
        self.i += 1
        raw = c.encode("utf-8")
        if len(raw) == 1:
            return ("set", 1 << raw[0])
        return ("cat", [("set", 1 << b) for b in raw])

    def escape(self):
        """at a backslash -> ("set", mask) or ("byte", value)"""
        if self.i + 1 >= len(self.p):
            self.fail("trailing backslash")
        c = self.p[self.i + 1]
        if c in _CLASS_ESC:
            out = ("set", _CLASS_ESC[c])
        elif c in _CHAR_ESC:
            out = ("byte", _CHAR_ESC[c])
        elif c in _PUNCT:
            out = ("byte", ord(c))
        elif c.isdigit():
            self.fail(f"back-reference '\\{c}'")
        elif c in "bBAZ":
            self.fail(f"anchor '\\{c}'")
        else:
            self.fail(f"escape '\\{c}'")
        self.i += 2
        return out

    def char_class(self):
        self.i += 1
        neg = self.peek() == "^"
        if neg:
            self.i += 1
        m, first = 0, True
        while True:
            c = self.peek()
            if c is None:
                self.fail("unterminated '['")
            if c == "]" and not first:
                self.i += 1
                break
            first = False
            lo = self.class_item()
            if isinstance(lo, tuple):   # \d \w \s
                m |= lo[1]
                continue
            if self.peek() == "-" and self.p[self.i + 1:self.i + 2] not in ("]", ""):
                self.i += 1
                hi = self.class_item()
                if isinstance(hi, tuple) or hi < lo:
                    self.fail("bad character range")
                m |= _mask(range(lo, hi + 1))
            else:
                m |= 1 << lo
        return ("set", (_ALL & ~m) if neg else m)

    def class_item(self):
        c = self.p[self.i]
        if c == "\\":
            kind, val = self.escape()
            return ("set", val) if kind == "set" else val
        if c == "[" and self.p[self.i + 1:self.i + 2] == ":":
            self.fail("POSIX character class")
        if ord(c) > 0x7f:
            self.fail("non-ASCII character inside [...] (Unicode character classes)")
        self.i += 1
        return ord(c)


# ----------------------------------------------------------------------------- AST -> NFA -> DFA over bytes
class _NFA:
    def __init__(self):
        self.eps, self.edges = [], []   # per state: [targets], [(mask, target)]

    def new(self) -> int:
        self.eps.append([])
        self.edges.append([])
        return len(self.eps) - 1

    def build(self, node):
        """-> (start, end) of the fragment (Thompson)"""
        kind = node[0]
        if kind == "set":
            a, b = self.new(), self.new()
            self.edges[a].append((node[1], b))
            return a, b
        if kind == "cat":
            a = b = self.new()
            for item in node[1]:
                s, t = self.build(item)
                self.eps[b].append(s)
                b = t
            return a, b
        if kind == "alt":
            a, b = self.new(), self.new()
            for item in node[1]:
                s, t = self.build(item)
                self.eps[a].append(s)
                self.eps[t].append(b)
            return a, b
        _, sub, lo, hi = node
        a = b = self.new()
        for _ in range(lo):
            s, t = self.build(sub)
            self.eps[b].append(s)
            b = t
        if hi is None:
            s, t = self.build(sub)
            loop = self.new()
            self.eps[b].append(loop)
            self.eps[loop].append(s)
            self.eps[t].append(loop)
            b = loop
        else:
            end = self.new()
            for _ in range(hi - lo):
                s, t = self.build(sub)
                self.eps[b].append(end)
                self.eps[b].append(s)
                b = t
            self.eps[b].append(end)
            b = end
        return a, b


def _closure(nfa: _NFA, states) -> frozenset:
    seen, todo = set(states), list(states)
    while todo:
        for t in nfa.eps[todo.pop()]:
            if t not in seen:
                seen.add(t)
                todo.append(t)
    return frozenset(seen)


def _minimise(table: np.ndarray, accepting: np.ndarray):
    """Moore refinement of a complete DFA whose LAST state is the dead sink -> (table [n, cols] with -1 = dead, accepting [n]),
    start state 0, states from which nothing accepts folded into -1, unreachable ones gone"""
    n = table.shape[0]
    part = accepting.astype(np.int64)
    blocks = len(np.unique(part))
    while True:   # (a refinement only ever splits: the same count is the same partition)
        sig = np.concatenate([part[:, None], part[table]], axis=1)
        _, part = np.unique(sig, axis=0, return_inverse=True)
        part = part.reshape(-1)
        if int(part.max()) + 1 == blocks:
            break
        blocks = int(part.max()) + 1
    dead = part[n - 1]
    # number the blocks in order of discovery from the start state
    order, todo, rep = {}, [0], {}
    for s in range(n):
        rep.setdefault(int(part[s]), s)
    if part[0] == dead:
        return np.full((1, table.shape[1]), -1, np.int32), np.zeros(1, np.uint8)
    order[int(part[0])] = 0
    while todo:
        s = todo.pop()
        for t in np.unique(table[s]):
            b = int(part[t])
            if b != dead and b not in order:
                order[b] = len(order)
                todo.append(rep[b])
    out = np.full((len(order), table.shape[1]), -1, np.int32)
    acc = np.zeros(len(order), np.uint8)
    lut = np.full(int(part.max()) + 1, -1, np.int32)
    for b, k in order.items():
        lut[b] = k
    for b, k in order.items():
        out[k] = lut[part[table[rep[b]]]]
        acc[k] = accepting[rep[b]]
    return out, acc


def byte_automaton(pattern: str):
    """The minimal DFA of `pattern` over bytes: (table int32 [n_states, 256] with -1 = rejected, accepting uint8 [n_states]), start
    state 0.  A prefix is still viable while walking its bytes from state 0 never meets -1."""
    if not isinstance(pattern, str):
        raise ValueError("the pattern must be a string")
    ast = _Parser(pattern).parse()
    nfa = _NFA()
    start, end = nfa.build(ast)
    # bytes that no set of the pattern tells apart behave alike: one column per group
    masks = sorted({m for edges in nfa.edges for m, _ in edges})
    sig = np.zeros((256, max(len(masks), 1)), np.uint8)
    for k, m in enumerate(masks):
        sig[:, k] = [(m >> b) & 1 for b in range(256)]
    _, col_of = np.unique(sig, axis=0, return_inverse=True)
    col_of = col_of.reshape(-1)
    n_cols = int(col_of.max()) + 1
    rep_byte = [int(np.nonzero(col_of == k)[0][0]) for k in range(n_cols)]
    s0 = _closure(nfa, [start])
    ids, rows, todo = {s0: 0}, [], [s0]
    while todo:
        cur = todo.pop()
        row = []
        for k in range(n_cols):
            bit = 1 << rep_byte[k]
            nxt = {t for s in cur for m, t in nfa.edges[s] if m & bit}
            if not nxt:
                row.append(-1)
                continue
            cl = _closure(nfa, nxt)
            if cl not in ids:
                ids[cl] = len(ids)
                todo.append(cl)
            row.append(ids[cl])
        rows.append((ids[cur], row))
        if len(ids) > 32 * MAX_GRAMMAR_STATES:
            raise ValueError("the pattern needs too many states")
    n = len(ids)
    table = np.full((n + 1, n_cols), n, np.int64)   # state n: the dead sink
    for k, row in rows:
        table[k] = [n if t < 0 else t for t in row]
    accepting = np.zeros(n + 1, bool)
    for st, k in ids.items():
        accepting[k] = end in st
    small, acc = _minimise(table, accepting)
    return np.ascontiguousarray(small[:, col_of]), acc


# ----------------------------------------------------------------------------- bytes -> tokens
def _lift(table: np.ndarray, vocab_bytes: Sequence[Optional[bytes]]) -> np.ndarray:
    """next[state, token] (int32, -1 = not allowed): every token walked through every state, one byte position at a time"""
    n, V = table.shape[0], len(vocab_bytes)
    lens = np.array([len(b) if b else 0 for b in vocab_bytes], np.int64)
    width = int(lens.max()) if V else 0
    mat = np.zeros((V, max(width, 1)), np.uint8)
    for i, b in enumerate(vocab_bytes):
        if b:
            mat[i, :len(b)] = np.frombuffer(bytes(b), np.uint8)
    usable = np.nonzero(lens > 0)[0]
    flat = np.concatenate([table, np.full((1, 256), n, table.dtype)]).astype(np.int32)   # row n: the dead sink
    flat[flat < 0] = n
    flat = flat.reshape(-1)
    out = np.full((n, V), -1, np.int32)
    for s in range(n):
        alive, cur = usable, np.full(usable.size, s, np.int32)
        for pos in range(width):
            cur = flat[cur * 256 + mat[alive, pos]]
            keep = cur != n
            alive, cur = alive[keep], cur[keep]
            done = lens[alive] == pos + 1
            out[s, alive[done]] = cur[done]
            alive, cur = alive[~done], cur[~done]
            if alive.size == 0:
                break
    return out


def _from_byte_dfa(table: np.ndarray, accepting: np.ndarray, vocab_bytes) -> TokenAutomaton:
    nxt = _lift(table, vocab_bytes)
    n = nxt.shape[0]
    succ = [np.unique(nxt[s]) for s in range(n)]
    succ = [u[u >= 0] for u in succ]
    # backward reachability ON THE TOKEN AUTOMATON: a state is live when tokens of this vocabulary lead from it to an accepting one
    live = accepting.astype(bool).copy()
    changed = True
    while changed:
        changed = False
        for s in range(n):
            if not live[s] and live[succ[s]].any():
                live[s] = changed = True
    if not live[0]:
        raise ValueError("no sequence of tokens of this vocabulary matches the pattern (the start state is dead)")
    # forward from the start through live states only; renumber in order of discovery
    order, todo = {0: 0}, [0]
    while todo:
        for t in succ[todo.pop()]:
            t = int(t)
            if live[t] and t not in order:
                order[t] = len(order)
                todo.append(t)
    if len(order) > MAX_GRAMMAR_STATES:
        raise ValueError(f"the grammar needs {len(order)} states, more than {MAX_GRAMMAR_STATES}")
    lut = np.full(n + 1, -1, np.int32)   # (index -1 -> -1 as well)
    for s, k in order.items():
        lut[s] = k
    keep = sorted(order, key=order.get)
    small = lut[nxt[keep]]               # transitions into dead or unreachable states are dropped here
    cols = np.ascontiguousarray(small.T.astype(np.int16))
    void = cols.view(np.dtype((np.void, cols.shape[1] * 2))).reshape(-1)
    _, first, inverse = np.unique(void, return_index=True, return_inverse=True)
    if first.size > MAX_GRAMMAR_CLASSES:
        raise ValueError(f"the grammar needs {first.size} token classes, more than {MAX_GRAMMAR_CLASSES}")
    trans = np.ascontiguousarray(cols[first].T)
    return TokenAutomaton(inverse.reshape(-1).astype(np.uint16), trans, np.ascontiguousarray(accepting[keep], dtype=np.uint8))


def compile_regex(pattern: str, vocab_bytes: Sequence[Optional[bytes]]) -> TokenAutomaton:
    """The token automaton of `pattern` (full match over bytes) for the vocabulary vocab_bytes[i] = the bytes of token i, or None for
    a token that is never allowed (specials, reserved ids; tokens of no bytes are never allowed either).  ValueError for an
    unsupported construct, a grammar over the limits, or a pattern no token sequence of this vocabulary can match."""
    table, accepting = byte_automaton(pattern)
    return _from_byte_dfa(table, accepting, vocab_bytes)


_SPECIAL = set("\\.^$*+?{}[]()|")


def escape(text: str) -> str:
    return "".join("\\n" if c == "\n" else "\\t" if c == "\t" else "\\r" if c == "\r" else "\\" + c if c in _SPECIAL else c for c in text)


def compile_choice(strings: Sequence[str], vocab_bytes: Sequence[Optional[bytes]]) -> TokenAutomaton:
    """The alternation of the escaped literals (vLLM's `guided_choice`)."""
    strings = list(strings)
    if not strings or not all(isinstance(s, str) and s for s in strings):
        raise ValueError("guided_choice must be a non-empty list of non-empty strings")
    return compile_regex("|".join("(?:" + escape(s) + ")" for s in strings), vocab_bytes)


# ----------------------------------------------------------------------------- the vocabulary of a byte-level BPE
def _unicode_to_byte() -> dict:
    """the inverse of GPT-2's byte-to-unicode alphabet"""
    bs = list(range(ord("!"), ord("~") + 1)) + list(range(0xa1, 0xad)) + list(range(0xae, 0x100))
    cs, n = bs[:], 0
    for b in range(256):
        if b not in bs:
            bs.append(b)
            cs.append(256 + n)
            n += 1
    return {chr(c): b for b, c in zip(bs, cs)}


def token_bytes(tokenizer, vocab_size: Optional[int] = None) -> list:
    """vocab_bytes of a byte-level BPE ZoomEarthTokenizer (the Qwen tokenizer): the bytes of every token of the model's vocabulary;
    None for added / special tokens and for ids the tokenizer does not have (up to vocab_size, the model's).  ValueError for any
    other tokenizer model."""
    import json
    tok = getattr(tokenizer, "_tok", tokenizer)
    spec = json.loads(tok.to_str())
    model = spec.get("model") or {}
    kinds = json.dumps([spec.get("pre_tokenizer"), spec.get("decoder")])
    if model.get("type") != "BPE" or "ByteLevel" not in kinds:
        raise ValueError(f"token_bytes needs a byte-level BPE tokenizer, not a {model.get('type')} model")
    added = {int(a["id"]) for a in spec.get("added_tokens") or ()}
    vocab = model["vocab"]
    size = max(max(vocab.values(), default=-1), max(added, default=-1)) + 1
    size = max(size, int(vocab_size or 0))
    inv = _unicode_to_byte()
    out = [None] * size
    for piece, i in vocab.items():
        if i in added:
            continue
        try:
            out[i] = bytes(inv[ch] for ch in piece)
        except KeyError:
            out[i] = None   # a piece outside the byte alphabet is no text the model can emit through it
    return out
