"""CPU: the grammar compiler (zoomearth_amd/grammar.py) against Python's `re`, liveness under a vocabulary that lacks a byte, the
stage-1 pattern against the host loop's own parsers, the numpy restatement on a hand-written automaton, and the host layers
(the scheduler's grammar cache, the server's validation) against a stub engine."""
import re
import types

import numpy as np
import pytest

import grammar_ref as R
from tiny_tok import make_bpe_tokenizer
from zoomearth_amd import grammar as G
from zoomearth_amd import hostloop


@pytest.fixture(scope="module")
def tok():
    return make_bpe_tokenizer()


@pytest.fixture(scope="module")
def vocab(tok):
    return G.token_bytes(tok)


def run(auto, ids):
    """True iff the automaton walks `ids` without meeting -1 and ends in an accepting state"""
    s = 0
    for t in ids:
        s = auto.step(s, t)
        if s < 0:
            return False
    return bool(auto.accepting[s])


def distances(auto):
    """token steps from every state to the nearest accepting one"""
    n = auto.trans.shape[0]
    succ = [set(int(t) for t in auto.trans[s] if t >= 0) for s in range(n)]
    dist = np.where(np.asarray(auto.accepting) > 0, 0, 10 ** 6)
    for _ in range(n):
        for s in range(n):
            for t in succ[s]:
                dist[s] = min(dist[s], dist[t] + 1)
    return dist


def walk(auto, dist, rng, free_steps, finish):
    """a random walk: `free_steps` uniform steps over the allowed ids, then (finish) downhill to an accepting state"""
    s, ids = 0, []
    for _ in range(free_steps):
        ok = auto.allowed(s)
        if ok.size == 0:
            break
        t = int(rng.choice(ok))
        ids.append(t)
        s = auto.step(s, t)
    while finish and not auto.accepting[s]:
        ok = auto.allowed(s)
        nxt = auto.trans[s][auto.token_class[ok]]
        down = ok[dist[nxt] < dist[s]]
        t = int(rng.choice(down))
        ids.append(t)
        s = auto.step(s, t)
    return ids


PATTERNS = [
    G.STAGE1_BBOX,
    r'(yes|no|maybe so)',                                   # alternation of literals, a group
    r'\d+(\.\d+)?',                                         # + ? \d, an escaped dot
    r'[a-c]{2,4}x*',                                        # a range, {m,n}, *
    r'w\d{3}( w\d{3})*',                                    # {m}, a repeated group
    r'[^0-9\n]+\n',                                         # a negated class, \n
    r'\w+\s\w+\t?',                                         # \w \s \t
    r'.{1,6}\\\[ok\]',                                      # . and escaped punctuation, an escaped backslash
    r'(?:café|naïve) [A-Z][a-z-]*',               # non-ASCII literals through their UTF-8 bytes, '-' inside a class
    r'"bbox_2d": ?\[\d{1,4}(, ?\d{1,4}){3}\]',              # the box alone
    r'(a|b)*abb',                                           # the subset construction has something to do
]


@pytest.mark.parametrize("pattern", PATTERNS)
def test_compiler_agrees_with_re(pattern, vocab):
    auto = G.compile_regex(pattern, vocab)
    assert auto.trans.shape[0] <= G.MAX_GRAMMAR_STATES and auto.trans.shape[1] <= G.MAX_GRAMMAR_CLASSES
    assert auto.token_class.dtype == np.uint16 and auto.trans.dtype == np.int16 and auto.accepting.dtype == np.uint8
    ref = re.compile(pattern.encode("utf-8"))
    dist = distances(auto)
    rng = np.random.default_rng(5)
    usable = np.array([i for i, b in enumerate(vocab) if b])
    cases = []
    for _ in range(60):                                               # walks stopped at an accepting state
        cases.append(walk(auto, dist, rng, int(rng.integers(0, 6)), True))
    for _ in range(30):                                               # walks stopped at random
        cases.append(walk(auto, dist, rng, int(rng.integers(0, 8)), False))
    for k in range(30):                                               # accepted walks with one id dropped or replaced
        ids = list(cases[k])
        j = int(rng.integers(0, len(ids)))
        ids[j:j + 1] = [] if k % 2 else [int(rng.choice(usable))]
        cases.append(ids)
    for _ in range(40):                                               # uniform draws
        cases.append([int(t) for t in rng.choice(usable, size=int(rng.integers(0, 5)))])
    accepted = 0
    for ids in cases:
        data = b"".join(vocab[t] for t in ids)
        want = ref.fullmatch(data) is not None
        assert run(auto, ids) == want, (pattern, ids, data)
        accepted += want
    assert accepted >= len(cases) / 4 and len(cases) - accepted >= len(cases) / 4, (pattern, accepted, len(cases))


@pytest.mark.parametrize("bad", [r'^a', r'a$', r'(a)\1', r'(?P<n>a)(?P=n)', r'(?=a)a', r'(?!a)b', r'(?<=a)b', r'a*?', r'a+?', r'a??',
                                 r'a{1,2}?', r'(?i)a', r'\bword', r'a\Z', r'\Aa', r'a*+', r'[[:alpha:]]', r'\x41', r'\D', r'a{2,1}',
                                 r'a{x}', r'(a', r'a)', r'[abc', r'*a', '[é]', 'a\\'])
def test_unsupported_constructs_raise(bad, vocab):
    with pytest.raises(ValueError, match="unsupported regular expression construct"):
        G.compile_regex(bad, vocab)


def test_limits_and_inputs(vocab):
    with pytest.raises(ValueError, match="states"):
        G.compile_regex(r'(a|b)*a(a|b){12}', vocab)                   # 2^13 states: over ZE_MAX_GRAMMAR_STATES
    with pytest.raises(ValueError):
        G.compile_choice([], vocab)
    auto = G.compile_choice(["a.b", "x|y", "(z)"], vocab)             # the literals are escaped
    ids = {b: i for i, b in enumerate(vocab) if b}
    assert run(auto, [ids[c.encode()] for c in "a.b"]) and run(auto, [ids[c.encode()] for c in "x|y"])
    assert not run(auto, [ids[b"a"], ids[b"x"], ids[b"b"]]) and not run(auto, [ids[b"x"]])
    from tiny_tok import make_tokenizer
    with pytest.raises(ValueError, match="byte-level BPE"):
        G.token_bytes(make_tokenizer())                               # a word-level model


def test_token_bytes_inverts_the_byte_alphabet(tok, vocab):
    assert len(vocab) == 2048 and all(vocab[i] is None for i in range(2002, 2048))
    assert sorted(b for b in vocab[:256]) == [bytes([i]) for i in range(256)]       # the 256 byte tokens
    for text in ['w12 "bbox_2d":[3,4,50,60] café', " \n\t<think>"]:
        ids = tok.encode(text)
        assert b"".join(vocab[t] for t in ids) == text.encode("utf-8")
    assert len(G.token_bytes(tok, 4096)) == 4096


# ---------------------------------------------------------------- 2. liveness under the vocabulary
def test_transitions_into_states_that_cannot_complete_are_dropped():
    voc = [b"a", b"b", b"c", b"e", None, b"cde", b""]                  # no token holds a lone 'd'
    auto = G.compile_regex(r'(ab|cd)e', voc)
    assert auto.step(0, 2) == -1                                       # 'c' is fine for the bytes, a dead end for these tokens
    assert auto.step(0, 0) >= 0 and run(auto, [0, 1, 3]) and run(auto, [5]) and not run(auto, [2])
    assert auto.step(0, 4) == -1 and auto.step(0, 6) == -1             # a special, a token of no bytes
    dist = distances(auto)
    assert (dist < 10 ** 6).all()                                      # every state of the automaton can complete
    for s in range(auto.trans.shape[0]):
        assert auto.accepting[s] or auto.allowed(s).size > 0
    with pytest.raises(ValueError, match="start state is dead"):
        G.compile_regex(r'cd', voc[:5])
    with pytest.raises(ValueError, match="start state is dead"):
        G.compile_regex(r'a+d', voc)


# ---------------------------------------------------------------- 3. the stage-1 pattern and the host loop's parsers
def test_stage1_replies_parse(vocab):
    auto = G.compile_regex(G.STAGE1_BBOX, vocab)
    dist = distances(auto)
    rng = np.random.default_rng(9)
    for k in range(200):
        ids = walk(auto, dist, rng, int(rng.integers(0, 40)), True)
        text = b"".join(vocab[t] for t in ids).decode("utf-8", "replace")
        boxes = hostloop.extract_bbox(text, 1)
        assert len(boxes) == 1 and len(boxes[0]) == 4, (k, text, boxes)
        assert hostloop.extract_answer(text) is not None, (k, text)


# ---------------------------------------------------------------- 4. the restatement on a hand-written automaton
class Hand:
    # ids 0..5: classes a a b c b -; id 5 is the EOS.  0 -a-> 1 -b-> 2 (accepting) -c-> 0
    token_class = np.array([0, 0, 1, 2, 1, 7], np.uint16)
    trans = np.array([[1, -1, -1], [-1, 2, -1], [-1, -1, 0]], np.int16)
    accepting = np.array([0, 0, 1], np.uint8)


def test_restatement_on_a_hand_written_automaton():
    eos = (5,)
    assert R.allowed(Hand, 0, eos).tolist() == [True, True, False, False, False, False]
    assert R.allowed(Hand, 1, eos).tolist() == [False, False, True, False, True, False]
    assert R.allowed(Hand, 2, eos).tolist() == [False, False, False, True, False, True]
    row = np.array([1.0, np.nan, 3.0, -np.inf, -0.0, 2.0], np.float32)
    got = R.mask_row(row, Hand, 1, eos)
    assert np.isneginf(got[[0, 1, 3, 5]]).all() and got[2] == 3.0 and np.signbit(got[4]) and got[4] == 0.0
    assert np.array_equal(R.mask_row(row, Hand, -1, eos).view(np.uint32), row.view(np.uint32))
    assert np.isnan(R.mask_row(row, Hand, 0, eos)[1])
    assert [R.advance(Hand, 0, t, eos) for t in range(6)] == [1, 1, -1, -1, -1, -1]
    assert [R.advance(Hand, 2, t, eos) for t in range(6)] == [-1, -1, -1, 0, -1, 2]
    assert R.advance(Hand, 3, 0, eos) == -1 and R.advance(Hand, 0, 6, eos) == -1 and R.advance(Hand, -1, 0, eos) == -1
    assert R.chain_advance(Hand, 1, 0, 2, eos) == (2, 0) and R.chain_advance(Hand, 1, 0, 0, eos) == (1, 1)
    assert R.chain_advance(Hand, 2, 1, 5, eos) == (2, 1)


# ---------------------------------------------------------------- 5. host layers against a stub engine
class StubEngine:
    max_seqs = 2

    def __init__(self):
        self.live, self.made, self.log, self.slots = set(), 0, [], {}

    def grammar_create(self, automaton):
        assert len(self.live) < 16
        gid = min(set(range(16)) - self.live)
        self.live.add(gid)
        self.made += 1
        return gid

    def grammar_destroy(self, gid):
        assert gid in self.live and gid not in self.slots.values()
        self.live.remove(gid)

    def set_grammar(self, slot, gid, state=0):
        if gid is None:
            self.slots.pop(slot, None)
        else:
            self.slots[slot] = gid


def test_scheduler_keeps_an_lru_of_compiled_grammars():
    from zoomearth_amd.scheduler import ChainScheduler, GrammarCache, Request
    eng, compiled = StubEngine(), []

    def compile_key(key):
        if key[1] == "(":
            raise ValueError("unsupported regular expression construct")
        compiled.append(key)
        return key

    cache = GrammarCache(eng, compile_key, 16)
    keys = [("regex", f"p{i}") for i in range(16)]
    ids = [cache.acquire(k) for k in keys]
    assert sorted(ids) == list(range(16)) and len(compiled) == 16
    assert cache.acquire(keys[3]) == ids[3] and len(compiled) == 16          # compiled once per pattern
    with pytest.raises(RuntimeError, match="in use"):                        # every grammar has a live chain: refused, nothing evicted
        cache.acquire(("regex", "new"))
    assert len(eng.live) == 16 and set(cache.ids) == set(keys)
    cache.release(keys[3])
    cache.release(keys[3])
    cache.release(keys[7])
    cache.release(keys[0])
    cache.acquire(keys[0])
    cache.release(keys[0])                                                   # keys[0] is idle too, but used more recently
    with pytest.raises(ValueError):
        cache.acquire(("regex", "("))                                        # a bad pattern evicts nothing
    assert len(eng.live) == 16
    new = cache.acquire(("regex", "new"))
    assert new == ids[7] and keys[7] not in cache.ids and keys[3] in cache.ids   # the least recently used idle one went (3 was touched later)
    cache.acquire(("choice", ("a", "b")))
    assert keys[3] not in cache.ids and keys[0] in cache.ids and len(eng.live) == 16
    # the scheduler's side: the request's grammar goes into its slot, and leaves it when the chain is over
    sched = object.__new__(ChainScheduler)
    sched.engine, sched.grammars = eng, cache
    req = Request(prompt="x", images=[], guided_choice=["a", "b"])
    req.slot = 1
    sched._set_grammar(req)
    assert eng.slots == {1: cache.ids[("choice", ("a", "b"))]} and cache.users[("choice", ("a", "b"))] == 2
    sched._drop_grammar(req)
    sched._drop_grammar(req)                                                 # (once)
    assert eng.slots == {} and cache.users[("choice", ("a", "b"))] == 1
    plain = Request(prompt="x", images=[])
    plain.slot = 0
    sched._set_grammar(plain)
    sched._drop_grammar(plain)
    assert eng.slots == {}
    with pytest.raises(ValueError, match="exclude"):
        sched._set_grammar(Request(prompt="x", images=[], guided_regex="a", guided_choice=["a"]))


def test_server_validates_the_guided_fields(tok):
    from zoomearth_amd import serve
    from zoomearth_amd.config import ModelConfig
    from zoomearth_amd.modeling import ZoomEarthForConditionalGeneration

    class Model:
        config = ModelConfig.tiny()
        engine = StubEngine()

    model = Model()
    model.compile_grammar = types.MethodType(ZoomEarthForConditionalGeneration.compile_grammar, model)
    srv = serve.ChatServer(model, types.SimpleNamespace(tokenizer=tok), "ZoomEarth")
    base = {"messages": [{"role": "user", "content": "w3 w6"}]}
    p = srv._parse({**base, "guided_regex": r"w\d+"})
    assert p.guided_regex == r"w\d+" and p.guided_choice is None and p.guided() and p.adjusts()
    assert p.adjust_kw(tok)["guided_regex"] == r"w\d+"
    p = srv._parse({**base, "guided_choice": ["yes", "no"]})
    assert p.guided_choice == ["yes", "no"] and p.guided_regex is None
    auto = model.compile_grammar(guided_choice=["yes", "no"], tokenizer=tok)
    assert auto is model.compile_grammar(guided_choice=["yes", "no"], tokenizer=tok)       # the host memo
    assert len(auto.token_class) == 2048
    p = srv._parse(base)
    assert not p.guided() and not p.adjusts() and p.adjust_kw(tok) == {}
    for bad in (dict(guided_regex=5), dict(guided_regex=["a"]), dict(guided_regex="a*?"), dict(guided_regex="(a"),
                dict(guided_choice="yes"), dict(guided_choice=[]), dict(guided_choice=["a", 5]), dict(guided_choice=[""]),
                dict(guided_regex="a", guided_choice=["a"]), dict(guided_regex="<|im_end|>☃{3}ÿ")):
        if bad == dict(guided_regex="<|im_end|>☃{3}ÿ"):
            continue   # (compiles: every byte has a token)
        with pytest.raises(serve.BadRequest):
            srv._parse({**base, **bad})
    with pytest.raises(ValueError, match="exclude"):
        model.compile_grammar(guided_regex="a", guided_choice=["a"], tokenizer=tok)
    with pytest.raises(ValueError, match="tokenizer"):
        model.compile_grammar(guided_regex="a")
