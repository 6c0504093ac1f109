"""numpy restatement of guided decoding (include/zoomearth.h, ze_grammar_create / ze_seq_set_grammar; zoomearth_amd/csrc/ze_grammar.hip):
what a state allows, the masked row, and the state after a token.  An automaton is anything with token_class [vocab], trans
[n_states, n_classes] (-1 = not allowed) and accepting [n_states] (zoomearth_amd.grammar.TokenAutomaton)."""
import numpy as np

from token_rules_ref import argmax_lowest  # noqa: F401  (torch.argmax's tie-break, shared by the decode-path checks)


def allowed(auto, state: int, eos_ids, vocab=None) -> np.ndarray:
    """bool [vocab]: the ids `state` allows.  An EOS id follows accepting[state]; its class is never looked at."""
    tc = np.asarray(auto.token_class).astype(np.int64)
    trans = np.asarray(auto.trans)
    ok = np.zeros(tc.size, bool)
    inside = tc < trans.shape[1]
    ok[inside] = trans[state][tc[inside]] >= 0
    for e in eos_ids:
        if 0 <= e < tc.size:
            ok[e] = bool(auto.accepting[state])
    return ok if vocab is None else ok[:vocab]


def mask_row(row, auto, state: int, eos_ids) -> np.ndarray:
    """the row the sampler reads: -inf wherever `state` does not allow the id, every other element as it is (NaN and -inf included);
    state -1 = a row without a grammar"""
    out = np.array(row, dtype=np.float32, copy=True)
    if state < 0:
        return out
    out[~allowed(auto, state, eos_ids, out.size)] = -np.inf
    return out


def advance(auto, state: int, token: int, eos_ids) -> int:
    """the state after `token`, or -1 when the automaton does not allow it (an EOS id keeps an accepting state)"""
    n_states, n_classes = np.asarray(auto.trans).shape
    if not (0 <= state < n_states) or not (0 <= token < len(auto.token_class)):
        return -1
    if token in eos_ids:
        return state if auto.accepting[state] else -1
    c = int(auto.token_class[token])
    return int(auto.trans[state][c]) if c < n_classes else -1


def chain_advance(auto, state: int, violated: int, token: int, eos_ids):
    """(state, violated) of a live chain after it accepted `token`: a token that is not allowed leaves the state and sets violated"""
    nxt = advance(auto, state, token, eos_ids)
    return (state, 1) if nxt < 0 else (nxt, violated)
