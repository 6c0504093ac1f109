"""CPU: the numpy restatement of speculative decoding by prompt lookup (tests/spec_ref.py) on hand-made cases, and the C ABI's
declarations.  The GPU tests hold the kernels to this restatement exactly."""
import ctypes as C

import numpy as np

import spec_ref as S
from zoomearth_amd import _lib


# ---------------------------------------------------------------- drafter
def test_longest_ngram_wins():
    #    the 1-gram [3] last occurred at index 5 (-> 9); the 2-gram [2, 3] at 1 (-> 7): the longer one decides
    h = [1, 2, 3, 7, 8, 3, 9, 2, 3]
    assert S.draft(h, 2, 1, 2) == [7, 8]
    assert S.draft(h, 2, 1, 1) == [9, 2]


def test_most_recent_occurrence_wins():
    h = [5, 6, 10, 5, 6, 20, 30, 5, 6]
    assert S.draft(h, 4, 2, 2) == [20, 30, 5, 6]


def test_the_tail_itself_is_no_occurrence():
    assert S.draft([1, 2, 3, 4], 4, 1, 3) == []          # the only [4] ends the history: nothing follows it
    assert S.draft([4, 4], 4, 1, 3) == [4]               # the earlier 4 has one id behind it: the tail
    assert S.draft([7], 4, 1, 3) == [] and S.draft([], 4, 1, 3) == []


def test_cut_by_history_end_and_by_room():
    h = [1, 2, 3, 9, 1, 2]
    assert S.draft(h, 8, 2, 2) == [3, 9, 1, 2]            # the history ends
    assert S.draft(h, 3, 2, 2) == [3, 9, 1]               # k
    assert S.draft(h, 8, 2, 2, cap=1) == [3] and S.draft(h, 8, 2, 2, cap=0) == []


def test_no_match_and_min_ngram():
    assert S.draft([1, 2, 3, 4, 5], 4, 1, 3) == []
    h = [1, 2, 8, 3, 2]
    assert S.draft(h, 4, 1, 3) == [8, 3, 2]               # only the 1-gram [2] repeats
    assert S.draft(h, 4, 2, 3) == []                      # ... and min_ngram = 2 does not take it


# ---------------------------------------------------------------- accept pass
V = 32


def rows_for(winners, runner_up=None):
    r = np.full((len(winners), V), -1.0, dtype=np.float32)
    for j, w in enumerate(winners):
        r[j, w] = 5.0
        if runner_up is not None:
            r[j, runner_up[j]] = 4.0
    return r


def test_all_none_and_middle():
    assert S.accept(rows_for([3, 4, 5]), [3, 4], np.zeros(V, np.uint8)) == ([3, 4, 5], False)
    assert S.accept(rows_for([9, 4, 5]), [3, 4], np.zeros(V, np.uint8)) == ([9], False)
    assert S.accept(rows_for([3, 9, 5]), [3, 4], np.zeros(V, np.uint8)) == ([3, 9], False)


def test_eos_inside_the_draft_stops_behind_it():
    seen = np.zeros(V, np.uint8)
    assert S.accept(rows_for([3, 30, 5]), [3, 30], seen, eos_ids=(30,)) == ([3, 30], True)
    assert seen[3] and seen[30] and not seen[5]
    assert S.accept(rows_for([3, 30, 5]), [3, 30], np.zeros(V, np.uint8), eos_ids=(30,), ignore_eos=True) == ([3, 30, 5], False)


def test_an_accepted_id_flips_a_later_row_under_the_penalty():
    # row 1: id 3 at 5.0 against id 7 at 4.0 -- id 3 was emitted by row 0, and 5.0 / 1.3 < 4.0
    rows = rows_for([3, 3], runner_up=[8, 7])
    assert S.accept(rows, [3], np.zeros(V, np.uint8), penalty=1.0) == ([3, 3], False)
    assert S.accept(rows, [3], np.zeros(V, np.uint8), penalty=1.3) == ([3, 7], False)


def test_the_room_ends_the_walk_mid_draft():
    assert S.accept(rows_for([3, 4, 5]), [3, 4], np.zeros(V, np.uint8), room=2) == ([3, 4], False)
    assert S.accept(rows_for([3, 4, 5]), [3, 4], np.zeros(V, np.uint8), room=1) == ([3], False)


def test_ties_and_nan_rows():
    r = np.zeros((1, V), np.float32)
    assert S.accept(r, [], np.zeros(V, np.uint8)) == ([0], False)
    r[:] = np.nan
    assert S.accept(r, [], np.zeros(V, np.uint8)) == ([0], False)


# ---------------------------------------------------------------- the C ABI
def test_the_abi_declares_the_entries():
    for name in ("ze_seq_set_speculation", "ze_chain_spec_stats", "ze_op_spec_draft", "ze_op_spec_accept", "ze_op_decode_rows"):
        assert name in _lib.EXPORTS
    res, args = _lib._SIGS["ze_seq_set_speculation"]
    assert res is C.c_int and len(args) == 8
