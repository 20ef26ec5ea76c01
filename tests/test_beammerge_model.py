"""The numpy restatement of `qg_beam_merge` (tests/beammerge_model.py) on inputs small enough to work out by hand: the state key against
constants computed once with a C program of the formula in include/qgym.h, and each merge rule on a hand-made group."""
import numpy as np

from beammerge_model import GOLDEN, MASK, close_key, merge, order_word, splitmix64, state_key

NINF, NAN = np.float32(-np.inf), np.float32(np.nan)


def test_splitmix64_is_the_published_function():
    assert splitmix64(0) == 0xE220A8397B1DCDAF  # the first output of the generator seeded with 0
    assert splitmix64(1) == 0x910A2DEC89025CC1 and splitmix64(2) == 0x975835DE1C9756CE
    assert splitmix64(0x61C8864680B583EB) == 0  # 2^64 - the increment: every stage of the mix maps 0 to 0


def test_key_of_tiny_inputs():
    assert state_key([0]) == splitmix64(1 ^ splitmix64(splitmix64(1))) == 0x6C5795E14B3B7E33  # n = 1, a zero word
    assert state_key([5]) == 0xF49233EC155161C7
    assert state_key([0, 0]) == 0x98389997F4E6E471 != state_key([0])  # zero words count: the position salts and n enter the key
    assert state_key([1, 2, 3]) == 0xDB2A4535AAAD7722
    assert state_key([3, 2, 1]) == 0x21E4FBDF126FBB88  # the same words in another order are another state
    assert state_key([MASK, 0]) == 0x128D6C63DF0F4671  # the sum wraps
    # the word size does not enter: the words are zero-extended; signed dtypes are read as bit patterns
    assert state_key(np.array([1, 2, 3], dtype=np.uint8)) == state_key(np.array([1, 2, 3], dtype=np.uint64)) == state_key(np.array([1, 2, 3], dtype=np.int32))
    assert state_key(np.array([-1, 0], dtype=np.int64)) == state_key([MASK, 0])
    assert state_key(np.array([-1], dtype=np.int32)) == state_key([0xFFFFFFFF])


def test_key_zero_is_replaced_on_the_final_stage():
    total = 0x61C8864680B583EB ^ 3  # n ^ total is the one argument that splitmix64 maps to 0
    assert splitmix64(3 ^ total) == 0 and close_key(3, total) == GOLDEN
    assert close_key(3, total + 1) == splitmix64(3 ^ (total + 1)) != GOLDEN
    assert close_key(2, MASK + 1 + 7) == close_key(2, 7)  # the sum is taken mod 2^64


def test_order_word():
    assert order_word(NAN) == 0 and order_word(NINF) == 0
    assert order_word(np.float32(0.0)) == order_word(np.float32(-0.0)) == 0x80000000
    assert order_word(np.float32(-1.0)) < order_word(np.float32(-0.5)) < order_word(np.float32(0.0)) < order_word(np.float32(2.0)) < order_word(np.float32(np.inf))


def rows(*ids):
    """One word per slot: slots with the same id hold the same state."""
    return np.array([[i] for i in ids], dtype=np.uint64)


def test_duplicates_the_best_cum_survives_ties_go_to_the_lowest_slot():
    words = rows(7, 7, 7, 9)
    live_out, keys, dropped = merge(words, np.float32([-2.0, -1.0, -1.0, -5.0]), [1, 1, 1, 1], 4)
    assert live_out.tolist() == [0, 1, 0, 1] and dropped.tolist() == [[0, 2]]  # slot 1 beats slot 0 on cum and slot 2 on the tie
    assert keys.tolist() == [state_key([7])] * 3 + [state_key([9])]


def test_minus_zero_ties_with_plus_zero():
    live_out, _, dropped = merge(rows(4, 4), np.float32([0.0, -0.0]), [1, 1], 2)
    assert live_out.tolist() == [1, 0] and dropped.tolist() == [[0, 1]]
    live_out, _, dropped = merge(rows(4, 4), np.float32([-0.0, 0.0]), [1, 1], 2)
    assert live_out.tolist() == [1, 0] and dropped.tolist() == [[0, 1]]  # +0 in the higher slot is not "larger"


def test_a_dead_slot_holding_a_duplicate_key_neither_wins_nor_counts():
    seen = [[]]
    live_out, keys, dropped = merge(rows(3, 3, 3), np.float32([0.0, -1.0, -2.0]), [0, 1, 1], 3, seen, 8)
    assert live_out.tolist() == [0, 1, 0] and dropped.tolist() == [[0, 1]]  # the dead slot 0 has the best cum and stays dead
    assert keys[0] == keys[1] and seen == [[state_key([3])]]  # its key is reported all the same, and recorded once


def test_a_slot_without_an_order_word_is_dropped_and_counted_nowhere():
    seen = [[]]
    live_out, _, dropped = merge(rows(1, 1, 2, 2), np.float32([NAN, -3.0, NINF, NINF]), [1, 1, 1, 1], 4, seen, 8)
    assert live_out.tolist() == [0, 1, 0, 0] and dropped.tolist() == [[0, 0]]
    assert seen == [[state_key([1])]]  # state 2 had no survivor: it is not recorded


def test_a_history_hit_is_a_revisit_and_groups_keep_their_own_history():
    seen = [[state_key([5])], []]
    words = rows(5, 5, 6, 5, 5, 6)
    live_out, _, dropped = merge(words, np.float32([0, -1, -2, 0, -1, -2]), [1] * 6, 3, seen, 8)
    assert live_out.tolist() == [0, 0, 1, 1, 0, 1]
    assert dropped.tolist() == [[2, 0], [0, 1]]  # group 0: both 5s are revisits, not duplicates; group 1 has not seen 5
    assert seen == [[state_key([5]), state_key([6])], [state_key([5]), state_key([6])]]
    live_out, _, dropped = merge(words, np.float32([0, -1, -2, 0, -1, -2]), [1] * 6, 3, seen, 8)
    assert live_out.tolist() == [0] * 6 and dropped.tolist() == [[3, 0], [3, 0]] and [len(h) for h in seen] == [2, 2]


def test_the_history_saturates_in_slot_order_and_then_only_prunes_less():
    seen = [[]]
    live_out, _, _ = merge(rows(1, 2, 3, 4), np.float32([-4, -3, -2, -1]), [1] * 4, 4, seen, 3)
    assert live_out.tolist() == [1, 1, 1, 1]  # all survive
    assert seen == [[state_key([1]), state_key([2]), state_key([3])]]  # slots 0, 1, 2 fit, whatever their cum; slot 3's key is lost
    live_out, _, dropped = merge(rows(4, 1, 4, 5), np.float32([-1, -1, -2, -1]), [1] * 4, 4, seen, 3)
    assert live_out.tolist() == [1, 0, 0, 1] and dropped.tolist() == [[1, 1]]  # 4 was never recorded: no revisit, still merged within the step
    assert len(seen[0]) == 3


def test_without_a_history_only_the_step_is_merged():
    a = merge(rows(1, 1, 2), np.float32([0, 0, 0]), [1, 1, 1], 3)
    b = merge(rows(1, 1, 2), np.float32([0, 0, 0]), [1, 1, 1], 3)
    assert a[0].tolist() == b[0].tolist() == [1, 0, 1] and a[2].tolist() == [[0, 1]]
