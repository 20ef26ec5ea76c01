"""tests/logcap_model.py against tests/envmodel.Model where the two must agree (a log that never fills), and against hand-written
truncations and values where only the restated contract speaks."""
import numpy as np
import pytest

from envmodel import Model
from logcap_model import LAST_EXACT, SATURATED, PushRecorder, reported
from util import grid_gateset, line_gateset

WILD = [-1, 2**31 - 2, 2**31 - 1, 2**31, 2**32 - 2, 2**32 - 1, 2**32, 2**32 + 5, -2**32 + 5, 2**63 - 1, -2**63]


@pytest.mark.parametrize("add_inverts", [False, True])
@pytest.mark.parametrize("kind,n", [("clifford", 4), ("linear_function", 5), ("permutation", 9)])
def test_a_log_that_never_fills_is_the_models(kind, n, add_inverts):
    gs = grid_gateset("permutation", 3, 3) if kind == "permutation" else line_gateset(kind, n)
    B, T, A = 24, 11, len(gs)
    m = Model(kind, n, gs, B, add_inverts=add_inverts, track_solution=True, max_depth=64)
    rec = PushRecorder(kind, B, A)
    rng = np.random.default_rng(n + add_inverts)
    for episode in range(2):
        m.reset_with(rng.integers(0, A, size=(3, B)))
        rec.clear()
        for t in range(T):
            acts = rng.integers(0, A, size=B)
            acts[t % 5::5] = [WILD[(t + i) % len(WILD)] for i in range(len(acts[t % 5::5]))]
            acts[(t + 2) % 7::7] = A + (t % 2) * 3
            coins = rng.integers(0, 2, size=B)
            rec.note_model(m, acts)
            m.step(acts, coins)
            want = [[reported(v, kind) for v in s] for s in m.solutions()]
            assert rec.expected_log(T) == want and rec.expected_log(10**6) == want, (episode, t)
            assert not rec.overflowed(T).any()
            if kind == "permutation":
                assert (rec.counts() <= t + 1).all() and (rec.counts() < t + 1).any()
            else:
                assert (rec.counts() == t + 1).all()
    if add_inverts:  # both frames were logged
        assert any(inv for p in rec.pushes for _, inv in p) and any(not inv for p in rec.pushes for _, inv in p)
    # a partial clear keeps the other envs' pushes
    before = rec.counts()
    rec.clear(np.arange(B) % 2 == 0)
    assert (rec.counts()[::2] == 0).all() and (rec.counts()[1::2] == before[1::2]).all()


def _recorded(kind, pushes, A=10):
    rec = PushRecorder(kind, 1, A)
    for a, inv in pushes:
        rec.note([a], [inv])
    return rec


def test_truncations_written_out_by_hand():
    # pushes in order: 1, 2 into solution, then 3, 4, 5 into solution_inv -> solution ++ reverse(solution_inv) = 1 2 5 4 3
    rec = _recorded("clifford", [(1, False), (2, False), (3, True), (4, True), (5, True)])
    assert rec.expected_log(5) == [[1, 2, 5, 4, 3]] and not rec.overflowed(5)[0]
    assert rec.expected_log(4) == [[1, 2, 4, 3]] and rec.overflowed(4)[0]  # the cut falls inside the solution_inv part: its last push goes
    assert rec.expected_log(2) == [[1, 2]] and rec.overflowed(2)[0]  # between the parts
    assert rec.expected_log(1) == [[1]] and rec.overflowed(1)[0]
    assert rec.expected_faults(4).tolist() == [8] and rec.expected_faults(5).tolist() == [0]
    # frames interleaved, an out-of-range and a negative action among them
    rec = _recorded("linear_function", [(7, True), (10, False), (-1, True), (3, False), (2**31 - 1, False), (4, True)])
    assert rec.expected_log(6) == [[10, 3, SATURATED, 4, SATURATED, 7]]
    assert rec.expected_log(4) == [[10, 3, SATURATED, 7]]
    assert rec.expected_log(3) == [[10, SATURATED, 7]]
    assert rec.expected_log(1) == [[7]]
    # PermutationEnv: out-of-range actions are no pushes, so they do not count towards the capacity
    rec = _recorded("permutation", [(3, False), (10, False), (-1, False), (4, True), (13, True), (5, False)])
    assert rec.counts().tolist() == [3]
    assert rec.expected_log(3) == [[3, 5, 4]] and not rec.overflowed(3)[0]
    assert rec.expected_log(2) == [[3, 4]] and rec.overflowed(2)[0]
    assert rec.expected_log(1) == [[3]]


def test_reported_values():
    assert LAST_EXACT == 2**31 - 2 and SATURATED == 2**64 - 1
    for kind in ("clifford", "linear_function"):
        got = [reported(v, kind) for v in (2**31 - 2, 2**31 - 1, 2**32 - 2, 2**32 - 1, 2**32 + 5, -1, 2**63 - 1, -2**63)]
        assert got == [2**31 - 2] + [2**64 - 1] * 7, kind
        assert [reported(v, kind) for v in (0, 1, 169, 2**31 - 3)] == [0, 1, 169, 2**31 - 3]
        assert reported(2**64 - 1, kind) == 2**64 - 1 and reported(2**63, kind) == 2**64 - 1  # a negative int64 after `as usize`
    for kind in ("permutation", "pauli"):
        assert [reported(v, kind) for v in (0, 5, 169)] == [0, 5, 169]
    with pytest.raises(AssertionError):
        reported(0, "toffoli")
