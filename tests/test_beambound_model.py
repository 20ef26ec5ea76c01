"""tests/beambound_model.py, the CPU restatement `qg_beam_advance` and the bounded beam search are compared with, checked on its own: the
five rules on hand-made rows, and the exactness of the "stop" bound -- on the oracle's envs under the reference's trained policies
(tests/golden/policies) the search that ends a target once none of its beams can beat its winner returns, list for list, what
`beammodel.beam_search` returns, in cases where the bound demonstrably fires."""
import numpy as np
import pytest

from beambound_model import advance, beam_search_bounded
from beammodel import beam_search
from oracle import OracleEnv
from test_reference_policies import MODELS, load

NINF = np.float32(-np.inf)
F = np.float32


def run(W, rows, best, found, mode, bonus=1.0, skip=-7, ret_in=None, bounded=None):
    """rows: per slot (parent, reward, success, done, live); the returns before the step are `ret_in` (default: all 0, so r = reward)."""
    parent, reward, success, done, live = (list(x) for x in zip(*rows))
    ret_in = np.zeros(len(rows), dtype=np.float32) if ret_in is None else np.asarray(ret_in, dtype=np.float32)
    ret, live, best, found, win_src, group_live, bounded = advance(parent, ret_in, np.asarray(reward, dtype=np.float32), success, done, live,
                                                                   np.asarray(best, dtype=np.float32), np.asarray(found, dtype=np.uint8), W, skip, bonus, mode,
                                                                   bounded)
    return dict(ret=ret, live=live.tolist(), best=best, found=found.tolist(), win_src=win_src.tolist(), group_live=group_live.tolist(),
                bounded=bounded.tolist())


def test_returns_follow_the_parent_and_dead_slots_get_zero():
    # slot 0 descends from slot 1 and slot 1 from slot 0; slot 2 is dead: its parent (out of range) is not read
    o = run(3, [(1, -0.5, 0, 0, 1), (0, -0.25, 0, 0, 1), (99, 5.0, 1, 1, 0)], [NINF], [0], None, ret_in=[-1.0, -2.0, -4.0])
    assert o["ret"].tolist() == [-2.5, -1.25, 0.0] and o["live"] == [1, 1, 0] and o["win_src"] == [-7] and o["found"] == [0] and o["group_live"] == [2]
    # one f32 addition: 1 + 2^-24 rounds to 1 in f32
    o = run(1, [(0, 2.0 ** -24, 0, 0, 1)], [NINF], [0], None, ret_in=[1.0])
    assert o["ret"].view(np.uint32).tolist() == [F(1.0).view(np.uint32)]


def test_two_solved_slots_of_equal_return_the_lowest_slot_wins():
    rows = [(0, 0.5, 0, 0, 1), (1, 0.75, 1, 1, 1), (2, 0.75, 1, 1, 1), (3, 0.7, 1, 1, 1)]
    o = run(4, rows, [NINF], [0], None)
    assert o["win_src"] == [1] and o["best"].tolist() == [0.75] and o["found"] == [1] and o["live"] == [1, 0, 0, 0]
    # in the second group of two the index is batch-wide; a larger return in a later slot beats an earlier one
    o = run(4, rows + [(4, 0.1, 1, 1, 1), (5, 0.9, 0, 0, 1), (6, 0.2, 1, 1, 1), (7, 0.2, 1, 1, 1)], [NINF, 0.1], [0, 1], None)
    assert o["win_src"] == [1, 6] and o["best"].tolist() == [0.75, F(0.2)] and o["group_live"] == [1, 1]
    # success without live is no result
    o = run(2, [(0, 0.9, 1, 1, 0), (1, 0.5, 1, 1, 1)], [NINF], [0], None)
    assert o["win_src"] == [1] and o["best"].tolist() == [0.5]


def test_a_return_equal_to_best_does_not_replace_the_winner():
    o = run(2, [(0, 0.75, 1, 1, 1), (1, 0.5, 0, 0, 1)], [0.75], [1], None)
    assert o["win_src"] == [-7] and o["best"].tolist() == [0.75] and o["found"] == [1] and o["live"] == [0, 1]
    # below best as well; and found stays 0 where nothing was found (best = -inf is beaten by any finite return, but not by -inf or NaN)
    o = run(2, [(0, 0.7, 1, 1, 1), (1, 0.5, 0, 0, 1)], [0.75], [1], None)
    assert o["win_src"] == [-7]
    o = run(2, [(0, NINF, 1, 1, 1), (1, np.nan, 1, 1, 1)], [NINF], [0], "stop")
    assert o["win_src"] == [-7] and o["found"] == [0] and o["live"] == [0, 0] and o["bounded"] == [0]


def test_reaching_best_exactly_is_hopeless():
    # best 0.75 (already found); slot 0: -0.25 + 1 == 0.75 hopeless; slot 1: -0.25 + 2^-23, whose sum with 1 is exact: hopeful; slot 2: well below
    up = F(F(-0.25) + F(2.0 ** -23))
    rows = [(0, -0.25, 0, 0, 1), (1, up, 0, 0, 1), (2, -0.5, 0, 0, 1)]
    assert F(up + F(1.0)) > F(0.75)
    o = run(3, rows, [0.75], [1], "prune")
    assert o["live"] == [0, 1, 0] and o["bounded"] == [2] and o["group_live"] == [1]
    o = run(3, rows, [0.75], [1], "stop")  # one hopeful slot keeps the whole group
    assert o["live"] == [1, 1, 1] and o["bounded"] == [0] and o["group_live"] == [3]
    o = run(3, [rows[0], rows[2], (2, 0.0, 0, 0, 0)], [0.75], [1], "stop", bounded=[5])  # none hopeful: all end; the count accumulates
    assert o["live"] == [0, 0, 0] and o["bounded"] == [7] and o["group_live"] == [0]
    o = run(3, rows, [0.75], [1], None)
    assert o["live"] == [1, 1, 1] and o["bounded"] == [0]
    # the bound reads the best of THIS step: slot 0 wins with 0.75, which makes slot 1 (-0.25) hopeless at once
    o = run(2, [(0, 0.75, 1, 1, 1), (1, -0.25, 0, 0, 1)], [NINF], [0], "stop")
    assert o["win_src"] == [0] and o["live"] == [0, 0] and o["bounded"] == [1]
    # rounding is the search's own: -2^-25 + 1 rounds to 1.0 in f32, which does not exceed a best of 1.0
    o = run(1, [(0, -(2.0 ** -25), 0, 0, 1)], [1.0], [1], "prune")
    assert o["live"] == [0] and o["bounded"] == [1]
    # bonus = +inf: nothing finite is hopeless
    o = run(3, rows, [0.75], [1], "prune", bonus=np.inf)
    assert o["live"] == [1, 1, 1] and o["bounded"] == [0]


def test_a_group_without_a_winner_is_never_bounded():
    rows = [(0, -50.0, 0, 0, 1), (1, -60.0, 0, 0, 1)]
    for mode in ("stop", "prune"):
        o = run(2, rows, [0.75], [0], mode)  # found == 0 decides, whatever best holds
        assert o["live"] == [1, 1] and o["bounded"] == [0] and o["found"] == [0] and o["best"].tolist() == [0.75]
        o = run(2, rows, [NINF], [0], mode)
        assert o["live"] == [1, 1] and o["bounded"] == [0]


def test_a_beam_that_ends_without_success_leaves_and_is_not_counted_as_bounded():
    rows = [(0, -0.5, 0, 1, 1), (1, -0.1, 0, 0, 1)]
    for mode in (None, "stop", "prune"):
        o = run(2, rows, [NINF], [0], mode)
        assert o["live"] == [0, 1] and o["win_src"] == [-7] and o["bounded"] == [0] and o["group_live"] == [1]
    o = run(2, rows, [0.95], [1], "prune")  # with a winner: slot 0 left by rule 3 (not counted), slot 1 by the bound (counted)
    assert o["live"] == [0, 0] and o["bounded"] == [1]


def test_an_all_dead_group():
    rows = [(7, 9.0, 1, 1, 0), (8, 9.0, 1, 0, 0)]
    for mode in (None, "stop", "prune"):
        for best, found in (([NINF], [0]), ([0.0], [1])):
            o = run(2, rows, best, found, mode)
            assert o["ret"].tolist() == [0.0, 0.0] and o["live"] == [0, 0] and o["win_src"] == [-7] and o["group_live"] == [0] and o["bounded"] == [0]
            assert o["found"] == found and o["best"].tolist() == best


def test_minus_zero_equals_plus_zero():
    # equal returns -0.0 and +0.0: the lowest slot wins and best keeps its bits
    o = run(2, [(0, -0.0, 1, 1, 1), (1, 0.0, 1, 1, 1)], [NINF], [0], None, ret_in=[-0.0, 0.0])
    assert o["win_src"] == [0] and o["best"].view(np.uint32).tolist() == [0x80000000]
    # +0.0 does not beat a best of -0.0, nor the other way round
    assert run(1, [(0, 0.0, 1, 1, 1)], [-0.0], [1], None)["win_src"] == [-7]
    assert run(1, [(0, -0.0, 1, 1, 1)], [0.0], [1], None, ret_in=[-0.0])["win_src"] == [-7]
    # r + bonus = -0.0 against best = +0.0: equal, hence hopeless
    o = run(1, [(0, -0.0, 0, 0, 1)], [0.0], [1], "prune", bonus=-0.0, ret_in=[-0.0])
    assert o["ret"].view(np.uint32).tolist() == [0x80000000] and o["live"] == [0] and o["bounded"] == [1]


# ---- exactness of "stop" ---------------------------------------------------------------------------------------------------------------------
# (difficulty, seed) per policy, chosen on the CPU so that the bound fires in at least half of the solved groups at W = 4 (the share is asserted)
CASES = {"clifford_3q_custom": (4, 2), "lf_5_line": (4, 2), "perm_square_3x3": (3, 1)}


def golden_model_case(name, count=32):
    """The targets of tests/test_gpu_beam.py's `golden_case` (`count` scrambled ones, then one that is solved on arrival) as oracle envs
    with the solution log on, and `logp_of`: the policy's log_softmax in numpy f32."""
    difficulty, seed = CASES[name]
    cfg, gateset, w = load(name)
    kind, n, A = MODELS[name], cfg["num_qubits"], len(gateset)
    kw = dict(add_inverts=0, add_perms=0, depth_slope=cfg["depth_slope"], max_depth=cfg["max_depth"])
    rng = np.random.default_rng(seed)
    states = []
    for _ in range(count):
        env = OracleEnv(kind, n, gateset, track_solution=0, difficulty=difficulty, **kw)
        env.reset_with(rng.integers(0, A, size=difficulty))
        states.append(env.get_state().tolist())
    states.append(OracleEnv(kind, n, gateset, add_inverts=0, add_perms=0).get_state().tolist())
    targets = []
    for s in states:
        env = OracleEnv(kind, n, gateset, track_solution=1, difficulty=1, **kw)
        env.set_state(s)
        targets.append(env)

    def logp_of(t, envs):
        out = np.zeros((len(envs), A), dtype=np.float32)
        rows = [b for b, e in enumerate(envs) if e is not None]
        x = np.stack([np.asarray(envs[b].dense_obs()).reshape(-1) for b in rows]).astype(np.float32)
        h = np.maximum(x @ w["embeddings_weight"].T + w["embeddings_bias"], 0)
        h = np.maximum(h @ w["common_0_weight"].T + w["common_0_bias"], 0)
        z = h @ w["action_0_weight"].T + w["action_0_bias"]
        z = z - z.max(axis=1, keepdims=True)
        out[rows] = z - np.log(np.exp(z).sum(axis=1, keepdims=True))
        return out

    return targets, A, int(cfg["max_depth"]), logp_of


@pytest.fixture(scope="module", params=sorted(MODELS))
def golden(request):
    return golden_model_case(request.param)


@pytest.mark.parametrize("W", [1, 4])
def test_stop_returns_what_the_plain_search_returns(golden, W):
    targets, A, T, logp_of = golden
    plain = beam_search(targets, W, A, T, logp_of)
    none_trace, stop_trace = {}, {}
    assert beam_search_bounded(targets, W, A, T, logp_of, None, trace=none_trace) == plain  # the bookkeeping of `advance` is beam_search's
    assert (none_trace["bounded"] == 0).all()
    stop = beam_search_bounded(targets, W, A, T, logp_of, "stop", trace=stop_trace)
    assert stop == plain  # winners, list for list
    assert plain[-1] == [] and stop_trace["steps"] <= none_trace["steps"]
    solved = np.array([s is not None for s in plain])
    ended_at = stop_trace["ended_at"]
    fired = solved & (ended_at >= 0)
    # where the bound ended a group, the plain search still held live beams of it after that very step
    for g in np.nonzero(fired)[0]:
        assert none_trace["group_live"][ended_at[g]][g] == stop_trace["bounded"][g] > 0
    print(f"W={W}: solved {solved.sum()} of {len(plain)}, bound fired in {fired.sum()}, steps {none_trace['steps']} -> {stop_trace['steps']}")
    assert solved.sum() >= 30
    if W == 1:  # a group of one slot: its only beam leaves when it is solved, so there is never a beam left to end
        assert not fired.any()
    else:  # the comparison above is not one of searches the bound never touched
        assert 2 * fired.sum() >= solved.sum()
