"""`BatchedSynthesis.solve(num_searches=S, num_mcts_searches=N, mcts_sampled=True)` against the CPU model of tests/mctssample_model.py,
decision by decision, for all four gyms, on the torch forward and on the policy-layer kernels.

As in tests/test_gpu_mcts.py the model is driven with the device's own numbers, by the recorder and the replay of tests/mctsrecord.py:
stand-ins on `synthesis.mcts_select`, `synthesis.mcts_backup` and `synthesis.mcts_decide` call the real function and keep what it read and
wrote, a stand-in on `VecEnv.step` the actions every handle was given.  The model then makes the same search on oracle envs: every selection, every forest array after every backup (by bit pattern), every
draw, every real move, the returns by bit pattern, the winners, the solutions and `last_stats` must be the device's."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")

from mctsrecord import Draws, model_for, record, replay, solutions_solve  # noqa: E402
from test_gpu_mcts import CASES, MAX_DEPTH, golden_case  # noqa: E402
from test_gpu_sampled_search import oracle_targets  # noqa: E402
from test_gpu_synthesis import replay as replay_gates  # noqa: E402
from util import bits  # noqa: E402

CALLS = [(case, 3, 4, None) for case in CASES] + [("clifford-3q", 2, 16, True)]
STATS = {"mcts", "searches", "targets", "steps", "solved", "searches_solved", "mean_gates", "nodes", "kernels"}


def call_id(call):
    case, S, N, fast = call
    return f"{case}-S={S}-N={N}" + ("-fast" if fast else "")


@pytest.mark.parametrize("call", CALLS, ids=call_id)
def test_search_against_the_model_decision_by_decision(monkeypatch, call):
    from qiskit_gym_amd.synthesis import BatchedSynthesis

    case, S, N, fast = call
    gym, policy, states, raw = CASES[case]()
    seed = 1
    syn = BatchedSynthesis(gym, policy, seed=seed)
    got = record(monkeypatch, syn, lambda syn: syn.solve(states, mcts_sampled=True, num_searches=S, num_mcts_searches=N, fast=fast))
    sols, stats, kept = got.out, got.stats, got.kept

    kind, n, gs = gym.env_kind, gym.config["num_qubits"], gym.config["gateset"]
    A, T, M = len(gs), gym.config["max_depth"], len(states)
    B = M * S
    assert set(syn._held) == {got.kind} == {"mcts-sampled"} and got.held.key == (B, B * (N + 1), B, False)
    assert stats["kernels"] is bool(fast) and stats["mcts"] == N and set(stats) == STATS
    model = model_for(oracle_targets(gym, states, raw), S=S, N=N, A=A, T=T, seed=seed)
    assert model.forest.M == B
    draws = Draws()
    seen = replay(got.log, model, seed=seed, on_decide=draws)
    want, want_stats = model.result()
    print(f"{call_id(call)}: {stats}; {seen.expanded} nodes expanded, {draws.off_top} draws off the most visited action")
    np.testing.assert_array_equal(bits(kept["ret"].reshape(-1)), bits(model.ret), err_msg="the returns")
    np.testing.assert_array_equal(kept["ok"].reshape(-1), np.array([e.success() for e in model.real]))
    winners = model.winners()
    assert [int(b) if w is not None else None for b, w in zip(kept["best"], winners)] == winners
    assert sols == want
    for key in want_stats:
        assert stats[key] == want_stats[key], key
    assert seen.expanded > 0 and 1.0 < stats["nodes"] <= N + 1 and draws.off_top > 0

    solutions_solve(sols, oracle_targets(gym, states, raw))
    if raw is None:
        cfg = dict(num_qubits=n, depth_slope=gym.config["depth_slope"], max_depth=T)
        assert all(replay_gates(kind, cfg, gs, state, sol).success() for state, sol in zip(states, sols) if sol is not None)
        assert sols[-1] == []  # the identity: solved on arrival, in every one of its searches
        assert stats["solved"] >= 2 and kept["ok"][-1].all()


def test_seeds_handles_and_zero_searches():
    from qiskit_gym_amd.synthesis import BatchedSynthesis

    gym, policy, states, _ = golden_case("clifford_3q_custom", 6)
    kw = dict(num_mcts_searches=4, mcts_sampled=True)
    syn = BatchedSynthesis(gym, policy, seed=5)
    first = syn.solve(states, num_searches=3, **kw)
    stats = dict(syn.last_stats)
    vecs = syn._held["mcts-sampled"].vecs
    assert syn.solve(states, num_searches=3, **kw) == first and syn.last_stats == stats  # the same seed repeats the draws ...
    assert syn._held["mcts-sampled"].vecs is vecs  # ... on the same handles
    assert stats["searches"] == 3 and stats["targets"] == len(states) and first[-1] == []
    kind, cfg, gs = gym.env_kind, dict(num_qubits=3, depth_slope=gym.config["depth_slope"], max_depth=MAX_DEPTH), gym.config["gateset"]
    for state, sol in zip(states, first):
        if sol is not None:
            assert replay_gates(kind, cfg, gs, state, sol).success()
    # num_searches=0 is one search per target, what num_searches=1 is
    one = syn.solve(states, num_searches=1, **kw)
    one_stats = dict(syn.last_stats)
    assert syn._held["mcts-sampled"].key == (len(states), len(states) * 5, len(states), False)
    assert syn.solve(states, num_searches=0, **kw) == one and syn.last_stats == one_stats and one_stats["searches"] == 1


def test_the_seed_changes_the_draws(monkeypatch):
    from qiskit_gym_amd.synthesis import BatchedSynthesis

    gym, policy, states, _ = golden_case("clifford_3q_custom", 6)
    draws = {}
    for seed in (5, 5, 6):
        log = record(monkeypatch, BatchedSynthesis(gym, policy, seed=seed),
                     lambda syn: syn.solve(states, mcts_sampled=True, num_searches=2, num_mcts_searches=8)).log
        got = [rec["move"] for kind_, rec in log if kind_ == "decide"]
        if seed in draws:
            assert len(got) == len(draws[seed]) and all((a == b).all() for a, b in zip(got, draws[seed]))
        draws[seed] = got
    assert (draws[5][0] != draws[6][0]).any()  # the first decision's trees are the same under both seeds: the draws are not


def test_without_the_keyword_nothing_changes_and_misuse_is_a_value_error():
    from qiskit_gym_amd.synthesis import BatchedSynthesis

    gym, policy, states, _ = golden_case("clifford_3q_custom", 6)
    syn, other = BatchedSynthesis(gym, policy, seed=5), BatchedSynthesis(gym, policy, seed=5)
    mcts = dict(num_mcts_searches=4)
    for bad in (dict(mcts_sampled=True), dict(mcts_sampled=True, num_mcts_searches=0), dict(mcts, mcts_sampled=True, deterministic=True),
                dict(mcts, mcts_sampled=True, beam_width=2), dict(mcts, mcts_sampled=True, beam_width=2, merge_duplicates=True),
                dict(mcts, mcts_sampled=True, merge_duplicates=True), dict(mcts, mcts_sampled=True, bound="stop"),
                dict(mcts, mcts_sampled=True, beam_width=2, bound="prune"), dict(mcts, mcts_sampled=True, twists=2),
                dict(mcts, mcts_sampled=True, twists=2, twist_kernels=True), dict(mcts, mcts_sampled=True, twist_kernels=True),
                dict(mcts, mcts_sampled=True, C=0.0), dict(mcts, mcts_sampled=True, max_expand_depth=2),
                dict(mcts, mcts_sampled=True, num_searches=2 ** 20),  # the forest limit counts targets * searches trees
                dict(mcts)):  # without the keyword a tree search with deterministic=False stays refused
        with pytest.raises(ValueError):
            syn.solve(states, **bad)
    assert not syn._held  # each refused before any handle was built
    # with `mcts_sampled` left out (or False) the deterministic tree search and the policy-sampled search answer as ever
    for kw in (dict(deterministic=True, num_mcts_searches=4), dict(num_searches=8), dict(deterministic=True)):
        want = other.solve(states, **kw)
        want_stats = dict(other.last_stats)
        assert syn.solve(states, mcts_sampled=False, **kw) == want and syn.last_stats == want_stats
        assert syn.solve(states, **kw) == want and syn.last_stats == want_stats
    assert "mcts-sampled" not in syn._held and syn._held["mcts"].key == (len(states), len(states) * 5, len(states), False)
    sols = syn.solve(states, num_searches=2, mcts_sampled=True, **mcts)
    assert "mcts-sampled" in syn._held and sols[-1] == []
    assert syn.solve(states, deterministic=True, **mcts) == other.solve(states, deterministic=True, **mcts)  # side by side with the new handles
    lf_gym, lf_policy, lf_states, _ = golden_case("lf_5_line", 3)
    with pytest.raises(ValueError):  # the policy-layer kernels do not read this env's layout: an error, not the torch forward
        BatchedSynthesis(lf_gym, lf_policy).solve(lf_states, fast=True, num_searches=2, mcts_sampled=True, **mcts)
