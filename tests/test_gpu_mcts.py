"""`BatchedSynthesis.solve(num_mcts_searches=N, deterministic=True)` against the CPU model of tests/mctsmodel.py, simulation by simulation, for
all four gyms, on the torch forward and on the policy-layer kernels.

The model is driven with the device's own numbers, by the recorder and the replay of tests/mctsrecord.py: stand-ins on
`synthesis.mcts_select` and `synthesis.mcts_backup` call the real function and keep every call's inputs and outputs (the rows of log-probabilities and the values the search handed over, the rewards and
terminal flags of the expanded envs, the selection's four outputs, the whole forest after the call), a stand-in on `VecEnv.step` the
actions every handle was given.  The model then makes the same search on oracle envs: every selection, every forest array after every
backup (by bit pattern; `prior` is taken from the device, so expf is no source of divergence), the reward and the terminal flag of every
expanded env and every decision must be the device's, and at the end the solutions and `last_stats`."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")

from mctsmodel import MARKER  # noqa: E402
from mctsrecord import model_for, record, replay, solutions_solve  # noqa: E402
from oracle import OracleEnv  # noqa: E402
from test_gpu_beam import pauli_case  # noqa: E402
from test_gpu_sampled_search import oracle_targets  # noqa: E402
from test_gpu_synthesis import GYMS, targets  # noqa: E402
from test_gpu_synthesis import replay as replay_gates  # noqa: E402
from test_reference_policies import MODELS, load  # noqa: E402

MAX_DEPTH = 32  # decisions at most: the policies are trained and the targets 12 gates from solved, so few are needed


def golden_case(name, seed):
    """11 targets at difficulty 12 and the identity, for one of the reference's trained policies."""
    import qiskit_gym_amd.envs as envs
    from qiskit_gym_amd.synthesis import policy_from_reference_state_dict

    cfg, gateset, w = load(name)
    kind = MODELS[name]
    cfg = dict(cfg, max_depth=MAX_DEPTH)
    gym = getattr(envs, GYMS[kind])(cfg["num_qubits"], gateset, depth_slope=cfg["depth_slope"], max_depth=MAX_DEPTH)
    states = targets(kind, cfg, gateset, 11, 12, seed)
    states.append(OracleEnv(kind, cfg["num_qubits"], gateset, add_inverts=0, add_perms=0).get_state().tolist())  # solved on arrival
    return gym, policy_from_reference_state_dict(w), states, None


CASES = {
    "clifford-3q": lambda: golden_case("clifford_3q_custom", 1),
    "linear-function-5q": lambda: golden_case("lf_5_line", 3),
    "permutation-9q": lambda: golden_case("perm_square_3x3", 4),
    "pauli-3q": pauli_case,
}

CALLS = [(case, N, None) for case in CASES for N in (4, 16)] + [("clifford-3q", 4, True), ("pauli-3q", 16, True)]
# The PauliGym policy is untrained: 4 or 16 simulations find none of the two-gate answers, and no answer means no rotation marker to read from
# the real env's log.  64 do: the model alone, on a CPU forward of the same policy, solves 6 of the 12 targets, every answer with a marker.
CALLS.append(("pauli-3q", 64, None))


def call_id(call):
    case, N, fast = call
    return f"{case}-N={N}" + ("-fast" if fast else "")


@pytest.mark.parametrize("call", CALLS, ids=call_id)
def test_search_against_the_model_simulation_by_simulation(monkeypatch, call):
    from qiskit_gym_amd.synthesis import BatchedSynthesis

    case, N, fast = call
    gym, policy, states, raw = CASES[case]()
    got = record(monkeypatch, BatchedSynthesis(gym, policy, seed=1), lambda syn: syn.solve(states, deterministic=True, num_mcts_searches=N, fast=fast))
    sols, stats = got.out, got.stats

    kind, n, gs = gym.env_kind, gym.config["num_qubits"], gym.config["gateset"]
    A, T, M = len(gs), gym.config["max_depth"], len(states)
    assert got.kind == "mcts" and got.held.key == (M, M * (N + 1), M, False) and len(got.held.vecs) == 3
    assert stats["kernels"] is bool(fast) and stats["mcts"] == N and stats["targets"] == M
    assert set(stats) == {"mcts", "targets", "steps", "solved", "mean_gates", "nodes", "kernels"}
    model = model_for(oracle_targets(gym, states, raw), S=None, N=N, A=A, T=T)
    seen = replay(got.log, model)
    want, want_stats = model.result()
    print(f"{call_id(call)}: {stats}; {seen.expanded} nodes expanded")
    assert sols == want
    for key in ("steps", "solved", "mean_gates", "nodes"):
        assert stats[key] == want_stats[key], key
    assert seen.expanded > 0 and 1.0 < stats["nodes"] <= N + 1

    solutions_solve(sols, oracle_targets(gym, states, raw))
    if case == "pauli-3q" and N == 64:
        assert any(any(a >= MARKER for a in s) for s in sols if s is not None)  # an answer's log carries the rotation it released
    if raw is None:
        cfg = dict(num_qubits=n, depth_slope=gym.config["depth_slope"], max_depth=T)
        assert all(replay_gates(kind, cfg, gs, state, sol).success() for state, sol in zip(states, sols) if sol is not None)
        assert sols[-1] == []  # the identity: solved on arrival
        assert stats["solved"] >= 2  # the trained policies solve targets this near: nothing is compared empty


def test_arguments_that_do_not_exist_are_value_errors_and_zero_is_no_tree_search():
    from qiskit_gym_amd.synthesis import BatchedSynthesis

    gym, policy, states, _ = golden_case("clifford_3q_custom", 6)
    syn = BatchedSynthesis(gym, policy, seed=5)
    plain = syn.solve(states, deterministic=True)
    plain_stats = dict(syn.last_stats)
    assert syn.solve(states, deterministic=True, num_mcts_searches=0, C=-1.0, max_expand_depth=3) == plain and syn.last_stats == plain_stats
    sampled = syn.solve(states, num_searches=8)
    assert syn.solve(states, num_searches=8, num_mcts_searches=0) == sampled
    assert "mcts" not in syn._held
    mcts = dict(deterministic=True, num_mcts_searches=4)
    for bad in (dict(mcts, num_mcts_searches=-1), dict(mcts, C=0.0), dict(mcts, C=-1.0), dict(mcts, max_expand_depth=2), dict(mcts, max_expand_depth=0),
                dict(mcts, deterministic=False), dict(num_mcts_searches=4), dict(mcts, beam_width=2), dict(mcts, beam_width=2, merge_duplicates=True),
                dict(mcts, merge_duplicates=True), dict(mcts, bound="stop"), dict(mcts, beam_width=2, bound="stop"), dict(mcts, twists=2),
                dict(mcts, twists=2, twist_kernels=True), dict(mcts, twist_kernels=True), dict(mcts, num_mcts_searches=2 ** 24)):
        with pytest.raises(ValueError):
            syn.solve(states, **bad)
    assert "mcts" not in syn._held  # refused before any handle was built
    sols = syn.solve(states, **mcts)
    assert syn.last_stats["mcts"] == 4 and sols[-1] == [] and syn.solve(states, **mcts) == sols  # no randomness; the handles are reused
    kind, cfg, gs = gym.env_kind, dict(num_qubits=3, depth_slope=gym.config["depth_slope"], max_depth=MAX_DEPTH), gym.config["gateset"]
    for state, sol in zip(states, sols):
        if sol is not None:
            assert replay_gates(kind, cfg, gs, state, sol).success()
    lf_gym, lf_policy, lf_states, _ = golden_case("lf_5_line", 3)
    with pytest.raises(ValueError):  # the policy-layer kernels do not read this env's layout: an error, not the torch forward
        BatchedSynthesis(lf_gym, lf_policy).solve(lf_states, fast=True, **mcts)
