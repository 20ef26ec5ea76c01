"""`BatchedSynthesis.solve(num_mcts_searches=N, deterministic=True)` against the CPU model of tests/mctsmodel.py, simulation by simulation, for
all four gyms, on the torch forward and on the policy-layer kernels.

The model is driven with the device's own numbers: stand-ins on `synthesis.mcts_select` and `synthesis.mcts_backup` call the real
function and keep every call's inputs and outputs (the rows of log-probabilities and the values the search handed over, the rewards and
terminal flags of the expanded envs, the selection's four outputs, the whole forest after the call), a stand-in on `VecEnv.step` the
actions every handle was given.  The model then makes the same search on oracle envs: every selection, every forest array after every
backup (by bit pattern; `prior` is taken from the device, so expf is no source of divergence), the reward and the terminal flag of every
expanded env and every decision must be the device's, and at the end the solutions and `last_stats`."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")

from mctsmodel import FIELDS, MARKER, MctsModel  # noqa: E402
from oracle import OracleEnv  # noqa: E402
from test_gpu_beam import pauli_case  # noqa: E402
from test_gpu_mcts_kernels import bits  # noqa: E402
from test_gpu_sampled_search import oracle_targets  # noqa: E402
from test_gpu_synthesis import GYMS, replay, targets  # noqa: E402
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


def recorded_search(monkeypatch, gym, policy, states, N, fast):
    """`solve` with the stand-ins in place.  Returns (solutions, last_stats, the calls in order -- ("root" | "select" | "backup" | "decide" |
    "move", what the call read and wrote, as numpy copies))."""
    from qiskit_gym_amd import synthesis
    from qiskit_gym_amd.vec import VecEnv

    log, steps = [], []
    real_select, real_backup, real_decide, real_step = synthesis.mcts_select, synthesis.mcts_backup, synthesis.mcts_decide, VecEnv.step

    def cpu(t):
        return None if t is None else t.cpu().numpy().copy()

    def snapshot(forest):
        return {name: cpu(getattr(forest, name)) for name in FIELDS}

    def select(forest, C, finished=None, *out):
        res = real_select(forest, C, finished, *out)
        log.append(("select", dict(C=C, finished=cpu(finished), picked=[cpu(t) for t in res])))
        return res

    def backup(forest, logp, values, reward=None, done=None, src=None, dst=None, act=None, leaf=None, root=False):
        res = real_backup(forest, logp, values, reward, done, src, dst, act, leaf, root)
        log.append(("root" if root else "backup", dict(logp=cpu(logp), values=cpu(values), reward=cpu(reward), done=cpu(done),
                                                       picked=[cpu(t) for t in (src, dst, act, leaf)], forest=snapshot(forest))))
        return res

    def decide(forest, sample=False, seed=0, counter=0, finished=None, move=None, counts=None):
        res = real_decide(forest, sample, seed, counter, finished, move, counts)
        log.append(("decide", dict(sample=sample, finished=cpu(finished), move=cpu(res))))
        return res

    def step(self, actions, coins=None):
        steps.append((self, len(log), cpu(actions).astype(np.int64)))
        return real_step(self, actions, coins)

    syn = synthesis.BatchedSynthesis(gym, policy, seed=1)
    with monkeypatch.context() as m:
        m.setattr(synthesis, "mcts_select", select)
        m.setattr(synthesis, "mcts_backup", backup)
        m.setattr(synthesis, "mcts_decide", decide)
        m.setattr(VecEnv, "step", step)
        sols = syn.solve(states, deterministic=True, num_mcts_searches=N, fast=fast)
    held = syn._held["mcts"]
    assert held.key == (len(states), len(states) * (N + 1), len(states), False) and len(held.vecs) == 3
    leaf, pool, real = held.vecs
    assert all(v is not pool for v, _, _ in steps)  # the pool is only ever copied into and out of
    moves = 0
    for v, at, actions in steps:  # the real envs' moves, each in its place among the tree's calls (`at` counted those alone)
        if v is real:
            log.insert(at + moves, ("move", dict(actions=actions)))
            moves += 1
    return sols, dict(syn.last_stats), log


def expect_forest(got, model, label):
    for name in FIELDS:
        want = getattr(model, name)
        assert got[name].dtype == want.dtype and got[name].shape == want.shape, (label, name)
        np.testing.assert_array_equal(bits(got[name]), bits(want), err_msg=f"{label}: {name}")


@pytest.mark.parametrize("call", CALLS, ids=call_id)
def test_search_against_the_model_simulation_by_simulation(monkeypatch, call):
    case, N, fast = call
    gym, policy, states, raw = CASES[case]()
    sols, stats, log = recorded_search(monkeypatch, gym, policy, states, N, fast)

    kind, n, gs = gym.env_kind, gym.config["num_qubits"], gym.config["gateset"]
    A, T, M = len(gs), gym.config["max_depth"], len(states)
    assert stats["kernels"] is bool(fast) and stats["mcts"] == N and stats["targets"] == M
    assert set(stats) == {"mcts", "targets", "steps", "solved", "mean_gates", "nodes", "kernels"}
    model = MctsModel(oracle_targets(gym, states, raw), N, A, T)
    f = model.forest
    events = iter(log)
    expanded = 0
    for t in range(stats["steps"]):
        assert not model.ended, f"the search went on after decision {t}"
        kind_, rec = next(events)
        assert kind_ == "root"
        np.testing.assert_array_equal(rec["done"] != 0, model.finished, err_msg=f"decision {t}: which real envs are final")
        prior = rec["forest"]["prior"][:, 0, :]
        want = np.exp(rec["logp"][:, :A])
        assert (np.abs(prior.astype(np.float64) - want) <= 4 * np.spacing(want)).all()
        model.start(prior, rec["values"])
        expect_forest(rec["forest"], f, f"decision {t}: root")
        for s in range(N):
            label = f"decision {t} simulation {s}"
            kind_, rec = next(events)
            assert kind_ == "select" and rec["C"] == 2 ** 0.5
            np.testing.assert_array_equal(rec["finished"] != 0, model.finished, err_msg=label)
            src, dst, act, leaf = model.select()
            for name, g, w in zip(("src", "dst", "act", "leaf"), rec["picked"], (src, dst, act, leaf)):
                np.testing.assert_array_equal(g, w, err_msg=f"{label}: {name}")
            fresh = model.expand()
            kind_, rec = next(events)
            assert kind_ == "backup"
            for g, w in zip(rec["picked"], (src, dst, act, leaf)):
                np.testing.assert_array_equal(g, w, err_msg=label)
            grown = act < A
            prior = np.zeros((M, A), dtype=np.float32)
            for m in np.nonzero(grown)[0]:
                prior[m] = rec["forest"]["prior"][m, leaf[m]]
            want = np.exp(rec["logp"][grown, :A])
            assert (np.abs(prior[grown].astype(np.float64) - want) <= 4 * np.spacing(want)).all(), label
            reward, done = model.backup(prior, rec["values"])
            np.testing.assert_array_equal(bits(rec["reward"][grown]), bits(reward[grown]), err_msg=f"{label}: the expanded envs' rewards")
            np.testing.assert_array_equal(rec["done"][grown] != 0, done[grown], err_msg=f"{label}: the expanded envs' terminal flags")
            expect_forest(rec["forest"], f, label)
            expanded += int(grown.sum())
        kind_, rec = next(events)  # one decision, on its kernel, between the last backup and the move
        assert kind_ == "decide" and rec["sample"] is False
        np.testing.assert_array_equal(rec["finished"] != 0, model.finished, err_msg=f"decision {t}")
        move = model.decide()
        np.testing.assert_array_equal(rec["move"], move, err_msg=f"decision {t}: the decision")
        kind_, rec = next(events)
        assert kind_ == "move"
        np.testing.assert_array_equal(rec["actions"], move, err_msg=f"decision {t}")
    assert model.ended and next(events, None) is None, f"the search stopped after {stats['steps']} decisions, the model goes on"
    want, want_stats = model.result()
    print(f"{call_id(call)}: {stats}; {expanded} nodes expanded")
    assert sols == want
    for key in ("steps", "solved", "mean_gates", "nodes"):
        assert stats[key] == want_stats[key], key
    assert expanded > 0 and 1.0 < stats["nodes"] <= N + 1

    okw_targets = oracle_targets(gym, states, raw)
    for m, sol in enumerate(sols):  # every solution, replayed on the oracle from its target, solves it with exactly those entries
        if sol is None:
            continue
        env = okw_targets[m]
        for a in sol:
            if a < MARKER:
                assert not env.success()
                env.step(int(a))
        assert env.success() and env.solution() == sol
        if raw is None:
            cfg = dict(num_qubits=n, depth_slope=gym.config["depth_slope"], max_depth=T)
            assert replay(kind, cfg, gs, states[m], sol).success()
    if case == "pauli-3q" and N == 64:
        assert any(any(a >= MARKER for a in s) for s in sols if s is not None)  # an answer's log carries the rotation it released
    if raw is None:
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
            assert replay(kind, cfg, gs, state, sol).success()
    lf_gym, lf_policy, lf_states, _ = golden_case("lf_5_line", 3)
    with pytest.raises(ValueError):  # the policy-layer kernels do not read this env's layout: an error, not the torch forward
        BatchedSynthesis(lf_gym, lf_policy).solve(lf_states, fast=True, **mcts)
