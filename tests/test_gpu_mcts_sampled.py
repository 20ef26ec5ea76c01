"""`BatchedSynthesis.solve(num_searches=S, num_mcts_searches=N, mcts_sampled=True)` against the CPU model of tests/mctssample_model.py,
decision by decision, for all four gyms, on the torch forward and on the policy-layer kernels.

As in tests/test_gpu_mcts.py the model is driven with the device's own numbers: stand-ins on `synthesis.mcts_select`, `synthesis.mcts_backup`
and `synthesis.mcts_decide` call the real function and keep what it read and wrote, a stand-in on `VecEnv.step` the actions every handle was
given.  The model then makes the same search on oracle envs: every selection, every forest array after every backup (by bit pattern), every
draw, every real move, the returns by bit pattern, the winners, the solutions and `last_stats` must be the device's."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")

from mctsmodel import FIELDS, MARKER  # noqa: E402
from mctssample_model import SampledMctsModel, counts  # noqa: E402
from test_gpu_mcts import CASES, MAX_DEPTH, expect_forest, golden_case  # noqa: E402
from test_gpu_mcts_kernels import bits  # noqa: E402
from test_gpu_sampled_search import oracle_targets  # noqa: E402
from test_gpu_synthesis import replay  # noqa: E402

CALLS = [(case, 3, 4, None) for case in CASES] + [("clifford-3q", 2, 16, True)]
STATS = {"mcts", "searches", "targets", "steps", "solved", "searches_solved", "mean_gates", "nodes", "kernels"}


def call_id(call):
    case, S, N, fast = call
    return f"{case}-S={S}-N={N}" + ("-fast" if fast else "")


def recorded_search(monkeypatch, gym, policy, states, seed, **kw):
    """`solve(states, mcts_sampled=True, **kw)` with the stand-ins in place.  Returns (solutions, last_stats, the calls in order -- ("root" |
    "select" | "backup" | "decide" | "move", what the call read and wrote, as numpy copies), the returns the search kept, the synthesis)."""
    from qiskit_gym_amd import synthesis
    from qiskit_gym_amd.vec import VecEnv

    log, steps, kept = [], [], {}
    real_select, real_backup, real_decide, real_step, real_winner = (synthesis.mcts_select, synthesis.mcts_backup, synthesis.mcts_decide, VecEnv.step,
                                                                     synthesis._winner)

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
        before = snapshot(forest)
        res = real_decide(forest, sample, seed, counter, finished, move, counts)
        log.append(("decide", dict(sample=sample, seed=seed, counter=counter, finished=cpu(finished), move=cpu(res), before=before, forest=snapshot(forest))))
        return res

    def step(self, actions, coins=None):
        steps.append((self, len(log), cpu(actions).astype(np.int64)))
        return real_step(self, actions, coins)

    def winner(solved, ret):
        kept["ok"], kept["ret"] = cpu(solved), cpu(ret)
        res = real_winner(solved, ret)
        kept["best"] = cpu(res[1])
        return res

    syn = synthesis.BatchedSynthesis(gym, policy, seed=seed)
    with monkeypatch.context() as m:
        m.setattr(synthesis, "mcts_select", select)
        m.setattr(synthesis, "mcts_backup", backup)
        m.setattr(synthesis, "mcts_decide", decide)
        m.setattr(synthesis, "_winner", winner)
        m.setattr(VecEnv, "step", step)
        sols = syn.solve(states, mcts_sampled=True, **kw)
    held = syn._held["mcts-sampled"]
    leaf, pool, real = held.vecs
    assert all(v is not pool for v, _, _ in steps)  # the pool is only ever copied into and out of
    moves = 0
    for v, at, actions in steps:  # the real envs' moves, each in its place among the tree's calls (`at` counted those alone)
        if v is real:
            log.insert(at + moves, ("move", dict(actions=actions)))
            moves += 1
    return sols, dict(syn.last_stats), log, kept, syn


@pytest.mark.parametrize("call", CALLS, ids=call_id)
def test_search_against_the_model_decision_by_decision(monkeypatch, call):
    case, S, N, fast = call
    gym, policy, states, raw = CASES[case]()
    seed = 1
    sols, stats, log, kept, syn = recorded_search(monkeypatch, gym, policy, states, seed, num_searches=S, num_mcts_searches=N, fast=fast)

    kind, n, gs = gym.env_kind, gym.config["num_qubits"], gym.config["gateset"]
    A, T, M = len(gs), gym.config["max_depth"], len(states)
    B = M * S
    assert syn._held["mcts-sampled"].key == (B, B * (N + 1), B, False) and "mcts" not in syn._held
    assert stats["kernels"] is bool(fast) and stats["mcts"] == N and set(stats) == STATS
    model = SampledMctsModel(oracle_targets(gym, states, raw), S, N, A, T, seed=seed)
    f = model.forest
    assert f.M == B
    events = iter(log)
    expanded = off_top = 0
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
            model.expand()
            kind_, rec = next(events)
            assert kind_ == "backup"
            grown = act < A
            prior = np.zeros((B, A), dtype=np.float32)
            for m in np.nonzero(grown)[0]:
                prior[m] = rec["forest"]["prior"][m, leaf[m]]
            reward, done = model.backup(prior, rec["values"])
            np.testing.assert_array_equal(bits(rec["reward"][grown]), bits(reward[grown]), err_msg=f"{label}: the expanded envs' rewards")
            np.testing.assert_array_equal(rec["done"][grown] != 0, done[grown], err_msg=f"{label}: the expanded envs' terminal flags")
            expect_forest(rec["forest"], f, label)
            expanded += int(grown.sum())
        kind_, rec = next(events)
        assert kind_ == "decide" and rec["sample"] is True and rec["seed"] == seed and rec["counter"] == t
        np.testing.assert_array_equal(rec["finished"] != 0, model.finished, err_msg=f"decision {t}")
        for name in FIELDS:  # the decision wrote nothing into the forest
            assert bits(rec["before"][name]).tobytes() == bits(rec["forest"][name]).tobytes(), (t, name)
        live = ~model.finished
        n_a = counts(f)
        draw = model.decide()
        np.testing.assert_array_equal(rec["move"], draw, err_msg=f"decision {t}: the draws")
        assert (draw[live] < A).all() and (n_a[np.arange(B), np.minimum(draw, A - 1)][live] > 0).all() and (draw[~live] == A).all()
        off_top += int((n_a[np.arange(B), np.minimum(draw, A - 1)] < n_a.max(axis=1))[live].sum())
        kind_, rec = next(events)
        assert kind_ == "move"
        np.testing.assert_array_equal(rec["actions"], draw, err_msg=f"decision {t}: the real envs' moves")
    assert model.ended and next(events, None) is None, f"the search stopped after {stats['steps']} decisions, the model goes on"
    want, want_stats = model.result()
    print(f"{call_id(call)}: {stats}; {expanded} nodes expanded, {off_top} draws off the most visited action")
    np.testing.assert_array_equal(bits(kept["ret"].reshape(-1)), bits(model.ret), err_msg="the returns")
    np.testing.assert_array_equal(kept["ok"].reshape(-1), np.array([e.success() for e in model.real]))
    winners = model.winners()
    assert [int(b) if w is not None else None for b, w in zip(kept["best"], winners)] == winners
    assert sols == want
    for key in want_stats:
        assert stats[key] == want_stats[key], key
    assert expanded > 0 and 1.0 < stats["nodes"] <= N + 1 and off_top > 0

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
    if raw is None:
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
            assert replay(kind, cfg, gs, state, sol).success()
    # num_searches=0 is one search per target, what num_searches=1 is
    one = syn.solve(states, num_searches=1, **kw)
    one_stats = dict(syn.last_stats)
    assert syn._held["mcts-sampled"].key == (len(states), len(states) * 5, len(states), False)
    assert syn.solve(states, num_searches=0, **kw) == one and syn.last_stats == one_stats and one_stats["searches"] == 1


def test_the_seed_changes_the_draws(monkeypatch):
    gym, policy, states, _ = golden_case("clifford_3q_custom", 6)
    draws = {}
    for seed in (5, 5, 6):
        _, _, log, _, _ = recorded_search(monkeypatch, gym, policy, states, seed, num_searches=2, num_mcts_searches=8)
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
