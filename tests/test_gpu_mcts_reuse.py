"""`BatchedSynthesis.solve(num_mcts_searches=N, reuse_tree=True)` against the CPU model of tests/mctsreuse_model.py, decision by decision,
for all four gyms, deterministic and sampled, on the torch forward and on the policy-layer kernels.

The recording stand-ins are those of tests/test_gpu_mcts_sampled.py plus one on `synthesis.mcts_rebase` (and, for one gym, one on
`VecEnv.copy_envs` that reads the pool the kept nodes' envs were copied into).  The model makes the same search on oracle envs with the
device's own numbers: every selection, every forest array after every backup and every rebase (by bit pattern, on the nodes below
n_nodes), every env_src, every move and draw, the returns by bit pattern, the winners, the solutions and `last_stats` -- "carried" and
"refused" among them -- must be the device's.  After decision 0 there is no root forward pass and no root backup, and no pool is ever
stepped."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")

from mctsmodel import FIELDS, MARKER  # noqa: E402
from mctsreuse_model import ReuseMctsModel, ReuseSampledMctsModel  # noqa: E402
from test_gpu_mcts import CASES, MAX_DEPTH, golden_case  # noqa: E402
from test_gpu_mcts_kernels import bits  # noqa: E402
from test_gpu_sampled_search import oracle_targets  # noqa: E402
from test_gpu_synthesis import replay  # noqa: E402
from test_mctsreuse_model import PINNED, PINNED_STATS  # noqa: E402

NODE_FIELDS = tuple(name for name in FIELDS if name != "n_nodes")


def clifford7_case():
    """CliffordGym on the line of 7 qubits: 71 actions, so the rebase moves its rows in two slices of 64 actions, 8 rows per trip (every
    other case here has fewer than 64: one slice).  No trained policy of that size ships: a seeded random one.  The recorded
    log-probabilities are the model's input, so any policy serves; it finds few answers, so the identity comes twice."""
    import qiskit_gym_amd.envs as envs
    from oracle import OracleEnv
    from qiskit_gym_amd.collector import BasicPolicy
    from util import line_gateset

    n = 7
    gs = line_gateset("clifford", n)
    assert len(gs) == 71
    gym = envs.CliffordGym(n, gs, max_depth=6)
    torch.manual_seed(7)
    policy = BasicPolicy(4 * n * n, len(gs))
    rng = np.random.default_rng(7)
    states = []
    for k in range(5):
        d = 1 + k % 3
        env = OracleEnv("clifford", n, gs, add_inverts=0, add_perms=0, track_solution=0, difficulty=d, max_depth=6)
        env.reset_with(rng.integers(0, len(gs), size=d))
        states.append(env.get_state().tolist())
    solved = OracleEnv("clifford", n, gs, add_inverts=0, add_perms=0).get_state().tolist()
    return gym, policy, states + [solved, solved], None


# (case, S or None: deterministic, N, fast, mcts_nodes)
CALLS = ([(case, None, 4, None, None) for case in CASES] + [(case, 3, 4, None, None) for case in CASES]
         + [("clifford-3q", None, 16, True, None), ("clifford-3q", 2, 16, True, None), ("pinned", None, PINNED["N"], None, PINNED["N"] + 1)])
CASES = dict(CASES, **{"clifford-7q": clifford7_case})
CALLS += [("clifford-7q", None, 16, None, None), ("clifford-7q", 3, 16, None, None)]
STATS = {"mcts", "targets", "steps", "solved", "mean_gates", "nodes", "kernels", "reuse", "capacity", "carried", "refused"}


def call_id(call):
    case, S, N, fast, nodes = call
    return f"{case}-" + (f"S={S}-" if S else "") + f"N={N}" + ("-fast" if fast else "") + (f"-nodes={nodes}" if nodes else "")


def pinned_case():
    assert (PINNED["name"], PINNED["targets"], PINNED["difficulty"], PINNED["max_depth"]) == ("clifford_3q_custom", 11, 12, MAX_DEPTH)
    return golden_case(PINNED["name"], PINNED["seed"])  # the targets of test_mctsreuse_model.trained_targets


def recorded_search(monkeypatch, gym, policy, states, seed, envs_too=False, **kw):
    """`solve(states, reuse_tree=True, **kw)` with the stand-ins in place.  Returns (solutions, last_stats, the calls in order -- ("root" |
    "select" | "backup" | "decide" | "move" | "rebase" | "pool", what the call read and wrote, as numpy copies), what `_winner` saw, the
    synthesis)."""
    from qiskit_gym_amd import synthesis
    from qiskit_gym_amd.vec import VecEnv

    log, steps, kept, last = [], [], {}, {}
    real = dict(select=synthesis.mcts_select, backup=synthesis.mcts_backup, decide=synthesis.mcts_decide, rebase=synthesis.mcts_rebase,
                step=VecEnv.step, copy=VecEnv.copy_envs, winner=synthesis._winner)

    def cpu(t):
        return None if t is None else t.cpu().numpy().copy()

    def snapshot(forest):
        return {name: cpu(getattr(forest, name)) for name in FIELDS}

    def select(forest, C, finished=None, *out):
        res = real["select"](forest, C, finished, *out)
        log.append(("select", dict(C=C, finished=cpu(finished), picked=[cpu(t) for t in res])))
        return res

    def backup(forest, logp, values, reward=None, done=None, src=None, dst=None, act=None, leaf=None, root=False):
        res = real["backup"](forest, logp, values, reward, done, src, dst, act, leaf, root)
        log.append(("root" if root else "backup", dict(logp=cpu(logp), values=cpu(values), reward=cpu(reward), done=cpu(done), forest=snapshot(forest))))
        return res

    def decide(forest, sample=False, seed=0, counter=0, finished=None, move=None, counts=None):
        res = real["decide"](forest, sample, seed, counter, finished, move, counts)
        log.append(("decide", dict(sample=sample, seed=seed, counter=counter, finished=cpu(finished), move=cpu(res))))
        return res

    def rebase(forest, move, finished=None, env_src=None):
        res = real["rebase"](forest, move, finished, env_src)
        last["env_src"] = res
        log.append(("rebase", dict(move=cpu(move), finished=cpu(finished), env_src=cpu(res), forest=snapshot(forest), cap=forest.cap)))
        return res

    def copy_envs(self, src, src_idx, dst_idx=None):
        res = real["copy"](self, src, src_idx, dst_idx)
        if src_idx is last.get("env_src"):
            last["copies"] = last.get("copies", 0) + 1
            last.setdefault("pools", []).append((self, src))
            if envs_too:
                log.append(("pool", dict(state=cpu(self.get_state()), depth=cpu(self.depth), done=cpu(self.done), reward=cpu(self.reward))))
        return res

    def step(self, actions, coins=None):
        steps.append((self, len(log), cpu(actions).astype(np.int64)))
        return real["step"](self, actions, coins)

    def winner(solved, ret):
        kept["ok"], kept["ret"] = cpu(solved), cpu(ret)
        res = real["winner"](solved, ret)
        kept["best"] = cpu(res[1])
        return res

    syn = synthesis.BatchedSynthesis(gym, policy, seed=seed)
    with monkeypatch.context() as m:
        for name, fn in (("mcts_select", select), ("mcts_backup", backup), ("mcts_decide", decide), ("mcts_rebase", rebase), ("_winner", winner)):
            m.setattr(synthesis, name, fn)
        m.setattr(VecEnv, "step", step)
        m.setattr(VecEnv, "copy_envs", copy_envs)
        sols = syn.solve(states, reuse_tree=True, **kw)
    held = syn._held["mcts-sampled-reuse" if kw.get("mcts_sampled") else "mcts-reuse"]
    leaf, pool_a, pool_b, real_envs = held.vecs
    assert all(v is not pool_a and v is not pool_b for v, _, _ in steps)  # the pools are only ever copied into and out of
    assert [p for p, _ in last["pools"]] == [(pool_b, pool_a)[i % 2] for i in range(len(last["pools"]))]  # they take turns
    assert all({p, s} == {pool_a, pool_b} for p, s in last["pools"])
    moves = 0
    for v, at, actions in steps:  # the real envs' moves, each in its place among the tree's calls (`at` counted those alone)
        if v is real_envs:
            log.insert(at + moves, ("move", dict(actions=actions)))
            moves += 1
    return sols, dict(syn.last_stats), log, kept, syn


def expect_trees(got, model, label):
    """The recorded forest against the model's: every tree on its nodes below n_nodes."""
    np.testing.assert_array_equal(got["n_nodes"], model.n_nodes, err_msg=f"{label}: n_nodes")
    for name in NODE_FIELDS:
        want = getattr(model, name)
        assert got[name].dtype == want.dtype and got[name].shape == want.shape, (label, name)
        for m in range(model.M):
            k = int(model.n_nodes[m])
            assert bits(got[name][m, :k]).tobytes() == bits(want[m, :k]).tobytes(), f"{label}: {name} of tree {m}"


@pytest.mark.parametrize("call", CALLS, ids=call_id)
def test_search_against_the_model_decision_by_decision(monkeypatch, call):
    case, S, N, fast, nodes = call
    gym, policy, states, raw = pinned_case() if case == "pinned" else CASES[case]()
    seed, sampled = 1, S is not None
    kw = dict(num_mcts_searches=N, fast=fast, mcts_nodes=nodes)
    kw.update(dict(mcts_sampled=True, num_searches=S) if sampled else dict(deterministic=True))
    envs_too = case == "clifford-3q" and not fast
    sols, stats, log, kept, syn = recorded_search(monkeypatch, gym, policy, states, seed, envs_too, **kw)

    kind, n, gs = gym.env_kind, gym.config["num_qubits"], gym.config["gateset"]
    A, T, M = len(gs), gym.config["max_depth"], len(states)
    B, cap = M * (S or 1), nodes or 2 * N + 1
    assert syn._held["mcts-sampled-reuse" if sampled else "mcts-reuse"].key == (B, B * cap, B * cap, B, False)  # both pools
    assert "mcts" not in syn._held and "mcts-sampled" not in syn._held
    assert set(stats) == STATS | ({"searches", "searches_solved"} if sampled else set())
    assert stats["kernels"] is bool(fast) and stats["mcts"] == N and stats["reuse"] is True and stats["capacity"] == cap
    targets = oracle_targets(gym, states, raw)
    model = ReuseSampledMctsModel(targets, S, N, A, T, seed=seed, cap=cap) if sampled else ReuseMctsModel(targets, N, A, T, cap=cap)
    f = model.forest
    assert f.M == B and f.cap == cap
    events = iter(log)
    expanded = pools = 0
    for t in range(stats["steps"]):
        assert not model.ended, f"the search went on after decision {t}"
        if t == 0:
            kind_, rec = next(events)
            assert kind_ == "root"
            np.testing.assert_array_equal(rec["done"] != 0, model.finished, err_msg="which real envs are final on arrival")
            model.start(rec["forest"]["prior"][:, 0, :], rec["values"])
            expect_trees(rec["forest"], f, "root")
        for s in range(N):
            label = f"decision {t} simulation {s}"
            kind_, rec = next(events)
            assert kind_ == "select", f"{label}: a {kind_} call (no root forward pass and no root backup after decision 0)"
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
            want = np.exp(rec["logp"][grown, :A])
            assert (np.abs(prior[grown].astype(np.float64) - want) <= 4 * np.spacing(want)).all(), label
            reward, done = model.backup(prior, rec["values"])
            np.testing.assert_array_equal(bits(rec["reward"][grown]), bits(reward[grown]), err_msg=f"{label}: the expanded envs' rewards")
            np.testing.assert_array_equal(rec["done"][grown] != 0, done[grown], err_msg=f"{label}: the expanded envs' terminal flags")
            expect_trees(rec["forest"], f, label)
            expanded += int(grown.sum())
        kind_, rec = next(events)  # the decision is `mcts_decide`'s in both searches: the most visited action, or a draw
        assert kind_ == "decide" and rec["sample"] is sampled and (not sampled or (rec["seed"] == seed and rec["counter"] == t))
        np.testing.assert_array_equal(rec["finished"] != 0, model.finished, err_msg=f"decision {t}")
        decided = rec["move"]
        move = model.decide()  # ... and the model's rebase
        np.testing.assert_array_equal(decided, move, err_msg=f"decision {t}: the decision")
        kind_, rec = next(events)
        assert kind_ == "move"
        np.testing.assert_array_equal(rec["actions"], move, err_msg=f"decision {t}: the real envs' moves")
        kind_, rec = next(events)
        assert kind_ == "rebase" and rec["cap"] == cap
        np.testing.assert_array_equal(rec["move"], move, err_msg=f"decision {t}: the move the rebase was given")
        np.testing.assert_array_equal(rec["finished"] != 0, model.finished, err_msg=f"decision {t}: `finished` is the array after the real envs' step")
        np.testing.assert_array_equal(rec["env_src"], model.env_srcs[-1], err_msg=f"decision {t}: env_src")
        expect_trees(rec["forest"], f, f"decision {t}: rebase")
        if envs_too:  # every kept node's env, in the pool it was copied into, is the model's
            kind_, rec = next(events)
            assert kind_ == "pool"
            for m in np.nonzero(~model.finished)[0]:
                for j, env in model.pool[m].items():
                    e = m * cap + j
                    assert (rec["state"][e] == env.get_state()).all() and rec["depth"][e] == env.depth(), (t, m, j)
                    assert bool(rec["done"][e]) == env.is_final() and bits(rec["reward"][e : e + 1])[0] == bits(np.float32([env.reward()]))[0], (t, m, j)
                    pools += 1
    assert model.ended and next(events, None) is None, f"the search stopped after {stats['steps']} decisions, the model goes on"
    want, want_stats = model.result()
    print(f"{call_id(call)}: {stats}; {expanded} nodes expanded, {pools} node envs compared")
    if sampled:
        np.testing.assert_array_equal(bits(kept["ret"].reshape(-1)), bits(model.ret), err_msg="the returns")
        np.testing.assert_array_equal(kept["ok"].reshape(-1), np.array([e.success() for e in model.real]))
        winners = model.winners()
        assert [int(b) if w is not None else None for b, w in zip(kept["best"], winners)] == winners
    assert sols == want
    for key in want_stats:
        assert stats[key] == want_stats[key], key
    assert expanded > 0 and stats["carried"] >= 1.0 and 1.0 < stats["nodes"] <= cap
    if envs_too:
        assert pools > 0
    if case == "pinned":  # the refusal path: carried trees that fill
        assert stats["refused"] > 0
        print(f"pinned on the CPU forward: {PINNED_STATS}; here: refused {stats['refused']}, carried {stats['carried']}")

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
        assert sols[-1] == [] and stats["solved"] >= 2


def test_without_the_keyword_nothing_changes_and_misuse_is_a_value_error(monkeypatch):
    from qiskit_gym_amd import synthesis
    from qiskit_gym_amd.synthesis import BatchedSynthesis

    gym, policy, states, _ = golden_case("clifford_3q_custom", 6)
    syn = BatchedSynthesis(gym, policy, seed=5)
    det, smp = dict(deterministic=True, num_mcts_searches=4), dict(mcts_sampled=True, num_searches=2, num_mcts_searches=4)
    for bad in (dict(reuse_tree=True), dict(reuse_tree=True, deterministic=True), dict(reuse_tree=True, num_mcts_searches=0, deterministic=True),
                dict(det, mcts_nodes=9), dict(smp, mcts_nodes=9), dict(mcts_nodes=9), dict(det, reuse_tree=True, mcts_nodes=4),
                dict(det, reuse_tree=True, mcts_nodes=0), dict(det, reuse_tree=True, mcts_nodes=8193), dict(smp, reuse_tree=True, mcts_nodes=4),
                dict(det, reuse_tree=True, beam_width=2), dict(det, reuse_tree=True, twists=2), dict(det, reuse_tree=True, max_expand_depth=2),
                dict(det, reuse_tree=True, deterministic=False), dict(smp, reuse_tree=True, deterministic=True), dict(det, reuse_tree=True, C=0.0),
                dict(smp, reuse_tree=True, num_searches=2 ** 20)):  # the forest limit counts cap nodes per tree
        with pytest.raises(ValueError):
            syn.solve(states, **bad)
    assert not syn._held  # each refused before any handle was built
    # without the keyword: the launches, the handles and the stats of the search as it was
    calls = []
    real_rebase = synthesis.mcts_rebase
    monkeypatch.setattr(synthesis, "mcts_rebase", lambda *a, **k: calls.append(a) or real_rebase(*a, **k))
    other = BatchedSynthesis(gym, policy, seed=5)
    for kw, kind, keys in ((det, "mcts", {"mcts", "targets", "steps", "solved", "mean_gates", "nodes", "kernels"}),
                           (smp, "mcts-sampled", {"mcts", "searches", "targets", "steps", "solved", "searches_solved", "mean_gates", "nodes", "kernels"})):
        want = other.solve(states, **kw)
        assert syn.solve(states, reuse_tree=False, **kw) == want and syn.last_stats == other.last_stats and set(syn.last_stats) == keys
        assert len(syn._held[kind].vecs) == 3 and syn._held[kind].key == (len(states) * (2 if kind != "mcts" else 1),
                                                                         len(states) * 5 * (2 if kind != "mcts" else 1),
                                                                         len(states) * (2 if kind != "mcts" else 1), False)
    assert not calls and set(syn._held) == {"mcts", "mcts-sampled"}
    # with it, beside them; the default capacity, one given, and the same answer from the same seed on the same handles
    first = syn.solve(states, reuse_tree=True, **det)
    assert calls and syn.last_stats["capacity"] == 9 and syn._held["mcts-reuse"].key == (len(states), len(states) * 9, len(states) * 9, len(states), False)
    vecs = syn._held["mcts-reuse"].vecs
    assert syn.solve(states, reuse_tree=True, **det) == first and syn._held["mcts-reuse"].vecs is vecs and first[-1] == []
    syn.solve(states, reuse_tree=True, mcts_nodes=17, **smp)
    assert syn.last_stats["capacity"] == 17 and len(syn._held["mcts-sampled-reuse"].vecs) == 4
    assert syn.solve(states, **det) == other.solve(states, **det)  # side by side with the new handles
    kind, cfg, gs = gym.env_kind, dict(num_qubits=3, depth_slope=gym.config["depth_slope"], max_depth=MAX_DEPTH), gym.config["gateset"]
    for state, sol in zip(states, first):
        if sol is not None:
            assert replay(kind, cfg, gs, state, sol).success()
    lf_gym, lf_policy, lf_states, _ = golden_case("lf_5_line", 3)
    with pytest.raises(ValueError):  # the policy-layer kernels do not read this env's layout: an error, not the torch forward
        BatchedSynthesis(lf_gym, lf_policy).solve(lf_states, fast=True, reuse_tree=True, **det)
