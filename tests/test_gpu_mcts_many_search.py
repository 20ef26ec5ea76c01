"""`BatchedSynthesis.solve(num_mcts_searches=N, mcts_leaves=K)` against the CPU models of tests/mctsmany_model.py, round by round and
decision by decision, for all four gyms: deterministic, sampled, with carried trees (at the default capacity and at N + 1 nodes, where the
trees fill in the middle of a round), on the torch forward and on the policy-layer kernels.

Recorded the way tests/test_gpu_mcts.py and tests/test_gpu_mcts_reuse.py record: stand-ins on the tree calls of `synthesis` run the real
function and keep what it read and wrote, the model makes the same search on oracle envs with the device's own log-probabilities and values,
and every selection, every forest array after every backup and every rebase (by bit pattern, on the nodes below n_nodes), every move, the
solutions and `last_stats` -- "rounds", "leaves" and "idle" among them -- must be the device's."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")

from mctsmany_model import ManyMctsModel, ManyReuseMctsModel, ManyReuseSampledMctsModel, ManySampledMctsModel  # noqa: E402
from mctsmodel import FIELDS, MARKER  # noqa: E402
from test_gpu_mcts import CASES, golden_case  # noqa: E402
from test_gpu_mcts_kernels import bits  # noqa: E402
from test_gpu_mcts_reuse import expect_trees  # noqa: E402
from test_gpu_sampled_search import oracle_targets  # noqa: E402

N, K = 6, 4  # rounds of 4 and 2
PICK = (0, 1, 11)  # of a case's twelve targets: two scrambled ones and the last, which the golden cases solve on arrival

# (case, S or None: deterministic, reuse, mcts_nodes, fast, virtual_loss)
CALLS = [(case, S, reuse, nodes, None, vl) for case in CASES for vl in (0.0, 0.5)
         for S, reuse, nodes in ((None, False, None), (2, False, None), (None, True, None), (None, True, N + 1))]
CALLS += [("clifford-3q", 2, True, None, None, 0.5), ("clifford-3q", 2, True, N + 1, None, 0.0)]
CALLS += [("clifford-3q", None, False, None, True, 0.5), ("clifford-3q", 2, False, None, True, 0.0), ("clifford-3q", None, True, N + 1, True, 0.5)]
STATS = {"mcts", "targets", "steps", "solved", "mean_gates", "nodes", "kernels", "leaves", "rounds", "idle"}


def call_id(call):
    case, S, reuse, nodes, fast, vl = call
    return f"{case}-" + (f"S={S}-" if S else "") + ("reuse-" if reuse else "") + (f"nodes={nodes}-" if nodes else "") + ("fast-" if fast else "") + f"vl={vl}"


def small_case(case):
    gym, policy, states, raw = CASES[case]()
    return gym, policy, [states[i] for i in PICK], None if raw is None else [raw[i] for i in PICK]


def recorded_search(monkeypatch, gym, policy, states, seed, **kw):
    """`solve(states, **kw)` with the stand-ins in place.  Returns (solutions, last_stats, the calls in order -- ("root" | "select" |
    "backup" | "decide" | "move" | "rebase", what the call read and wrote, as numpy copies), what `_winner` saw, the synthesis)."""
    from qiskit_gym_amd import synthesis
    from qiskit_gym_amd.vec import VecEnv

    log, steps, kept = [], [], {}
    real = dict(select=synthesis.mcts_select_many, backup=synthesis.mcts_backup_many, root=synthesis.mcts_backup, decide=synthesis.mcts_decide,
                rebase=synthesis.mcts_rebase, step=VecEnv.step, winner=synthesis._winner)

    def cpu(t):
        return None if t is None else t.cpu().numpy().copy()

    def snapshot(forest):
        return {name: cpu(getattr(forest, name)) for name in FIELDS}

    def select(forest, C, K, k=None, virtual_loss=0.0, finished=None, *out):
        res = real["select"](forest, C, K, k, virtual_loss, finished, *out)
        log.append(("select", dict(C=C, K=K, k=k, vl=virtual_loss, finished=cpu(finished), picked=[cpu(t) for t in res])))
        return res

    def backup(forest, K, logp, values, reward, done, src, dst, act, leaf, k=None):
        res = real["backup"](forest, K, logp, values, reward, done, src, dst, act, leaf, k)
        log.append(("backup", dict(K=K, k=k, logp=cpu(logp), values=cpu(values), reward=cpu(reward), done=cpu(done),
                                   picked=[cpu(t) for t in (src, dst, act, leaf)], forest=snapshot(forest))))
        return res

    def root(forest, logp, values, reward=None, done=None, src=None, dst=None, act=None, leaf=None, root=False):
        assert root, "a search in rounds backs up through mcts_backup_many"
        res = real["root"](forest, logp, values, reward, done, src, dst, act, leaf, root)
        log.append(("root", dict(logp=cpu(logp), values=cpu(values), done=cpu(done), forest=snapshot(forest))))
        return res

    def decide(forest, sample=False, seed=0, counter=0, finished=None, move=None, counts=None):
        res = real["decide"](forest, sample, seed, counter, finished, move, counts)
        log.append(("decide", dict(sample=sample, seed=seed, counter=counter, finished=cpu(finished), move=cpu(res))))
        return res

    def rebase(forest, move, finished=None, env_src=None):
        res = real["rebase"](forest, move, finished, env_src)
        log.append(("rebase", dict(move=cpu(move), finished=cpu(finished), env_src=cpu(res), forest=snapshot(forest))))
        return res

    def step(self, actions, coins=None):
        steps.append((self, len(log), cpu(actions).astype(np.int64)))
        return real["step"](self, actions, coins)

    def winner(solved, ret):
        kept["ok"], kept["ret"] = cpu(solved), cpu(ret)
        res = real["winner"](solved, ret)
        kept["best"] = cpu(res[1])
        return res

    def never(*a, **k):
        raise AssertionError("a search in rounds selects through mcts_select_many")

    syn = synthesis.BatchedSynthesis(gym, policy, seed=seed)
    with monkeypatch.context() as m:
        for name, fn in (("mcts_select_many", select), ("mcts_backup_many", backup), ("mcts_backup", root), ("mcts_decide", decide),
                         ("mcts_rebase", rebase), ("_winner", winner), ("mcts_select", never)):
            m.setattr(synthesis, name, fn)
        m.setattr(VecEnv, "step", step)
        sols = syn.solve(states, **kw)
    assert len(syn._held) == 1
    (kind, held), = syn._held.items()
    real_envs = held.vecs[-1]
    assert all(v is held.vecs[0] or v is real_envs for v, _, _ in steps)  # the pools are only ever copied into and out of
    moves = 0
    for v, at, actions in steps:  # the real envs' moves, each in its place among the tree's calls (`at` counted those alone)
        if v is real_envs:
            log.insert(at + moves, ("move", dict(actions=actions)))
            moves += 1
    return sols, dict(syn.last_stats), log, kept, kind, held


@pytest.mark.parametrize("call", CALLS, ids=call_id)
def test_search_against_the_model_round_by_round(monkeypatch, call):
    case, S, reuse, nodes, fast, vl = call
    gym, policy, states, raw = small_case(case)
    seed, sampled = 1, S is not None
    kw = dict(num_mcts_searches=N, fast=fast, mcts_leaves=K, virtual_loss=vl)
    kw.update(dict(mcts_sampled=True, num_searches=S) if sampled else dict(deterministic=True))
    if reuse:
        kw.update(reuse_tree=True, mcts_nodes=nodes)
    sols, stats, log, kept, kind, held = recorded_search(monkeypatch, gym, policy, states, seed, **kw)

    gs = gym.config["gateset"]
    A, T, M = len(gs), gym.config["max_depth"], len(states)
    B, cap = M * (S or 1), (nodes or 2 * N + 1) if reuse else N + 1
    assert kind == ("mcts-sampled" if sampled else "mcts") + ("-reuse" if reuse else "") + "-many"
    assert held.key == ((B * K, B * cap, B * cap, B, False) if reuse else (B * K, B * cap, B, False))  # the leaf batch has K envs per tree
    assert set(stats) == STATS | ({"searches", "searches_solved"} if sampled else set()) | ({"reuse", "capacity", "carried", "refused"} if reuse else set())
    assert stats["kernels"] is bool(fast) and stats["mcts"] == N and stats["leaves"] == K and stats["rounds"] == 2
    targets = oracle_targets(gym, states, raw)
    many = dict(leaves=K, virtual_loss=vl)
    if reuse:
        model = (ManyReuseSampledMctsModel(targets, S, N, A, T, seed=seed, cap=cap, **many) if sampled
                 else ManyReuseMctsModel(targets, N, A, T, cap=cap, **many))
    else:
        model = ManySampledMctsModel(targets, S, N, A, T, seed=seed, **many) if sampled else ManyMctsModel(targets, N, A, T, **many)
    f = model.forest
    assert f.M == B and f.cap == cap and model.rounds == 2
    events = iter(log)
    expanded = several = 0
    for t in range(stats["steps"]):
        assert not model.ended, f"the search went on after decision {t}"
        if t == 0 or not reuse:
            kind_, rec = next(events)
            assert kind_ == "root", f"decision {t}: a {kind_} call"
            np.testing.assert_array_equal(rec["done"] != 0, model.finished, err_msg=f"decision {t}: which real envs are final")
            assert rec["logp"].shape[0] == B and rec["values"].shape == (B,)
            model.start(rec["forest"]["prior"][:, 0, :], rec["values"])
            expect_trees(rec["forest"], f, f"decision {t}: root")
        for r, k in enumerate((4, 2)):
            label = f"decision {t} round {r}"
            kind_, rec = next(events)
            assert kind_ == "select" and (rec["C"], rec["K"], rec["k"], rec["vl"]) == (2 ** 0.5, K, k, vl), f"{label}: a {kind_} call"
            np.testing.assert_array_equal(rec["finished"] != 0, model.finished, err_msg=label)
            src, dst, act, leaf = model.select()
            for name, g, w in zip(("src", "dst", "act", "leaf"), rec["picked"], (src, dst, act, leaf)):
                np.testing.assert_array_equal(g, w, err_msg=f"{label}: {name}")
            model.expand()
            kind_, rec = next(events)
            assert kind_ == "backup" and (rec["K"], rec["k"]) == (K, k) and rec["logp"].shape[0] == B * K
            for g, w in zip(rec["picked"], (src, dst, act, leaf)):
                np.testing.assert_array_equal(g, w, err_msg=label)
            grown = act < A
            prior = np.zeros((B * K, A), dtype=np.float32)
            for e in np.nonzero(grown)[0]:
                prior[e] = rec["forest"]["prior"][e // K, leaf[e]]
            want = np.exp(rec["logp"][grown, :A])
            assert (np.abs(prior[grown].astype(np.float64) - want) <= 4 * np.spacing(want)).all(), label
            reward, done = model.backup(prior, rec["values"])
            np.testing.assert_array_equal(bits(rec["reward"][grown]), bits(reward[grown]), err_msg=f"{label}: the expanded envs' rewards")
            np.testing.assert_array_equal(rec["done"][grown] != 0, done[grown], err_msg=f"{label}: the expanded envs' terminal flags")
            expect_trees(rec["forest"], f, label)
            expanded += int(grown.sum())
            several += int((grown.reshape(B, K).sum(axis=1) >= 2).sum())
        kind_, rec = next(events)  # the decision on its kernel, in every mode
        assert kind_ == "decide" and rec["sample"] is sampled and (not sampled or (rec["seed"] == seed and rec["counter"] == t))
        np.testing.assert_array_equal(rec["finished"] != 0, model.finished, err_msg=f"decision {t}")
        move = model.decide()  # ... and the model's rebase
        np.testing.assert_array_equal(rec["move"], move, err_msg=f"decision {t}: the decision")
        kind_, rec = next(events)
        assert kind_ == "move"
        np.testing.assert_array_equal(rec["actions"], move, err_msg=f"decision {t}: the real envs' moves")
        if reuse:
            kind_, rec = next(events)
            assert kind_ == "rebase"
            np.testing.assert_array_equal(rec["move"], move, err_msg=f"decision {t}: the move the rebase was given")
            np.testing.assert_array_equal(rec["env_src"], model.env_srcs[-1], err_msg=f"decision {t}: env_src")
            expect_trees(rec["forest"], f, f"decision {t}: rebase")
    assert model.ended and next(events, None) is None, f"the search stopped after {stats['steps']} decisions, the model goes on"
    want, want_stats = model.result()
    print(f"{call_id(call)}: {stats}; {expanded} nodes expanded, {several} (tree, round) pairs with several")
    if sampled:
        np.testing.assert_array_equal(bits(kept["ret"].reshape(-1)), bits(model.ret), err_msg="the returns")
        winners = model.winners()
        assert [int(b) if w is not None else None for b, w in zip(kept["best"], winners)] == winners
    assert sols == want
    for key in want_stats:
        assert stats[key] == want_stats[key], key
    assert {"leaves", "rounds", "idle"} <= set(want_stats)
    assert expanded > 0 and several > 0 and 1.0 < stats["nodes"] <= cap
    if reuse and nodes == N + 1 and raw is None:  # carried trees with no room beyond one decision's nodes: they fill in the middle of a round
        assert stats["idle"] > 0 and stats["refused"] == stats["idle"]
    if not reuse:
        assert stats["idle"] == 0  # N + 1 nodes hold a decision's N descents
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
        assert sols[-1] == []  # the identity: solved on arrival


def test_one_leaf_is_the_search_without_the_keyword(monkeypatch):
    from qiskit_gym_amd import synthesis
    from qiskit_gym_amd.synthesis import BatchedSynthesis

    gym, policy, states, _ = golden_case("clifford_3q_custom", 6)
    calls = []
    for name in ("mcts_select_many", "mcts_backup_many"):
        monkeypatch.setattr(synthesis, name, lambda *a, _n=name, **k: calls.append(_n))
    syn, other = BatchedSynthesis(gym, policy, seed=5), BatchedSynthesis(gym, policy, seed=5)
    det, smp = dict(deterministic=True, num_mcts_searches=4), dict(mcts_sampled=True, num_searches=2, num_mcts_searches=4)
    for kw in (det, smp, dict(det, reuse_tree=True), dict(smp, reuse_tree=True, mcts_nodes=7), dict(det, fast=True)):
        want = other.solve(states, **kw)
        got = syn.solve(states, mcts_leaves=1, virtual_loss=0.0, **kw)
        assert got == want and syn.last_stats == other.last_stats and list(syn.last_stats) == list(other.last_stats), kw
        assert not {"leaves", "rounds", "idle"} & set(syn.last_stats)
        assert {k: v.key for k, v in syn._held.items()} == {k: v.key for k, v in other._held.items()}  # the same handles: no kind of its own
    assert not calls and not any(k.endswith("-many") for k in syn._held)
    monkeypatch.undo()
    # beside them, the handles of a search in rounds; a K = 1 handle set is not reused with another leaf size
    vecs = syn._held["mcts"].vecs
    sols = syn.solve(states, mcts_leaves=2, **det)
    assert syn._held["mcts"].vecs is vecs and syn._held["mcts-many"].key == (len(states) * 2, len(states) * 5, len(states), False)
    assert syn.last_stats["leaves"] == 2 and syn.last_stats["rounds"] == 2 and sols[-1] == [] and syn.solve(states, mcts_leaves=2, **det) == sols
    assert syn.solve(states, **det) == other.solve(states, **det)
