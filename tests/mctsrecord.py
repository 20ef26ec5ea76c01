"""What the tests that hold `BatchedSynthesis`'s tree search to the CPU models share (tests/test_gpu_mcts.py, test_gpu_mcts_sampled.py,
test_gpu_mcts_reuse.py, test_gpu_mcts_many_search.py, test_gpu_self_play.py): ONE recorder, which runs a call with a stand-in on every tree
call the search looks up in `synthesis` and keeps what each read and wrote, and ONE replay, which walks that log against any model of the
family (tests/mctsmodel.py, mctssample_model.py, mctsreuse_model.py, mctsmany_model.py, azmodel.py) and applies every check at every event
in every mode.  The events of a search, per decision:

    root? (select backup){rounds} decide move rebase? pool?

`root` at every decision, with carried trees at decision 0 only; `rebase` with carried trees; `pool` where the recorder was asked for the
pool's envs.  TEST INFRASTRUCTURE ONLY.  Nothing here imports torch or the package at module level: tests/test_mctsrecord.py checks the replay
without a GPU."""
from collections import namedtuple

import numpy as np

from azmodel import SelfPlayModel
from mctsmany_model import ManyMctsModel, ManyReuseMctsModel, ManyReuseSampledMctsModel, ManySampledMctsModel
from mctsmodel import FIELDS, MARKER, MctsModel
from mctsreuse_model import ReuseMctsModel, ReuseSampledMctsModel
from mctssample_model import SampledMctsModel, counts
from util import bits

NODE_FIELDS = tuple(name for name in FIELDS if name != "n_nodes")
PICKED = ("src", "dst", "act", "leaf")
# every name the search looks up in `synthesis`, whatever the mode; `_TreeSearch` itself tells the recorder the options and the handles
TREE_CALLS = ("mcts_select", "mcts_select_many", "mcts_backup", "mcts_backup_many", "mcts_decide", "mcts_rebase", "_winner", "_TreeSearch")

# what `record` returns: what the call returned, `last_stats`, the events in order -- (kind, what the call read and wrote, as numpy copies) --,
# what `_winner` saw, the kind and the `_Handles` of the one search the call made, and its `_MctsOptions`
Recorded = namedtuple("Recorded", "out stats log kept kind held opts")


def record(monkeypatch, syn, call, envs_too=False) -> Recorded:
    """`call(syn)` -- `lambda syn: syn.solve(states, **kw)` or `lambda syn: syn.self_play(**kw)` -- with the stand-ins in place.  Each runs
    the real function and appends one event; the one-descent pair records K = k = 1 and vl = 0.0, so a replay never asks which pair ran.
    Which pair must have run follows from the options of the search the call made.  `envs_too`: a "pool" event after every rebase, the
    envs of the pool the kept nodes' envs were copied into."""
    import torch

    from qiskit_gym_amd import synthesis
    from qiskit_gym_amd.vec import VecEnv

    log, steps, kept, made, turns, last = [], [], {}, [], [], {}
    real = {name: getattr(synthesis, name) for name in TREE_CALLS}
    real_step, real_copy = VecEnv.step, VecEnv.copy_envs

    def cpu(t):
        return None if t is None else t.cpu().numpy().copy()

    def snapshot(forest):
        return {name: cpu(getattr(forest, name)) for name in FIELDS}

    def leaves():
        return made[-1][0].K

    def search(opts, held, *a, **k):
        made.append((opts, held))
        return real["_TreeSearch"](opts, held, *a, **k)

    def select(forest, C, finished=None, *out):
        assert leaves() == 1, "a search in rounds selects through mcts_select_many"
        res = real["mcts_select"](forest, C, finished, *out)
        log.append(("select", dict(C=C, K=1, k=1, vl=0.0, finished=cpu(finished), picked=[cpu(t) for t in res])))
        return res

    def select_many(forest, C, K, k=None, virtual_loss=0.0, finished=None, *out):
        assert leaves() > 1, "a search of one leaf selects through mcts_select"
        res = real["mcts_select_many"](forest, C, K, k, virtual_loss, finished, *out)
        log.append(("select", dict(C=C, K=K, k=k, vl=virtual_loss, finished=cpu(finished), picked=[cpu(t) for t in res])))
        return res

    def backup(forest, logp, values, reward=None, done=None, src=None, dst=None, act=None, leaf=None, root=False):
        assert root or leaves() == 1, "a search in rounds backs up through mcts_backup_many"
        res = real["mcts_backup"](forest, logp, values, reward, done, src, dst, act, leaf, root)
        log.append(("root" if root else "backup", dict(K=1, k=1, logp=cpu(logp), values=cpu(values), reward=cpu(reward), done=cpu(done),
                                                       picked=[cpu(t) for t in (src, dst, act, leaf)], forest=snapshot(forest))))
        return res

    def backup_many(forest, K, logp, values, reward, done, src, dst, act, leaf, k=None):
        assert leaves() > 1, "a search of one leaf backs up through mcts_backup"
        res = real["mcts_backup_many"](forest, K, logp, values, reward, done, src, dst, act, leaf, k)
        log.append(("backup", dict(K=K, k=k, logp=cpu(logp), values=cpu(values), reward=cpu(reward), done=cpu(done),
                                   picked=[cpu(t) for t in (src, dst, act, leaf)], forest=snapshot(forest))))
        return res

    def decide(forest, sample=False, seed=0, counter=0, finished=None, move=None, counts=None):
        before = {name: getattr(forest, name).clone() for name in FIELDS}
        res = real["mcts_decide"](forest, sample, seed, counter, finished, move, counts)
        for name in FIELDS:  # the decision wrote nothing into the forest (compared on the device, byte by byte)
            assert torch.equal(before[name].view(torch.uint8), getattr(forest, name).view(torch.uint8)), (counter, name)
        log.append(("decide", dict(sample=sample, seed=seed, counter=counter, finished=cpu(finished), move=cpu(res), counts=cpu(counts))))
        return res

    def rebase(forest, move, finished=None, env_src=None):
        res = real["mcts_rebase"](forest, move, finished, env_src)
        last["env_src"] = res
        log.append(("rebase", dict(move=cpu(move), finished=cpu(finished), env_src=cpu(res), forest=snapshot(forest), cap=forest.cap)))
        return res

    def copy_envs(self, src, src_idx, dst_idx=None):
        res = real_copy(self, src, src_idx, dst_idx)
        if "env_src" in last and src_idx is last["env_src"]:  # the kept nodes' envs, into the other pool
            turns.append((self, src))
            if envs_too:
                log.append(("pool", dict(state=cpu(self.get_state()), depth=cpu(self.depth), done=cpu(self.done), reward=cpu(self.reward))))
        return res

    def step(self, actions, coins=None):
        steps.append((self, len(log), cpu(actions).astype(np.int64)))
        return real_step(self, actions, coins)

    def winner(solved, ret):
        kept["ok"], kept["ret"] = cpu(solved), cpu(ret)
        res = real["_winner"](solved, ret)
        kept["best"] = cpu(res[1])
        return res

    stand_ins = dict(mcts_select=select, mcts_select_many=select_many, mcts_backup=backup, mcts_backup_many=backup_many, mcts_decide=decide,
                     mcts_rebase=rebase, _winner=winner, _TreeSearch=search)
    with monkeypatch.context() as m:
        for name in TREE_CALLS:
            m.setattr(synthesis, name, stand_ins[name])
        m.setattr(VecEnv, "step", step)
        m.setattr(VecEnv, "copy_envs", copy_envs)
        out = call(syn)
    (opts, held), = made  # one search
    (kind,) = [k for k, h in syn._held.items() if h is held]
    leaf, *pools, real_envs = held.vecs
    assert all(v is leaf or v is real_envs for v, _, _ in steps)  # the pools are only ever copied into and out of
    if opts.cap is None:
        assert len(pools) == 1 and not turns
    else:
        pool_a, pool_b = pools
        assert [p for p, _ in turns] == [(pool_b, pool_a)[i % 2] for i in range(len(turns))]  # they take turns
        assert all({p, s} == {pool_a, pool_b} for p, s in turns)
    moves = 0
    for v, at, actions in steps:  # the real envs' moves, each in its place among the tree's calls (`at` counted those alone)
        if v is real_envs:
            log.insert(at + moves, ("move", dict(actions=actions)))
            moves += 1
    return Recorded(out, dict(syn.last_stats), log, kept, kind, held, opts)


def expect_forest(got, model, label):
    """The recorded forest against the model's: the whole arrays, by bit pattern."""
    for name in FIELDS:
        want = getattr(model, name)
        assert got[name].dtype == want.dtype and got[name].shape == want.shape, (label, name)
        np.testing.assert_array_equal(bits(got[name]), bits(want), err_msg=f"{label}: {name}")


def expect_trees(got, model, label):
    """The recorded forest against the model's: every tree on its nodes below n_nodes."""
    np.testing.assert_array_equal(got["n_nodes"], model.n_nodes, err_msg=f"{label}: n_nodes")
    for name in NODE_FIELDS:
        want = getattr(model, name)
        assert got[name].dtype == want.dtype and got[name].shape == want.shape, (label, name)
        for m in range(model.M):
            k = int(model.n_nodes[m])
            assert bits(got[name][m, :k]).tobytes() == bits(want[m, :k]).tobytes(), f"{label}: {name} of tree {m}"


def near_exp(prior, logp):
    """The device's priors against exp(logp): within 4 spacings, the difference taken in f64."""
    want = np.exp(logp)
    return bool((np.abs(prior.astype(np.float64) - want) <= 4 * np.spacing(want)).all())


Counters = namedtuple("Counters", "expanded several pools")  # nodes expanded; (tree, round) pairs that expanded several; pool envs compared


def replay(log, model, *, seed=None, on_decide=None, envs_too=False) -> Counters:
    """Walks `log` against `model`, which makes the same search on oracle envs with the device's own priors and values.  `seed`: the
    call's, for a sampled model; `on_decide(t, rec, model)` is called at every decision before the model decides; `envs_too`: a "pool"
    event follows every rebase.  A search that rebuilds its trees for every decision and makes one descent per round is compared on the
    whole forest arrays, one with carried trees or several descents per round on every tree's nodes below n_nodes."""
    f, A, K, trees = model.forest, model.A, model.K, model.forest.M
    sampled = isinstance(model, SampledMctsModel)
    expect = expect_trees if model.carries or K > 1 else expect_forest
    events = iter(log)
    expanded = several = pools = 0

    def take(kind, label):
        got, rec = next(events, ("no", None))
        assert got == kind, f"{label}: {got} call where a {kind} call is due"
        return rec

    def same(got, want, label):
        np.testing.assert_array_equal(got, want, err_msg=label)

    t = 0
    while not model.ended:
        if t == 0 or not model.carries:  # with carried trees: no root forward pass and no root backup after decision 0
            label = f"decision {t}: root"
            rec = take("root", label)
            same(rec["done"] != 0, model.finished, f"{label}: which real envs are final")
            assert rec["logp"].shape[0] == trees and rec["values"].shape == (trees,), label
            prior = rec["forest"]["prior"][:, 0, :]
            assert near_exp(prior, rec["logp"][:, :A]), label
            model.start(prior, rec["values"])
            expect(rec["forest"], f, label)
        for r in range(model.rounds):
            label, k = f"decision {t} round {r}", model.k_of(r)
            rec = take("select", label)
            assert (rec["C"], rec["K"], rec["k"], rec["vl"]) == (model.C, K, k, model.vl), label
            same(rec["finished"] != 0, model.finished, label)
            picked = model.select()
            for name, g, w in zip(PICKED, rec["picked"], picked):
                same(g, w, f"{label}: {name}")
            model.expand()
            rec = take("backup", label)
            assert (rec["K"], rec["k"]) == (K, k) and rec["logp"].shape[0] == trees * K, label
            for name, g, w in zip(PICKED, rec["picked"], picked):
                same(g, w, f"{label}: {name} as the backup was given it")
            act, leaf = picked[2], picked[3]
            grown = act < A
            prior = np.zeros((trees * K, A), dtype=np.float32)
            for e in np.nonzero(grown)[0]:
                prior[e] = rec["forest"]["prior"][e // K, leaf[e]]
            assert near_exp(prior[grown], rec["logp"][grown, :A]), label
            reward, done = model.backup(prior, rec["values"])
            same(bits(rec["reward"][grown]), bits(reward[grown]), f"{label}: the expanded envs' rewards")
            same(rec["done"][grown] != 0, done[grown], f"{label}: the expanded envs' terminal flags")
            expect(rec["forest"], f, label)
            expanded += int(grown.sum())
            several += int((grown.reshape(trees, K).sum(axis=1) >= 2).sum())
        label = f"decision {t}"
        rec = take("decide", label)  # one decision, on its kernel, in every mode: the most visited action, or a draw
        assert rec["sample"] is sampled and (not sampled or (rec["seed"] == seed and rec["counter"] == t)), label
        same(rec["finished"] != 0, model.finished, label)
        if on_decide is not None:
            on_decide(t, rec, model)
        move = model.decide()  # ... and, with carried trees, the model's rebase
        same(rec["move"], move, f"{label}: the decision")
        same(take("move", label)["actions"], move, f"{label}: the real envs' moves")
        if model.carries:
            rec = take("rebase", label)
            assert rec["cap"] == f.cap, label
            same(rec["move"], move, f"{label}: the move the rebase was given")
            same(rec["finished"] != 0, model.finished, f"{label}: `finished` is the array after the real envs' step")
            same(rec["env_src"], model.env_srcs[-1], f"{label}: env_src")
            expect_trees(rec["forest"], f, f"{label}: rebase")
            if envs_too:  # every kept node's env, in the pool it was copied into, is the model's
                rec = take("pool", label)
                for m in np.nonzero(~model.finished)[0]:
                    for j, env in model.pool[m].items():
                        e = m * f.cap + j
                        assert (rec["state"][e] == env.get_state()).all() and rec["depth"][e] == env.depth(), (t, m, j)
                        assert bool(rec["done"][e]) == env.is_final() and bits(rec["reward"][e : e + 1])[0] == bits(np.float32([env.reward()]))[0], (t, m, j)
                        pools += 1
        t += 1
    got, _ = next(events, (None, None))
    assert got is None, f"the model ended after {t} decisions, the search goes on: a {got} call"
    return Counters(expanded, several, pools)


class Draws:
    """`on_decide` for a sampled search: every live tree's draw is an action with visits, a finished tree gets none; counts the draws off
    the most visited action.  `rows`: the decision was asked for its rows of counts (`self_play`), which must be the model's."""

    def __init__(self, rows=False):
        self.rows, self.off_top = rows, 0

    def __call__(self, t, rec, model):
        A, live, n_a, draw = model.A, ~model.finished, counts(model.forest), rec["move"]
        if self.rows:
            assert rec["counts"] is not None, "self_play asks every decision for its rows of counts"
            np.testing.assert_array_equal(rec["counts"][:, :A], n_a, err_msg=f"decision {t}: the rows of counts")
        drawn = n_a[np.arange(len(draw)), np.minimum(draw, A - 1)]
        assert (draw[live] < A).all() and (drawn[live] > 0).all() and (draw[~live] == A).all(), f"decision {t}"
        self.off_top += int((drawn < n_a.max(axis=1))[live].sum())


def solutions_solve(sols, targets):
    """Every solution, replayed on the oracle from its target (`targets`: fresh envs, stepped here), solves it with exactly those entries."""
    for sol, env in zip(sols, targets):
        if sol is None:
            continue
        for a in sol:
            if a < MARKER:
                assert not env.success()
                env.step(int(a))
        assert env.success() and env.solution() == sol


MODELS = {(False, False, False): MctsModel, (True, False, False): SampledMctsModel, (False, True, False): ReuseMctsModel,
          (True, True, False): ReuseSampledMctsModel, (False, False, True): ManyMctsModel, (True, False, True): ManySampledMctsModel,
          (False, True, True): ManyReuseMctsModel, (True, True, True): ManyReuseSampledMctsModel}


def model_for(targets, *, S, N, A, T, seed=0, cap=None, leaves=1, virtual_loss=0.0, self_play=False):
    """The model of a search by the rule of `_MctsOptions.kind`: `S` searches per target with drawn moves (None: one tree, the most visited
    action), `cap` nodes per tree carried between decisions (None: N + 1, rebuilt), `leaves` > 1 descents per round.  `self_play` logs every
    decision; `SelfPlayModel` is the plain sampled search's only."""
    sampled, reuse, many = S is not None, cap is not None, leaves > 1
    kw = dict(seed=seed) if sampled else {}
    if reuse:
        kw.update(cap=cap)
    if many:
        kw.update(leaves=leaves, virtual_loss=virtual_loss)
    if self_play:
        assert sampled and not reuse and not many, "SelfPlayModel is the plain sampled search with a log"
        return SelfPlayModel(targets, S, N, A, T, **kw)
    return MODELS[sampled, reuse, many](targets, *((S,) if sampled else ()), N, A, T, **kw)
