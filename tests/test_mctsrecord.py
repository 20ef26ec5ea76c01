"""The replay of tests/mctsrecord.py on its own: it is where the checks of five search modes live, so it is checked once, without a GPU.  A
second model instance plays the device: `run_alone` under the hand-written policy of tests/test_mctsmodel.py, emitting the recorder's event
records from the model's own arrays.  The clean log passes; every single wrong number in it, and every event too few or too many, is an
AssertionError."""
import copy

import numpy as np
import pytest

from mctsmodel import FIELDS, run_alone
from mctsrecord import Draws, model_for, replay
from mctssample_model import SampledMctsModel
from test_mctsmodel import handmade, target_envs

N, T, SEED = 5, 8, 3
# one configuration per family: the arguments of `model_for`
CONFIGS = {
    "plain": dict(S=None),
    "sampled": dict(S=2, seed=SEED),
    "reuse": dict(S=None, cap=N + 1),
    "rounds": dict(S=None, leaves=4, virtual_loss=0.5),  # k = 4, then 1
    "all": dict(S=2, seed=SEED, cap=2 * N + 1, leaves=4, virtual_loss=0.5),
}
_logs = {}


def model(config):
    gs, envs = target_envs("clifford", 2, 11)
    return model_for(envs, N=N, A=len(gs), T=T, **CONFIGS[config])


def device_log(dev, evaluate, envs_too):
    """The events a recorded search of `dev`'s kind leaves, from `dev` driven by `run_alone`."""
    log, held = [], {"round": 0}
    f = dev.forest

    def snapshot():
        return {name: getattr(f, name).copy() for name in FIELDS}

    def flags(x):
        return np.asarray(x).astype(np.uint8)

    def asked(envs):
        logp, values = evaluate(envs)
        if envs is dev.real:  # the roots: the forest is theirs only after `start`, so the event waits for the first selection
            held["root"] = dict(K=1, k=1, logp=logp, values=values, reward=None, done=flags(dev.finished), picked=[None] * 4)
            return logp, values
        if "root" in held:
            log.append(("root", dict(held.pop("root"), forest=snapshot())))  # (a selection writes nothing into the forest)
        k = dev.k_of(held["round"])
        log.append(("select", dict(C=dev.C, K=dev.K, k=k, vl=dev.vl, finished=flags(dev.finished), picked=[p.copy() for p in dev.picked])))
        held["backup"] = dict(K=dev.K, k=k, logp=logp, values=values, picked=[p.copy() for p in dev.picked])
        return logp, values

    def after_round(m):
        reward = np.array([0 if e is None else e.reward() for e in m.fresh], dtype=np.float32)
        done = flags([False if e is None else e.is_final() for e in m.fresh])
        log.append(("backup", dict(held.pop("backup"), reward=reward, done=done, forest=snapshot())))
        held["round"] += 1
        held["finished"] = flags(m.finished)  # what the decision reads: the real envs step after it

    def after_decision(m, move):
        sampled = isinstance(m, SampledMctsModel)
        log.append(("decide", dict(sample=sampled, seed=SEED if sampled else 0, counter=m.t - 1 if sampled else 0, finished=held["finished"],
                                   move=move.copy(), counts=None)))
        log.append(("move", dict(actions=move.astype(np.int64))))
        held["round"] = 0
        if not m.carries:
            return
        log.append(("rebase", dict(move=move.copy(), finished=flags(m.finished), env_src=m.env_srcs[-1].copy(), forest=snapshot(), cap=f.cap)))
        if envs_too:
            some = m.real[0]
            rec = dict(state=np.zeros((f.M * f.cap, len(some.get_state())), dtype=np.int64), depth=np.zeros(f.M * f.cap, dtype=np.int32),
                       done=np.zeros(f.M * f.cap, dtype=np.uint8), reward=np.zeros(f.M * f.cap, dtype=np.float32))
            for tree in range(f.M):
                for j, env in m.pool[tree].items():
                    e = tree * f.cap + j
                    rec["state"][e], rec["depth"][e], rec["done"][e], rec["reward"][e] = env.get_state(), env.depth(), env.is_final(), env.reward()
            log.append(("pool", rec))

    run_alone(dev, asked, after_round, after_decision)
    return log


def clean_log(config):
    if config not in _logs:
        dev = model(config)
        _logs[config] = device_log(dev, handmade(dev.A), envs_too=config == "reuse")
    return copy.deepcopy(_logs[config])


def replayed(config, log):
    return replay(log, model(config), seed=SEED, on_decide=Draws() if CONFIGS[config]["S"] else None, envs_too=config == "reuse")


@pytest.mark.parametrize("config", CONFIGS)
def test_the_clean_log_passes(config):
    log = clean_log(config)
    kinds = [kind for kind, _ in log]
    assert kinds.count("decide") == kinds.count("move") == T
    assert kinds.count("root") == (1 if "cap" in CONFIGS[config] else T) and kinds.count("rebase") == (T if "cap" in CONFIGS[config] else 0)
    seen = replayed(config, log)
    assert seen.expanded > 0
    assert (seen.several > 0) == ("leaves" in CONFIGS[config]) and (seen.pools > 0) == (config == "reuse")


def event(log, kind, where=lambda rec: True, nth=0):
    """The index of the nth event of `kind` that `where` accepts."""
    found = [i for i, (k, rec) in enumerate(log) if k == kind and where(rec)]
    return found[nth]


def grows(rec):  # a backup that links a node
    return (rec["picked"][2] < rec["forest"]["child"].shape[2]).any()


def grown(rec):
    return int(np.nonzero(rec["picked"][2] < rec["forest"]["child"].shape[2])[0][0])


def bump(kind, field, index=0, where=lambda rec: True, nth=1, by=1):
    """One entry of an array field of an event, off by `by`."""
    def corrupt(log):
        rec = log[event(log, kind, where, nth)][1]
        rec[field].reshape(-1)[index] += by
    return corrupt


def flip(kind, field, index=0, nth=1):
    """One flag of a uint8 field of an event, flipped."""
    def corrupt(log):
        rec = log[event(log, kind, nth=nth)][1]
        rec[field].reshape(-1)[index] ^= 1
    return corrupt


def picked(kind, which, by=1):
    def corrupt(log):
        rec = log[event(log, kind, nth=1)][1]
        rec["picked"][which][0] += by
    return corrupt


def in_forest(kind, name):
    """One element of a forest array after an event: of the root (node 0 of tree 0, below n_nodes in every tree), or n_nodes itself."""
    def corrupt(log):
        rec = log[event(log, kind, nth=1)][1]
        rec["forest"][name].reshape(-1)[0] += 1
    return corrupt


def of_grown(field):
    def corrupt(log):
        rec = log[event(log, "backup", grows)][1]
        if field == "reward":
            rec["reward"][grown(rec)] = np.nextafter(rec["reward"][grown(rec)], np.float32(9))  # one bit
        else:
            rec["done"][grown(rec)] ^= 1
    return corrupt


def setter(kind, field, value, nth=1):
    def corrupt(log):
        rec = log[event(log, kind, nth=nth)][1]
        rec[field] = value(rec[field])
    return corrupt


def second_root(log):
    root = copy.deepcopy(log[event(log, "root")])
    at = event(log, "rebase") + 1  # behind the first rebase and its pool event: where decision 1 starts
    log.insert(at + (log[at][0] == "pool"), root)


def dropped(log):
    del log[event(log, "backup", nth=2)]


def trailing(log):
    log.append(copy.deepcopy(log[-1]))


EVERYWHERE = tuple(CONFIGS)
CORRUPTIONS = {
    "select-src": (picked("select", 0), EVERYWHERE),
    "select-dst": (picked("select", 1), EVERYWHERE),
    "select-act": (picked("select", 2), EVERYWHERE),
    "select-leaf": (picked("select", 3), EVERYWHERE),
    "backup-picked-src": (picked("backup", 0), EVERYWHERE),
    "backup-picked-leaf": (picked("backup", 3), EVERYWHERE),
    "backup-forest-visits": (in_forest("backup", "visits"), EVERYWHERE),
    "backup-forest-prior": (in_forest("backup", "prior"), ("plain", "all")),
    "backup-forest-child": (in_forest("backup", "child"), ("reuse", "rounds")),
    "rebase-forest-visits": (in_forest("rebase", "visits"), ("reuse", "all")),
    "rebase-forest-value": (in_forest("rebase", "value"), ("reuse", "all")),
    "backup-n_nodes": (in_forest("backup", "n_nodes"), EVERYWHERE),
    "rebase-n_nodes": (in_forest("rebase", "n_nodes"), ("reuse", "all")),
    "root-forest-visits": (in_forest("root", "visits"), ("plain", "sampled", "rounds")),
    "grown-reward-bit": (of_grown("reward"), EVERYWHERE),
    "grown-done": (of_grown("done"), EVERYWHERE),
    "select-finished": (flip("select", "finished"), EVERYWHERE),
    "decide-finished": (flip("decide", "finished"), EVERYWHERE),
    "rebase-finished": (flip("rebase", "finished"), ("reuse", "all")),
    "root-done": (flip("root", "done"), ("plain", "sampled", "rounds")),
    "sample-flipped": (setter("decide", "sample", lambda x: not x), EVERYWHERE),
    "counter-off-by-one": (setter("decide", "counter", lambda x: x + 1), ("sampled", "all")),
    "wrong-seed": (setter("decide", "seed", lambda x: x + 1), ("sampled", "all")),
    "decide-move": (bump("decide", "move"), EVERYWHERE),
    "move-action": (bump("move", "actions"), EVERYWHERE),
    "rebase-move": (bump("rebase", "move"), ("reuse", "all")),
    "env_src": (bump("rebase", "env_src"), ("reuse", "all")),
    "cap": (setter("rebase", "cap", lambda x: x + 1), ("reuse", "all")),
    "select-k": (setter("select", "k", lambda x: x + 1), EVERYWHERE),
    "backup-k": (setter("backup", "k", lambda x: x + 1), EVERYWHERE),
    "select-K": (setter("select", "K", lambda x: x + 1), EVERYWHERE),
    "select-vl": (setter("select", "vl", lambda x: x + 0.25), EVERYWHERE),
    "select-C": (setter("select", "C", lambda x: x + 0.25), EVERYWHERE),
    "backup-logp-rows": (setter("backup", "logp", lambda x: x[:-1]), EVERYWHERE),
    "second-root-under-reuse": (second_root, ("reuse", "all")),
    "pool-depth": (bump("pool", "depth", nth=0), ("reuse",)),
    "dropped-event": (dropped, EVERYWHERE),
    "trailing-event": (trailing, EVERYWHERE),
}
CASES = [(name, config) for name, (_, configs) in CORRUPTIONS.items() for config in configs]


@pytest.mark.parametrize("case", CASES, ids=lambda case: "-".join(case))
def test_one_wrong_number_is_an_assertion_error(case):
    name, config = case
    log = clean_log(config)
    CORRUPTIONS[name][0](log)
    with pytest.raises(AssertionError):
        replayed(config, log)
