"""The CPU model of the PUCT search (tests/mctsmodel.py) on its own: oracle envs, a hand-written prior / value function.  The device kernels
and `BatchedSynthesis.solve(num_mcts_searches=N)` are held to this model bit for bit (tests/test_gpu_mcts_kernels.py, tests/test_gpu_mcts.py),
so the model's own rules are checked here: tree invariants after every simulation, a one-hot prior that must be followed, and the
selection's arg-max against a plain loop over every combination of a small set of numbers."""
import itertools

import numpy as np
import pytest

from mctsmodel import F32, Forest, MctsModel, best_action, check_invariants, decide, root, run_alone, scores, select
from oracle import OracleEnv
from util import line_gateset

KINDS = ["linear_function", "clifford"]


def target_envs(kind, count, seed, scramble=3):
    gs = line_gateset(kind, 3)
    rng = np.random.default_rng(seed)
    kw = dict(add_inverts=0, add_perms=0, difficulty=4, max_depth=12)
    out = []
    for _ in range(count):
        src = OracleEnv(kind, 3, gs, track_solution=0, **dict(kw, difficulty=scramble))  # `reset_with` takes exactly `difficulty` gates
        src.reset_with(rng.integers(0, len(gs), size=scramble))
        env = OracleEnv(kind, 3, gs, track_solution=1, **kw)
        env.set_state(src.get_state().tolist())
        out.append(env)
    out.append(OracleEnv(kind, 3, gs, track_solution=1, **kw))  # solved on arrival
    return gs, out


def handmade(A):
    """A prior and a value that depend on the observation only, quantised so that equal scores are frequent."""
    def evaluate(envs):
        logp, values = np.zeros((len(envs), A), dtype=F32), np.zeros(len(envs), dtype=F32)
        for i, env in enumerate(envs):
            if env is None:
                continue
            obs = env.observe()
            h = sum((k + 3) * (x + 1) for k, x in enumerate(obs))
            logits = np.array([((h * (a + 7)) % 5) / 4.0 for a in range(A)], dtype=F32)
            logp[i] = logits - F32(np.log(np.exp(logits.astype(np.float64)).sum()))
            values[i] = F32(-(len(obs) % 4) / 8.0)
        return logp, values
    return evaluate


@pytest.mark.parametrize("N", [1, 2, 9])
@pytest.mark.parametrize("kind", KINDS)
def test_invariants_hold_after_every_simulation(kind, N):
    gs, envs = target_envs(kind, 5, 11)
    A = len(gs)
    model = MctsModel(envs, N, A, 12)
    seen = {"sims": 0, "full": 0}

    def after(model):
        seen["sims"] += 1
        check_invariants(model.forest, model.sims)
        f = model.forest
        assert (f.n_nodes <= f.cap).all() and (f.visits[:, 0] == 1 + model.sims).all()
        assert (model.sims[model.finished] == 0).all()  # a finished tree makes no simulation that counts
        seen["full"] += int((f.n_nodes == f.cap).sum())

    sols, stats = run_alone(model, handmade(A), after)
    assert seen["sims"] == stats["steps"] * N and seen["full"] > 0  # some tree filled its N + 1 nodes exactly
    assert sols[-1] == [] and len(sols) == len(envs)
    assert stats["solved"] == sum(s is not None for s in sols) >= 1
    assert 1.0 < stats["nodes"] <= N + 1
    for env, sol in zip(envs, sols):
        if sol is not None:  # the answer is the real env's log: replayed from the target it solves it
            again = env.clone()
            for a in sol:
                assert not again.success()
                again.step(a)
            assert again.success() and again.solution() == sol


def shortest_solution(env, A, limit=4):
    """Breadth first over the gates: the first sequence that reaches success."""
    layer = [([], env)]
    for _ in range(limit):
        nxt = []
        for seq, e in layer:
            for a in range(A):
                c = e.clone()
                c.step(a)
                if c.success():
                    return seq + [a]
                nxt.append((seq + [a], c))
        layer = nxt
    return None


@pytest.mark.parametrize("N", [1, 2, 9])
@pytest.mark.parametrize("kind", KINDS)
def test_a_one_hot_prior_on_a_solving_sequence_is_followed(kind, N):
    gs, envs = target_envs(kind, 4, 5)
    A = len(gs)
    for env in envs[:-1]:  # one target at a time: the table of a target's sequence is its own
        seq = shortest_solution(env, A)
        assert seq, "three scrambling gates are undone by at most four"
        follow, e = {}, env.clone()
        for a in seq:  # the states along a shortest sequence differ
            follow[tuple(e.observe())] = a
            e.step(a)

        def one_hot(envs_):
            logp = np.full((len(envs_), A), -np.inf, dtype=F32)
            for i, env_ in enumerate(envs_):
                a = None if env_ is None else follow.get(tuple(env_.observe()))
                if a is None:
                    logp[i] = F32(-np.log(A))  # off the sequence (past its end): uniform
                else:
                    logp[i, a] = 0.0
            return logp, np.zeros(len(envs_), dtype=F32)

        sols, stats = run_alone(MctsModel([env], N, A, 12), one_hot)
        assert sols == [seq] and stats["solved"] == 1 and stats["steps"] == 8  # the first look at the real envs is after decision 7


def plain_scores(f, x, C):
    """The rule as a loop over the actions, one np.float32 operation at a time."""
    out = []
    for a in range(f.A):
        c = int(f.child[0, x, a])
        if c >= 0:
            q = F32(f.wsum[0, c]) / F32(int(f.visits[0, c]))
            n_a = int(f.visits[0, c])
        else:
            q, n_a = F32(f.value[0, x]), 0
        u = F32(C) * F32(f.prior[0, x, a])
        u = u * np.sqrt(F32(int(f.visits[0, x])))
        u = u / F32(1 + n_a)
        out.append(F32(q + u))
    return out


def test_selection_argmax_against_a_plain_loop():
    """Every assignment of (expanded?, visits, wsum) and prior from small sets to the three edges of a root: the model's winner is the plain
    loop's, the lowest action among equal scores, and an unvisited edge is valued at the node's own value."""
    A, C = 3, 2 ** 0.5
    edges = [None, (1, 0.5), (1, -0.25), (2, 1.0), (3, 0.0)]  # None: not expanded; else (visits, wsum)
    priors = [0.0, 0.25, 0.5]
    checked = ties = unvisited_wins = 0
    for value in (0.0, 0.5, -0.25):
        for combo in itertools.product(edges, repeat=A):
            for pr in itertools.product(priors, repeat=A):
                f = Forest(1, 4, A)
                root(f, np.array([pr], dtype=F32), np.array([value], dtype=F32))
                n = 1
                for a, e in enumerate(combo):
                    if e is None:
                        continue
                    f.child[0, 0, a], f.parent[0, n], f.visits[0, n], f.wsum[0, n] = n, 0, e[0], e[1]
                    f.child[0, n] = -1
                    f.terminal[0, n] = 1  # the descent stops below the root: one level is compared
                    n += 1
                f.n_nodes[0] = n
                f.visits[0, 0] = 1 + sum(e[0] for e in combo if e is not None)
                sc = plain_scores(f, 0, C)
                np.testing.assert_array_equal(np.array(sc, dtype=F32).view(np.uint32), scores(f, 0, 0, C).view(np.uint32))
                top = max(sc)
                want = min(a for a in range(A) if sc[a] == top)
                assert best_action(np.array(sc, dtype=F32)) == want
                ties += sum(s == top for s in sc) > 1
                src, dst, act, leaf = select(f, C)
                checked += 1
                if combo[want] is None:
                    unvisited_wins += 1
                    if n < f.cap:
                        assert (src[0], dst[0], act[0], leaf[0]) == (0, n, want, n)
                else:  # the child is terminal: the descent ends there, nothing is expanded
                    assert (src[0], dst[0], act[0], leaf[0]) == (f.child[0, 0, want], f.skip, A, f.child[0, 0, want])
    assert checked == 3 * 5 ** 3 * 3 ** 3 and ties > 500 and unvisited_wins > 500
    assert best_action(np.array([np.nan, -0.0, 0.0], dtype=F32)) == 1  # a NaN is no candidate, -0 ties with +0
    assert best_action(np.array([np.nan, np.nan], dtype=F32)) is None


def test_decision_takes_the_most_visited_child_lowest_on_ties():
    f = Forest(2, 4, 3)
    root(f, np.full((2, 3), 1 / 3, dtype=F32), np.zeros(2, dtype=F32))
    f.child[0, 0] = [-1, 1, 2]
    f.visits[0, 1:3] = [2, 2]
    f.n_nodes[0] = 3
    assert decide(f).tolist() == [1, 3]  # equal visits: the lower action; no child: A
