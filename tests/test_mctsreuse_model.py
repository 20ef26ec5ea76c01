"""The CPU model of the tree search that keeps the chosen move's subtree between decisions (tests/mctsreuse_model.py) on its own.
`collector.mcts_rebase` and `BatchedSynthesis.solve(reuse_tree=True)` are held to this model bit for bit (tests/test_gpu_mcts_rebase.py,
tests/test_gpu_mcts_reuse.py), so the model's own rules are checked here, on trees grown by the model under a hand-written policy and under
the committed clifford_3q_custom weights: the invariants after every rebase, every kept node's fields, that the rebased tree IS the subtree
(the same descent, the same arrays after the same backup), the corner cases by hand, and one pinned search whose carried trees fill."""
import copy

import numpy as np
import pytest

from mctsmodel import F32, FIELDS, Forest, backup, best_action, check_invariants, root, scores
from mctsreuse_model import ReuseMctsModel, ReuseSampledMctsModel, carried_child, rebase, select
from oracle import OracleEnv
from test_mctsmodel import handmade, target_envs
from test_reference_policies import MODELS, load
from util import bits

C = 2 ** 0.5
NODE_FIELDS = ("parent", "reward", "value", "visits", "wsum", "terminal", "child", "prior")


def same(a, b):
    return bits(a).tobytes() == bits(b).tobytes()


def trained(name):
    """`evaluate` of mctsmodel.run_alone on the committed weights: log_softmax of the action head and the value head, f32."""
    _, _, w = load(name)

    def evaluate(envs):
        A = w["action_0_weight"].shape[0]
        logp, values = np.zeros((len(envs), A), dtype=F32), np.zeros(len(envs), dtype=F32)
        for i, env in enumerate(envs):
            if env is None:
                continue
            h = np.maximum(env.dense_obs().reshape(-1).astype(F32) @ w["embeddings_weight"].T + w["embeddings_bias"], 0)
            h = np.maximum(h @ w["common_0_weight"].T + w["common_0_bias"], 0)
            z = (h @ w["action_0_weight"].T + w["action_0_bias"]).astype(np.float64)
            logp[i] = (z - z.max() - np.log(np.exp(z - z.max()).sum())).astype(F32)
            values[i] = F32((h @ w["value_0_weight"].T + w["value_0_bias"])[0])
        return logp, values
    return evaluate


def trained_targets(name, count, difficulty, seed, max_depth):
    """`count` targets `difficulty` gates from solved and the identity, as oracle envs (the targets of test_gpu_mcts.golden_case)."""
    cfg, gateset, _ = load(name)
    kind, rng = MODELS[name], np.random.default_rng(seed)
    kw = dict(add_inverts=0, add_perms=0, depth_slope=cfg["depth_slope"], max_depth=max_depth)
    out = []
    for _ in range(count):
        src = OracleEnv(kind, cfg["num_qubits"], gateset, track_solution=0, difficulty=difficulty, **kw)
        src.reset_with(rng.integers(0, len(gateset), size=difficulty))
        env = OracleEnv(kind, cfg["num_qubits"], gateset, track_solution=1, **kw)
        env.set_state(src.get_state().tolist())
        out.append(env)
    out.append(OracleEnv(kind, cfg["num_qubits"], gateset, track_solution=1, **kw))
    return gateset, out


# The pinned search whose carried trees fill: no room beyond one decision's N + 1 nodes, a trained (peaked) policy, so the most visited
# child holds most of the tree and the next decision's simulations soon find it full.  tests/test_gpu_mcts_reuse.py runs the same case.
PINNED = dict(name="clifford_3q_custom", targets=11, difficulty=12, seed=1, max_depth=32, N=4)
PINNED_STATS = dict(refused=78, carried=2.6515151515151514)


def descend(f, m, start):
    """The descent of the selection rule from node `start` of tree m: (the node it ends on, the action of the unexpanded edge or None)."""
    x = start
    while True:
        if f.terminal[m, x]:
            return x, None
        a = best_action(scores(f, m, x, C))
        if a is None:
            return x, None
        c = int(f.child[m, x, a])
        if c < 0:
            return x, a
        x = c


def below(f, m, c):
    """The nodes under c by the child rows, c included: what the parent chains must agree with in a tree the rules built."""
    out, todo = [], [c]
    while todo:
        x = todo.pop()
        out.append(x)
        todo += [int(k) for k in f.child[m, x] if k >= 0]
    return sorted(out)


def check_rebase(before, after, move, finished, env_src, rng, seen):
    """`after` = `before` rebased under (move, finished), with env_src: every rule, and the rebased trees continued on both sides."""
    M, cap, A, none = before.M, before.cap, before.A, before.skip
    env_src = env_src.reshape(M, cap)
    maps = {}
    for m in range(M):
        n = int(before.n_nodes[m])
        c = None if finished[m] else carried_child(before, m, int(move[m]))
        if c is None:
            for name in FIELDS:
                assert same(getattr(after, name)[m], getattr(before, name)[m]), (m, name)
            want = np.full(cap, none) if finished[m] else np.where(np.arange(cap) < n, m * cap + np.arange(cap), none)
            np.testing.assert_array_equal(env_src[m], want)
            seen["untouched"] += 1
            continue
        assert c == before.child[m, 0, move[m]] and 0 < c < n
        kept = below(before, m, c)
        new = {j: i for i, j in enumerate(kept)}
        maps[m] = (c, new)
        assert after.n_nodes[m] == len(kept)
        np.testing.assert_array_equal(env_src[m], [m * cap + j for j in kept] + [none] * (cap - len(kept)))
        for j, i in new.items():
            for name in ("value", "visits", "terminal", "prior"):
                assert same(getattr(after, name)[m, i], getattr(before, name)[m, j]), (m, j, name)
            if i:
                assert same(after.reward[m, i], before.reward[m, j]) and same(after.wsum[m, i], before.wsum[m, j])
                assert after.parent[m, i] == new[int(before.parent[m, j])]
            else:
                assert after.parent[m, 0] == -1 and same(after.reward[m, 0], F32(0)) and same(after.wsum[m, 0], F32(0))
            assert after.child[m, i].tolist() == [new[int(k)] if k >= 0 else -1 for k in before.child[m, j]]
        seen["kept"] += len(kept)
        seen["dropped"] += n - len(kept)
        seen["one"] += len(kept) == 1
    live = np.array([m in maps for m in range(M)])
    check_invariants(_only(after, live))
    if not maps:
        return
    # the rebased tree is the subtree: the same descent, and after the same backup the same arrays
    old2, new2 = copy.deepcopy(before), copy.deepcopy(after)
    src, dst = np.zeros(M, dtype=np.int32), np.full(M, none, dtype=np.int32)
    act, leaf = np.full(M, A, dtype=np.int32), np.full(M, -1, dtype=np.int32)
    got = select(new2, C, ~live)
    for m, (c, new) in maps.items():
        x, a = descend(before, m, c)
        assert descend(after, m, 0) == (new[x], a)
        n, n2 = int(before.n_nodes[m]), int(after.n_nodes[m])
        if a is None:
            want = (m * cap + new[x], none, A, new[x])
            src[m], leaf[m] = m * cap + x, x
        elif n2 < cap:
            want = (m * cap + new[x], m * cap + n2, a, n2)
            if n < cap:
                src[m], dst[m], act[m], leaf[m] = m * cap + x, m * cap + n, a, n
        else:
            want = (m * cap + new[x], none, A, -1)
        assert tuple(int(g[m]) for g in got) == want, m
    prior = rng.dirichlet(np.ones(A), size=M).astype(F32)
    values, reward = rng.standard_normal(M).astype(F32), rng.random(M).astype(F32)
    done = rng.random(M) < 0.2
    backup(old2, src, dst, act, leaf, prior, values, reward, done)
    backup(new2, *got, prior, values, reward, done)
    rebase(old2, move, ~live)
    for m in maps:
        if leaf[m] < 0:  # the old tree was full: nothing to compare the new one's growth with
            continue
        k = int(new2.n_nodes[m])
        assert k == old2.n_nodes[m]
        for name in NODE_FIELDS:
            assert same(getattr(new2, name)[m, :k], getattr(old2, name)[m, :k]), (m, name)
        seen["continued"] += 1


def _only(f, rows):
    """The trees `rows` of f as a forest of their own."""
    rows = np.nonzero(rows)[0]
    g = Forest(len(rows), f.cap - 1, f.A)
    for name in FIELDS:
        setattr(g, name, getattr(f, name)[rows].copy())
    return g


def drive(model, evaluate, seen, rng):
    """`mctsreuse_model.run_alone`, with every rebase checked."""
    def priors(envs):
        logp, values = evaluate(envs)
        return np.exp(np.asarray(logp, dtype=F32)).astype(F32), np.asarray(values, dtype=F32)

    while not model.ended:
        if model.t == 0:
            model.start(*priors(model.roots()))
        for _ in range(model.N):
            model.select()
            model.backup(*priors(model.expand()))
        before = copy.deepcopy(model.forest)
        sizes = before.n_nodes.copy()
        move = model.decide()
        check_rebase(before, model.forest, move, model.finished, model.env_srcs[-1], rng, seen)
        for m in np.nonzero(~model.finished)[0]:  # a node's env is the one it had, under its new index
            assert sorted(model.pool[m]) == list(range(int(model.forest.n_nodes[m])))
        seen["full"] += int((sizes == before.cap).sum())
    return model.result()


def new_seen():
    return {k: 0 for k in ("untouched", "kept", "dropped", "one", "continued", "full")}


@pytest.mark.parametrize("sampled", [False, True], ids=["most-visited", "sampled"])
@pytest.mark.parametrize("N,cap", [(2, None), (9, None), (9, 10), (5, 61)])
@pytest.mark.parametrize("kind", ["linear_function", "clifford"])
def test_every_rebase_of_a_search_under_a_handmade_policy(kind, N, cap, sampled):
    gs, envs = target_envs(kind, 5, 11)
    A = len(gs)
    model = ReuseSampledMctsModel(envs, 2, N, A, 12, seed=5, cap=cap) if sampled else ReuseMctsModel(envs, N, A, 12, cap=cap)
    assert model.cap == (2 * N + 1 if cap is None else cap) == model.forest.cap
    seen = new_seen()
    sols, stats = drive(model, handmade(A), seen, np.random.default_rng(N))
    print(f"{kind} N={N} cap={model.cap} sampled={sampled}: {stats}; {seen}")
    assert seen["kept"] > 0 and seen["dropped"] > 0 and seen["untouched"] > 0
    assert seen["continued"] > 0 or cap == N + 1  # (there every tree is full at its decision: no room to grow the old one for the comparison)
    assert stats["reuse"] is True and stats["capacity"] == model.cap and stats["carried"] >= 1.0 and sols[-1] == []
    if cap == 61:  # 1 + 12 decisions of 5 simulations: a tree cannot fill
        assert stats["refused"] == 0 and seen["full"] == 0
    for env, sol in zip(envs, sols):
        if sol is not None:
            again = env.clone()
            for a in sol:
                assert not again.success()
                again.step(a)
            assert again.success()


@pytest.mark.parametrize("sampled", [False, True], ids=["most-visited", "sampled"])
def test_every_rebase_of_a_search_under_the_trained_policy(sampled):
    gs, envs = trained_targets("clifford_3q_custom", 5, 12, 2, 24)
    A = len(gs)
    model = ReuseSampledMctsModel(envs, 2, 6, A, 24, seed=3) if sampled else ReuseMctsModel(envs, 6, A, 24)
    seen = new_seen()
    sols, stats = drive(model, trained("clifford_3q_custom"), seen, np.random.default_rng(8))
    print(f"trained, sampled={sampled}: {stats}; {seen}")
    assert seen["kept"] > 0 and seen["dropped"] > 0 and seen["continued"] > 0
    if not sampled:  # a peaked policy: most of the tree is under the most visited move (a drawn move may be any visited one)
        assert seen["kept"] > seen["dropped"] and stats["carried"] > 2.0
    assert stats["solved"] >= 2 and sols[-1] == []


def test_the_pinned_search_whose_carried_trees_fill():
    p = PINNED
    gs, envs = trained_targets(p["name"], p["targets"], p["difficulty"], p["seed"], p["max_depth"])
    model = ReuseMctsModel(envs, p["N"], len(gs), p["max_depth"], cap=p["N"] + 1)
    seen = new_seen()
    sols, stats = drive(model, trained(p["name"]), seen, np.random.default_rng(1))
    print(f"pinned: {stats}; {seen}")
    assert stats["capacity"] == p["N"] + 1 and seen["full"] > 0
    assert {k: stats[k] for k in PINNED_STATS} == PINNED_STATS
    uniform = ReuseMctsModel(envs, p["N"], len(gs), p["max_depth"], cap=p["N"] + 1)
    _, flat = drive(uniform, lambda e: (np.full((len(e), len(gs)), -np.log(len(gs)), dtype=F32), np.zeros(len(e), dtype=F32)), new_seen(),
                    np.random.default_rng(1))
    assert flat["carried"] < stats["carried"]  # uniform priors spread the simulations over the root's edges: little is carried


def corner_forests():
    """Forests written by hand, cap 8 over 3 actions, every number of a node its own, with what the rules give: (forest, move, finished,
    per tree the kept old nodes in order -- None: the forest is untouched -- and the env_src row as node indices, -1 for none)."""
    shape = {1: (0, 0), 2: (0, 1), 3: (1, 0), 4: (2, 0), 5: (1, 1), 6: (3, 2)}  # node: (parent, action)
    star = {1: (0, 0), 2: (0, 1), 3: (0, 2)}
    cases = [  # (nodes, move, finished, what is broken, kept, env_src row)
        (shape, 0, 0, None, [1, 3, 5, 6], [1, 3, 5, 6]),  # kept and dropped nodes interleaved
        (shape, 3, 0, None, None, [0, 1, 2, 3, 4, 5, 6]),  # move = A
        (shape, 2, 0, None, None, [0, 1, 2, 3, 4, 5, 6]),  # an unexpanded edge
        (shape, 0, 1, None, None, []),  # the real env is final
        (shape, 1, 0, None, [2, 4], [2, 4]),
        (star, 2, 0, None, [3], [3]),  # c is the last node
        (shape, 0, 0, "parent[5] = 5", [1, 3, 6], [1, 3, 6]),  # a link that does not descend
        (shape, 0, 0, "children outside", [1, 3, 5, 6], [1, 3, 5, 6]),
        (shape, 0, 0, "n_nodes = 9", None, [0, 1, 2, 3, 4, 5, 6, 7]),  # above cap: the identity, clamped
        (shape, 0, 0, "n_nodes = 0", None, []),
        (shape, 0, 0, "parent[3] = -5", [1, 5], [1, 5]),  # the chain of 6 breaks at 3
        (shape, 1, 0, "parent[4] = 1", [2], [2]),  # a chain that passes below c
        (shape, -1, 0, None, None, [0, 1, 2, 3, 4, 5, 6]),  # a move below 0
        (shape, 0, 0, "child[0][0] = 0", None, [0, 1, 2, 3, 4, 5, 6]),  # the root is no child of itself
    ]
    M, cap, A = len(cases), 8, 3
    rng = np.random.default_rng(21)
    f = Forest(M, cap - 1, A)
    f.reward[:], f.value[:], f.wsum[:] = (rng.standard_normal((M, cap)).astype(F32) for _ in range(3))
    f.visits[:] = rng.integers(1, 90, size=(M, cap))
    f.terminal[:] = rng.integers(0, 2, size=(M, cap))
    f.prior[:] = rng.random((M, cap, A)).astype(F32)
    f.child[:] = -1
    f.parent[:] = -1
    move, finished = np.zeros(M, dtype=np.int32), np.zeros(M, dtype=np.uint8)
    for m, (nodes, mv, fin, broken, _, _) in enumerate(cases):
        for j, (p, a) in nodes.items():
            f.parent[m, j], f.child[m, p, a] = p, j
        f.n_nodes[m], move[m], finished[m] = 1 + len(nodes), mv, fin
        if broken == "parent[5] = 5":
            f.parent[m, 5] = 5
        elif broken == "children outside":
            f.child[m, 3, 1], f.child[m, 1, 2], f.child[m, 5, 0] = 7, 100, -3
        elif broken == "n_nodes = 9":
            f.n_nodes[m] = 9
        elif broken == "n_nodes = 0":
            f.n_nodes[m] = 0
        elif broken == "parent[3] = -5":
            f.parent[m, 3] = -5
        elif broken == "parent[4] = 1":
            f.parent[m, 4] = 1
        elif broken == "child[0][0] = 0":
            f.child[m, 0, 0] = 0
    return f, move, finished, [(kept, row) for *_, kept, row in cases]


def test_corner_cases_by_hand():
    f, move, finished, want = corner_forests()
    before = copy.deepcopy(f)
    env_src = rebase(f, move, finished).reshape(f.M, f.cap)
    for m, (kept, row) in enumerate(want):
        np.testing.assert_array_equal(env_src[m], [m * f.cap + j for j in row] + [f.skip] * (f.cap - len(row)), err_msg=str(m))
        if kept is None:
            for name in FIELDS:
                assert same(getattr(f, name)[m], getattr(before, name)[m]), (m, name)
            continue
        assert f.n_nodes[m] == len(kept), m
        new = {j: i for i, j in enumerate(kept)}
        for j, i in new.items():
            for name in ("value", "visits", "terminal", "prior"):
                assert same(getattr(f, name)[m, i], getattr(before, name)[m, j]), (m, j, name)
            assert f.parent[m, i] == (new[int(before.parent[m, j])] if i else -1)
            assert same(f.reward[m, i], before.reward[m, j] if i else F32(0)) and same(f.wsum[m, i], before.wsum[m, j] if i else F32(0))
            assert f.child[m, i].tolist() == [new.get(int(k), -1) for k in before.child[m, j]], (m, j)
    assert f.child[6, 0].tolist() == [1, -1, -1]  # old 1: 3 is kept, 5 is not
    assert f.child[7, 0].tolist() == [1, 2, -1] and f.child[7, 1].tolist() == [-1, -1, 3] and f.child[7, 2].tolist() == [-1, -1, -1]  # 100, 7, -3: no nodes
    # without a `finished` array every tree is live
    g = copy.deepcopy(before)
    assert rebase(g, move).reshape(g.M, g.cap)[3].tolist()[:4] == [3 * g.cap + j for j in (1, 3, 5, 6)] and g.n_nodes[3] == 4


def test_the_kept_nodes_without_the_walks_are_those_of_the_walks():
    """`rebase` settles a node by its parent's answer; the rule walks every chain.  The same nodes on the corner cases (broken links, chains
    that pass below c), on random trees under every child of the root, on chains, and on parents drawn without any rule."""
    from mctsreuse_model import kept_nodes, kept_nodes_by_walk

    compared = 0
    corners, move, _, _ = corner_forests()
    wild = random_forest(3, 200, 4, 180, 5)
    wild.parent[:, 1:] = np.random.default_rng(6).integers(-3, 200, size=(3, 199))
    for f, moves in ((corners, [int(a) for a in move]), (random_forest(3, 300, 7, 280, 2), None), (chain_forest(2, 70, 70), None), (wild, None)):
        for m in range(f.M):
            for a in range(f.A) if moves is None else [moves[m]]:
                c = carried_child(f, m, a)
                if c is not None:
                    assert kept_nodes(f, m, c) == kept_nodes_by_walk(f, m, c), (m, a)
                    compared += 1
    assert compared > 20


def chain_forest(M, cap, n):
    """A = 1: every tree is a chain of n nodes."""
    f = Forest(M, cap - 1, 1)
    rng = np.random.default_rng(cap)
    root(f, np.ones((M, 1), dtype=F32), rng.standard_normal(M).astype(F32))
    for s in range(n - 1):
        picked = select(f, C)
        assert (picked[3] == s + 1).all()
        backup(f, *picked, np.ones((M, 1), dtype=F32), rng.standard_normal(M).astype(F32), rng.random(M).astype(F32), np.zeros(M, dtype=bool))
    return f


def test_a_chain_keeps_everything_but_the_root():
    f = chain_forest(3, 130, 130)
    picked = select(f, C)
    assert (picked[3] == -1).all() and (picked[2] == 1).all() and (picked[0] == np.arange(3) * 130 + 129).all()  # full: refused at the last node
    before = copy.deepcopy(f)
    env_src = rebase(f, np.zeros(3, dtype=np.int32)).reshape(3, 130)
    assert f.n_nodes.tolist() == [129] * 3  # c = 1 with every other node below it
    for m in range(3):
        assert env_src[m].tolist() == [m * 130 + j for j in range(1, 130)] + [f.skip]
        assert f.parent[m, :129].tolist() == list(range(-1, 128)) and f.child[m, :129, 0].tolist() == list(range(1, 129)) + [-1]
        assert same(f.visits[m, :129], before.visits[m, 1:]) and same(f.value[m, :129], before.value[m, 1:])
        assert same(f.wsum[m, 1:129], before.wsum[m, 2:]) and f.wsum[m, 0] == 0 and f.visits[m, 0] == 129
    check_invariants(f)


def random_forest(M, cap, A, n, seed):
    """Trees of n nodes in which node j hangs under a node drawn from all those before it: the subtree of an early node is spread over the
    whole index range, kept and dropped nodes interleaved.  Every number of a node is its own; leaves are terminal at random."""
    rng = np.random.default_rng(seed)
    f = Forest(M, cap - 1, A)
    f.reward[:], f.value[:], f.wsum[:] = (rng.standard_normal((M, cap)).astype(F32) for _ in range(3))
    f.visits[:] = rng.integers(1, 50, size=(M, cap))
    f.prior[:] = rng.random((M, cap, A)).astype(F32)
    f.child[:] = -1
    f.parent[:] = -1
    f.terminal[:] = rng.random((M, cap)) < 0.3
    for m in range(M):
        for j in range(1, n):
            while True:
                p = int(rng.integers(0, j))
                free = np.nonzero(f.child[m, p] < 0)[0]
                if len(free):
                    break
            f.child[m, p, rng.choice(free)], f.parent[m, j], f.terminal[m, p] = j, p, 0
        for j in range(n - 1, -1, -1):  # visits as the backup rule leaves them: 1 + the children's, a terminal leaf's any
            kids = f.child[m, j][f.child[m, j] >= 0]
            f.visits[m, j] = rng.integers(1, 6) if f.terminal[m, j] else 1 + int(f.visits[m, kids].sum())
    f.value[f.terminal != 0] = 0
    f.reward[:, 0], f.wsum[:, 0] = 0, 0
    f.n_nodes[:] = n
    return f


def interleaving(kept):
    """Do the kept old nodes, and the dropped ones between them, each lie in more than one slice of 64 nodes?"""
    kept = np.asarray(kept)
    gaps = np.setdiff1d(np.arange(kept[0], kept[-1] + 1), kept)
    return len(set((kept // 64).tolist())) > 1 and len(set((gaps // 64).tolist())) > 1


@pytest.mark.parametrize("M,cap,A,n", [(3, 130, 5, 129), (2, 300, 256, 280), (4, 20, 2, 17)])
def test_random_trees_kept_and_dropped_nodes_interleaved(M, cap, A, n):
    before = random_forest(M, cap, A, n, cap + A)
    move = np.array([int(np.nonzero(before.child[m, 0] == 1)[0][0]) for m in range(M)], dtype=np.int32)  # the edge to node 1
    after = copy.deepcopy(before)
    env_src = rebase(after, move)
    seen = new_seen()
    check_rebase(before, after, move, np.zeros(M, dtype=bool), env_src, np.random.default_rng(3), seen)
    assert seen["kept"] > M and seen["dropped"] > M and seen["continued"] > 0
    if cap > 64:
        assert all(interleaving(env_src[m * cap : m * cap + after.n_nodes[m]] - m * cap) for m in range(M))
