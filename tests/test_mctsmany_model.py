"""tests/mctsmany_model.py against the one-descent models and against its own rules, on the CPU: random forests and hand-built corner
trees for `select_many` / `backup_many`, whole searches on oracle envs for the model classes."""
import copy

import numpy as np
import pytest

from mctsmany_model import (ManyMctsModel, ManyReuseMctsModel, ManyReuseSampledMctsModel, ManySampledMctsModel, backup_many, run_alone, select_many)
from mctsmodel import F32, FIELDS, Forest, MctsModel, backup, check_invariants, root
from mctsmodel import run_alone as run_one
from mctsreuse_model import select
from test_mctsmodel import handmade, target_envs
from test_mctsreuse_model import random_forest, same

C = 2 ** 0.5


def results(rng, rows, A, quantised=True):
    """Stand-ins for the expanded envs' priors, values, rewards and terminal flags."""
    prior = (rng.integers(0, 4, size=(rows, A)) / F32(4 * A)).astype(F32) if quantised else rng.dirichlet(np.ones(A), size=rows).astype(F32)
    values, reward = (rng.integers(-2, 5, size=rows) / 4.0).astype(F32), (rng.integers(-2, 5, size=rows) / 4.0).astype(F32)
    return prior, values, reward, rng.random(rows) < 0.2


def stalls_of(f, k, stride, act, leaf):
    """The (tree, node) of every counted descent that found no candidate on a node that is not terminal: such a simulation adds a visit to
    the node and its ancestors and to no child, which the one-descent search never does (there a candidate always exists)."""
    out = []
    for e in range(f.M * stride):
        if e % stride < k and leaf[e] >= 0 and act[e] == f.A and not f.terminal[e // stride, leaf[e]]:
            out.append((e // stride, int(leaf[e])))
    return out


def invariants(f, sims=None, stalls=()):
    """`mctsmodel.check_invariants` with the visits of `stalls` taken back along their paths."""
    g = copy.deepcopy(f)
    sims = None if sims is None else np.array(sims, dtype=np.int64)
    for m, x in stalls:
        y = x
        while y >= 0:
            g.visits[m, y] -= 1
            y = int(g.parent[m, y])
        if sims is not None:
            sims[m] -= 1
    check_invariants(g, sims)


def loose_invariants(f):
    """What holds of a carried tree whatever stalled in it: the structure, and no node with fewer visits than 1 + its children's."""
    for m in range(f.M):
        n = int(f.n_nodes[m])
        assert 1 <= n <= f.cap
        for x in range(n):
            kids = [int(c) for c in f.child[m, x] if c >= 0]
            assert all(x < c < n and f.parent[m, c] == x for c in kids) and len(set(kids)) == len(kids)
            assert f.terminal[m, x] and not kids or f.visits[m, x] >= 1 + sum(int(f.visits[m, c]) for c in kids), (m, x)


def equal_forests(f, g):
    return all(same(getattr(f, name), getattr(g, name)) for name in FIELDS)


@pytest.mark.parametrize("vl", [0.0, 0.5])
@pytest.mark.parametrize("M,cap,A,n", [(4, 20, 2, 17), (3, 40, 5, 33), (2, 12, 70, 12)])
def test_one_descent_is_the_one_descent_models(M, cap, A, n, vl):
    f = random_forest(M, cap, A, n, cap + A)
    g = copy.deepcopy(f)
    finished = np.zeros(M, dtype=bool)
    finished[M - 1] = True
    rng = np.random.default_rng(n)
    counted = refused = 0
    for s in range(6):
        want = select(g, C, finished)
        got = select_many(f, C, 1, 1, vl, finished)
        for name, a, b in zip(("src", "dst", "act", "leaf"), got, want):
            np.testing.assert_array_equal(a, b, err_msg=f"simulation {s}: {name}")
        prior, values, reward, done = results(rng, M, A)
        backup(g, *want, prior, values, reward, done)
        backup_many(f, 1, 1, *got, prior, values, reward, done)
        assert equal_forests(f, g), s
        counted += int((want[3] >= 0).sum())
        refused += int(((want[3] < 0) & ~finished).sum())
    assert (counted > 0 or n == cap) and (refused > 0) == (n + 6 > cap)  # six simulations: do the trees fill?


@pytest.mark.parametrize("vl", [0.0, 0.5])
@pytest.mark.parametrize("M,cap,A,n,k,stride", [(4, 40, 3, 17, 8, 8), (3, 64, 5, 33, 3, 5), (2, 130, 70, 60, 64, 64), (3, 20, 2, 17, 7, 64)])
def test_rounds_on_random_forests(M, cap, A, n, k, stride, vl):
    f = random_forest(M, cap, A, n, cap + A + k)
    finished = np.zeros(M, dtype=bool)
    finished[M - 1] = True
    rng = np.random.default_rng(k)
    several = full = 0
    stalls = []
    for r in range(4):
        before, overlays = copy.deepcopy(f), []
        src, dst, act, leaf = (t.reshape(M, stride) for t in select_many(f, C, k, stride, vl, finished, overlays))
        assert equal_forests(f, before)  # the selection writes nothing
        assert (leaf[:, k:] == -1).all() and (act[:, k:] == A).all() and (dst[:, k:] == f.skip).all() and (src[:, k:] == np.arange(M)[:, None] * cap).all()
        assert (leaf[M - 1] == -1).all() and overlays[M - 1] is None
        for m in range(M - 1):
            n0 = int(before.n_nodes[m])
            grown = act[m] < A
            edges = [(int(s), int(a)) for s, a in zip(src[m][grown], act[m][grown])]
            assert len(set(edges)) == len(edges), "no two descents of a call expand the same edge"
            assert dst[m][grown].tolist() == [m * cap + n0 + e for e in range(int(grown.sum()))]  # numbered in order, no two alike
            assert (leaf[m][grown] == dst[m][grown] - m * cap).all() and (src[m] - m * cap < n0).all()  # no descent stands on a node that is not there
            several += int(grown.sum()) >= 2
            full += int(((leaf[m, :k] < 0)).sum())
        prior, values, reward, done = results(rng, M * stride, A, quantised=r % 2 == 0)
        linked = backup_many(f, k, stride, src.reshape(-1), dst.reshape(-1), act.reshape(-1), leaf.reshape(-1), prior, values, reward, done)
        np.testing.assert_array_equal(f.n_nodes - before.n_nodes, linked)
        np.testing.assert_array_equal(linked, (act < A).sum(axis=1))
        for m in range(M - 1):
            n0 = int(before.n_nodes[m])
            if (leaf[m, :k] >= 0).all():  # (a descent refused for a full tree leaves virtual visits and no real ones)
                np.testing.assert_array_equal(f.visits[m, :n0], overlays[m][:n0], err_msg=f"round {r}: the old nodes' visits are the overlay's")
            assert f.visits[m, 0] == before.visits[m, 0] + int((leaf[m, :k] >= 0).sum())
        for name in FIELDS:
            assert same(getattr(f, name)[M - 1], getattr(before, name)[M - 1])  # the finished tree
        stalls += stalls_of(f, k, stride, act.reshape(-1), leaf.reshape(-1))
        invariants(f, None, stalls)
    assert several > 0
    if cap - n < 4 * k:
        assert full > 0


def open_single_node(A, cap, prior):
    f = Forest(1, cap - 1, A)
    root(f, np.asarray([prior], dtype=F32), np.asarray([0.25], dtype=F32))
    return f


def test_room_for_one_node():
    """k = 3 on a tree with room for one node: one is linked, the others are refused unless they end on a terminal node."""
    A = 4
    for seed in range(6):
        f = random_forest(1, 18, A, 17, seed)
        src, dst, act, leaf = select_many(f, C, 3, 3, 0.5)
        grown = act < A
        ends_terminal = np.array([lf >= 0 and not g and f.terminal[0, lf] for lf, g in zip(leaf, grown)])
        assert grown.sum() <= 1 and ((leaf < 0) | grown | ends_terminal).all()
        if grown.any():
            first = int(np.nonzero(grown)[0][0])
            assert leaf[first] == 17 and all(leaf[i] < 0 or ends_terminal[i] for i in range(first + 1, 3))
        n_before = int(f.n_nodes[0])
        prior, values, reward, done = results(np.random.default_rng(seed), 3, A)
        backup_many(f, 3, 3, src, dst, act, leaf, prior, values, reward, done)
        assert f.n_nodes[0] == n_before + int(grown.sum()) <= 18
    f = random_forest(1, 18, A, 17, 1)
    f.terminal[:] = 0  # no terminal node: one expansion, two refusals
    src, dst, act, leaf = select_many(f, C, 3, 3, 0.0)
    assert leaf.tolist() == [17, -1, -1] and act[1:].tolist() == [A, A] and dst[1:].tolist() == [f.skip, f.skip]


def test_a_single_node_tree_runs_out_of_candidates():
    """A = 3, k = 5: three edges are expanded, then two simulations find no candidate and count on the root."""
    f = open_single_node(3, 9, [0.5, 0.25, 0.25])
    src, dst, act, leaf = select_many(f, C, 5, 5, 0.0)
    assert act.tolist() == [0, 1, 2, 3, 3] and leaf.tolist() == [1, 2, 3, 0, 0] and dst.tolist() == [1, 2, 3, 9, 9] and src.tolist() == [0] * 5
    prior, values, reward, done = results(np.random.default_rng(0), 5, 3)
    backup_many(f, 5, 5, src, dst, act, leaf, prior, values, reward, np.zeros(5, dtype=bool))
    assert f.n_nodes[0] == 4 and f.visits[0, 0] == 6 and f.visits[0, 1:4].tolist() == [1, 1, 1] and f.child[0, 0].tolist() == [1, 2, 3]
    invariants(f, [5], [(0, 0), (0, 0)])


def test_two_descents_that_end_on_the_same_terminal_node_both_count():
    f = open_single_node(1, 9, [1.0])
    one = select_many(f, C, 1, 2)
    backup_many(f, 1, 2, *one, np.ones((2, 1), dtype=F32), np.zeros(2, dtype=F32), np.full(2, 0.5, dtype=F32), np.array([True, True]))
    assert f.n_nodes[0] == 2 and f.terminal[0, 1] == 1
    src, dst, act, leaf = select_many(f, C, 2, 2, 0.5)
    assert leaf.tolist() == [1, 1] and act.tolist() == [1, 1] and src.tolist() == [1, 1] and dst.tolist() == [9, 9]
    backup_many(f, 2, 2, src, dst, act, leaf, np.ones((2, 1), dtype=F32), np.zeros(2, dtype=F32), np.zeros(2, dtype=F32), np.zeros(2, dtype=bool))
    assert f.visits[0, 1] == 3 and f.visits[0, 0] == 4 and f.wsum[0, 1] == F32(1.5)


def test_a_failed_range_check_ends_the_trees_work():
    f = random_forest(2, 20, 3, 10, 4)
    f.terminal[:] = 0
    f.child[0, 0, 1] = 15  # outside the tree
    before = copy.deepcopy(f)
    src, dst, act, leaf = (t.reshape(2, 4) for t in select_many(f, C, 3, 4))
    assert (leaf[0] == -1).all() and (act[0] == 3).all() and (dst[0] == f.skip).all() and (src[0] == 0).all() and (leaf[1, :3] >= 0).all()
    f.n_nodes[1] = 21
    got = select_many(f, C, 3, 4)
    assert (got[3] == -1).all()
    backup_many(f, 3, 4, *got, *results(np.random.default_rng(1), 8, 3))
    f.n_nodes[1] = 10
    assert equal_forests(f, before)
    # a backup whose entry fails a check skips it; the later expansion then names a node that is not n_nodes and is skipped by itself
    src, dst, act, leaf = select_many(before, C, 3, 4)
    assert (act.reshape(2, 4)[1, :3] < 3).all()
    src[4] = -1
    g = copy.deepcopy(before)
    backup_many(g, 3, 4, src, dst, act, leaf, *results(np.random.default_rng(1), 8, 3))
    assert g.n_nodes[1] == 10 and same(g.visits[1], before.visits[1])


@pytest.mark.parametrize("vl", [0.0, 0.5])
@pytest.mark.parametrize("N,K", [(6, 4), (9, 9), (5, 2)])
@pytest.mark.parametrize("kind", ["linear_function", "clifford"])
def test_searches_in_rounds_keep_the_invariants(kind, N, K, vl):
    gs, envs = target_envs(kind, 4, 11)
    A = len(gs)
    for cls, args, kw in ((ManyMctsModel, (envs, N, A, 12), {}), (ManySampledMctsModel, (envs, 2, N, A, 12), dict(seed=5)),
                          (ManyReuseMctsModel, (envs, N, A, 12), {}), (ManyReuseSampledMctsModel, (envs, 2, N, A, 12), dict(seed=5, cap=N + 1))):
        model = cls(*args, leaves=K, virtual_loss=vl, **kw)
        seen = {"rounds": 0, "stalls": []}

        def after_round(mdl):
            seen["rounds"] += 1
            f = mdl.forest
            if hasattr(mdl, "refused"):  # carried trees: the nodes are renumbered between decisions
                return loose_invariants(f)
            if mdl.round == 1:  # the trees are new
                seen["stalls"] = []
            seen["stalls"] += stalls_of(f, mdl.per_round[-1], mdl.K, mdl.picked[2], mdl.picked[3])
            invariants(f, np.where(~mdl.finished, mdl.sims, 0), seen["stalls"])

        sols, stats = run_alone(model, handmade(A), after_round)
        assert stats["leaves"] == K and stats["rounds"] == -(-N // K) and seen["rounds"] == stats["steps"] * stats["rounds"]
        assert set(model.per_round) == {min(K, N - r * K) for r in range(stats["rounds"])}
        assert sols[-1] == [] and stats["idle"] >= 0
        if "refused" in stats:
            assert stats["refused"] == stats["idle"]
        else:
            assert stats["idle"] == 0  # cap = N + 1 and at most N descents per decision: never full
        for env, sol in zip(envs, sols):
            if sol is not None:
                again = env.clone()
                for a in sol:
                    again.step(a)
                assert again.success()


def test_one_leaf_per_round_is_the_search_as_it_was():
    gs, envs = target_envs("clifford", 4, 11)
    A = len(gs)
    want = run_one(MctsModel(envs, 5, A, 12), handmade(A))
    for vl in (0.0, 0.5):
        sols, stats = run_alone(ManyMctsModel(envs, 5, A, 12, leaves=1, virtual_loss=vl), handmade(A))
        assert sols == want[0] and all(stats[k] == v for k, v in want[1].items()) and stats["rounds"] == 5
