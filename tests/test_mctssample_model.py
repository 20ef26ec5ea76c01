"""The CPU model of the sampled tree search (tests/mctssample_model.py) on its own.  `collector.mcts_decide` and
`BatchedSynthesis.solve(mcts_sampled=True)` are held to this model bit for bit (tests/test_gpu_mcts_decide.py, tests/test_gpu_mcts_sampled.py),
so the model's own rules are checked here: the draw against the distribution it claims, the draw's edges by hand, and the whole search on
oracle envs with a hand-written prior / value function."""
import numpy as np
import pytest

from collect_ref import chi2_quantile
from mctsmodel import F32, Forest, check_invariants, root, run_alone
from mctssample_model import MASK64, STREAM, SampledMctsModel, counts, decide_most, decide_sampled, draw_from
from test_mctsmodel import handmade, target_envs
from util import rng_draw


def forest_of(rows, N=None):
    """A forest whose tree m has the root's visit counts rows[m] (0: no child)."""
    rows = np.asarray(rows, dtype=np.int64)
    M, A = rows.shape
    f = Forest(M, A if N is None else N, A)
    root(f, np.full((M, A), 1.0 / A, dtype=F32), np.zeros(M, dtype=F32))
    for m in range(M):
        n = 1
        for a in range(A):
            if rows[m, a] > 0:
                f.child[m, 0, a], f.parent[m, n], f.visits[m, n] = n, 0, rows[m, a]
                f.child[m, n] = -1
                n += 1
        f.n_nodes[m], f.visits[m, 0] = n, min(1 + int(rows[m].sum()), 2 ** 31 - 1)
    return f


@pytest.mark.parametrize("seed", [0, 1, 12345])
def test_draws_follow_the_visit_counts(seed):
    row = [5, 0, 3, 1, 0, 7, 0, 0, 2, 1]
    trees, counters = 400, 50
    f = forest_of([row] * trees)
    assert (counts(f) == np.array(row)).all()
    seen = np.zeros(len(row), dtype=np.int64)
    for t in range(counters):
        seen += np.bincount(decide_sampled(f, seed, t), minlength=len(row))
    assert seen.sum() == trees * counters == 20000
    assert (seen[np.array(row) == 0] == 0).all()  # no draw lands on an action without visits
    nz = np.array(row) > 0
    expect = np.array(row)[nz] * (seen.sum() / sum(row))
    chi2 = float(((seen[nz] - expect) ** 2 / expect).sum())
    print(f"seed {seed}: chi-square {chi2:.1f} over {int(nz.sum())} actions, bound {chi2_quantile(5):.2f}")
    assert nz.sum() == 6 and chi2 < chi2_quantile(5)


def test_the_draw_by_hand():
    top = (1 << 64) - 1
    assert draw_from([0, 0, 1, 0], 0) == 2 and draw_from([0, 0, 1, 0], top) == 2  # total = 1: r = 0 whatever the draw
    assert draw_from([9, 0, 0], top) == 0 and draw_from([0, 0, 9], 0) == 2  # all mass on action 0, on action A - 1
    assert draw_from([0, 0, 0], 5) is None
    # counts [2, 3, 1]: r = 0, 1 -> action 0; r = 2, 3, 4 -> action 1; r = 5 -> action 2.  r = (d * 6) >> 64: d = ceil(r * 2^64 / 6) is the
    # first draw that gives r, the one before it the last that gives r - 1
    row = [2, 3, 1]
    for r, a in enumerate([0, 0, 1, 1, 1, 2]):
        first = -((-r << 64) // 6)
        assert draw_from(row, first) == a and (first * 6) >> 64 == r
        if r:
            assert ((first - 1) * 6) >> 64 == r - 1 and draw_from(row, first - 1) == [0, 0, 1, 1, 1, 2][r - 1]
    assert draw_from(row, top) == 2
    # the model's draw is that function on the counter RNG's number, per tree index
    f = forest_of([row, [0, 0, 4], [0, 0, 0], [1, 1, 1]])
    for seed, counter in ((0, 0), (7, 3), (2 ** 63 + 5, 2 ** 40)):
        d = rng_draw((seed ^ STREAM) & MASK64, np.arange(4, dtype=np.uint64), counter)
        got = decide_sampled(f, seed, counter)
        assert got.tolist() == [draw_from(row, int(d[0])), 2, 3, draw_from([1, 1, 1], int(d[3]))]  # no child: A
        assert decide_sampled(f, seed, counter, np.array([0, 1, 0, 1])).tolist() == [got[0], 3, 3, 3]
    assert decide_most(f).tolist() == [1, 2, 3, 0]


def test_a_forest_the_rules_refuse_has_no_move_and_no_counts():
    f = forest_of([[2, 0, 1], [2, 0, 1], [2, 0, 1], [2, 0, 1], [1, 1, 0]])
    f.child[0, 0, 1] = 3  # n_nodes is 3: no node of the tree
    f.child[1, 0, 1] = 0  # the root is no child of itself
    f.n_nodes[2] = 0
    f.visits[3, 1] = -1
    assert counts(f).tolist() == [[0, 0, 0]] * 4 + [[1, 1, 0]]
    assert decide_most(f).tolist() == [3, 3, 3, 3, 0]
    assert decide_sampled(f, 0, 0)[:4].tolist() == [3, 3, 3, 3]


@pytest.mark.parametrize("S,N", [(1, 3), (3, 4)])
def test_the_model_alone_on_oracle_envs(S, N):
    gs, envs = target_envs("linear_function", 4, 11)
    A = len(gs)
    model = SampledMctsModel(envs, S, N, A, 12, seed=5)
    assert model.M == len(envs) * S
    seen = {"sims": 0}

    def after(model):
        seen["sims"] += 1
        check_invariants(model.forest, model.sims)
        assert (model.sims[model.finished] == 0).all()

    sols, stats = run_alone(model, handmade(A), after)
    assert seen["sims"] == stats["steps"] * N
    assert sols[-1] == [] and len(sols) == len(envs)  # solved on arrival: every one of its searches answers []
    assert model.winners()[-1] == 0 and (model.ret[-S:] == 0).all()  # S successful searches of equal return: the lowest s
    assert stats["searches"] == S and stats["targets"] == len(envs) and stats["solved"] == sum(s is not None for s in sols) >= 1
    assert 1 / (len(envs) * S) <= stats["searches_solved"] <= 1.0
    for m, (env, sol) in enumerate(zip(envs, sols)):
        if sol is not None:
            again = env.clone()
            for a in sol:
                assert not again.success()
                again.step(a)
            assert again.success()
    again = SampledMctsModel(envs, S, N, A, 12, seed=5)
    assert run_alone(again, handmade(A)) == (sols, stats)  # the same seed repeats the search
    other = SampledMctsModel(envs, S, N, A, 12, seed=6)
    run_alone(other, handmade(A))
    assert any((a != b).any() for a, b in zip(model.moves, other.moves)) or len(model.moves) != len(other.moves)


def test_equal_returns_go_to_the_lowest_search():
    gs, envs = target_envs("linear_function", 1, 3)
    model = SampledMctsModel(envs, 4, 2, len(gs), 12)
    assert model.pick(np.array([False, True, True, True]), np.array([9.0, 1.5, 1.5, 1.0], dtype=F32)) == 1  # two successes of equal return
    assert model.pick(np.array([False, True, True, True]), np.array([9.0, 1.0, 1.5, 1.5], dtype=F32)) == 2
    assert model.pick(np.array([False, False, False, False]), np.zeros(4, dtype=F32)) is None
