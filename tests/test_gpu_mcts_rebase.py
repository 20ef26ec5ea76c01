"""`collector.mcts_rebase` against the CPU model of tests/mctsreuse_model.py, bit for bit, on forests the test drives itself with the
`Device` / `Data` scheme of tests/test_gpu_mcts_kernels.py: decisions of driven simulations, a rebase on device and model, further
simulations on the rebased trees and a second rebase -- so `mcts_select`, `mcts_backup` and `mcts_decide` are shown to accept rebased
trees -- then the corner cases and hand-broken forests of tests/test_mctsreuse_model.py, a captured rebase + `copy_envs` pair, the
argument checks and `mcts_forest(cap=...)`.  A rebased tree is compared on the nodes below its new n_nodes (the entries past them mean
nothing), an untouched tree in full, `env_src` in full."""
import ctypes

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")

from mctsmodel import FIELDS, Forest, backup, check_invariants, root  # noqa: E402
from mctsreuse_model import carried_child, rebase, select  # noqa: E402
from mctssample_model import decide_most, decide_sampled  # noqa: E402
from test_gpu_mcts_kernels import C, Data, Device, bits  # noqa: E402
from test_mctsreuse_model import chain_forest, corner_forests, interleaving, random_forest  # noqa: E402

NODE_FIELDS = ("parent", "reward", "value", "visits", "wsum", "terminal", "child", "prior")


def expect_rebased(dev, model, touched, label):
    """Device forest against the model's: tree m on its nodes below n_nodes where `touched[m]`, in full elsewhere."""
    torch.cuda.synchronize()
    np.testing.assert_array_equal(dev.n_nodes.cpu().numpy(), model.n_nodes, err_msg=f"{label}: n_nodes")
    for name in NODE_FIELDS:
        got, want = getattr(dev, name).cpu().numpy(), getattr(model, name)
        assert got.dtype == want.dtype and got.shape == want.shape, (label, name)
        for m in range(model.M):
            k = int(model.n_nodes[m]) if touched[m] else model.cap
            assert bits(got[m, :k]).tobytes() == bits(want[m, :k]).tobytes(), f"{label}: {name} of tree {m}"


def upload(model):
    from qiskit_gym_amd.collector import mcts_forest

    dev = mcts_forest(model.M, 1, model.A, "cuda", cap=model.cap)
    for name in FIELDS:
        getattr(dev, name).copy_(torch.as_tensor(getattr(model, name)))
    return dev


def rebase_both(dev, model, move, finished, label):
    """One rebase on the device forest and on the model; compares and returns env_src."""
    from qiskit_gym_amd.collector import mcts_rebase

    touched = [not (finished is not None and finished[m]) and carried_child(model, m, int(move[m])) is not None for m in range(model.M)]
    env_src = torch.full((model.M * model.cap,), -7, dtype=torch.int32, device="cuda")
    out = mcts_rebase(dev, torch.as_tensor(np.asarray(move, dtype=np.int32)).cuda(),
                      None if finished is None else torch.as_tensor(np.asarray(finished, dtype=np.uint8)).cuda(), env_src)
    assert out is env_src
    want = rebase(model, move, finished)
    expect_rebased(dev, model, touched, label)
    np.testing.assert_array_equal(env_src.cpu().numpy(), want, err_msg=f"{label}: env_src")
    # what the model left past n_nodes is not what the device left there: from here on the model holds the device's
    for name in NODE_FIELDS:
        setattr(model, name, getattr(dev, name).cpu().numpy().copy())
    return want, touched


def simulate(dev, data, model, finished, sims, label):
    """`sims` select / backup pairs on device and model, compared after each; returns the refused simulations."""
    M, A = model.M, model.A
    refused = 0
    for s in range(sims):
        logp, values, reward, done = data.rows()
        dev.load(logp, values, reward, done)
        dev.pair()
        torch.cuda.synchronize()
        want = select(model, C, finished)
        for name, g, w in zip(("src", "dst", "act", "leaf"), (p.cpu().numpy() for p in dev.picked), want):
            np.testing.assert_array_equal(g, w, err_msg=f"{label} simulation {s}: {name}")
        src, dst, act, leaf = want
        new_prior, dev_prior = np.zeros((M, A), dtype=np.float32), dev.forest.prior.cpu().numpy()
        for m in np.nonzero(act < A)[0]:
            new_prior[m] = dev_prior[m, leaf[m]]
        backup(model, src, dst, act, leaf, new_prior, values, reward, done)
        expect_rebased(dev.forest, model, [True] * M, f"{label} simulation {s}")
        refused += int(((leaf < 0) & (finished == 0)).sum())
    return refused


def drive(M, cap, A, rounds, quantised=False):
    """`rounds`: the simulations before each rebase.  Returns what was seen."""
    from qiskit_gym_amd.collector import mcts_decide

    ld = (A + 3) // 4 * 4 + 4
    data, dev, model = Data(M, A, ld, 77 + M + cap + A, quantised), Device(M, cap - 1, A, ld), Forest(M, cap - 1, A)
    finished = np.zeros(M, dtype=np.uint8)
    if M > 2:
        finished[2] = 1
    dev.finished.copy_(torch.as_tensor(finished))
    logp, values, _, _ = data.rows()
    dev.load(logp, values, done=np.zeros(M, dtype=np.uint8))
    dev.root(True)
    torch.cuda.synchronize()
    root(model, dev.forest.prior.cpu().numpy()[:, 0, :], values, np.zeros(M, dtype=np.uint8))
    seen = {"kept": 0, "dropped": 0, "refused": 0, "untouched": 0}
    for r, sims in enumerate(rounds):
        seen["refused"] += simulate(dev, data, model, finished, sims, f"round {r}")
        sizes = model.n_nodes.copy()
        if r % 2 == 0:  # the most visited action; else one drawn from the counts
            move = decide_most(model, finished)
            got = mcts_decide(dev.forest, finished=dev.finished).cpu().numpy()
        else:
            move = decide_sampled(model, 9, r, finished)
            got = mcts_decide(dev.forest, sample=True, seed=9, counter=r, finished=dev.finished).cpu().numpy()
        np.testing.assert_array_equal(got, move, err_msg=f"round {r}: the decision on a rebased tree")
        if M > 3 and r == 0:
            move[3] = A  # a live tree with no move: nothing to carry
        env_src, touched = rebase_both(dev.forest, model, move, finished, f"round {r}")
        check_invariants(_trees(model, touched))
        for m in np.nonzero(touched)[0]:
            kept = env_src[m * cap : m * cap + model.n_nodes[m]] - m * cap
            seen["kept"] += len(kept)
            seen["dropped"] += int(sizes[m]) - len(kept)
        seen["untouched"] += M - int(np.sum(touched))
        if r == 0 and M > 4:  # the real envs move on: one more tree ends before the second rebase
            finished[M - 1] = 1
            dev.finished.copy_(torch.as_tensor(finished))
    return seen


def _trees(f, rows):
    rows = np.nonzero(rows)[0]
    g = Forest(len(rows), f.cap - 1, f.A)
    for name in FIELDS:
        setattr(g, name, getattr(f, name)[rows].copy())
    return g


@pytest.mark.parametrize("M,cap,A,rounds", [(1, 2, 1, (1, 1, 1)), (5, 7, 3, (4, 4, 8)), (3, 130, 5, (100, 70, 40)), (2, 300, 256, (200, 150)),
                                            (3, 130, 1, (129, 3, 60))])
def test_rebase_against_the_model_bit_for_bit(M, cap, A, rounds):
    seen = drive(M, cap, A, rounds)
    print(f"M={M} cap={cap} A={A}: {seen}")
    assert seen["kept"] > 0
    if A > 1 and cap > 2:
        assert seen["dropped"] > 0 and (seen["untouched"] > 0 or M <= 2)  # (a finished tree, a tree without a move: from three trees on)
    if (cap, A) in ((7, 3), (130, 1)):
        # tree 0 never meets a terminal node: it fills (1 + 4 nodes, at least one carried twice, 4 + 8 simulations; the chain at once)
        assert seen["refused"] > 0  # `mcts_select` refuses, the rebase makes room again


@pytest.mark.parametrize("M,cap,A,n", [(3, 130, 5, 129), (2, 300, 256, 280)])
def test_random_trees_kept_and_dropped_nodes_interleaved_across_slices(M, cap, A, n):
    """A driven search is narrow: most of a tree hangs under the move.  Here node j hangs under any node before it, so the subtree of
    node 1 is spread over every slice of 64 nodes, dropped nodes in between; then the search goes on below it and a second rebase follows."""
    ld = (A + 3) // 4 * 4 + 4
    model, dev, data = random_forest(M, cap, A, n, cap + A), Device(M, cap - 1, A, ld), Data(M, A, ld, 5, False)
    for name in FIELDS:
        getattr(dev.forest, name).copy_(torch.as_tensor(getattr(model, name)))
    move = np.array([int(np.nonzero(model.child[m, 0] == 1)[0][0]) for m in range(M)], dtype=np.int32)
    env_src, touched = rebase_both(dev.forest, model, move, None, "random trees")
    assert all(touched) and (model.n_nodes < n).all() and model.n_nodes.max() > 64
    assert all(interleaving(env_src[m * cap : m * cap + model.n_nodes[m]] - m * cap) for m in range(M))
    finished = np.zeros(M, dtype=np.uint8)
    simulate(dev, data, model, finished, 20, "random trees, rebased")
    move = decide_most(model)
    sizes = model.n_nodes.copy()
    rebase_both(dev.forest, model, move, None, "random trees, second rebase")
    assert (model.n_nodes < sizes).all()


def test_quantised_numbers_and_ties():
    seen = drive(6, 40, 9, (25, 25, 25), quantised=True)
    assert seen["kept"] > 0 and seen["dropped"] > 0


def test_corner_cases_and_hand_broken_forests():
    model, move, finished, want = corner_forests()
    dev = upload(model)
    before = {name: getattr(dev, name).clone() for name in FIELDS}
    env_src, touched = rebase_both(dev, model, move, finished, "corners")
    assert touched == [kept is not None for kept, _ in want]
    for m, (kept, row) in enumerate(want):
        assert env_src[m * model.cap : (m + 1) * model.cap].tolist() == [m * model.cap + j for j in row] + [model.skip] * (model.cap - len(row)), m
        if kept is None:  # untouched: every array in full, entries past n_nodes included
            for name in FIELDS:
                assert getattr(dev, name)[m].equal(before[name][m]), (m, name)
        else:
            assert int(dev.n_nodes[m]) == len(kept)
    # no `finished` array: every tree is live
    model2, move2, _, _ = corner_forests()
    rebase_both(upload(model2), model2, move2, None, "corners, nobody finished")


def test_chains_at_the_slice_boundaries():
    """A = 1, cap 130: a full chain of three slices of nodes loses its root; then its last node alone is kept."""
    model = chain_forest(4, 130, 130)
    model.n_nodes[3] = 65  # a shorter chain in the same launch: its nodes past 64 are no nodes
    dev = upload(model)
    env_src, touched = rebase_both(dev, model, np.zeros(4, dtype=np.int32), None, "chains")
    assert touched == [True] * 4 and model.n_nodes.tolist() == [129, 129, 129, 64]
    assert env_src[:130].tolist() == list(range(1, 130)) + [model.skip]
    for _ in range(3):  # ... and again and again: 126 nodes
        rebase_both(dev, model, np.zeros(4, dtype=np.int32), None, "chains, again")
    assert model.n_nodes.tolist() == [126, 126, 126, 61] and model.visits[0, 0] == 126


def test_a_captured_rebase_and_copy_pair_replayed_equals_the_eager_calls():
    """The step between two decisions as the search makes it: `mcts_rebase`, then the kept nodes' envs into the other pool."""
    import qiskit_gym_amd.envs as envs
    from qiskit_gym_amd.collector import mcts_decide, mcts_rebase
    from util import line_gateset

    M, cap = 6, 9
    gs = line_gateset("clifford", 3)
    A = len(gs)
    ld = (A + 3) // 4 * 4 + 4
    gym = envs.CliffordGym(3, gs, max_depth=16)
    data = Data(M, A, ld, 4, False)
    rows = [data.rows() for _ in range(cap)]
    fin = torch.zeros(M, dtype=torch.uint8, device="cuda")
    fin[1] = 1

    class Side:
        def __init__(self):
            self.dev = Device(M, cap - 1, A, ld)
            self.pools = [gym.vec(M * cap, add_inverts=False, add_perms=False, track_solution=True) for _ in range(2)]
            self.pools[0].reset(3)
            self.pools[0].step(torch.arange(M * cap, dtype=torch.int32, device="cuda") % A)  # no two envs of a tree alike
            self.pools[1].reset(4)
            self.env_src = torch.full((M * cap,), -7, dtype=torch.int32, device="cuda")
            self.move = torch.zeros(M, dtype=torch.int32, device="cuda")
            self.dev.load(rows[0][0], rows[0][1], done=np.zeros(M, dtype=np.uint8))
            self.dev.root(False)

        def grow(self):
            for r in rows[1:]:
                self.dev.load(*r)
                self.dev.pair()
            mcts_decide(self.dev.forest, finished=fin, move=self.move)

        def pair(self):
            mcts_rebase(self.dev.forest, self.move, fin, self.env_src)
            self.pools[1].copy_envs(self.pools[0], self.env_src)

    eager, graphed, warm = Side(), Side(), Side()
    warm.pair()  # both kernels have run once before the capture
    eager.grow()
    graphed.grow()
    torch.cuda.synchronize()
    start = {name: getattr(graphed.dev.forest, name).clone() for name in FIELDS}
    before = graphed.pools[1].get_state().clone()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        graphed.pair()
    torch.cuda.synchronize()
    for name in FIELDS:  # the capture ran nothing
        assert getattr(graphed.dev.forest, name).equal(start[name])
    assert graphed.pools[1].get_state().equal(before)
    eager.pair()
    graph.replay()
    torch.cuda.synchronize()
    assert eager.env_src.equal(graphed.env_src)
    for name in FIELDS:
        assert getattr(eager.dev.forest, name).equal(getattr(graphed.dev.forest, name)), name
    kept = (eager.env_src != M * cap).nonzero().flatten()
    assert M <= len(kept) < M * cap and int(eager.dev.forest.n_nodes.sum()) - cap == len(kept)  # (tree 1 is finished: untouched, nothing copied)
    a, b, src = eager.pools[1].get_state(), graphed.pools[1].get_state(), eager.pools[0].get_state()
    assert a.equal(b) and a[kept].equal(src[eager.env_src[kept].long()])
    for name in ("reward", "done", "success"):
        assert getattr(eager.pools[1], name).equal(getattr(graphed.pools[1], name)), name
        assert getattr(eager.pools[1], name)[kept].equal(getattr(eager.pools[0], name)[eager.env_src[kept].long()]), name
    rest = torch.ones(M * cap, dtype=torch.bool, device="cuda")
    rest[kept] = False
    assert b[rest].equal(before[rest])  # what is not copied stays
    for side in (eager, graphed, warm):
        for v in side.pools:
            v.close()


def test_the_wrapper_and_the_library_check_their_arguments_and_the_capacity_has_bounds():
    from qiskit_gym_amd import _lib
    from qiskit_gym_amd.collector import mcts_forest, mcts_rebase

    M, A, i32 = 4, 5, torch.int32
    f = mcts_forest(M, 3, A, "cuda", cap=9)
    assert f.cap == 9 and f.N == 3 and f.child.shape == (M, 9, A) and f.skip == 36
    assert mcts_forest(M, 3, A, "cuda").cap == 4 and mcts_forest(M, 3, A, "cuda", cap=4).cap == 4 and mcts_forest(1, 1, 1, "cuda", cap=8192).cap == 8192
    for bad in (3, 0, -1, 8193):
        with pytest.raises(ValueError):
            mcts_forest(M, 3, A, "cuda", cap=bad)
    with pytest.raises(ValueError, match="limit"):
        mcts_forest(M, 3, A, "cuda", cap=9, max_bytes=4 * 4 * (21 + 8 * A) + 16)  # what cap = 4 takes
    move = torch.zeros(M, dtype=i32, device="cuda")
    out = mcts_rebase(f, move)  # n_nodes = 0: nothing to carry, no env
    assert out.shape == (M * 9,) and out.dtype == i32 and (out == f.skip).all()
    assert (mcts_rebase(f, move, finished=torch.ones(M, dtype=torch.bool, device="cuda")) == f.skip).all()
    with pytest.raises(TypeError):
        mcts_rebase(object(), move)
    for bad in (dict(move=move.to(torch.int64)), dict(move=move[:3]), dict(move=move.cpu()), dict(move=torch.zeros(2 * M, dtype=i32, device="cuda")[::2]),
                dict(move=None), dict(finished=torch.zeros(M, dtype=i32, device="cuda")), dict(finished=torch.zeros(M + 1, dtype=torch.uint8, device="cuda")),
                dict(env_src=torch.zeros(M * 9 - 1, dtype=i32, device="cuda")), dict(env_src=torch.zeros(M * 9, dtype=torch.int64, device="cuda")),
                dict(env_src=torch.zeros((M, 9), dtype=i32, device="cuda")), dict(env_src=torch.zeros(M * 9, dtype=i32))):
        with pytest.raises(ValueError):
            mcts_rebase(f, **dict(dict(move=move), **bad))
    with pytest.raises(_lib.QGymError) as e:
        mcts_rebase(mcts_forest(1, 1, 257, "cuda"), torch.zeros(1, dtype=i32, device="cuda"))  # more than four actions per lane
    assert e.value.status == -3
    L, src = _lib.load(), torch.zeros(M * 9 + 1, dtype=i32, device="cuda")
    good = dict(move=move.data_ptr(), src=src.data_ptr())
    for change in (dict(move=None), dict(src=None), dict(move=move.data_ptr() + 2), dict(src=src.data_ptr() + 1)):
        a = dict(good, **change)
        assert L.qg_mcts_rebase(ctypes.byref(f._c), a["move"], None, a["src"], None) == -1, change
    assert L.qg_mcts_rebase(None, good["move"], None, good["src"], None) == -1
    assert L.qg_mcts_rebase(ctypes.byref(f._c), good["move"], None, good["src"], None) == 0
    torch.cuda.synchronize()
