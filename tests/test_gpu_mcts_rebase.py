"""`collector.mcts_rebase` against the CPU model of tests/mctsreuse_model.py, bit for bit, on forests the test drives itself with the
`Device` / `Data` scheme of tests/mctsdevice.py: decisions of driven simulations, a rebase on device and model, further
simulations on the rebased trees and a second rebase -- so `mcts_select`, `mcts_backup` and `mcts_decide` are shown to accept rebased
trees -- then the corner cases and hand-broken forests of tests/test_mctsreuse_model.py, a captured rebase + `copy_envs` pair, the
argument checks and `mcts_forest(cap=...)`.  A rebased tree is compared on the nodes below its new n_nodes (the entries past them mean
nothing), an untouched tree in full, `env_src` in full."""
import ctypes

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")

from mctsdevice import Data, Device, drive, rebase_both, simulate, upload  # noqa: E402
from mctsmodel import FIELDS  # noqa: E402
from mctssample_model import decide_most  # noqa: E402
from test_mctsreuse_model import chain_forest, corner_forests, interleaving, random_forest  # noqa: E402


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
