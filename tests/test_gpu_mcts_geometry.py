"""The tree-search kernels at every launch geometry, against the CPU models bit for bit.

`mcts_select` and `mcts_rebase` run min(4, 65536 / (8 cap)) trees per workgroup -- 4, 3, 2 or 1 waves, the breaks at cap 2048 | 2049,
2730 | 2731 and 4096 | 4097, one tree and all 64 KiB of a workgroup's LDS at cap 8192 -- and the rebase moves the kept nodes' rows in
trips of 16 / K rows, K = ceil(A / 64): 16, 8, 5 or 4.  No result depends on either, which is why nothing else would notice a slip in the
tree index of a three-wave workgroup, in a ragged last workgroup or in a trip of five rows.  tests/test_search_dispatch.py pins on the CPU
that the shapes below reach the brackets they are here for.

Large trees are built by hand and uploaded (the models are per-tree Python: thousands of driven simulations would take minutes): per launch
a single-node tree, a bushy random tree of thousands of nodes, a chain that one lane descends and walks back up node by node, trees with
room for exactly one more node and for none, and a finished tree.  Every array is compared as in tests/test_gpu_mcts_rebase.py."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")

from mctsdevice import C, Data, Device, drive, rebase_both, simulate  # noqa: E402
from mctsmodel import F32, FIELDS, Forest  # noqa: E402
from mctsreuse_model import select  # noqa: E402
from mctssample_model import decide_most, decide_sampled  # noqa: E402
from test_mctsreuse_model import interleaving, random_forest  # noqa: E402

SEED = 11  # of the sampled decisions


def join(trees):
    """Forests of one capacity and action count as one forest, tree after tree."""
    f = Forest(sum(t.M for t in trees), trees[0].cap - 1, trees[0].A)
    for name in FIELDS:
        setattr(f, name, np.concatenate([getattr(t, name) for t in trees]))
    return f


def on_device(model, finished):
    """The model's forest on the device, behind the operand buffers of a `Device`."""
    ld = (model.A + 3) // 4 * 4 + 4
    dev = Device(model.M, model.cap - 1, model.A, ld)
    for name in FIELDS:
        getattr(dev.forest, name).copy_(torch.as_tensor(getattr(model, name)))
    dev.finished.copy_(torch.as_tensor(finished))
    return dev


def single_node(cap, A, seed):
    f = random_forest(1, cap, A, 1, seed)
    f.terminal[:] = 0
    return f


def open_tree(cap, A, n, seed):
    """A random tree without a terminal node: every descent ends on an edge without a child."""
    f = random_forest(1, cap, A, n, seed)
    f.terminal[:] = 0
    return f


def without_its_last_node(f):
    """The same tree one node smaller: the last node was a leaf (no node hangs under a later one)."""
    g = join([f])
    n = int(g.n_nodes[0])
    g.child[0, g.parent[0, n - 1]][g.child[0, g.parent[0, n - 1]] == n - 1] = -1
    g.n_nodes[0] = n - 1
    return g


def one_hot_chain(cap, A, n, a0, seed):
    """A chain of n nodes on action a0 whose every node the selection descends: the priors are one-hot on a0, so every other edge scores
    exactly the node's value, -1, and the chain's edge Q + U = 1/4 + (C * sqrt(visits)) / (1 + n_a) > 0; at the last node a0 scores
    -1 + C.  Visits as the backup leaves them: node j has seen the n - j nodes from itself down."""
    rng = np.random.default_rng(seed)
    f = Forest(1, cap - 1, A)
    f.child[:] = -1
    f.prior[:] = rng.random((1, cap, A)).astype(F32)  # (past n_nodes: no node's)
    f.prior[0, :n] = 0
    f.prior[0, :n, a0] = 1
    f.parent[0] = np.arange(cap) - 1
    f.child[0, np.arange(n - 1), a0] = np.arange(1, n)
    f.value[:] = -1
    f.visits[0, :n] = n - np.arange(n)
    f.wsum[0, :n] = (f.visits[0, :n] * F32(0.25)).astype(F32)
    f.reward[0] = rng.random(cap).astype(F32)
    f.reward[0, 0], f.wsum[0, 0] = 0, 0
    f.n_nodes[0] = n
    return f


KINDS = ("single", "bushy", "chain", "room for one", "full", "finished")


def launches(cap, A, M):
    """The forests of one capacity: the six kinds of tree dealt to launches of M trees, the last launch filled up with small trees.  Returns
    [(forest, finished, the kind of every tree)]."""
    a0 = min(3, A - 1) if A < 64 else A - 1
    full = open_tree(cap, A, cap, cap + 1)
    trees = [("single", single_node(cap, A, cap + 2)), ("bushy", random_forest(1, cap, A, cap * 7 // 10, cap + 3)),
             ("chain", one_hot_chain(cap, A, cap - 1, a0, cap + 4)), ("room for one", without_its_last_node(full)), ("full", full),
             ("finished", random_forest(1, cap, A, 700, cap + 5))]
    assert tuple(k for k, _ in trees) == KINDS
    fill = 0
    while len(trees) % M:  # a launch has M trees: more small ones
        trees.append(("single", single_node(cap, A, cap + 6 + fill)) if fill % 2 else ("small", random_forest(1, cap, A, 150 + fill, cap + 6 + fill)))
        fill += 1
    out = []
    for at in range(0, len(trees), M):
        kinds = [k for k, _ in trees[at : at + M]]
        out.append((join([t for _, t in trees[at : at + M]]), np.array([k == "finished" for k in kinds], dtype=np.uint8), kinds))
    return out


def decisions(dev, model, finished, counter, label):
    """`mcts_decide` in both modes against the models; returns (the most visited moves, the drawn ones)."""
    from qiskit_gym_amd.collector import mcts_decide

    most, drawn = decide_most(model, finished), decide_sampled(model, SEED, counter, finished)
    np.testing.assert_array_equal(mcts_decide(dev.forest, finished=dev.finished).cpu().numpy(), most, err_msg=f"{label}: the most visited")
    got = mcts_decide(dev.forest, sample=True, seed=SEED, counter=counter, finished=dev.finished).cpu().numpy()
    np.testing.assert_array_equal(got, drawn, err_msg=f"{label}: the draw")
    return most, drawn


# (cap, trees per launch, actions): every number of trees per workgroup on both sides of its breaks, more than one workgroup per launch,
# the last one partly filled wherever a workgroup has more than one wave
LARGE = [(2048, 5, 5), (2049, 7, 5), (2730, 7, 5), (2731, 5, 5), (4096, 5, 5), (4097, 3, 5), (8192, 3, 5), (2049, 7, 170)]


@pytest.mark.parametrize("cap,M,A", LARGE, ids=[f"cap{c}-M{m}-A{a}" for c, m, a in LARGE])
def test_large_trees_at_every_number_of_trees_per_workgroup(cap, M, A):
    seen = set()
    for launch, (model, finished, kinds) in enumerate(launches(cap, A, M)):
        label = f"cap {cap}, launch {launch}"
        dev, data = on_device(model, finished), Data(M, A, (A + 3) // 4 * 4 + 4, cap + launch, False)
        base = np.arange(M) * cap
        sizes = model.n_nodes.copy()
        # 1. one select / backup pair: what the model says of each kind first, then device and model side by side
        src, dst, act, leaf = select(model, C, finished)
        for m, kind in enumerate(kinds):
            picked = (int(src[m]) - base[m], int(dst[m]), int(act[m]), int(leaf[m]))
            if kind == "single":
                assert picked == (0, base[m] + 1, picked[2], 1) and picked[2] < A
            elif kind == "chain":  # descended to its last node, cap - 2 levels down: the new node is the last that fits
                assert picked == (cap - 2, base[m] + cap - 1, picked[2], cap - 1) and model.prior[m, 0, picked[2]] == 1
            elif kind == "room for one":
                assert picked[1:] == (base[m] + cap - 1, picked[2], cap - 1) and picked[2] < A
            elif kind == "full":  # refused: the skip index, no action, no leaf
                assert picked[1:] == (model.skip, A, -1)
            elif kind == "finished":
                assert picked == (0, model.skip, A, -1)
            seen.add(kind)
        before = model.visits.copy()
        refused = simulate(dev, data, model, finished, 1, f"{label}, first pair")
        assert refused == kinds.count("full")
        for m, kind in enumerate(kinds):
            if kind == "chain":  # the backup walked the whole chain on one lane: cap - 1 steps
                assert model.n_nodes[m] == cap and (model.visits[m, : cap - 1] == before[m, : cap - 1] + 1).all() and model.visits[m, cap - 1] == 1
            if kind in ("full", "finished"):
                assert (model.visits[m] == before[m]).all() and model.n_nodes[m] == sizes[m]
        # 2. the decision in both modes, 3. a rebase under the most visited move
        most, _ = decisions(dev, model, finished, 0, label)
        sizes = model.n_nodes.copy()
        env_src, touched = rebase_both(dev.forest, model, most, finished, f"{label}, first rebase")
        for m, kind in enumerate(kinds):
            kept = env_src[m * cap : m * cap + model.n_nodes[m]] - base[m]
            assert touched[m] == (kind != "finished"), (m, kind)  # (the single node has a child by now)
            if kind == "chain":  # everything but the root, across every slice of 64 nodes
                assert kept.tolist() == list(range(1, cap))
            if kind in ("bushy", "room for one", "full"):  # kept and dropped nodes interleaved over dozens of slices
                gaps = np.setdiff1d(np.arange(kept[0], kept[-1] + 1), kept)
                assert interleaving(kept) and len(set((kept // 64).tolist())) >= 12 and len(set((gaps // 64).tolist())) >= 12, (m, kind)
        # 4. a second pair on the rebased forest (the full trees have room again), 5. a second rebase, under a drawn move
        assert simulate(dev, data, model, finished, 1, f"{label}, second pair") == 0
        _, drawn = decisions(dev, model, finished, 1, f"{label}, rebased")
        rebase_both(dev.forest, model, drawn, finished, f"{label}, second rebase")
    assert seen >= set(KINDS)


# ---- the rebase at every K ----------------------------------------------------------------------------------------------------------------
ACTIONS = [64, 65, 128, 129, 170, 192, 193]  # K = 1, 2, 2, 3, 3, 3, 4
DRIVEN = [(5, 130, (100, 70, 40)), (5, 300, (120, 90))]


@pytest.mark.parametrize("M,cap,rounds", DRIVEN, ids=["cap130", "cap300"])
@pytest.mark.parametrize("A", ACTIONS)
def test_driven_searches_rebased_at_every_number_of_action_slices(A, M, cap, rounds):
    seen = drive(M, cap, A, rounds)
    print(f"M={M} cap={cap} A={A}: {seen}")
    assert seen["kept"] > 0 and seen["dropped"] > 0 and seen["untouched"] > 0


@pytest.mark.parametrize("cap,n", [(130, 129), (300, 280)])
@pytest.mark.parametrize("A", ACTIONS)
def test_random_trees_rebased_at_every_number_of_action_slices(A, cap, n):
    """The interleaving test of tests/test_gpu_mcts_rebase.py at these A.  With this many actions the root has many children, each with a
    part of the tree: the move is the child whose kept nodes, and the dropped ones between them, lie in more than one slice of 64 nodes and
    are the most (where a tree has no such child: the child with the most nodes)."""
    from mctsreuse_model import kept_nodes

    M = 2
    model = random_forest(M, cap, A, n, cap + A + 2000)
    move, spread = np.zeros(M, dtype=np.int32), 0
    for m in range(M):
        sizes = [(interleaving(np.array(k)), len(k), int(a)) for a in np.nonzero(model.child[m, 0] > 0)[0] for k in [kept_nodes(model, m, int(model.child[m, 0, a]))]]
        move[m] = max(sizes)[2]
        spread += max(sizes)[0]
    dev, data = on_device(model, np.zeros(M, dtype=np.uint8)), Data(M, A, (A + 3) // 4 * 4 + 4, 5, False)
    env_src, touched = rebase_both(dev.forest, model, move, None, "random trees")
    assert all(touched) and spread >= 1 and (model.n_nodes < n).all() and model.n_nodes.max() > 64
    finished = np.zeros(M, dtype=np.uint8)
    simulate(dev, data, model, finished, 20, "random trees, rebased")
    sizes = model.n_nodes.copy()
    rebase_both(dev.forest, model, decide_most(model), None, "random trees, second rebase")
    assert (model.n_nodes < sizes).all()


def spread_actions(A):
    """Actions in turn from every slice of 64, the last action first."""
    K = (A + 63) // 64
    out = [A - 1]
    for i in range(64):
        out += [64 * s + i for s in range(K) if 64 * s + i < A - 1]
    return out


def hand_built(cap, A, kept_counts, starts):
    """One tree per (number of kept nodes, start): the root's child by the LAST action, node 1, is kept with k - 1 nodes below it at the old
    indices start, start + 1, ... -- every other node hangs under the root's side -- so the kept nodes' rows are read from the slice of
    node 1 and from the slices around `start`.  A kept node's children lie at actions of every slice of 64; so do entries that still name a
    dropped node (the rule: not kept, so -1), and the row of the last kept node has nothing else."""
    cases = [(k, s) for k in kept_counts for s in starts]
    M, n = len(cases), cap
    rng = np.random.default_rng(cap + A)
    f = Forest(M, cap - 1, A)
    f.reward[:], f.value[:], f.wsum[:] = (rng.standard_normal((M, cap)).astype(F32) for _ in range(3))
    f.visits[:] = rng.integers(1, 50, size=(M, cap))
    f.prior[:] = rng.random((M, cap, A)).astype(F32)
    f.child[:], f.parent[:] = -1, -1
    f.n_nodes[:] = n
    want = []
    for m, (k, start) in enumerate(cases):
        kept = [1] + list(range(start, start + k - 1))
        assert kept[-1] < n - 1
        slots = {}  # node: the actions of its row still to be given out

        def hang(j, p):
            f.parent[m, j] = p
            f.child[m, p, slots.setdefault(p, spread_actions(A)).pop(0)] = j

        hang(1, 0)  # by action A - 1
        for i, j in enumerate(kept[1:]):
            hang(j, 1 if i % 2 == 0 else kept[i])  # under node 1, or under the kept node before it
        dropped = [j for j in range(2, n) if j not in kept]
        for i, j in enumerate(dropped):
            hang(j, 0 if i < 6 else dropped[i - 1 - i % 5])
        for x in kept:  # entries in every slice that name a dropped node
            for a in slots.setdefault(x, spread_actions(A))[:4]:
                f.child[m, x, a] = dropped[int(rng.integers(0, len(dropped)))]
        want.append(kept)
    f.reward[:, 0], f.wsum[:, 0] = 0, 0
    return f, want


@pytest.mark.parametrize("A", [65, 128, 129, 170, 192])
def test_hand_built_trees_at_every_remainder_of_a_trip_of_rows(A):
    K = (A + 63) // 64
    rows = 16 // K  # 8 or 5
    cap, counts, starts = 300, (1, rows - 1, rows, rows + 1, 2 * rows + 1), (62, 187)
    model, want = hand_built(cap, A, counts, starts)
    M = model.M
    finished = np.zeros(M, dtype=np.uint8)
    dev = on_device(model, finished)
    before = {name: getattr(model, name).copy() for name in ("child", "prior")}
    move = np.full(M, A - 1, dtype=np.int32)
    env_src, touched = rebase_both(dev.forest, model, move, None, f"A={A}, hand-built")
    assert all(touched)
    for m, kept in enumerate(want):
        assert env_src[m * cap : (m + 1) * cap].tolist() == [m * cap + j for j in kept] + [model.skip] * (cap - len(kept)), m
        assert len({j // 64 for j in kept[:rows]}) >= 2 or len(kept) == 1  # the first trip reads rows of two slices of nodes
        new = {j: i for i, j in enumerate(kept)}
        for i, j in enumerate(kept):
            row, old = model.child[m, i], before["child"][m, j]
            assert row.tolist() == [new.get(int(c), -1) for c in old], (m, j)
            named = old >= 0
            assert all(named[64 * s : 64 * s + 64].any() for s in range(K)), (m, j)  # every slice of the row had something to renumber
            assert (row[named] == -1).any()  # ... and a dropped child among it
            assert model.prior[m, i].tobytes() == before["prior"][m, j].tobytes()
        if len(kept) > 1:  # the new root's first child hangs by the last action
            assert model.child[m, 0, A - 1] == 1
    assert sorted({len(kept) for kept in want}) == sorted(set(counts))
    # the rebased trees are trees the other kernels take: a pair, a decision, a second rebase
    data = Data(M, A, (A + 3) // 4 * 4 + 4, A, False)
    simulate(dev, data, model, finished, 1, f"A={A}, rebased")
    most, _ = decisions(dev, model, finished, 0, f"A={A}, rebased")
    rebase_both(dev.forest, model, most, finished, f"A={A}, second rebase")


def test_the_largest_capacity_takes_all_of_a_workgroups_lds_and_is_launched():
    """cap 8192: one tree per workgroup, 65536 bytes of dynamic LDS in `mcts_select` and in `mcts_rebase`.  A launch the runtime refused
    would be a QGymError here, not a retry and not another geometry."""
    from qiskit_gym_amd.collector import mcts_forest, mcts_rebase, mcts_select

    M, cap, A = 2, 8192, 3
    model = join([one_hot_chain(cap, A, cap, 2, 1), single_node(cap, A, 2)])
    dev = mcts_forest(M, 1, A, "cuda", cap=cap)
    for name in FIELDS:
        getattr(dev, name).copy_(torch.as_tensor(getattr(model, name)))
    got = [t.cpu().numpy() for t in mcts_select(dev, C)]
    for name, g, w in zip(("src", "dst", "act", "leaf"), got, select(model, C)):
        np.testing.assert_array_equal(g, w, err_msg=name)
    assert got[0].tolist() == [cap - 1, cap] and got[3].tolist() == [-1, 1]  # the full chain, descended to its end, is refused there
    env_src, touched = rebase_both(dev, model, np.array([2, 0], dtype=np.int32), None, "cap 8192")
    assert touched == [True, False] and model.n_nodes.tolist() == [cap - 1, 1]
