"""`collector.mcts_select_many` and `collector.mcts_backup_many` against tests/mctsmany_model.py, bit for bit, driven like
tests/test_gpu_mcts_kernels.py: forests the test builds and drives itself, several rounds on one forest, every output of every selection and
every forest array after every backup compared by bit pattern.  `prior` of a new node is taken from the device as the model's input (it is
expf of the test's own log-probabilities, which tests/test_gpu_mcts_kernels.py holds to a few ulp), so expf is no source of divergence.

The large capacities -- every number of trees per workgroup, and the one tree that takes a workgroup's whole LDS, where the list of pending
edges has nowhere to live but the lanes -- use the hand-built trees of tests/test_gpu_mcts_geometry.py."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")

from mctsdevice import C, Data, bits  # noqa: E402
from mctsmany_model import backup_many, select_many  # noqa: E402
from mctsmodel import FIELDS, Forest, root  # noqa: E402
from test_gpu_mcts_geometry import KINDS, LARGE, launches  # noqa: E402
from test_mctsmany_model import invariants, stalls_of  # noqa: E402
from test_mctsreuse_model import random_forest  # noqa: E402


class DeviceMany:
    """A forest on the device with static operand buffers for rounds of K entries per tree."""

    def __init__(self, M, cap, A, K, ld, model=None):
        from qiskit_gym_amd.collector import mcts_forest

        self.M, self.K = M, K
        self.forest = mcts_forest(M, 1, A, "cuda", cap=cap)
        if model is not None:
            for name in FIELDS:
                getattr(self.forest, name).copy_(torch.as_tensor(getattr(model, name)))
        self.logp = torch.empty((M * K, ld), dtype=torch.float32, device="cuda")
        self.values, self.reward = (torch.empty(M * K, dtype=torch.float32, device="cuda") for _ in range(2))
        self.done = torch.zeros(M * K, dtype=torch.uint8, device="cuda")
        self.finished = torch.zeros(M, dtype=torch.uint8, device="cuda")
        self.picked = tuple(torch.full((M * K,), -7, dtype=torch.int32, device="cuda") for _ in range(4))
        self.graph = None

    def load(self, logp, values, reward, done):
        for t, a in ((self.logp, logp), (self.values, values), (self.reward, reward), (self.done, done)):
            t.copy_(torch.as_tensor(a))

    def pair(self, k, vl):
        from qiskit_gym_amd.collector import mcts_backup_many, mcts_select_many

        out = mcts_select_many(self.forest, C, self.K, k, vl, self.finished, *self.picked)
        assert all(o is p for o, p in zip(out, self.picked))
        mcts_backup_many(self.forest, self.K, self.logp, self.values, self.reward, self.done, *self.picked, k=k)

    def replay(self, k, vl):
        if self.graph is None:
            torch.cuda.synchronize()
            self.graph = torch.cuda.CUDAGraph()
            with torch.cuda.graph(self.graph):
                self.pair(k, vl)
        self.graph.replay()


def expect_forest(dev, model, label):
    torch.cuda.synchronize()
    for name in FIELDS:
        got, want = getattr(dev, name).cpu().numpy(), getattr(model, name)
        assert got.dtype == want.dtype and got.shape == want.shape, (label, name)
        np.testing.assert_array_equal(bits(got), bits(want), err_msg=f"{label}: {name}")


def one_round(dev, model, data, k, vl, finished, label, seen, captured=False, no_done=False):
    """A select / backup pair on device and model, everything compared; what happened is added to `seen`."""
    M, A, K, cap = model.M, model.A, dev.K, model.cap
    logp, values, reward, done = data.rows()
    done[:K] = 0  # tree 0 never meets a terminal node: it takes a node per descent
    if no_done:
        done[:] = 0
    dev.load(logp, values, reward, done)
    dev.replay(k, vl) if captured else dev.pair(k, vl)
    torch.cuda.synchronize()
    want = select_many(model, C, k, K, vl, finished)
    got = [p.cpu().numpy() for p in dev.picked]
    for name, g, w in zip(("src", "dst", "act", "leaf"), got, want):
        np.testing.assert_array_equal(g, w, err_msg=f"{label}: {name}")
    src, dst, act, leaf = want
    new_prior, dev_prior = np.zeros((M * K, A), dtype=np.float32), dev.forest.prior.cpu().numpy()
    for e in np.nonzero(act < A)[0]:
        new_prior[e] = dev_prior[e // K, leaf[e]]
    sizes = model.n_nodes.copy()
    linked = backup_many(model, k, K, src, dst, act, leaf, new_prior, values, reward, done)
    expect_forest(dev.forest, model, label)
    np.testing.assert_array_equal(linked, (act < A).reshape(M, K).sum(axis=1))
    made = np.arange(K)[None, :] < k
    live = (np.asarray(finished) == 0)[:, None] & ((sizes >= 1) & (sizes <= cap))[:, None]
    lf, ac = leaf.reshape(M, K), act.reshape(M, K)
    seen["several"] += int(((ac < A).sum(axis=1) >= 2).sum())
    seen["full"] += int((made & live & (lf < 0)).sum())
    seen["stalls"] += stalls_of(model, k, K, act, leaf)
    for m in range(M):
        ends = [int(x) for x, a in zip(lf[m, :k], ac[m, :k]) if x >= 0 and a == A and model.terminal[m, x]]
        seen["shared"] += len(ends) - len(set(ends))
    return want


def new_seen():
    return {"several": 0, "full": 0, "stalls": [], "shared": 0}


def drive(M, cap, A, K, k, vl, rounds, quantised, seed, captured=False):
    ld = (A + 3) // 4 * 4 + 4
    first, data = Data(M, A, ld, seed, quantised), Data(M * K, A, ld, seed + 1, quantised)
    dev, model = DeviceMany(M, cap, A, K, ld), Forest(M, cap - 1, A)
    logp, values, _, _ = first.rows()
    root_done, finished = np.zeros(M, dtype=np.uint8), np.zeros(M, dtype=np.uint8)
    if M > 1:
        root_done[1] = 1  # a terminal root: every descent of every round ends on it
    if M > 2:
        finished[2] = 1  # a finished tree among live ones
    from qiskit_gym_amd.collector import mcts_backup

    rows = torch.as_tensor(logp).cuda()
    mcts_backup(dev.forest, rows, torch.as_tensor(values).cuda(), done=torch.as_tensor(root_done).cuda(), root=True)
    dev.finished.copy_(torch.as_tensor(finished))
    torch.cuda.synchronize()
    root(model, dev.forest.prior.cpu().numpy()[:, 0, :], values, root_done)
    expect_forest(dev.forest, model, "root")
    if captured:  # both kernels have run once before the capture, on a forest of their own
        warm = DeviceMany(M, cap, A, K, ld, model)
        warm.load(*data.rows())
        warm.pair(k, vl)
    seen = new_seen()
    for r in range(rounds):
        src, dst, act, leaf = one_round(dev, model, data, k, vl, finished, f"round {r}", seen, captured)
        if M > 1:
            e = slice(K, K + k)
            assert (leaf[e] == 0).all() and (act[e] == A).all() and (src[e] == cap).all() and (dst[e] == model.skip).all()
        if M > 2:
            e = slice(2 * K, 3 * K)
            assert (leaf[e] == -1).all() and (act[e] == A).all() and (src[e] == 2 * cap).all() and (dst[e] == model.skip).all()
    sims = model.visits[:, 0] - 1
    invariants(model, sims, seen["stalls"])
    if M > 1:
        assert model.n_nodes[1] == 1 and model.visits[1, 0] == 1 + rounds * k
        seen["shared"] -= rounds * (k - 1)  # (the terminal root is not what "shared" is there for)
    if M > 2:
        assert model.n_nodes[2] == 1 and model.visits[2, 0] == 1
    return seen


SHAPES = [(1, 1), (2, 2), (5, 3), (64, 64), (64, 7)]  # (stride, k)
ACTIONS = [3, 64, 65, 256]
CASES = [(i, (1, 5, 9)[i % 3], (8, 40)[i % 2], A, K, k, (0.0, 0.5)[(i // 2) % 2]) for i, (A, (K, k)) in enumerate((A, s) for A in ACTIONS for s in SHAPES)]


@pytest.mark.parametrize("i,M,cap,A,K,k,vl", CASES, ids=[f"M{c[1]}-cap{c[2]}-A{c[3]}-K{c[4]}-k{c[5]}-vl{c[6]}" for c in CASES])
def test_kernels_against_the_model_bit_for_bit(i, M, cap, A, K, k, vl):
    rounds = 6 if k == 1 else 3
    seen = drive(M, cap, A, K, k, vl, rounds, quantised=i % 4 < 2, seed=100 + i)
    print(f"M={M} cap={cap} A={A} K={K} k={k} vl={vl}: several {seen['several']}, full {seen['full']}, no candidate {len(seen['stalls'])}, "
          f"shared terminal leaves {seen['shared']}")
    if k >= 2:
        assert seen["several"] > 0  # tree 0 never meets a terminal node: a round gives it several nodes
    if 1 + rounds * k > cap and A > 3:
        assert seen["full"] > 0  # tree 0 wants a node per descent (with three actions a round soon runs out of edges instead)
    if A == 3 and k >= 7:
        assert len(seen["stalls"]) > 0  # a node's three edges are all pending


def test_every_case_occurs_in_one_small_forest():
    """A = 3, cap = 8, rounds of 7: several expansions per round, trees that fill, nodes without a candidate left and descents that share a
    terminal leaf, all in one forest -- none of the comparisons above passes for want of the case."""
    seen = drive(9, 8, 3, 8, 7, 0.5, 4, True, seed=5)
    assert seen["several"] > 0 and seen["full"] > 0 and len(seen["stalls"]) > 0 and seen["shared"] > 0, seen


def test_unquantised_numbers_on_random_trees():
    M, cap, A, K, k = 5, 130, 21, 16, 11
    model = random_forest(M, cap, A, 90, 3)
    ld = 24
    dev, data = DeviceMany(M, cap, A, K, ld, model), Data(M * K, A, ld, 8, False)
    finished = np.zeros(M, dtype=np.uint8)
    seen = new_seen()
    for r in range(6):
        one_round(dev, model, data, k, 0.25, finished, f"round {r}", seen)
    assert seen["several"] > 0 and seen["full"] > 0 and (model.n_nodes == cap).any()


@pytest.mark.parametrize("vl", [0.0, 0.5])
def test_one_descent_is_mcts_select_and_mcts_backup_on_the_device(vl):
    """k = stride = 1 against the one-descent kernels on a copy of the same forest: every output and every array, whatever virtual_loss."""
    from qiskit_gym_amd.collector import mcts_backup, mcts_select

    M, cap, A, ld = 9, 40, 65, 72
    model = random_forest(M, cap, A, 30, 12)
    one, many = DeviceMany(M, cap, A, 1, ld, model), DeviceMany(M, cap, A, 1, ld, model)
    data = Data(M, A, ld, 4, True)
    finished = np.zeros(M, dtype=np.uint8)
    finished[3] = 1
    expanded = refused = 0
    for dev in (one, many):
        dev.finished.copy_(torch.as_tensor(finished))
    for s in range(14):
        rows = data.rows()
        for dev in (one, many):
            dev.load(*rows)
        mcts_select(one.forest, C, one.finished, *one.picked)
        mcts_backup(one.forest, one.logp, one.values, one.reward, one.done, *one.picked)
        many.pair(1, vl)
        torch.cuda.synchronize()
        for name, a, b in zip(("src", "dst", "act", "leaf"), one.picked, many.picked):
            assert torch.equal(a, b), f"simulation {s}: {name}"
        for name in FIELDS:
            a, b = getattr(one.forest, name), getattr(many.forest, name)
            assert torch.equal(a.view(torch.uint8 if a.element_size() == 1 else torch.int32), b.view(torch.uint8 if b.element_size() == 1 else torch.int32)), (s, name)
        expanded += int((one.picked[2] < A).sum())
        refused += int(((one.picked[3] < 0) & (one.finished == 0)).sum())
    assert expanded > M and refused > 0  # the trees fill on the way


def test_a_captured_launch_pair_replayed_on_new_contents():
    seen = drive(9, 40, 21, 5, 3, 0.5, 5, True, seed=3, captured=True)
    assert seen["several"] > 0


def test_failed_range_checks_end_a_trees_work():
    """What tests/test_gpu_mcts_kernels.py and test_gpu_mcts_rebase.py feed the one-descent kernels: a child index outside the tree, below
    the root or on the way down, and n_nodes outside [1, cap].  Every descent from the failure on is refused and the backup leaves the
    tree alone."""
    M, cap, A, K, k, ld = 6, 20, 3, 4, 3, 8
    model = random_forest(M, cap, A, 10, 4)
    model.terminal[:] = 0
    model.child[0, 0, 1] = 15  # the root names a node that is not there
    model.n_nodes[1] = 0
    model.n_nodes[2] = cap + 1
    model.child[3, 0, :] = -1
    model.child[3, 0, 2], model.prior[3, 0] = 4, (0, 0, 1)  # the root's only visited child ...
    model.visits[3, 4], model.wsum[3, 4], model.child[3, 4, 0] = 1, 50.0, 3  # ... wins every score and names a node above itself
    dev, data = DeviceMany(M, cap, A, K, ld, model), Data(M * K, A, ld, 2, True)
    before = {name: getattr(model, name).copy() for name in FIELDS}
    seen = new_seen()
    src, dst, act, leaf = (t.reshape(M, K) for t in one_round(dev, model, data, k, 0.5, np.zeros(M, dtype=np.uint8), "broken trees", seen, no_done=True))
    for m in range(4):
        assert (leaf[m] == -1).all() and (act[m] == A).all() and (dst[m] == model.skip).all(), m
        for name in FIELDS:
            assert bits(getattr(model, name)[m]).tobytes() == bits(before[name][m]).tobytes(), (m, name)
    assert src[3, 0] == 3 * cap + 4 and (src[3, 1:] == 3 * cap).all()  # the descent that failed stood on node 4; the later ones were not made
    assert (leaf[4:, :k] >= 0).all() and (model.n_nodes[4:] > 10).all()  # the trees beside them are searched as ever
    # entries that fail the backup's own checks are skipped, later ones go on; a skipped expansion takes the later expansions with it
    src, dst, act, leaf = (p.clone() for p in dev.picked)
    from qiskit_gym_amd import collector as mcts

    mcts.mcts_select_many(dev.forest, C, K, k, 0.5, dev.finished, src, dst, act, leaf)
    want = [t.copy() for t in select_many(model, C, k, K, 0.5, np.zeros(M, dtype=np.uint8))]
    assert (want[2].reshape(M, K)[4:, :k] < A).all()
    src[4 * K] = -1
    want[0][4 * K] = -1  # tree 4: the first entry names no node of the tree
    leaf[5 * K + 1] = 3
    want[3][5 * K + 1] = 3  # tree 5: the second entry's leaf is not its new node
    sizes = model.n_nodes.copy()
    logp, values, reward, done = data.rows()
    dev.load(logp, values, reward, done)
    mcts.mcts_backup_many(dev.forest, K, dev.logp, dev.values, dev.reward, dev.done, src, dst, act, leaf, k=k)
    torch.cuda.synchronize()
    new_prior, dev_prior = np.zeros((M * K, A), dtype=np.float32), dev.forest.prior.cpu().numpy()
    new_prior[5 * K] = dev_prior[5, sizes[5]]
    linked = backup_many(model, k, K, *want, new_prior, values, reward, done)
    assert linked.tolist() == [0, 0, 0, 0, 0, 1]
    expect_forest(dev.forest, model, "skipped entries")


@pytest.mark.parametrize("cap,M,A", LARGE[:-1], ids=[f"cap{c}-M{m}-A{a}" for c, m, a in LARGE[:-1]])
def test_large_trees_at_every_number_of_trees_per_workgroup(cap, M, A):
    K, k, vl, ld = 8, 5, 0.5, (A + 3) // 4 * 4 + 4
    kinds_seen = set()
    for launch, (model, finished, kinds) in enumerate(launches(cap, A, M)):
        dev, data = DeviceMany(M, cap, A, K, ld, model), Data(M * K, A, ld, cap + launch, False)
        dev.finished.copy_(torch.as_tensor(finished))
        sizes = model.n_nodes.copy()
        seen = new_seen()
        src, dst, act, leaf = (t.reshape(M, K) for t in one_round(dev, model, data, k, vl, finished, f"cap {cap}, launch {launch}", seen))
        for m, kind in enumerate(kinds):
            grown = int((act[m] < A).sum())
            if kind == "single":  # A = 5 = k: every edge of the root, in the order of the scores, each once
                assert grown == min(k, A) and sorted(act[m, :k].tolist()) == list(range(A)) and (src[m, :k] == m * cap).all()
            elif kind == "bushy":  # the pending edges are in use, and at cap 8192 they have no LDS to live in
                assert grown >= 2 and len({(int(s), int(a)) for s, a in zip(src[m, :k], act[m, :k]) if a < A}) == grown
            elif kind == "chain":  # five walks of the whole chain; the first takes the last node, the others find the tree full
                assert leaf[m, 0] == cap - 1 and (leaf[m, 1:k] == -1).all() and (src[m, :k] == m * cap + cap - 2).all()
            elif kind == "room for one":
                assert grown == 1 and leaf[m, 0] == cap - 1 and (leaf[m, 1:k] == -1).all() and model.n_nodes[m] == cap
            elif kind == "full":
                assert (leaf[m] == -1).all() and (act[m] == A).all() and model.n_nodes[m] == sizes[m] == cap
            elif kind == "finished":
                assert (leaf[m] == -1).all() and (src[m] == m * cap).all() and model.n_nodes[m] == sizes[m]
            kinds_seen.add(kind)
        assert seen["full"] >= 4 * kinds.count("chain") + 4 * kinds.count("room for one") + 5 * kinds.count("full")
    assert kinds_seen >= set(KINDS)


def test_wrappers_check_their_arguments():
    from qiskit_gym_amd import _lib
    from qiskit_gym_amd.collector import mcts_backup_many, mcts_forest, mcts_select_many

    M, A, K = 4, 5, 3
    f = mcts_forest(M, 3, A, "cuda")
    i32 = dict(dtype=torch.int32, device="cuda")
    for bad in (dict(K=0), dict(K=65), dict(K=3, k=4), dict(K=3, k=0), dict(K=3, virtual_loss=-0.5), dict(K=3, virtual_loss=float("inf")),
                dict(K=3, virtual_loss=float("nan")), dict(K=3, src=torch.zeros(M, **i32)), dict(K=3, leaf=torch.zeros(M * K, dtype=torch.int64, device="cuda")),
                dict(K=3, finished=torch.zeros(M * K, dtype=torch.uint8, device="cuda"))):
        with pytest.raises(ValueError):
            mcts_select_many(f, C, **bad)
    with pytest.raises(ValueError):
        mcts_select_many(f, 0.0, K)
    with pytest.raises(TypeError):
        mcts_select_many(None, C, K)
    logp, vals, done = torch.zeros((M * K, A), device="cuda"), torch.zeros(M * K, device="cuda"), torch.zeros(M * K, dtype=torch.uint8, device="cuda")
    picked = mcts_select_many(f, C, K)  # a forest nobody started: every entry refused, all four arrays written in full
    assert all(p.shape == (M * K,) for p in picked) and (picked[3] == -1).all() and (picked[2] == A).all() and (picked[1] == f.skip).all()
    assert picked[0].tolist() == [m * f.cap for m in range(M) for _ in range(K)]
    for bad in ((K, logp[:, :4], vals, vals, done, *picked), (K, logp[:M], vals, vals, done, *picked), (K, logp, vals[:M], vals, done, *picked),
                (K, logp, vals, vals, done[:M], *picked), (K, logp, vals, vals, done, picked[0][:M], *picked[1:]), (K, logp, vals, None, done, *picked),
                (65, logp, vals, vals, done, *picked)):
        with pytest.raises(ValueError):
            mcts_backup_many(f, *bad)
    with pytest.raises(ValueError):
        mcts_backup_many(f, K, logp, vals, vals, done, *picked, k=4)
    L = _lib.load()
    ptrs = [p.data_ptr() for p in picked]
    for k, stride, vl in ((0, 3, 0.0), (4, 3, 0.0), (3, 65, 0.0), (3, 3, -1.0), (3, 3, float("inf")), (3, 3, float("nan"))):  # QG_ERR_INVALID, no launch
        assert L.qg_mcts_select_many(f._c, C, vl, k, stride, None, *ptrs, None) == -1, (k, stride, vl)
    assert L.qg_mcts_backup_many(f._c, 4, 3, *ptrs, logp.data_ptr(), A, vals.data_ptr(), vals.data_ptr(), done.data_ptr(), None) == -1
    with pytest.raises(_lib.QGymError) as e:
        mcts_select_many(mcts_forest(1, 1, 257, "cuda"), C, 2)  # the forest's own limits
    assert e.value.status == -3
    mcts_backup_many(f, K, logp, vals, vals, done, *picked)  # nothing to do on trees nobody started
    torch.cuda.synchronize()
    assert f.n_nodes.tolist() == [0] * M
