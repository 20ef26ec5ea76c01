"""`collector.mcts_decide` against the CPU model of tests/mctssample_model.py, bit for bit, on forests the test drives itself with the
`Device` / `Data` scheme of tests/test_gpu_mcts_kernels.py: after the root call and after every simulation both modes' moves and the rows of
visit counts are compared, and the forest must be what the model's is -- the call writes nothing into it."""
import ctypes

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")

from mctsmodel import FIELDS, Forest, backup, root, select  # noqa: E402
from mctssample_model import counts, decide_most, decide_sampled, refused  # noqa: E402
from test_gpu_mcts_kernels import C, Data, Device, bits, expect_forest  # noqa: E402

SENTINEL = -5
SHAPES = [(5, 6, 1), (5, 6, 64), (6, 9, 65), (3, 40, 170), (2, 300, 256), (9, 3, 7)]


class Decision:
    """The decision's own buffers: one move vector per mode and a counts matrix wider than A, whose last columns hold a sentinel."""

    def __init__(self, M, A, finished):
        self.A = A
        self.finished_np = np.asarray(finished, dtype=np.uint8)
        self.finished = torch.as_tensor(self.finished_np).cuda()
        self.move = torch.full((M,), -7, dtype=torch.int32, device="cuda")
        self.counts = torch.full((M, A + 3), SENTINEL, dtype=torch.int32, device="cuda")

    def run(self, forest, sample, seed, counter, with_counts=True):
        from qiskit_gym_amd.collector import mcts_decide

        out = mcts_decide(forest, sample=sample, seed=seed, counter=counter, finished=self.finished, move=self.move, counts=self.counts if with_counts else None)
        assert out is self.move
        torch.cuda.synchronize()
        return self.move.cpu().numpy().copy(), self.counts.cpu().numpy().copy()

    def expect(self, forest, model, seed, counter, label):
        """Both modes on `forest` against the model; returns (most, drawn)."""
        want_counts = counts(model)
        got = {}
        for sample in (False, True):
            self.counts[:, : self.A] = -9  # the row is written by every call
            move, cnt = self.run(forest, sample, seed, counter)
            want = decide_sampled(model, seed, counter, self.finished_np) if sample else decide_most(model, self.finished_np)
            np.testing.assert_array_equal(move, want, err_msg=f"{label}: move, sample={sample}")
            np.testing.assert_array_equal(cnt[:, : self.A], want_counts, err_msg=f"{label}: counts, sample={sample}")  # finished trees too
            assert (cnt[:, self.A:] == SENTINEL).all(), f"{label}: columns past A were written"
            got[sample] = move
        return got[False], got[True]


def drive(M, N, A, quantised, seed, counter):
    ld = (A + 3) // 4 * 4 + 4
    data, dev, model = Data(M, A, ld, 1000 + M + N + A, quantised), Device(M, N, A, ld), Forest(M, N, A)
    fin = np.zeros(M, dtype=np.uint8)
    fin[M - 1] = 1  # real env final: no move, but its tree is simulated here, so its counts are not zero
    dec = Decision(M, A, fin)
    # a forest nobody started: n_nodes = 0, no move, no counts
    move, cnt = dec.run(dev.forest, True, seed, counter)
    assert (move == A).all() and (cnt[:, :A] == 0).all() and (cnt[:, A:] == SENTINEL).all()
    logp, values, _, _ = data.rows()
    root_done = np.zeros(M, dtype=np.uint8)
    if M > 1:
        root_done[1] = 1  # a terminal root never gets a child
    dev.load(logp, values, done=root_done)
    dev.root(True)
    torch.cuda.synchronize()
    root(model, dev.forest.prior.cpu().numpy()[:, 0, :], values, root_done)
    # straight after the root call: no root has a child
    most, drawn = dec.expect(dev.forest, model, seed, counter, "root")
    assert (most == A).all() and (drawn == A).all()
    seen = {"differ": 0, "ties": 0, "drawn": set()}
    for s in range(N):
        logp, values, reward, done = data.rows()
        dev.load(logp, values, reward, done)
        dev.pair()
        torch.cuda.synchronize()
        src, dst, act, leaf = select(model, C)
        grown = act < A
        new_prior = np.zeros((M, A), dtype=np.float32)
        dev_prior = dev.forest.prior.cpu().numpy()
        for m in np.nonzero(grown)[0]:
            new_prior[m] = dev_prior[m, leaf[m]]
        backup(model, src, dst, act, leaf, new_prior, values, reward, done)
        expect_forest(dev.forest, model, f"simulation {s}")
        most, drawn = dec.expect(dev.forest, model, seed, counter + s, f"simulation {s}")
        expect_forest(dev.forest, model, f"simulation {s}, after the decision")  # nothing was written into the forest
        live = fin == 0
        seen["differ"] += int((most != drawn)[live].sum())
        n = counts(model)
        seen["ties"] += int(((n == n.max(axis=1, keepdims=True)) & (n > 0)).sum(axis=1).max() > 1)
        seen["drawn"].update(int(a) for a in drawn[live] if a < A)
        assert (n[np.arange(M), np.minimum(drawn, A - 1)][live & (drawn < A)] > 0).all()  # an action without visits is never drawn
        assert most[M - 1] == A and drawn[M - 1] == A
        if M > 1:
            assert most[1] == A and drawn[1] == A and (n[1] == 0).all()
    assert counts(model)[M - 1].sum() == N or root_done[M - 1]  # the finished tree's row is its counts, not zeros
    return seen


@pytest.mark.parametrize("quantised", [True, False], ids=["quantised", "dirichlet"])
@pytest.mark.parametrize("M,N,A", SHAPES)
def test_both_modes_against_the_model_after_every_simulation(M, N, A, quantised):
    seed, counter = (0, 0) if quantised else (0x5EED0000C01F, 2 ** 40)
    seen = drive(M, N, A, quantised, seed, counter)
    print(f"M={M} N={N} A={A}: {seen['differ']} draws off the most visited action, {seen['ties']} simulations with tied counts, "
          f"{len(seen['drawn'])} distinct actions drawn")
    # (with two trees one alone is live and has children, and its search may well stay on one root action: the shape is there for its four
    # slices of actions, which test_counts_written_by_hand_into_every_slice fills)
    if A > 1 and N >= 6 and M > 2:
        assert seen["differ"] > 0  # the two modes are told apart
    if quantised and A > 1 and M > 2:
        assert seen["ties"] > 0


@pytest.mark.parametrize("A", [65, 170, 256])
def test_counts_written_by_hand_into_every_slice(A):
    """What a driven tree rarely shows: visits in every slice of 64 actions, all of them in the last one, counts up to 2^31 - 1 whose sum
    needs more than 32 bits, and roots with a single child."""
    from qiskit_gym_amd.collector import mcts_decide, mcts_forest
    from test_mctssample_model import forest_of

    rng = np.random.default_rng(A)
    M = 48
    rows = np.zeros((M, A), dtype=np.int64)
    for m in range(M):
        kind = m % 4
        if kind == 0:  # a few children anywhere
            rows[m, rng.choice(A, size=rng.integers(1, 9), replace=False)] = rng.integers(1, 40, size=1)
        elif kind == 1:  # many, of few distinct counts
            rows[m] = rng.integers(0, 3, size=A)
        elif kind == 2:  # the last slice alone
            lo = (A - 1) // 64 * 64
            rows[m, lo + rng.integers(0, A - lo)] = 1 + m
            rows[m, A - 1] += 2
        else:  # sums above 2^32
            rows[m, rng.choice(A, size=5, replace=False)] = 2 ** 31 - 1 - rng.integers(0, 3, size=5)
    model = forest_of(rows, N=A)
    dev = mcts_forest(M, A, A, "cuda")
    for name in FIELDS:
        getattr(dev, name).copy_(torch.as_tensor(getattr(model, name)))
    cnt = torch.zeros((M, A), dtype=torch.int32, device="cuda")
    np.testing.assert_array_equal(mcts_decide(dev, counts=cnt).cpu().numpy(), decide_most(model))
    np.testing.assert_array_equal(cnt.cpu().numpy(), rows)
    drawn = set()
    for counter in range(24):
        move = mcts_decide(dev, sample=True, seed=A, counter=counter).cpu().numpy()
        np.testing.assert_array_equal(move, decide_sampled(model, A, counter), err_msg=f"counter {counter}")
        assert (rows[np.arange(M), move] > 0).all()
        drawn.update((move // 64).tolist())
    assert drawn == set(range((A + 63) // 64))  # every slice was drawn from


def test_the_seed_and_the_counter_change_the_draws():
    M, N, A = 64, 12, 20
    ld = 24
    data, dev = Data(M, A, ld, 5, False), Device(M, N, A, ld)
    logp, values, _, _ = data.rows()
    dev.load(logp, values)
    dev.root(False)
    for _ in range(N):
        dev.load(*data.rows())
        dev.pair()
    from qiskit_gym_amd.collector import mcts_decide

    model = model_of(dev.forest)
    a = mcts_decide(dev.forest, sample=True, seed=1, counter=0).cpu().numpy()
    np.testing.assert_array_equal(a, decide_sampled(model, 1, 0))
    assert (mcts_decide(dev.forest, sample=True, seed=1, counter=0).cpu().numpy() == a).all()
    for seed, counter in ((2, 0), (1, 1), (1, 2 ** 40), (2 ** 64 - 1, 2 ** 64 - 1)):
        b = mcts_decide(dev.forest, sample=True, seed=seed, counter=counter).cpu().numpy()
        np.testing.assert_array_equal(b, decide_sampled(model, seed, counter))
        assert (a != b).sum() > M // 8
    np.testing.assert_array_equal(mcts_decide(dev.forest).cpu().numpy(), decide_most(model))  # the defaults: the most visited action


def model_of(forest):
    """The device forest's arrays as a model forest."""
    torch.cuda.synchronize()
    f = Forest(forest.M, forest.N, forest.A)
    for name in FIELDS:
        setattr(f, name, getattr(forest, name).cpu().numpy().copy())
    return f


def test_a_captured_triple_replayed_equals_the_eager_calls():
    from qiskit_gym_amd.collector import mcts_decide

    M, N, A, ld = 37, 9, 21, 24
    data = Data(M, A, ld, 3, True)
    eager, graphed = Device(M, N, A, ld), Device(M, N, A, ld)
    fin = np.zeros(M, dtype=np.uint8)
    fin[5] = 1
    dec = {id(eager): Decision(M, A, fin), id(graphed): Decision(M, A, fin)}

    def triple(dev):
        dev.pair()
        d = dec[id(dev)]
        mcts_decide(dev.forest, sample=True, seed=11, counter=4, finished=d.finished, move=d.move, counts=d.counts)

    logp, values, _, _ = data.rows()
    for dev in (eager, graphed):
        dev.load(logp, values)
        dev.root(False)
    warm = Device(M, N, A, ld)  # every kernel has run once before the capture, on a forest of its own
    warm.load(logp, values, values, np.zeros(M, dtype=np.uint8))
    warm.root(False)
    dec[id(warm)] = Decision(M, A, fin)
    triple(warm)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    start = {name: getattr(graphed.forest, name).clone() for name in FIELDS}
    with torch.cuda.graph(graph):
        triple(graphed)
    for name in FIELDS:  # the capture ran nothing
        assert getattr(graphed.forest, name).equal(start[name])
    moves = set()
    for s in range(N):
        rows = data.rows()
        for dev in (eager, graphed):
            dev.load(*rows)
        triple(eager)
        graph.replay()
        torch.cuda.synchronize()
        for name in FIELDS:
            assert getattr(graphed.forest, name).equal(getattr(eager.forest, name)), (s, name)
        for a, b in zip(eager.picked, graphed.picked):
            assert a.equal(b), s
        assert dec[id(eager)].move.equal(dec[id(graphed)].move) and dec[id(eager)].counts.equal(dec[id(graphed)].counts), s
        model = model_of(eager.forest)
        np.testing.assert_array_equal(dec[id(graphed)].move.cpu().numpy(), decide_sampled(model, 11, 4, fin))
        moves.update(dec[id(graphed)].move.tolist())
    assert len(moves) > 3


def test_forests_the_kernel_must_refuse():
    """A root that claims a child outside the tree, or itself; a negative visit count; n_nodes out of range: no move, a row of zeros, the
    launch returns, the other trees are answered as ever and nothing is written into the forest."""
    from qiskit_gym_amd.collector import mcts_decide

    M, N, A, ld = 8, 3, 5, 8
    data, dev = Data(M, A, ld, 9, False), Device(M, N, A, ld)
    logp, values, _, _ = data.rows()
    dev.load(logp, values)
    dev.root(False)
    for _ in range(2):
        dev.load(*data.rows())
        dev.done.zero_()
        dev.pair()
    torch.cuda.synchronize()
    f = dev.forest
    assert f.n_nodes.tolist() == [3] * M
    free = [int((f.child[m, 0] < 0).nonzero()[0]) for m in range(M)]  # an action the root has not tried
    kid = [int(f.child[m, 0].max()) for m in range(M)]
    f.child[0, 0, free[0]] = 3  # n_nodes is 3, cap 4: inside the arrays, outside the tree
    f.child[1, 0, free[1]] = 0  # the root itself
    f.child[2, 0, free[2]] = 2 ** 31 - 1
    f.visits[3, kid[3]] = -1
    f.n_nodes[4] = 0
    f.n_nodes[5] = 5  # above cap
    f.child[6, 0, free[6]] = -2  # below zero: no child, as -1
    model = model_of(f)
    assert refused(model).tolist() == [True] * 6 + [False, False]
    before = {name: getattr(f, name).clone() for name in FIELDS}
    cnt = torch.full((M, A), SENTINEL, dtype=torch.int32, device="cuda")
    for sample in (False, True):
        move = mcts_decide(f, sample=sample, seed=3, counter=1, counts=cnt).cpu().numpy()
        want = decide_sampled(model, 3, 1) if sample else decide_most(model)
        np.testing.assert_array_equal(move, want)
        assert (move[:6] == A).all() and (move[6:] < A).all()
        np.testing.assert_array_equal(cnt.cpu().numpy(), counts(model))
        assert (cnt[:6] == 0).all() and (cnt[6:].sum(dim=1) == 2).all()
    for name in FIELDS:
        assert bits(getattr(f, name).cpu().numpy()).tobytes() == bits(before[name].cpu().numpy()).tobytes(), name


def test_the_wrapper_and_the_library_check_their_arguments():
    from qiskit_gym_amd import _lib
    from qiskit_gym_amd.collector import mcts_decide, mcts_forest

    M, A = 4, 5
    f = mcts_forest(M, 3, A, "cuda")
    i32 = torch.int32
    ok = torch.zeros((M, A), dtype=i32, device="cuda")
    assert mcts_decide(f, counts=ok).tolist() == [A] * M and mcts_decide(f, counts=torch.zeros((M, 8), dtype=i32, device="cuda")[:, :6]).tolist() == [A] * M
    assert mcts_decide(f, finished=torch.ones(M, dtype=torch.bool, device="cuda")).tolist() == [A] * M
    with pytest.raises(TypeError):
        mcts_decide(object())
    for bad in (dict(counts=ok.to(torch.int64)), dict(counts=ok[:, : A - 1]), dict(counts=ok[: M - 1]), dict(counts=ok.view(-1)),
                dict(counts=torch.zeros((A, M), dtype=i32, device="cuda").t()), dict(counts=ok.cpu()),
                dict(move=torch.zeros(M, dtype=torch.int64, device="cuda")), dict(move=torch.zeros(M + 1, dtype=i32, device="cuda")),
                dict(move=torch.zeros(2 * M, dtype=i32, device="cuda")[::2]), dict(finished=torch.zeros(M, dtype=i32, device="cuda")),
                dict(finished=torch.zeros(M - 1, dtype=torch.uint8, device="cuda"))):
        with pytest.raises(ValueError):
            mcts_decide(f, **bad)
    with pytest.raises(_lib.QGymError) as e:
        mcts_decide(mcts_forest(1, 1, 257, "cuda"))  # more than four actions per lane
    assert e.value.status == -3
    # the library's own checks: QG_ERR_INVALID
    L, move = _lib.load(), torch.zeros(M + 1, dtype=i32, device="cuda")
    good = dict(mode=_lib.MCTS_SAMPLE, move=move.data_ptr(), counts=ok.data_ptr(), ld=A)
    for change in (dict(mode=2), dict(mode=-1), dict(move=None), dict(move=move.data_ptr() + 2), dict(counts=ok.data_ptr() + 1), dict(ld=A - 1)):
        a = dict(good, **change)
        assert L.qg_mcts_decide(ctypes.byref(f._c), a["mode"], 0, 0, None, a["move"], a["counts"], a["ld"], None) == -1, change
    assert L.qg_mcts_decide(ctypes.byref(f._c), good["mode"], 0, 0, None, good["move"], None, 0, None) == 0  # no counts: counts_ld means nothing
    assert L.qg_mcts_decide(None, 0, 0, 0, None, good["move"], None, 0, None) == -1
    torch.cuda.synchronize()
