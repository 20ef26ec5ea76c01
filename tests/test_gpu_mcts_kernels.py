"""`collector.mcts_select` and `collector.mcts_backup` against the CPU model of tests/mctsmodel.py, bit for bit, on forests the test builds
and drives itself: no env is involved, rewards, terminal flags, log-probabilities and values are test data.  After the root call and after
every simulation every forest array is compared by bit pattern, and so are the selection's outputs.  `prior` is compared with
`np.exp(logp)` within a few ulp and then taken from the device as the model's input, so expf is no source of divergence."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")

from mctsdevice import C, Data, Device, bits  # noqa: E402
from mctsmodel import FIELDS, Forest, backup, check_invariants, root, select  # noqa: E402

EXP_ULPS = 4


def expect_forest(dev, model, label):
    torch.cuda.synchronize()
    for name in FIELDS:
        got, want = getattr(dev, name).cpu().numpy(), getattr(model, name)
        assert got.dtype == want.dtype and got.shape == want.shape, (label, name)
        np.testing.assert_array_equal(bits(got), bits(want), err_msg=f"{label}: {name}")


def expect_priors(got, logp, label):
    """Rows of `prior` against exp(logp) in f32."""
    want = np.exp(logp.astype(np.float32))
    assert (np.abs(got.astype(np.float64) - want) <= EXP_ULPS * np.spacing(want)).all(), label


def drive(M, N, A, ld, seed, quantised=True, captured=False):
    data, dev, model = Data(M, A, ld, seed, quantised), Device(M, N, A, ld), Forest(M, N, A)
    logp, values, _, _ = data.rows()
    root_done = np.zeros(M, dtype=np.uint8)
    finished = np.zeros(M, dtype=np.uint8)
    if M > 1:
        root_done[1] = 1  # a terminal root: every descent ends on it, nothing is ever expanded
    if M > 2:
        finished[2] = 1  # a tree whose real env is final: no simulation
    dev.load(logp, values, done=root_done)
    dev.finished.copy_(torch.as_tensor(finished))
    if captured:  # every kernel has run once before the capture, on a forest of its own
        warm = Device(M, N, A, ld)
        warm.load(logp, values, values, root_done)
        warm.root(True)
        warm.pair()
    dev.root(True)
    torch.cuda.synchronize()
    prior = dev.forest.prior.cpu().numpy()[:, 0, :]
    expect_priors(prior, logp[:, :A], "root")
    root(model, prior, values, root_done)
    expect_forest(dev.forest, model, "root")
    assert model.value[1, 0] == 0 if M > 1 else True

    seen = {"expanded": 0, "terminal_leaf": 0}
    for s in range(N):
        logp, values, reward, done = data.rows()
        dev.load(logp, values, reward, done)
        dev.simulate(captured)
        torch.cuda.synchronize()
        want = select(model, C, finished)
        got = [p.cpu().numpy() for p in dev.picked]
        for name, g, w in zip(("src", "dst", "act", "leaf"), got, want):
            np.testing.assert_array_equal(g, w, err_msg=f"simulation {s}: {name}")
        src, dst, act, leaf = want
        grown = act < A
        new_prior = np.zeros((M, A), dtype=np.float32)
        dev_prior = dev.forest.prior.cpu().numpy()
        for m in np.nonzero(grown)[0]:
            new_prior[m] = dev_prior[m, leaf[m]]
        expect_priors(new_prior[grown], logp[grown, :A], f"simulation {s}")
        backup(model, src, dst, act, leaf, new_prior, values, reward, done)
        expect_forest(dev.forest, model, f"simulation {s}")
        seen["expanded"] += int(grown.sum())
        seen["terminal_leaf"] += int(((leaf >= 0) & ~grown).sum())
        if M > 1:
            assert (src[1], dst[1], act[1], leaf[1]) == (model.cap, model.skip, A, 0)
        if M > 2:
            assert (src[2], dst[2], act[2], leaf[2]) == (2 * model.cap, model.skip, A, -1)
    live = finished == 0
    check_invariants(model, np.where(live, N, 0))
    assert model.n_nodes[0] == model.cap  # filled exactly
    if M > 1:
        assert model.n_nodes[1] == 1 and model.visits[1, 0] == 1 + N
    if M > 2:
        assert model.n_nodes[2] == 1 and model.visits[2, 0] == 1
    return seen


@pytest.mark.parametrize("M,N,A", [(1, 1, 3), (5, 2, 3), (130, 7, 65), (64, 64, 170), (3, 33, 222)])
def test_kernels_against_the_model_bit_for_bit(M, N, A):
    seen = drive(M, N, A, ld=(A + 3) // 4 * 4 + 4, seed=M + N + A)
    assert seen["expanded"] >= N
    if M * N >= 200:
        assert seen["terminal_leaf"] > N  # descents that end on a terminal node below the root as well


def test_unquantised_numbers():
    drive(33, 12, 50, ld=50, seed=7, quantised=False)


def near_tie_forest(M, seed):
    """Trees whose root offers seven actions of mathematically equal score: action a has prior k * p0 and a terminal child visited k - 1
    times with wsum 0 (k = 1: no child), and value[0] = 0, so every score is U = ((C * k p0) * sqrt(V)) / k.  In f32 the seven differ in
    their last bits -- by the roundings of the two products, the square root and the division -- so the winner is the arithmetic's."""
    A = 7
    rng = np.random.default_rng(seed)
    f = Forest(M, A, A)
    root(f, np.zeros((M, A), dtype=np.float32), np.zeros(M, dtype=np.float32))
    for m in range(M):
        p0, n = np.float32(0.01 + 0.1 * rng.random()), 1
        for a, k in enumerate(rng.permutation(np.arange(1, A + 1))):
            f.prior[m, 0, a] = np.float32(k) * p0
            if k > 1:
                f.child[m, 0, a], f.parent[m, n], f.visits[m, n], f.terminal[m, n] = n, 0, k - 1, 1
                f.child[m, n] = -1
                n += 1
        f.n_nodes[m], f.visits[m, 0] = n, rng.integers(2, 500)
    return f


def test_near_ties_are_decided_by_the_last_bit():
    """The other tests' scores are either equal, whatever the rounding, or far apart; here the winner changes with the order of the two
    products, and would with a division or a square root that is an ulp off."""
    from mctsmodel import F32, best_action, scores
    from qiskit_gym_amd.collector import mcts_forest, mcts_select

    M = 512
    model = near_tie_forest(M, 17)
    dev = mcts_forest(M, model.N, model.A, "cuda")
    for name in FIELDS:
        getattr(dev, name).copy_(torch.as_tensor(getattr(model, name)))
    got = [t.cpu().numpy() for t in mcts_select(dev, C)]
    for name, g, w in zip(("src", "dst", "act", "leaf"), got, select(model, C)):
        np.testing.assert_array_equal(g, w, err_msg=name)
    # what the data can tell apart: the same scores with the products associated the other way pick another action in many trees
    distinct = other = 0
    for m in range(M):
        n_a = np.where(model.child[m, 0] >= 0, model.visits[m, np.maximum(model.child[m, 0], 0)], 0)
        alt = (F32(C) * (model.prior[m, 0] * np.sqrt(F32(model.visits[m, 0])))) / (1 + n_a).astype(F32)
        sc = scores(model, m, 0, C)
        distinct += len(set(sc.tolist())) > 1
        other += best_action(alt) != best_action(sc)
    print(f"near ties: {distinct} of {M} trees with unequal scores, {other} where the other association picks another action")
    assert distinct >= M // 2 and other >= M // 8


def test_a_captured_launch_pair_replayed_on_new_contents():
    seen = drive(37, 9, 21, ld=24, seed=3, captured=True)
    assert seen["expanded"] > 9


def test_wrappers_check_their_arguments():
    from qiskit_gym_amd import _lib
    from qiskit_gym_amd.collector import mcts_backup, mcts_forest, mcts_select

    f = mcts_forest(4, 3, 5, "cuda")
    assert f.child.shape == (4, 4, 5) and f.prior.dtype == torch.float32 and f.n_nodes.shape == (4,) and f.skip == 16
    assert _lib.load().qg_mcts_forest_bytes(4, 4, 5) == sum(getattr(f, n).numel() * getattr(f, n).element_size() for n in f.FIELDS)
    with pytest.raises(ValueError, match="limit"):
        mcts_forest(4, 3, 5, "cuda", max_bytes=100)
    with pytest.raises(ValueError):
        mcts_forest(4, 0, 5, "cuda")
    logp, vals = torch.zeros((4, 5), device="cuda"), torch.zeros(4, device="cuda")
    with pytest.raises(ValueError):
        mcts_select(f, 0.0)
    with pytest.raises(ValueError):
        mcts_select(f, C, src=torch.zeros(4, dtype=torch.int64, device="cuda"))
    with pytest.raises(ValueError):
        mcts_backup(f, logp[:, :4], vals, root=True)  # fewer columns than actions
    with pytest.raises(ValueError):
        mcts_backup(f, logp, vals)  # a backup without the selection's outputs
    with pytest.raises(_lib.QGymError) as e:
        mcts_select(mcts_forest(1, 1, 257, "cuda"), C)  # more than four actions per lane
    assert e.value.status == -3
    # a forest nobody started (n_nodes = 0) and one whose root claims a child outside the tree: the call ends those trees' work, leaf = -1
    out = [t.cpu().numpy() for t in mcts_select(f, C)]
    assert (out[3] == -1).all() and (out[2] == 5).all() and (out[1] == f.skip).all()
    mcts_backup(f, logp, vals, root=True)
    f.child[0, 0, 2] = 3  # n_nodes is 1
    f.prior[0, 0] = 0.0
    out = [t.cpu().numpy() for t in mcts_select(f, C)]
    assert out[3].tolist() == [-1, 1, 1, 1] and out[2].tolist() == [5, 0, 0, 0]
    before = f.visits.clone()
    mcts_backup(f, logp, vals, vals, torch.zeros(4, dtype=torch.uint8, device="cuda"), *(torch.as_tensor(o).cuda() for o in out))
    torch.cuda.synchronize()
    assert f.visits[0].equal(before[0]) and f.n_nodes.tolist() == [1, 2, 2, 2]
