"""What the device tests of the tree-search kernels share (tests/test_gpu_mcts_kernels.py, test_gpu_mcts_rebase.py,
test_gpu_mcts_geometry.py): the stand-in for envs and policy, the forest on the device with static operand buffers, and one select / backup
pair, one rebase and one driven search on device and model with every array compared by bit pattern.  TEST INFRASTRUCTURE ONLY; imported
by tests that have already found torch and are marked `gpu`."""
import numpy as np
import torch

from mctsmodel import FIELDS, Forest, backup, check_invariants, root
from mctsreuse_model import carried_child, rebase, select
from mctssample_model import decide_most, decide_sampled
from util import bits  # noqa: F401  (the device tests import it from here)

C = 2 ** 0.5
NODE_FIELDS = ("parent", "reward", "value", "visits", "wsum", "terminal", "child", "prior")


class Data:
    """The test's stand-in for envs and policy: per call rows of log-probabilities [M, ld] (the columns past A hold a value that would
    win every comparison, and turn every prior into +inf, if it were read), values, rewards and terminal flags."""

    def __init__(self, M, A, ld, seed, quantised):
        self.M, self.A, self.ld, self.quantised, self.rng = M, A, ld, quantised, np.random.default_rng(seed)

    def rows(self):
        rng, M, A = self.rng, self.M, self.A
        logp = np.full((M, self.ld), 3.0e38, dtype=np.float32)
        if self.quantised:  # few distinct priors, some of them 0: equal scores are frequent
            with np.errstate(divide="ignore"):  # a prior of 0: log-probability -inf, a masked action
                logp[:, :A] = np.log(rng.integers(0, 4, size=(M, A)).astype(np.float32) / np.float32(4.0 * A)).astype(np.float32)
            values = (rng.integers(-2, 5, size=M) / 4.0).astype(np.float32)
            reward = (rng.integers(-2, 5, size=M) / 4.0).astype(np.float32)
        else:
            logp[:, :A] = np.log(rng.dirichlet(np.ones(A), size=M)).astype(np.float32)
            values = rng.standard_normal(M).astype(np.float32)
            reward = (rng.random(M) * 1.5 - 0.5).astype(np.float32)
        done = (rng.random(M) < 0.15).astype(np.uint8)
        done[0] = 0  # tree 0 never meets a terminal node: it fills its N + 1 nodes exactly
        return logp, values, reward, done


class Device:
    """The forest on the device with static operand buffers, so that a select / backup pair can be captured once and replayed."""

    def __init__(self, M, N, A, ld):
        from qiskit_gym_amd.collector import mcts_forest

        self.forest = mcts_forest(M, N, A, "cuda")
        self.logp = torch.empty((M, ld), dtype=torch.float32, device="cuda")
        self.values, self.reward = (torch.empty(M, dtype=torch.float32, device="cuda") for _ in range(2))
        self.done, self.finished = (torch.zeros(M, dtype=torch.uint8, device="cuda") for _ in range(2))
        self.picked = tuple(torch.full((M,), -7, dtype=torch.int32, device="cuda") for _ in range(4))
        self.graph = None

    def load(self, logp, values, reward=None, done=None):
        for t, a in ((self.logp, logp), (self.values, values), (self.reward, reward), (self.done, done)):
            if a is not None:
                t.copy_(torch.as_tensor(a))

    def root(self, with_done):
        from qiskit_gym_amd.collector import mcts_backup

        mcts_backup(self.forest, self.logp, self.values, done=self.done if with_done else None, root=True)

    def pair(self):
        from qiskit_gym_amd.collector import mcts_backup, mcts_select

        out = mcts_select(self.forest, C, self.finished, *self.picked)
        assert all(o is p for o, p in zip(out, self.picked))
        mcts_backup(self.forest, self.logp, self.values, self.reward, self.done, *self.picked)

    def simulate(self, captured):
        if not captured:
            return self.pair()
        if self.graph is None:
            torch.cuda.synchronize()
            self.graph = torch.cuda.CUDAGraph()
            with torch.cuda.graph(self.graph):
                self.pair()
        self.graph.replay()


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
    """A search the test drives itself, `rounds`: the simulations before each rebase.  Returns what was seen."""
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
        check_invariants(only_trees(model, touched))
        for m in np.nonzero(touched)[0]:
            kept = env_src[m * cap : m * cap + model.n_nodes[m]] - m * cap
            seen["kept"] += len(kept)
            seen["dropped"] += int(sizes[m]) - len(kept)
        seen["untouched"] += M - int(np.sum(touched))
        if r == 0 and M > 4:  # the real envs move on: one more tree ends before the second rebase
            finished[M - 1] = 1
            dev.finished.copy_(torch.as_tensor(finished))
    return seen


def only_trees(f, rows):
    """The trees `rows` (a mask) of f as a forest of their own."""
    rows = np.nonzero(rows)[0]
    g = Forest(len(rows), f.cap - 1, f.A)
    for name in FIELDS:
        setattr(g, name, getattr(f, name)[rows].copy())
    return g
