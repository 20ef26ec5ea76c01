"""CPU restatement of the PUCT search of `BatchedSynthesis.solve(num_mcts_searches=N, deterministic=True)` and of its two device kernels
(`collector.mcts_select`, `collector.mcts_backup`): numpy f32 for the tree, `OracleEnv.clone` for the envs.  TEST INFRASTRUCTURE ONLY; it
shares no code with qiskit_gym_amd.

The rules.
  layout     M targets, one tree per target, rebuilt for every decision; cap = N + 1 nodes.  Node 0 is the root, a clone of the target's real
             env.  Per (tree, node): parent (int32, -1 for the root), reward (f32, of the step into the node), value (f32, the value head at
             the node, 0 for a terminal node), visits (int32), wsum (f32), terminal (uint8, the env's `is_final`).  Per (tree, node, action):
             child (int32, -1 = not expanded), prior (f32).  Per tree: n_nodes.  Node j of tree m has pool index m * cap + j.
  root       From the policy's answer about the real envs: prior[0, a] = exp(logp[a]) (f32), value[0] (0 if the root is terminal),
             visits[0] = 1, every child[0, a] = -1, parent[0] = -1, reward[0] = wsum[0] = 0, n_nodes = 1.
  selection  One descent per simulation and tree, from node 0.  At a terminal node x it ends there and nothing is expanded.  Else for every
             action a, with c = child[x, a]:   Q = wsum[c] / f32(visits[c]) where c >= 0, else value[x];   n_a = visits[c] where c >= 0, else 0;
             U = ((C * prior[x, a]) * sqrt(f32(visits[x]))) / f32(1 + n_a);   score = Q + U -- every operation one f32 operation, in
             that order.  The greatest score wins (-0 = +0), ties go to the lowest action, a NaN is no candidate.  An unexpanded winner ends
             the descent with (x, a), the new node is n_nodes; else the descent goes on at the child.  Outputs: src = pool index of x; dst =
             pool index of the new node, or M * cap where nothing is expanded; act = a, or A where nothing is expanded; leaf = the node the
             backup starts from (the new node; x where nothing is expanded), or -1 for a tree whose real env is finished: no simulation.
  expansion  The new node's env is a clone of x's, stepped with a; the policy is asked about it.
  backup     Where a node was expanded: child[x, a] = j, parent[j] = x, reward[j], terminal[j], value[j] (0 if terminal), prior[j] =
             exp(logp), child[j] = -1, visits[j] = 0, wsum[j] = 0, n_nodes += 1.  Then G = value[leaf]; every node y != 0 from the leaf
             towards the root gets G = reward[y] + G (one f32 addition), visits[y] += 1, wsum[y] += G; the root gets visits[0] += 1.
  decision   After N simulations the move is the root's expanded action with the most visits, the lowest among equals (A: the root has
             no child).  The real env takes it.  A tree whose real env is final -- or solved on arrival -- gets no gate from then on.
  end        After `max_depth` decisions, or after the first decision t with t % 8 == 7 and every real env final.
  answer     The real env's solution log where it ended in success, else None; `[]` for a target solved on arrival.
  stats      steps = decisions made; solved; mean_gates over the answers (log entries below the rotation marker; 0.0 without any); nodes =
             mean n_nodes, after the N simulations, over the (tree, decision) pairs whose real env was not final.
"""
from __future__ import annotations

from typing import Callable, List, Optional, Sequence

import numpy as np

MARKER = 0x80000000
F32 = np.float32
FIELDS = ("parent", "reward", "value", "visits", "wsum", "terminal", "child", "prior", "n_nodes")


class Forest:
    def __init__(self, M: int, N: int, A: int):
        self.M, self.N, self.A, self.cap = int(M), int(N), int(A), int(N) + 1
        M, cap = self.M, self.cap
        self.parent = np.zeros((M, cap), dtype=np.int32)
        self.reward = np.zeros((M, cap), dtype=F32)
        self.value = np.zeros((M, cap), dtype=F32)
        self.visits = np.zeros((M, cap), dtype=np.int32)
        self.wsum = np.zeros((M, cap), dtype=F32)
        self.terminal = np.zeros((M, cap), dtype=np.uint8)
        self.child = np.zeros((M, cap, A), dtype=np.int32)
        self.prior = np.zeros((M, cap, A), dtype=F32)
        self.n_nodes = np.zeros(M, dtype=np.int32)

    @property
    def skip(self) -> int:
        return self.M * self.cap


def root(f: Forest, prior: np.ndarray, values: np.ndarray, done: Optional[np.ndarray] = None):
    """Start every tree.  prior: f32 [M, >= A], exp(logp) as the device computed it (so expf is no source of divergence)."""
    done = np.zeros(f.M, dtype=bool) if done is None else np.asarray(done).astype(bool)
    f.prior[:, 0, :] = np.asarray(prior, dtype=F32)[:, : f.A]
    f.child[:, 0, :] = -1
    f.parent[:, 0] = -1
    f.reward[:, 0] = 0
    f.wsum[:, 0] = 0
    f.value[:, 0] = np.where(done, F32(0), np.asarray(values, dtype=F32))
    f.visits[:, 0] = 1
    f.terminal[:, 0] = done
    f.n_nodes[:] = 1


def scores(f: Forest, m: int, x: int, C: float) -> np.ndarray:
    """The PUCT scores of node x of tree m, f32 [A]."""
    c = f.child[m, x]
    ex = c >= 0
    cc = np.where(ex, c, 0)
    vis = f.visits[m, cc]
    with np.errstate(all="ignore"):
        q = np.where(ex, f.wsum[m, cc] / vis.astype(F32), f.value[m, x]).astype(F32)
        n_a = np.where(ex, vis, 0).astype(np.int32)
        u = ((F32(C) * f.prior[m, x]) * np.sqrt(F32(f.visits[m, x]))) / (1 + n_a).astype(F32)
        out = q + u
    assert out.dtype == F32 and u.dtype == F32
    return out


def best_action(score: np.ndarray) -> Optional[int]:
    """The greatest score, the lowest action among equals; a NaN is no candidate.  None without a candidate."""
    score = np.asarray(score, dtype=F32)
    valid = score == score
    if not valid.any():
        return None
    top = score[valid].max()
    return int(np.nonzero(score == top)[0][0])  # -0 == +0 as floats: a tie; a NaN equals nothing


def select(f: Forest, C: float, finished: Optional[np.ndarray] = None):
    src, dst = np.zeros(f.M, dtype=np.int32), np.full(f.M, f.skip, dtype=np.int32)
    act, leaf = np.full(f.M, f.A, dtype=np.int32), np.full(f.M, -1, dtype=np.int32)
    for m in range(f.M):
        src[m] = m * f.cap
        if finished is not None and finished[m]:
            continue
        x = 0
        while True:
            if f.terminal[m, x]:
                leaf[m] = x
                break
            a = best_action(scores(f, m, x, C))
            if a is None:
                leaf[m] = x
                break
            c = int(f.child[m, x, a])
            if c < 0:
                j = int(f.n_nodes[m])
                assert j < f.cap, "a tree never holds more than N + 1 nodes"
                leaf[m], dst[m], act[m] = j, m * f.cap + j, a
                break
            x = c
        src[m] = m * f.cap + x
    return src, dst, act, leaf


def backup(f: Forest, src, dst, act, leaf, prior, values, reward, done):
    """prior: f32 [M, >= A], exp(logp) of the expanded envs; values, reward f32 [M]; done [M].  Rows of trees that expanded nothing are not read."""
    for m in range(f.M):
        lf = int(leaf[m])
        if lf < 0:
            continue
        if act[m] < f.A:
            x, j, a = int(src[m]) - m * f.cap, int(dst[m]) - m * f.cap, int(act[m])
            assert j == f.n_nodes[m] == lf and f.child[m, x, a] == -1
            term = bool(done[m])
            f.child[m, x, a] = j
            f.parent[m, j] = x
            f.reward[m, j] = F32(reward[m])
            f.terminal[m, j] = term
            f.value[m, j] = F32(0) if term else F32(values[m])
            f.prior[m, j] = np.asarray(prior[m], dtype=F32)[: f.A]
            f.child[m, j] = -1
            f.visits[m, j] = 0
            f.wsum[m, j] = 0
            f.n_nodes[m] += 1
        g, y = F32(f.value[m, lf]), lf
        while y != 0:
            g = F32(f.reward[m, y] + g)
            f.visits[m, y] += 1
            f.wsum[m, y] = F32(f.wsum[m, y] + g)
            y = int(f.parent[m, y])
        f.visits[m, 0] += 1


def decide(f: Forest) -> np.ndarray:
    """Per tree the root's expanded action with the most visits, the lowest among equals; A where the root has no child."""
    out = np.full(f.M, f.A, dtype=np.int32)
    for m in range(f.M):
        best = -1
        for a in range(f.A):
            c = int(f.child[m, 0, a])
            if c >= 0 and f.visits[m, c] > best:
                best, out[m] = int(f.visits[m, c]), a
    return out


def check_invariants(f: Forest, sims: Optional[Sequence[int]] = None):
    """What every tree satisfies between two simulations; `sims[m]`: the simulations tree m has made."""
    for m in range(f.M):
        n = int(f.n_nodes[m])
        assert 1 <= n <= f.cap
        if sims is not None:
            assert f.visits[m, 0] == 1 + sims[m], (m, f.visits[m, 0], sims[m])
        for x in range(n):
            kids = [int(c) for c in f.child[m, x] if c >= 0]
            assert all(x < c < n and f.parent[m, c] == x for c in kids) and len(set(kids)) == len(kids)
            if f.terminal[m, x]:
                assert not kids and f.value[m, x] == 0
            else:
                assert f.visits[m, x] == 1 + sum(int(f.visits[m, c]) for c in kids), (m, x)


class MctsModel:
    """The whole search on oracle envs.  Driven step by step -- `start`, then `rounds` times `select` / `expand` / `backup`, then `decide`
    -- with the policy's numbers handed in, so a device's own can be used; `run_alone` drives it with a function.  Here a round is one
    descent per tree (K = 1, no virtual loss) and the trees are rebuilt for every decision; the mix-ins of mctsmany_model and
    mctsreuse_model change either."""
    carries = False  # True: the chosen move's subtree is kept between decisions, so `start` is for decision 0 only

    def __init__(self, targets: Sequence, N: int, A: int, max_depth: int, C: float = 2 ** 0.5):
        self.real = [t.clone() for t in targets]  # track_solution on
        self.M, self.N, self.A, self.T, self.C = len(self.real), int(N), int(A), int(max_depth), float(C)
        self.finished = np.array([env.success() for env in self.real], dtype=bool)
        self.K, self.vl, self.rounds = 1, 0.0, self.N
        self.forest = Forest(self.M, self.N, self.A)
        self.pool: List[dict] = [{} for _ in range(self.M)]  # per tree: node -> env
        self.t = 0
        self.ended = self.T == 0
        self.moves: List[np.ndarray] = []
        self.node_counts: List[int] = []
        self.picked = self.fresh = None

    def k_of(self, r: int) -> int:
        """The descents per tree of round r."""
        return 1

    def roots(self) -> list:
        """The envs the policy is asked about at the start of a decision: the real ones."""
        return self.real

    def start(self, prior: np.ndarray, values: np.ndarray):
        assert not self.ended
        self.pool = [{0: env.clone()} for env in self.real]
        self.live = ~self.finished
        self.sims = np.zeros(self.M, dtype=np.int64)
        root(self.forest, prior, values, self.finished)

    def select(self):
        self.picked = select(self.forest, self.C, self.finished)
        return self.picked

    def expand(self) -> list:
        """The new nodes' envs (None where nothing is expanded): clones of the source nodes', stepped."""
        src, dst, act, leaf = self.picked
        self.fresh = []
        for m in range(self.M):
            if act[m] >= self.A:
                self.fresh.append(None)
                continue
            env = self.pool[m][int(src[m]) - m * self.forest.cap].clone()
            env.step(int(act[m]))
            self.fresh.append(env)
        return self.fresh

    def backup(self, prior: np.ndarray, values: np.ndarray):
        src, dst, act, leaf = self.picked
        reward = np.array([F32(0) if e is None else F32(e.reward()) for e in self.fresh], dtype=F32)
        done = np.array([False if e is None else e.is_final() for e in self.fresh], dtype=bool)
        for m, env in enumerate(self.fresh):
            if env is not None:
                self.pool[m][int(leaf[m])] = env
        backup(self.forest, src, dst, act, leaf, prior, values, reward, done)
        self.sims += leaf >= 0
        return reward, done

    def decide(self) -> np.ndarray:
        move = np.where(self.finished, self.A, decide(self.forest)).astype(np.int32)
        self.node_counts += [int(n) for n, l in zip(self.forest.n_nodes, self.live) if l]
        for m, env in enumerate(self.real):
            if move[m] < self.A:
                env.step(int(move[m]))
                self.finished[m] = env.is_final()
        self.moves.append(move)
        t = self.t
        self.t = t + 1
        if (t % 8 == 7 and self.finished.all()) or self.t == self.T:
            self.ended = True
        return move

    def result(self):
        assert self.ended
        sols = [[int(x) for x in env.solution()] if env.success() else None for env in self.real]
        gates = [sum(1 for x in s if x < MARKER) for s in sols if s is not None]
        stats = {"steps": self.t, "solved": len(gates), "mean_gates": float(np.mean(gates)) if gates else 0.0,
                 "nodes": float(np.mean(self.node_counts)) if self.node_counts else 0.0}
        return sols, stats


def run_alone(model: MctsModel, evaluate: Callable, after_simulation: Optional[Callable] = None, after_decision: Optional[Callable] = None):
    """The model as its own device, whichever of the family.  `evaluate(envs) -> (logp f32 [len, A], values f32 [len])` for a list of oracle
    envs (None entries get any row); a model with carried trees is asked about its roots at decision 0 only.  `after_simulation(model)` is
    called after every backup -- every round, where a round makes several descents -- and `after_decision(model, move)` after every
    decision and its rebase."""
    def priors(envs):
        logp, values = evaluate(envs)
        return np.exp(np.asarray(logp, dtype=F32)).astype(F32), np.asarray(values, dtype=F32)

    while not model.ended:
        if model.t == 0 or not model.carries:
            model.start(*priors(model.roots()))
        for _ in range(model.rounds):
            model.select()
            model.backup(*priors(model.expand()))
            if after_simulation is not None:
                after_simulation(model)
        move = model.decide()
        if after_decision is not None:
            after_decision(model, move)
    return model.result()
