"""CPU restatement of `collector.mcts_rebase` and of `BatchedSynthesis.solve(num_mcts_searches=N, reuse_tree=True)`: the tree searches of
tests/mctsmodel.py and tests/mctssample_model.py with the chosen move's subtree kept between decisions.  TEST INFRASTRUCTURE ONLY; it
shares no code with qiskit_gym_amd.

The rules, on top of those of mctsmodel and mctssample_model.
  capacity   A tree has room for cap nodes, N + 1 <= cap <= 8192, min(2 N + 1, 8192) by default: `Forest(M, cap - 1, A)`.
  full       A descent that ends on an unexpanded edge of a tree with n_nodes = cap expands nothing and does not count: leaf = -1, act = A,
             dst = M * cap, src the node it stood on.  The backup leaves such a tree alone.
  rebase     After every decision, per tree m with n = n_nodes[m], a = move[m], none = M * cap; env_src is int32 [M * cap]:
    finished       the real env is final (after its step): the forest is untouched, env_src[m * cap + j] = none for every j < cap.
    nothing        n outside [1, cap], a outside [0, A) or c = child[0, a] outside (0, n): the forest is untouched, env_src is the identity
                   m * cap + j for j < min(n, cap) (no j where n < 1) and none for every other j.
    kept           else node c is kept, and a node j with c < j < n iff the chain j -> parent[j] -> ... reaches c exactly, every link
                   strictly below the one before it and >= 0.  A chain that breaks or passes below c keeps nothing; no node <= c but c.
    renumbering    the new index j' of a kept node is the number of kept nodes below j.
    fields         reward, value, visits, wsum, terminal and the prior row move unchanged to j'; parent[j'] is the new index of the old
                   parent; a child entry c2 becomes its new index where 0 <= c2 < n and c2 is kept, else -1.  The new root gets parent = -1,
                   reward = 0 and wsum = 0 and keeps the rest, its visits above all.
    sizes          n_nodes[m] = the kept nodes; env_src[m * cap + j'] = m * cap + j for every kept node, none for j' >= n_nodes.  Entries
                   at node indices >= the new n_nodes mean nothing (the model leaves there what was there).
  search     Decision 0 starts the trees as ever.  Every decision makes N simulations, decides, steps the real envs, rebases with the real
             envs' new `finished` and re-keys every tree's node envs by env_src; decisions t >= 1 start from the carried tree: no root call.
  stats      reuse = True; capacity = cap; carried = mean n_nodes right after the rebase over the trees whose real env is not final (0.0
             without any); refused = the (tree, simulation) pairs with leaf < 0 whose real env was not final; nodes as in mctsmodel.
"""
from __future__ import annotations

from typing import List, Optional

import numpy as np

from mctsmodel import F32, Forest, MctsModel, best_action, run_alone, scores  # noqa: F401  (`run_alone`: the one driver, for every model)
from mctssample_model import SampledMctsModel

MAX_CAP = 8192


def select(f: Forest, C: float, finished: Optional[np.ndarray] = None):
    """`mctsmodel.select` with the rule for a full tree."""
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
                if j < f.cap:
                    leaf[m], dst[m], act[m] = j, m * f.cap + j, a
                break
            x = c
        src[m] = m * f.cap + x
    return src, dst, act, leaf


def kept_nodes_by_walk(f: Forest, m: int, c: int) -> List[int]:
    """The nodes of tree m that hang below c, c first, ascending: the rule as it is stated, every node's chain walked to its end."""
    n = int(f.n_nodes[m])
    out = [c]
    for j in range(c + 1, n):
        y = j
        for _ in range(f.cap):
            p = int(f.parent[m, y])
            if p < 0 or p >= y or p < c:
                break
            if p == c:
                out.append(j)
                break
            y = p
    return out


def kept_nodes(f: Forest, m: int, c: int) -> List[int]:
    """`kept_nodes_by_walk` without the walks.  The chain of j goes on at p = parent[j] where c < p < j, and from there it is the chain of
    p, a node settled before j: j is kept iff p is c, or c < p < j and p is kept.  A chain of thousands of nodes costs one step per node
    here and a walk of its whole length per node there; tests/test_mctsreuse_model.py holds the two together."""
    n = int(f.n_nodes[m])
    parent = f.parent[m, :n].tolist()
    kept = [False] * n
    kept[c] = True
    for j in range(c + 1, n):
        p = parent[j]
        kept[j] = c <= p < j and kept[p]  # (p == c: kept[c]; below c, at or above j, negative: the chain breaks)
    return [j for j in range(c, n) if kept[j]]


def carried_child(f: Forest, m: int, a: int) -> Optional[int]:
    """The node that becomes the root of tree m under move a; None where there is nothing to carry."""
    n = int(f.n_nodes[m])
    if not 1 <= n <= f.cap or not 0 <= a < f.A:
        return None
    c = int(f.child[m, 0, a])
    return c if 0 < c < n else None


def rebase(f: Forest, move, finished=None) -> np.ndarray:
    """In place on `f`; returns env_src, int32 [M * cap]."""
    none, cap = f.skip, f.cap
    env_src = np.full(f.M * cap, none, dtype=np.int32)
    for m in range(f.M):
        if finished is not None and finished[m]:
            continue
        n = int(f.n_nodes[m])
        c = carried_child(f, m, int(move[m]))
        if c is None:
            for j in range(max(0, min(n, cap))):
                env_src[m * cap + j] = m * cap + j
            continue
        kept = kept_nodes(f, m, c)
        new = {j: i for i, j in enumerate(kept)}
        old = {name: getattr(f, name)[m].copy() for name in ("parent", "reward", "value", "visits", "wsum", "terminal", "child", "prior")}
        for j, i in new.items():
            for name in ("reward", "value", "visits", "wsum", "terminal", "prior"):
                getattr(f, name)[m, i] = old[name][j]
            f.parent[m, i] = new[int(old["parent"][j])] if i else -1
            f.child[m, i] = [new.get(int(c2), -1) if 0 <= c2 < n else -1 for c2 in old["child"][j]]
            env_src[m * cap + i] = m * cap + j
        f.reward[m, 0] = F32(0)
        f.wsum[m, 0] = F32(0)
        f.n_nodes[m] = len(kept)
    return env_src


class _Reuse:
    """What both searches share; in front of `MctsModel` / `SampledMctsModel` in the bases."""
    carries = True

    def __init__(self, *args, cap: Optional[int] = None, **kw):
        super().__init__(*args, **kw)
        self.cap = min(2 * self.N + 1, MAX_CAP) if cap is None else int(cap)
        assert self.N + 1 <= self.cap <= MAX_CAP
        self.forest = Forest(self.M, self.cap - 1, self.A)
        self.refused = 0
        self.carried: List[int] = []
        self.env_srcs: List[np.ndarray] = []

    def start(self, prior, values):
        assert self.t == 0, "a root call at decision 0 only: later decisions start from the carried tree"
        super().start(prior, values)

    def select(self):
        self.picked = select(self.forest, self.C, self.finished)
        self.refused += int(((self.picked[3] < 0) & ~self.finished).sum())
        return self.picked

    def decide(self) -> np.ndarray:
        move = super().decide()  # steps the real envs: `finished` is the array after the step
        f = self.forest
        env_src = rebase(f, move, self.finished)
        for m in range(self.M):
            if self.finished[m]:
                continue  # nothing is copied
            row = env_src[m * f.cap : (m + 1) * f.cap]
            self.pool[m] = {i: self.pool[m][int(s) - m * f.cap] for i, s in enumerate(row) if s != f.skip}
            assert sorted(self.pool[m]) == list(range(int(f.n_nodes[m])))
        self.env_srcs.append(env_src)
        self.carried += [int(n) for n, fin in zip(f.n_nodes, self.finished) if not fin]
        self.live = ~self.finished  # the next decision's
        self.sims = np.zeros(self.M, dtype=np.int64)
        return move

    def result(self):
        sols, stats = super().result()
        stats.update(reuse=True, capacity=self.cap, carried=float(np.mean(self.carried)) if self.carried else 0.0, refused=self.refused)
        return sols, stats


class ReuseMctsModel(_Reuse, MctsModel):
    """`MctsModel(targets, N, A, max_depth, C)` with `cap=`: the deterministic search, trees carried."""


class ReuseSampledMctsModel(_Reuse, SampledMctsModel):
    """`SampledMctsModel(targets, S, N, A, max_depth, seed, C)` with `cap=`: the sampled search, trees carried."""
