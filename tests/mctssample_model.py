"""CPU restatement of `collector.mcts_decide` and of `BatchedSynthesis.solve(num_searches=S, num_mcts_searches=N, mcts_sampled=True)`: the
tree search of tests/mctsmodel.py on M * S trees, every move drawn from the root's visit counts, the best successful episode kept per
target.  TEST INFRASTRUCTURE ONLY; it shares no code with qiskit_gym_amd.

The rules, on top of those of mctsmodel.
  counts     For every action a with c = child[0, a]: n_a = visits[c] where 0 < c < n_nodes, 0 where c < 0.  A child index c >= 0 outside
             that range, n_nodes outside [1, cap] or a negative visits value ends the tree's work: no move (A), every count 0.
  most       The action of the greatest n_a among the expanded edges, the lowest among equals; A where the root has no child
             (`mctsmodel.decide`).
  draw       total = sum of the n_a.  total = 0: the answer of `most`.  Else r = (rng_draw(seed ^ 0x6D637473, tree, counter) * total) >> 64
             -- the counter RNG of tests/util.py, 0 <= r < total -- and the move is the lowest action a with n_0 + ... + n_a > r.  Integers
             only: action a is drawn for exactly n_a of the total values of r, an action without visits never.
  finished   A tree whose real env is final gets no move (A); its counts are those of its forest all the same.
  layout     Tree and real env e = m * S + s is search s of target m, S = max(1, num_searches); the draw of decision t has counter t.
  return     An env's return is the f32 sum, in step order, of the rewards of the steps it was live for.
  winner     Per target the successful search of the greatest f32 return, the lowest s among equals; the answer is that env's solution
             log, None where no search succeeded, `[]` for a target solved on arrival.
  stats      searches = S; targets = M; searches_solved = successful envs / (M * S); solved, mean_gates over the answers; steps and nodes as
             in mctsmodel, nodes over all M * S trees.
"""
from __future__ import annotations

from typing import List, Optional, Sequence

import numpy as np

from mctsmodel import F32, MARKER, Forest, MctsModel, decide
from util import rng_draw

STREAM = 0x6D637473
MASK64 = (1 << 64) - 1


def counts(f: Forest) -> np.ndarray:
    """int32 [M, A]: the visit counts of every root's actions; a row of zeros for a tree the rules refuse."""
    out = np.zeros((f.M, f.A), dtype=np.int32)
    for m in range(f.M):
        n = int(f.n_nodes[m])
        if not 1 <= n <= f.cap:
            continue
        row = np.zeros(f.A, dtype=np.int32)
        for a in range(f.A):
            c = int(f.child[m, 0, a])
            if c < 0:
                continue
            if c == 0 or c >= n or f.visits[m, c] < 0:
                row = None
                break
            row[a] = f.visits[m, c]
        if row is not None:
            out[m] = row
    return out


def refused(f: Forest) -> np.ndarray:
    """bool [M]: trees whose work the rules end (their counts are zero and they have no move)."""
    out = np.ones(f.M, dtype=bool)
    for m in range(f.M):
        n = int(f.n_nodes[m])
        if 1 <= n <= f.cap:
            c = f.child[m, 0]
            out[m] = bool(((c == 0) | (c >= n)).any()) or bool((f.visits[m, c[(c > 0) & (c < n)]] < 0).any())
    return out


def decide_most(f: Forest, finished: Optional[np.ndarray] = None) -> np.ndarray:
    """Per tree the most visited of the root's expanded actions, the lowest among equals; A without a child, for a refused or a finished tree."""
    bad = refused(f)
    move = np.full(f.M, f.A, dtype=np.int32)
    for m in np.nonzero(~bad)[0]:
        best = -1
        for a in range(f.A):
            c = int(f.child[m, 0, a])
            if c >= 0 and f.visits[m, c] > best:
                best, move[m] = int(f.visits[m, c]), a
    if not bad.any():
        assert (move == decide(f)).all()  # the rule of the deterministic search
    return move if finished is None else np.where(np.asarray(finished).astype(bool), f.A, move).astype(np.int32)


def draw_from(row: Sequence[int], d: int) -> Optional[int]:
    """The action the 64-bit draw `d` gives on the counts `row`; None where there is no visit."""
    total = int(sum(int(x) for x in row))
    if total == 0:
        return None
    r = (int(d) * total) >> 64
    acc = 0
    for a, x in enumerate(row):
        acc += int(x)
        if acc > r:
            return a
    raise AssertionError("r < total: some running sum exceeds it")


def decide_sampled(f: Forest, seed: int, counter: int, finished: Optional[np.ndarray] = None) -> np.ndarray:
    """Per tree the move drawn from its root's visit counts, int32 [M]."""
    n = counts(f)
    most = decide_most(f)
    draws = rng_draw((int(seed) ^ STREAM) & MASK64, np.arange(f.M, dtype=np.uint64), int(counter) & MASK64)
    out = np.zeros(f.M, dtype=np.int32)
    for m in range(f.M):
        a = draw_from(n[m], int(draws[m]))
        out[m] = most[m] if a is None else a
    return out if finished is None else np.where(np.asarray(finished).astype(bool), f.A, out).astype(np.int32)


class SampledMctsModel(MctsModel):
    """The whole sampled search on oracle envs: `MctsModel` on M * S trees, driven the same way -- `start`, N times `select` / `expand` /
    `backup`, then `decide`, which here draws."""

    def __init__(self, targets: Sequence, S: int, N: int, A: int, max_depth: int, seed: int = 0, C: float = 2 ** 0.5):
        self.targets_, self.S, self.seed = len(targets), int(S), int(seed)
        super().__init__([targets[e // self.S] for e in range(len(targets) * self.S)], N, A, max_depth, C)
        self.ret = np.zeros(self.M, dtype=F32)

    def decide(self) -> np.ndarray:
        move = decide_sampled(self.forest, self.seed, self.t, self.finished)
        self.node_counts += [int(n) for n, l in zip(self.forest.n_nodes, self.live) if l]
        for e, env in enumerate(self.real):
            if self.finished[e]:
                continue
            env.step(int(move[e]))  # A where the root has no child: no gate, the step counts all the same
            self.ret[e] = F32(self.ret[e] + F32(env.reward()))
            self.finished[e] = env.is_final()
        self.moves.append(move)
        t = self.t
        self.t = t + 1
        if (t % 8 == 7 and self.finished.all()) or self.t == self.T:
            self.ended = True
        return move

    def pick(self, ok: np.ndarray, ret: np.ndarray) -> Optional[int]:
        """The winner among a target's S searches: the greatest return of the successful ones, the lowest s among equals."""
        best = None
        for s in range(len(ok)):
            if ok[s] and (best is None or ret[s] > ret[best]):
                best = s
        return best

    def winners(self) -> List[Optional[int]]:
        ok = np.array([env.success() for env in self.real], dtype=bool).reshape(self.targets_, self.S)
        ret = self.ret.reshape(self.targets_, self.S)
        return [self.pick(ok[m], ret[m]) for m in range(self.targets_)]

    def result(self):
        assert self.ended
        sols = [None if s is None else [int(x) for x in self.real[m * self.S + s].solution()] for m, s in enumerate(self.winners())]
        gates = [sum(1 for x in s if x < MARKER) for s in sols if s is not None]
        stats = {"searches": self.S, "targets": self.targets_, "steps": self.t, "solved": len(gates),
                 "searches_solved": sum(env.success() for env in self.real) / self.M, "mean_gates": float(np.mean(gates)) if gates else 0.0,
                 "nodes": float(np.mean(self.node_counts)) if self.node_counts else 0.0}
        return sols, stats
