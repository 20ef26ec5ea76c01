"""CPU restatement of `collector.mcts_select_many` / `collector.mcts_backup_many` and of `BatchedSynthesis.solve(num_mcts_searches=N,
mcts_leaves=K)`: the tree searches of tests/mctsmodel.py, mctssample_model.py and mctsreuse_model.py with K descents per tree in one round
of launches.  TEST INFRASTRUCTURE ONLY; it shares no code with qiskit_gym_amd.

The rules, on top of those of the three models (include/qgym.h states them for the kernels).
  layout      stride = K; entry m * stride + i of src, dst, act, leaf, values, reward, done and row m * stride + i of the priors belong to
              descent i of tree m.
  select      Per tree n0 = n_nodes at entry and an OVERLAY, a copy of its (visits, wsum).  Descents i = 0 .. k - 1 in that order, each the
              descent of `mctsreuse_model.select` (scores, f32 order, ties, terminal rule, the full tree) with: visits and wsum read from
              the overlay; an edge (x, a) that an earlier descent of the call chose for expansion is no candidate (a NaN score) -- with none
              left, leaf = x, act = A, the simulation counts; the e-th expanding descent names node n0 + e, refused like a full tree where
              that is >= cap (leaf = -1, act = A, dst = M * cap, src the node it stood on; its edge is not pending).  After a descent every
              node y it stood on gets overlay visits[y] += 1 and, y != 0, overlay wsum[y] = f32(wsum[y] - virtual_loss); so does a descent
              refused for a full tree.
  checks      A child index c >= 0 of the node a descent stands on (pending edges aside) with c >= n0 or c <= x ends the tree's work:
              that descent gets leaf = -1 with src the node it stood on, the later ones are not made.  A descent that is not made -- after
              such a failure, i in [k, stride), a finished tree, n0 outside [1, cap] -- is src = m * cap, dst = M * cap, act = A, leaf = -1.
  backup      Per tree, i = 0 .. k - 1 in that order, the backup rule with the kernel's checks on entry m * stride + i; an entry that fails
              one is skipped, later ones go on; n_nodes grows as nodes are linked.  n_nodes outside [1, cap] at entry skips the tree.
  search      A decision makes R = ceil(N / K) rounds; round r makes k_r = min(K, N - r K) descents: select, expand (K envs per tree, env
              m * K + i a clone of src's stepped with act; None where act = A), one evaluation, backup.  Everything else -- root, decision,
              draw, rebase -- is the underlying model's.
  stats       leaves = K; rounds = R; idle = the (tree, round, i < k_r) triples with leaf < 0 whose real env was not final (with
              `reuse_tree` that is also "refused").
"""
from __future__ import annotations

from typing import List, Optional

import numpy as np

from mctsmodel import F32, Forest, MctsModel, best_action, run_alone, scores  # noqa: F401  (`run_alone`: the one driver, for every model)
from mctsreuse_model import _Reuse
from mctssample_model import SampledMctsModel

MAX_LEAVES = 64


class _Overlay:
    """What `mctsmodel.scores` reads of a forest, with visits and wsum of tree m replaced by the call's copies."""

    def __init__(self, f: Forest, m: int):
        self.child, self.prior, self.value = f.child, f.prior, f.value
        self.visits, self.wsum = f.visits.copy(), f.wsum.copy()  # (only tree m's rows are ever touched)


def select_many(f: Forest, C: float, k: int, stride: int, virtual_loss: float = 0.0, finished: Optional[np.ndarray] = None, overlays: Optional[list] = None):
    """int32 [M * stride] each: src, dst, act, leaf.  `overlays`: a list that gets, per tree, the overlay's visits row after the call (None
    for a tree that made no descent)."""
    assert 1 <= k <= stride <= MAX_LEAVES and np.isfinite(virtual_loss) and virtual_loss >= 0
    M, A, cap = f.M, f.A, f.cap
    src = np.repeat(np.arange(M, dtype=np.int32) * cap, stride)
    dst = np.full(M * stride, f.skip, dtype=np.int32)
    act, leaf = np.full(M * stride, A, dtype=np.int32), np.full(M * stride, -1, dtype=np.int32)
    vl = F32(virtual_loss)
    for m in range(M):
        n0 = int(f.n_nodes[m])
        if (finished is not None and finished[m]) or not 1 <= n0 <= cap:
            if overlays is not None:
                overlays.append(None)
            continue
        o = _Overlay(f, m)
        pending, grown = set(), 0
        for i in range(k):
            e = m * stride + i
            x, path, broken = 0, [], False
            while True:
                path.append(x)
                if f.terminal[m, x]:
                    leaf[e] = x
                    break
                c = f.child[m, x]
                mine = np.zeros(A, dtype=bool)
                mine[np.array([pa for px, pa in pending if px == x], dtype=np.int64)] = True
                if ((c >= 0) & ~mine & ((c >= n0) | (c <= x))).any():
                    broken = True
                    break
                sc = scores(o, m, x, C)
                sc[mine] = np.nan
                a = best_action(sc)
                if a is None:
                    leaf[e] = x
                    break
                if c[a] < 0:
                    j = n0 + grown
                    if j < cap:
                        leaf[e], dst[e], act[e] = j, m * cap + j, a
                        pending.add((x, a))
                        grown += 1
                    break
                x = int(c[a])
            src[e] = m * cap + x
            if broken:
                break
            for y in path:
                o.visits[m, y] += 1
                if y != 0:
                    o.wsum[m, y] = F32(o.wsum[m, y] - vl)
        if overlays is not None:
            overlays.append(o.visits[m].copy())
    return src, dst, act, leaf


def backup_many(f: Forest, k: int, stride: int, src, dst, act, leaf, prior, values, reward, done) -> np.ndarray:
    """prior: f32 [M * stride, >= A], exp(logp) as the device computed it; values, reward f32 [M * stride]; done [M * stride].  Returns the
    number of nodes linked per tree."""
    assert 1 <= k <= stride <= MAX_LEAVES
    M, A, cap = f.M, f.A, f.cap
    linked = np.zeros(M, dtype=np.int64)
    for m in range(M):
        n = int(f.n_nodes[m])
        if not 1 <= n <= cap:
            continue
        for i in range(k):
            e = m * stride + i
            lf, a = int(leaf[e]), int(act[e])
            if lf < 0:
                continue
            if 0 <= a < A:
                x, j = int(src[e]) - m * cap, int(dst[e]) - m * cap
                if x < 0 or x >= n or j != n or j >= cap or lf != j or f.child[m, x, a] != -1:
                    continue
                term = bool(done[e])
                f.child[m, x, a] = j
                f.parent[m, j] = x
                f.reward[m, j] = F32(reward[e])
                f.terminal[m, j] = term
                f.value[m, j] = F32(0) if term else F32(values[e])
                f.prior[m, j] = np.asarray(prior[e], dtype=F32)[:A]
                f.child[m, j] = -1
                f.visits[m, j] = 0
                f.wsum[m, j] = 0
                n += 1
                f.n_nodes[m] = n
                linked[m] += 1
            elif lf >= n:
                continue
            g, y, whole = F32(f.value[m, lf]), lf, True
            for _ in range(cap):
                if y == 0:
                    break
                up = int(f.parent[m, y])
                g = F32(f.reward[m, y] + g)
                f.visits[m, y] += 1
                f.wsum[m, y] = F32(f.wsum[m, y] + g)
                if up < 0 or up >= y:
                    whole = False
                    break
                y = up
            if whole and y == 0:
                f.visits[m, 0] += 1
    return linked


class _Many:
    """What the searches with K leaves per round share; in front of the model it extends in the bases.  Driven like that model, with
    `rounds` select / expand / backup triples per decision in place of N, on M * K entries."""

    def __init__(self, *args, leaves: int = 1, virtual_loss: float = 0.0, **kw):
        super().__init__(*args, **kw)
        self.K, self.vl = int(leaves), float(virtual_loss)
        assert 1 <= self.K <= min(self.N, MAX_LEAVES)
        self.rounds = -(-self.N // self.K)
        self.round = 0  # within the decision
        self.idle = 0
        self.per_round: List[int] = []  # k_r of every round made

    def k_of(self, r: int) -> int:
        return min(self.K, self.N - r * self.K)

    def select(self):
        k = self.k_of(self.round)
        assert k >= 1, "a decision makes ceil(N / K) rounds"
        self.picked = select_many(self.forest, self.C, k, self.K, self.vl, self.finished)
        missed = int(((self.picked[3].reshape(self.M, self.K)[:, :k] < 0) & ~self.finished[:, None]).sum())
        self.idle += missed
        if hasattr(self, "refused"):
            self.refused += missed
        self.per_round.append(k)
        return self.picked

    def expand(self) -> list:
        src, dst, act, leaf = self.picked
        self.fresh = []
        for e in range(self.M * self.K):
            if act[e] >= self.A:
                self.fresh.append(None)
                continue
            m = e // self.K
            env = self.pool[m][int(src[e]) - m * self.forest.cap].clone()
            env.step(int(act[e]))
            self.fresh.append(env)
        return self.fresh

    def backup(self, prior: np.ndarray, values: np.ndarray):
        src, dst, act, leaf = self.picked
        k = self.per_round[-1]
        reward = np.array([F32(0) if e is None else F32(e.reward()) for e in self.fresh], dtype=F32)
        done = np.array([False if e is None else e.is_final() for e in self.fresh], dtype=bool)
        for e, env in enumerate(self.fresh):
            if env is not None:
                self.pool[e // self.K][int(leaf[e])] = env
        backup_many(self.forest, k, self.K, src, dst, act, leaf, prior, values, reward, done)
        self.sims += (leaf.reshape(self.M, self.K)[:, :k] >= 0).sum(axis=1)
        self.round += 1
        return reward, done

    def decide(self) -> np.ndarray:
        assert self.round == self.rounds
        move = super().decide()
        self.round = 0
        return move

    def result(self):
        sols, stats = super().result()
        stats.update(leaves=self.K, rounds=self.rounds, idle=self.idle)
        return sols, stats


class ManyMctsModel(_Many, MctsModel):
    """`MctsModel(targets, N, A, max_depth, C)` with `leaves=`, `virtual_loss=`."""


class ManySampledMctsModel(_Many, SampledMctsModel):
    """`SampledMctsModel(targets, S, N, A, max_depth, seed, C)` with `leaves=`, `virtual_loss=`."""


class ManyReuseMctsModel(_Many, _Reuse, MctsModel):
    """`ReuseMctsModel` with `leaves=`, `virtual_loss=`."""


class ManyReuseSampledMctsModel(_Many, _Reuse, SampledMctsModel):
    """`ReuseSampledMctsModel` with `leaves=`, `virtual_loss=`."""
