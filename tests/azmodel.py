"""CPU restatement of `collector.az_pack` (`qg_az_pack`) and of `BatchedSynthesis.self_play`: the sampled tree search of
tests/mctssample_model.py with every decision logged, and the log packed into training samples.  TEST INFRASTRUCTURE ONLY; it shares no
code with qiskit_gym_amd.

The pack rules (T decisions, E episodes, A actions).
  rows     total(t, e) = the sum of counts[t, e, :A] in Python integers.  A row is BAD if any count is negative or total >= 2^24.  It is
           VALID iff live != 0, it is not bad and total > 0.
  value    G(T, e) = 0; for t = T-1 .. 0: G(t, e) = f32(reward[t, e] + G(t+1, e)) where live, else G(t+1, e).  A live decision that is not
           valid still contributes its reward.
  order    The valid (t, e) in ascending t * E + e; the first `capacity` of them are written.
  sample   index = t * E + e; z = G(t, e); move as it stands; pi[a] = f32(counts[a]) / f32(total), one f32 division; the words copied.
  n        (min(valid, capacity), valid, live rows that are bad).
"""
from __future__ import annotations

from dataclasses import dataclass
from typing import List, Optional, Sequence

import numpy as np

from mctssample_model import SampledMctsModel, counts as root_counts

F32 = np.float32
TOTAL_LIMIT = 1 << 24


@dataclass
class Packed:
    n: np.ndarray          # int32 [3]
    index: np.ndarray      # int32 [n0]
    z: np.ndarray          # f32 [n0]
    move: np.ndarray       # int32 [n0]
    pi: np.ndarray         # f32 [n0, A]
    words: Optional[np.ndarray]  # [n0, W]


def returns_to_go(reward: np.ndarray, live: np.ndarray) -> np.ndarray:
    """f32 [T, E]: G(t, e) of the value rule, for every (t, e)."""
    T, E = reward.shape
    g = np.zeros(E, dtype=F32)
    out = np.zeros((T, E), dtype=F32)
    for t in range(T - 1, -1, -1):
        for e in range(E):
            if live[t, e] != 0:
                g[e] = F32(F32(reward[t, e]) + g[e])
        out[t] = g
    return out


def pack(counts: np.ndarray, reward: np.ndarray, live: np.ndarray, move: np.ndarray, words: Optional[np.ndarray] = None,
         capacity: Optional[int] = None) -> Packed:
    counts = np.asarray(counts)
    T, E, A = counts.shape
    capacity = T * E if capacity is None else int(capacity)
    assert capacity >= 1
    G = returns_to_go(np.asarray(reward, dtype=F32), np.asarray(live))
    index, z, mv, pi, ws = [], [], [], [], []
    valid = bad = 0
    for t in range(T):
        for e in range(E):
            if live[t, e] == 0:
                continue
            row = [int(c) for c in counts[t, e]]
            total = sum(row)
            if any(c < 0 for c in row) or total >= TOTAL_LIMIT:
                bad += 1
                continue
            if total == 0:
                continue
            valid += 1
            if valid > capacity:
                continue
            index.append(t * E + e)
            z.append(G[t, e])
            mv.append(move[t, e])
            pi.append(np.array([F32(c) / F32(total) for c in row], dtype=F32))
            if words is not None:
                ws.append(np.asarray(words)[t, e].copy())
    n0 = len(index)
    return Packed(np.array([n0, valid, bad], dtype=np.int32), np.array(index, dtype=np.int32), np.array(z, dtype=F32),
                  np.array(mv, dtype=np.int32), np.array(pi, dtype=F32).reshape(n0, A),
                  None if words is None else np.array(ws, dtype=np.asarray(words).dtype).reshape(n0, np.asarray(words).shape[2]))


class SelfPlayModel(SampledMctsModel):
    """`SampledMctsModel` that keeps, per decision, what `self_play` logs: the root counts, which episodes were live, the oracle envs' dense
    observation before the move, the reward of the real step and the move; `samples` packs them."""

    def __init__(self, targets: Sequence, S: int, N: int, A: int, max_depth: int, seed: int = 0, C: float = 2 ** 0.5):
        super().__init__(targets, S, N, A, max_depth, seed, C)
        self.log_counts: List[np.ndarray] = []
        self.log_live: List[np.ndarray] = []
        self.log_obs: List[np.ndarray] = []
        self.log_reward: List[np.ndarray] = []
        self.log_move: List[np.ndarray] = []

    def decide(self) -> np.ndarray:
        live = ~self.finished.copy()
        self.log_counts.append(root_counts(self.forest))
        self.log_live.append(live.astype(np.uint8))
        self.log_obs.append(np.stack([env.dense_obs().reshape(-1) for env in self.real]))
        move = super().decide()
        # a finished env is not stepped: whatever its reward entry holds is never read (live = 0)
        self.log_reward.append(np.array([F32(env.reward()) if l else F32(0) for env, l in zip(self.real, live)], dtype=F32))
        self.log_move.append(move.copy())
        return move

    def samples(self, capacity: Optional[int] = None) -> Packed:
        assert self.ended
        return pack(np.stack(self.log_counts), np.stack(self.log_reward), np.stack(self.log_live), np.stack(self.log_move), capacity=capacity)

    def lengths(self) -> np.ndarray:
        return np.stack(self.log_live).astype(np.int32).sum(axis=0).astype(np.int32)

    def observation(self, index: int) -> np.ndarray:
        """The dense observation, flat int8, before the move of sample `index` = t * E + e."""
        t, e = divmod(int(index), self.M)
        return self.log_obs[t][e]
