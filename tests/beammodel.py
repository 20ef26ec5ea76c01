"""CPU restatement of the beam search of `BatchedSynthesis.solve(..., beam_width=W)`: numpy f32 for the score addition and the ordering
(the rules in the comment of `qg_beam_select`, include/qgym.h), `OracleEnv.clone` for the envs.  TEST INFRASTRUCTURE ONLY; it shares no code
with qiskit_gym_amd.

The rules.  The batch is M groups (targets) of W slots; group g owns slots g*W .. g*W + W-1.
  selection  A candidate is (live slot b, action a < A) with score f32(cum[b]) + f32(logp[b, a]), one f32 addition.  NaN and -inf scores
             do not exist.  A group's candidates are ordered by score descending (-0 = +0), ties by slot, then by action, ascending.  Output
             slot j of the group gets candidate j: parent = its slot's batch-wide index, its action, its score, live = 1; the slots past the
             last candidate get parent = their own index, action = A, score = -inf, live = 0.
  search     Every slot of group g starts as a clone of target g; only slot 0 is live, unless the target is solved on arrival: then no slot
             is, and the target's result is the empty solution with return 0.  Per step: select; slot j becomes a clone of its parent,
             stepped with its action; its return is f32(parent's return) + f32(reward of the step).  A live slot whose env is final leaves
             the search; if it ended with success it is a result.  Per group the best result of the step (return descending, then slot
             ascending) replaces the group's winner if its return is strictly greater.  The search ends when no slot is live, or after
             `max_steps` steps.  A group's answer is its winner's solution log, or None without a winner.
"""
from __future__ import annotations

from typing import Callable, List, Optional, Sequence

import numpy as np

NEG_INF = np.float32(-np.inf)


def select(logp: np.ndarray, cum: np.ndarray, live: np.ndarray, W: int, A: int):
    """logp: [B, >= A] float32 (a bf16 / f16 input is passed widened, which is exact); cum: [B] float32; live: [B] bool or 0/1.
    Returns (parent int64 [B], actions int64 [B], cum_out float32 [B], live_out uint8 [B])."""
    logp = np.asarray(logp, dtype=np.float32)
    cum = np.asarray(cum, dtype=np.float32)
    live = np.asarray(live).astype(bool)
    B = logp.shape[0]
    assert B % W == 0 and logp.shape[1] >= A and cum.shape == (B,) and live.shape == (B,)
    with np.errstate(invalid="ignore", over="ignore"):
        score = (cum[:, None] + logp[:, :A]).astype(np.float32)  # f32 + f32 in numpy is one f32 addition
    exists = live[:, None] & ~np.isnan(score) & (score != NEG_INF)
    parent = np.arange(B, dtype=np.int64)
    actions = np.full(B, A, dtype=np.int64)
    cum_out = np.full(B, NEG_INF, dtype=np.float32)
    live_out = np.zeros(B, dtype=np.uint8)
    for g in range(B // W):
        sl = slice(g * W, (g + 1) * W)
        slot, act = np.nonzero(exists[sl])  # row-major: already slot-, then action-ascending
        s = score[sl][slot, act]
        with np.errstate(invalid="ignore"):
            order = np.argsort(-s, kind="stable")[:W]  # stable: ties keep slot-then-action order; -(-0.0) == -(0.0)
        k = order.size
        parent[g * W : g * W + k] = g * W + slot[order]
        actions[g * W : g * W + k] = act[order]
        cum_out[g * W : g * W + k] = s[order]
        live_out[g * W : g * W + k] = 1
    return parent, actions, cum_out, live_out


def beam_search(targets: Sequence, W: int, A: int, max_steps: int, logp_of: Callable[[int, list], np.ndarray]) -> List[Optional[List[int]]]:
    """targets: M oracle envs (track_solution on), each holding its target; they are cloned, not stepped.
    logp_of(t, envs) -> [M * W, >= A] float32 scores of step t; envs[b] is slot b's oracle env (None for a slot that holds no beam: its row
    is not read)."""
    M = len(targets)
    B = M * W
    envs: list = [None] * B
    live = np.zeros(B, dtype=bool)
    cum = np.zeros(B, dtype=np.float32)
    ret = np.zeros(B, dtype=np.float32)
    best = np.full(M, NEG_INF, dtype=np.float32)
    winner: List[Optional[List[int]]] = [None] * M
    for g, target in enumerate(targets):
        if target.success():
            best[g] = np.float32(0.0)
            winner[g] = [int(x) for x in target.solution()]
        else:
            envs[g * W] = target.clone()
            live[g * W] = True
    for t in range(max_steps):
        if not live.any():
            break
        logp = np.asarray(logp_of(t, envs), dtype=np.float32)
        parent, actions, cum, live_sel = select(logp, cum, live, W, A)
        new_envs: list = [None] * B
        new_ret = np.zeros(B, dtype=np.float32)
        live = live_sel.astype(bool)
        for b in np.nonzero(live)[0]:
            env = envs[parent[b]].clone()
            env.step(int(actions[b]))
            new_envs[b] = env
            new_ret[b] = np.float32(ret[parent[b]]) + np.float32(env.reward())
        envs, ret = new_envs, new_ret
        for g in range(M):
            pick = None
            for b in range(g * W, (g + 1) * W):
                if live[b] and envs[b].success() and (pick is None or ret[b] > ret[pick]):
                    pick = b
            if pick is not None and ret[pick] > best[g]:
                best[g] = ret[pick]
                winner[g] = [int(x) for x in envs[pick].solution()]
        for b in np.nonzero(live)[0]:
            if envs[b].is_final():
                live[b] = False
                envs[b] = None
    return winner
