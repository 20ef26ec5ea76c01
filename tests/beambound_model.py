"""CPU restatement of `qg_beam_advance` (the rules in its comment in include/qgym.h) and of the beam search of
`BatchedSynthesis.solve(..., beam_width=W, bound=...)` that runs on it: numpy f32 for the two additions and the comparisons, `OracleEnv.clone`
for the envs, `beammodel.select` for the selection step.  TEST INFRASTRUCTURE ONLY; it shares no code with qiskit_gym_amd.

The rules of one call.  The batch is M groups of W slots; group g owns slots g*W .. g*W + W-1.  Per group g, in this order:
  1. A live slot b gets r[b] = f32(ret_in[parent[b]]) + f32(reward[b]), one f32 addition, and ret_out[b] = r[b].  A slot that is not live
     gets ret_out[b] = 0; nothing else of it is read.
  2. solved[b] = live[b] and success[b].  The pick j is the solved slot of the largest r (-0 = +0; NaN and -inf are no pick), the lowest
     slot among equals.  With a pick and r[j] > best[g], strictly: best[g] = r[j], found[g] = 1, win_src[g] = g*W + j.  Otherwise
     win_src[g] = skip and best[g], found[g] stay.
  3. live[b] = live[b] and not done[b].
  4. With a mode other than none and found[g] set after rule 2: hopeful[b] = live[b] and f32(r[b] + bonus) > best[g], against the best[g]
     of rule 2; equality is hopeless.  "stop": if no slot of the group is hopeful, all its live slots end.  "prune": every live slot that
     is not hopeful ends.  bounded[g] grows by the number of slots ended this way.  A group with found[g] == 0 is left alone.
  5. live is 0 / 1, group_live[g] = the number of slots of g still live.
"""
from __future__ import annotations

from typing import Callable, List, Optional, Sequence

import numpy as np

from beammodel import NEG_INF, select

MODES = {None: 0, "none": 0, 0: 0, "stop": 1, 1: 1, "prune": 2, 2: 2}


def advance(parent, ret_in, reward, success, done, live, best, found, W: int, skip: int, bonus, mode, bounded=None):
    """One call, on copies: returns (ret_out f32 [B], live uint8 [B], best f32 [M], found uint8 [M], win_src int64 [M], group_live int64 [M],
    bounded int64 [M]).  parent: [B] ints; ret_in, reward: [B] float32; success, done, live: [B] bool or 0 / not 0; best: [M] float32;
    found: [M] bool or 0 / not 0; bounded: [M] ints or None (zeros)."""
    m = MODES[mode]
    parent = np.asarray(parent).astype(np.int64)
    ret_in, reward = np.asarray(ret_in, dtype=np.float32), np.asarray(reward, dtype=np.float32)
    success, done = np.asarray(success).astype(bool), np.asarray(done).astype(bool)
    lv = np.asarray(live).astype(bool).copy()
    best = np.asarray(best, dtype=np.float32).copy()
    found_in = np.asarray(found)
    found = found_in.astype(np.uint8)  # (a copy) the bytes that are not rewritten stay
    B = parent.shape[0]
    assert B % W == 0 and 1 <= W
    M = B // W
    assert ret_in.shape == reward.shape == success.shape == done.shape == lv.shape == (B,) and best.shape == found.shape == (M,)
    bounded = np.zeros(M, dtype=np.int64) if bounded is None else np.asarray(bounded).astype(np.int64).copy()
    bonus = np.float32(bonus)
    idx = np.nonzero(lv)[0]
    assert ((parent[idx] >= 0) & (parent[idx] < B)).all(), "a live slot's parent is an env of the batch"
    r = np.zeros(B, dtype=np.float32)
    with np.errstate(invalid="ignore", over="ignore"):
        r[idx] = ret_in[parent[idx]] + reward[idx]  # f32 + f32 in numpy is one f32 addition
        reach = (r + bonus).astype(np.float32)      # and so is this one
    win_src = np.full(M, skip, dtype=np.int64)
    group_live = np.zeros(M, dtype=np.int64)
    for g in range(M):
        lo, hi = g * W, (g + 1) * W
        pick = None
        for b in range(lo, hi):  # ascending, and replaced only by a strictly larger r: the lowest slot among equals; 0.0 > -0.0 is False
            if lv[b] and success[b] and not np.isnan(r[b]) and r[b] != NEG_INF and (pick is None or r[b] > r[pick]):
                pick = b
        if pick is not None and r[pick] > best[g]:
            best[g], found[g], win_src[g] = r[pick], 1, pick
        lv[lo:hi] &= ~done[lo:hi]
        if m and found[g]:
            hopeful = lv[lo:hi] & (reach[lo:hi] > best[g])  # a NaN compares False
            if m == 2 or not hopeful.any():
                bounded[g] += int(lv[lo:hi].sum()) - int(hopeful.sum())
                lv[lo:hi] = hopeful
        group_live[g] = int(lv[lo:hi].sum())
    return r, lv.astype(np.uint8), best, found, win_src, group_live, bounded


def beam_search_bounded(targets: Sequence, W: int, A: int, max_steps: int, logp_of: Callable[[int, list], np.ndarray], mode, bonus=1.0,
                        trace: Optional[dict] = None) -> List[Optional[List[int]]]:
    """`beammodel.beam_search` with the step's bookkeeping done by `advance` (bonus 1.0, skip = the batch size) -- mode None is that search,
    "stop" and "prune" are the bounded ones.  targets, logp_of: as there.  `trace`, if given, receives "steps", "bounded" (int64 [M], the
    beams the bound ended per group), "ended_at" (int64 [M]: the step whose bound first ended beams of the group, -1 if none did) and
    "group_live" (per step the [M] live counts after it)."""
    M = len(targets)
    B = M * W
    envs: list = [None] * B
    live = np.zeros(B, dtype=np.uint8)
    cum = np.zeros(B, dtype=np.float32)
    ret = np.zeros(B, dtype=np.float32)
    best = np.full(M, NEG_INF, dtype=np.float32)
    found = np.zeros(M, dtype=np.uint8)
    bounded = np.zeros(M, dtype=np.int64)
    ended_at = np.full(M, -1, dtype=np.int64)
    counts = []
    winner: List[Optional[List[int]]] = [None] * M
    for g, target in enumerate(targets):
        if target.success():
            best[g], found[g] = np.float32(0.0), 1
            winner[g] = [int(x) for x in target.solution()]
        else:
            envs[g * W] = target.clone()
            live[g * W] = 1
    steps = 0
    for t in range(max_steps):
        if not live.any():
            break
        logp = np.asarray(logp_of(t, envs), dtype=np.float32)
        parent, actions, cum, live = select(logp, cum, live, W, A)
        new_envs: list = [None] * B
        reward, success, done = np.zeros(B, dtype=np.float32), np.zeros(B, dtype=np.uint8), np.zeros(B, dtype=np.uint8)
        for b in np.nonzero(live)[0]:
            env = envs[parent[b]].clone()
            env.step(int(actions[b]))
            new_envs[b] = env
            reward[b], success[b], done[b] = np.float32(env.reward()), bool(env.success()), bool(env.is_final())
        before = bounded
        ret, live, best, found, win_src, group_live, bounded = advance(parent, ret, reward, success, done, live, best, found, W, B, bonus, mode, bounded)
        for g in np.nonzero(win_src != B)[0]:
            winner[g] = [int(x) for x in new_envs[win_src[g]].solution()]
        envs = [env if live[b] else None for b, env in enumerate(new_envs)]
        ended_at[(bounded > before) & (ended_at < 0)] = t
        counts.append(group_live)
        steps = t + 1
    if trace is not None:
        trace.update(steps=steps, bounded=bounded, ended_at=ended_at, group_live=counts)
    return winner
