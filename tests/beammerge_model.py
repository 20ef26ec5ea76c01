"""CPU restatement of `qg_beam_merge` (the rules in its comment, include/qgym.h) and of the beam search of
`BatchedSynthesis.solve(..., beam_width=W, merge_duplicates=True)`: Python-int arithmetic for the state key, numpy f32 for the order of the
scores, `beammodel.select` and `OracleEnv.clone` for the rest.  TEST INFRASTRUCTURE ONLY; it shares no code with qiskit_gym_amd.

The rules.  The batch is groups of W slots; group g owns slots g*W .. g*W + W-1 and a history: a list of at most `cap` distinct keys.
  key        n words w_0 .. w_{n-1} (unsigned, below 2^64) of one slot:  key = mix(n ^ (sum_i mix(w_i ^ mix(i + 1)) mod 2^64)), mix =
             splitmix64; a key of 0 becomes 0x9E3779B97F4A7C15.  Equal keys = the same state.
  merge      1. a live slot whose cum is NaN or -inf is dropped, counted nowhere;  2. a live slot whose key is in the history is dropped
             (a revisit);  3. of the remaining live slots of a group that share a key the one with the largest cum (-0 = +0; ties: the lowest
             slot) survives, the others are dropped (duplicates);  4. live_out = 1 exactly for the survivors;  5. the survivors' keys are
             appended to the history in ascending slot order while it holds fewer than `cap`.
  search     `beammodel.beam_search`, and after the slots whose env is final have left a step: merge, on the envs' packed observations,
             with one history per target.  Before the first step the same merge runs on the initial batch (one live slot per unsolved
             target), which records every target's own key.
"""
from __future__ import annotations

from typing import Callable, List, Optional, Sequence

import numpy as np
from beammodel import NEG_INF, select

MASK = (1 << 64) - 1
GOLDEN = 0x9E3779B97F4A7C15


def splitmix64(x: int) -> int:
    x = (x + GOLDEN) & MASK
    x = ((x ^ (x >> 30)) * 0xBF58476D1CE4E5B9) & MASK
    x = ((x ^ (x >> 27)) * 0x94D049BB133111EB) & MASK
    return x ^ (x >> 31)


def close_key(n: int, total: int) -> int:
    """The last stage of the key: `total` is the wrapped sum over the words."""
    k = splitmix64(n ^ (total & MASK))
    return k if k else GOLDEN


def state_key(words: Sequence[int]) -> int:
    """words: one slot's packed observation; signed integer dtypes count as their two's-complement bit pattern."""
    if isinstance(words, np.ndarray) and words.dtype.kind == "i":
        words = words.view(words.dtype.str.replace("i", "u"))
    ws = [int(w) for w in words]  # Python ints from here on: no fixed-width arithmetic to overflow
    assert all(0 <= w <= MASK for w in ws)
    return close_key(len(ws), sum(splitmix64(w ^ splitmix64(i + 1)) for i, w in enumerate(ws)))


def order_word(score) -> int:
    """`beam_order` of the select kernel: larger score <=> larger word, -0 = +0, 0 = NaN or -inf."""
    s = np.float32(score)
    if np.isnan(s) or s == NEG_INF:
        return 0
    u = int(s.view(np.uint32))
    if u == 0x80000000:
        u = 0
    return (~u & 0xFFFFFFFF) if u & 0x80000000 else (u | 0x80000000)


def merge(words: np.ndarray, cum: np.ndarray, live: np.ndarray, W: int, seen: Optional[List[List[int]]] = None, cap: int = 0):
    """words: [B, n] unsigned (or signed: bit patterns); cum: [B] float32; live: [B] bool or 0/1; seen: one list of keys per group, EXTENDED in
    place (None: merge within the call only).  Returns (live_out uint8 [B], keys uint64 [B], dropped uint32 [B // W, 2])."""
    words = np.asarray(words)
    B = words.shape[0]
    cum = np.asarray(cum, dtype=np.float32)
    live = np.asarray(live).astype(bool)
    assert B % W == 0 and cum.shape == (B,) and live.shape == (B,) and (seen is None or len(seen) == B // W)
    keys = [state_key(words[b]) for b in range(B)]
    live_out = np.zeros(B, dtype=np.uint8)
    dropped = np.zeros((B // W, 2), dtype=np.uint32)
    for g in range(B // W):
        hist = seen[g] if seen is not None else []
        best: dict = {}  # key -> the slot that survives so far
        for b in range(g * W, (g + 1) * W):
            o = order_word(cum[b]) if live[b] else 0
            if o == 0:
                continue
            if keys[b] in hist:
                dropped[g, 0] += 1
                continue
            dropped[g, 1] += keys[b] in best
            if keys[b] not in best or o > order_word(cum[best[keys[b]]]):  # a tie keeps the earlier, lower slot
                best[keys[b]] = b
        for b in sorted(best.values()):
            live_out[b] = 1
            if seen is not None and len(hist) < cap:
                hist.append(keys[b])
    return live_out, np.array(keys, dtype=np.uint64), dropped


def words_of(env) -> List[int]:
    """An oracle env's dense observation packed as QG_FMT_PACKED does: word r has bit c set where entry (r, c) is; a PermutationEnv row is
    the byte that holds its set column."""
    dense = np.asarray(env.dense_obs())
    if env.kind == "permutation":
        return [int(np.argmax(row)) for row in dense]
    return [sum(1 << int(c) for c in np.nonzero(row)[0]) for row in dense]


def beam_search_merged(targets: Sequence, W: int, A: int, max_steps: int, logp_of: Callable[[int, list], np.ndarray],
                       words_of: Callable = words_of, stats: Optional[dict] = None) -> List[Optional[List[int]]]:
    """`beammodel.beam_search` with the merge step; arguments as there.  stats (optional dict) receives "revisits" and "merged"."""
    M = len(targets)
    B = M * W
    envs: list = [None] * B
    live = np.zeros(B, dtype=bool)
    cum = np.zeros(B, dtype=np.float32)
    ret = np.zeros(B, dtype=np.float32)
    best = np.full(M, NEG_INF, dtype=np.float32)
    winner: List[Optional[List[int]]] = [None] * M
    cap = max_steps * W + 1
    seen: List[List[int]] = [[] for _ in range(M)]
    total = np.zeros(2, dtype=np.int64)

    def merged(live):
        n = max(len(words_of(e)) for e in envs if e is not None) if any(e is not None for e in envs) else 1
        words = [words_of(e) if e is not None else [0] * n for e in envs]  # a slot without a beam is not live: its words are not looked at
        out, _, dropped = merge(np.array(words, dtype=np.uint64), cum, live, W, seen, cap)
        total[:] += dropped.sum(axis=0).astype(np.int64)
        return out.astype(bool)

    for g, target in enumerate(targets):
        if target.success():
            best[g] = np.float32(0.0)
            winner[g] = [int(x) for x in target.solution()]
        else:
            envs[g * W] = target.clone()
            live[g * W] = True
    live = merged(live)
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
        live = merged(live)
        for b in range(B):
            if not live[b]:
                envs[b] = None
    if stats is not None:
        stats.update(revisits=int(total[0]), merged=int(total[1]))
    return winner
