"""The policy-layer kernels from Python: thin ctypes wrappers around libqgym's sampling, beam, tree-search, twist and policy-layer entries, the
reference-shaped `BasicPolicy`, and the kernels' packed operands -- the one layer below both of their callers, the rollout collector
(`collector.py`) and the batched searches (`synthesis.py`): vec -> policy_kernels -> {collector, synthesis}.

What the two callers share is written once here: `PolicyOperands` (fused head, first-layer bias, packed middle layer and head),
`FirstLayer` / `first_layer` (the one place that says which route a handle's first layer takes) and `run_first_layer` (the one dispatch
to `embed`, `embed_observe` and `embed_words`).  Who refreshes them differs: the collector repacks in place at the top of every collection
(`PolicyOperands.repack_`: the same buffers, so a captured collection follows an in-place parameter update), the searches take a new
snapshot when a parameter's version counter has moved.
"""
from __future__ import annotations

from dataclasses import dataclass
from typing import NamedTuple, Optional, Tuple

import torch
import torch.nn as nn

from . import _lib
from .vec import VecEnv, _stream_ptr

_DT = {torch.float32: _lib.QG_DT_F32, torch.bfloat16: _lib.QG_DT_BF16, torch.float16: _lib.QG_DT_F16, torch.int8: _lib.QG_DT_I8}


def sample_actions(logits: torch.Tensor, seed: int, counter: int, num_actions: Optional[int] = None, mask: Optional[torch.Tensor] = None,
                   value_col: Optional[int] = None, actions: Optional[torch.Tensor] = None, logp: Optional[torch.Tensor] = None,
                   entropy: Optional[torch.Tensor] = None, values: Optional[torch.Tensor] = None, clock: Optional[torch.Tensor] = None):
    """One categorical draw per row of `logits[:, :num_actions]` (f32 / bf16 / f16, row stride free).
    `clock`: optional int64 device scalar added to `counter` on the device (graph replays).
    Returns (actions int64, logp f32, entropy f32, values f32 or None); see `qg_sample_actions`."""
    if logits.dim() != 2 or logits.stride(1) != 1:
        raise ValueError("logits must be [B, >=num_actions] with unit column stride")
    B, dev = logits.shape[0], logits.device
    A = int(num_actions) if num_actions is not None else logits.shape[1]
    actions = torch.empty(B, dtype=torch.int64, device=dev) if actions is None else actions
    logp = torch.empty(B, dtype=torch.float32, device=dev) if logp is None else logp
    entropy = torch.empty(B, dtype=torch.float32, device=dev) if entropy is None else entropy
    if value_col is not None and values is None:
        values = torch.empty(B, dtype=torch.float32, device=dev)
    if mask is not None:
        mask = mask.to(torch.uint8).contiguous()
    act_dt = {torch.int32: _lib.ACT_I32, torch.int64: _lib.ACT_I64}[actions.dtype]
    L = _lib.load()
    _lib.check(L.qg_sample_actions(
        logits.data_ptr(), _DT[logits.dtype], logits.stride(0), B, A, mask.data_ptr() if mask is not None else None,
        int(seed) & (2**64 - 1), int(counter), clock.data_ptr() if clock is not None else None, actions.data_ptr(), act_dt, logp.data_ptr(), entropy.data_ptr(),
        -1 if value_col is None else int(value_col), values.data_ptr() if value_col is not None else None, _stream_ptr()))
    return actions, logp, entropy, values


def beam_select(logp: torch.Tensor, cum: torch.Tensor, live: torch.Tensor, width: int, num_actions: Optional[int] = None,
                parent: Optional[torch.Tensor] = None, actions: Optional[torch.Tensor] = None, cum_out: Optional[torch.Tensor] = None,
                live_out: Optional[torch.Tensor] = None):
    """The selection step of a beam search (`qg_beam_select`): the batch is groups of `width` consecutive envs; from every group's live
    slots x actions keep the `width` best continuations by `cum[b] + logp[b, a]` (f32; ties by slot, then action; NaN / -inf = no such
    candidate).  logp: [B, >= num_actions] f32 / bf16 / f16 with unit column stride; cum: f32 [B]; live: uint8 / bool [B].
    Returns (parent int32 [B] -- batch-wide env indices, for `VecEnv.copy_envs`; actions int32 [B] -- num_actions where a slot stays empty;
    cum_out f32 [B]; live_out uint8 [B]).  Preallocated outputs may be passed (actions int32 or int64); they may not alias the inputs."""
    if logp.dim() != 2 or logp.stride(1) != 1:
        raise ValueError("logp must be [B, >=num_actions] with unit column stride")
    B, dev, W = logp.shape[0], logp.device, int(width)
    A = int(num_actions) if num_actions is not None else logp.shape[1]
    if W < 1 or B % W:
        raise ValueError(f"beam_select: {B} envs do not divide into groups of {W}")
    if live.dtype == torch.bool:
        live = live.view(torch.uint8)
    for name, t, dt in (("cum", cum, torch.float32), ("live", live, torch.uint8)):
        if t.dtype != dt or t.numel() != B or not t.is_contiguous() or t.device != dev:
            raise ValueError(f"beam_select: {name} must be a contiguous [B] {dt} tensor on logp's device")
    parent = torch.empty(B, dtype=torch.int32, device=dev) if parent is None else parent
    actions = torch.empty(B, dtype=torch.int32, device=dev) if actions is None else actions
    cum_out = torch.empty(B, dtype=torch.float32, device=dev) if cum_out is None else cum_out
    live_out = torch.empty(B, dtype=torch.uint8, device=dev) if live_out is None else live_out
    for name, t, dts in (("parent", parent, (torch.int32,)), ("actions", actions, (torch.int32, torch.int64)), ("cum_out", cum_out, (torch.float32,)),
                         ("live_out", live_out, (torch.uint8,))):
        if t.dtype not in dts or t.numel() != B or not t.is_contiguous() or t.device != dev:
            raise ValueError(f"beam_select: {name} must be a contiguous [B] tensor of {' / '.join(str(d) for d in dts)} on logp's device")
    act_dt = {torch.int32: _lib.ACT_I32, torch.int64: _lib.ACT_I64}[actions.dtype]
    _lib.check(_lib.load().qg_beam_select(logp.data_ptr(), _DT[logp.dtype], logp.stride(0), A, B // W, W, cum.data_ptr(), live.data_ptr(), parent.data_ptr(),
                                          actions.data_ptr(), act_dt, cum_out.data_ptr(), live_out.data_ptr(), _stream_ptr()))
    return parent, actions, cum_out, live_out


def beam_seen(n_groups: int, cap: int, device=None) -> torch.Tensor:
    """An empty history for `beam_merge`: room for `cap` state keys for each of `n_groups` groups (`qg_beam_seen_bytes`), zeroed.  Opaque;
    `zero_()` empties it again."""
    if int(n_groups) < 0 or int(cap) < 1:
        raise ValueError("beam_seen: n_groups >= 0 and cap >= 1")
    nbytes = int(_lib.load().qg_beam_seen_bytes(int(n_groups), int(cap)))
    return torch.zeros(nbytes // 8, dtype=torch.int64, device="cuda" if device is None else device)


def beam_merge(words: torch.Tensor, cum: torch.Tensor, live: torch.Tensor, width: int, seen: Optional[torch.Tensor] = None, seen_cap: int = 0,
               keys: Optional[torch.Tensor] = None, dropped: Optional[torch.Tensor] = None, live_out: Optional[torch.Tensor] = None) -> torch.Tensor:
    """The merge step of a beam search (`qg_beam_merge`): the batch is groups of `width` consecutive envs; a live slot leaves when its state
    key -- a 64-bit hash of its row of `words` -- is in its group's history `seen` (a revisit), or when another live slot of its group holds
    the same key with a larger `cum` (ties: the lower slot stays; a duplicate).  The survivors' keys enter the history.
    words: [B, words_per_env] of 1-, 4- or 8-byte integers (`VecEnv.observe_packed`); cum: f32 [B]; live: uint8 / bool [B]; seen: from
    `beam_seen(B // width, seen_cap)`, or None to merge within the call only.  keys: optional int64 [B], receives every slot's key;
    dropped: optional int32 [B // width, 2], (revisits, duplicates) are added to it.  Returns live_out uint8 [B] (not `live` itself)."""
    if words.dim() != 2 or not words.is_contiguous() or words.is_floating_point() or words.element_size() not in (1, 4, 8):
        raise ValueError("beam_merge: words must be a contiguous [B, words_per_env] tensor of 1-, 4- or 8-byte integers")
    B, dev, W = words.shape[0], words.device, int(width)
    if W < 1 or B % W:
        raise ValueError(f"beam_merge: {B} envs do not divide into groups of {W}")
    if live.dtype == torch.bool:
        live = live.view(torch.uint8)
    live_out = torch.empty(B, dtype=torch.uint8, device=dev) if live_out is None else live_out
    for name, t, dt, numel in (("cum", cum, (torch.float32,), B), ("live", live, (torch.uint8,), B), ("live_out", live_out, (torch.uint8,), B),
                               ("keys", keys, (torch.int64, torch.uint64), B), ("dropped", dropped, (torch.int32, torch.uint32), 2 * (B // W))):
        if t is not None and (t.dtype not in dt or t.numel() != numel or not t.is_contiguous() or t.device != dev):
            raise ValueError(f"beam_merge: {name} must be a contiguous tensor of {numel} {' / '.join(str(d) for d in dt)} on the device of words")
    L = _lib.load()
    if seen is not None and (seen.dtype != torch.int64 or not seen.is_contiguous() or seen.device != dev
                             or seen.numel() * 8 != L.qg_beam_seen_bytes(B // W, int(seen_cap))):
        raise ValueError("beam_merge: seen must come from beam_seen(B // width, seen_cap) on the device of words")
    _lib.check(L.qg_beam_merge(words.data_ptr(), words.element_size(), words.shape[1], B // W, W, cum.data_ptr(), live.data_ptr(),
                               seen.data_ptr() if seen is not None else None, int(seen_cap) if seen is not None else 0, live_out.data_ptr(),
                               keys.data_ptr() if keys is not None else None, dropped.data_ptr() if dropped is not None else None, _stream_ptr()))
    return live_out


def beam_advance(parent: torch.Tensor, ret_in: torch.Tensor, reward: torch.Tensor, success: torch.Tensor, done: torch.Tensor, live: torch.Tensor,
                 best: torch.Tensor, found: torch.Tensor, width: int, skip: int, bonus: float = 1.0, mode: Optional[str] = None,
                 ret_out: Optional[torch.Tensor] = None, win_src: Optional[torch.Tensor] = None, group_live: Optional[torch.Tensor] = None,
                 bounded: Optional[torch.Tensor] = None):
    """What a beam search does with a step's results (`qg_beam_advance`): the batch is groups of `width` consecutive envs.  Per live slot
    `ret_out[b] = ret_in[parent[b]] + reward[b]` (f32; 0 where not live); per group the solved slot of the largest return (lowest slot among
    equals) becomes the winner if its return is strictly above `best[g]` -- `best`, `found` are updated IN PLACE and `win_src[g]` is its env
    index for `VecEnv.copy_envs`, else `skip` --; `live` (IN PLACE) loses the slots that are `done`.  mode "stop" / "prune" (None: neither)
    then apply the bound in groups that have a winner: a live slot is hopeful when `ret_out[b] + bonus > best[g]`; "stop" ends a group's
    beams once none is hopeful, "prune" ends every hopeless beam; `bounded[g]` (optional, int32 [B // width]) is added to.  Contract:
    finite returns (the envs' rewards are).  A solved slot whose return is NaN or -inf has no order word and is no pick, where an `argmax`
    over the scores would have let it shadow its group.
    parent: int32 [B]; ret_in, reward: f32 [B]; success, done, live: uint8 / bool [B]; best: f32 [B // width]; found: uint8 / bool [B // width].
    Returns (ret_out f32 [B] -- not `ret_in` itself --, win_src int32 [B // width], group_live uint8 [B // width]: the live slots left)."""
    B, dev, W = parent.numel(), parent.device, int(width)
    if W < 1 or B % W:
        raise ValueError(f"beam_advance: {B} envs do not divide into groups of {W}")
    if mode not in _lib.BOUND_MODES:
        raise ValueError(f"beam_advance: mode must be None, 'stop' or 'prune', not {mode!r}")
    M = B // W
    success, done, live, found = (t.view(torch.uint8) if t.dtype == torch.bool else t for t in (success, done, live, found))
    ret_out = torch.empty(B, dtype=torch.float32, device=dev) if ret_out is None else ret_out
    win_src = torch.empty(M, dtype=torch.int32, device=dev) if win_src is None else win_src
    group_live = torch.empty(M, dtype=torch.uint8, device=dev) if group_live is None else group_live
    for name, t, dt, numel in (("parent", parent, torch.int32, B), ("ret_in", ret_in, torch.float32, B), ("reward", reward, torch.float32, B),
                               ("success", success, torch.uint8, B), ("done", done, torch.uint8, B), ("live", live, torch.uint8, B),
                               ("best", best, torch.float32, M), ("found", found, torch.uint8, M), ("ret_out", ret_out, torch.float32, B),
                               ("win_src", win_src, torch.int32, M), ("group_live", group_live, torch.uint8, M), ("bounded", bounded, torch.int32, M)):
        if t is not None and (t.dtype != dt or t.numel() != numel or t.dim() != 1 or not t.is_contiguous() or t.device != dev):
            raise ValueError(f"beam_advance: {name} must be a contiguous [{numel}] {dt} tensor on parent's device")
    if ret_out.data_ptr() == ret_in.data_ptr() and B:
        raise ValueError("beam_advance: ret_out may not alias ret_in (a slot's parent is another slot)")
    _lib.check(_lib.load().qg_beam_advance(M, W, parent.data_ptr(), ret_in.data_ptr(), reward.data_ptr(), success.data_ptr(), done.data_ptr(),
                                           live.data_ptr(), best.data_ptr(), found.data_ptr(), ret_out.data_ptr(), win_src.data_ptr(),
                                           group_live.data_ptr(), bounded.data_ptr() if bounded is not None else None, int(skip), float(bonus),
                                           _lib.BOUND_MODES[mode], _stream_ptr()))
    return ret_out, win_src, group_live


MCTS_MAX_FOREST_BYTES = 1 << 30  # what `mcts_forest` allocates at most unless told otherwise: 1 GiB


class MctsForest:
    """The trees of a PUCT search as a struct of arrays (`qg_mcts_forest`), one tree per target, torch tensors on one device:
    `parent` int32, `reward` f32, `value` f32, `visits` int32, `wsum` f32, `terminal` uint8, all [M, cap]; `child` int32 (-1 = not expanded)
    and `prior` f32, [M, cap, A]; `n_nodes` int32 [M].  `cap` = N + 1 nodes for N simulations unless told otherwise (trees that
    `mcts_rebase` carries from decision to decision want more); node 0 is the root; node j of tree m goes
    with env m * cap + j of a pool handle.  Only the nodes below `n_nodes[m]` mean anything.  `mcts_backup(root=True)` starts every tree."""
    FIELDS = ("parent", "reward", "value", "visits", "wsum", "terminal", "child", "prior", "n_nodes")

    def __init__(self, M: int, N: int, A: int, device, cap: Optional[int] = None):
        cap = N + 1 if cap is None else cap
        self.M, self.N, self.A, self.cap, self.device = M, N, A, cap, torch.device(device)
        i32, f32 = torch.int32, torch.float32
        for name, shape, dt in (("parent", (M, cap), i32), ("reward", (M, cap), f32), ("value", (M, cap), f32), ("visits", (M, cap), i32), ("wsum", (M, cap), f32),
                                ("terminal", (M, cap), torch.uint8), ("child", (M, cap, A), i32), ("prior", (M, cap, A), f32), ("n_nodes", (M,), i32)):
            setattr(self, name, torch.zeros(shape, dtype=dt, device=self.device))
        self._c = _lib.QGMctsForest(*(getattr(self, name).data_ptr() for name in self.FIELDS), M, cap, A)

    @property
    def skip(self) -> int:
        """What `mcts_select` writes to `dst` where nothing is expanded: no env of the pool, `copy_envs` skips it."""
        return self.M * self.cap


MCTS_MAX_CAP = 8192  # the kernels' limit on a tree's nodes


def mcts_forest(M: int, N: int, A: int, device=None, max_bytes: int = MCTS_MAX_FOREST_BYTES, cap: Optional[int] = None) -> MctsForest:
    """An empty forest for `mcts_select` / `mcts_backup`: M trees of N + 1 nodes over A actions (`qg_mcts_forest_bytes` says what it takes:
    (N + 1) * (21 + 8 A) + 4 bytes per tree).  cap: the nodes a tree has room for, N + 1 <= cap <= 8192, where trees are carried from
    decision to decision (`mcts_rebase`); None: N + 1.  ValueError for M < 1, N < 1, A < 1, a cap outside its range or a forest of more
    than `max_bytes`."""
    M, N, A = int(M), int(N), int(A)
    if M < 1 or N < 1 or A < 1:
        raise ValueError("mcts_forest: M >= 1, N >= 1 and A >= 1")
    if cap is not None:
        cap = int(cap)
        if not N + 1 <= cap <= MCTS_MAX_CAP:
            raise ValueError(f"mcts_forest: cap must satisfy N + 1 = {N + 1} <= cap <= {MCTS_MAX_CAP}")
    nodes = N + 1 if cap is None else cap
    nbytes = int(_lib.load().qg_mcts_forest_bytes(M, nodes, A))
    if nbytes > int(max_bytes):
        raise ValueError(f"mcts_forest: {M} trees of {nodes} nodes over {A} actions take {nbytes} bytes, more than the limit of {int(max_bytes)}")
    return MctsForest(M, N, A, "cuda" if device is None else device, cap)


def _mcts_vectors(name: str, forest: MctsForest, items):
    """`items`: (name, tensor or None, dtype); every tensor given must be a contiguous [M] tensor of its dtype on the forest's device."""
    for nm, t, dt in items:
        if t is not None and (t.dtype != dt or t.dim() != 1 or t.numel() != forest.M or not t.is_contiguous() or t.device != forest.parent.device):
            raise ValueError(f"{name}: {nm} must be a contiguous [{forest.M}] {dt} tensor on the forest's device")


def mcts_select(forest: MctsForest, C: float, finished: Optional[torch.Tensor] = None, src: Optional[torch.Tensor] = None,
                dst: Optional[torch.Tensor] = None, act: Optional[torch.Tensor] = None, leaf: Optional[torch.Tensor] = None):
    """One PUCT descent per tree (`qg_mcts_select`): from the root, at every node the action of the greatest
    `Q + ((C * prior) * sqrt(visits[node])) / (1 + n_a)` (f32, each operation rounded once; Q = wsum / visits of the child, the node's
    own value where the edge has no child; ties to the lowest action), down to an edge without a child or a terminal node.
    finished: optional uint8 / bool [M], trees whose real env is final: they make no simulation.  Returns int32 [M] each: (src, the pool
    index of the node to expand from; dst, the pool index of the new node -- `forest.skip`, out of range, where nothing is expanded; act,
    the action -- A where nothing is expanded; leaf, the node `mcts_backup` starts from, -1: none).  Preallocated outputs may be passed."""
    if not isinstance(forest, MctsForest):
        raise TypeError("mcts_select: forest must come from mcts_forest")
    if not float(C) > 0.0:
        raise ValueError("mcts_select: C must be positive")
    dev, i32 = forest.parent.device, torch.int32
    if finished is not None and finished.dtype == torch.bool:
        finished = finished.view(torch.uint8)
    src, dst, act, leaf = (torch.empty(forest.M, dtype=i32, device=dev) if t is None else t for t in (src, dst, act, leaf))
    _mcts_vectors("mcts_select", forest, (("finished", finished, torch.uint8), ("src", src, i32), ("dst", dst, i32), ("act", act, i32), ("leaf", leaf, i32)))
    _lib.check(_lib.load().qg_mcts_select(forest._c, float(C), finished.data_ptr() if finished is not None else None, src.data_ptr(), dst.data_ptr(),
                                          act.data_ptr(), leaf.data_ptr(), _stream_ptr()))
    return src, dst, act, leaf


def mcts_backup(forest: MctsForest, logp: torch.Tensor, values: torch.Tensor, reward: Optional[torch.Tensor] = None, done: Optional[torch.Tensor] = None,
                src: Optional[torch.Tensor] = None, dst: Optional[torch.Tensor] = None, act: Optional[torch.Tensor] = None,
                leaf: Optional[torch.Tensor] = None, root: bool = False) -> MctsForest:
    """The other half of a simulation (`qg_mcts_backup`), in place on `forest`.  logp: f32 [M, >= A] with unit column stride, the rows of
    log-probabilities (`mid_head_logp`'s, or `log_softmax`) and values: f32 [M], the value head, of the envs just evaluated.
    root=True starts every tree from them: node 0 with prior = exp(logp), value (0 if `done`: optional), visits 1, no children.
    Otherwise src, dst, act, leaf are `mcts_select`'s outputs and reward f32 [M], done uint8 / bool [M] the expanded envs' step results:
    where act < A the new node is linked under (src, act) with prior = exp(logp), its value (0 if done), reward and terminal flag; then
    from `leaf` up G = value[leaf], G = reward[y] + G, visits[y] += 1, wsum[y] += G for every node but the root, whose visits grow by 1.
    Trees with leaf < 0 are left alone."""
    if not isinstance(forest, MctsForest):
        raise TypeError("mcts_backup: forest must come from mcts_forest")
    M, A, dev, i32, f32 = forest.M, forest.A, forest.parent.device, torch.int32, torch.float32
    if logp.dtype != f32 or logp.dim() != 2 or logp.shape[0] != M or logp.shape[1] < A or logp.device != dev or (logp.stride(1) != 1 and logp.shape[1] > 1) or (
            M > 1 and logp.stride(0) < A):
        raise ValueError("mcts_backup: logp must be f32 [M, >= A] with unit column stride on the forest's device")
    if done is not None and done.dtype == torch.bool:
        done = done.view(torch.uint8)
    _mcts_vectors("mcts_backup", forest, (("values", values, f32), ("reward", reward, f32), ("done", done, torch.uint8), ("src", src, i32), ("dst", dst, i32),
                                         ("act", act, i32), ("leaf", leaf, i32)))
    if values is None or (not root and any(t is None for t in (reward, done, src, dst, act, leaf))):
        raise ValueError("mcts_backup: values always; reward, done, src, dst, act and leaf unless root=True")
    ptr = [t.data_ptr() if t is not None else None for t in (src, dst, act, leaf)]
    _lib.check(_lib.load().qg_mcts_backup(forest._c, _lib.MCTS_ROOT if root else _lib.MCTS_BACKUP, *ptr, logp.data_ptr(), logp.stride(0) if M > 1 else logp.shape[1],
                                          values.data_ptr(), reward.data_ptr() if reward is not None else None, done.data_ptr() if done is not None else None,
                                          _stream_ptr()))
    return forest


MCTS_MAX_LEAVES = 64  # descents per tree and launch: one lane of the tree's wave per pending edge


def _mcts_many_shape(name: str, forest: MctsForest, K, k):
    """(K, k) as ints after the checks both many-descent wrappers share: 1 <= k <= K <= 64, M * K within 32-bit indices."""
    if not isinstance(forest, MctsForest):
        raise TypeError(f"{name}: forest must come from mcts_forest")
    K = int(K)
    k = K if k is None else int(k)
    if not 1 <= k <= K <= MCTS_MAX_LEAVES:
        raise ValueError(f"{name}: 1 <= k <= K <= {MCTS_MAX_LEAVES}, got k={k}, K={K}")
    if forest.M * K >= 2 ** 31 - 1:
        raise ValueError(f"{name}: {forest.M} trees of {K} descents are too many for 32-bit indices")
    return K, k


def _mcts_many_vectors(name: str, forest: MctsForest, K: int, items):
    """`_mcts_vectors` for the per-descent arrays: contiguous [M * K]."""
    for nm, t, dt in items:
        if t is not None and (t.dtype != dt or t.dim() != 1 or t.numel() != forest.M * K or not t.is_contiguous() or t.device != forest.parent.device):
            raise ValueError(f"{name}: {nm} must be a contiguous [{forest.M * K}] {dt} tensor on the forest's device")


def mcts_select_many(forest: MctsForest, C: float, K: int, k: Optional[int] = None, virtual_loss: float = 0.0, finished: Optional[torch.Tensor] = None,
                     src: Optional[torch.Tensor] = None, dst: Optional[torch.Tensor] = None, act: Optional[torch.Tensor] = None,
                     leaf: Optional[torch.Tensor] = None):
    """k PUCT descents per tree in one launch (`qg_mcts_select_many`), made one after another on a copy of the tree's visits and wsum: each
    is `mcts_select`'s descent, leaves a virtual visit on every node of its path (and takes `virtual_loss` from the wsum of every node but
    the root), so the next one goes elsewhere; an edge an earlier descent of the call chose for expansion is no candidate, and the e-th
    expansion names node n_nodes + e (refused, leaf = -1, where the tree is full).  K is the row length of the outputs, 1 <= k <= K <= 64,
    k=None: K.  Returns int32 [M * K] each, entry m * K + i for descent i of tree m: (src, dst, act, leaf) as `mcts_select` gives them;
    entries i >= k and those of `finished` trees are refused descents.  The forest is only read.  Preallocated outputs may be passed."""
    K, k = _mcts_many_shape("mcts_select_many", forest, K, k)
    if not float(C) > 0.0:
        raise ValueError("mcts_select_many: C must be positive")
    vl = float(virtual_loss)
    if not (vl >= 0.0 and vl < float("inf")):
        raise ValueError("mcts_select_many: virtual_loss must be finite and at least 0")
    dev, i32 = forest.parent.device, torch.int32
    if finished is not None and finished.dtype == torch.bool:
        finished = finished.view(torch.uint8)
    src, dst, act, leaf = (torch.empty(forest.M * K, dtype=i32, device=dev) if t is None else t for t in (src, dst, act, leaf))
    _mcts_vectors("mcts_select_many", forest, (("finished", finished, torch.uint8),))
    _mcts_many_vectors("mcts_select_many", forest, K, (("src", src, i32), ("dst", dst, i32), ("act", act, i32), ("leaf", leaf, i32)))
    _lib.check(_lib.load().qg_mcts_select_many(forest._c, float(C), vl, k, K, finished.data_ptr() if finished is not None else None, src.data_ptr(),
                                               dst.data_ptr(), act.data_ptr(), leaf.data_ptr(), _stream_ptr()))
    return src, dst, act, leaf


def mcts_backup_many(forest: MctsForest, K: int, logp: torch.Tensor, values: torch.Tensor, reward: torch.Tensor, done: torch.Tensor,
                     src: torch.Tensor, dst: torch.Tensor, act: torch.Tensor, leaf: torch.Tensor, k: Optional[int] = None) -> MctsForest:
    """The other half of a round (`qg_mcts_backup_many`), in place on `forest`: per tree `mcts_backup`'s rule for entries m * K + i,
    i = 0 .. k - 1 in that order -- link the new node where act < A, carry the leaf's value to the root -- with n_nodes growing as the
    nodes are linked.  logp: f32 [M * K, >= A] with unit column stride; values, reward f32 [M * K]; done uint8 / bool [M * K]; src, dst,
    act, leaf `mcts_select_many`'s outputs.  Entries with leaf < 0, and those that fail a check, are skipped."""
    K, k = _mcts_many_shape("mcts_backup_many", forest, K, k)
    R, A, dev, i32, f32 = forest.M * K, forest.A, forest.parent.device, torch.int32, torch.float32
    if logp is None or logp.dtype != f32 or logp.dim() != 2 or logp.shape[0] != R or logp.shape[1] < A or logp.device != dev or (
            logp.stride(1) != 1 and logp.shape[1] > 1) or (R > 1 and logp.stride(0) < A):
        raise ValueError("mcts_backup_many: logp must be f32 [M * K, >= A] with unit column stride on the forest's device")
    if done is not None and done.dtype == torch.bool:
        done = done.view(torch.uint8)
    if any(t is None for t in (values, reward, done, src, dst, act, leaf)):
        raise ValueError("mcts_backup_many: values, reward, done, src, dst, act and leaf are required")
    _mcts_many_vectors("mcts_backup_many", forest, K, (("values", values, f32), ("reward", reward, f32), ("done", done, torch.uint8), ("src", src, i32),
                                                       ("dst", dst, i32), ("act", act, i32), ("leaf", leaf, i32)))
    _lib.check(_lib.load().qg_mcts_backup_many(forest._c, k, K, src.data_ptr(), dst.data_ptr(), act.data_ptr(), leaf.data_ptr(), logp.data_ptr(),
                                               logp.stride(0) if R > 1 else logp.shape[1], values.data_ptr(), reward.data_ptr(), done.data_ptr(),
                                               _stream_ptr()))
    return forest


def mcts_decide(forest: MctsForest, sample: bool = False, seed: int = 0, counter: int = 0, finished: Optional[torch.Tensor] = None,
                move: Optional[torch.Tensor] = None, counts: Optional[torch.Tensor] = None) -> torch.Tensor:
    """The decision after a decision's simulations (`qg_mcts_decide`), one launch; the forest is only read.  Per tree the visit counts of
    the root's actions, n_a = visits of the child under action a, 0 where there is none, and the move they give: sample=False the action of
    the most visits among the expanded ones, the lowest among equals; sample=True the lowest a with n_0 + ... + n_a > r, where
    r = mulhi64(rng_draw(seed ^ 0x6D637473, tree, counter), sum of the counts) -- an action is drawn in proportion to its visits, in
    integers, the same for the same (seed, counter, tree); without any visit the answer of sample=False.  A where the root has no child.
    finished: optional uint8 / bool [M], trees whose real env is final: their move is A.  counts: optional int32 [M, >= A] with unit
    column stride, gets the rows of n_a (finished trees too; columns past A are left alone).  Returns move, int32 [M]; a preallocated one
    may be passed."""
    if not isinstance(forest, MctsForest):
        raise TypeError("mcts_decide: forest must come from mcts_forest")
    M, A, dev, i32 = forest.M, forest.A, forest.parent.device, torch.int32
    if finished is not None and finished.dtype == torch.bool:
        finished = finished.view(torch.uint8)
    if move is None:
        move = torch.empty(M, dtype=i32, device=dev)
    _mcts_vectors("mcts_decide", forest, (("finished", finished, torch.uint8), ("move", move, i32)))
    if counts is not None and (counts.dtype != i32 or counts.dim() != 2 or counts.shape[0] != M or counts.shape[1] < A or counts.device != dev or (
            counts.stride(1) != 1 and counts.shape[1] > 1) or (M > 1 and counts.stride(0) < A)):
        raise ValueError("mcts_decide: counts must be int32 [M, >= A] with unit column stride on the forest's device")
    ld = 0 if counts is None else counts.stride(0) if M > 1 else counts.shape[1]
    _lib.check(_lib.load().qg_mcts_decide(forest._c, _lib.MCTS_SAMPLE if sample else _lib.MCTS_MOST_VISITED, int(seed) & (2 ** 64 - 1), int(counter) & (2 ** 64 - 1),
                                          finished.data_ptr() if finished is not None else None, move.data_ptr(),
                                          counts.data_ptr() if counts is not None else None, ld, _stream_ptr()))
    return move


def mcts_rebase(forest: MctsForest, move: torch.Tensor, finished: Optional[torch.Tensor] = None, env_src: Optional[torch.Tensor] = None) -> torch.Tensor:
    """The step between two decisions (`qg_mcts_rebase`), one launch, in place on `forest`: per tree the subtree below the root's child by
    action `move` (int32 [M], `mcts_decide`'s) becomes the tree -- the kept nodes renumbered in their order, the child the new root -- so
    the next decision's simulations go on where this one's went.  finished: optional uint8 / bool [M], trees whose real env is final: left
    alone.  Returns env_src, int32 [M * cap] (a preallocated one may be passed): for every new pool index the old pool index of the
    node's env, `forest.skip` where there is none -- the `src_idx` of `other_pool.copy_envs(pool, env_src)`.  A tree with nothing to carry
    (no such child, a move of A) stays as it is and its env_src is the identity on its nodes."""
    if not isinstance(forest, MctsForest):
        raise TypeError("mcts_rebase: forest must come from mcts_forest")
    dev, i32 = forest.parent.device, torch.int32
    if finished is not None and finished.dtype == torch.bool:
        finished = finished.view(torch.uint8)
    if env_src is None:
        env_src = torch.empty(forest.M * forest.cap, dtype=i32, device=dev)
    _mcts_vectors("mcts_rebase", forest, (("finished", finished, torch.uint8), ("move", move, i32)))
    if move is None:
        raise ValueError("mcts_rebase: move is required")
    if env_src.dtype != i32 or env_src.dim() != 1 or env_src.numel() != forest.M * forest.cap or not env_src.is_contiguous() or env_src.device != dev:
        raise ValueError(f"mcts_rebase: env_src must be a contiguous [{forest.M * forest.cap}] int32 tensor on the forest's device")
    _lib.check(_lib.load().qg_mcts_rebase(forest._c, move.data_ptr(), finished.data_ptr() if finished is not None else None, env_src.data_ptr(),
                                          _stream_ptr()))
    return env_src


class AzPack(NamedTuple):
    """What `az_pack` writes, all on the device: n int32 [3] = (samples written, valid decisions, live rows with bad counts); per sample
    index int32 [capacity] (t * E + e), z f32 [capacity], move int32 [capacity], pi f32 [capacity, A], words [capacity, W] or None; and the
    call's scratch (uint8).  Only the first n[0] rows mean anything."""
    n: torch.Tensor
    index: torch.Tensor
    z: torch.Tensor
    move: torch.Tensor
    pi: torch.Tensor
    words: Optional[torch.Tensor]
    scratch: torch.Tensor


_AZ_WORD_DTYPES = {torch.uint8: 1, torch.int32: 4, torch.int64: 8}
if hasattr(torch, "uint32"):
    _AZ_WORD_DTYPES.update({torch.uint32: 4, torch.uint64: 8})


def az_pack(counts: torch.Tensor, reward: torch.Tensor, live: torch.Tensor, move: torch.Tensor, words: Optional[torch.Tensor] = None,
            capacity: Optional[int] = None, out: Optional[AzPack] = None) -> AzPack:
    """A finished self-play log -> a dense batch of training samples (`qg_az_pack`), four launches, no host read.  counts: int32 [T, E, A]
    with unit column stride (a view of [T, E, >= A] will do: the columns past A are never read), the rows `mcts_decide(counts=)` wrote;
    reward f32, live uint8 / bool, move int32, all contiguous [T, E]; words: optional contiguous [T, E, W] of 1-, 4- or 8-byte integers,
    the packed observation before the move.  The valid decisions -- live, no negative count, 0 < sum of the counts < 2^24 -- are compacted in
    t * E + e order, the first `capacity` of them (None: T * E) written: index, z = the undiscounted return to go in f32 (a live decision
    that is not valid still contributes its reward), the move, pi = counts / their sum, the words.  out: the `AzPack` of an earlier call
    of the same shapes, written again; rows at or past n[0] are left as they were.  Inputs and outputs may not alias."""
    i32, f32 = torch.int32, torch.float32
    if counts.dtype != i32 or counts.dim() != 3 or min(counts.shape) < 1:
        raise ValueError("az_pack: counts must be int32 [T, E, A] with T, E, A >= 1")
    T, E, A = counts.shape
    dev = counts.device
    ld = counts.stride(1) if E > 1 else counts.stride(0) if T > 1 else A  # the stride from one (t, e) row to the next
    if (A > 1 and counts.stride(2) != 1) or ld < A or (T > 1 and E > 1 and counts.stride(0) != E * ld):
        raise ValueError("az_pack: counts must have unit column stride and rows at one stride >= A over all of [T, E]")
    if live.dtype == torch.bool:
        live = live.view(torch.uint8)
    for nm, t, dt in (("reward", reward, f32), ("live", live, torch.uint8), ("move", move, i32)):
        if t is None or t.dtype != dt or tuple(t.shape) != (T, E) or not t.is_contiguous() or t.device != dev:
            raise ValueError(f"az_pack: {nm} must be a contiguous [{T}, {E}] {dt} tensor on the device of counts")
    W, wb = 0, 0
    if words is not None:
        if words.dtype not in _AZ_WORD_DTYPES or words.dim() != 3 or tuple(words.shape[:2]) != (T, E) or words.shape[2] < 1 or not words.is_contiguous() or words.device != dev:
            raise ValueError(f"az_pack: words must be a contiguous [{T}, {E}, W >= 1] tensor of 1-, 4- or 8-byte integers on the device of counts")
        W, wb = words.shape[2], _AZ_WORD_DTYPES[words.dtype]
    cap = T * E if capacity is None else int(capacity)
    if cap < 1:
        raise ValueError("az_pack: capacity must be at least 1")
    L = _lib.load()
    need = int(L.qg_az_pack_scratch_bytes(T, E))
    if need == 0:
        raise ValueError(f"az_pack: {T} decisions of {E} episodes are too many for 32-bit indices")
    if out is None:
        out = AzPack(torch.empty(3, dtype=i32, device=dev), torch.empty(cap, dtype=i32, device=dev), torch.empty(cap, dtype=f32, device=dev),
                     torch.empty(cap, dtype=i32, device=dev), torch.empty((cap, A), dtype=f32, device=dev),
                     torch.empty((cap, W), dtype=words.dtype, device=dev) if words is not None else None,
                     torch.empty(need, dtype=torch.uint8, device=dev))
    else:
        shapes = ((out.n, (3,), i32), (out.index, (cap,), i32), (out.z, (cap,), f32), (out.move, (cap,), i32), (out.scratch, None, torch.uint8)) + (
            ((out.words, (cap, W), words.dtype),) if words is not None else ())
        for t, shape, dt in shapes:
            if t is None or t.dtype != dt or t.device != dev or not t.is_contiguous() or (shape is not None and tuple(t.shape) != shape):
                raise ValueError("az_pack: out must be the AzPack of a call of the same shapes, capacity and device")
        if out.scratch.numel() < need:
            raise ValueError(f"az_pack: out.scratch holds {out.scratch.numel()} bytes, {need} are needed")
        # pi may be a view of wider rows: the columns past A are not written
        if out.pi.dtype != f32 or out.pi.device != dev or tuple(out.pi.shape) != (cap, A) or (A > 1 and out.pi.stride(1) != 1) or (cap > 1 and out.pi.stride(0) < A):
            raise ValueError(f"az_pack: out.pi must be f32 [{cap}, {A}] with unit column stride on the device of counts")
    pi_ld = out.pi.stride(0) if cap > 1 else A
    _lib.check(L.qg_az_pack(counts.data_ptr(), ld, reward.data_ptr(), live.data_ptr(), move.data_ptr(), words.data_ptr() if words is not None else None, wb, W,
                            T, E, A, cap, out.n.data_ptr(), out.index.data_ptr(), out.z.data_ptr(), out.move.data_ptr(), out.pi.data_ptr(), pi_ld,
                            out.words.data_ptr() if words is not None else None, out.scratch.data_ptr(), _stream_ptr()))
    return out


def gae(rewards: torch.Tensor, values: torch.Tensor, dones: torch.Tensor, last_values: Optional[torch.Tensor], gamma: float,
        gae_lambda: float, advantages: Optional[torch.Tensor] = None, returns: Optional[torch.Tensor] = None):
    """GAE(lambda) over a [T, B] rollout; `dones[t]` = the episode ended with step t.  Returns (advantages, returns)."""
    T, B = rewards.shape
    for x, dt in ((rewards, torch.float32), (values, torch.float32), (dones, torch.uint8)):
        if x.shape != (T, B) or x.dtype != dt or not x.is_contiguous():
            raise ValueError("gae: rewards/values must be contiguous f32 [T, B], dones uint8 [T, B]")
    advantages = torch.empty_like(rewards) if advantages is None else advantages
    returns = torch.empty_like(rewards) if returns is None else returns
    lv = None
    if last_values is not None:
        lv = last_values.to(torch.float32).contiguous()
    _lib.check(_lib.load().qg_gae(rewards.data_ptr(), values.data_ptr(), dones.data_ptr(), lv.data_ptr() if lv is not None else None,
                                  float(gamma), float(gae_lambda), T, B, advantages.data_ptr(), returns.data_ptr(), _stream_ptr()))
    return advantages, returns


def expand_packed(packed: torch.Tensor, cols: int, dtype: torch.dtype, out: Optional[torch.Tensor] = None) -> torch.Tensor:
    """Bit-packed observation rows (`VecEnv.observe_packed`, any leading shape) -> dense {0,1} [..., rows, cols] in `dtype`."""
    packed = packed.contiguous()
    if out is None:
        out = torch.empty((*packed.shape, cols), dtype=dtype, device=packed.device)
    _lib.check(_lib.load().qg_expand_packed(packed.data_ptr(), packed.element_size(), packed.numel(), int(cols), out.data_ptr(), _DT[dtype],
                                            _stream_ptr()))
    return out


def _twist_operands(name: str, perms: torch.Tensor, twist_idx: torch.Tensor, batch: int, width: int, dev):
    if perms.dtype != torch.int32 or perms.dim() != 2 or perms.shape[1] != width or perms.shape[0] < 1 or not perms.is_contiguous() or perms.device != dev:
        raise ValueError(f"{name}: the permutation table must be a contiguous int32 [n_twists, {width}] tensor on the device of the input")
    if twist_idx.dtype != torch.int32 or twist_idx.numel() != batch or not twist_idx.is_contiguous() or twist_idx.device != dev:
        raise ValueError(f"{name}: twist_idx must be a contiguous int32 [{batch}] tensor on the device of the input")


def twist_expand_packed(packed: torch.Tensor, cols: int, obs_perms: torch.Tensor, twist_idx: torch.Tensor, dtype: torch.dtype,
                        out: Optional[torch.Tensor] = None) -> torch.Tensor:
    """Symmetry views of packed observations (`qg_twist_expand_packed`): out[e, i] = element obs_perms[twist_idx[e]][i] of what
    `expand_packed` writes for env e -- a gather through the table, made while the bits are expanded.  packed: [B, rows] of 1-, 4- or 8-byte
    integers (`VecEnv.observe_packed`); obs_perms: int32 [n_twists, rows*cols] (any table: the kernel knows no env); twist_idx: int32 [B],
    an index outside [0, n_twists) gives that env its untwisted observation.  Returns dense {0,1} [B, rows*cols] in `dtype`."""
    if packed.dim() != 2 or not packed.is_contiguous() or packed.is_floating_point() or packed.element_size() not in (1, 4, 8):
        raise ValueError("twist_expand_packed: packed must be a contiguous [B, rows] tensor of 1-, 4- or 8-byte integers")
    B, rows = packed.shape
    _twist_operands("twist_expand_packed", obs_perms, twist_idx, B, rows * int(cols), packed.device)
    if out is None:
        out = torch.empty((B, rows * int(cols)), dtype=dtype, device=packed.device)
    if out.dtype != dtype or out.numel() != B * rows * int(cols) or not out.is_contiguous() or out.device != packed.device:
        raise ValueError("twist_expand_packed: `out` must be a contiguous [B, rows*cols] tensor of the requested dtype on the device of packed")
    _lib.check(_lib.load().qg_twist_expand_packed(packed.data_ptr(), packed.element_size(), B, rows, int(cols), obs_perms.data_ptr(), obs_perms.shape[0],
                                                  twist_idx.data_ptr(), out.data_ptr(), _DT[dtype], _stream_ptr()))
    return out


def twist_pack_words(packed: torch.Tensor, cols: int, obs_perms: torch.Tensor, twist_idx: torch.Tensor, rows_out: Optional[int] = None,
                     out: Optional[torch.Tensor] = None) -> torch.Tensor:
    """`twist_expand_packed` with the view left packed (`qg_twist_pack_words`): int64 [B, rows_out], bit c of out[e, r] = element
    obs_perms[twist_idx[e]][r*cols + c] of what `expand_packed` writes for env e; bits past `cols` and the words rows .. rows_out-1 are 0.
    The operands are those of `twist_expand_packed` (cols <= 64); rows_out defaults to rows rounded up to even, the row count
    `embed_words` takes -- with a first layer packed from the weight padded by `cols` zero columns when rows is odd."""
    if packed.dim() != 2 or not packed.is_contiguous() or packed.is_floating_point() or packed.element_size() not in (1, 4, 8):
        raise ValueError("twist_pack_words: packed must be a contiguous [B, rows] tensor of 1-, 4- or 8-byte integers")
    B, rows = packed.shape
    _twist_operands("twist_pack_words", obs_perms, twist_idx, B, rows * int(cols), packed.device)
    rows_out = (rows + 1) // 2 * 2 if rows_out is None else int(rows_out)
    if rows_out < rows:
        raise ValueError(f"twist_pack_words: rows_out must be at least the {rows} rows of the input")
    if out is None:
        out = torch.empty((B, rows_out), dtype=torch.int64, device=packed.device)
    if out.dtype != torch.int64 or out.numel() != B * rows_out or not out.is_contiguous() or out.device != packed.device:
        raise ValueError("twist_pack_words: `out` must be a contiguous int64 [B, rows_out] tensor on the device of packed")
    _lib.check(_lib.load().qg_twist_pack_words(packed.data_ptr(), packed.element_size(), B, rows, int(cols), obs_perms.data_ptr(), obs_perms.shape[0],
                                               twist_idx.data_ptr(), out.data_ptr(), rows_out, _stream_ptr()))
    return out


def untwist_actions(actions: torch.Tensor, act_perms: torch.Tensor, twist_idx: torch.Tensor, out: Optional[torch.Tensor] = None) -> torch.Tensor:
    """Actions chosen on views -> real actions (`qg_untwist_actions`): out[e] = act_perms[twist_idx[e]][actions[e]].  actions: int32 / int64
    [B]; act_perms: int32 [n_twists, num_actions]; twist_idx: int32 [B].  An action outside [0, num_actions) and every action of an env whose
    twist index is out of range pass through unchanged.  `out` may be `actions` itself."""
    if actions.dtype not in (torch.int32, torch.int64) or actions.dim() != 1 or not actions.is_contiguous():
        raise ValueError("untwist_actions: actions must be a contiguous int32 / int64 [B] tensor")
    B = actions.numel()
    _twist_operands("untwist_actions", act_perms, twist_idx, B, act_perms.shape[1] if act_perms.dim() == 2 else 0, actions.device)
    out = torch.empty_like(actions) if out is None else out
    if out.dtype != actions.dtype or out.numel() != B or not out.is_contiguous() or out.device != actions.device:
        raise ValueError("untwist_actions: `out` must match actions in dtype, size and device")
    act_dt = {torch.int32: _lib.ACT_I32, torch.int64: _lib.ACT_I64}[actions.dtype]
    _lib.check(_lib.load().qg_untwist_actions(actions.data_ptr(), act_dt, B, act_perms.shape[1], act_perms.data_ptr(), act_perms.shape[0],
                                              twist_idx.data_ptr(), out.data_ptr(), _stream_ptr()))
    return out


def pack_embedding(env: VecEnv, weight: torch.Tensor, out: Optional[torch.Tensor] = None) -> torch.Tensor:
    """First-layer weight [hidden, rows*cols] (f32 / bf16) in the k order `embed` consumes (`qg_vec_pack_embedding`);
    repack after every optimiser step (pass `out` to rewrite the same buffer: graph-safe)."""
    if weight.dim() != 2 or weight.stride(1) != 1:
        raise ValueError("weight must be [hidden, obs_size] with unit column stride")
    L = _lib.load()
    hidden = weight.shape[0]
    nbytes = L.qg_vec_embed_packed_bytes(env._h, hidden)
    if nbytes == 0:
        raise ValueError("embed needs a TILE-layout env (CliffordEnv N <= 16, LinearFunctionEnv 8 < N <= 32) and hidden % 64 == 0")
    if out is None:
        out = torch.empty(nbytes // 2, dtype=torch.bfloat16, device=weight.device)
    _lib.check(L.qg_vec_pack_embedding(env._h, weight.data_ptr(), _DT[weight.dtype], weight.stride(0), hidden, out.data_ptr(), env._stream()))
    return out


def embed(env: VecEnv, packed: torch.Tensor, bias: Optional[torch.Tensor], hidden: int, relu: bool = True, out: Optional[torch.Tensor] = None,
          obs_out: Optional[torch.Tensor] = None) -> torch.Tensor:
    """act(obs @ W.T + bias) in bf16 [B, hidden], computed from the env's resident bit-packed state (`qg_vec_embed`).  `obs_out`: also
    `env.observe_packed(out=obs_out)` of the same state (`qg_vec_embed_observe`: one launch for small batches)."""
    if out is None:
        out = torch.empty((env.batch, hidden), dtype=torch.bfloat16, device=env.device)
    if bias is not None and (bias.dtype != torch.float32 or not bias.is_contiguous()):
        raise ValueError("bias must be a contiguous f32 vector")
    L = _lib.load()
    if obs_out is not None:
        if (not obs_out.is_contiguous() or obs_out.numel() != env.batch * env.packed_words_per_env or obs_out.element_size() != env.packed_word_bytes
                or obs_out.device != out.device):
            raise ValueError("obs_out must be a contiguous [batch, packed_words_per_env] tensor of the env's packed word type on its device")
        _lib.check(L.qg_vec_embed_observe(env._h, packed.data_ptr(), bias.data_ptr() if bias is not None else None, hidden, int(relu), out.data_ptr(),
                                          out.stride(0), obs_out.data_ptr(), env._stream()))
        return out
    _lib.check(L.qg_vec_embed(env._h, packed.data_ptr(), bias.data_ptr() if bias is not None else None, hidden, int(relu), out.data_ptr(),
                              out.stride(0), env._stream()))
    return out


def pack_embed_words(weight: torch.Tensor, rows: int, cols: int, out: Optional[torch.Tensor] = None) -> torch.Tensor:
    """First-layer weight [hidden, rows*cols] (f32 / bf16) in the order `embed_words` consumes (`qg_policy_pack_embed_words`)."""
    if weight.dim() != 2 or weight.stride(1) != 1:
        raise ValueError("weight must be [hidden, rows*cols] with unit column stride")
    L = _lib.load()
    nbytes = L.qg_policy_embed_words_packed_bytes(int(rows), int(cols), weight.shape[0])
    if nbytes == 0:
        raise ValueError("embed_words needs an even number of rows, cols <= 64 and hidden % 128 == 0")
    if out is None:
        out = torch.empty(nbytes // 2, dtype=torch.bfloat16, device=weight.device)
    _lib.check(L.qg_policy_pack_embed_words(weight.data_ptr(), _DT[weight.dtype], weight.stride(0), int(rows), int(cols), weight.shape[0], out.data_ptr(),
                                            _stream_ptr()))
    return out


def embed_words(words: torch.Tensor, cols: int, packed: torch.Tensor, bias: Optional[torch.Tensor], hidden: int, relu: bool = True,
                out: Optional[torch.Tensor] = None) -> torch.Tensor:
    """act(obs @ W.T + bias) in bf16 [B, hidden] from packed observation rows [B, rows] int64 (`VecEnv.observe_packed` of a handle with
    64-bit row words, a packed rollout buffer, a gathered shard): `qg_policy_embed_words`."""
    if words.dim() != 2 or words.dtype != torch.int64 or not words.is_contiguous():
        raise ValueError("words must be a contiguous int64 [B, rows] tensor")
    B, rows = words.shape
    if out is None:
        out = torch.empty((B, hidden), dtype=torch.bfloat16, device=words.device)
    if bias is not None and (bias.dtype != torch.float32 or not bias.is_contiguous()):
        raise ValueError("bias must be a contiguous f32 vector")
    _lib.check(_lib.load().qg_policy_embed_words(words.data_ptr(), B, rows, int(cols), packed.data_ptr(), bias.data_ptr() if bias is not None else None, hidden,
                                                 int(relu), out.data_ptr(), out.stride(0), _stream_ptr()))
    return out


def pack_head(weight: torch.Tensor, bias: Optional[torch.Tensor], num_actions: int, value_row: int, out: Optional[torch.Tensor] = None,
              after_mid: bool = False) -> torch.Tensor:
    """Last-layer weight [rows, in_features] (+ bias [rows]; f32 or bf16, same dtype) in the order `head_sample` (or, with
    after_mid, `mid_head_sample`) consumes: rows 0..num_actions-1 are the actions, row `value_row` the value head (`qg_policy_pack_head`)."""
    L = _lib.load()
    nbytes = L.qg_policy_head_packed_bytes(num_actions, weight.shape[1])
    if nbytes == 0:
        raise ValueError("fused head needs num_actions <= 222 and in_features % 64 == 0, <= 512")
    if weight.stride(1) != 1 or (bias is not None and (bias.dtype != weight.dtype or not bias.is_contiguous())):
        raise ValueError("weight must have unit column stride; bias contiguous and of the same dtype")
    if out is None:
        out = torch.empty(nbytes // 2, dtype=torch.bfloat16, device=weight.device)
    _lib.check(L.qg_policy_pack_head(weight.data_ptr(), bias.data_ptr() if bias is not None else None, _DT[weight.dtype], weight.stride(0), weight.shape[1],
                                     int(num_actions), int(value_row), int(after_mid), out.data_ptr(), _stream_ptr()))
    return out


def pack_mid(weight: torch.Tensor, bias: Optional[torch.Tensor], out: Optional[torch.Tensor] = None) -> torch.Tensor:
    """Middle-layer weight [256, in_features] (+ bias) in the order `mid_head_sample` consumes (`qg_policy_pack_mid`)."""
    L = _lib.load()
    nbytes = L.qg_policy_mid_packed_bytes(weight.shape[1], weight.shape[0])
    if nbytes == 0:
        raise ValueError("fused middle layer needs 256 output features and in_features % 32 == 0, <= 2048")
    if weight.stride(1) != 1 or (bias is not None and (bias.dtype != weight.dtype or not bias.is_contiguous())):
        raise ValueError("weight must have unit column stride; bias contiguous and of the same dtype")
    if out is None:
        out = torch.empty(nbytes // 2, dtype=torch.bfloat16, device=weight.device)
    _lib.check(L.qg_policy_pack_mid(weight.data_ptr(), bias.data_ptr() if bias is not None else None, _DT[weight.dtype], weight.stride(0), weight.shape[1],
                                    weight.shape[0], out.data_ptr(), _stream_ptr()))
    return out


def mid_head_sample(h: torch.Tensor, packed_mid: torch.Tensor, mid_features: int, packed_head: torch.Tensor, num_actions: int, seed: int, counter: int,
                    actions: Optional[torch.Tensor] = None, logp: Optional[torch.Tensor] = None, entropy: Optional[torch.Tensor] = None,
                    values: Optional[torch.Tensor] = None, clock: Optional[torch.Tensor] = None):
    """relu(h W2^T + b2) -> last layer -> categorical draw in one kernel (`qg_policy_mid_head_sample`); the head packed with after_mid=True."""
    if h.dim() != 2 or h.dtype != torch.bfloat16 or h.stride(1) != 1:
        raise ValueError("h must be bf16 [B, in_features] with unit column stride")
    B, dev = h.shape[0], h.device
    actions = torch.empty(B, dtype=torch.int64, device=dev) if actions is None else actions
    logp = torch.empty(B, dtype=torch.float32, device=dev) if logp is None else logp
    entropy = torch.empty(B, dtype=torch.float32, device=dev) if entropy is None else entropy
    values = torch.empty(B, dtype=torch.float32, device=dev) if values is None else values
    act_dt = {torch.int32: _lib.ACT_I32, torch.int64: _lib.ACT_I64}[actions.dtype]
    _lib.check(_lib.load().qg_policy_mid_head_sample(h.data_ptr(), h.stride(0), B, h.shape[1], packed_mid.data_ptr(), int(mid_features), packed_head.data_ptr(),
                                                     int(num_actions), int(seed) & (2**64 - 1), int(counter), clock.data_ptr() if clock is not None else None,
                                                     actions.data_ptr(), act_dt, logp.data_ptr(), entropy.data_ptr(), values.data_ptr(), _stream_ptr()))
    return actions, logp, entropy, values


def mid_head_sample_step(env: VecEnv, h: torch.Tensor, packed_mid: torch.Tensor, mid_features: int, packed_head: torch.Tensor, seed: int, counter: int,
                         actions: torch.Tensor, logp: torch.Tensor, entropy: torch.Tensor, values: torch.Tensor,
                         rewards: Optional[torch.Tensor] = None, dones: Optional[torch.Tensor] = None, reset_seed: Optional[int] = None):
    """`mid_head_sample` followed, in the same launch, by `env.step(actions)` and by the compaction of the finished envs for the next
    `env.reset_done` (`qg_vec_mid_head_sample_step`): same draws, same env results, two launches less per collection step.  The env's
    device clock (`env.set_clock`) is the sampling clock.  `reset_seed`: also `env.reset_done(reset_seed)` (`..._step_reset`: inside the
    same launch for small batches)."""
    if h.dim() != 2 or h.dtype != torch.bfloat16 or h.stride(1) != 1 or h.shape[0] != env.batch:
        raise ValueError("h must be bf16 [env.batch, in_features] with unit column stride")
    act_dt = {torch.int32: _lib.ACT_I32, torch.int64: _lib.ACT_I64}[actions.dtype]
    args = (env._h, h.data_ptr(), h.stride(0), h.shape[1], packed_mid.data_ptr(), int(mid_features), packed_head.data_ptr(), int(seed) & (2**64 - 1),
            int(counter), actions.data_ptr(), act_dt, logp.data_ptr(), entropy.data_ptr(), values.data_ptr(),
            rewards.data_ptr() if rewards is not None else None, dones.data_ptr() if dones is not None else None)
    if reset_seed is None:
        _lib.check(_lib.load().qg_vec_mid_head_sample_step(*args, env._stream()))
    else:
        _lib.check(_lib.load().qg_vec_mid_head_sample_step_reset(*args, int(reset_seed) & (2**64 - 1), env._stream()))
    return actions, logp, entropy, values


def head_sample(h: torch.Tensor, packed: torch.Tensor, num_actions: int, seed: int, counter: int, actions: Optional[torch.Tensor] = None,
                logp: Optional[torch.Tensor] = None, entropy: Optional[torch.Tensor] = None, values: Optional[torch.Tensor] = None,
                clock: Optional[torch.Tensor] = None):
    """Last layer + categorical draw in one kernel (`qg_policy_head_sample`): h bf16 [B, in_features] -> (actions, logp, entropy, values)."""
    if h.dim() != 2 or h.dtype != torch.bfloat16 or h.stride(1) != 1:
        raise ValueError("h must be bf16 [B, in_features] with unit column stride")
    B, dev = h.shape[0], h.device
    actions = torch.empty(B, dtype=torch.int64, device=dev) if actions is None else actions
    logp = torch.empty(B, dtype=torch.float32, device=dev) if logp is None else logp
    entropy = torch.empty(B, dtype=torch.float32, device=dev) if entropy is None else entropy
    values = torch.empty(B, dtype=torch.float32, device=dev) if values is None else values
    act_dt = {torch.int32: _lib.ACT_I32, torch.int64: _lib.ACT_I64}[actions.dtype]
    _lib.check(_lib.load().qg_policy_head_sample(h.data_ptr(), h.stride(0), B, h.shape[1], packed.data_ptr(), int(num_actions), int(seed) & (2**64 - 1),
                                                 int(counter), clock.data_ptr() if clock is not None else None, actions.data_ptr(), act_dt,
                                                 logp.data_ptr(), entropy.data_ptr(), values.data_ptr(), _stream_ptr()))
    return actions, logp, entropy, values


def _logp_outputs(name: str, B: int, A: int, dev, want_rows: bool, logp_rows, actions, best_logp, entropy, values):
    """Outputs of the two `_logp` wrappers: allocated where None (rows with a stride rounded up to 4 floats: 16-byte stores), checked otherwise."""
    if want_rows and logp_rows is None:
        logp_rows = torch.empty((B, (A + 3) // 4 * 4), dtype=torch.float32, device=dev)[:, :A]
    if not want_rows:
        logp_rows = None
    elif (logp_rows.dtype != torch.float32 or logp_rows.dim() != 2 or logp_rows.shape[0] != B or logp_rows.shape[1] < A or logp_rows.device != dev
          or (logp_rows.stride(1) != 1 and logp_rows.shape[1] > 1) or (B > 1 and logp_rows.stride(0) < A)):
        raise ValueError(f"{name}: logp_rows must be f32 [B, >= num_actions] with unit column stride on the device of h")
    actions = torch.empty(B, dtype=torch.int64, device=dev) if actions is None else actions
    best_logp = torch.empty(B, dtype=torch.float32, device=dev) if best_logp is None else best_logp
    entropy = torch.empty(B, dtype=torch.float32, device=dev) if entropy is None else entropy
    values = torch.empty(B, dtype=torch.float32, device=dev) if values is None else values
    if actions.dtype not in (torch.int32, torch.int64) or actions.numel() != B or not actions.is_contiguous() or actions.device != dev:
        raise ValueError(f"{name}: actions must be a contiguous int32 / int64 [B] tensor on the device of h")
    for nm, t in (("best_logp", best_logp), ("entropy", entropy), ("values", values)):
        if t.dtype != torch.float32 or t.numel() != B or not t.is_contiguous() or t.device != dev:
            raise ValueError(f"{name}: {nm} must be a contiguous f32 [B] tensor on the device of h")
    return logp_rows, actions, best_logp, entropy, values


def mid_head_logp(h: torch.Tensor, packed_mid: torch.Tensor, mid_features: int, packed_head: torch.Tensor, num_actions: int, want_rows: bool = True,
                  logp_rows: Optional[torch.Tensor] = None, actions: Optional[torch.Tensor] = None, best_logp: Optional[torch.Tensor] = None,
                  entropy: Optional[torch.Tensor] = None, values: Optional[torch.Tensor] = None):
    """`mid_head_sample` without the draw (`qg_policy_mid_head_logp`): relu(h W2^T + b2) -> last layer -> the whole row of log-probabilities
    and the arg-max (equal logits: the lowest action), in one kernel, from the same operands.  Returns (logp_rows f32 [B, num_actions] --
    -inf where an action is masked, ready for `beam_select`; None with want_rows=False, which writes no row: the greedy step --, actions,
    best_logp = logp_rows[e, actions[e]], entropy, values).  Preallocated outputs may be passed; `logp_rows` may be any f32 [B, >= num_actions]
    view with unit column stride (rows of 16-byte aligned base and stride are written 16 bytes at a time)."""
    if h.dim() != 2 or h.dtype != torch.bfloat16 or h.stride(1) != 1:
        raise ValueError("h must be bf16 [B, in_features] with unit column stride")
    B, A = h.shape[0], int(num_actions)
    logp_rows, actions, best_logp, entropy, values = _logp_outputs("mid_head_logp", B, A, h.device, want_rows, logp_rows, actions, best_logp, entropy, values)
    act_dt = {torch.int32: _lib.ACT_I32, torch.int64: _lib.ACT_I64}[actions.dtype]
    _lib.check(_lib.load().qg_policy_mid_head_logp(h.data_ptr(), h.stride(0), B, h.shape[1], packed_mid.data_ptr(), int(mid_features), packed_head.data_ptr(), A,
                                                   logp_rows.data_ptr() if logp_rows is not None else None,
                                                   (logp_rows.stride(0) if B > 1 else logp_rows.shape[1]) if logp_rows is not None else A,
                                                   actions.data_ptr(), act_dt, best_logp.data_ptr(), entropy.data_ptr(), values.data_ptr(), _stream_ptr()))
    return (logp_rows[:, :A] if logp_rows is not None else None), actions, best_logp, entropy, values


def head_logp(h: torch.Tensor, packed: torch.Tensor, num_actions: int, want_rows: bool = True, logp_rows: Optional[torch.Tensor] = None,
              actions: Optional[torch.Tensor] = None, best_logp: Optional[torch.Tensor] = None, entropy: Optional[torch.Tensor] = None,
              values: Optional[torch.Tensor] = None):
    """`head_sample` without the draw (`qg_policy_head_logp`): last layer -> log-prob rows and arg-max; arguments and results as `mid_head_logp`."""
    if h.dim() != 2 or h.dtype != torch.bfloat16 or h.stride(1) != 1:
        raise ValueError("h must be bf16 [B, in_features] with unit column stride")
    B, A = h.shape[0], int(num_actions)
    logp_rows, actions, best_logp, entropy, values = _logp_outputs("head_logp", B, A, h.device, want_rows, logp_rows, actions, best_logp, entropy, values)
    act_dt = {torch.int32: _lib.ACT_I32, torch.int64: _lib.ACT_I64}[actions.dtype]
    _lib.check(_lib.load().qg_policy_head_logp(h.data_ptr(), h.stride(0), B, h.shape[1], packed.data_ptr(), A,
                                               logp_rows.data_ptr() if logp_rows is not None else None,
                                               (logp_rows.stride(0) if B > 1 else logp_rows.shape[1]) if logp_rows is not None else A,
                                               actions.data_ptr(), act_dt, best_logp.data_ptr(), entropy.data_ptr(), values.data_ptr(), _stream_ptr()))
    return (logp_rows[:, :A] if logp_rows is not None else None), actions, best_logp, entropy, values


class BasicPolicy(nn.Module):
    def __init__(self, obs_size: int, num_actions: int, embedding_size: int = 512, common: int = 256):
        super().__init__()
        self.embeddings = nn.Linear(obs_size, embedding_size)
        self.common = nn.Linear(embedding_size, common)
        self.policy_head = nn.Linear(common, num_actions)
        self.value_head = nn.Linear(common, 1)

    def forward(self, obs_flat: torch.Tensor):
        h = torch.relu(self.embeddings(obs_flat))
        h = torch.relu(self.common(h))
        return self.policy_head(h), self.value_head(h).squeeze(-1)

    @torch.no_grad()
    def fused_heads(self) -> Tuple[torch.Tensor, torch.Tensor, int]:
        """Policy and value heads as ONE weight [pad8(A + 1), common] / bias, so a collection step runs
        three GEMMs; column A of the output is the value.  Rebuild after every optimiser step."""
        A = self.policy_head.out_features
        rows = (A + 1 + 7) // 8 * 8
        w = torch.zeros((rows, self.common.out_features), dtype=self.policy_head.weight.dtype, device=self.policy_head.weight.device)
        b = torch.zeros(rows, dtype=w.dtype, device=w.device)
        w[:A], w[A] = self.policy_head.weight, self.value_head.weight[0]
        b[:A], b[A] = self.policy_head.bias, self.value_head.bias[0]
        return w, b, A


def _linear_relu(x: torch.Tensor, w: torch.Tensor, b: torch.Tensor) -> torch.Tensor:
    try:  # bias + ReLU in the GEMM epilogue (hipBLASLt)
        return torch._addmm_activation(b, x, w.t())
    except Exception:  # pragma: no cover - older torch
        return torch.relu_(torch.addmm(b, x, w.t()))


@dataclass
class FirstLayer:
    """The first layer packed for one route of the kernel forward: "state" is `embed` on the handle's resident bits (TILE layout), "words"
    `embed_words` on `observe_packed` (64-bit row words: PauliEnv, wide CliffordEnv), "views" `embed_words` on `observe_twisted_words`."""
    route: str
    weight: torch.Tensor


def pack_first(route: str, vec: VecEnv, weight: torch.Tensor, out: Optional[torch.Tensor] = None) -> torch.Tensor:
    """The first-layer weight [hidden, rows*cols] packed for `route` on the handle `vec`, into `out` if given; ValueError (or the
    library's error) where the route does not take the handle or the shape.  "state" packs through the handle that will read it.  The two
    words routes read one 64-bit word per observation row; a view's row count is the env's rounded up to even, so at an odd row count
    the weight gets `cols` zero columns for the pad word (a padded copy: that route is not repacked in place)."""
    rows, cols = vec.obs_shape_
    if route == "state":
        return pack_embedding(vec, weight, out=out)
    if route == "words":
        if vec.packed_word_bytes != 8 or vec.packed_words_per_env != rows:
            raise ValueError("embed_words reads one 64-bit word per observation row")
        return pack_embed_words(weight, rows, cols, out=out)
    if cols > 64 or vec.packed_words_per_env != rows:
        raise ValueError("a row of the view is one 64-bit word")
    w = weight.detach()
    if rows % 2:
        w = torch.nn.functional.pad(w, (0, cols))
    return pack_embed_words(w, rows + rows % 2, cols, out=out)


def first_layer(vec: VecEnv, weight: torch.Tensor, routes: Tuple[str, ...] = ("state", "words")) -> FirstLayer:
    """The one place that chooses a handle's first-layer route: the first of `routes` whose packer accepts the handle and the shape
    ("state" before "words"; ("views",) for a search under twists; the collector leaves "words" out where it stores no packed row).
    ValueError with the last packer's reason where none does."""
    reason = "no route to try"
    for route in routes:
        try:
            return FirstLayer(route, pack_first(route, vec, weight))
        except (ValueError, _lib.QGymError) as e:
            reason = str(e)
    raise ValueError(reason)


def run_first_layer(first: FirstLayer, vec: VecEnv, bias: torch.Tensor, hidden: int, out: torch.Tensor, words: Optional[torch.Tensor] = None,
                    obs_out: Optional[torch.Tensor] = None, tw: Optional[torch.Tensor] = None) -> torch.Tensor:
    """relu(obs W1^T + b1) of the handle's current state into `out` (bf16 [B, hidden]): the single dispatch to `embed`, `embed_observe`
    and `embed_words`.  "state": `obs_out`, if given, also receives the packed observation, in the same launch.  "words": the packed
    observation is written to `words` (a rollout row, a scratch buffer) and read from there.  "views": so is the view under `tw`."""
    if first.route == "state":
        return embed(vec, first.weight, bias, hidden, relu=True, out=out, obs_out=obs_out)
    if first.route == "words":
        words = vec.observe_packed(out=words)
    else:
        words = vec.observe_twisted_words(tw, words.shape[1], out=words)
    return embed_words(words, vec.obs_shape_[1], first.weight, bias, hidden, relu=True, out=out)


class PolicyOperands:
    """What the kernels (and the library GEMMs of the collector's other tails) read of a `BasicPolicy` beside a handle's first layer:
    `w`, `b`, `A` the fused head (`BasicPolicy.fused_heads`); `bias` the first layer's, f32; `mid` the packed middle layer, None where
    `pack_mid` refuses the shape; `head` the packed last layer, for `mid_head_sample` where `mid` is there and for `head_sample` where
    not, None where `pack_head` refuses -- and then `mid` is None too: there is no kernel for it alone.  `why` keeps the first refusal.
    fused_tail=False packs neither (the collector: another dtype than bf16, or switched off)."""

    def __init__(self, policy: BasicPolicy, fused_tail: bool = True):
        self.w, self.b, self.A = policy.fused_heads()
        self.bias = policy.embeddings.bias.detach().float().contiguous()
        self.mid = self.head = self.why = None
        if not fused_tail:
            return
        try:
            self.mid = pack_mid(policy.common.weight, policy.common.bias)
        except ValueError as e:
            self.why = str(e)
        try:
            self.head = pack_head(self.w, self.b, self.A, self.A, after_mid=self.mid is not None)
        except ValueError as e:
            self.mid, self.why = None, self.why or str(e)

    @torch.no_grad()
    def repack_(self, policy: BasicPolicy, first: Optional[FirstLayer] = None, vec: Optional[VecEnv] = None):
        """Every buffer again from the policy's current weights, in place -- and `first`, packed for `vec`, with the first layer's bias:
        no allocation, every `data_ptr()` stays, so this can run inside a captured collection and a replay follows an in-place
        parameter update."""
        w, b, A = self.w, self.b, self.A
        w[:A].copy_(policy.policy_head.weight)
        w[A].copy_(policy.value_head.weight[0])
        b[:A].copy_(policy.policy_head.bias)
        b[A : A + 1].copy_(policy.value_head.bias)
        if first is not None:
            pack_first(first.route, vec, policy.embeddings.weight, out=first.weight)
            self.bias.copy_(policy.embeddings.bias)
        if self.head is not None:
            pack_head(w, b, A, A, out=self.head, after_mid=self.mid is not None)
        if self.mid is not None:
            pack_mid(policy.common.weight, policy.common.bias, out=self.mid)
