"""Batched synthesis: many targets x many policy-guided searches as ONE env batch on the GPU.

The inference-side caller of the hot path.  The reference's `RLSynthesis.synth(input)`
(src/qiskit_gym/rl/synthesis.py:111-126) is `env.get_state(input)` -> twisterl's
`algorithm.solve(state, deterministic, num_searches, ...)` -> `env.build_circuit_from_solution`: per
target, `num_searches` episodes that clone the scalar env, `set_state` it and step it under the
policy until `is_final`, one target at a time on the CPU.  Here every (target, search) pair is one env
of a `VecEnv` batch: `set_state` once, then observe -> policy -> draw -> `env.step` for all of them per
launch, and the successful episode with the highest return (the env's own metrics-weighted reward,
metrics.rs:135-146) wins per target.  Same seed => same draws => same circuits.

The search batch runs without inversions and observation permutations (both are training-time
augmentations: clifford.rs:262-270, pauli.rs:653-665), so a solution is the winner's action sequence;
PauliGym solutions also carry the rotations each gate released (pauli.rs:612-626), which are
recovered by replaying the winners on a `track_solution` batch.

`solve(..., beam_width=W)` searches differently: a deterministic beam search over the policy's log-probabilities, W beams per target, on
the batched clone (`VecEnv.copy_envs`) and the device-side selection kernel (`collector.beam_select`); see `solve`.  `bound="stop"` ends a
target's search once no beam of it can beat its winner (`collector.beam_advance`, which is also the step's bookkeeping in one launch).

`solve(..., deterministic=True, num_mcts_searches=N)` is the reference's third way to search: a PUCT tree search per target, N simulations
per decision, the trees in plain device arrays (`collector.mcts_forest`), selection and backup on two kernels (`collector.mcts_select`,
`collector.mcts_backup`), the expansion on the batched clone and one forward pass for all targets; see `solve`.  `mcts_sampled=True` is the
reference's default shape of that call: `num_searches` tree-search episodes per target, every move drawn from the root's visit counts on the
device (`collector.mcts_decide`), the best successful episode kept.

`solve(..., fast=True)` takes the policy off the tensor library: the first layer reads the bit-packed state (`collector.embed` /
`embed_words`), the rest is one kernel that either draws (`mid_head_sample`: the sampled searches) or, for the greedy and the beam search,
writes the arg-max and the row of log-probabilities (`mid_head_logp`), which `beam_select` reads as it stands.

`solve(..., twists=V)` gives every target V symmetry views (`VecEnv.observe_twisted` / `untwist_actions`): the policy looks at a target through
an automorphism of the coupling map and its choice is mapped back, what `RLSynthesis.init_algorithm` hands the reference's policy as
`obs_perms` / `act_perms` (rl/synthesis.py:97-104) -- here one fixed view per search, so the deterministic searches get V opinions per target.
`twist_kernels=True` runs such a search on the policy-layer kernels: the view is written as packed words (`VecEnv.observe_twisted_words`),
which is what `embed_words` reads.

How the policy's opinion about a handle's current state is obtained is one decision, taken once per `solve`: the step loops ask a forward
object (`_TorchForward`, `_KernelForward`) for the row of log-probabilities, the arg-max or the draw, and know nothing else about it.  The
kernels' operands are a snapshot of the weights (`_Packed`: the `policy_kernels.PolicyOperands` the collector also holds, plus the version
counters they were taken at); the first layer packed through a handle (`policy_kernels.first_layer` names its route) stays with the
handle's owner (`_Handles.first`) and goes when the handle is closed or the snapshot dropped.  What a beam search does with a step's
results (returns, winners, `live`) is likewise one thing in every mode: `collector.beam_advance`.
"""
from __future__ import annotations

from collections import namedtuple
from dataclasses import dataclass, field
from typing import Dict, List, Optional, Sequence, Tuple

import numpy as np
import torch

from . import _lib
from .collector import SelfPlayBatch
from .envs.gyms import ROTATION_MARKER
from .policy_kernels import (MCTS_MAX_CAP, MCTS_MAX_FOREST_BYTES, MCTS_MAX_LEAVES, AzPack, BasicPolicy, FirstLayer, PolicyOperands, az_pack, beam_advance, beam_merge, beam_seen, beam_select, first_layer,
                             mcts_backup, mcts_backup_many, mcts_decide, mcts_forest, mcts_rebase, mcts_select, mcts_select_many, mid_head_logp, mid_head_sample, run_first_layer, sample_actions)
from .vec import VecEnv


def policy_from_reference_state_dict(sd: Dict[str, "np.ndarray | torch.Tensor"]) -> BasicPolicy:
    """A `BasicPolicy` holding a reference checkpoint (`examples/models/*.pt`: embeddings / common.0 / action.0 /
    value.0, weight + bias; keys with '.' or '_' separators)."""
    t = {k.replace(".", "_"): torch.as_tensor(np.asarray(v, dtype=np.float32) if not isinstance(v, torch.Tensor) else v).float() for k, v in sd.items()}
    hidden, obs_size = t["embeddings_weight"].shape
    pol = BasicPolicy(obs_size, t["action_0_weight"].shape[0], embedding_size=hidden, common=t["common_0_weight"].shape[0])
    with torch.no_grad():
        for mod, key in ((pol.embeddings, "embeddings"), (pol.common, "common_0"), (pol.policy_head, "action_0"), (pol.value_head, "value_0")):
            mod.weight.copy_(t[key + "_weight"])
            mod.bias.copy_(t[key + "_bias"])
    return pol


class _Packed(PolicyOperands):
    """The policy-layer kernels' operands (`bias`, `mid`, `head`: packed once, shared by every handle and by the views): a snapshot of the
    policy's weights at `at`, the parameters' version counters, never repacked.  An in-place update of the policy drops all of it, the
    per-handle first layers (`_Handles.first`) included, so the kernels never run one layer of the new weights with another of the old,
    and follow the policy as the torch forward does.  ValueError where the packers refuse the middle layer or the head."""

    def __init__(self, policy: BasicPolicy, at: tuple):
        super().__init__(policy)
        if self.mid is None:
            raise ValueError(self.why)
        self.at = at
        self.views: Optional[FirstLayer] = None  # twist_kernels: the first layer for the views' words (no handle in it: packed once)


@dataclass
class _Handles:
    """The handles of one kind, all of one batch shape (`key`), and per handle the first layer packed through it (`pack_embedding` goes
    through the handle that will read it), in the route the handle takes: closed and dropped together."""
    key: tuple
    vecs: Tuple[VecEnv, ...]
    first: Dict[VecEnv, FirstLayer] = field(default_factory=dict)
    log: Optional["_SelfPlayLog"] = None  # the self-play kinds: the decision log and the packed samples, reused from call to call


SELF_PLAY_MAX_LOG_BYTES = 1 << 30  # what `self_play` allocates at most for its log and samples: 1 GiB


class _SelfPlayLog:
    """The recorder of `_TreeSearch` for `self_play`: per decision t and episode e the root's visit counts, the live flag, the packed
    observation before the move, the real step's reward and the move, all on the device, and the `az_pack` outputs they are packed into.
    `reset` (states=None): (difficulty, seed) for the real envs' own reset instead of loaded targets."""

    def __init__(self, T: int, E: int, A: int, real: VecEnv, capacity: int):
        dev, i32, f32 = real.device, torch.int32, torch.float32
        self.shape = (T, E, A, capacity)
        self.counts = torch.zeros((T, E, A), dtype=i32, device=dev)
        self.live = torch.zeros((T, E), dtype=torch.bool, device=dev)
        self.reward = torch.zeros((T, E), dtype=f32, device=dev)
        self.move = torch.zeros((T, E), dtype=i32, device=dev)
        self.words = torch.zeros((T, E, real.packed_words_per_env), dtype={1: torch.uint8, 4: i32, 8: torch.int64}[real.packed_word_bytes], device=dev)
        self.out: Optional[AzPack] = None
        self.reset: Optional[Tuple[int, int]] = None

    @staticmethod
    def nbytes(T: int, E: int, A: int, W: int, word_bytes: int, capacity: int) -> int:
        return T * E * (4 * A + 9 + W * word_bytes + 8) + T * E // 32 + 8 + capacity * (4 * A + 12 + W * word_bytes)

    def before(self, t: int, real: VecEnv, finished: torch.Tensor):
        real.observe_packed(out=self.words[t])
        torch.eq(finished, 0, out=self.live[t])

    def after(self, t: int, real: VecEnv, move: torch.Tensor):
        self.reward[t].copy_(real.reward)
        self.move[t].copy_(move)

    def pack(self, steps: int) -> AzPack:
        """One `az_pack` over the `steps` >= 1 decisions made, into the first rows of the outputs (made for `capacity` samples; a log of
        `steps` decisions holds at most steps * E)."""
        T, E, A, capacity = self.shape
        if self.out is None:
            dev, i32, f32 = self.counts.device, torch.int32, torch.float32
            self.out = AzPack(torch.zeros(3, dtype=i32, device=dev), torch.zeros(capacity, dtype=i32, device=dev), torch.zeros(capacity, dtype=f32, device=dev),
                              torch.zeros(capacity, dtype=i32, device=dev), torch.zeros((capacity, A), dtype=f32, device=dev),
                              torch.zeros((capacity, self.words.shape[2]), dtype=self.words.dtype, device=dev),
                              torch.empty(int(_lib.load().qg_az_pack_scratch_bytes(T, E)), dtype=torch.uint8, device=dev))
        o, cap = self.out, min(capacity, steps * E)
        return az_pack(self.counts[:steps], self.reward[:steps], self.live[:steps], self.move[:steps], self.words[:steps], capacity=cap,
                       out=AzPack(o.n, o.index[:cap], o.z[:cap], o.move[:cap], o.pi[:cap], o.words[:cap], o.scratch))


def _winner(solved: torch.Tensor, ret: torch.Tensor):
    """Per row of `solved` / `ret` [N, K]: the scores (the return where solved, else -inf) and the index of the best; argmax takes the first
    of equal maxima: the lowest index."""
    score = torch.where(solved, ret, torch.full(ret.shape, -float("inf"), device=ret.device))
    return score, score.argmax(dim=1)


@dataclass(frozen=True)
class _MctsOptions:
    """A tree search as `_check_mcts` resolved it: `N` simulations per decision under `C`; `S` searches per target, their moves drawn (None: one tree,
    the most visited action); `cap` nodes per tree, carried between decisions (None: N + 1, no reuse); `K` leaves per tree and round under
    `virtual_loss`.  The one place that knows the default capacity, the handle kinds' names and their batch shapes."""
    N: int
    C: float
    S: Optional[int]
    cap: Optional[int]
    K: int
    virtual_loss: float

    @staticmethod
    def default_cap(N: int) -> int:  # `reuse_tree` without `mcts_nodes`
        return min(2 * N + 1, MCTS_MAX_CAP)

    @property
    def nodes(self) -> int:  # the nodes a tree has room for
        return self.N + 1 if self.cap is None else self.cap

    def rounds(self) -> List[int]:  # the descents k_r of a decision's R = ceil(N / K) rounds: K, in the last what is left of N
        return [min(self.K, self.N - r * self.K) for r in range(-(-self.N // self.K))]

    def kind(self, prefix: Optional[str] = None) -> str:
        """`prefix` ("self-play"; None: "mcts" / "mcts-sampled"), "-reuse" with a second pool, "-many" with K leaf envs per tree."""
        base = prefix if prefix is not None else "mcts" if self.S is None else "mcts-sampled"
        return base + ("-reuse" if self.cap is not None else "") + ("-many" if self.K > 1 else "")

    def batches(self, trees: int) -> tuple:
        """The leaf batch (env m * K + i: descent i of tree m), the pool (env m * nodes + j: node j; reuse: two, taking turns), the real envs."""
        return (trees * self.K, *(trees * self.nodes,) * (1 if self.cap is None else 2), trees)


# what a tree search leaves: the answers, `last_stats`, the decisions made; `returns` (sampled searches) and `success` per tree; `self_play`'s samples
_MctsResult = namedtuple("_MctsResult", "solutions stats steps returns success packed")


class _TreeSearch:
    """The PUCT tree search of `solve(num_mcts_searches=N)` and `self_play` on the handles of `held`: the leaf batch, which is all the forward
    object reads, the pool(s) of node envs and the real envs.  Rules: include/qgym.h, restated in tests/mcts*model.py; tree m * S + s is search s
    of target m.  A decision makes R rounds of k_r descents (`_MctsOptions.rounds`): N of one on `mcts_select` / `mcts_backup` (K = 1), or
    ceil(N / K) on the `_many` pair, virtual visits between a round's descents; the pair is chosen here, once, and looked up in this module at
    every call.  `leaves` [R, M, K], every round's leaf outputs, is read by the count of descents that did not count: kept under reuse and
    K >= 2 only (the N + 1 nodes of a plain search of one leaf cannot fill)."""

    def __init__(self, opts: _MctsOptions, held: _Handles, seed: int, rec: Optional[_SelfPlayLog] = None):
        self.opts, self.seed, self.rec = opts, seed, rec
        self.leaf, self.pool, *other, self.real = held.vecs
        self.other = other[0] if other else None  # reuse: the pool the kept nodes' envs move into
        real, K, per_round = self.real, opts.K, opts.rounds()
        M, dev, i32, i64 = real.batch, real.device, torch.int32, torch.int64  # M: trees
        self.T = T = int(real._cfg.max_depth)
        self.forest = mcts_forest(M, opts.N, real.num_actions(), dev, cap=opts.cap)
        self.ids, self.per_round = torch.arange(M, dtype=i32, device=dev), per_round
        self.roots = self.ids * opts.nodes
        self.slots = self.ids if K == 1 else torch.arange(M * K, dtype=i32, device=dev)  # the leaf batch's envs: what a round copies back
        self.picked = tuple(torch.empty(M * K, dtype=i32, device=dev) for _ in range(4))  # src, dst, act, leaf of a round
        self.drawn = torch.empty(M, dtype=i32, device=dev)
        self.ret = None if opts.S is None else torch.zeros(M, dtype=torch.float32, device=dev)  # a sampled search's return per tree
        if K == 1:  # called alike, the search handed in: kept here, a closure over `self` is a cycle that holds the forest; one descent ignores k
            self.select = lambda s, k, out: mcts_select(s.forest, opts.C, s.finished, *out)
            self.backup = lambda s, k, rows, values, picked: mcts_backup(s.forest, rows, values, s.leaf.reward, s.leaf.done, *picked)
        else:
            self.select = lambda s, k, out: mcts_select_many(s.forest, opts.C, K, k, opts.virtual_loss, s.finished, *out)
            self.backup = lambda s, k, rows, values, picked: mcts_backup_many(s.forest, K, rows, values, s.leaf.reward, s.leaf.done, *picked, k=k)
        self.leaves = torch.empty((len(per_round), M, K), dtype=i32, device=dev) if self.other is not None or K > 1 else None  # for the stats
        self.made = (torch.arange(K, device=dev)[None, :] < torch.tensor(per_round, device=dev)[:, None])[:, None, :] if K > 1 else None  # i < k_r
        self.outs = [self.picked if self.leaves is None else (*self.picked[:3], self.leaves[r].view(-1)) for r in range(len(per_round))]  # per round
        if self.other is not None:  # and per decision the live trees and their carried sizes
            self.env_src = torch.empty(M * opts.cap, dtype=i32, device=dev)
            self.sizes, self.lives = torch.zeros((T, M), dtype=i32, device=dev), torch.zeros((T, M), dtype=torch.bool, device=dev)
        self.missed, self.nodes, self.decisions = (torch.zeros((), dtype=i64, device=dev) for _ in range(3))

    def _round(self, r: int, k: int):
        """k descents per tree.  One that is refused or not made names its tree's root, no gate (A) and, as `dst`, no env of the pool."""
        leaf, picked = self.leaf, self.select(self, k, self.outs[r])
        leaf.copy_envs(self.pool, picked[0])  # src
        leaf.step(picked[2])  # act
        rows, values = self.fwd.logp_values(leaf)
        self.pool.copy_envs(leaf, self.slots, picked[1])  # dst
        self.backup(self, k, rows, values, picked)

    def _decide(self, t: int) -> torch.Tensor:
        """Decision t, one launch: the most visited action, or (`S`) one drawn by the visits; `rec` logs the real envs first and keeps the counts."""
        how = {} if self.opts.S is None else dict(sample=True, seed=self.seed, counter=t)
        if self.rec is not None:
            self.rec.before(t, self.real, self.finished)
            how["counts"] = self.rec.counts[t]
        return mcts_decide(self.forest, finished=self.finished, move=self.drawn, **how)

    def _carry(self, t: int, move: torch.Tensor):
        """`reuse_tree`: the move's subtree becomes the tree, the kept nodes' envs move; a tree whose real env just ended is left alone."""
        mcts_rebase(self.forest, move, self.finished, self.env_src)
        self.other.copy_envs(self.pool, self.env_src)  # into the other pool: `copy_envs` allows no index on both sides within one handle
        self.pool, self.other = self.other, self.pool
        torch.eq(self.finished, 0, out=self.lives[t])
        torch.mul(self.forest.n_nodes, self.lives[t], out=self.sizes[t])

    def run(self, fwd: _Forward) -> _MctsResult:  # from the targets the real envs hold now
        leaf, real, M, steps, self.fwd = self.leaf, self.real, self.real.batch, 0, fwd
        self.finished = real.success.bool().to(torch.uint8)  # a target that is already solved needs no gates
        for t in range(self.T):
            if t == 0 or self.other is None:  # a fresh tree per real env, the root its clone (the leaf batch has K envs per tree: the first M)
                leaf.copy_envs(real, self.ids)
                rows, values = self.fwd.logp_values(leaf)
                self.pool.copy_envs(leaf, self.ids, self.roots)
                mcts_backup(self.forest, rows[:M], values[:M], done=self.finished, root=True)
            for r, k in enumerate(self.per_round):
                self._round(r, k)
            live = self.finished == 0
            if self.leaves is not None:  # descents that did not count (leaf < 0: a full tree), over live trees and descents made
                lost = (self.leaves < 0) & live[None, :, None]
                self.missed += (lost if self.made is None else lost & self.made).sum()
            move = self._decide(t)
            self.nodes += (self.forest.n_nodes * live).sum()
            self.decisions += live.sum()
            real.step(move)
            if self.rec is not None:
                self.rec.after(t, real, move)
            if self.ret is not None:  # a search's return: the f32 sum, in step order, of the rewards of the steps it was live for
                self.ret += torch.where(live, real.reward, torch.zeros_like(self.ret))
            self.finished |= real.done.bool().to(torch.uint8)
            if self.other is not None:
                self._carry(t, move)
            steps = t + 1
            if t % 8 == 7 and bool(self.finished.all()):
                break
        return self._answers(steps)

    def _answers(self, steps: int) -> _MctsResult:
        """Per target the real env's own solution log where its episode succeeded; `S`: that of its winning search (`_winner`)."""
        o, real, M, A, S = self.opts, self.real, self.real.batch, self.real.num_actions(), self.opts.S or 1
        packed = None if self.rec is None else self.rec.pack(steps)  # the samples, packed behind the loop on its stream
        real.sync()
        sols, lens = real.solutions(self.T + 64)  # the log holds an episode's steps, PauliEnv: plus one entry per rotation (<= 32)
        success = real.success.bool()
        stats = {"mcts": o.N}
        if o.S is None:
            mine, ok = range(M), success.cpu().numpy()
        else:
            won = success.view(-1, S)
            mine = (torch.arange(M // S, device=real.device) * S + _winner(won, self.ret.view(-1, S))[1]).tolist()
            stats.update(searches=S, searches_solved=int(won.sum()) / M)
            ok = won.any(dim=1).cpu().numpy()
        # a finished env was handed A from then on, which the log of some env kinds records: such entries are no gates and no markers
        out = [[int(x) for x in sols[e, : lens[e]] if x < A or x >= ROTATION_MARKER] if ok[m] else None for m, e in enumerate(mine)]
        gates = [sum(1 for x in s if x < ROTATION_MARKER) for s in out if s is not None]
        stats.update({"targets": M // S, "steps": steps, "solved": int(ok.sum()), "mean_gates": float(np.mean(gates)) if gates else 0.0,
                      "nodes": float(self.nodes) / max(int(self.decisions), 1), "kernels": self.fwd.kernels})
        if self.other is not None:
            stats.update(reuse=True, capacity=o.cap, carried=float(self.sizes.sum()) / max(int(self.lives.sum()), 1), refused=int(self.missed))
        if o.K > 1:
            stats.update(leaves=o.K, rounds=len(self.per_round), idle=int(self.missed))
        return _MctsResult(out, stats, steps, self.ret, success, packed)


class _Forward:
    """What the step loops ask about a handle's current state: `logp(vec)`, the rows of log-probabilities [B, A] f32 (beam search);
    `greedy(vec)`, the arg-max, int32 [B]; `draw(vec, t)`, the draw of step t from `seed`, int32 [B]; `logp_values(vec)`, the rows and the
    value head, f32 [B] (the tree search: priors and leaf values).  Under twists (`tw` int32 [B]: env e
    is seen through twist tw[e]) the answers are about the view, and `real_actions` maps a choice back.  `kernels` is for `last_stats`."""

    def __init__(self, seed: int, tw: Optional[torch.Tensor]):
        self.seed, self.tw = seed, tw

    def real_actions(self, vec: VecEnv, act: torch.Tensor) -> torch.Tensor:
        """`act` was chosen on the view: the real action, in place."""
        return act if self.tw is None else vec.untwist_actions(act, self.tw, out=act)


class _TorchForward(_Forward):
    """The answers of the policy module in `dtype`."""
    kernels = False

    def __init__(self, policy: torch.nn.Module, dtype: torch.dtype, seed: int, tw: Optional[torch.Tensor]):
        super().__init__(seed, tw)
        self.policy, self.dtype = policy, dtype

    def _outputs(self, vec: VecEnv):
        """The policy's two outputs on what it reads, in its dtype: the observation, or the view.  A dtype the library does not write
        (float64) is written as float32 and widened: the entries are 0 and 1."""
        dt = self.dtype if self.dtype in VecEnv._DTYPES else torch.float32
        x = vec.observe_as(dt) if self.tw is None else vec.observe_twisted(self.tw, dt)
        return self.policy(x if dt == self.dtype else x.to(self.dtype))

    def _logits(self, vec: VecEnv) -> torch.Tensor:
        return self._outputs(vec)[0]

    def logp(self, vec: VecEnv) -> torch.Tensor:
        return torch.log_softmax(self._logits(vec).float(), dim=1)

    def logp_values(self, vec: VecEnv) -> Tuple[torch.Tensor, torch.Tensor]:
        logits, value = self._outputs(vec)
        return torch.log_softmax(logits.float(), dim=1), value.float().reshape(-1).contiguous()

    def greedy(self, vec: VecEnv) -> torch.Tensor:
        return self._logits(vec).argmax(dim=1).to(torch.int32)

    def draw(self, vec: VecEnv, t: int) -> torch.Tensor:
        return sample_actions(self._logits(vec).contiguous(), self.seed, t)[0].to(torch.int32)


class _KernelForward(_Forward):
    """The answers of the policy-layer kernels (bf16 products, f32 accumulation): the first layer from the bits (`first`: per handle
    its packed first layer and route), then middle layer + head + log-softmax or draw in one kernel, no logits in memory.  The buffers are
    allocated here, once per search; `greedy` and `draw` return the same buffer every step."""
    kernels = True

    def __init__(self, packed: _Packed, first: Dict[VecEnv, FirstLayer], policy: BasicPolicy, seed: int, tw: Optional[torch.Tensor], rows: bool):
        super().__init__(seed, tw)
        self.packed, self.first = packed, first
        vec = next(iter(first))  # the handles of a search are alike
        B, dev = vec.batch, vec.device
        self.hidden, self.common, self.A = policy.embeddings.out_features, policy.common.out_features, vec.num_actions()
        self.h1 = torch.empty((B, self.hidden), dtype=torch.bfloat16, device=dev)
        # 16-byte row stride: 16-byte stores
        self.rows = torch.empty((B, (self.A + 3) // 4 * 4), dtype=torch.float32, device=dev)[:, : self.A] if rows else None
        self.act = torch.empty(B, dtype=torch.int32, device=dev)
        self.scratch = torch.empty((3, B), dtype=torch.float32, device=dev)  # the kernels' other outputs: not used by the searches
        # where the two words routes keep the packed observation; the views' row count is the env's rounded up to even
        words = {"state": 0, "words": vec.packed_words_per_env, "views": vec.obs_shape_[0] + vec.obs_shape_[0] % 2}[first[vec].route]
        self.words = torch.empty((B, words), dtype=torch.int64, device=dev) if words else None

    def _first_layer(self, vec: VecEnv) -> torch.Tensor:
        """relu(obs W1^T + b1) of the handle's current state into `h1` (bf16)."""
        return run_first_layer(self.first[vec], vec, self.packed.bias, self.hidden, out=self.h1, words=self.words, tw=self.tw)

    def logp(self, vec: VecEnv) -> torch.Tensor:
        p, s = self.packed, self.scratch
        return mid_head_logp(self._first_layer(vec), p.mid, self.common, p.head, self.A, logp_rows=self.rows, actions=self.act, best_logp=s[0],
                             entropy=s[1], values=s[2])[0]

    def logp_values(self, vec: VecEnv) -> Tuple[torch.Tensor, torch.Tensor]:
        return self.logp(vec), self.scratch[2]  # `mid_head_logp` writes both

    def greedy(self, vec: VecEnv) -> torch.Tensor:
        p, s = self.packed, self.scratch
        mid_head_logp(self._first_layer(vec), p.mid, self.common, p.head, self.A, want_rows=False, actions=self.act, best_logp=s[0], entropy=s[1],
                      values=s[2])  # the arg-max alone: no row is written
        return self.act

    def draw(self, vec: VecEnv, t: int) -> torch.Tensor:
        p, s = self.packed, self.scratch
        mid_head_sample(self._first_layer(vec), p.mid, self.common, p.head, self.A, self.seed, t, actions=self.act, logp=s[0], entropy=s[1],
                        values=s[2])
        return self.act


class BatchedSynthesis:
    """`env`: one of the *Gym front ends (its configuration and gateset are used); `policy`: a module mapping the flat
    observation [B, rows*cols] to (logits [B, num_actions], value [B])."""

    def __init__(self, env, policy: torch.nn.Module, dtype: torch.dtype = torch.float32, seed: int = 0, device=None):
        self.env = env
        self.dtype = dtype
        self.seed = int(seed)
        self.device = device
        self._policy = policy
        self._held: Dict[str, _Handles] = {}  # by kind, see `_handles`
        self._view_list = None  # twists: the twist index behind each view (`_views`)
        self._packed: Optional[_Packed] = None
        self.last_stats: dict = {}

    _NO_KERNELS = "fast=True needs a BasicPolicy of the default shape and an env whose state or packed observation the first-layer kernels read"

    _NO_TWIST_KERNELS = "twist_kernels=True needs a BasicPolicy of the default shape and an env with twists whose observation has at most 64 columns"

    @property
    def _beam(self) -> Optional[_Handles]:
        """The beam search's handles (two search batches that take turns, and the winners); None until a beam search has run."""
        return self._held.get("beam")

    def _handles(self, kind: str, batches: Sequence[int], perms: bool = False) -> _Handles:
        """The handles of `kind`, one per entry of `batches`: "search" (the sampled and greedy searches' batch), "replay" (the winners of a
        PauliGym search, replayed with the solution log on) or "beam" (the two batches of targets * width envs that take turns as source and
        destination of the per-step copy, and the winners, all three with the same constructor arguments: the rule of `copy_envs`; no layout
        choice depends on the batch size) or a tree search's kind (`_MctsOptions.kind` and `.batches`: the leaf batch, the pool or pools of
        node envs and the real batch, again all with the same constructor arguments).  One batch shape at a time per kind: the handles own
        device memory."""
        key = (*batches, perms)  # add_perms: twists() only, the env steps alike
        held = self._held.get(kind)
        if held is not None and held.key != key:
            del self._held[kind]
            for v in held.vecs:
                v.close()
            held = None
        if held is None:
            held = self._held[kind] = _Handles(key, tuple(self.env.vec(b, device=self.device, add_inverts=False, add_perms=perms,
                                                                       track_solution=kind != "search") for b in batches))
            self._policy = self._policy.to(device=held.vecs[0].device, dtype=self.dtype)
        return held

    def _snapshot(self) -> _Packed:
        """The packed operands of the weights as they are now: after an in-place update everything packed before is dropped first."""
        pol = self._policy
        at = tuple((id(p), p._version) for p in pol.parameters())
        if self._packed is None or self._packed.at != at:
            self._packed = None
            for held in self._held.values():
                held.first.clear()
            self._packed = _Packed(pol, at)
        return self._packed

    def _first_layer(self, vec: VecEnv, kept: Dict[VecEnv, FirstLayer], views: bool) -> FirstLayer:
        """The first layer of the policy-layer kernels (qg_vec_embed / qg_policy_embed_words in front of qg_policy_mid_head_sample / _logp) for
        `vec`, packed on first use (`policy_kernels.first_layer` chooses the route): through the handle and kept in `kept`, its owner's
        `_Handles.first`; or, `views`, for `embed_words` on `observe_twisted_words`, kept with the snapshot.
        ValueError where the kernels do not apply: another policy class or shape, no TILE layout nor 64-bit row words, a view too wide."""
        pol = self._policy
        if not isinstance(pol, BasicPolicy):
            raise ValueError(self._NO_TWIST_KERNELS if views else self._NO_KERNELS)
        # as the two builders this one replaces: a weight dtype the packers do not take (KeyError) is an error of its own on the handle routes
        caught = (ValueError, KeyError, _lib.QGymError) if views else (ValueError, _lib.QGymError)
        try:
            packed = self._snapshot()
            if views:
                if packed.views is None:
                    packed.views = first_layer(vec, pol.embeddings.weight, ("views",))
                return packed.views
            if vec not in kept:
                kept[vec] = first_layer(vec, pol.embeddings.weight)
            return kept[vec]
        except caught as e:
            raise ValueError(f"{self._NO_TWIST_KERNELS} ({e})" if views else self._NO_KERNELS) from None

    def _forward(self, held: _Handles, readers: int, tw: Optional[torch.Tensor], kernels: Optional[bool], rows: bool = False) -> _Forward:
        """The forward object of one search on the first `readers` handles of `held`, under the views `tw` if any.  `kernels` True: the
        policy-layer kernels, or ValueError where they do not apply; None: the kernels where they apply, else torch; False: torch.
        `rows`: the search asks for `logp`."""
        if kernels is not False:
            try:
                first = {v: self._first_layer(v, held.first, tw is not None) for v in held.vecs[:readers]}
            except ValueError:
                if kernels:
                    raise
            else:
                return _KernelForward(self._snapshot(), first, self._policy, self.seed, tw, rows)
        return _TorchForward(self._policy, self.dtype, self.seed, tw)

    def _load(self, vec: VecEnv, states: Sequence[Sequence[int]], repeat: int):
        if vec.env_kind == "pauli":
            n = vec.num_qubits
            tabs, labels = [], []
            for s in states:  # the set_state wire format (envs/synthesis.py:451-461): [rot_count, tableau..., len, chars, ...]
                s = list(s)
                tabs.append(np.asarray(s[1 : 1 + 4 * n * n], dtype=np.uint8))
                pos, rots = 1 + 4 * n * n, []
                for _ in range(int(s[0])):
                    ln = int(s[pos])
                    rots.append("".join(chr(c) for c in s[pos + 1 : pos + 1 + ln]))
                    pos += 1 + ln
                labels.append(rots)
            vec.pauli_reset_from(np.repeat(np.stack(tabs), repeat, axis=0), [l for l in labels for _ in range(repeat)])
        else:
            vec.set_state(np.repeat(np.asarray(states, dtype=np.int64), repeat, axis=0), fmt="i64")

    def _views(self, V: int) -> List[int]:
        """Twist index of each of a target's views: view 0 is the untwisted one (-1: no such twist, `observe_twisted` and `untwist_actions`
        pass through), then the env's non-identity twists -- those that move an observation entry -- in `twists()` order; at most V of them."""
        if self._view_list is None:
            probe = self.env.vec(1, device=self.device, add_inverts=False, add_perms=True, track_solution=False)
            obs_perms = probe.twists()[0]
            probe.close()
            self._view_list = [-1] + [t for t, p in enumerate(obs_perms) if p != list(range(len(p)))]
        return self._view_list[:V]

    def _twist_index(self, views: List[int], groups: int, M: int, width: Optional[int], dev) -> torch.Tensor:
        """Every env's twist index, int32 [B]: per target `groups` consecutive groups, group g under view g mod V.  Sampled and greedy
        searches: a group is one search (`width` None), env m * S + s sees view s mod V.  Beam search: V groups of `width` beams, env b is in
        group b // W under view (b // W) % V."""
        tw = torch.tensor([views[g % len(views)] for g in range(groups)], dtype=torch.int32, device=dev).repeat(M)
        return (tw if width is None else tw.repeat_interleave(width)).contiguous()

    def _beam_search(self, states, held: _Handles, views: Optional[List[int]], W: int, kernels: bool, merge: bool, bound: Optional[str]):
        """The search of `solve(beam_width=W)` on the handles of `held`: `cur` and `oth` take turns, the forward object (`kernels`: the policy-layer
        kernels or a ValueError, else torch) reads whichever is current.  `views` None: one group per target.  Else the groups are the (target,
        view) pairs, V consecutive ones per target, each under its own fixed view (and with its own merge history); a target's winner is the best
        of its V groups, ties to the lowest view.  Returns, winners and `live`: one `beam_advance` per step in mode `bound` (in place on them)."""
        cur, oth, win = held.vecs
        targets, V = len(states), 1 if views is None else len(views)
        M = targets * V  # groups
        B, A, dev = cur.batch, cur.num_actions(), cur.device
        T = int(cur._cfg.max_depth)
        tw = None if views is None else self._twist_index(views, V, targets, W, dev)
        if bound is not None:  # the handle's config: the caller's metrics weights over the reference's defaults
            low = {k: float(getattr(cur._cfg, "w_" + k)) for k in ("n_cnots", "n_layers_cnots", "n_layers", "n_gates")}
            low = {k: w for k, w in low.items() if not w >= 0.0}
            if low:
                raise ValueError(f"bound needs rewards that cannot exceed 1: every metrics weight must be >= 0, got {low}")
        fwd = self._forward(held, 2, tw, kernels, rows=True)
        self._load(win, states, V)  # the targets once per group; a group nobody solves keeps its slot, a solved one is overwritten by its winner
        cur.copy_envs(win, torch.arange(M, dtype=torch.int32, device=dev).repeat_interleave(W))
        found = win.success.bool().to(torch.uint8)  # a target that is already solved needs no gates: its winner is the target itself
        best = torch.where(found.bool(), 0.0, -float("inf")).to(torch.float32)
        live = torch.zeros((M, W), dtype=torch.uint8, device=dev)
        live[:, 0] = 1 - found
        live = live.view(B)
        cum = torch.zeros(B, dtype=torch.float32, device=dev)
        ret, spare = torch.zeros(B, dtype=torch.float32, device=dev), torch.empty(B, dtype=torch.float32, device=dev)  # the returns alternate between two buffers
        win_src, group_live = torch.empty(M, dtype=torch.int32, device=dev), torch.empty(M, dtype=torch.uint8, device=dev)
        bounded = None if bound is None else torch.zeros(M, dtype=torch.int32, device=dev)
        steps = 0
        if merge:  # the targets' own keys open the histories (one live slot per unsolved target: nothing to drop), so coming back to a target is a revisit
            cap = T * W + 1  # a step adds at most W keys per target: the history of a search never fills
            seen, dropped = beam_seen(M, cap, dev), torch.zeros((M, 2), dtype=torch.int32, device=dev)
            words = cur.observe_packed()
            live = beam_merge(words, cum, live, W, seen, cap)
        for t in range(T):
            parent, act, cum, live = beam_select(fwd.logp(cur), cum, live, W, A)
            fwd.real_actions(cur, act)  # a child lives in its parent's group, hence under its view
            oth.copy_envs(cur, parent)
            oth.step(act)
            # The return `solve` ranks by is the parent's plus this step's reward.  A slot that is not live gets 0 instead: it is never a parent
            # (`beam_select` gives a dead slot its own index and live = 0) and never solved (live & success), so nothing reads it.  The bound, if
            # any: no reward after this step exceeds 1.0 in total (the weights are checked above); mode None reads neither bonus nor `bounded`.
            beam_advance(parent, ret, oth.reward, oth.success, oth.done, live, best, found, W, skip=B, bonus=1.0, mode=bound, ret_out=spare,
                         win_src=win_src, group_live=group_live, bounded=bounded)
            ret, spare = spare, ret
            win.copy_envs(oth, win_src)  # B, out of range and skipped, where the winner stays
            if merge:  # beams that ended (the step's results among them) have left `live`: they are neither merged nor recorded
                live = beam_merge(oth.observe_packed(out=words), cum, live, W, seen, cap, dropped=dropped)
            cur, oth = oth, cur
            steps = t + 1
            if t % 8 == 7 and not bool(live.any()):
                break
        for v in (cur, oth, win):
            v.sync()
        sols, lens = win.solutions(T + 64)  # the log holds an episode's steps, PauliEnv: plus one entry per rotation (<= 32)
        ok = found.bool().cpu().numpy()
        if tw is not None:  # per target the best of its V groups, the lowest view among equals
            pick = (torch.arange(targets, device=dev) * V + _winner(found.bool().view(targets, V), best.view(targets, V))[1]).cpu().numpy()
            ok, sols, lens = ok[pick], sols[pick], lens[pick]
        out = [[int(x) for x in sols[m, : lens[m]]] if ok[m] else None for m in range(targets)]
        gates = [sum(1 for x in s if x < ROTATION_MARKER) for s in out if s is not None]
        self.last_stats = {"beam_width": W, "targets": targets, "steps": steps, "solved": int(ok.sum()), "mean_gates": float(np.mean(gates)) if gates else 0.0}
        if fwd.kernels:
            self.last_stats["kernels"] = True
        if tw is not None:
            self.last_stats["views"] = V
        if merge:
            n_rev, n_dup = (int(x) for x in dropped.sum(dim=0).cpu())
            self.last_stats.update(merged=n_dup, revisits=n_rev)
        if bound is not None:
            self.last_stats.update(bound=bound, bounded=int(bounded.sum()))
        return out

    def _tree_search(self, states, held: _Handles, opts: _MctsOptions, kernels: bool, rec: Optional[_SelfPlayLog] = None) -> _MctsResult:
        """`_TreeSearch` from `states`, every target `S` times, or (`rec.reset`) from the real envs' own reset on the device; sets `last_stats`."""
        search, real = _TreeSearch(opts, held, self.seed, rec), held.vecs[-1]  # the forest and the buffers first
        fwd = self._forward(held, 1, None, kernels, rows=True)
        if rec is not None and rec.reset is not None:
            real.difficulty = rec.reset[0]
            real.reset(rec.reset[1])
        else:
            self._load(real, states, 1 if opts.S is None else opts.S)
        res = search.run(fwd)
        self.last_stats = res.stats
        return res

    @torch.no_grad()
    def solve(self, states: Sequence[Sequence[int]], deterministic: bool = False, num_searches: int = 100, fast: Optional[bool] = None,
              beam_width: Optional[int] = None, merge_duplicates: bool = False, twists: Optional[int] = None,
              twist_kernels: bool = False, bound: Optional[str] = None, num_mcts_searches: int = 0, C: float = 2 ** 0.5,
              max_expand_depth: int = 1, mcts_sampled: bool = False, reuse_tree: bool = False,
              mcts_nodes: Optional[int] = None, mcts_leaves: int = 1, virtual_loss: float = 0.0) -> List[Optional[List[int]]]:
        """One entry per target: `Env::solution()` of the best successful search, or None (rl/synthesis.py:121-126).
        The rules of the sampled and the greedy search -- env m * S + s is search s of target m, the draw of step t is the race of
        `sample_actions(logits, seed, t)`, a finished env gets no gate and adds no reward, the loop ends at the first step t with
        t % 8 == 7 and every env finished, the winner is the successful search of the greatest f32 return, the lowest s among equals --
        are stated in tests/searchmodel.py, which tests/test_gpu_sampled_search.py holds every draw and every answer against.
        fast: run the forward pass on the policy-layer kernels (bf16 products, f32 accumulation; `last_stats["kernels"]` says whether they
        ran).  Sampled searches: forward pass and draw (default, fast=None: when the kernels apply and the batch has at least 4 096 envs).
        deterministic=True and beam_width: only on fast=True (None and False: the torch forward in `dtype`) -- the greedy step takes the
        arg-max of `collector.mid_head_logp`, the beam search its rows of log-probabilities in place of `log_softmax(logits)`.  fast=True
        where the kernels do not apply (another policy class or shape, an env without TILE layout or 64-bit observation words) is a
        ValueError.  Solutions are valid either way -- the env decides what solves a target, the policy only proposes -- but bf16 products
        may rank two nearly equal actions the other way round than f32 torch, so the greedy and beam results of the two paths can differ.

        beam_width=W >= 1: beam search over the policy's log-probabilities instead (`deterministic` and `num_searches` are then
        ignored; no randomness).  Every target keeps up to W partial gate sequences ("beams"), at first the empty one.  Per step every beam is
        scored `cum + log_softmax(logits)[a]` for each action a (f32), the W best continuations of a target survive (`collector.beam_select`:
        ties by slot, then action), each as a copy of its parent env (`VecEnv.copy_envs`) stepped with its action.  A beam that ends
        (`is_final`) leaves the search; if it ended with `success` it is a result, valued by its return like the sampled searches, and the
        first result of the highest return seen so far (lowest slot among equals in one step) is the target's winner.  The search ends when
        no beam is left or after max_depth steps.  The winner's own solution log is returned, so a PauliGym solution carries its rotation
        markers without a replay.  Known limit: beams that reach the same state through commuting gates are not merged; they occupy a slot each.

        merge_duplicates=True (with beam_width) lifts that limit for the envs whose observation is their state (not PauliGym: ValueError).
        After every step, among a target's beams that are still running, those whose state the target has held before -- the target
        itself, or a survivor of an earlier step -- leave the search, and of those that share a state the one with the best score stays
        (`collector.beam_merge` on the packed observation, one history of state keys per target).  Such a state was reached before with
        at least as much depth left, so nothing is lost but slots are freed for distinct states; which targets are solved, and with how
        many gates, may still change either way, since other beams survive.  `last_stats` then also counts the beams dropped: "merged"
        (same state within a step) and "revisits".

        bound="stop" or "prune" (with beam_width; default None: the search exactly as above) uses what the rewards of CliffordGym,
        LinearFunctionGym and PermutationGym have in common: a step earns 1.0 when it reaches the target, minus penalties that are never
        negative while no metrics weight is, so a running beam with return r can end with at most r + 1.0 (in f32, as the search adds).  A
        target's winner changes only for a strictly greater return, so a beam with r + 1.0 <= the winner's return is hopeless, and so is
        everything that descends from it.  "stop": once every running beam of a target (under twists: of a (target, view) group) is
        hopeless they all leave; this returns exactly what bound=None returns, in fewer steps where every target has found its winner early
        -- the loop still ends only when no beam is left anywhere, looked at every 8th step, so a target nobody solves keeps it running to
        max_depth.  "prune": every hopeless beam leaves on its own and its slot goes to other continuations of the target; like
        merge_duplicates this may change which targets are solved and with how many gates, either way.  Every beam search, bounded or not, does the
        step's bookkeeping (returns, winners, `live`) in one kernel, `collector.beam_advance`; either mode combines with fast, twists,
        twist_kernels and merge_duplicates.  `last_stats` gains "bound" (the mode) and "bounded" (beams ended by the bound).  ValueError:
        without beam_width, an unknown mode, a metrics weight below 0 (the bound needs rewards that cannot exceed 1), or PauliGym -- its step
        adds pauli_layer_reward per released rotation (pauli.rs:634) and a target may hold rotations beyond the observed columns, so the
        reward still to come has no bound the search can see: the reason merge_duplicates refuses it.

        twists=V >= 1: V symmetry views per target (None: none of this; every code path, handle and `last_stats` as without the argument).
        View 0 is the untwisted observation, views 1 .. V-1 the env's non-identity twists in `VecEnv.twists()` order; V is cut to what the
        coupling map has and `last_stats["views"]` says how many were used.  The policy reads `VecEnv.observe_twisted`, its choice goes
        through `VecEnv.untwist_actions` before `step`: solutions hold real actions.  The search handles are built with `add_perms=True`,
        which for these env kinds changes `twists()` only.  Sampled and greedy searches: search s of a target keeps view s mod V for its whole
        episode, and `deterministic=True` runs V episodes per target instead of one (ties between equal returns go to the lowest view).  Beam
        search: the groups are the (target, view) pairs -- V groups of W beams per target, each under its own view and with its own merge
        history -- and a target's winner is the best result over its groups, ties to the lowest view.  View 0 is the search without twists,
        so under the default reward weights `twists=V` never solves fewer targets nor needs more gates than `twists=None` in the two
        deterministic modes.  The policy-layer kernels read the resident state and cannot see a view: the torch forward is used, and
        `fast=True` with `twists` is a ValueError; so is PauliGym, which permutes inside observe / step and has no twists (pauli.rs:675-679).

        twist_kernels=True (with `twists`; default False: everything as above) runs the twisted search on the policy-layer kernels all the
        same, in all three modes: `VecEnv.observe_twisted_words` writes every env's view as packed 64-bit row words, which is the input of
        `collector.embed_words`; then `mid_head_sample` (the `(seed, t)` counters of the `fast` path) or `mid_head_logp` (greedy: the
        arg-max; beam: the rows for `beam_select`), `untwist_actions`, `step`.  The first layer is packed once per weight version for the
        env's rows rounded up to even (an odd row count gets a zero pad word and `cols` zero weight columns), so this also reaches envs
        `fast=True` does not: byte and 32-bit observation words, odd row counts.  Groups, views, tie rules and winners are those of the
        torch path, solutions hold real actions, and `last_stats` carries "kernels": True beside "views"; as for `fast`, bf16 products may
        rank two nearly equal actions the other way round than the torch forward, so results can differ from `twists=V` alone.
        ValueError: without `twists`, together with `fast=True`, on PauliGym, with a policy that is not a `BasicPolicy` of the kernels'
        shape, or an observation of more than 64 columns.

        num_mcts_searches=N >= 1, with deterministic=True (default 0: none of this; every code path, handle and `last_stats` as without
        the argument): a PUCT tree search per target, the reference's `num_mcts_searches`, `C` and `max_expand_depth`
        (rl/synthesis.py:112-124; here keyword arguments behind the others, with the reference's defaults).  Every target gets a tree of
        N + 1 nodes, rebuilt for every decision: the root is a clone of the target's real env with the policy's probabilities as priors and
        its value head as value; each of N simulations descends by the greatest `Q + C * prior * sqrt(visits[node]) / (1 + visits[child])`
        (Q: the child's mean backed-up return, the node's own value for an edge not yet tried; ties to the lowest action;
        `collector.mcts_select`), expands one node -- a clone of its parent's env (`VecEnv.copy_envs`) stepped with the action, asked
        about by one forward pass for all targets -- and adds its value plus the rewards on the way up to every node above it
        (`collector.mcts_backup`).  After N simulations the real env takes the root's most visited action (the lowest among equals; one
        launch, `collector.mcts_decide`, in every mode); a real env that is final gets no more gates and its tree no more simulations; the
        loop ends like the other searches'.  The answer is the real env's solution log where the episode ended in success (PauliGym:
        rotation markers included), else None.  The exact rules, operation by operation, are in include/qgym.h and restated in
        tests/mctsmodel.py.  fast=True runs the forward passes on the policy-layer kernels (`mid_head_logp`: rows and values), None / False
        on the torch forward.  `last_stats`: "mcts" (N), "targets", "steps" (decisions), "solved", "mean_gates", "nodes" (mean nodes per
        tree and decision) and "kernels".  ValueError: N < 0; C <= 0; max_expand_depth != 1 (not built: what twisterl means by it cannot
        be read from the reference); deterministic=False (unless `mcts_sampled`, below); together with beam_width, merge_duplicates, bound,
        twists or twist_kernels; a forest -- targets * (N + 1) * (21 + 8 * num_actions) bytes -- of more than 1 GiB
        (`policy_kernels.MCTS_MAX_FOREST_BYTES`; the pool of targets * (N + 1) envs comes on top); N + 1 > 8 192 or more than 256 actions
        is the library's QGymError.  Every mode, here and below, has handles of a kind of its own (`_MctsOptions.kind`, `.batches`).

        mcts_sampled=True, with num_mcts_searches=N >= 1 and deterministic=False (default False: every code path, handle key and `last_stats`
        as without the argument, the ValueError for a tree search with deterministic=False included -- which is why this mode is opted
        into by a keyword of its own): the reference's default shape of the call, S = max(1, num_searches) independent tree-search
        episodes per target.  Tree and real env m * S + s is search s of target m, the layout of the sampled search; the root and the N
        simulations of a decision are those of the tree search above, on targets * S trees in the same launches.  After them the move of
        decision t is drawn from the root's visit counts on the device (`collector.mcts_decide`): r = mulhi64(rng_draw(seed ^ 0x6D637473,
        tree, t), sum of the counts), the lowest action whose running sum of counts exceeds r -- integers, so the same seed gives the same
        episodes.  A search's return is the f32 sum, in step order, of the rewards of the steps it was live for; a target's answer is the
        solution log of its successful search of the greatest return, the lowest s among equals (None without one; PauliGym: rotation
        markers included, no replay).  The rules are restated in tests/mctssample_model.py.  `last_stats`: "mcts", "searches" (S),
        "targets", "steps", "solved", "searches_solved" (successful searches / all), "mean_gates", "nodes", "kernels".  ValueError: without
        num_mcts_searches >= 1; with deterministic=True; with beam_width, merge_duplicates, bound, twists or twist_kernels; and the tree
        search's own, the forest limit now on targets * S trees.

        reuse_tree=True, with num_mcts_searches=N >= 1, deterministic or `mcts_sampled` (default False: not one launch, handle or
        `last_stats` entry changes): the chosen move's subtree is kept between decisions.  The search handles step deterministically, so
        the child under the move IS the next root, and its priors, values, children and stepped envs are valid search work.  The trees
        have room for cap = `mcts_nodes` nodes, by default min(2 N + 1, 8192).  Decision 0 runs as above; after every decision
        `collector.mcts_rebase` compacts every live tree to that subtree on the device (the new root keeps its visits, 1 + the simulations
        below it) and the kept nodes' envs move into a second pool; decisions t >= 1 make their N simulations on the carried tree, without
        the copy of the real envs, the root's forward pass and the root backup.  A tree that is full makes no further nodes: a simulation
        that wants to expand does not count (`collector.mcts_select`: leaf = -1).  The rules are in include/qgym.h and restated in
        tests/mctsreuse_model.py.  `last_stats` gains "reuse" (True), "capacity" (cap), "carried" (mean nodes right after the rebase, over
        live trees and decisions t >= 1) and "refused" ((live tree, simulation) pairs that did not count); "nodes" is the mean size at
        the decision, carried nodes included.  The handles: the leaf batch, two pools of trees * cap envs, the real batch.  ValueError:
        reuse_tree without num_mcts_searches >= 1; mcts_nodes without reuse_tree; mcts_nodes outside [N + 1, 8192]; the forest limit counts
        cap nodes per tree.

        mcts_leaves=K >= 2, with num_mcts_searches=N >= K (default 1: not one launch, handle or `last_stats` entry changes): K leaves per
        tree and round of launches.  A decision makes R = ceil(N / K) rounds instead of N simulations; round r makes k_r = min(K, N - r K)
        descents per tree in ONE selection launch (`collector.mcts_select_many`), one after another on the tree's statistics: each descent
        leaves a virtual visit on every node of its path and takes `virtual_loss` (default 0.0) from the wsum of every node but the root,
        for the rest of the launch only, so the next descent goes elsewhere; an edge already chosen in the round is no candidate.  The
        k_r leaves are cloned, stepped and evaluated in one forward pass on a leaf batch of trees * K envs (env m * K + i is descent i of
        tree m) and linked and backed up in one launch (`collector.mcts_backup_many`).  A decision spends at most N simulations, so
        cap = N + 1 still holds them.  It combines with fast=True, `mcts_sampled` and `reuse_tree`: the decision and the rebase do not care
        how the tree was grown.  The rules are in include/qgym.h and restated in tests/mctsmany_model.py.  `last_stats` gains "leaves" (K),
        "rounds" (R) and "idle" ((live tree, descent) pairs that did not count: leaf < 0, a full tree; with `reuse_tree` "refused" is the
        same number).  ValueError: mcts_leaves < 1 or > 64; mcts_leaves > 1 without num_mcts_searches >= 1; mcts_leaves >
        num_mcts_searches; virtual_loss negative or not finite; virtual_loss != 0 with mcts_leaves = 1."""
        M = len(states)
        S = max(1, int(num_searches)) if mcts_sampled else 1
        self._check_options(M == 0, fast, beam_width, merge_duplicates, twists, twist_kernels, bound)
        opts = self._check_mcts(M * S, num_mcts_searches, C, max_expand_depth, deterministic, S if mcts_sampled else None, reuse_tree, mcts_nodes,
                                mcts_leaves, virtual_loss, dict(beam_width=beam_width is not None, merge_duplicates=merge_duplicates,
                                                                bound=bound is not None, twists=twists is not None, twist_kernels=twist_kernels))
        if M == 0:
            return []
        if opts is not None:
            held = self._handles(opts.kind(), opts.batches(M * S))
            return self._tree_search(states, held, opts, fast is True).solutions  # kernels: on request only
        views = None if twists is None else self._views(int(twists))
        if beam_width is None:
            return self._sampled_search(states, deterministic, num_searches, fast, views, twist_kernels)
        W, groups = int(beam_width), M * (1 if views is None else len(views))
        held = self._handles("beam", (groups * W, groups * W, groups), views is not None)
        return self._beam_search(states, held, views, W, bool(twist_kernels) or fast is True, bool(merge_duplicates), bound)  # kernels: on request only

    @torch.no_grad()
    def self_play(self, states: Optional[Sequence[Sequence[int]]] = None, num_episodes: Optional[int] = None, episodes_per_state: int = 1,
                  difficulty: Optional[int] = None, reset_seed: int = 0, num_mcts_searches: int = 0, C: float = 2 ** 0.5, reuse_tree: bool = False,
                  mcts_nodes: Optional[int] = None, mcts_leaves: int = 1, virtual_loss: float = 0.0, fast: Optional[bool] = None,
                  capacity: Optional[int] = None) -> SelfPlayBatch:
        """Self-play collection for an AlphaZero-style learner (the reference's `AlphaZeroConfig` -> `twisterl.rl.AZ` collects the same):
        E episodes, each a sampled tree search of N = `num_mcts_searches` simulations per decision, every decision logged on the device --
        the packed observation before the move, the root's visit counts, the move drawn from them, the real step's reward -- and the log
        packed by `collector.az_pack` into dense samples (obs, pi, z, action) in (decision, episode) order: one call behind the loop,
        then one host read, the number of samples.  No learner is built: `examples/az_linear_function.py` closes the loop in plain torch.

        states given: exactly the episodes of `solve(states, num_searches=episodes_per_state, num_mcts_searches=N, mcts_sampled=True, ...)`
        under the same seed -- episode m * S + s is search s of target m, the draw of decision t has stream 0x6D637473 and counter t, the
        loop ends by the same rule, every move is the same.  states=None: `num_episodes` real envs get `difficulty` (None: the gym's own)
        and `reset(reset_seed)` on the device; no target crosses the host.  `C`, `reuse_tree`, `mcts_nodes`, `mcts_leaves`, `virtual_loss`
        and `fast` are `solve`'s.  capacity: the samples the batch has room for (None: max_depth * E, every decision); the first
        `capacity` in order are kept and `stats["valid"]` says how many there were.

        A decision gives a sample where its episode was live and its root had a visited child (a row of counts without a visit, or one
        `az_pack` calls bad, gives none: `stats["bad"]` counts the latter; neither occurs in a search that made a simulation).  A target
        that is solved on arrival gives none.  z is the undiscounted return to go, f32 sums from the episode's end (rules: include/qgym.h,
        restated in tests/azmodel.py).  `stats`: `last_stats` of the search, plus "episodes" (E), "episodes_solved" (share ending in
        success), "samples", "valid", "bad".  The handles are of kinds of their own ("self-play", with "-reuse" / "-many" as `solve`'s),
        so a `solve` before and after answers as ever.  The batch's tensors are views of buffers those handles own: the next `self_play`
        writes them again.  PauliGym: the handles are built without add_perms, so `observe_packed` draws nothing and the logged
        observation is a function of the state alone (qg_vec_observe_packed never permutes; kernels_pauli_tile.hip).

        ValueError: the tree search's own (`solve`); neither or both of `states` / `num_episodes`; `difficulty` with `states`;
        num_episodes, episodes_per_state or capacity below 1; a log and samples of more than `SELF_PLAY_MAX_LOG_BYTES`; an env whose
        packed observation does not exist (a PauliGym of more than 64 observation columns).  All before any handle is built."""
        if (states is None) == (num_episodes is None):
            raise ValueError("self_play: give either states or num_episodes (states=None: targets reset on the device)")
        if states is not None and difficulty is not None:
            raise ValueError("self_play: difficulty goes with states=None (it is the scramble length of the device-side reset)")
        S = int(episodes_per_state)
        if S < 1 or (states is None and S != 1):
            raise ValueError("self_play: episodes_per_state must be at least 1, and 1 with states=None (every episode has a target of its own)")
        if states is None and int(num_episodes) < 1:
            raise ValueError("self_play: num_episodes must be at least 1")
        if states is not None and len(states) == 0:
            raise ValueError("self_play: no states")
        E = int(num_episodes) if states is None else len(states) * S
        opts = self._check_mcts(E, num_mcts_searches, C, searches=S, reuse_tree=reuse_tree, mcts_nodes=mcts_nodes, mcts_leaves=mcts_leaves,
                                virtual_loss=virtual_loss)
        cfg = self.env.config
        n, A, T = int(cfg["num_qubits"]), len(cfg["gateset"]), int(cfg["max_depth"])
        kind = self.env.env_kind
        cols = 2 * n + max(int(cfg.get("max_rotations", 5)), 1) if kind == "pauli" else 2 * n if kind == "clifford" else n
        if cols > 64:
            raise ValueError(f"self_play: the packed observation needs at most 64 observation columns, this env has {cols}")
        cap_samples = T * E if capacity is None else int(capacity)
        if cap_samples < 1:
            raise ValueError("self_play: capacity must be at least 1")
        rows = 2 * n if kind in ("pauli", "clifford") else n
        nbytes = _SelfPlayLog.nbytes(T, E, A, rows, 8, cap_samples)  # a row word is 8 bytes at most
        if nbytes > SELF_PLAY_MAX_LOG_BYTES:
            raise ValueError(f"self_play: the log of {T} decisions x {E} episodes and {cap_samples} samples takes up to {nbytes} bytes, more than the limit "
                             f"of {SELF_PLAY_MAX_LOG_BYTES}")
        held = self._handles(opts.kind("self-play"), opts.batches(E))
        real = held.vecs[-1]
        if held.log is None or held.log.shape != (T, E, A, cap_samples):
            held.log = None  # (the old buffers go first)
            held.log = _SelfPlayLog(T, E, A, real, cap_samples)
        rec = held.log
        rec.reset = None if states is not None else (real.difficulty if difficulty is None else int(difficulty), int(reset_seed))
        res = self._tree_search(states, held, opts, fast is True, rec)
        packed = res.packed
        n_samples, valid, bad = (int(x) for x in packed.n.tolist())  # the one host read of the collection
        stats = dict(res.stats, episodes=E, episodes_solved=float(res.success.sum()) / E, samples=n_samples, valid=valid, bad=bad)
        return SelfPlayBatch(n=n_samples, obs=packed.words[:n_samples], pi=packed.pi[:n_samples], z=packed.z[:n_samples], actions=packed.move[:n_samples],
                             index=packed.index[:n_samples], returns=res.returns, success=res.success,
                             lengths=rec.live[: res.steps].sum(dim=0, dtype=torch.int32), stats=stats, obs_cols=real.obs_shape_[1])

    def _check_options(self, empty: bool, fast, beam_width, merge_duplicates, twists, twist_kernels, bound):
        """ValueError for a combination of `solve`'s options that does not exist; what needs a handle's config (the metrics weights under `bound`)
        or the policy (`fast`, `twist_kernels`) is checked where those are at hand.  `empty`: no targets, only the checks on the views are made."""
        if twist_kernels and twists is None:
            raise ValueError("twist_kernels=True needs twists: it is the kernel path of a search under symmetry views")
        if twists is not None:
            if int(twists) < 1:
                raise ValueError("twists must be at least 1")
            if self.env.env_kind == "pauli":
                raise ValueError("twists: PauliGym permutes inside observe() / step() and exposes no twists (pauli.rs:675-679)")
            if fast:
                raise ValueError("fast=True cannot be combined with twists: the policy-layer kernels read the resident state, not a view"
                                 " (twist_kernels=True runs a twisted search on the kernels)")
        if empty:
            return
        if beam_width is not None:
            if int(beam_width) < 1:
                raise ValueError("beam_width must be at least 1")
            if merge_duplicates and self.env.env_kind == "pauli":
                raise ValueError("merge_duplicates: a PauliGym observation does not determine its state (rotations beyond the observed columns, DAG order)")
        elif merge_duplicates:
            raise ValueError("merge_duplicates needs beam_width")
        if bound is not None:
            if bound not in ("stop", "prune"):
                raise ValueError(f"bound must be None, 'stop' or 'prune', not {bound!r}")
            if beam_width is None:
                raise ValueError("bound needs beam_width")
            if self.env.env_kind == "pauli":
                raise ValueError("bound: a PauliGym step adds pauli_layer_reward per released rotation (pauli.rs:634), and a target may hold rotations "
                                 "beyond the observed columns: the reward still to come has no bound the search can see")

    def _check_mcts(self, trees: int, num_mcts_searches, C, max_expand_depth=1, deterministic=False, searches: Optional[int] = None, reuse_tree=False,
                    mcts_nodes=None, mcts_leaves=1, virtual_loss=0.0, conflicts: Optional[Dict[str, bool]] = None) -> Optional[_MctsOptions]:
        """The tree search on `trees` trees these arguments resolve to, after its ValueErrors; None (N = 0): none, and `C` and `max_expand_depth` mean
        nothing.  `searches`: S of `mcts_sampled`, else None.  `conflicts`: which of `solve`'s other options are on, by name -- it takes none."""
        N, mcts_sampled = int(num_mcts_searches), searches is not None
        K, vl = int(mcts_leaves), float(virtual_loss)
        for bad, why in ((N < 0, "num_mcts_searches must be at least 0"),
                         (mcts_sampled and N == 0, "mcts_sampled=True needs num_mcts_searches >= 1: it draws the moves of a tree search"),
                         (reuse_tree and N == 0, "reuse_tree=True needs num_mcts_searches >= 1: it keeps the subtree of a tree search's move"),
                         (mcts_nodes is not None and not reuse_tree, "mcts_nodes needs reuse_tree=True: without it a tree holds the N + 1 nodes of one decision"),
                         (not 1 <= K <= MCTS_MAX_LEAVES, f"mcts_leaves must satisfy 1 <= mcts_leaves <= {MCTS_MAX_LEAVES}, got {K}"),
                         (not (vl >= 0.0 and vl < float("inf")), "virtual_loss must be finite and at least 0"),
                         (K > 1 and N == 0, "mcts_leaves > 1 needs num_mcts_searches >= 1: it is the leaf batch of a tree search"),
                         (vl != 0.0 and K == 1, "virtual_loss needs mcts_leaves > 1: one descent per launch leaves no virtual visits behind"),
                         (K > N >= 1, f"mcts_leaves={K} is more than num_mcts_searches={N}: a decision makes at most N descents")):
            if bad:
                raise ValueError(why)
        if N == 0:
            return None
        for bad, why in ((not float(C) > 0.0, "C must be positive"),
                         (int(max_expand_depth) != 1, "max_expand_depth: only 1 is built (one new node per simulation)"),
                         (mcts_sampled and deterministic, "mcts_sampled=True draws its moves: it cannot be combined with deterministic=True"),
                         (not (mcts_sampled or deterministic), "num_mcts_searches needs deterministic=True, or mcts_sampled=True to draw the moves from the visit counts")):
            if bad:
                raise ValueError(why)
        mixed = [name for name, on in (conflicts or {}).items() if on]
        if mixed:
            raise ValueError(f"num_mcts_searches cannot be combined with {', '.join(mixed)}")
        cap = (int(mcts_nodes) if mcts_nodes is not None else _MctsOptions.default_cap(N)) if reuse_tree else None
        if cap is not None and not N + 1 <= cap <= MCTS_MAX_CAP:
            raise ValueError(f"mcts_nodes must satisfy num_mcts_searches + 1 = {N + 1} <= mcts_nodes <= {MCTS_MAX_CAP}, got {cap}")
        opts = _MctsOptions(N, float(C), searches, cap, K, vl)
        nbytes = int(_lib.load().qg_mcts_forest_bytes(trees, min(opts.nodes, 2 ** 32 - 1), len(self.env.config["gateset"])))
        if nbytes > MCTS_MAX_FOREST_BYTES:
            raise ValueError(f"num_mcts_searches={N}: the forest of {trees} trees takes {nbytes} bytes, more than the limit of {MCTS_MAX_FOREST_BYTES}")
        return opts

    def _sampled_search(self, states, deterministic: bool, num_searches: int, fast: Optional[bool], views: Optional[List[int]], twist_kernels: bool):
        """The sampled and the greedy search of `solve`: every (target, search) pair is one env of the "search" handle, one view per search;
        per target the successful search of the highest return wins.  PauliGym: the winners are replayed for their rotation markers."""
        M, V = len(states), 1 if views is None else len(views)
        S = 1 if deterministic else max(1, int(num_searches))  # greedy episodes are all alike
        if views is not None and deterministic:
            S = V  # ... but for the view they are seen through
        held = self._handles("search", (M * S,), views is not None)
        vec = held.vecs[0]
        B, A, dev = vec.batch, vec.num_actions(), vec.device
        tw = None if views is None else self._twist_index(views, S, M, None, dev)
        self._load(vec, states, S)
        T = int(vec._cfg.max_depth)
        actions = torch.empty((T, B), dtype=torch.int32, device=dev)
        finished = vec.success.bool().clone()  # a target that is already solved needs no gates
        solved_at = torch.where(finished, 0, -1).to(torch.int32)
        ret = torch.zeros(B, dtype=torch.float32, device=dev)
        parked = torch.full((B,), A, dtype=torch.int32, device=dev)  # out of range: no gate (clifford.rs:324)
        steps = 0
        if twist_kernels or fast:
            kernels = True
        elif tw is None and fast is not False and not deterministic and B >= 4096:  # fast=None: where the kernels apply; greedy: on request only
            kernels = None
        else:
            kernels = False
        fwd = self._forward(held, 1, tw, kernels)
        choose = (lambda t: fwd.greedy(vec)) if deterministic else (lambda t: fwd.draw(vec, t))
        self.last_stats = {"kernels": fwd.kernels}
        for t in range(T):
            act = fwd.real_actions(vec, choose(t))
            actions[t] = torch.where(finished, parked, act)
            vec.step(actions[t])
            live = ~finished
            ret += torch.where(live, vec.reward, torch.zeros_like(ret))
            solved_at = torch.where(live & vec.success.bool(), t + 1, solved_at)
            finished |= vec.done.bool()
            steps = t + 1
            if t % 8 == 7 and bool(finished.all()):
                break
        vec.sync()
        ok = (solved_at >= 0).view(M, S)
        best = _winner(ok, ret.view(M, S))[1]
        idx = torch.arange(M, device=dev) * S + best
        lengths = solved_at[idx].cpu().numpy()
        found = ok.any(dim=1).cpu().numpy()
        win = actions[:steps, idx].t().contiguous()  # [M, steps]
        self.last_stats.update({"targets": M, "searches": S, "steps": steps, "solved": int(found.sum()),
                           "searches_solved": float(ok.float().mean()), "mean_gates": float(lengths[found].mean()) if found.any() else 0.0})
        if tw is not None:
            self.last_stats["views"] = V
        if vec.env_kind != "pauli":
            w = win.cpu().numpy()
            return [w[m, : lengths[m]].tolist() if found[m] else None for m in range(M)]
        # PauliEnv: replay the winners with the solution log on; padding entries (no gate, no marker) are dropped
        rep = self._handles("replay", (M,)).vecs[0]
        self._load(rep, states, 1)
        keep = torch.arange(steps, device=dev).view(1, -1) < solved_at[idx].view(-1, 1)
        rep.rollout(torch.where(keep, win, torch.full_like(win, A)).t().contiguous())
        rep.sync()
        out: List[Optional[List[int]]] = []
        for m in range(M):
            out.append([v for v in rep.solution(m) if v >= ROTATION_MARKER or v < A] if found[m] else None)
        return out

    def synth(self, inputs, deterministic: bool = False, num_searches: int = 100, beam_width: Optional[int] = None, merge_duplicates: bool = False,
              twists: Optional[int] = None, fast: Optional[bool] = None, twist_kernels: bool = False, bound: Optional[str] = None,
              num_mcts_searches: int = 0, C: float = 2 ** 0.5, max_expand_depth: int = 1, mcts_sampled: bool = False, reuse_tree: bool = False,
              mcts_nodes: Optional[int] = None, mcts_leaves: int = 1, virtual_loss: float = 0.0):
        """`RLSynthesis.synth` over a list of inputs: circuits (needs qiskit) or None where no search succeeded."""
        sols = self.solve([self.env.get_state(x) for x in inputs], deterministic, num_searches, fast=fast, beam_width=beam_width,
                          merge_duplicates=merge_duplicates, twists=twists, twist_kernels=twist_kernels, bound=bound,
                          num_mcts_searches=num_mcts_searches, C=C, max_expand_depth=max_expand_depth, mcts_sampled=mcts_sampled,
                          reuse_tree=reuse_tree, mcts_nodes=mcts_nodes, mcts_leaves=mcts_leaves, virtual_loss=virtual_loss)
        return [self.env.build_circuit_from_solution(s, x) if s is not None else None for s, x in zip(sols, inputs)]

    def gate_lists(self, solutions):
        """Solutions as `(name, qubits)` lists (rotation markers of PauliGym solutions are skipped)."""
        gs = self.env.config["gateset"]
        return [None if s is None else [(gs[a][0], tuple(gs[a][1])) for a in s if a < ROTATION_MARKER] for s in solutions]
