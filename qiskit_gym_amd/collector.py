"""GPU-resident rollout collection: observation, policy forward, sampling, env.step, auto-reset and
advantage estimation all stay on the device.

The reference collects episodes inside twisterl: rayon workers clone the scalar env per episode and
run a Rust copy of the policy on the CPU (`rl/synthesis.py:128-138`, notebook timing keys `collect`,
`data_to_torch`).  With the env batch resident in HBM one collection step is

    reset_done -> observe (bits -> policy dtype) -> 3 GEMMs -> sample -> step

i.e. five libqgym launches plus the policy's GEMMs, and the trajectories are born as torch tensors --
there is no `data_to_torch`.  The observation is written straight in the dtype the first layer
reads (`qg_vec_observe_dense_as`), actions / log-probs / entropy / values come out of one sampling
kernel (`qg_sample_actions`), rewards and episode ends are written by the step kernel into row t of
the rollout, and GAE(lambda) runs as one kernel over the finished [T, B] rollout (`qg_gae`).

For the reference's default policy shape in bf16 (and batches of a few thousand envs or more) the forward
pass needs no tensor library and no observation at all:

    reset_done -> [packed observation for the rollout] -> first layer from the bits -> middle layer + head + draw -> step

`qg_vec_embed` reads the resident TILE-layout state, `qg_policy_embed_words` the packed observation words of every
other layout (PauliEnv, wide CliffordEnv), `qg_policy_mid_head_sample` does the rest in one kernel.

`BasicPolicy` mirrors the shape of the reference's default policy network (`twisterl.nn.BasicPolicy`
as configured by `BasicPolicyConfig`, `rl/configs.py:531-607`; checkpoint shapes in
`examples/models/*.pt`): Linear(prod(obs_shape) -> 512) -> ReLU -> Linear(512 -> 256) -> ReLU ->
{Linear(256 -> num_actions), Linear(256 -> 1)}.

The kernels' wrappers, `BasicPolicy` and the packed operands live in `policy_kernels.py`, the layer below this module and the searches
(`synthesis.py`); every name of theirs that was importable from here still is.
"""
from __future__ import annotations

from dataclasses import dataclass, field
from typing import Optional, Tuple  # noqa: F401

import torch
import torch.nn as nn

from . import _lib
from .policy_kernels import (_DT, AzPack, BasicPolicy, FirstLayer, PolicyOperands, _linear_relu, _logp_outputs, _twist_operands, az_pack, beam_advance, beam_merge, beam_seen, beam_select,  # noqa: F401
                             embed, embed_words, expand_packed, first_layer, gae, head_logp, head_sample, mcts_backup, mcts_backup_many, mcts_decide, mcts_forest, mcts_rebase, mcts_select, mcts_select_many, mid_head_logp,
                             mid_head_sample, mid_head_sample_step, pack_embed_words, pack_embedding, pack_first, pack_head, pack_mid, run_first_layer, sample_actions,
                             twist_expand_packed, twist_pack_words, untwist_actions)
from .vec import VecEnv, _stream_ptr


@dataclass
class Rollout:
    obs: torch.Tensor         # [T, B, rows*cols] int8 dense observation before each action, or
                              # [T, B, words] bit-packed rows when the collector stores packed observations
    actions: torch.Tensor     # [T, B] int64
    logp: torch.Tensor        # [T, B] float32 log-prob of the action under the collecting policy
    entropy: torch.Tensor     # [T, B] float32
    values: torch.Tensor      # [T, B] float32
    rewards: torch.Tensor     # [T, B] float32
    dones: torch.Tensor       # [T, B] uint8 (episode ended with this step)
    advantages: torch.Tensor  # [T, B] float32 GAE(lambda)
    returns: torch.Tensor     # [T, B] float32 advantages + values
    last_values: Optional[torch.Tensor] = None  # [B] float32 value of the state after the last step (GAE bootstrap)
    obs_packed: bool = False
    obs_cols: int = 0

    def dense_obs(self, dtype: torch.dtype = torch.float32, t: Optional[slice] = None) -> torch.Tensor:
        """[T', B, rows*cols] dense observation in `dtype` (re-expanded from the packed rows when stored packed)."""
        o = self.obs if t is None else self.obs[t]
        if not self.obs_packed:
            return o.to(dtype)
        return expand_packed(o, self.obs_cols, dtype).flatten(-2)


@dataclass
class SelfPlayBatch:
    """What `BatchedSynthesis.self_play` returns: the decisions of a batch of self-play episodes (E of them, each a sampled tree search) as
    the samples an AlphaZero-style learner reads, packed on the device by `az_pack` in (decision, episode) order.  The tensors are views of
    buffers that the synthesis object's self-play handles own: the next `self_play` call writes them again, so a learner that keeps a
    batch across calls clones what it keeps."""
    n: int                  # samples
    obs: torch.Tensor       # [n, W] bit-packed observation before the move (`VecEnv.observe_packed` words)
    pi: torch.Tensor        # [n, A] float32: the root's visit counts over their sum
    z: torch.Tensor         # [n] float32: the undiscounted return from this decision to the episode's end (f32 sums from the end)
    actions: torch.Tensor   # [n] int32: the move drawn from the counts
    index: torch.Tensor     # [n] int32: t * E + e, decision t of episode e; strictly ascending
    returns: torch.Tensor   # [E] float32: the episode's rewards summed forward in f32 by the search (not z at t = 0: it rounds differently)
    success: torch.Tensor   # [E] bool: the episode ended in success
    lengths: torch.Tensor   # [E] int32: the decisions the episode was live for
    stats: dict = field(default_factory=dict)  # the search's `last_stats` plus episodes, episodes_solved, samples, valid, bad
    obs_cols: int = 0

    def dense_obs(self, dtype: torch.dtype = torch.float32) -> torch.Tensor:
        """[n, rows*cols] dense {0,1} observation in `dtype`, re-expanded from the packed rows (`expand_packed`)."""
        if self.n == 0:
            return torch.empty((0, self.obs.shape[1] * self.obs_cols), dtype=dtype, device=self.obs.device)
        return expand_packed(self.obs, self.obs_cols, dtype).flatten(-2)


@dataclass(frozen=True)
class CollectorRoute:
    """How a collector runs its policy, decided once in its constructor.  first: "state" / "words" (the first layer from the env's bits,
    `policy_kernels.first_layer`) or "dense" (`observe_as` into the policy input, then a library GEMM).  tail: "mid_head" (middle layer +
    head + draw in one kernel), "head" (a library GEMM for the middle layer, then `head_sample`), "heads_gemm" (three library GEMMs on the
    fused head weight, then `sample_actions`) or "module" (any `nn.Module`, then `sample_actions`).  fused_step: sampling, `env.step` and
    the reset of the finished envs in one call."""
    first: str
    tail: str
    fused_step: bool


class _DenseFirst:
    """first == "dense".  `observe(row)`: the observation of the current state into `row` (the rollout's, in its store's form; None: nowhere)
    and, as `dtype`, into the policy input `x`, which it returns; calling the object: the first layer of a `BasicPolicy` on it."""
    layer = None  # no packed first layer to refresh

    def __init__(self, env: VecEnv, policy: nn.Module, dtype: torch.dtype, packed_store: bool):
        self.env, self.policy, self.dtype, self.packed_store = env, policy, dtype, packed_store
        self.x = torch.empty((env.batch, env.obs_shape_[0] * env.obs_shape_[1]), dtype=dtype, device=env.device)

    def observe(self, row: Optional[torch.Tensor]) -> torch.Tensor:
        env = self.env
        if row is None:
            return env.observe_as(self.dtype, out=self.x)
        if self.packed_store:
            env.observe_packed(out=row)
        else:
            env.observe(out=row.view(env.batch, *env.obs_shape_))
        if env.env_kind != "pauli":
            env.observe_as(self.dtype, out=self.x)
        elif self.packed_store:
            # PauliEnv.observe() with add_perms draws a permutation (pauli.rs:657-662): observe once, expand the stored row words
            expand_packed(row, env.obs_shape_[1], self.dtype, out=self.x.view(env.batch, *env.obs_shape_))
        else:  # ... observe once, widen the stored bytes
            _lib.check(_lib.load().qg_widen_dense(row.data_ptr(), row.numel(), self.x.data_ptr(), _DT[self.dtype], _stream_ptr()))
        return self.x

    def __call__(self, row: Optional[torch.Tensor]) -> torch.Tensor:
        emb = self.policy.embeddings
        return _linear_relu(self.observe(row), emb.weight, emb.bias)


class _KernelFirst:
    """first == "state" / "words": relu(obs W1^T + b1) from the env's bits into `h1`, no dense observation exists.  Called with the
    rollout's row, which receives the observation on the way, or with None.  "state" with a packed store: the layer's own launch writes the
    row (qg_vec_embed_observe).  "words" (packed store only): the layer reads the row the rollout stores, or a scratch buffer."""

    def __init__(self, env: VecEnv, layer: FirstLayer, ops: PolicyOperands, hidden: int, packed_store: bool):
        self.env, self.layer, self.ops, self.hidden, self.packed_store = env, layer, ops, hidden, packed_store
        self.h1 = torch.empty((env.batch, hidden), dtype=torch.bfloat16, device=env.device)
        self.words = torch.empty((env.batch, env.packed_words_per_env), dtype=torch.int64, device=env.device) if layer.route == "words" else None

    def __call__(self, row: Optional[torch.Tensor]) -> torch.Tensor:
        env = self.env
        if row is not None and not self.packed_store:
            env.observe(out=row.view(env.batch, *env.obs_shape_))
            row = None
        # where the packed observation goes: `obs_out` on the state route, `words` on the words route
        return run_first_layer(self.layer, env, self.ops.bias, self.hidden, out=self.h1, words=self.words if row is None else row, obs_out=row)


class _Forward:
    """What `_body` asks of the policy: `refresh()` the operands from the current weights, in place; `sample(ro, t)`: observe the current
    state into row t of the rollout and draw row t's actions, log-probs, entropy and values; `value()`: the value of the current state,
    f32 [B].  One subclass per `CollectorRoute.tail`; the first layer is `first`, a `_DenseFirst` or a `_KernelFirst`."""

    def __init__(self, env: VecEnv, policy: nn.Module, first, ops: Optional[PolicyOperands], seed: int, clock: torch.Tensor):
        self.env, self.policy, self.first, self.ops, self.seed, self.clock = env, policy, first, ops, seed, clock

    def refresh(self):
        self.ops.repack_(self.policy, self.first.layer, self.env)


class _ModuleForward(_Forward):
    """tail == "module": any policy module on the dense observation."""

    def refresh(self):
        pass

    def sample(self, ro: Rollout, t: int):
        logits, value = self.policy(self.first.observe(ro.obs[t]))
        sample_actions(logits.contiguous(), self.seed, t, actions=ro.actions[t], logp=ro.logp[t], entropy=ro.entropy[t], clock=self.clock)
        ro.values[t].copy_(value)

    def value(self) -> torch.Tensor:
        return self.policy(self.first.observe(None))[1].float()


class _GemmForward(_Forward):
    """tail == "heads_gemm": library GEMMs up to the fused head's output [B, pad8(A + 1)], column A is the value."""

    def _trunk(self, row: Optional[torch.Tensor]) -> torch.Tensor:
        pol, ops = self.policy, self.ops
        return torch.addmm(ops.b, _linear_relu(self.first(row), pol.common.weight, pol.common.bias), ops.w.t())

    def sample(self, ro: Rollout, t: int):
        A = self.ops.A
        sample_actions(self._trunk(ro.obs[t]), self.seed, t, num_actions=A, value_col=A, actions=ro.actions[t], logp=ro.logp[t], entropy=ro.entropy[t],
                       values=ro.values[t], clock=self.clock)

    def value(self) -> torch.Tensor:
        return self._trunk(None)[:, self.ops.A].float()


class _HeadForward(_Forward):
    """tail == "head": a library GEMM for the middle layer, then last layer + draw in one kernel; the logits never reach memory.  The value
    of the current state is that kernel's value output (its draw is discarded)."""

    def __init__(self, *args):
        super().__init__(*args)
        self.scratch_actions = torch.empty(self.env.batch, dtype=torch.int64, device=self.env.device)
        self.scratch = torch.empty((3, self.env.batch), dtype=torch.float32, device=self.env.device)

    def _draw(self, row: Optional[torch.Tensor], counter: int, actions, logp, entropy, values, clock):
        pol = self.policy
        head_sample(_linear_relu(self.first(row), pol.common.weight, pol.common.bias), self.ops.head, self.ops.A, self.seed, counter, actions=actions,
                    logp=logp, entropy=entropy, values=values, clock=clock)

    def sample(self, ro: Rollout, t: int):
        self._draw(ro.obs[t], t, ro.actions[t], ro.logp[t], ro.entropy[t], ro.values[t], self.clock)

    def value(self) -> torch.Tensor:
        s = self.scratch
        self._draw(None, 0, self.scratch_actions, s[0], s[1], s[2], None)
        return s[2]


class _MidHeadForward(_HeadForward):
    """tail == "mid_head": middle layer + head + draw in one kernel, only the first layer stays outside; `sample_step` is `sample` with
    `env.step` and the reset of the envs that finished in the same call (`CollectorRoute.fused_step`)."""

    def _draw(self, row: Optional[torch.Tensor], counter: int, actions, logp, entropy, values, clock):
        mid_head_sample(self.first(row), self.ops.mid, self.policy.common.out_features, self.ops.head, self.ops.A, self.seed, counter, actions=actions,
                        logp=logp, entropy=entropy, values=values, clock=clock)

    def sample_step(self, ro: Rollout, t: int):
        # reset_seed: the seed of step t + 1's reset_done; the device clock advances by T between collections, so the last step of a
        # collection resets with what the next collection's first reset_done would use
        mid_head_sample_step(self.env, self.first(ro.obs[t]), self.ops.mid, self.policy.common.out_features, self.ops.head, self.seed, t, ro.actions[t],
                             ro.logp[t], ro.entropy[t], ro.values[t], rewards=ro.rewards[t], dones=ro.dones[t],
                             reset_seed=self.seed + 0x9E3779B9 * (t + 2))


_FORWARDS = {"module": _ModuleForward, "heads_gemm": _GemmForward, "head": _HeadForward, "mid_head": _MidHeadForward}


class RolloutCollector:
    """Steps `env` for T steps under `policy`, resetting finished episodes on the device.

    store_obs: "dense" keeps the int8 observation of every step (the Gym adapter's format);
    "packed" keeps the bit-packed rows (8x smaller for CliffordGym, one 64-bit word per observation row for
    PauliGym; `Rollout.dense_obs` expands them on demand).

    use_graph: capture the whole T-step collection (every env kernel, the policy GEMMs, sampling,
    GAE) into one hipGraph on the first call and replay it afterwards -- one host call per rollout
    instead of ~10 per step.  The rollout tensors are then reused between calls (clone what must
    outlive the next `collect`), and policy parameters must be updated in place (optimisers do).

    Randomness: step number n of the collector (counted over its lifetime, kept in a device clock
    so that graph replays advance it) resets finished episodes with seed `seed + 0x9E3779B9 * (n + 1)`
    and samples with counter n; both modes therefore produce the same trajectories.

    `env.difficulty = d` between two collections holds for every reset of the next one, on every route: a graph captured at another
    difficulty is captured again (as for a new T).

    `route` (a `CollectorRoute`) says which kernels run the policy; `operands` are the `PolicyOperands` of a `BasicPolicy` (None for
    another module), repacked in place at the top of every collection."""

    def __init__(self, env: VecEnv, policy: nn.Module, dtype: torch.dtype = torch.bfloat16, seed: int = 0, gamma: float = 0.995,
                 gae_lambda: float = 0.995, store_obs: str = "dense", use_graph: bool = False, use_bit_embedding: Optional[bool] = None,
                 use_fused_head: Optional[bool] = None, use_fused_step: Optional[bool] = None):
        self.env = env
        self.policy = policy.to(device=env.device, dtype=dtype)
        self.dtype = dtype
        self.seed = int(seed)
        self.gamma, self.gae_lambda = float(gamma), float(gae_lambda)  # rl/configs.py:136-137
        r, c = env.obs_shape_
        self.obs_size = r * c
        if store_obs not in ("dense", "packed"):
            raise ValueError("store_obs must be 'dense' or 'packed'")
        if store_obs == "packed" and env.env_kind == "pauli" and env.obs_shape_[1] > 64:
            raise ValueError("PauliGym observations wider than 64 columns have no packed form")
        self.store_obs = store_obs
        self.use_graph = bool(use_graph)
        self.clock = torch.zeros(1, dtype=torch.int64, device=env.device)  # collector steps taken so far
        env.set_clock(self.clock)
        # the policy-layer kernels at every batch size: below ~ 4 096 envs the launches take their small-batch shapes (a 32-env tile per
        # wave / workgroup, weight fragments straight from L2: CliffordGym 16q x 1 024 envs 19 us per step against 42 us on library GEMMs,
        # PauliGym 20q 36 against 44)
        if use_bit_embedding is None:
            use_bit_embedding = True
        if use_fused_head is None:
            use_fused_head = True
        pol, packed_store = self.policy, store_obs == "packed"
        kernels = isinstance(pol, BasicPolicy) and dtype == torch.bfloat16  # what the policy-layer kernels read
        self.operands = PolicyOperands(pol, fused_tail=bool(kernels and use_fused_head)) if isinstance(pol, BasicPolicy) else None
        # the first layer from the env's bits: the resident TILE-layout state, or -- the layouts that kernel does not cover (PauliEnv,
        # CliffordEnv N > 16, ...) -- the packed observation words the rollout stores anyway; every other layout keeps the dense first layer
        first = _DenseFirst(env, pol, dtype, packed_store)
        if use_bit_embedding and kernels and pol.embeddings.in_features == self.obs_size:
            try:
                layer = first_layer(env, pol.embeddings.weight, ("state", "words") if packed_store else ("state",))
                first = _KernelFirst(env, layer, self.operands, pol.embeddings.out_features, packed_store)
            except (ValueError, _lib.QGymError):
                pass
        ops = self.operands
        tail = "module" if ops is None else "heads_gemm" if ops.head is None else "head" if ops.mid is None else "mid_head"
        # sampling, env.step and the reset of the finished envs in ONE call (qg_vec_mid_head_sample_step_reset): TILE-layout envs
        inverts = bool(env.config.get("add_inverts", True))
        can_fuse_step = (tail == "mid_head" and ((env.env_kind == "clifford" and env.num_qubits <= 16)  # with add_inverts too (qm_inv2_body)
                                                 or (env.env_kind == "linear_function" and 8 < env.num_qubits <= 32 and not inverts)))
        self.route = CollectorRoute("dense" if first.layer is None else first.layer.route, tail,
                                    can_fuse_step if use_fused_step is None else bool(use_fused_step) and can_fuse_step)
        self._fwd = _FORWARDS[tail](env, pol, first, ops, self.seed, self.clock)
        self._graph = None
        self._graph_T = 0
        self._graph_ro: Optional[Rollout] = None
        self._difficulty = env.difficulty  # of the latest collection; a graph keeps the one it was captured with
        self._last_dones: Optional[torch.Tensor] = None  # the latest collection's last row of `dones`

    @property
    def steps_done(self) -> int:
        return int(self.clock.item())

    def _alloc(self, T: int) -> Rollout:
        env, B, dev = self.env, self.env.batch, self.env.device
        f32 = dict(dtype=torch.float32, device=dev)
        if self.store_obs == "packed":
            dt = {1: torch.uint8, 4: torch.int32, 8: torch.int64}[env.packed_word_bytes]
            obs = torch.empty((T, B, env.packed_words_per_env), dtype=dt, device=dev)
        else:
            obs = torch.empty((T, B, self.obs_size), dtype=torch.int8, device=dev)
        return Rollout(obs=obs, actions=torch.empty((T, B), dtype=torch.int64, device=dev), logp=torch.empty((T, B), **f32),
                       entropy=torch.empty((T, B), **f32), values=torch.empty((T, B), **f32), rewards=torch.empty((T, B), **f32),
                       dones=torch.empty((T, B), dtype=torch.uint8, device=dev), advantages=torch.empty((T, B), **f32),
                       returns=torch.empty((T, B), **f32), obs_packed=self.store_obs == "packed", obs_cols=env.obs_shape_[1])

    def _body(self, ro: Rollout, T: int):
        env, fwd = self.env, self._fwd
        fwd.refresh()
        for t in range(T):
            # finished episodes start over (reference: the collector calls reset() on a fresh clone);
            # the kernels add the device clock: effective seed = seed + 0x9E3779B9 * (clock + t + 1)
            env.set_counters(t, t)  # coin / permutation draws: counter t + clock, eager or replayed
            if t == 0 or not self.route.fused_step:  # with the fused step the envs that finish in step t are reset by step t's own call
                env.reset_done(self.seed + 0x9E3779B9 * (t + 1))
            # masks() is all-true for a live env (clifford.rs:349-351), so sampling needs no mask
            if self.route.fused_step:
                fwd.sample_step(ro, t)
            else:
                fwd.sample(ro, t)
                env.rollout(ro.actions[t : t + 1], rewards_out=ro.rewards[t : t + 1], dones_out=ro.dones[t : t + 1])
        # bootstrap value of the state after the last step (masked by `dones` where the episode ended)
        if env.env_kind != "pauli":  # PauliEnv: observing would draw a permutation; episodes are short, bootstrap with 0 (last_values stays None)
            if ro.last_values is None:
                ro.last_values = torch.empty(env.batch, dtype=torch.float32, device=env.device)
            ro.last_values.copy_(fwd.value())
        gae(ro.rewards, ro.values, ro.dones, ro.last_values, self.gamma, self.gae_lambda, advantages=ro.advantages, returns=ro.returns)
        self.clock.add_(T)

    @torch.no_grad()
    def collect(self, T: int, out: Optional[Rollout] = None) -> Rollout:
        env = self.env
        new_difficulty = env.difficulty != self._difficulty  # `env.difficulty = d` since the latest collection (a curriculum's next stage)
        if new_difficulty:
            self._difficulty = env.difficulty
            # the fused step has already restarted the envs that finished in the latest collection's last step, with the old scramble length:
            # end those episodes again, and this collection's first reset_done restarts them -- same seed -- at the new difficulty, which is
            # what the separate launches do
            if self.route.fused_step and self._last_dones is not None:
                torch.maximum(env.done, self._last_dones, out=env.done)
        if not self.use_graph:
            ro = self._alloc(T) if out is None else out
            self._body(ro, T)
            self._last_dones = ro.dones[T - 1] if T else None
            return ro
        if self._graph is not None and self._graph_T == T and not new_difficulty:
            self._graph.replay()
            return self._graph_ro
        # first call (or a new T, or a new difficulty: the scramble length, the start depth and the choice of reset kernels are arguments the
        # captured launches keep): one eager pass (allocates scratch, warms the GEMM handles, and IS
        # this call's rollout), then capture the same body for the calls that follow
        ro = self._alloc(T)
        self._body(ro, T)
        self._last_dones = ro.dones[T - 1] if T else None
        torch.cuda.synchronize()
        graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(graph):  # records, does not run: the env state and the clock are untouched
            self._body(ro, T)
        torch.cuda.synchronize()
        self._graph, self._graph_T, self._graph_ro = graph, T, ro
        return ro

