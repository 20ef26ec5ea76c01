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
the batched clone (`VecEnv.copy_envs`) and the device-side selection kernel (`collector.beam_select`); see `solve`.

`solve(..., fast=True)` takes the policy off the tensor library: the first layer reads the bit-packed state (`collector.embed` /
`embed_words`), the rest is one kernel that either draws (`mid_head_sample`: the sampled searches) or, for the greedy and the beam search,
writes the arg-max and the row of log-probabilities (`mid_head_logp`), which `beam_select` reads as it stands.

`solve(..., twists=V)` gives every target V symmetry views (`VecEnv.observe_twisted` / `untwist_actions`): the policy looks at a target through
an automorphism of the coupling map and its choice is mapped back, what `RLSynthesis.init_algorithm` hands the reference's policy as
`obs_perms` / `act_perms` (rl/synthesis.py:97-104) -- here one fixed view per search, so the deterministic searches get V opinions per target.
`twist_kernels=True` runs such a search on the policy-layer kernels: the view is written as packed words (`VecEnv.observe_twisted_words`),
which is what `embed_words` reads.
"""
from __future__ import annotations

from typing import Dict, List, Optional, Sequence

import numpy as np
import torch

from . import _lib
from .collector import (BasicPolicy, beam_merge, beam_seen, beam_select, embed, embed_words, mid_head_logp, mid_head_sample, pack_embed_words, pack_embedding,
                        pack_head, pack_mid, sample_actions)
from .envs.gyms import ROTATION_MARKER
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


class BatchedSynthesis:
    """`env`: one of the *Gym front ends (its configuration and gateset are used); `policy`: a module mapping the flat
    observation [B, rows*cols] to (logits [B, num_actions], value [B])."""

    def __init__(self, env, policy: torch.nn.Module, dtype: torch.dtype = torch.float32, seed: int = 0, device=None):
        self.env = env
        self.dtype = dtype
        self.seed = int(seed)
        self.device = device
        self._policy = policy
        self._vecs: Dict[tuple, VecEnv] = {}
        self._beam = None  # ((targets, width), (two search batches, the winners)): the beam search's handles
        self._view_list = None  # twists: the twist index behind each view (`_views`)
        # the policy-layer kernels' operands per search handle, by id(vec): (vec, packed first layer, its f32 bias, packed middle layer, packed
        # head, words route?) or None where they do not apply.  The first layer is packed through the handle it will read (`pack_embedding`);
        # bias, middle layer and head are packed once and shared (`_packed_tail`).  All of it is a snapshot of the policy's weights at
        # `_packed_at` (the parameters' version counters): an in-place update of the policy drops the whole cache, so the kernels never run
        # one layer of the new weights with another of the old, and follow the policy as the torch forward does.
        self._packed: Dict[int, Optional[tuple]] = {}
        self._packed_tail = None
        self._packed_views = None  # twist_kernels: the first layer packed for `embed_words` on the views' words (no handle in it: packed once)
        self._packed_at = None
        self.last_stats: dict = {}

    _NO_KERNELS = "fast=True needs a BasicPolicy of the default shape and an env whose state or packed observation the first-layer kernels read"

    _NO_TWIST_KERNELS = "twist_kernels=True needs a BasicPolicy of the default shape and an env with twists whose observation has at most 64 columns"

    def _weights_current(self):
        """Drop every packed operand when the weights were updated in place since they were packed."""
        at = tuple((id(p), p._version) for p in self._policy.parameters())
        if at != self._packed_at:
            self._packed.clear()
            self._packed_tail, self._packed_views, self._packed_at = None, None, at

    def _tail(self):
        """Bias of the first layer, packed middle layer and head: packed once, shared by every handle and by the views."""
        if self._packed_tail is None:
            pol = self._policy
            w, b, A = pol.fused_heads()
            self._packed_tail = (pol.embeddings.bias.detach().float().contiguous(), pack_mid(pol.common.weight, pol.common.bias),
                                 pack_head(w, b, A, A, after_mid=True))
        return self._packed_tail

    def _view_kernels(self, vec: VecEnv):
        """Operands of the policy-layer kernels for a search under twists, in the form of `_kernels`: the first layer is `embed_words` on
        `observe_twisted_words`, whose row count is the env's rounded up to even -- the weight gets `cols` zero columns for the pad word.
        ValueError where they do not apply."""
        pol = self._policy
        if not isinstance(pol, BasicPolicy):
            raise ValueError(self._NO_TWIST_KERNELS)
        self._weights_current()
        if self._packed_views is None:
            rows, cols = vec.obs_shape_
            try:
                if cols > 64 or vec.packed_words_per_env != rows:
                    raise ValueError("a row of the view is one 64-bit word")
                w = pol.embeddings.weight.detach()
                if rows % 2:
                    w = torch.nn.functional.pad(w, (0, cols))
                self._packed_views = (pack_embed_words(w, rows + rows % 2, cols), *self._tail())
            except (ValueError, KeyError, _lib.QGymError) as e:
                raise ValueError(f"{self._NO_TWIST_KERNELS} ({e})") from None
        return (vec, *self._packed_views, True)

    def _kernels(self, vec: VecEnv):
        """Operands of the two policy-layer kernels (qg_vec_embed, qg_policy_mid_head_sample / _logp: bf16 products, f32 accumulation) when the
        policy has the default shape and the env a TILE layout or 64-bit observation words; None otherwise (the torch forward is used)."""
        pol = self._policy
        if not isinstance(pol, BasicPolicy):
            return None
        self._weights_current()
        hit = self._packed.get(id(vec))
        if hit is not None and hit[0] is vec:
            return hit
        packed = None
        try:
            try:
                first = pack_embedding(vec, pol.embeddings.weight)  # TILE layout: the first layer reads the resident state
                words = False
            except (ValueError, _lib.QGymError):
                if vec.packed_word_bytes != 8 or vec.packed_words_per_env != vec.obs_shape_[0]:
                    raise
                first = pack_embed_words(pol.embeddings.weight, *vec.obs_shape_)  # 64-bit row words (PauliEnv, wide CliffordEnv): qg_policy_embed_words
                words = True
            packed = (vec, first, *self._tail(), words)
        except (ValueError, _lib.QGymError):
            packed = None
        if packed is not None:
            self._packed[id(vec)] = packed
        return packed

    def _close(self, vec: VecEnv):
        self._packed.pop(id(vec), None)
        vec.close()

    def _words_buf(self, vec: VecEnv, kern, tw: Optional[torch.Tensor]) -> Optional[torch.Tensor]:
        """Where the words route of `_first_layer` keeps its packed observation (None for the resident-state route)."""
        if not kern[5]:
            return None
        rows = vec.obs_shape_[0] + vec.obs_shape_[0] % 2 if tw is not None else vec.packed_words_per_env
        return torch.empty((vec.batch, rows), dtype=torch.int64, device=vec.device)

    def _first_layer(self, vec: VecEnv, kern, h1: torch.Tensor, words_buf: Optional[torch.Tensor], tw: Optional[torch.Tensor] = None) -> torch.Tensor:
        """relu(obs W1^T + b1) of the handle's current state into `h1` (bf16), from the resident bits or the packed observation words; under
        twists (`tw`, operands of `_view_kernels`) from the words of every env's view."""
        if tw is not None:
            words = vec.observe_twisted_words(tw, words_buf.shape[1], out=words_buf)
            return embed_words(words, vec.obs_shape_[1], kern[1], kern[2], h1.shape[1], relu=True, out=h1)
        if kern[5]:
            return embed_words(vec.observe_packed(out=words_buf), vec.obs_shape_[1], kern[1], kern[2], h1.shape[1], relu=True, out=h1)
        return embed(vec, kern[1], kern[2], h1.shape[1], relu=True, out=h1)

    def _vec(self, batch: int, track_solution: bool, perms: bool = False) -> VecEnv:
        key = (batch, track_solution, True) if perms else (batch, track_solution)  # add_perms: twists() only, the env steps alike
        if key not in self._vecs:
            for k in [k for k in self._vecs if k[1] == track_solution]:  # one batch size at a time: the handles own device memory
                self._close(self._vecs.pop(k))
            self._vecs[key] = self.env.vec(batch, device=self.device, add_inverts=False, add_perms=perms, track_solution=track_solution)
            self._policy = self._policy.to(device=self._vecs[key].device, dtype=self.dtype)
        return self._vecs[key]

    def _observe(self, vec: VecEnv, tw: Optional[torch.Tensor]) -> torch.Tensor:
        """What the policy reads, in its dtype: the observation, or under twists env e through twist tw[e].  A dtype the library does not
        write (float64) is written as float32 and widened: the entries are 0 and 1."""
        dt = self.dtype if self.dtype in VecEnv._DTYPES else torch.float32
        x = vec.observe_as(dt) if tw is None else vec.observe_twisted(tw, dt)
        return x if dt == self.dtype else x.to(self.dtype)

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

    def _beam_vecs(self, M: int, W: int, perms: bool = False):
        """The beam search's handles: two batches of M * W envs that take turns as source and destination of the per-step copy, and the M
        winners.  All three have the same constructor arguments (the rule of `copy_envs`; no layout choice depends on the batch size)."""
        key = (M, W, True) if perms else (M, W)
        if self._beam is None or self._beam[0] != key:
            if self._beam is not None:
                for v in self._beam[1]:
                    self._close(v)
            mk = lambda batch: self.env.vec(batch, device=self.device, add_inverts=False, add_perms=perms, track_solution=True)  # noqa: E731
            self._beam = (key, (mk(M * W), mk(M * W), mk(M)))
            self._policy = self._policy.to(device=self._beam[1][0].device, dtype=self.dtype)
        return self._beam[1]

    def _views(self, V: int) -> List[int]:
        """Twist index of each of a target's views: view 0 is the untwisted one (-1: no such twist, `observe_twisted` and `untwist_actions`
        pass through), then the env's non-identity twists -- those that move an observation entry -- in `twists()` order; at most V of them."""
        if self._view_list is None:
            probe = self.env.vec(1, device=self.device, add_inverts=False, add_perms=True, track_solution=False)
            obs_perms = probe.twists()[0]
            probe.close()
            self._view_list = [-1] + [t for t, p in enumerate(obs_perms) if p != list(range(len(p)))]
        return self._view_list[:V]

    def _solve_beam(self, states: Sequence[Sequence[int]], W: int, merge: bool = False, twists: Optional[int] = None,
                    fast: bool = False, twist_kernels: bool = False) -> List[Optional[List[int]]]:
        if twists is not None:
            return self._solve_beam_views(states, W, merge, twists, twist_kernels)
        M = len(states)
        cur, oth, win = self._beam_vecs(M, W)
        return self._beam_search(states, 1, None, W, merge, cur, oth, win, fast)

    def _solve_beam_views(self, states, W: int, merge: bool, twists: int, twist_kernels: bool = False) -> List[Optional[List[int]]]:
        """Beam search under V views per target: the groups are the (target, view) pairs, each searched under its own fixed view (and with
        its own merge history); a target's winner is the best result of its V groups, ties to the lowest view."""
        M = len(states)
        views = self._views(int(twists))
        V = len(views)
        cur, oth, win = self._beam_vecs(M * V, W, True)
        tw = torch.tensor(views, dtype=torch.int32, device=cur.device).repeat(M).repeat_interleave(W).contiguous()  # env b: group b // W, view (b // W) % V
        return self._beam_search(states, V, tw, W, merge, cur, oth, win, view_kernels=twist_kernels)

    def _beam_search(self, states, V: int, tw: Optional[torch.Tensor], W: int, merge: bool, cur: VecEnv, oth: VecEnv, win: VecEnv, fast: bool = False,
                     view_kernels: bool = False):
        """`tw` None: the search of `solve(beam_width=W)`.  Else int32 [B]: every env's twist index; there are V consecutive groups per target.
        `fast`: the log-probabilities come from the policy-layer kernels (`tw` is None then); `view_kernels`: the same under `tw`, the first
        layer reading the views as packed words."""
        targets = len(states)
        M = targets * V  # groups
        B, A, dev = cur.batch, cur.num_actions(), cur.device
        kern = None
        if fast or view_kernels:  # the two search handles take turns: each has its own packed first layer (packed through the handle), the rest is shared
            if view_kernels:
                kern = {id(v): self._view_kernels(v) for v in (cur, oth)}
            else:
                kern = {id(v): self._kernels(v) for v in (cur, oth)}
            if any(k is None for k in kern.values()):
                raise ValueError(self._NO_KERNELS)
            pol = self._policy
            h1 = torch.empty((B, pol.embeddings.out_features), dtype=torch.bfloat16, device=dev)
            rows = torch.empty((B, (A + 3) // 4 * 4), dtype=torch.float32, device=dev)[:, :A]  # 16-byte row stride: 16-byte stores
            top = torch.empty(B, dtype=torch.int32, device=dev)  # the kernel's other outputs: not used by the search
            scratch = torch.empty((3, B), dtype=torch.float32, device=dev)
            words_buf = self._words_buf(cur, kern[id(cur)], tw)
        T = int(cur._cfg.max_depth)
        self._load(win, states, V)  # the targets once per group; a group nobody solves keeps its slot, a solved one is overwritten by its winner
        group = torch.arange(M, dtype=torch.int32, device=dev)
        cur.copy_envs(win, group.repeat_interleave(W))
        found = win.success.bool().clone()  # a target that is already solved needs no gates: its winner is the target itself
        best = torch.where(found, 0.0, -float("inf")).to(torch.float32)
        live = torch.zeros((M, W), dtype=torch.uint8, device=dev)
        live[:, 0] = (~found).to(torch.uint8)
        live = live.view(B)
        cum = torch.zeros(B, dtype=torch.float32, device=dev)
        ret = torch.zeros(B, dtype=torch.float32, device=dev)
        nowhere = torch.full((M,), B, dtype=torch.int32, device=dev)  # out of range as a copy source: that entry is skipped
        steps = 0
        if merge:  # the targets' own keys open the histories (one live slot per unsolved target: nothing to drop), so coming back to a target is a revisit
            cap = T * W + 1  # a step adds at most W keys per target: the history of a search never fills
            seen, dropped = beam_seen(M, cap, dev), torch.zeros((M, 2), dtype=torch.int32, device=dev)
            words = cur.observe_packed()
            live = beam_merge(words, cum, live, W, seen, cap)
        for t in range(T):
            if kern is not None:  # first layer from the bits, then middle layer + head + log-softmax in one kernel: no logits in memory
                k = kern[id(cur)]
                logp = mid_head_logp(self._first_layer(cur, k, h1, words_buf, tw), k[3], pol.common.out_features, k[4], A, logp_rows=rows, actions=top,
                                     best_logp=scratch[0], entropy=scratch[1], values=scratch[2])[0]
            else:
                logits = self._policy(self._observe(cur, tw))[0]
                logp = torch.log_softmax(logits.float(), dim=1)
            parent, act, cum, live = beam_select(logp, cum, live, W, A)
            if tw is not None:  # chosen on the view: the real action (a child lives in its parent's group, hence under its view)
                cur.untwist_actions(act, tw, out=act)
            oth.copy_envs(cur, parent)
            oth.step(act)
            ret = ret[parent.long()] + oth.reward  # the return `solve` ranks by: the parent's plus this step's reward
            solved = (live.bool() & oth.success.bool()).view(M, W)
            live = live & (1 - oth.done)
            score = torch.where(solved, ret.view(M, W), torch.full((M, W), -float("inf"), device=dev))
            j = score.argmax(dim=1)  # the first of equal maxima: the lowest slot
            val = score.gather(1, j.view(M, 1)).view(M)
            better = val > best
            win.copy_envs(oth, torch.where(better, group * W + j.to(torch.int32), nowhere))
            best = torch.where(better, val, best)
            found |= better
            if merge:  # beams that ended (the step's results among them) have left `live`: they are neither merged nor recorded
                live = beam_merge(oth.observe_packed(out=words), cum, live, W, seen, cap, dropped=dropped)
            cur, oth = oth, cur
            steps = t + 1
            if t % 8 == 7 and not bool(live.any()):
                break
        for v in (cur, oth, win):
            v.sync()
        sols, lens = win.solutions(T + 64)  # the log holds an episode's steps, PauliEnv: plus one entry per rotation (<= 32)
        if tw is not None:  # per target the best of its V groups; argmax takes the first of equal maxima: the lowest view
            pick = (torch.arange(targets, device=dev) * V + best.view(targets, V).argmax(dim=1)).cpu().numpy()
            ok = found.cpu().numpy()[pick]
            sols, lens = sols[pick], lens[pick]
        else:
            ok = found.cpu().numpy()
        out = [[int(x) for x in sols[m, : lens[m]]] if ok[m] else None for m in range(targets)]
        gates = [sum(1 for x in s if x < ROTATION_MARKER) for s in out if s is not None]
        self.last_stats = {"beam_width": W, "targets": targets, "steps": steps, "solved": int(ok.sum()), "mean_gates": float(np.mean(gates)) if gates else 0.0}
        if kern is not None:
            self.last_stats["kernels"] = True
        if tw is not None:
            self.last_stats["views"] = V
        if merge:
            n_rev, n_dup = (int(x) for x in dropped.sum(dim=0).cpu())
            self.last_stats.update(merged=n_dup, revisits=n_rev)
        return out

    @torch.no_grad()
    def solve(self, states: Sequence[Sequence[int]], deterministic: bool = False, num_searches: int = 100, fast: Optional[bool] = None,
              beam_width: Optional[int] = None, merge_duplicates: bool = False, twists: Optional[int] = None,
              twist_kernels: bool = False) -> List[Optional[List[int]]]:
        """One entry per target: `Env::solution()` of the best successful search, or None (rl/synthesis.py:121-126).
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
        shape, or an observation of more than 64 columns."""
        M = len(states)
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
        if M == 0:
            return []
        if beam_width is not None:
            if int(beam_width) < 1:
                raise ValueError("beam_width must be at least 1")
            if merge_duplicates and self.env.env_kind == "pauli":
                raise ValueError("merge_duplicates: a PauliGym observation does not determine its state (rotations beyond the observed columns, DAG order)")
            return self._solve_beam(states, int(beam_width), bool(merge_duplicates), twists, fast is True, bool(twist_kernels))
        if merge_duplicates:
            raise ValueError("merge_duplicates needs beam_width")
        S = 1 if deterministic else max(1, int(num_searches))  # greedy episodes are all alike
        tw = None
        if twists is not None:
            views = self._views(int(twists))
            if deterministic:
                S = len(views)  # ... but for the view they are seen through
            vec = self._vec(M * S, False, True)
            tw = torch.tensor([views[s % len(views)] for s in range(S)], dtype=torch.int32, device=vec.device).repeat(M).contiguous()  # env m * S + s: view s mod V
        else:
            vec = self._vec(M * S, False)
        B, A, dev = vec.batch, vec.num_actions(), vec.device
        self._load(vec, states, S)
        T = int(vec._cfg.max_depth)
        actions = torch.empty((T, B), dtype=torch.int32, device=dev)
        finished = vec.success.bool().clone()  # a target that is already solved needs no gates
        solved_at = torch.where(finished, 0, -1).to(torch.int32)
        ret = torch.zeros(B, dtype=torch.float32, device=dev)
        parked = torch.full((B,), A, dtype=torch.int32, device=dev)  # out of range: no gate (clifford.rs:324)
        steps = 0
        kern = None
        if twist_kernels:
            kern = self._view_kernels(vec)
        elif tw is None and fast is not False and (fast or (not deterministic and B >= 4096)):  # greedy: on request only
            kern = self._kernels(vec)
            if fast and kern is None:
                raise ValueError(self._NO_KERNELS)
        if kern is not None:
            pol = self._policy
            h1 = torch.empty((B, pol.embeddings.out_features), dtype=torch.bfloat16, device=dev)
            act = torch.empty(B, dtype=torch.int32, device=dev)
            scratch = torch.empty((3, B), dtype=torch.float32, device=dev)
            words_buf = self._words_buf(vec, kern, tw)
        self.last_stats = {"kernels": kern is not None}
        for t in range(T):
            if kern is not None:
                self._first_layer(vec, kern, h1, words_buf, tw)
                if deterministic:  # the arg-max alone: no row is written
                    mid_head_logp(h1, kern[3], pol.common.out_features, kern[4], A, want_rows=False, actions=act, best_logp=scratch[0], entropy=scratch[1],
                                  values=scratch[2])
                else:
                    mid_head_sample(h1, kern[3], pol.common.out_features, kern[4], A, self.seed, t, actions=act, logp=scratch[0], entropy=scratch[1],
                                    values=scratch[2])
            else:
                x = self._observe(vec, tw)
                logits = self._policy(x)[0]
                if deterministic:
                    act = logits.argmax(dim=1).to(torch.int32)
                else:
                    act = sample_actions(logits.contiguous(), self.seed, t)[0].to(torch.int32)
            if tw is not None:  # chosen on the view: the real action
                vec.untwist_actions(act, tw, out=act)
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
        score = torch.where(ok, ret.view(M, S), torch.full((M, S), -float("inf"), device=dev))
        best = score.argmax(dim=1)
        idx = torch.arange(M, device=dev) * S + best
        lengths = solved_at[idx].cpu().numpy()
        found = ok.any(dim=1).cpu().numpy()
        win = actions[:steps, idx].t().contiguous()  # [M, steps]
        self.last_stats.update({"targets": M, "searches": S, "steps": steps, "solved": int(found.sum()),
                           "searches_solved": float(ok.float().mean()), "mean_gates": float(lengths[found].mean()) if found.any() else 0.0})
        if tw is not None:
            self.last_stats["views"] = len(views)
        if vec.env_kind != "pauli":
            w = win.cpu().numpy()
            return [w[m, : lengths[m]].tolist() if found[m] else None for m in range(M)]
        # PauliEnv: replay the winners with the solution log on; padding entries (no gate, no marker) are dropped
        rep = self._vec(M, True)
        self._load(rep, states, 1)
        keep = torch.arange(steps, device=dev).view(1, -1) < solved_at[idx].view(-1, 1)
        rep.rollout(torch.where(keep, win, torch.full_like(win, A)).t().contiguous())
        rep.sync()
        out: List[Optional[List[int]]] = []
        for m in range(M):
            out.append([v for v in rep.solution(m) if v >= ROTATION_MARKER or v < A] if found[m] else None)
        return out

    def synth(self, inputs, deterministic: bool = False, num_searches: int = 100, beam_width: Optional[int] = None, merge_duplicates: bool = False,
              twists: Optional[int] = None, fast: Optional[bool] = None, twist_kernels: bool = False):
        """`RLSynthesis.synth` over a list of inputs: circuits (needs qiskit) or None where no search succeeded."""
        sols = self.solve([self.env.get_state(x) for x in inputs], deterministic, num_searches, fast=fast, beam_width=beam_width,
                          merge_duplicates=merge_duplicates, twists=twists, twist_kernels=twist_kernels)
        return [self.env.build_circuit_from_solution(s, x) if s is not None else None for s, x in zip(sols, inputs)]

    def gate_lists(self, solutions):
        """Solutions as `(name, qubits)` lists (rotation markers of PauliGym solutions are skipped)."""
        gs = self.env.config["gateset"]
        return [None if s is None else [(gs[a][0], tuple(gs[a][1])) for a in s if a < ROTATION_MARKER] for s in solutions]
