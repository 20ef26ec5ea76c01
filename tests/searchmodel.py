"""CPU restatement of the sampled and the greedy search of `BatchedSynthesis.solve(num_searches=S)` / `solve(deterministic=True)`, alone
or under `twists=V`: numpy for the draws (tests/collect_ref.py) and the f32 returns, `OracleEnv.clone` for the envs, the oracle's
symmetry code for the views.  TEST INFRASTRUCTURE ONLY; it shares no code with qiskit_gym_amd.

The rules.
  layout     M targets, S searches each: env e = m * S + s is search s of target m, a clone of the target.  S is max(1, num_searches) for a
             sampled search, 1 for the greedy one, V for the greedy one under V views.
  views      Under views search s sees view s mod V for its whole episode.  View 0 is the untwisted observation; views 1.. are the env's
             twists that move an observation entry, in `twists()` order.  The policy reads view(obs)[i] = obs[obs_perm[i]] (the gather of
             tests/test_twist_views.py); an action a chosen on a view is the real action act_perm[a].
  draws      The draw of step t for env e is the winner of the exponential race `race_keys(logits[e], u[e])` with
             u = `sample_uniforms(seed, B, t, A)`: counter t, env index e, env_base 0.  The greedy step takes the arg-max of the row.
  step       A live env takes its real action.  A finished env (final after one of its steps, or solved on arrival) gets no gate from then
             on and does not move.  An env's return is the f32 sum, in step order, of the rewards of the steps it was live for; its
             `solved_at` is t + 1 at the step that reached success, 0 for a target solved on arrival, -1 while unsolved.
  end        The loop ends after the first step t with t % 8 == 7 at which every env is finished, else after `max_depth` steps; the number
             of steps made is `steps`.
  winner     Per target the successful search (solved_at >= 0) of the greatest f32 return, the lowest s among equals.  The answer is its
             real actions up to `solved_at` -- for a PauliEnv the oracle's solution log (gates and rotation markers) of those gates replayed
             from the target --, or None where no search succeeded.
  stats      steps; solved = targets with an answer; searches_solved = successful envs / B; mean_gates = mean `solved_at` of the winners
             (0.0 without any).

The model is driven step by step with the numbers a device used: `step(logits, chosen, stepped)` takes the f32 rows the search drew from,
the actions the device chose on the views and / or the actions it handed the env.  At every live draw the model computes its own winner in
f64.  Where the key margin is above `threshold`, the device's action must be that winner; where it is not, the device's action must still
have a key within `threshold` of the smallest, and the draw is counted as unclear.  Greedy: the device's action must be an arg-max of the
row, the lowest such index under `lowest_on_ties`.  Either way the env then takes the device's action, so everything after the draw is
compared exactly.  A device that is wrong raises AssertionError.  `choose(logits)` is the model's own choice: `step(logits, choose(logits))`
is the model alone.
"""
from __future__ import annotations

from typing import List, Optional, Sequence, Tuple

import numpy as np

from collect_ref import race_keys, race_winner, sample_uniforms

MARKER = 0x80000000  # solution-log entries from here on are rotation markers, not gates


class SearchModel:
    def __init__(self, targets: Sequence, S: int, A: int, max_depth: int, seed: int = 0, greedy: bool = False,
                 views: Optional[Sequence[Tuple[Sequence[int], Sequence[int]]]] = None, threshold: float = 1e-4, lowest_on_ties: bool = True):
        """targets: M oracle envs (track_solution on), each holding its target; they are cloned, not stepped.  views: None, or the
        (obs_perm, act_perm) of every view, the identity first (`views_of`)."""
        self.targets = list(targets)
        self.M, self.S, self.A, self.T = len(self.targets), int(S), int(A), int(max_depth)
        self.B = self.M * self.S
        self.seed, self.greedy, self.threshold, self.lowest_on_ties = int(seed), bool(greedy), float(threshold), bool(lowest_on_ties)
        self.views = None if views is None else [(np.asarray(o, dtype=np.int64), np.asarray(a, dtype=np.int64)) for o, a in views]
        self.V = 1 if views is None else len(self.views)
        self.envs = [self.targets[e // self.S].clone() for e in range(self.B)]
        self.view = np.array([self.view_of(e % self.S) for e in range(self.B)], dtype=np.int64)
        self.finished = np.array([env.success() for env in self.envs], dtype=bool)
        self.solved_at = np.where(self.finished, 0, -1).astype(np.int64)
        self.ret = np.zeros(self.B, dtype=np.float32)
        self.actions: List[List[int]] = [[] for _ in range(self.B)]  # the real actions of the steps an env was live for
        self.t = 0  # steps made
        self.ended = self.T == 0
        self.live_draws = self.unclear = 0
        self.all_finished_at = 0 if self.finished.all() else None  # the number of steps after which every env was finished, once it is so

    # ---- the rules a wrong search would break: one method each ------------------------------------------------------------------------
    def view_of(self, s: int) -> int:
        return s % self.V

    def counter(self, t: int) -> int:
        return t

    def adds_reward(self, was_live: bool) -> bool:
        return was_live

    def pick(self, ok: np.ndarray, ret: np.ndarray) -> Optional[int]:
        """The winner among a target's S searches: the greatest return of the successful ones, the lowest s among equals."""
        best = None
        for s in range(len(ok)):
            if ok[s] and (best is None or ret[s] > ret[best]):
                best = s
        return best

    # ---- one step ----------------------------------------------------------------------------------------------------------------------
    def observations(self) -> np.ndarray:
        """What the policy reads now, [B, rows * cols] of 0 / 1: every env's dense observation through its view, finished envs included."""
        out = []
        for e, env in enumerate(self.envs):
            obs = env.dense_obs().reshape(-1)
            out.append(obs if self.views is None else obs[self.views[self.view[e]][0]])
        return np.stack(out)

    def _keys(self, logits: np.ndarray) -> np.ndarray:
        u = sample_uniforms(self.seed, self.B, self.counter(self.t), self.A)
        return race_keys(np.asarray(logits, dtype=np.float32)[:, : self.A], u)

    def choose(self, logits: np.ndarray) -> np.ndarray:
        """The model's own choice on the views, int64 [B] (A for a finished env)."""
        logits = np.asarray(logits, dtype=np.float32)[:, : self.A]
        act = logits.argmax(axis=1) if self.greedy else race_winner(self._keys(logits))[0]
        return np.where(self.finished, self.A, act).astype(np.int64)

    def _check_draw(self, e: int, a: int, row: np.ndarray, keys: Optional[np.ndarray]):
        assert 0 <= a < self.A, f"step {self.t} env {e}: a live env was given {a}, which is no action"
        if self.greedy:
            top = row.max()
            assert row[a] == top, f"step {self.t} env {e}: action {a} (logit {row[a]!r}) is no arg-max (logit {top!r} at {int(row.argmax())})"
            if self.lowest_on_ties:
                assert a == int(row.argmax()), f"step {self.t} env {e}: action {a}, but the lowest arg-max is {int(row.argmax())}"
            return
        k = keys[e]
        want, margin = race_winner(k[None, :])
        want, margin = int(want[0]), float(margin[0])
        if margin > self.threshold:
            assert a == want, f"step {self.t} env {e}: drew {a}, the race's winner is {want} by a key margin of {margin:.3e}"
        else:
            self.unclear += 1
            assert k[a] - k.min() <= self.threshold, f"step {self.t} env {e}: drew {a}, whose key is {k[a] - k.min():.3e} above the smallest"

    def step(self, logits: np.ndarray, chosen: Optional[np.ndarray] = None, stepped: Optional[np.ndarray] = None):
        """One step of the search.  logits: [B, >= A] f32, the rows the device drew from (any per-row shift of them).  chosen: the actions
        it chose on the views; stepped: the actions it handed the env; at least one of the two."""
        assert not self.ended, "the search has ended"
        assert chosen is not None or stepped is not None
        logits = np.asarray(logits, dtype=np.float32)[:, : self.A]
        assert logits.shape == (self.B, self.A)
        keys = None if self.greedy else self._keys(logits)
        t = self.t
        for e, env in enumerate(self.envs):
            was_live = not self.finished[e]
            act_perm = None if self.views is None else self.views[self.view[e]][1]
            if not was_live:
                if stepped is not None:
                    assert not 0 <= int(stepped[e]) < self.A, f"step {t} env {e}: a finished env was given gate {int(stepped[e])}"
                if self.adds_reward(was_live):  # no rule of the search: what a search that goes on adding would read
                    env.step(self.A)
                    self.ret[e] = np.float32(self.ret[e] + np.float32(env.reward()))
                continue
            if chosen is not None:
                a = int(chosen[e])
            else:  # the action on the view that gives the real one
                r = int(stepped[e])
                assert 0 <= r < self.A, f"step {t} env {e}: a live env was given {r}, which is no action"
                a = r if act_perm is None else int(np.nonzero(act_perm == r)[0][0])
            self.live_draws += 1
            self._check_draw(e, a, logits[e], keys)
            real = a if act_perm is None else int(act_perm[a])
            if stepped is not None:
                assert int(stepped[e]) == real, f"step {t} env {e}: view {self.view[e]} chose {a}, the env was given {int(stepped[e])} instead of {real}"
            env.step(real)
            self.actions[e].append(real)
            if self.adds_reward(was_live):
                self.ret[e] = np.float32(self.ret[e] + np.float32(env.reward()))
            if env.success():
                self.solved_at[e] = t + 1
            if env.is_final():
                self.finished[e] = True
        self.t = t + 1
        if self.all_finished_at is None and self.finished.all():
            self.all_finished_at = self.t
        if (t % 8 == 7 and self.finished.all()) or self.t == self.T:
            self.ended = True

    # ---- the answer --------------------------------------------------------------------------------------------------------------------
    def winners(self) -> List[Optional[int]]:
        ok, ret = (self.solved_at >= 0).reshape(self.M, self.S), self.ret.reshape(self.M, self.S)
        return [self.pick(ok[m], ret[m]) for m in range(self.M)]

    def result(self):
        """(solutions, stats) once the search has ended."""
        assert self.ended, "the search is still running"
        sols: List[Optional[List[int]]] = []
        lengths = []
        for m, s in enumerate(self.winners()):
            if s is None:
                sols.append(None)
                continue
            e = m * self.S + s
            gates = self.actions[e][: self.solved_at[e]]
            assert len(gates) == self.solved_at[e]
            lengths.append(len(gates))
            if self.targets[m].kind == "pauli":
                env = self.targets[m].clone()
                for g in gates:
                    env.step(g)
                sols.append([int(x) for x in env.solution()])
            else:
                sols.append([int(g) for g in gates])
        stats = {"steps": self.t, "solved": len(lengths), "searches_solved": int((self.solved_at >= 0).sum()) / self.B,
                 "mean_gates": float(np.mean(lengths)) if lengths else 0.0}
        return sols, stats


def views_of(env) -> List[Tuple[List[int], List[int]]]:
    """(obs_perm, act_perm) of every view of an oracle env built with add_perms on: the identity, then the twists that move an observation
    entry, in `twists()` order."""
    obs_perms, act_perms = env.twists()
    ident = list(range(len(obs_perms[0])))
    return [(ident, list(range(env.num_actions())))] + [(o, a) for o, a in zip(obs_perms, act_perms) if o != ident]


def run_alone(model: SearchModel, logits_of):
    """The model as its own device: `logits_of(obs [B, n] float32) -> [B, A]` until the search ends.  Returns `model.result()`."""
    while not model.ended:
        logits = np.asarray(logits_of(model.observations().astype(np.float32)), dtype=np.float32)
        model.step(logits, model.choose(logits))
    return model.result()
