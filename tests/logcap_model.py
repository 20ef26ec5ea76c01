"""The solution log's contract at its edges, restated: what a logged action reads back as, and what a log of `cap` entries holds
after more than `cap` pushes.  Imports nothing from the library or the oracle; drives tests/envmodel.Model (and, for the values only,
tests/paulimodel).

The contract (include/qgym.h, "Solution log"):
  * CliffordEnv and LinearFunctionEnv push every stepped action, valid or not (clifford.rs:334-340, linear_function.rs:315-321), into
    `solution`, or into `solution_inv` while the env is inverted; PermutationEnv pushes in-range actions only (permutation.rs:210-216);
    PauliEnv pushes in-range actions and the rotations they release (pauli.rs:612-626).
  * An entry is exact up to 2^31 - 2.  Anything else an action can be -- larger, or negative, which `as usize` turns into a huge
    number -- reads back as 2^64 - 1.  Only CliffordEnv and LinearFunctionEnv ever log such a value.
  * The log holds `cap` pushes of an episode.  A push beyond them is dropped and sets QG_FAULT_SOLUTION_OVERFLOW (8) in the env's
    status word; the entries already logged stay as they are.  Env::solution is `solution ++ reverse(solution_inv)` of what was kept."""
from __future__ import annotations

import numpy as np

LAST_EXACT = 2**31 - 2  # the documented bound, not the code's constant
SATURATED = 2**64 - 1
OVERFLOW_BIT = 8  # QG_FAULT_SOLUTION_OVERFLOW
LOGS_EVERY_ACTION = ("clifford", "linear_function")
KINDS = LOGS_EVERY_ACTION + ("permutation", "pauli")


def reported(value, kind):
    """What Env::solution returns for the logged action `value` (any Python int: an int64 action, or what `as usize` made of it)."""
    assert kind in KINDS
    value = int(value)
    if kind in LOGS_EVERY_ACTION:
        return value if 0 <= value <= LAST_EXACT else SATURATED
    return value  # PermutationEnv and PauliEnv log in-range actions only: always the value itself


class PushRecorder:
    """Every push of the current episode, per env, in order: (action, pushed into solution_inv).  Call `note` BEFORE each model step
    (the frame an action is logged in is the one the env is in when it is stepped, before that step's coin), `clear` where the model
    starts a new episode."""

    def __init__(self, kind, batch, num_actions):
        assert kind in ("clifford", "linear_function", "permutation")
        self.kind, self.B, self.A = kind, int(batch), int(num_actions)
        self.pushes = [[] for _ in range(self.B)]

    def note(self, actions, inverted=None):
        actions = np.asarray(actions, dtype=np.int64).reshape(self.B)
        inverted = np.zeros(self.B, bool) if inverted is None else np.asarray(inverted, bool).reshape(self.B)
        for b in range(self.B):
            a = int(actions[b])
            if self.kind in LOGS_EVERY_ACTION or 0 <= a < self.A:
                self.pushes[b].append((a, bool(inverted[b])))

    def note_model(self, model, actions):
        """`note` with the frame read from a tests/envmodel.Model about to step `actions`."""
        self.note(actions, model.inverted)

    def clear(self, mask=None):
        for b in range(self.B) if mask is None else np.flatnonzero(np.asarray(mask, bool)):
            self.pushes[b] = []

    def counts(self):
        return np.array([len(p) for p in self.pushes], np.int64)

    def overflowed(self, cap):
        """[B] bool: the envs that pushed more than `cap` times this episode."""
        return self.counts() > int(cap)

    def expected_log(self, cap):
        """Env::solution of every env from a log of `cap` entries: the first `cap` pushes, as solution ++ reverse(solution_inv)."""
        out = []
        for pushes in self.pushes:
            kept = pushes[: int(cap)]
            front = [reported(a, self.kind) for a, inv in kept if not inv]
            back = [reported(a, self.kind) for a, inv in kept if inv]
            out.append(front + back[::-1])
        return out

    def expected_faults(self, cap):
        return np.where(self.overflowed(cap), OVERFLOW_BIT, 0).astype(np.uint32)
