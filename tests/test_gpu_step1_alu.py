"""The arithmetic of the one-step kernel of the TILE layout (qm_step1_mask_body) on lane masks: the gate word decoded once into 0 / -1 words, every
select and merge one bit-select instruction, every term of the 4x4 GF(2) map one a ^ (b & c), `bad` updated by shifts, no branch around "no gate".
Every case is bit-exact against the CPU oracle: reward bit patterns, success, is_final, depth, final state and observation.  Shapes are the
smallest at which that arithmetic can go wrong: every gate of the line gateset on every env (so every qubit parity, same-group and cross-group
pairs), N == NXP and N < NXP, both row layouts, a ragged third wave."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

from util import f32_bits, line_gateset, make_pair  # noqa: E402

PLAIN = dict(add_inverts=False, add_perms=False, track_solution=False)
B = 130  # two full waves and a ragged third


def _dev(a, dtype=None):
    return torch.as_tensor(np.ascontiguousarray(a), device="cuda").to(dtype or torch.int32)


def _per_env(kind, n):
    return {"clifford": 4 * n * n, "linear_function": n * n}[kind]


def _scramble(ov, gv, rng, n_draws, A):
    draws = rng.integers(0, A, size=(n_draws, gv.batch))
    ov.proto.difficulty = n_draws
    for i in range(ov.batch):
        ov.env(i).difficulty = n_draws
    gv.difficulty = n_draws
    ov.reset_with(draws)
    gv.reset_with(_dev(draws))


def _step_both(ov, gv, acts, dtype=None, oracle_acts=None, label=""):
    r_o, s_o, f_o, d_o = ov.step(np.asarray(acts if oracle_acts is None else oracle_acts, dtype=np.int32))
    gv.step(_dev(acts, dtype))
    gv.sync()
    np.testing.assert_array_equal(f32_bits(gv.reward.cpu().numpy()), f32_bits(r_o), err_msg=f"reward {label}")
    np.testing.assert_array_equal(gv.success.cpu().numpy(), s_o, err_msg=f"success {label}")
    np.testing.assert_array_equal(gv.done.cpu().numpy(), f_o, err_msg=f"is_final {label}")
    np.testing.assert_array_equal(gv.depth.cpu().numpy(), d_o, err_msg=f"depth {label}")
    return r_o, s_o, f_o, d_o


def _same_state(ov, gv, kind, n, label):
    np.testing.assert_array_equal(gv.get_state("i64").cpu().numpy(), ov.get_state(_per_env(kind, n)), err_msg=f"state {label}")
    np.testing.assert_array_equal(gv.observe().cpu().numpy().reshape(gv.batch, -1), ov.observe_dense(), err_msg=f"obs {label}")


def _every_gate_on_every_env(ov, gv, A, label, every=None, dtype=None, spoil=None):
    """Env e takes action (t + e) % A at step t: every env applies every action once, neighbouring lanes never hold the same gate.
    `every(t)` runs after each step; `spoil(t, acts)` may replace actions (returns the oracle's view of them)."""
    env = np.arange(gv.batch)
    for t in range(A):
        acts = (t + env) % A
        oracle_acts = None
        if spoil is not None:
            acts, oracle_acts = spoil(t, acts)
        _step_both(ov, gv, acts, dtype, oracle_acts, label=f"{label} t={t}")
        if every is not None:
            every(t)


# ---- every gate, every qubit parity, every group relation ----------------------------------------------------------------------------
@pytest.mark.parametrize("kind,n", [("clifford", 16), ("clifford", 13), ("clifford", 3), ("linear_function", 12), ("linear_function", 32)])
def test_every_gate_on_every_env(kind, n):
    gs = line_gateset(kind, n)
    A = len(gs)
    ov, gv = make_pair(kind, n, gs, B, max_depth=A + 8, **PLAIN)
    _scramble(ov, gv, np.random.default_rng(1000 + n), 3 * n, A)
    _every_gate_on_every_env(ov, gv, A, f"{kind}{n}")
    _same_state(ov, gv, kind, n, f"{kind}{n}")


# ---- `bad` in both directions --------------------------------------------------------------------------------------------------------
def _action(gs, name, qubits):
    return gs.index((name, tuple(qubits)))


@pytest.mark.parametrize("kind,n", [("clifford", 16), ("clifford", 13), ("linear_function", 12)])
def test_gate_then_inverse_from_the_identity(kind, n):
    """From the identity (a scramble of zero draws) a gate, then its inverse: success goes 1 -> 0 -> 1.  Env e takes pair e % len(pairs), so one
    wave holds all of them: both qubit parities, a same-group and a cross-group pair of qubits."""
    gs = line_gateset(kind, n)
    A = len(gs)
    if kind == "clifford":  # groups of two qubits: (2, 3) share one, (3, 4) do not
        singles = [("H", "H"), ("S", "Sdg"), ("Sdg", "S"), ("SX", "SXdg"), ("SXdg", "SX")]
        pairs = [(_action(gs, a, (q,)), _action(gs, b, (q,))) for a, b in singles for q in (4, 7, n - 1)]
        doubles, edges = ["CX", "CZ", "SWAP"], [(2, 3), (3, 2), (3, 4), (4, 3), (n - 2, n - 1)]
    else:  # groups of four rows: (4, 5) share one, (3, 4) do not
        pairs, doubles, edges = [], ["CX", "SWAP"], [(4, 5), (5, 4), (3, 4), (4, 3), (n - 2, n - 1)]
    pairs += [(_action(gs, g, e), _action(gs, g, e)) for g in doubles for e in edges]
    first = np.array([pairs[e % len(pairs)][0] for e in range(B)])
    second = np.array([pairs[e % len(pairs)][1] for e in range(B)])
    ov, gv = make_pair(kind, n, gs, B, max_depth=8, **PLAIN)
    _scramble(ov, gv, np.random.default_rng(0), 0, A)
    _, s1, _, _ = _step_both(ov, gv, first, label=f"{kind}{n} gate")
    assert not s1.any(), "every gate of the list leaves the identity"
    _same_state(ov, gv, kind, n, f"{kind}{n} gate")
    _, s2, _, _ = _step_both(ov, gv, second, label=f"{kind}{n} inverse")
    assert s2.all(), "and its inverse returns to it"
    _same_state(ov, gv, kind, n, f"{kind}{n} inverse")
    _step_both(ov, gv, first, label=f"{kind}{n} gate again")
    _same_state(ov, gv, kind, n, f"{kind}{n} gate again")


# ---- out-of-range actions in waves that also hold valid ones -------------------------------------------------------------------------
@pytest.mark.parametrize("adt", ["int32", "int64"])
def test_out_of_range_actions_between_valid_ones(adt):
    kind, n = "clifford", 13
    gs = line_gateset(kind, n)
    A = len(gs)
    ov, gv = make_pair(kind, n, gs, B, max_depth=A + 8, **PLAIN)
    _scramble(ov, gv, np.random.default_rng(55), 3 * n, A)
    edges = [A + 3, -1] + ([2**32 + 5] if adt == "int64" else [])  # int64: the low half alone is in range

    def spoil(t, acts):
        acts = acts.astype(np.int64)
        seen = acts.copy()
        for k, e in enumerate(edges):
            acts[(t + k) % 7::7] = e
            seen[(t + k) % 7::7] = -1  # to an env without a solution log every out-of-range action is the same no-op
        return acts, seen

    _every_gate_on_every_env(ov, gv, A, f"{kind}{n} {adt}", dtype=getattr(torch, adt), spoil=spoil)
    _same_state(ov, gv, kind, n, f"{kind}{n} {adt}")


# ---- the instantiations with extra stores --------------------------------------------------------------------------------------------
def test_tracked_dense_observation():
    kind, n = "clifford", 16
    gs = line_gateset(kind, n)
    A = len(gs)
    ov, gv = make_pair(kind, n, gs, B, max_depth=A + 8, **PLAIN)
    _scramble(ov, gv, np.random.default_rng(66), 3 * n, A)
    tracked = gv.track_dense()

    def every(t):
        assert torch.equal(tracked, gv.observe()), t

    _every_gate_on_every_env(ov, gv, A, "dense", every=every)
    np.testing.assert_array_equal(tracked.cpu().numpy().reshape(B, -1), ov.observe_dense())
    _same_state(ov, gv, kind, n, "dense")


def test_solution_log():
    kind, n = "clifford", 16
    gs = line_gateset(kind, n)
    A = len(gs)
    ov, gv = make_pair(kind, n, gs, B, max_depth=A + 8, **dict(PLAIN, track_solution=True))
    _scramble(ov, gv, np.random.default_rng(67), 3 * n, A)
    _every_gate_on_every_env(ov, gv, A, "log")
    _same_state(ov, gv, kind, n, "log")
    for e in (0, 1, 63, 64, B - 1):
        assert gv.solution(e) == ov.env(e).solution(), e


def test_done_mask_form():
    """A handle on which reset_done is in use: its steps record the envs that finish, and the reset that follows re-scrambles exactly those."""
    kind, n, diff = "clifford", 16, 4
    gs = line_gateset(kind, n)
    A = len(gs)
    ov, gv = make_pair(kind, n, gs, B, max_depth=3, difficulty=diff, **PLAIN)
    _scramble(ov, gv, np.random.default_rng(68), diff, A)
    env, resets = np.arange(B), 0
    for t in range(A):
        _, _, fin, _ = _step_both(ov, gv, (t + env) % A, label=f"list t={t}")
        done = fin.astype(bool)
        if done.any():
            gv.reset_done(900 + t)
            ov.reset_seeded(900 + t, mask=done)
            resets += int(done.sum())
            if t % 16 == 0:
                _same_state(ov, gv, kind, n, f"list after reset_done t={t}")
    _same_state(ov, gv, kind, n, "list")
    assert resets > B
