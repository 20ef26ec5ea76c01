"""tests/envmodel.py proved on the CPU: against the explicit unitaries at n <= 3, against the reference's recorded transcripts and
solutions, and against the CPU oracle at every size the library supports (the one place the oracle meets the model)."""
import json
import os

import numpy as np
import pytest

from envmodel import Model, metrics_of, decomposition_table
from test_physics import clifford_state, unitary
from util import f32_bits, grid_gateset, line_gateset


def _names(gs):
    return [(a.lower(), tuple(b)) for a, b in gs]


# ---- physics, n <= 3 ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", [2, 3])
def test_clifford_model_states_are_the_unitaries_tableaus(n):
    rng = np.random.default_rng(n)
    gs = line_gateset("clifford", n) + [("CX", (0, 0)), ("SWAP", (n - 1, n - 1))]
    names = _names(gs)
    B, T = 120, 14
    circs = rng.integers(0, len(gs), size=(B, T))
    m = Model("clifford", n, gs, B)
    got = m.wire(m.state_of_circuit(circs))
    for b in range(B):
        # a gate on one qubit twice is the reference's no-op (clifford.rs:121,131,140)
        circ = [names[a] for a in circs[b] if len(set(names[a][1])) == len(names[a][1])]
        assert got[b].tolist() == clifford_state(circ, n), circ


def lf_state(circ, n):
    """LinearFunction(Clifford(circ).adjoint()).linear from the unitary: column j is the basis state U^dagger |e_j>."""
    v = unitary(circ, n).conj().T
    a = np.zeros((n, n), np.int64)
    for j in range(n):
        out = int(np.flatnonzero(np.abs(v[:, 1 << j]) > 0.5)[0])
        a[:, j] = [(out >> i) & 1 for i in range(n)]
    return a.flatten().tolist()


def test_linear_function_model_states_are_the_unitaries_linear_maps():
    rng = np.random.default_rng(2)
    for n in (2, 3):
        gs = line_gateset("linear_function", n)
        names = _names(gs)
        circs = rng.integers(0, len(gs), size=(100, 12))
        m = Model("linear_function", n, gs, 100)
        got = m.wire(m.state_of_circuit(circs))
        for b in range(100):
            assert got[b].tolist() == lf_state([names[a] for a in circs[b]], n)


def test_replaying_the_target_solves_it_and_logs_it():
    rng = np.random.default_rng(3)
    for kind, n in (("clifford", 3), ("linear_function", 5), ("permutation", 9)):
        gs = grid_gateset(kind, 3, 3) if kind == "permutation" else line_gateset(kind, n)
        B, T = 64, 9
        circs = rng.integers(0, len(gs), size=(B, T))
        m = Model(kind, n, gs, B, track_solution=True)
        m.set_state(m.wire(m.state_of_circuit(circs)))
        for t in range(T):
            m.step(circs[:, t])
        assert m.success.all()
        assert m.solutions() == circs.tolist()


def test_gf2_inverse_reports_singular_states():
    m = Model("clifford", 2, line_gateset("clifford", 2), 3)
    st = m.identity(3)
    st[1, 2] = st[1, 0]  # row 2 = row 0: singular
    st[2, 0, 1] = 1      # invertible, not symplectic
    inv, ok = m.inverse(st)
    assert ok.tolist() == [True, False, True]
    assert (m.matmul(inv[[0, 2]], st[[0, 2]]) == m.identity(2)).all()


def test_metrics_are_longest_paths():
    gs = [("H", (0,)), ("CX", (0, 1)), ("CZ", (0, 1)), ("SWAP", (1, 2)), ("CZ", (2, 2)), ("CX", (1, 1)), ("S", (2,))]
    tab = decomposition_table(_names(gs), 3)
    # CZ(0, 1): H(1) CX(0, 1) H(1) -> 3 layers, 1 CX layer; CZ(2, 2): two one-qubit gates on 2; CX(1, 1): nothing
    assert metrics_of([[2]], tab, 3).tolist() == [[1, 1, 3, 3]]
    assert metrics_of([[4, 5]], tab, 3).tolist() == [[0, 0, 2, 2]]
    # H(0) S(2) | SWAP(1, 2) = 3 CX | CX(0, 1): CX chain 1-2, 2-1, 1-2, 0-1 -> 4 CX layers; 1q + 4 -> 5 layers
    assert metrics_of([[0, 6, 3, 1, -1]], tab, 3).tolist() == [[4, 4, 5, 6]]


# ---- the reference's recorded data --------------------------------------------------------------------------------------
def test_model_replays_the_linear_function_transcripts(golden_dir):
    d = json.load(open(os.path.join(golden_dir, "lf_line3_transcripts.json")))
    for seq in d["sequences"]:
        m = Model("linear_function", d["num_qubits"], d["gateset"], 1)
        m.set_state(np.array(d["start_state"]).reshape(1, -1))
        for a, want, fin in zip(seq["actions"], seq["states"], seq["is_final"]):
            assert not m.is_final()[0]
            m.step([a])
            assert m.observe().reshape(np.shape(want)).tolist() == want, (seq["source"], a)
            assert m.is_final()[0] == fin


@pytest.mark.parametrize("key", ["permutation_swap_0_8", "linear_function_cx_0_4", "clifford_h_2"])
def test_model_replays_the_notebook_solutions(golden_dir, key):
    rec = json.load(open(os.path.join(golden_dir, "notebook_solutions.json")))[key]
    gs = [(n, tuple(q)) for n, q in rec["gateset"]]
    m = Model(rec["env"], rec["num_qubits"], gs, 1, track_solution=True)
    m.set_state(np.array(rec["state"]).reshape(1, -1))
    actions = [gs.index((n, tuple(q))) for n, q in rec["circuit"]]
    for a in actions:
        assert not m.is_final()[0]
        m.step([a])
    assert m.success[0] and m.is_final()[0] and m.solutions()[0] == actions


# ---- the oracle, at every size --------------------------------------------------------------------------------------------
def _random_gateset(kind, n, rng):
    if kind == "permutation" and n in (9, 16, 36, 64, 256) and rng.random() < 0.5:
        side = int(round(n ** 0.5))
        gs = grid_gateset(kind, side, side, bidirectional=bool(rng.integers(0, 2)))
    else:
        gs = line_gateset(kind, n)
    gs = [gs[i] for i in np.sort(rng.choice(len(gs), size=max(1, min(len(gs), int(rng.integers(len(gs) // 2 + 1, len(gs) + 1)))), replace=False))]
    q = int(rng.integers(0, n))  # gates on one qubit twice
    gs += [("SWAP", (q, q))] + ([] if kind == "permutation" else [("CX", (q, q))]) + ([("CZ", (q, q))] if kind == "clifford" else [])
    return gs


CROSS = [("clifford", n) for n in (2, 3, 7, 16, 17, 32)] + [("linear_function", n) for n in (2, 8, 9, 32, 33, 64)] + \
        [("permutation", n) for n in (2, 9, 16, 17, 64, 256)]


@pytest.mark.parametrize("kind,n", CROSS)
def test_model_equals_the_oracle(kind, n):
    from oracle import OracleEnv

    rng = np.random.default_rng(100 * n + len(kind))
    for trial in range(2):
        gs = _random_gateset(kind, n, rng)
        A = len(gs)
        B = 24 if n <= 32 else 8
        inverts, track = bool(trial == 0 or rng.integers(0, 2)), bool(rng.integers(0, 2) or trial == 0)
        w = {k: float(np.float32(rng.choice([0.0, rng.uniform(0, 0.5)]))) for k in ("n_cnots", "n_layers_cnots", "n_layers", "n_gates")}
        cfg = dict(max_depth=int(rng.integers(10, 40)), depth_slope=int(rng.integers(1, 4)))
        m = Model(kind, n, gs, B, add_inverts=inverts, track_solution=track, metrics_weights=w, **cfg)
        m.want_depths = True
        envs = [OracleEnv(kind, n, gs, metrics_weights=w, add_inverts=int(inverts), track_solution=int(track), add_perms=0, **cfg)
                for _ in range(B)]
        diff = int(rng.integers(1, 2 * n + 2))
        draws = rng.integers(0, A, size=(diff, B))
        m.reset_with(draws)
        for e, o in enumerate(envs):
            o.difficulty = diff
            o.reset_with(draws[:, e])
        for t in range(cfg["max_depth"] + 4):
            acts = rng.integers(0, A, size=B)
            acts[rng.random(B) < 0.1] = A + int(rng.integers(0, 4))
            acts[rng.random(B) < 0.05] = -1
            coins = rng.integers(0, 2, size=B)
            m.step(acts, coins)
            for e, o in enumerate(envs):
                o.step(int(acts[e]), int(coins[e]))
            lbl = f"{kind} {n} trial {trial} t={t}"
            np.testing.assert_array_equal(m.wire(), np.stack([o.get_state() for o in envs]), err_msg=lbl)
            np.testing.assert_array_equal(f32_bits(m.reward), [o.reward_bits() for o in envs], err_msg=lbl)
            np.testing.assert_array_equal(m.metrics, [o.metrics() for o in envs], err_msg=lbl)
            np.testing.assert_array_equal(m.depth, [o.depth() for o in envs], err_msg=lbl)
            np.testing.assert_array_equal(m.success, [o.success() for o in envs], err_msg=lbl)
            np.testing.assert_array_equal(m.is_final(), [o.is_final() for o in envs], err_msg=lbl)
            np.testing.assert_array_equal(m.masks(), [o.masks() for o in envs], err_msg=lbl)
        if track:
            assert m.solutions() == [o.solution() for o in envs]


@pytest.mark.parametrize("kind,n", [("clifford", 3), ("linear_function", 4), ("permutation", 4)])
def test_replayed_targets_succeed_on_the_oracle_at_the_predicted_step(kind, n):
    """Even envs replay their target with zero coins: they solve at the step the model predicts (at or before the target's last gate),
    with reward 1 - penalty.  Odd envs act at random with random coins: the model's logs compose to its state after every step."""
    from oracle import OracleEnv

    rng = np.random.default_rng(7)
    gs = line_gateset(kind, n)
    B, T = 40, 8
    circs = rng.integers(0, len(gs), size=(B, T))
    m = Model(kind, n, gs, B, add_inverts=True, track_solution=True)
    start = m.state_of_circuit(circs)
    m.set_state(m.wire(start))
    envs = [OracleEnv(kind, n, gs, add_inverts=1, track_solution=1, add_perms=0) for _ in range(B)]
    for e, o in enumerate(envs):
        o.set_state(m.wire(start)[e])
    first = np.full(B, -1)
    for t in range(T):
        acts = np.where(np.arange(B) % 2 == 0, circs[:, t], rng.integers(0, len(gs), size=B))
        coins = rng.integers(0, 2, size=B) * (np.arange(B) % 2)
        m.step(acts, coins)
        for e, o in enumerate(envs):
            o.step(int(acts[e]), int(coins[e]))
            if e % 2 == 0 and first[e] < 0 and o.success():
                first[e] = t + 1
                assert m.success[e] and m.reward[e] == np.float32(1) - m.penalty[e]
        np.testing.assert_array_equal(m.logged_state(start), m.state)
        np.testing.assert_array_equal(m.success, [o.success() for o in envs])
    # the prediction from the target alone: after k replayed gates the state is G(target[k:])^-1, solved where that suffix is the identity
    suffix = Model(kind, n, gs, B)
    solved_after = np.stack([suffix.solved(suffix.product(circs[:, k:].tolist())) for k in range(1, T + 1)])
    np.testing.assert_array_equal(first[::2], solved_after.argmax(0)[::2] + 1)
    assert m.solutions() == [o.solution() for o in envs]


# ---- a curriculum: the difficulty set through the setter, many times over, on live envs ----------------------------------------------
@pytest.mark.parametrize("kind,n", [("clifford", 3), ("linear_function", 5), ("permutation", 6)])
def test_difficulty_set_along_a_ladder_equals_envs_built_at_it(kind, n):
    """What tests/test_gpu_curriculum.py leans on: an oracle batch whose difficulty is SET, rung after rung (0 included: no gate, depth 0,
    final at once), resets like fresh oracle envs CONSTRUCTED at that difficulty -- its seeded reset with the draws util.rng_actions makes
    in numpy -- and like the model, whose start depth follows the number of draws; a reset with another number of draws is refused."""
    from oracle import OracleEnv, OracleError, OracleVec
    from util import rng_actions

    ladder = [1, 2, 8, 9, 16, 17, 63, 64, 65, 256, 70, 9, 8, 1, 5, 0, 0, 3]
    gs = line_gateset(kind, n)
    A, B = len(gs), 7
    cfg = dict(add_inverts=0, add_perms=0, track_solution=0, depth_slope=2, max_depth=128)
    per_env = {"clifford": 4 * n * n, "linear_function": n * n, "permutation": n}[kind]
    ov = OracleVec(OracleEnv(kind, n, gs, **cfg), B)  # built at the default, 1
    live = [ov.env(e) for e in range(B)]
    m = Model(kind, n, gs, B, depth_slope=2, max_depth=128)
    rng = np.random.default_rng(n)
    for i, d in enumerate(ladder):
        for o in live + [ov.proto]:
            o.difficulty = d
            assert o.difficulty == d
        seed = 60 + i
        draws = rng_actions(seed, B, d, A)
        assert draws.shape == (d, B)
        ov.reset_seeded(seed)
        fresh = OracleVec(OracleEnv(kind, n, gs, difficulty=d, **cfg), B)
        fresh.reset_with(draws)
        m.reset_with(draws)
        lbl = f"{kind} {n} rung {i} (difficulty {d})"
        np.testing.assert_array_equal(ov.get_state(per_env), fresh.get_state(per_env), err_msg=lbl)
        np.testing.assert_array_equal(ov.get_state(per_env), m.wire(), err_msg=lbl)
        np.testing.assert_array_equal([o.depth() for o in live], min(2 * d, 128), err_msg=lbl)  # clifford.rs:317
        np.testing.assert_array_equal(m.depth, min(2 * d, 128), err_msg=lbl)
        np.testing.assert_array_equal([o.is_final() for o in live], m.is_final(), err_msg=lbl)
        if d == 0:
            assert all(o.is_final() and o.success() for o in live)
        with pytest.raises(OracleError, match="exactly `difficulty`"):
            live[0].reset_with(rng.integers(0, A, size=d + 1))
        for t in range(2):
            acts = rng.integers(-1, A + 2, size=B)
            got, want = ov.step(acts), fresh.step(acts)
            m.step(acts)
            for g, w, name in zip(got, want, ("reward", "success", "is_final", "depth")):
                np.testing.assert_array_equal(f32_bits(g) if name == "reward" else g, f32_bits(w) if name == "reward" else w, err_msg=f"{name} {lbl} t={t}")
            np.testing.assert_array_equal(f32_bits(got[0]), f32_bits(m.reward), err_msg=lbl)
            np.testing.assert_array_equal(got[2], m.is_final(), err_msg=lbl)
            np.testing.assert_array_equal(got[3], m.depth, err_msg=lbl)
            np.testing.assert_array_equal(ov.get_state(per_env), m.wire(), err_msg=lbl)
