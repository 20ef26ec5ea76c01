"""tests/paulimodel.py proved on the CPU: against explicit 2^n x 2^n unitaries at n <= 3 (the signed rotations, the tableau and the
decoded solution logs), and against the CPU oracle at every size the library supports (the one place the oracle meets the model)."""
import numpy as np
import pytest

from envmodel import ONE, op1, two
from paulimodel import PauliModel, PauliPanic, heap_permutations, parse_label, qubit_perms, to_wire
from test_physics import PHYSICAL, encode, random_circuit, same_up_to_phase, unitary
from util import f32_bits, grid_gateset, line_gateset

KINDS = ("h", "s", "sdg", "sx", "sxdg", "cx", "cz", "swap")


def _names(gs):
    return [(a.lower(), tuple(int(q) for q in b)) for a, b in gs]


def random_labels(rng, n, count, max_weight=4, signs=True):
    out = []
    for _ in range(count):
        w = int(rng.integers(1, min(max_weight, n) + 1))
        s = ["I"] * n
        for q in rng.choice(n, size=w, replace=False):
            s[n - 1 - q] = "XYZ"[rng.integers(3)]
        out.append(("-" if signs and rng.random() < 0.4 else "") + "".join(s))
    return out


def random_tableau(rng, n, steps):
    """A random symplectic tableau: random elementary gates applied to the identity through the model's own tables."""
    m = PauliModel(n, [("H", (q,)) for q in range(n)], 1)
    net = m.nets[0]
    for _ in range(steps):
        if n > 1 and rng.random() < 0.6:
            a, b = rng.choice(n, size=2, replace=False)
            net.act("cx", int(a), int(b))
        else:
            net.act(["h", "s", "sx"][rng.integers(3)], int(rng.integers(n)), 0)
    return net.tab.copy()


# ---- physics, n <= 3 ------------------------------------------------------------------------------------------------------
def physical(kind, a, b, n):
    """The unitary the network applies for one action: CX(a, b) is the network's cnot(a, b) = CX with control b, target a; CZ and
    SWAP as the reference composes them (pauli_network.rs:242-256)."""
    cnot = lambda i, j: two("cx", j, i, n)  # noqa: E731
    if kind in ONE:
        return op1(ONE[kind], a, n)
    if kind == "cx":
        return cnot(a, b)
    h = op1(ONE["h"], b, n)
    if kind == "cz":
        return h @ cnot(a, b) @ h
    return cnot(a, b) @ cnot(b, a) @ cnot(a, b)


def label_matrix(x, z, k):
    from envmodel import _pauli

    return (-1j) ** k * _pauli(list(x), list(z))


@pytest.mark.parametrize("n", [2, 3])
def test_rotations_and_tableau_evolve_by_conjugation(n):
    """Every gate kind: each rotation -- removed or not -- is W P W^dagger, and each tableau column's bits are those of W C W^dagger,
    W the product of the actions' unitaries."""
    rng = np.random.default_rng(n)
    gs = line_gateset("pauli", n)
    names = _names(gs)
    assert {k for k, _ in names} == set(KINDS)
    for trial in range(40):
        labels = random_labels(rng, n, int(rng.integers(1, 6)))
        if trial % 5 == 0:
            labels.append("i" + labels[0].lstrip("-"))  # a non-Hermitian coefficient rides along unchanged
        tab = random_tableau(rng, n, 6)
        m = PauliModel(n, gs, 1, max_rotations=8)
        m.reset_from([tab], [labels])
        w = np.eye(2 ** n, dtype=complex)
        for a in rng.integers(0, len(gs), size=12):
            kind, qs = names[a]
            m.step([a])
            w = physical(kind, qs[0], qs[-1], n) @ w
        net = m.nets[0]
        for r, lab in enumerate(labels):
            p0 = label_matrix(*parse_label(lab, n))
            np.testing.assert_allclose(label_matrix(*net.signed(r)), w @ p0 @ w.conj().T, atol=1e-9, err_msg=f"{labels} rotation {r}")
        for c in range(2 * n):
            c0 = label_matrix(tab[:n, c], tab[n:, c], 0)
            img = w @ c0 @ w.conj().T
            got = label_matrix(net.tab[:n, c], net.tab[n:, c], 0)
            assert abs(abs(np.trace(got.conj().T @ img)) / 2 ** n - 1) < 1e-9, (labels, c)


class _ScalarModel:
    """test_physics.replay's env interface on a batch of one."""

    def __init__(self, n, gs):
        self.m = PauliModel(n, gs, 1, max_rotations=6, add_perms=False, track_solution=True, max_depth=128)

    def set_state(self, state):
        self.m.set_state([state])

    def step(self, a):
        self.m.step([a])

    def success(self):
        return bool(self.m.success[0])

    def solution(self):
        return self.m.solutions()[0]


@pytest.mark.parametrize("seed", range(3))
def test_model_solutions_reproduce_the_encoded_unitary(seed):
    """test_physics's encode / replay / decode round trip on the model: the log, decoded, is the circuit up to global phase."""
    from test_physics import replay

    rng = np.random.default_rng(50 + seed)
    for _ in range(50):
        n = int(rng.integers(2, 4))
        names = _names(line_gateset("pauli", n))
        circ = random_circuit(n, rng, names, PHYSICAL)
        solved, dec = replay(_ScalarModel, n, circ)
        assert solved, circ
        assert same_up_to_phase(unitary(circ, n), unitary(dec, n)), (circ, dec)


def test_model_reproduces_the_reference_quirks():
    """CZ's H sits on what cnot makes the control, so no action undoes a CZ; a SWAP logs a rotation collected mid-gate behind it."""
    n = 3
    gs = line_gateset("pauli", n)
    state, _ = encode([("cz", (0, 1))], n)
    for a in range(len(gs)):
        m = _ScalarModel(n, gs)
        m.set_state(state)
        m.step(a)
        assert not m.success()
    from test_physics import replay

    circ = [("rx", 0, 1.3), ("swap", (0, 1)), ("cx", (0, 1)), ("cx", (0, 1))]
    solved, dec = replay(_ScalarModel, 2, circ)
    assert solved and dec[:2] == [("swap", (0, 1)), ("rx", 0, 1.3)]


def test_node_order_is_swap_remove_and_the_clean_repeats():
    """Five mutually commuting rotations, all in the front layer; 0, 1 and 3 trivial from the start: reverse visit, swap-remove."""
    n = 4
    labels = ["IIIZ", "IIXI", "ZZII", "IZII", "XXXX"]
    m = PauliModel(n, line_gateset("pauli", n), 1, max_rotations=5)
    m.reset_from([np.eye(2 * n, dtype=np.uint8)], [labels])
    # order [0 1 2 3 4]: remove 3 -> [0 1 2 4]; remove 1 -> [0 4 2]; remove 0 -> [2 4]
    assert m.active() == [[2, 4]]
    # a later rotation that anticommutes with an earlier trivial one waits for it: the second pass removes it
    m.reset_from([np.eye(2 * n, dtype=np.uint8)], [["IIIZ", "IIIX", "IXZI"]])
    assert m.active() == [[2]]


def test_weight_zero_and_perm_index_panics():
    n = 3
    gs = line_gateset("pauli", n)
    m = PauliModel(n, gs, 2, max_rotations=4)
    with pytest.raises(PauliPanic):
        m.reset_from([np.eye(2 * n, dtype=np.uint8)] * 2, [["XXI"], ["III"]])
    assert m.dead.tolist() == [False, True]
    # CX on one qubit twice clears qubit 0: rotation 0 drops to weight 1 and leaves, rotation 1 (Z_0, waiting behind it) has weight 0
    gs2 = gs + [("CX", (0, 0))]
    m = PauliModel(n, gs2, 1, max_rotations=4)
    m.reset_from([np.eye(2 * n, dtype=np.uint8)], [["IXX", "IIZ"]])
    assert m.active() == [[0, 1]]
    with pytest.raises(PauliPanic):
        m.step([len(gs2) - 1])
    mp = PauliModel(n, gs, 2, max_rotations=4, add_perms=True)
    mp.observe_perm([0, 1])
    with pytest.raises(PauliPanic):
        mp.step([0, len(gs)])
    assert mp.dead.tolist() == [False, True]


def test_heap_order_and_automorphisms():
    assert heap_permutations(3) == [(0, 1, 2), (1, 0, 2), (2, 0, 1), (0, 2, 1), (1, 2, 0), (2, 1, 0)]
    qp, _ = qubit_perms(4, line_gateset("pauli", 4))
    assert qp == [[0, 1, 2, 3], [3, 2, 1, 0]]
    qp, _ = qubit_perms(3, [("H", (q,)) for q in range(3)])  # no edge: Heap's order
    assert qp == [list(p) for p in heap_permutations(3)]
    qp, _ = qubit_perms(3, [("CX", (0, 1)), ("CX", (1, 2))])  # one direction only: the reflection maps CX(0, 1) to CX(2, 1), absent
    assert qp == [[0, 1, 2]]


# ---- the oracle, at every size --------------------------------------------------------------------------------------------
def all_to_all(n):
    gs = [(k, (q,)) for q in range(n) for k in ("H", "S", "SX")]
    return gs + [(k, (a, b)) for a in range(n) for b in range(n) if a != b for k in ("CX", "CZ", "SWAP")]


def _gateset(shape, n, rng):
    if shape == "line":
        gs = line_gateset("pauli", n)
    elif shape in ("grid", "bigrid"):
        side = {2: (1, 2), 3: (1, 3), 5: (1, 5), 8: (2, 4), 20: (4, 5), 24: (4, 6), 25: (5, 5), 32: (4, 8)}[n]
        gs = grid_gateset("pauli", *side, bidirectional=shape == "bigrid")
    else:
        gs = all_to_all(n)
    keep = np.sort(rng.choice(len(gs), size=max(2, int(len(gs) * rng.uniform(0.6, 1.0))), replace=False))
    return [gs[i] for i in keep]


CROSS = [(n, shape) for n, shapes in ((2, ("line", "all")), (3, ("line", "grid", "all")), (5, ("line", "bigrid", "all")),
                                       (8, ("line", "grid", "bigrid", "all")), (20, ("line", "bigrid")), (24, ("grid",)), (25, ("bigrid",)),
                                       (32, ("line", "grid"))) for shape in shapes]


def _compare(m, envs, alive, label):
    idx = [e for e in range(m.B) if alive[e]]
    if not idx:
        return
    o = [envs[e] for e in idx]
    np.testing.assert_array_equal(f32_bits(m.reward[idx]), [x.reward_bits() for x in o], err_msg=f"reward {label}")
    np.testing.assert_array_equal(m.is_final()[idx], [x.is_final() for x in o], err_msg=f"done {label}")
    np.testing.assert_array_equal(m.success[idx], [x.success() for x in o], err_msg=f"success {label}")
    np.testing.assert_array_equal(m.depth[idx], [x.depth() for x in o], err_msg=f"depth {label}")
    np.testing.assert_array_equal(m.masks()[idx], [x.masks() for x in o], err_msg=f"masks {label}")
    np.testing.assert_array_equal(m.tableau()[idx], np.stack([x.get_state() for x in o]), err_msg=f"tableau {label}")
    assert [m.active()[e] for e in idx] == [x.active_rotations() for x in o], label
    if not m.perms:
        np.testing.assert_array_equal(m.observe()[idx], np.stack([x.dense_obs().reshape(-1) for x in o]), err_msg=f"observe {label}")


def _run_against_oracle(m, envs, rng, T, alive, perms_n, out_of_range, label):
    from oracle import OracleError

    A = m.A
    for t in range(T):
        if perms_n:
            draws = rng.integers(0, 3 * perms_n, size=m.B)
            got = m.observe_perm(draws)
            for e in np.flatnonzero(alive):
                np.testing.assert_array_equal(got[e], envs[e].dense_obs(int(draws[e])).reshape(-1), err_msg=f"permuted obs {label} t={t}")
        acts = rng.integers(0, A, size=m.B)
        if out_of_range:
            acts[rng.random(m.B) < 0.1] = A + int(rng.integers(0, 3))
            acts[rng.random(m.B) < 0.04] = -1
        try:
            m.step(acts)
        except PauliPanic:
            pass
        for e in np.flatnonzero(alive):
            try:
                envs[e].step(int(acts[e]))
                assert not m.dead[e], f"{label} t={t} env {e}: the model panicked, the oracle did not"
            except OracleError:
                assert m.dead[e], f"{label} t={t} env {e}: the oracle panicked, the model did not"
                alive[e] = False
        _compare(m, envs, alive, f"{label} t={t}")
    if m.track_solution:
        for e in np.flatnonzero(alive):
            assert m.solutions()[e] == envs[e].solution(), (label, e)


@pytest.mark.parametrize("n,shape", CROSS)
def test_model_equals_the_oracle(n, shape):
    from oracle import OracleEnv, OracleError

    rng = np.random.default_rng(1000 * n + len(shape))
    for trial in range(3):  # 0: set_state; 1: explicit targets, gates on one qubit twice; 2: explicit targets, more than max_rotations
        gs = _gateset(shape, n, rng)
        if trial == 1 and n <= 8:  # two-qubit gates on one qubit twice
            q = int(rng.integers(n))
            gs = gs + [(k, (q, q)) for k in ("CX", "CZ", "SWAP")]
        max_rot = int(rng.choice([1, 3, 5, 8, 9, 16, 17] + ([32] if trial < 2 else [])))
        final = {0: int(min(32, max_rot + rng.integers(0, 12))), 1: max_rot, 2: int(min(32, max_rot + rng.integers(4, 16)))}[trial]
        B = 12 if n >= 20 else 24
        w = {k: float(np.float32(rng.choice([0.0, rng.uniform(0, 0.3)]))) for k in ("n_cnots", "n_layers_cnots", "n_layers", "n_gates")}
        cfg = dict(max_rotations=max_rot, final_pauli_layers=final, max_depth=int(rng.integers(8, 30)), depth_slope=int(rng.integers(1, 4)),
                   difficulty=int(rng.integers(1, 12)), pauli_layer_reward=float(np.float32(rng.uniform(0.001, 0.2))), track_solution=1)
        m = PauliModel(n, gs, B, max_rotations=max_rot, track_solution=True, metrics_weights=w,
                       **{k: cfg[k] for k in ("max_depth", "depth_slope", "difficulty", "pauli_layer_reward")})
        envs = [OracleEnv("pauli", n, gs, metrics_weights=w, add_perms=0, **cfg) for _ in range(B)]
        alive = np.ones(B, bool)
        tabs = [random_tableau(rng, n, int(rng.integers(0, 3 * n))) for _ in range(B)]
        low = max_rot + 1 if trial == 2 else 0
        labs = [random_labels(rng, n, int(rng.integers(low, final + 1)), max_weight=int(rng.integers(2, 5))) for _ in range(B)]
        if trial == 0:  # entry by the wire format: labels beyond max_rotations dropped, no clean, tableau entries > 1
            wires = [to_wire(tabs[e], labs[e], scale=int(rng.integers(1, 4))) for e in range(B)]
            width = max(len(x) for x in wires)
            m.set_state([x + [0] * (width - len(x)) for x in wires])
            for e, o in enumerate(envs):
                o.set_state(wires[e] + [0] * (width - len(wires[e])))
        else:
            try:
                m.reset_from(tabs, labs)
            except PauliPanic:
                pass
            for e, o in enumerate(envs):
                try:
                    o.pauli_reset_from(tabs[e], labs[e])
                    assert not m.dead[e]
                except OracleError:
                    assert m.dead[e]
                    alive[e] = False
        _compare(m, envs, alive, f"{n} {shape} trial {trial} entry")
        if trial == 2 and n >= 5:  # more rotations active than the observation shows
            assert max(len(a) for a in m.active()) > max_rot
        _run_against_oracle(m, envs, rng, cfg["max_depth"] + 4, alive, 0, True, f"{n} {shape} trial {trial}")


@pytest.mark.parametrize("n,shape", [(3, "line"), (4, "grid"), (5, "bigrid"), (4, "all"), (6, "line")])
def test_permuted_observations_and_unpermuted_actions_equal_the_oracle(n, shape):
    from oracle import OracleEnv

    rng = np.random.default_rng(7 * n)
    if shape == "grid":
        gs = grid_gateset("pauli", 2, 2)
    elif shape == "bigrid":
        gs = grid_gateset("pauli", 1, 5, bidirectional=True)
    elif shape == "all":
        gs = all_to_all(n)
    else:
        gs = line_gateset("pauli", n)
    B, max_rot = 24, 6
    m = PauliModel(n, gs, B, max_rotations=max_rot, add_perms=True, max_depth=20, difficulty=3, pauli_layer_reward=0.05)
    envs = [OracleEnv("pauli", n, gs, add_perms=1, track_solution=1, max_rotations=max_rot, max_depth=20, difficulty=3,
                      pauli_layer_reward=0.05) for _ in range(B)]
    tabs = [random_tableau(rng, n, 2 * n) for _ in range(B)]
    labs = [random_labels(rng, n, int(rng.integers(0, max_rot + 3)), 3) for _ in range(B)]
    m.reset_from(tabs, labs)
    for e, o in enumerate(envs):
        o.pauli_reset_from(tabs[e], labs[e])
    alive = np.ones(B, bool)
    _compare(m, envs, alive, "entry")
    _run_against_oracle(m, envs, rng, 24, alive, len(m.perms), False, f"perms {n} {shape}")
    assert len(m.perms) > 1


def test_qubit_perms_equal_the_oracle():
    from oracle import qubit_perms as oracle_perms

    for n, gs in ((4, line_gateset("pauli", 4)), (4, grid_gateset("pauli", 2, 2)), (5, grid_gateset("pauli", 1, 5, bidirectional=True)),
                  (4, all_to_all(4)), (3, [("H", (q,)) for q in range(3)]), (4, [("CX", (0, 1)), ("CX", (2, 3)), ("SWAP", (1, 2)), ("S", (0,))])):
        assert qubit_perms(n, gs) == oracle_perms(n, gs), (n, gs)
