"""An env model that shares no code with the oracle or libqgym: numpy, vectorised over the batch, CPU only.

Every gate's action is derived ONCE, at import, from its unitary (the matrices `test_physics.py` checks against quantum
mechanics): conjugating the 1- and 2-qubit Paulis by the 2x2 / 4x4 unitary gives the local symplectic map of CliffordEnv,
and applying the CX / SWAP basis permutation to basis states gives the GF(2) map of LinearFunctionEnv (and, for SWAP, the
index map of PermutationEnv).  A step gathers the rows (or entries) the gate touches, multiplies them by the local map
over GF(2) and scatters them back -- no per-gate row rule is written out by hand.

What is NOT physics and is restated from the reference text (rust/src/envs/*.rs of qiskit-gym):
  * a 2-qubit gate on one qubit twice leaves the state unchanged (clifford.rs:121,131,140; linear_function.rs:60,70);
  * the gate metrics decompose SWAP into 3 CX and CZ(a, b) into 1q(b) CX(a, b) 1q(b), dropping CX with c == t
    (metrics.rs:67-124), so CZ(a, a) still counts two one-qubit gates;
  * the step order: metrics and state, then the solution log, depth, the add_inverts coin, then `success`
    (clifford.rs:318-345, linear_function.rs step); PermutationEnv logs valid actions only and spends depth after the coin
    (permutation.rs:185-216);
  * rewards: achieved - (w_cnots*d_cnots + w_layers_cnots*d_layers_cnots + w_layers*d_layers + w_gates*d_gates), f32, in that order
    (metrics.rs:135-148).

Metrics are recomputed from the whole logged episode prefix at every step, as the longest path of the gate DAG (all gates for
`n_layers`, CX only for `n_layers_cnots`); the inversion is a plain Gauss-Jordan elimination over GF(2)."""
from __future__ import annotations

import itertools

import numpy as np

# ---- the gates' unitaries (qiskit conventions: qubit 0 is the least significant bit) ---------------------------------------
I2 = np.eye(2, dtype=complex)
X = np.array([[0, 1], [1, 0]], dtype=complex)
Y = np.array([[0, -1j], [1j, 0]])
Z = np.diag([1, -1]).astype(complex)
ONE = {"h": (X + Z) / np.sqrt(2), "s": np.diag([1, 1j]), "sdg": np.diag([1, -1j]),
       "sx": 0.5 * np.array([[1 + 1j, 1 - 1j], [1 - 1j, 1 + 1j]]), "sxdg": 0.5 * np.array([[1 - 1j, 1 + 1j], [1 + 1j, 1 - 1j]])}
P1 = {"I": I2, "X": X, "Y": Y, "Z": Z}
TWO_KINDS = ("cx", "cz", "swap")
KINDS = tuple(ONE) + TWO_KINDS


def op1(g, q, n):
    m = np.array([[1]], dtype=complex)
    for k in range(n - 1, -1, -1):  # qubit 0 is the least significant bit
        m = np.kron(m, g if k == q else I2)
    return m


def two(kind, a, b, n):
    d = 2 ** n
    m = np.zeros((d, d), dtype=complex)
    for i in range(d):
        ba, bb = (i >> a) & 1, (i >> b) & 1
        if kind == "cx":  # control a, target b
            m[i ^ (1 << b) if ba else i, i] = 1
        elif kind == "cz":
            m[i, i] = -1 if ba and bb else 1
        else:
            m[i & ~((1 << a) | (1 << b)) | (bb << a) | (ba << b), i] = 1
    return m


def local_unitary(kind):
    return ONE[kind] if kind in ONE else two(kind, 0, 1, 2)


def _pauli(x, z):
    """Pauli string X^x Z^z (x, z bit lists, qubit 0 first) with the Y = iXZ convention: Hermitian."""
    m = np.array([[1]], dtype=complex)
    for q in range(len(x) - 1, -1, -1):
        m = np.kron(m, P1["IXZY"[x[q] + 2 * z[q]]])
    return m


def _conjugation_map(u):
    """(S, sign) of P -> u P u^dagger on k qubits: column j of S is the (x, z) of the image of generator j (X_0..X_{k-1}, Z_0..Z_{k-1}),
    sign[j] is its sign (+1 / -1) relative to the Hermitian Pauli string of those bits."""
    k = int(round(np.log2(u.shape[0])))
    S = np.zeros((2 * k, 2 * k), dtype=np.uint8)
    sign = np.zeros(2 * k, dtype=np.int64)
    strings = [(list(b[:k]), list(b[k:])) for b in itertools.product((0, 1), repeat=2 * k)]
    for j in range(2 * k):
        bits = [0] * (2 * k)
        bits[j] = 1
        img = u @ _pauli(bits[:k], bits[k:]) @ u.conj().T
        for x, z in strings:
            c = np.trace(_pauli(x, z).conj().T @ img) / 2 ** k
            if abs(abs(c) - 1) < 1e-9:
                assert abs(c.imag) < 1e-9
                S[:, j] = x + z
                sign[j] = 1 if c.real > 0 else -1
                break
        else:
            raise AssertionError("not a Clifford")
    return S, sign


def _basis_map(u):
    """L with u|x> = |L x> over GF(2), for a basis permutation u (CX, SWAP)."""
    k = int(round(np.log2(u.shape[0])))
    L = np.zeros((k, k), dtype=np.uint8)
    for j in range(k):
        out = np.flatnonzero(np.abs(u[:, 1 << j]) > 0.5)
        assert out.size == 1 and abs(abs(u[out[0], 1 << j]) - 1) < 1e-9
        L[:, j] = [(out[0] >> i) & 1 for i in range(k)]
    for col in range(2 ** k):  # linear on every basis state, not only on the unit vectors
        out = np.flatnonzero(np.abs(u[:, col]) > 0.5)
        want = sum(int((L @ [(col >> i) & 1 for i in range(k)])[i] % 2) << i for i in range(k))
        assert out.size == 1 and out[0] == want
    return L


SYMPLECTIC = {k: _conjugation_map(local_unitary(k)) for k in KINDS}  # (S [2k, 2k], sign [2k])
LINEAR = {k: _basis_map(local_unitary(k)) for k in ("cx", "swap")}  # [2, 2]


# ---- GF(2) linear algebra ------------------------------------------------------------------------------------------------
def gf2_inverse(m):
    """Gauss-Jordan over GF(2) of a batch of square matrices [B, d, d] -> (inverse, ok [B] bool: False where singular)."""
    m = np.array(m, dtype=np.uint8) & 1
    B, d, _ = m.shape
    aug = np.concatenate([m, np.broadcast_to(np.eye(d, dtype=np.uint8), (B, d, d))], axis=2)
    ok = np.ones(B, dtype=bool)
    ar = np.arange(B)
    for col in range(d):
        cand = aug[:, col:, col].astype(bool)
        has = cand.any(axis=1)
        ok &= has
        piv = col + np.argmax(cand, axis=1)
        rows_c, rows_p = aug[ar, col].copy(), aug[ar, piv].copy()
        aug[ar, col], aug[ar, piv] = rows_p, rows_c
        elim = aug[:, :, col].astype(bool) & has[:, None]
        elim[:, col] = False
        aug ^= elim[:, :, None] * aug[:, col:col + 1, :]
    return aug[:, :, d:], ok


def gf2_matmul(a, b):
    return (np.einsum("bij,bjk->bik", a.astype(np.int64), b.astype(np.int64)) & 1).astype(np.uint8)


# ---- gatesets ------------------------------------------------------------------------------------------------------------
def parse(gateset):
    """[(name, qubits)] -> (kind index into KINDS [A], q0 [A], q1 [A]) (q1 = q0 for one-qubit gates)."""
    kid = np.array([KINDS.index(g[0].lower()) for g in gateset], dtype=np.int64)
    q0 = np.array([int(g[1][0]) for g in gateset], dtype=np.int64)
    q1 = np.array([int(g[1][1]) if len(g[1]) > 1 else int(g[1][0]) for g in gateset], dtype=np.int64)
    return kid, q0, q1


# ---- the metrics, from the whole prefix -----------------------------------------------------------------------------------
def elementary(kind, a, b, n):
    """The decomposition the metrics count (metrics.rs:67-124): [('1q', q) | ('cx', c, t)], invalid pieces dropped."""
    if kind in ONE:
        out = [("1q", a)]
    elif kind == "cx":
        out = [("cx", a, b)]
    elif kind == "swap":
        out = [("cx", a, b), ("cx", b, a), ("cx", a, b)]
    else:  # CZ: the one-qubit gates sit on the target
        out = [("1q", b), ("cx", a, b), ("1q", b)]
    return [g for g in out if all(q < n for q in g[1:]) and not (g[0] == "cx" and g[1] == g[2])]


def decomposition_table(gateset, n):
    """[A, 3, 3] int64: each action's elementary gates (kind 0 none / 1 one-qubit / 2 CX, qubit, qubit)."""
    tab = np.zeros((max(len(gateset), 1), 3, 3), np.int64)
    for a, (name, qs) in enumerate(gateset):
        for k, g in enumerate(elementary(name.lower(), int(qs[0]), int(qs[-1]), n)):
            tab[a, k] = (1 if g[0] == "1q" else 2, g[1], g[-1])
    return tab


def metrics_of(episodes, table, n, depths=True):
    """(n_cnots, n_layers_cnots, n_layers, n_gates) [B, 4] of each env's applied actions `episodes` [B, T] (-1: none).

    Both depths are the longest path of the circuit's gate DAG (an edge joins consecutive gates on a qubit; for n_layers_cnots the
    circuit of its CX alone): walking the gates in circuit order, which is a topological order, the longest path that ends at a
    gate is one more than the longest that ends at the latest earlier gate on any of its qubits."""
    episodes = np.asarray(episodes, dtype=np.int64)
    B, T = episodes.shape
    ops = np.where((episodes >= 0)[:, :, None, None], table[np.maximum(episodes, 0)], 0).reshape(B, 3 * T, 3)
    kind = ops[:, :, 0]
    out = np.zeros((B, 4), np.int64)
    out[:, 0] = (kind == 2).sum(1)
    out[:, 3] = (kind > 0).sum(1)
    if not depths:
        return out
    ar = np.arange(B)
    for col, cx_only in ((1, True), (2, False)):
        end = np.zeros((B, n + 1), np.int64)  # longest path ending at the latest gate on each qubit (column n: a sink)
        for j in range(3 * T):
            k = kind[:, j]
            live = (k == 2) | ((k == 1) & (not cx_only))
            a = np.where(live, ops[:, j, 1], n)
            b = np.where(live & (k == 2), ops[:, j, 2], a)
            length = np.maximum(end[ar, a], end[ar, b]) + 1
            end[ar, a] = np.where(live, length, end[ar, a])
            end[ar, b] = np.where(live, length, end[ar, b])
        out[:, col] = end[:, :n].max(1)
    return out


WEIGHT_KEYS = ("n_cnots", "n_layers_cnots", "n_layers", "n_gates")
DEFAULT_WEIGHTS = {"n_cnots": 0.01, "n_layers_cnots": 0.0, "n_layers": 0.0, "n_gates": 0.0001}  # metrics.rs:153-162


# ---- the batched env -----------------------------------------------------------------------------------------------------
class Model:
    """B envs of one kind ("clifford" | "linear_function" | "permutation"), driven like the trait: set_state / reset_with / step."""

    def __init__(self, kind, n, gateset, batch, *, add_inverts=False, track_solution=False, max_depth=128, depth_slope=2,
                 metrics_weights=None):
        assert kind in ("clifford", "linear_function", "permutation")
        self.kind, self.n, self.B = kind, int(n), int(batch)
        self.gateset = [(g[0].lower(), tuple(int(q) for q in g[1])) for g in gateset]
        self.A = len(self.gateset)
        self.kid, self.q0, self.q1 = parse(self.gateset) if self.A else (np.zeros(0, np.int64),) * 3
        assert (self.q0 < n).all() and (self.q1 < n).all()
        self.add_inverts, self.track_solution = bool(add_inverts), bool(track_solution)
        self.max_depth, self.depth_slope = int(max_depth), int(depth_slope)
        w = dict(DEFAULT_WEIGHTS)
        w.update({k: v for k, v in (metrics_weights or {}).items() if k in w})
        self.w = [np.float32(w[k]) for k in WEIGHT_KEYS]
        self.table = decomposition_table(self.gateset, self.n)
        self.layers = bool(self.w[1] or self.w[2])
        self.want_depths = False  # compute n_layers / n_layers_cnots also when no weight reads them
        self.state = self.identity(self.B)
        self.depth = np.zeros(self.B, np.int64)
        self.success = np.zeros(self.B, bool)
        self.reward = np.zeros(self.B, np.float32)
        self.penalty = np.zeros(self.B, np.float32)
        self.inverted = np.zeros(self.B, bool)
        self._clear(np.ones(self.B, bool))

    # -- the state algebra of the kind
    def identity(self, B):
        if self.kind == "permutation":
            return np.broadcast_to(np.arange(self.n, dtype=np.int64), (B, self.n)).copy()
        d = 2 * self.n if self.kind == "clifford" else self.n
        return np.broadcast_to(np.eye(d, dtype=np.uint8), (B, d, d)).copy()

    def solved(self, state):
        return (state == self.identity(1)).reshape(len(state), int(np.prod(state.shape[1:]))).all(axis=1)

    def inverse(self, state):
        """-> (inverse, ok): Gauss-Jordan for the matrices (ok False where singular), argsort for the permutations."""
        if self.kind == "permutation":
            return np.argsort(state, axis=1, kind="stable"), (np.sort(state, axis=1) == np.arange(self.n)).all(axis=1)
        return gf2_inverse(state)

    def matmul(self, a, b):
        """The product of the states as operators: a permutation's index vector p is the matrix with a 1 at (i, p[i])."""
        return np.take_along_axis(b, a, axis=1) if self.kind == "permutation" else gf2_matmul(a, b)

    def apply(self, state, actions):
        """Left-multiply each env's state by its action's gate (out-of-range actions: unchanged); returns a new array."""
        state = state.copy()
        actions = np.asarray(actions, dtype=np.int64)
        valid = (actions >= 0) & (actions < self.A)
        a = np.where(valid, actions, 0)
        if not self.A:
            return state
        kid, qa, qb = self.kid[a], self.q0[a], self.q1[a]
        n = self.n
        for k_i, kind in enumerate(KINDS):
            sel = np.flatnonzero(valid & (kid == k_i))
            if kind in TWO_KINDS:
                sel = sel[qa[sel] != qb[sel]]  # clifford.rs:121,131,140 / linear_function.rs:60,70: no-op on one qubit twice
            if not sel.size:
                continue
            if self.kind == "clifford":
                S = SYMPLECTIC[kind][0]
                rows = np.stack([qa[sel], n + qa[sel]], 1) if kind in ONE else np.stack([qa[sel], qb[sel], n + qa[sel], n + qb[sel]], 1)
            elif kind in LINEAR:
                S = LINEAR[kind]
                rows = np.stack([qa[sel], qb[sel]], 1)
            else:
                continue  # not a gate of this env's state (LinearFunction: only CX / SWAP; Permutation: only SWAP)
            if self.kind == "permutation" and kind != "swap":
                continue
            got = state[sel[:, None], rows]  # [b, r, ...]
            if self.kind == "permutation":  # a permutation matrix S moves entry j to position i where S[i, j] = 1
                new = got[:, np.argmax(S, axis=1)]
            else:
                new = (np.einsum("ij,bj...->bi...", S.astype(np.int64), got.astype(np.int64)) & 1).astype(np.uint8)
            state[sel[:, None], rows] = new
        return state

    def state_of_circuit(self, circuits):
        """The state that replaying `circuits[b]` (action lists, equal length) solves: G(circuit)^-1."""
        circuits = np.asarray(circuits, dtype=np.int64).reshape(self.B, -1)
        g = self.identity(self.B)
        for t in range(circuits.shape[1]):
            g = self.apply(g, circuits[:, t])
        inv, ok = self.inverse(g)
        assert ok.all()
        return inv

    # -- the wire format of get_state / set_state (i64) and the dense observation
    def wire(self, state=None):
        s = self.state if state is None else state
        return s.reshape(self.B, -1).astype(np.int64)

    def from_wire(self, wire):
        wire = np.asarray(wire, dtype=np.int64).reshape(self.B, -1)
        if self.kind == "permutation":
            return wire.copy()
        d = 2 * self.n if self.kind == "clifford" else self.n
        return (wire > 0).astype(np.uint8).reshape(self.B, d, d)

    def observe(self):
        """[B, rows * cols] int8: the tableau / matrix, or the permutation's one-hot rows (permutation.rs:232-234)."""
        if self.kind == "permutation":
            return (self.state[:, :, None] == np.arange(self.n)).astype(np.int8).reshape(self.B, -1)
        return self.state.reshape(self.B, -1).astype(np.int8)

    def masks(self):
        return np.repeat(~self.success[:, None], self.A, axis=1)

    def is_final(self):
        return (self.depth == 0) | self.success

    # -- episodes
    def _clear(self, m):
        if not hasattr(self, "episode"):
            self.episode = np.full((self.B, 0), -1, np.int64)  # the valid actions stepped this episode (the metrics' prefix)
            self.sol = [[] for _ in range(self.B)]
            self.sol_inv = [[] for _ in range(self.B)]
            self.metrics = np.zeros((self.B, 4), np.int64)
        for b in np.flatnonzero(m):
            self.sol[b], self.sol_inv[b] = [], []
        self.episode[m] = -1
        self.metrics[m] = 0
        self.inverted[m] = False
        self.success[m] = self.solved(self.state[m])
        self.reward[m] = np.where(self.success[m], np.float32(1), np.float32(0))

    def set_state(self, wire, mask=None):
        m = np.ones(self.B, bool) if mask is None else np.asarray(mask, bool)
        self.state[m] = self.from_wire(wire)[m]
        self.depth[m] = self.max_depth
        self._clear(m)

    def reset_with(self, draws, mask=None):
        """Env::reset with the scramble's draws given ([n_draws, B]): gates applied to the identity, depth = slope * difficulty."""
        m = np.ones(self.B, bool) if mask is None else np.asarray(mask, bool)
        draws = np.asarray(draws, dtype=np.int64)
        draws = draws.reshape(-1 if draws.size else 0, self.B)[:, m]  # (no draws: the identity, depth 0)
        s = self.identity(int(m.sum()))
        for t in range(draws.shape[0]):
            s = self.apply(s, draws[t])
        self.state[m] = s
        self.depth[m] = min(self.depth_slope * draws.shape[0], self.max_depth)
        self._clear(m)

    def step(self, actions, coins=None):
        actions = np.asarray(actions, dtype=np.int64).reshape(self.B)
        coins = np.zeros(self.B, bool) if coins is None or not self.add_inverts else np.asarray(coins).reshape(self.B).astype(bool)
        valid = (actions >= 0) & (actions < self.A)
        self.episode = np.concatenate([self.episode, np.where(valid, actions, -1)[:, None]], axis=1)
        new = metrics_of(self.episode, self.table, self.n, depths=self.layers or self.want_depths)
        delta = (new - self.metrics).astype(np.float32)
        pen = self.w[0] * delta[:, 0] + self.w[1] * delta[:, 1] + self.w[2] * delta[:, 2] + self.w[3] * delta[:, 3]
        pen = np.where(valid, pen, np.float32(0)).astype(np.float32)
        self.penalty = pen
        self.metrics = new
        self.state = self.apply(self.state, actions)
        if self.track_solution:
            logged = valid if self.kind == "permutation" else np.ones(self.B, bool)  # permutation.rs:188-208
            for b in np.flatnonzero(logged):
                (self.sol_inv if self.inverted[b] else self.sol)[b].append(int(actions[b]) & (2**64 - 1))  # as a usize
        self.depth = np.maximum(self.depth - 1, 0)
        if coins.any():
            inv, ok = self.inverse(self.state[coins])
            if not ok.all():
                raise ValueError("singular state inverted")
            self.state[coins] = inv
            self.inverted ^= coins
        self.success = self.solved(self.state)
        self.reward = (np.where(self.success, np.float32(1), np.float32(0)) - pen).astype(np.float32)
        return self.reward, self.is_final(), self.success, self.depth

    def solutions(self):
        return [self.sol[b] + self.sol_inv[b][::-1] for b in range(self.B)]

    # -- the add_inverts invariant: M = G(s) V G(s_inv)^-1 (or its inverse while inverted)
    def product(self, seqs):
        """G(seq) for one action list per env (later gates on the left), as states."""
        g = self.identity(self.B)
        T = max((len(s) for s in seqs), default=0)
        for t in range(T):
            g = self.apply(g, np.array([s[t] if t < len(s) and s[t] < self.A else -1 for s in seqs], np.int64))  # (logged -1 is 2^64 - 1)
        return g

    def logged_state(self, start):
        """What the solution logs say the state is, given the episode's start states `start` (model states)."""
        gs, gi = self.product(self.sol), self.product(self.sol_inv)
        gi_inv, ok = self.inverse(gi)
        assert ok.all()
        m = self.matmul(self.matmul(gs, start), gi_inv)
        minv, ok = self.inverse(m)
        return np.where(self.inverted.reshape((-1,) + (1,) * (m.ndim - 1)), minv, m)
