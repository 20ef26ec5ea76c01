"""A PauliEnv model that shares no code with the oracle or libqgym: numpy, one Python object per env, CPU only.

Derived from physics.  A rotation is a Pauli operator (-i)^k P, P a Hermitian Pauli string (x bits, z bits; k in {0, 1, 2, 3},
k = 0 / 2 for the signed Hermitian strings every well-formed target holds).  A gate acts on it by conjugation, P -> U P U^dagger
(the Heisenberg frame of `test_physics.py`'s docstring: qiskit conventions, qubit 0 the least significant bit).  The action of each
elementary gate on the 4 (or 16) Pauli strings of the qubits it touches is computed ONCE, at import, from its 2x2 (4x4) unitary
(envmodel's matrices); a step looks the touched qubits' bits up in that table, and a -1 in the image adds 2 to k.  The tableau's
columns are Pauli strings too (x in rows 0..n-1, z in rows n..2n-1) and take the same table, without the sign.  No per-gate bit or
phase rule is written out, so Sdg and SXdg are just their own unitaries.

Restated from the reference (paths under its rust/src/; `pauli.rs` = envs/pauli.rs, `pauli_network.rs` / `pauli_dag.rs` in pauli/),
because it is not physics:
  * the wire format and the tableau (pauli_network.rs:37-77; pauli.rs:517-552): the 4n^2 tableau entries are the data matrix row by
    row (entry > 0 is a one); rotation k of the label list is column 2n + k, x bits on top of z bits;
  * labels (pauli/pauli.rs:22-81): an optional coefficient [+-]?[ij1]?, canonicalised by dropping '1' and '+' and reading j as i,
    with "" -> 0, "-i" -> 1, "-" -> 2, "i" -> 3 as the power of -i; then one of IXYZ per qubit, the LAST character on qubit 0.
    `Pauli::phase` (:125-133) reports that power after evolution, i.e. k;
  * the elementary gates of an action (pauli_network.rs:183-260): the network's `cnot(i, j)` is a CX with control j and target i
    (row ops plus evolve_cx(j, i)), followed by a clean; H, S, SX and their inverses do not clean.  CZ(a, b) is h(b); cnot(a, b);
    h(b), so its clean runs mid-gate; SWAP(a, b) is cnot(a, b); cnot(b, a); cnot(a, b) with a clean after each;
  * a two-qubit gate on one qubit twice: `xor_rows(q, q)` clears a row and `evolve_cx(q, q)` clears x_q and z_q (:183-187,
    pauli/pauli.rs:99-103) -- not a unitary.  evolve_cx leaves the group phase alone and phase() = group phase - #Y, so clearing a
    Y adds one to k.  H on both sides of CZ(q, q) follows physics;
  * triviality (pauli_network.rs:79-93): a rotation's data column has weight <= 1.  Its logged qubit is the first one it acts on,
    its axis Y where x and z are set, else X or Z (:95-137); weight 0 panics there (`unwrap` on None);
  * the DAG (pauli_dag.rs:25-57): built once from the initial rotations, an edge from each rotation to every EARLIER one it does not
    commute with; the front layer is the present nodes without an edge to a present node;
  * clean (pauli_network.rs:139-165): passes until one removes nothing; a pass takes the front layer as it stands at its start,
    walks it in node order, records and zeroes the data column of every trivial rotation, then removes those nodes.  The rotation
    itself (`rotation_qk`) is NOT removed: it keeps being conjugated by every later gate (:189-223);
  * node order: the DAG is a petgraph `Graph`, and its node order is what `active_rotation_indices` returns.  That is a library
    behaviour, not a reference rule: `retain_nodes` visits the node indices from the last to the first and `remove_node` fills the
    freed slot with the node in the last slot (a `Vec::swap_remove`);
  * solution log (pauli.rs:612-627, 685-720): the actual action, then one entry per rotation removed during the gate, in removal
    order: 0x8000_0000 | axis << 21 | qubit << 11 | original index << 1 | (0 if phase() == 2 else 1), phase() read after the WHOLE
    gate.  Out-of-range actions log nothing;
  * observation (pauli.rs:411-437): the tableau, then the first max_rotations present rotations in node order, zero-padded;
    with add_perms (pauli.rs:445-485): row i / n + i take row perm[i] / n + perm[i], then tableau column i / n + i takes column
    perm[i] / n + perm[i]; rotation columns are not moved; the next step maps its action through act_perms[perm] (:594-599), and
    an action that is no index into it panics;
  * the permutations (envs/symmetry.rs:84-176, 178-203, 307-361): the automorphisms of the coupling graph of the two-qubit gates on
    two distinct qubits -- in lexicographic order (sorted) when there is an edge; with none, every permutation in the order Heap's
    algorithm generates them.  Each is kept if every gate maps to a gate of the set (key: kind and qubits, SWAP's sorted; the last
    gate with a key wins), the action permutation being that map; when none is kept, the identity;
  * set_state (pauli.rs:517-552) keeps the first max_rotations labels, does not clean, depth = max_depth; an explicit target
    (`pauli_reset_from`, the tail of reset(), :554-586) keeps every label, cleans once, depth = min(slope * difficulty, max_depth);
  * step (pauli.rs:588-635): metrics and penalty of the actual gate, the gate, the log, depth saturating at 0, success = no node
    left and the tableau is the identity, reward = (achieved - penalty) + pauli_layer_reward * removed in f32, in that order.
    The metrics are envmodel's, recomputed from the episode prefix."""
from __future__ import annotations

import itertools

import numpy as np

from envmodel import DEFAULT_WEIGHTS, ONE, WEIGHT_KEYS, _pauli, decomposition_table, metrics_of, two


# ---- the conjugation tables, from the unitaries -----------------------------------------------------------------------------
def _image_table(u):
    """[4^k, 2k + 1] int64 for a k-qubit unitary: row idx = sum x_j << j + z_j << (k + j) holds the image's bits in the same order
    and its sign (+1 / -1) relative to the Hermitian string of those bits."""
    k = int(round(np.log2(u.shape[0])))
    strings = [(list(b[:k]), list(b[k:])) for b in itertools.product((0, 1), repeat=2 * k)]
    out = np.zeros((4 ** k, 2 * k + 1), np.int64)
    for idx in range(4 ** k):
        x, z = [(idx >> j) & 1 for j in range(k)], [(idx >> (k + j)) & 1 for j in range(k)]
        img = u @ _pauli(x, z) @ u.conj().T
        for x2, z2 in strings:
            c = np.trace(_pauli(x2, z2).conj().T @ img) / 2 ** k
            if abs(abs(c) - 1) < 1e-9:
                assert abs(c.imag) < 1e-9
                out[idx] = x2 + z2 + [1 if c.real > 0 else -1]
                break
        else:
            raise AssertionError("not a Clifford")
    return out


ONE_TABLE = {k: _image_table(u) for k, u in ONE.items()}
CNOT_TABLE = _image_table(two("cx", 1, 0, 2))  # the network's cnot(i, j) on local qubits (i, j): control j, target i


def micro_ops(kind, a, b):
    """PauliNetwork::act (pauli_network.rs:225-260): [(table, qubits, clean after)]; `None` table: cnot on one qubit twice."""
    if kind in ONE:
        return [(ONE_TABLE[kind], (a,), False)]
    cnot = lambda i, j: (CNOT_TABLE if i != j else None, (i, j), True)  # noqa: E731
    if kind == "cx":
        return [cnot(a, b)]
    if kind == "cz":
        return [(ONE_TABLE["h"], (b,), False), cnot(a, b), (ONE_TABLE["h"], (b,), False)]
    return [cnot(a, b), cnot(b, a), cnot(a, b)]


def conjugate(xs, zs, table, qubits):
    """Apply a conjugation table to Pauli strings given as bit rows xs, zs [n, C] (in place); returns the sign [C] of each image."""
    k = len(qubits)
    idx = sum(xs[q].astype(np.int64) << j for j, q in enumerate(qubits)) + sum(zs[q].astype(np.int64) << (k + j) for j, q in enumerate(qubits))
    img = table[idx]  # [C, 2k + 1]
    for j, q in enumerate(qubits):
        xs[q], zs[q] = img[:, j], img[:, k + j]
    return img[:, 2 * k]


# ---- labels, gatesets, permutations -----------------------------------------------------------------------------------------
def parse_label(label, n):
    """(x [n], z [n], k) of a label (pauli/pauli.rs:22-81); raises where the reference panics."""
    i = 0
    coeff = ""
    if i < len(label) and label[i] in "+-":
        coeff += label[i]
        i += 1
    if i < len(label) and label[i] in "ij1":
        coeff += label[i]
        i += 1
    body = label[i:]
    if any(ch not in "IXYZ" for ch in body):
        raise ValueError(f"invalid Pauli label {label!r}")
    if len(body) != n:
        raise ValueError(f"label {label!r} is not on {n} qubits")
    k = {"": 0, "-i": 1, "-": 2, "i": 3}[coeff.replace("1", "").replace("+", "").replace("j", "i")]
    x = np.array([body[n - 1 - q] in "XY" for q in range(n)], np.uint8)
    z = np.array([body[n - 1 - q] in "ZY" for q in range(n)], np.uint8)
    return x, z, k


def heap_permutations(n):
    """Every permutation of 0..n-1 in the order of Heap's algorithm (recursive form: generate k - 1 with the last element fixed,
    then k - 1 times exchange the last element with element i (k even) or element 0 (k odd) and generate again)."""
    a, out = list(range(n)), []

    def gen(k):
        if k <= 1:
            out.append(tuple(a))
            return
        gen(k - 1)
        for i in range(k - 1):
            j = i if k % 2 == 0 else 0
            a[j], a[k - 1] = a[k - 1], a[j]
            gen(k - 1)

    gen(n)
    return out


def qubit_perms(n, gateset):
    """(qubit perms, action perms) of compute_qubit_perms, by brute force over all n! orderings (small n only)."""
    gates = [(g[0].lower(), tuple(int(q) for q in g[1])) for g in gateset]
    key = lambda kind, qs: (kind, tuple(sorted(qs)) if kind == "swap" else tuple(qs))  # noqa: E731
    index = {}
    for i, (kind, qs) in enumerate(gates):
        index[key(kind, qs)] = i  # the last gate with a key wins
    adj = np.zeros((n, n), bool)
    for kind, qs in gates:
        if len(qs) == 2 and qs[0] != qs[1]:
            adj[qs[0], qs[1]] = adj[qs[1], qs[0]] = True
    if adj.any():
        cands = [p for p in itertools.permutations(range(n)) if (adj[np.ix_(p, p)] == adj).all()]  # lexicographic
    else:
        cands = heap_permutations(n)

    def act_perm(p):
        out = []
        for kind, qs in gates:
            k2 = key(kind, [p[q] for q in qs])
            if k2 not in index:
                return None
            out.append(index[k2])
        return out

    qp, ap = [], []
    for p in cands:
        a = act_perm(p)
        if a is not None:
            qp.append(list(p))
            ap.append(a)
    if not qp:
        qp, ap = [list(range(n))], [act_perm(tuple(range(n)))]
    return qp, ap


class PauliPanic(RuntimeError):
    """Where the reference panics."""


# ---- one env ----------------------------------------------------------------------------------------------------------------
class PauliNet:
    """The network of one env: tableau [2n, 2n], rotations (x, z [R, n], k [R]), present flags, node order, DAG edges."""

    def __init__(self, n, tableau, labels):
        self.n = n
        self.tab = (np.asarray(tableau).reshape(2 * n, 2 * n) > 0).astype(np.uint8)
        R = len(labels)
        self.rx, self.rz, self.rk = np.zeros((R, n), np.uint8), np.zeros((R, n), np.uint8), np.zeros(R, np.int64)
        for r, lab in enumerate(labels):
            self.rx[r], self.rz[r], self.rk[r] = parse_label(lab, n)
        sym = (self.rx.astype(np.int64) @ self.rz.T.astype(np.int64) + self.rz.astype(np.int64) @ self.rx.T.astype(np.int64)) & 1
        self.edge = np.tril(sym, -1).astype(bool)  # edge[i, j]: i > j and they anticommute (pauli_dag.rs:35-41)
        self.present = np.ones(R, bool)
        self.order = list(range(R))

    def column(self, r):
        """Data column of rotation r: its bits while present, zero once removed."""
        if not self.present[r]:
            return np.zeros(self.n, np.uint8), np.zeros(self.n, np.uint8)
        return self.rx[r], self.rz[r]

    def clean(self):
        removed = []
        while True:
            front = [r for r in self.order if not (self.edge[r] & self.present).any()]
            doomed = []
            for r in front:
                x, z = self.column(r)
                support = np.flatnonzero(x | z)
                if support.size <= 1:
                    if support.size == 0:
                        raise PauliPanic(f"rotation {r} has weight 0 in the front layer")
                    q = int(support[0])
                    removed.append((1 if x[q] and z[q] else 0 if x[q] else 2, q, r))
                    doomed.append(r)
            if not doomed:
                return removed
            for r in doomed:
                self.present[r] = False
            for i in range(len(self.order) - 1, -1, -1):  # petgraph retain_nodes: reverse visit, swap-remove
                if self.order[i] in doomed:
                    self.order[i] = self.order[-1]
                    self.order.pop()

    def act(self, kind, a, b):
        """One action's gate; returns the removed rotations [(axis, qubit, index)] in removal order."""
        n = self.n
        removed = []
        for table, qs, cleans in micro_ops(kind, a, b):
            xs = np.concatenate([self.tab[:n], self.rx.T], axis=1)
            zs = np.concatenate([self.tab[n:], self.rz.T], axis=1)
            if table is None:  # cnot(q, q): rows and bits of q cleared; a cleared Y raises phase() by one
                q = qs[0]
                self.rk = (self.rk + (xs[q, 2 * n:] & zs[q, 2 * n:])) % 4
                xs[q] = 0
                zs[q] = 0
            else:
                sign = conjugate(xs, zs, table, qs)
                self.rk = (self.rk + np.where(sign[2 * n:] < 0, 2, 0)) % 4
            self.tab = np.concatenate([xs[:, :2 * n], zs[:, :2 * n]], axis=0).astype(np.uint8)
            self.rx, self.rz = xs[:, 2 * n:].T.astype(np.uint8).copy(), zs[:, 2 * n:].T.astype(np.uint8).copy()
            if cleans:
                removed += self.clean()
        return removed

    def solved(self):
        return not self.order and (self.tab == np.eye(2 * self.n, dtype=np.uint8)).all()

    def dense(self, max_rotations):
        n = self.n
        out = np.zeros((2 * n, 2 * n + max_rotations), np.int8)
        out[:, :2 * n] = self.tab
        for i, r in enumerate(self.order[:max_rotations]):
            x, z = self.column(r)
            out[:n, 2 * n + i], out[n:, 2 * n + i] = x, z
        return out

    def signed(self, r):
        """(x, z, k) of rotation r, present or not."""
        return self.rx[r].copy(), self.rz[r].copy(), int(self.rk[r])


def permute_obs(dense, perm, n):
    p = np.concatenate([np.asarray(perm), n + np.asarray(perm)])
    out = dense[p].copy()
    out[:, :2 * n] = out[:, p]
    return out


def log_entry(axis, qubit, index, k):
    return 0x80000000 | (axis << 21) | (qubit << 11) | (index << 1) | (0 if k == 2 else 1)


# ---- the batch --------------------------------------------------------------------------------------------------------------
class PauliModel:
    """B PauliEnvs: set_state / reset_from / step / observe, outputs as arrays like tests/envmodel.Model's."""

    def __init__(self, n, gateset, batch, *, max_rotations=5, add_perms=False, track_solution=True, max_depth=128, depth_slope=2,
                 difficulty=1, metrics_weights=None, pauli_layer_reward=0.01):
        self.n, self.B = int(n), int(batch)
        self.gateset = [(g[0].lower(), tuple(int(q) for q in g[1])) for g in gateset]
        self.A = len(self.gateset)
        self.max_rotations = max(int(max_rotations), 1)
        self.track_solution = bool(track_solution)
        self.max_depth, self.depth_slope, self.difficulty = int(max_depth), int(depth_slope), int(difficulty)
        w = dict(DEFAULT_WEIGHTS)
        w.update({k: v for k, v in (metrics_weights or {}).items() if k in w})
        self.w = [np.float32(w[k]) for k in WEIGHT_KEYS]
        self.layers = bool(self.w[1] or self.w[2])
        self.plr = np.float32(pauli_layer_reward)
        self.table = decomposition_table(self.gateset, self.n)
        self.perms, self.act_perms = qubit_perms(self.n, self.gateset) if add_perms else ([], [])
        self.cur = np.zeros(self.B, np.int64)
        self.dead = np.zeros(self.B, bool)  # envs the reference would have panicked on
        eye = np.eye(2 * self.n, dtype=np.uint8)
        self.nets = [PauliNet(self.n, eye, []) for _ in range(self.B)]
        self.depth = np.ones(self.B, np.int64)
        self.success = np.array([w.solved() for w in self.nets])
        self.reward = np.where(self.success, np.float32(1), np.float32(0)).astype(np.float32)
        self.penalty = np.zeros(self.B, np.float32)
        self.removed = np.zeros(self.B, np.int64)
        self.episode = np.full((self.B, 0), -1, np.int64)
        self.metrics = np.zeros((self.B, 4), np.int64)
        self.sol = [[] for _ in range(self.B)]

    def _clear(self, m):
        for b in np.flatnonzero(m):
            self.sol[b] = []
        self.episode[m] = -1
        self.metrics[m] = 0
        self.success[m] = [self.nets[b].solved() for b in np.flatnonzero(m)]
        self.reward[m] = np.where(self.success[m], np.float32(1), np.float32(0))

    def _mask(self, mask):
        return np.ones(self.B, bool) if mask is None else np.asarray(mask, bool).reshape(self.B)

    def set_state(self, wires, mask=None):
        """The trait's Vec<i64> per env (pauli.rs:517-552)."""
        m = self._mask(mask)
        for b in np.flatnonzero(m):
            tab, labels = parse_wire(wires[b], self.n)
            self.nets[b] = PauliNet(self.n, tab, labels[:self.max_rotations])
            self.dead[b] = False
        self.depth[m] = self.max_depth
        self._clear(m)

    def reset_from(self, tableaus, labels, mask=None):
        """An explicit target: reset() with it (pauli.rs:554-586)."""
        m = self._mask(mask)
        died = []
        for b in np.flatnonzero(m):
            self.nets[b] = PauliNet(self.n, tableaus[b], list(labels[b]))
            self.dead[b] = False
            try:
                self.nets[b].clean()
            except PauliPanic:
                died.append(int(b))
                self.dead[b] = True
        self.depth[m] = min(self.depth_slope * self.difficulty, self.max_depth)
        self._clear(m & ~self.dead)
        if died:
            raise PauliPanic(died)

    def step(self, actions):
        """One step of every live env.  Where the reference panics the env dies (is never stepped again) and, after the others
        have stepped, PauliPanic names the envs that died."""
        actions = np.asarray(actions, np.int64).reshape(self.B)
        died = []
        if self.perms:
            bad = ~self.dead & ((actions < 0) | (actions >= self.A))  # act_perms[perm][action] out of bounds
            died += np.flatnonzero(bad).tolist()
            self.dead |= bad
            actual = np.array([self.act_perms[c][a] if 0 <= a < self.A else -1 for c, a in zip(self.cur, actions)], np.int64)
        else:
            actual = actions
        valid = (actual >= 0) & (actual < self.A) & ~self.dead
        self.episode = np.concatenate([self.episode, np.where(valid, actual, -1)[:, None]], axis=1)
        new = metrics_of(self.episode, self.table, self.n, depths=self.layers)
        delta = (new - self.metrics).astype(np.float32)
        pen = self.w[0] * delta[:, 0] + self.w[1] * delta[:, 1] + self.w[2] * delta[:, 2] + self.w[3] * delta[:, 3]
        self.penalty = np.where(valid, pen, np.float32(0)).astype(np.float32)
        self.metrics = new
        self.removed = np.zeros(self.B, np.int64)
        for b in np.flatnonzero(valid):
            kind, qs = self.gateset[actual[b]]
            try:
                rem = self.nets[b].act(kind, qs[0], qs[-1])
            except PauliPanic:
                died.append(int(b))
                self.dead[b] = True
                continue
            self.removed[b] = len(rem)
            if self.track_solution:
                self.sol[b].append(int(actual[b]))
                self.sol[b] += [log_entry(ax, q, r, int(self.nets[b].rk[r])) for ax, q, r in rem]
        live = ~self.dead
        self.depth[live] = np.maximum(self.depth[live] - 1, 0)
        self.success[live] = [self.nets[b].solved() for b in np.flatnonzero(live)]
        achieved = np.where(self.success, np.float32(1), np.float32(0)).astype(np.float32)
        reward = ((achieved - self.penalty) + self.plr * self.removed.astype(np.float32)).astype(np.float32)
        self.reward[live] = reward[live]
        if died:
            raise PauliPanic(sorted(died))
        return self.reward, self.is_final(), self.success, self.depth

    def is_final(self):
        return (self.depth == 0) | self.success

    def masks(self):
        return np.repeat(~self.success[:, None], self.A, axis=1)

    def observe(self):
        """[B, 2n * (2n + max_rotations)] int8: the observation without the qubit permutation."""
        return np.stack([w.dense(self.max_rotations).reshape(-1) for w in self.nets])

    def observe_perm(self, draws):
        """observe() of add_perms with the permutation draws given: perm draws[b] % count, which the next step un-permutes with."""
        self.cur = np.asarray(draws, np.int64).reshape(self.B) % len(self.perms)
        n = self.n
        return np.stack([permute_obs(w.dense(self.max_rotations), self.perms[c], n).reshape(-1) for w, c in zip(self.nets, self.cur)])

    def tableau(self):
        return np.stack([w.tab.reshape(-1).astype(np.int64) for w in self.nets])

    def active(self):
        return [list(w.order) for w in self.nets]

    def solutions(self):
        return [list(s) for s in self.sol]


def parse_wire(wire, n):
    """(tableau [2n, 2n], labels) of the Vec<i64> wire format (pauli.rs:517-537; missing values read as 0)."""
    it = iter(int(v) for v in wire)
    nxt = lambda: next(it, 0)  # noqa: E731
    count = max(nxt(), 0)
    tab = np.array([nxt() > 0 for _ in range(4 * n * n)], np.uint8).reshape(2 * n, 2 * n)
    labels = []
    for _ in range(count):
        length = max(nxt(), 0)
        chars = []
        for _ in range(length):
            c = next(it, None)
            if c is None:
                raise PauliPanic("malformed state: not enough characters for rotation string")
            chars.append(chr(c))
        labels.append("".join(chars))
    return tab, labels


def to_wire(tableau, labels, scale=1):
    out = [len(labels)] + (np.asarray(tableau, np.int64).reshape(-1) * scale).tolist()
    for lab in labels:
        out += [len(lab)] + [ord(c) for c in lab]
    return out
