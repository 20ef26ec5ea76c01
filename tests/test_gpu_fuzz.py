import os
"""Randomised parity: arbitrary gatesets (any of the eight gate kinds on any qubit pair, repeated
gates, two-qubit gates on equal qubits, gates an env ignores), random option / weight / depth
combinations and batch sizes, stepped against the CPU oracle.  Every case is seeded."""
import numpy as np
import pytest

SEED_OFFSET = int(os.environ.get("QGYM_FUZZ_SEED_OFFSET", "0"))  # soak runs: shift every case to fresh seeds
pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")

from logcap_model import PushRecorder, reported  # noqa: E402
from oracle import OracleEnv  # noqa: E402
from test_gpu_pauli import random_labels, random_tableau  # noqa: E402
from util import f32_bits, make_pair  # noqa: E402

KINDS_1Q = ["H", "S", "Sdg", "SX", "SXdg"]
KINDS_2Q = ["CX", "CZ", "SWAP"]

# (env kind, qubit counts that between them reach every kernel family)
SIZES = {
    "clifford": [1, 2, 3, 7, 8, 9, 12, 16, 17, 24, 32],
    "linear_function": [1, 2, 5, 8, 9, 13, 16, 17, 32, 33, 50, 64],
    "permutation": [1, 2, 6, 9, 16, 17, 31, 32, 33, 64, 100, 200],
}


def random_gateset(rng, n, size, allow_equal=True):
    gs = []
    for _ in range(size):
        if n == 1 or rng.random() < 0.4:
            gs.append((KINDS_1Q[rng.integers(5)], (int(rng.integers(n)),)))
        else:
            a, b = int(rng.integers(n)), int(rng.integers(n))
            if a == b and not (allow_equal and rng.random() < 0.5):
                b = (a + 1 + int(rng.integers(n - 1))) % n
            gs.append((KINDS_2Q[rng.integers(3)], (a, b)))
    return gs


def random_weights(rng):
    pick = rng.integers(4)
    if pick == 0:
        return None  # reference defaults
    if pick == 1:
        return {"n_cnots": 0.0, "n_layers_cnots": 0.0, "n_layers": 0.0, "n_gates": 0.0}
    if pick == 2:
        return {"n_cnots": float(rng.random()), "n_gates": float(rng.random() * 0.01)}
    return {k: float(np.float32(rng.random() * 0.3)) for k in ("n_cnots", "n_layers_cnots", "n_layers", "n_gates")}


def _case(seed):
    rng = np.random.default_rng(seed)
    kind = ["clifford", "linear_function", "permutation"][seed % 3]
    n = int(rng.choice(SIZES[kind]))
    gs = random_gateset(rng, n, int(rng.integers(1, 41)))
    cfg = dict(add_inverts=bool(rng.integers(2)), add_perms=False, track_solution=bool(rng.integers(2)),
               max_depth=int(rng.integers(1, 60)), depth_slope=int(rng.integers(1, 4)), difficulty=int(rng.integers(1, 12)))
    w = random_weights(rng)
    if w is not None:
        cfg["metrics_weights"] = w
    batch = int(rng.choice([1, 2, 63, 64, 65, 200, 257]))
    return rng, kind, n, gs, cfg, batch


@pytest.mark.parametrize("seed", range(150))
def test_random_gatesets_and_options(seed):
    seed += SEED_OFFSET
    rng, kind, n, gs, cfg, batch = _case(seed)
    A = len(gs)
    ov, gv = make_pair(kind, n, gs, batch, **cfg)
    draws = rng.integers(0, A, size=(cfg["difficulty"], batch))
    ov.reset_with(draws)
    gv.reset_with(torch.as_tensor(draws, device="cuda", dtype=torch.int32).reshape(cfg["difficulty"], batch))
    gv.sync()
    per_env = {"clifford": 4 * n * n, "linear_function": n * n, "permutation": n}[kind]
    label = f"seed={seed} {kind} n={n} A={A} B={batch} {cfg}"
    np.testing.assert_array_equal(gv.get_state("i64").cpu().numpy(), ov.get_state(per_env), err_msg=f"reset state {label}")
    np.testing.assert_array_equal(gv.depth.cpu().numpy(), [ov.env(i).depth() for i in range(batch)], err_msg=f"reset depth {label}")
    # free-running past is_final; a tracked env can log the max_depth steps an episode lasts
    n_steps = min(30, cfg["max_depth"]) if cfg["track_solution"] else 30
    for t in range(n_steps):
        acts = rng.integers(-1, A + 1, size=batch)  # includes both kinds of invalid action
        coins = rng.integers(0, 2, size=batch)
        r_o, s_o, f_o, d_o = ov.step(acts, coins)
        gv.step(torch.as_tensor(acts, device="cuda", dtype=torch.int64), torch.as_tensor(coins, device="cuda", dtype=torch.uint8))
        gv.sync()
        np.testing.assert_array_equal(f32_bits(gv.reward.cpu().numpy()), f32_bits(r_o), err_msg=f"reward t={t} {label}")
        np.testing.assert_array_equal(gv.success.cpu().numpy(), s_o, err_msg=f"success t={t} {label}")
        np.testing.assert_array_equal(gv.done.cpu().numpy(), f_o, err_msg=f"is_final t={t} {label}")
        np.testing.assert_array_equal(gv.depth.cpu().numpy(), d_o, err_msg=f"depth t={t} {label}")
    np.testing.assert_array_equal(gv.get_state("i64").cpu().numpy(), ov.get_state(per_env), err_msg=f"end state {label}")
    np.testing.assert_array_equal(gv.observe().cpu().numpy().reshape(batch, -1), ov.observe_dense(), err_msg=f"obs {label}")
    if cfg["track_solution"]:
        for e in {0, batch // 2, batch - 1}:
            assert gv.solution(e) == ov.env(e).solution(), (label, e)


@pytest.mark.parametrize("seed", range(40))
def test_random_pauli_networks(seed):
    from qiskit_gym_amd.vec import VecEnv

    seed += SEED_OFFSET
    rng = np.random.default_rng(1000 + seed)
    n = int(rng.choice([2, 3, 5, 8, 13, 20, 24, 25, 32]))
    gs = random_gateset(rng, n, int(rng.integers(2, 36)), allow_equal=False)
    pairs = [g[1] for g in gs if len(g[1]) == 2] or [(0, 1)]
    max_rot = int(rng.integers(1, 9)) if rng.random() < 0.7 else int(rng.integers(9, 31))  # > 16 rotations: the 32-rotation kernels
    final_layers = None if rng.random() < 0.5 else int(rng.integers(1, 33))
    rmax = final_layers if final_layers is not None else max_rot + 2
    cfg = dict(add_perms=False, track_solution=bool(rng.integers(2)), max_rotations=max_rot, max_depth=int(rng.integers(4, 80)),
               difficulty=int(rng.integers(1, 20)), pauli_layer_reward=float(np.float32(rng.random() * 0.05)))
    if final_layers is not None:
        cfg["final_pauli_layers"] = final_layers
    w = random_weights(rng)
    if w is not None:
        cfg["metrics_weights"] = w
    batch = int(rng.choice([1, 64, 70, 150]))
    label = f"seed={seed} n={n} A={len(gs)} B={batch} {cfg}"
    gv = VecEnv("pauli", n, gs, batch, **cfg)
    envs = [OracleEnv("pauli", n, gs, **cfg) for _ in range(batch)]
    tabs, labs = [], []
    for e in range(batch):
        t = random_tableau(rng, n, int(rng.integers(0, 3 * n)), pairs)
        l = random_labels(rng, n, int(rng.integers(0, rmax + 1)), max_weight=min(4, n))
        envs[e].pauli_reset_from(t, l)
        tabs.append(t)
        labs.append(l)
    gv.pauli_reset_from(np.stack(tabs), labs)
    gv.sync()
    n_steps = min(36, cfg["max_depth"]) if cfg["track_solution"] else 36
    for t in range(n_steps):
        acts = rng.integers(-1, len(gs) + 1, size=batch)
        for o, a in zip(envs, acts):
            o.step(int(a))
        gv.step(torch.as_tensor(acts, device="cuda", dtype=torch.int32))
        gv.sync()
        np.testing.assert_array_equal(f32_bits(gv.reward.cpu().numpy()), np.array([o.reward_bits() for o in envs], dtype=np.uint32), err_msg=f"reward t={t} {label}")
        np.testing.assert_array_equal(gv.done.cpu().numpy(), [int(o.is_final()) for o in envs], err_msg=f"final t={t} {label}")
        np.testing.assert_array_equal(gv.depth.cpu().numpy(), [o.depth() for o in envs], err_msg=f"depth t={t} {label}")
    if not cfg["track_solution"]:  # a fused rollout on top (T steps in one launch: LDS-resident tile on the compact layout, registers otherwise)
        T = 10
        acts = rng.integers(-1, len(gs) + 1, size=(T, batch))
        rew = torch.zeros((T, batch), dtype=torch.float32, device="cuda")
        fin = torch.zeros((T, batch), dtype=torch.uint8, device="cuda")
        gv.rollout(torch.as_tensor(acts, device="cuda", dtype=torch.int32), fused=True, rewards_out=rew, dones_out=fin)
        gv.sync()
        want_r, want_f = np.zeros((T, batch), np.uint32), np.zeros((T, batch), np.uint8)
        for t in range(T):
            for e, o in enumerate(envs):
                o.step(int(acts[t, e]))
                want_r[t, e], want_f[t, e] = o.reward_bits(), o.is_final()
        np.testing.assert_array_equal(f32_bits(rew.cpu().numpy()), want_r, err_msg=f"fused rewards {label}")
        np.testing.assert_array_equal(fin.cpu().numpy(), want_f, err_msg=f"fused finals {label}")
    np.testing.assert_array_equal(gv.observe().cpu().numpy(), np.stack([o.dense_obs() for o in envs]), err_msg=f"obs {label}")
    np.testing.assert_array_equal(gv.get_state("i64").cpu().numpy(), np.stack([o.get_state() for o in envs]), err_msg=f"state {label}")
    if cfg["track_solution"]:
        for e in {0, batch - 1}:
            assert gv.solution(e) == envs[e].solution(), (label, e)


@pytest.mark.parametrize("seed", range(16))
def test_random_pauli_reset_done_as_trees(seed):
    """qg_vec_reset_done of PauliEnv on random sizes, couplings and generator settings: a short list of finished envs (a workgroup per env: the
    label generator as ballots over a wave, the tableau scramble as a tree) against the same envs regenerated with many others finished beside
    them (one lane per env: the serial generator) and, for a few, against the oracle."""
    from qiskit_gym_amd.vec import VecEnv

    seed += SEED_OFFSET
    rng = np.random.default_rng(7000 + seed)
    n = int(rng.choice([4, 7, 12, 16, 20, 24, 27, 32]))
    gs = random_gateset(rng, n, int(rng.integers(6, 60)), allow_equal=False)
    if not any(g[0] == "CX" for g in gs):
        gs.append(("CX", (0, 1)))  # the tableau scramble draws from the gateset's CX gates
    max_rot = int(rng.choice([1, 3, 5, 8, 12, 20, 30]))
    cfg = dict(add_perms=False, track_solution=False, max_rotations=max_rot, difficulty=int(rng.choice([64, 65, 100, 128, 200, 256])),
               pauli_diff_scale=int(rng.choice([1, 4, 8, 16, 50])), num_qubits_decay=float(np.float32(rng.choice([0.0, 0.3, 0.5, 0.9]))), max_depth=300)
    B = int(rng.choice([4160, 6000, 8192]))  # lists are compacted above 4 096 envs
    few, many = int(rng.integers(1, B // 32 + 1)), B // 8
    label = f"seed={seed} n={n} A={len(gs)} B={B} few={few} {cfg}"
    a, b = VecEnv("pauli", n, gs, B, **cfg), VecEnv("pauli", n, gs, B, **cfg)
    a.reset(seed)
    b.reset(seed)
    perm = rng.permutation(B)
    listed, extra = np.sort(perm[:few]), perm[few:few + many]
    for h, idx in ((a, listed), (b, np.concatenate([listed, extra]))):
        h.done.zero_()
        h.done[torch.as_tensor(idx, device="cuda")] = 1
    a.reset_done(900 + seed)   # <= B / 32 finished: trees
    b.reset_done(900 + seed)   # > B / 32: one lane per env
    a.sync()
    b.sync()
    li = torch.as_tensor(listed, device="cuda")
    oa, ob = a.observe(), b.observe()
    assert torch.equal(oa[li], ob[li]), label
    for name in ("depth", "done", "success"):
        assert torch.equal(getattr(a, name)[li], getattr(b, name)[li]), (name, label)
    assert torch.equal(a.reward[li].view(torch.int32), b.reward[li].view(torch.int32)), label
    for e in listed[:3]:
        o = OracleEnv("pauli", n, gs, **cfg)
        o.pauli_reset_seeded(900 + seed, int(e))
        np.testing.assert_array_equal(oa[int(e)].cpu().numpy(), o.dense_obs(), err_msg=label)


@pytest.mark.parametrize("seed", range(40))
def test_random_auto_reset_loops_with_tracked_observations(seed):
    """Random interleavings of the calls a collection loop makes -- step, reset_done, reset_done_step (one launch), whole resets, rollouts --
    on random gatesets and sizes of the 32-bit-row layout, with and without a tracked dense observation, against a twin handle that only uses
    the plain calls (step + reset_done + observe) and, for the first envs, against the oracle: flags, depths, reward bits after every call,
    states and observations at the end."""
    from qiskit_gym_amd._lib import QGymError
    from qiskit_gym_amd.vec import VecEnv

    seed += SEED_OFFSET + 5000
    rng = np.random.default_rng(seed)
    kind = ["clifford", "linear_function"][seed % 2]
    n = int(rng.choice([3, 8, 12, 16] if kind == "clifford" else [9, 16, 24, 32]))
    gs = random_gateset(rng, n, int(rng.integers(2, 30)), allow_equal=False)
    A = len(gs)
    B = int(rng.choice([64, 130, 257, 1024, 4096]))
    diff = int(rng.choice([1, 2, 5, 70]))
    cfg = dict(add_inverts=False, add_perms=False, track_solution=bool(rng.integers(2)), difficulty=diff, depth_slope=int(rng.integers(1, 3)),
               max_depth=int(rng.integers(2, 9)))
    a, twin = VecEnv(kind, n, gs, B, **cfg), VecEnv(kind, n, gs, B, **cfg)
    trackable = (2 * n if kind == "clifford" else n) in (16, 32)
    dense = a.track_dense() if trackable and rng.integers(2) else None
    ne = min(B, 96)
    envs = [OracleEnv(kind, n, gs, **{k: int(v) for k, v in cfg.items()}) for _ in range(ne)]
    label = f"seed={seed} {kind} n={n} A={A} B={B} {cfg} dense={dense is not None}"

    # the solution log's pushes of every env's current episode (tests/logcap_model.py): a plain step on a finished env may push past the
    # max_depth entries the log holds, which drops the entry and sets status bit 8 until the env is reset
    rec = PushRecorder(kind, B, A)
    cap = cfg["max_depth"]

    def oracle_reset(seed_, only_done):
        from util import rng_actions
        d = rng_actions(seed_, ne, diff, A)
        for e, o in enumerate(envs):
            if not only_done or o.is_final():
                o.reset_with(d[:, e])
        rec.clear(finished if only_done else None)

    def oracle_step(actions):
        for o, x in zip(envs, actions[:ne]):
            o.step(int(x), 0)
        rec.note(actions)

    def compare(what):
        want = rec.expected_faults(cap) if cfg["track_solution"] else np.zeros(B, np.uint32)
        for h in (a, twin):
            np.testing.assert_array_equal(h.faults(), want, err_msg=f"status words {what} {label}")
            if want.any():
                with pytest.raises(QGymError, match="solution log overflow"):
                    h.sync()
            else:
                h.sync()
        assert torch.equal(a.reward.view(torch.int32), twin.reward.view(torch.int32)) and torch.equal(a.done, twin.done), (what, label)
        assert torch.equal(a.depth, twin.depth) and torch.equal(a.success, twin.success), (what, label)
        np.testing.assert_array_equal(f32_bits(a.reward.cpu().numpy()[:ne]), np.array([o.reward_bits() for o in envs], dtype=np.uint32), err_msg=f"{what} {label}")
        np.testing.assert_array_equal(a.done.cpu().numpy()[:ne].astype(bool), [o.is_final() for o in envs], err_msg=f"{what} {label}")

    a.reset(seed)
    twin.reset(seed)
    oracle_reset(seed, False)
    for t in range(40):
        op = int(rng.integers(10))
        acts = rng.integers(-1, A + 1, size=B)
        ta = torch.as_tensor(acts, device="cuda", dtype=torch.int64 if t % 2 else torch.int32)
        s2 = int(rng.integers(1 << 30))
        finished = a.done.cpu().numpy().astype(bool)  # (the envs a reset_done resets: equal to the twin's and, for the first envs, the oracle's)
        if op < 5:  # the collection loop's pair, as one call
            a.reset_done_step(s2, ta)
            twin.reset_done(s2)
            twin.step(ta)
            oracle_reset(s2, True)
            oracle_step(acts)
        elif op < 7:  # the two calls
            for h in (a, twin):
                h.reset_done(s2)
                h.step(ta)
            oracle_reset(s2, True)
            oracle_step(acts)
        elif op == 7:  # a plain step (finished envs keep stepping: the trait allows it); a full log drops the entry and reports it
            for h in (a, twin):
                h.step(ta)
            oracle_step(acts)
        elif op == 8:  # everybody starts over
            for h in (a, twin):
                h.reset(s2)
            oracle_reset(s2, False)
        else:  # a graph rollout of three steps after a reset_done
            if cfg["track_solution"] and cfg["max_depth"] < 4:
                continue
            seq = rng.integers(0, A, size=(3, B))
            tseq = torch.as_tensor(seq, device="cuda", dtype=torch.int32)
            for h in (a, twin):
                h.reset(s2)
                h.rollout(tseq)
            oracle_reset(s2, False)
            for k in range(3):
                oracle_step(seq[k])
        compare(f"t={t} op={op}")
        if dense is not None:
            assert torch.equal(dense, twin.observe()), (t, op, label)
    assert torch.equal(a.get_state("packed"), twin.get_state("packed")), label
    np.testing.assert_array_equal(a.get_state("i64").cpu().numpy()[:ne], np.stack([o.get_state() for o in envs]), err_msg=label)
    if cfg["track_solution"]:
        kept = rec.expected_log(cap)
        for e in (0, ne - 1):  # (no add_inverts here: the entries a full log keeps are the first `cap` of the reference's list)
            assert a.solution(e) == [reported(x, kind) for x in envs[e].solution()[:cap]] == twin.solution(e) == kept[e], (label, e)
