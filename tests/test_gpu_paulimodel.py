"""Every PauliEnv kernel row the dispatcher picks (tests/test_dispatch.py) against tests/paulimodel.py, a model that shares no code
with the oracle: reward bit patterns, flags, depth, masks, observations (plain, permuted, packed), tableau and solution logs after
every step.  Each case first asserts that `plan()` routes its configuration to the kernel it means to exercise.  Device-generated
targets are checked for the facts that hold without restating the generator's random stream."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

from paulimodel import PauliModel, conjugate, micro_ops, permute_obs, to_wire  # noqa: E402
from test_dispatch import FUSED, LAYOUT, RESET_DONE, STEP, plan  # noqa: E402
from test_paulimodel import random_labels, random_tableau  # noqa: E402
from util import f32_bits, line_gateset  # noqa: E402

PLAIN = dict(add_perms=False, track_solution=False)
TRACK = dict(add_perms=False, track_solution=True)
PERMS = dict(add_perms=True, track_solution=False)
BOTH = dict(add_perms=True, track_solution=True)
INVERSE = {"s": "sdg", "sdg": "s", "sx": "sxdg", "sxdg": "sx"}
# a layer weight sets F_LAYERS, a step-kernel feature like track_solution (qgym_plan.hpp pauli_step_kernel_of): the plain and
# add_perms-only cases weigh counts only, so that they run the non-feature kernels; the solution-logging cases also pay for layers
W_COUNTS = {"n_cnots": 0.02, "n_layers_cnots": 0.0, "n_layers": 0.0, "n_gates": 0.001}
W_LAYERS = {"n_cnots": 0.02, "n_layers_cnots": 0.03, "n_layers": 0.05, "n_gates": 0.001}


def _dev(a, dtype):
    return torch.as_tensor(np.ascontiguousarray(a), device="cuda").to(dtype)


def _label(x, z, k):
    n = len(x)
    return ("-" if k == 2 else "") + "".join("IXZY"[int(x[q]) + 2 * int(z[q])] for q in range(n - 1, -1, -1))


def replay_target(m, circ, n_rot, rng, paulis=None):
    """(tableau, labels) that replaying `circ` solves: the identity tableau and n_rot signed weight-1 Paulis, conjugated by the
    circuit's inverse (reversed, S / SX and their inverses exchanged; every action's micro-op sequence is its own reverse).
    `paulis`: the weight-1 Paulis as (qubit, axis 1 X / 2 Z / 3 Y) instead of random ones."""
    n = m.n
    xs = np.zeros((n, 2 * n + n_rot), np.int64)
    zs = np.zeros((n, 2 * n + n_rot), np.int64)
    xs[:, :n], zs[:, n:2 * n] = np.eye(n, dtype=np.int64), np.eye(n, dtype=np.int64)
    if paulis is None:
        q = rng.integers(0, n, size=n_rot)
        ax = rng.integers(1, 4, size=n_rot)
    else:
        q, ax = (np.array(v, np.int64) for v in zip(*paulis))
    xs[q, 2 * n + np.arange(n_rot)] = ax & 1
    zs[q, 2 * n + np.arange(n_rot)] = ax >> 1
    ks = np.where(rng.random(n_rot) < 0.5, 2, 0)
    for a in circ[::-1]:
        kind, qs = m.gateset[a]
        for table, mq, _ in micro_ops(INVERSE.get(kind, kind), qs[0], qs[-1]):
            sign = conjugate(xs, zs, table, mq)
            ks = (ks + np.where(sign[2 * n:] < 0, 2, 0)) % 4
    tab = np.concatenate([xs[:, :2 * n], zs[:, :2 * n]]).astype(np.uint8)
    return tab, [_label(xs[:, 2 * n + r], zs[:, 2 * n + r], ks[r]) for r in range(n_rot)]


CASES = [
    # n, options, max_rotations, final_pauli_layers, batch, steps, int64 actions, layout, step kernel, fused kernel
    (20, PLAIN, 5, None, 257, 14, False, "PTILE-compact", "ptile_step1c_kernel", "ptile_fused1c_kernel"),   # BASELINE config 5
    (20, TRACK, 5, None, 1, 14, True, "PTILE-compact", "ptile_step1c_kernel", "ptile_step_kernel"),
    (5, PERMS, 5, None, 130, 14, False, "PTILE-compact", "ptile_step1c_kernel", "ptile_step_kernel"),
    (28, PLAIN, 5, None, 65, 12, True, "PTILE", "ptile_step1_kernel", "ptile_step_kernel"),
    # layout edges: the last compact / first wide qubit counts, qubit counts padded to a multiple of 4, the 32-qubit maximum
    (24, TRACK, 5, None, 100, 12, False, "PTILE-compact", "ptile_step1c_kernel", "ptile_step_kernel"),
    (24, PLAIN, 5, None, 63, 12, True, "PTILE-compact", "ptile_step1c_kernel", "ptile_fused1c_kernel"),
    (25, TRACK, 5, None, 65, 12, False, "PTILE", "ptile_step1_kernel", "ptile_step_kernel"),
    (25, PLAIN, 5, None, 66, 12, True, "PTILE", "ptile_step1_kernel", "ptile_step_kernel"),
    (21, PLAIN, 5, None, 129, 12, True, "PTILE-compact", "ptile_step1c_kernel", "ptile_fused1c_kernel"),
    (23, TRACK, 5, None, 70, 12, False, "PTILE-compact", "ptile_step1c_kernel", "ptile_step_kernel"),
    (29, PLAIN, 5, None, 66, 12, False, "PTILE", "ptile_step1_kernel", "ptile_step_kernel"),
    (32, TRACK, 5, None, 65, 12, True, "PTILE", "ptile_step1_kernel", "ptile_step_kernel"),
    (32, PLAIN, 5, None, 64, 12, False, "PTILE", "ptile_step1_kernel", "ptile_step_kernel"),
    # rotation buckets: 8 (compact), 9, 16, 17, 32; final_pauli_layers above max_rotations takes the 16- and 32-rotation bookkeeping
    (20, PLAIN, 8, 8, 130, 12, False, "PTILE-compact", "ptile_step1c_kernel", "ptile_fused1c_kernel"),
    (20, TRACK, 9, None, 65, 12, True, "PTILE", "ptile_step1_kernel", "ptile_step_kernel"),
    (20, PLAIN, 16, 16, 65, 12, False, "PTILE", "ptile_step1_kernel", "ptile_step_kernel"),
    (20, TRACK, 17, None, 65, 12, False, "PTILE", "ptile_step1_kernel", "ptile_step_kernel"),
    (12, TRACK, 32, 32, 65, 12, True, "PTILE", "ptile_step1_kernel", "ptile_step_kernel"),
    (8, TRACK, 3, 12, 100, 12, False, "PTILE", "ptile_step1_kernel", "ptile_step_kernel"),
    (8, PLAIN, 5, 20, 100, 12, True, "PTILE", "ptile_step1_kernel", "ptile_step_kernel"),
    (6, BOTH, 8, None, 100, 12, False, "PTILE", "ptile_step1_kernel", "ptile_step_kernel"),
]


def _ids(c):
    return f"n{c[0]}-r{c[2]}-f{c[3]}-{'perms' if c[1]['add_perms'] else 'track' if c[1]['track_solution'] else 'plain'}-B{c[4]}"


def _config(n, opts, max_rot, final, idx):
    """The configuration of a case, metrics weights included -- the same for plan() and the VecEnv.  The cases without a solution log
    weigh no layers: no step-kernel feature, so they run the FEAT = false one-step kernels and, where compact, ptile_fused1c_kernel."""
    # short episodes (run past max_depth) where no solution is logged: the log holds max_depth + rotations entries (qgym_api.cpp)
    short = idx % 2 and not opts["track_solution"]
    cfg = dict(opts, max_rotations=max_rot, difficulty=6, depth_slope=2, max_depth=9 if short else 128, pauli_layer_reward=0.0625,
               metrics_weights=W_LAYERS if opts["track_solution"] else W_COUNTS)
    if final is not None:
        cfg["final_pauli_layers"] = final
    return cfg


def _expect(gv, m, label, packed_ok):
    gv.sync()
    np.testing.assert_array_equal(f32_bits(gv.reward.cpu().numpy()), f32_bits(m.reward), err_msg=f"reward {label}")
    np.testing.assert_array_equal(gv.done.cpu().numpy(), m.is_final(), err_msg=f"done {label}")
    np.testing.assert_array_equal(gv.success.cpu().numpy(), m.success, err_msg=f"success {label}")
    np.testing.assert_array_equal(gv.depth.cpu().numpy(), m.depth, err_msg=f"depth {label}")
    np.testing.assert_array_equal(gv.masks().cpu().numpy(), m.masks(), err_msg=f"masks {label}")
    np.testing.assert_array_equal(gv.get_state("i64").cpu().numpy(), m.tableau(), err_msg=f"tableau {label}")
    _expect_obs(gv, m, label, packed_ok)


def _expect_obs(gv, m, label, packed_ok, rng=None):
    B = m.B
    plain = m.observe()
    got = gv.observe().cpu().numpy().reshape(B, -1)
    if not m.perms:
        np.testing.assert_array_equal(got, plain, err_msg=f"observe {label}")
        if packed_ok:
            from qiskit_gym_amd.collector import expand_packed

            packed = expand_packed(gv.observe_packed(), gv.obs_shape_[1], torch.int8)
            np.testing.assert_array_equal(packed.cpu().numpy().reshape(B, -1), plain, err_msg=f"packed {label}")
        return
    # observe() draws its own permutation: it must be one of the model's; then pin the next one with explicit draws
    rows, cols = 2 * m.n, 2 * m.n + m.max_rotations
    for b in range(B):
        dense = plain[b].reshape(rows, cols)
        assert any((permute_obs(dense, p, m.n).reshape(-1) == got[b]).all() for p in m.perms), f"observe {label} env {b}"
    draws = (rng or np.random.default_rng(0)).integers(0, 4 * len(m.perms), size=B)
    got = gv.pauli_observe(_dev(draws, torch.int32)).cpu().numpy().reshape(B, -1)
    np.testing.assert_array_equal(got, m.observe_perm(draws), err_msg=f"pauli_observe {label}")


def _expect_logs(gv, m, label):
    sol, lens = gv.solutions(cap=2048)
    want = m.solutions()
    np.testing.assert_array_equal(lens, [len(w) for w in want], err_msg=f"log lengths {label}")
    for b in range(m.B):
        assert sol[b, : lens[b]].tolist() == want[b], (label, b)


@pytest.mark.parametrize("path", ["step", "graph", "fused"])
@pytest.mark.parametrize("case", range(len(CASES)), ids=[_ids(c) for c in CASES])
def test_pauli_kernels_against_the_model(case, path):
    from qiskit_gym_amd.vec import VecEnv

    n, opts, max_rot, final, B, T, act64, layout, step_k, fused_k = CASES[case]
    gs = line_gateset("pauli", n)
    A = len(gs)
    cfg = _config(n, opts, max_rot, final, case)
    assert plan("pauli", n, STEP, batch=B, num_actions=A, **cfg) == step_k
    assert plan("pauli", n, FUSED, batch=B, arg=T, num_actions=A, **cfg) == fused_k
    assert plan("pauli", n, LAYOUT, batch=B, num_actions=A, **cfg) == layout
    rmax = final if final is not None else max_rot + 2
    gv = VecEnv("pauli", n, gs, B, **cfg)
    m = PauliModel(n, gs, B, max_rotations=max_rot, add_perms=opts["add_perms"], track_solution=opts["track_solution"],
                   max_depth=cfg["max_depth"], depth_slope=2, difficulty=6, metrics_weights=cfg["metrics_weights"], pauli_layer_reward=0.0625)
    rng = np.random.default_rng(100 * case + len(path))
    packed_ok = 2 * n + max_rot <= 64
    # even envs replay a target circuit that ends in a CX pair (a clean after the last gate); odd envs get random targets
    T0 = max(3, T // 2)
    cx = [a for a, (k, _) in enumerate(m.gateset) if k == "cx"]
    circs = rng.integers(0, A, size=(B, T0))
    circs[:, -2] = circs[:, -1] = rng.choice(cx, size=B)
    tabs, labs = [], []
    for b in range(B):
        if b % 2 == 0:
            t, l = replay_target(m, circs[b], int(rng.integers(0, rmax + 1)), rng)
        else:
            t, l = random_tableau(rng, n, int(rng.integers(0, 2 * n))), random_labels(rng, n, int(rng.integers(0, rmax + 1)), 4)
        tabs.append(t)
        labs.append(l)
    by_wire = path == "graph" or (path == "fused" and case % 2 == 0)
    if by_wire:
        wires = [to_wire(tabs[b], labs[b], scale=3) for b in range(B)]
        width = max(len(x) for x in wires)
        wires = np.array([x + [0] * (width - len(x)) for x in wires], np.int64)
        gv.set_state(wires, "i64")
        m.set_state(wires)
    else:  # (pauli_reset_from takes bare IXYZ strings)
        labs = [[x.lstrip("-") for x in l] for l in labs]
        gv.pauli_reset_from(np.stack(tabs), labs)
        m.reset_from(tabs, labs)
    _expect(gv, m, "entry", packed_ok)
    depth0 = m.depth.copy()
    adt =torch.int64 if act64 else torch.int32

    def actions(t):
        acts = rng.integers(0, A, size=B)
        if t < T0:
            acts[::2] = circs[::2, t]
            if m.perms:  # submit the action that the env's current permutation maps to the circuit's gate
                inv = np.argsort(np.asarray(m.act_perms), axis=1)
                acts[::2] = inv[m.cur[::2], circs[::2, t]]
        if t % 4 == 2 and not m.perms:
            acts[1::14] = A
            acts[3::22] = A + 3
            acts[5::26] = -1
        return acts

    never = 10 ** 6
    first, first_gpu = np.full(B, never), np.full(B, never)
    reward_at = np.zeros(B, np.float32)
    want_reward_at = np.zeros(B, np.float32)

    def model_step(acts, t):
        m.step(acts)
        hit = m.success & (first == never)
        first[hit] = t + 1
        reward_at[hit] = m.reward[hit]
        want_reward_at[hit] = (np.float32(1) - m.penalty[hit]) + np.float32(0.0625) * m.removed[hit].astype(np.float32)

    if path == "step":
        for t in range(T):
            acts = actions(t)
            model_step(acts, t)
            gv.step(_dev(acts, adt))
            _expect(gv, m, f"t={t}", packed_ok)
            if m.perms:
                _expect_obs(gv, m, f"t={t}", packed_ok, rng)
            first_gpu = np.where((gv.success.cpu().numpy() > 0) & (first_gpu == never), t + 1, first_gpu)
            if m.track_solution:
                _expect_logs(gv, m, f"t={t}")
    else:
        if m.perms:
            _expect_obs(gv, m, "before the rollout", packed_ok, rng)
        acts = np.stack([actions(t) for t in range(T)])
        rew, fin, suc = np.zeros((T, B), np.float32), np.zeros((T, B), np.uint8), np.zeros((T, B), bool)
        for t in range(T):
            model_step(acts[t], t)
            rew[t], fin[t], suc[t] = m.reward, m.is_final(), m.success
        rew_out = torch.zeros((T, B), dtype=torch.float32, device="cuda")
        fin_out = torch.zeros((T, B), dtype=torch.uint8, device="cuda")
        gv.rollout(_dev(acts, adt), fused=path == "fused", rewards_out=rew_out, dones_out=fin_out)
        gv.sync()
        np.testing.assert_array_equal(f32_bits(rew_out.cpu().numpy()), f32_bits(rew), err_msg="per-step rewards")
        np.testing.assert_array_equal(fin_out.cpu().numpy(), fin, err_msg="per-step dones")
        _expect(gv, m, "after the rollout", packed_ok)
        # the device's own first success: its first done while depth is left (a done before the depth runs out is a success)
        solved_gpu = (fin_out.cpu().numpy() > 0) & (depth0[None, :] > np.arange(1, T + 1)[:, None])
        first_gpu = np.where(solved_gpu.any(0), solved_gpu.argmax(0) + 1, never)
        for k in range(3):  # single steps on what the rollout left behind
            if m.perms:
                _expect_obs(gv, m, f"after the rollout {k}", packed_ok, rng)
            last = actions(T + k)
            m.step(last)
            gv.step(_dev(last, adt))
            _expect(gv, m, f"after the rollout, step {k}", packed_ok)
        if m.track_solution:
            _expect_logs(gv, m, "end")
    # the replaying envs solve at the step the model predicts, at or before their circuit's end, with 1 - penalty + reward * removed
    np.testing.assert_array_equal(first_gpu[::2], first[::2])
    assert (first[::2] <= T0).all() and (first[::2] < depth0[::2]).all()
    np.testing.assert_array_equal(f32_bits(reward_at[::2]), f32_bits(want_reward_at[::2]))


# ---- device-generated targets -------------------------------------------------------------------------------------------------
GEN_CASES = [
    # how, batch, finished envs, max_rotations, final_pauli_layers, path   (test_dispatch.RESETS)
    ("reset", 300, 0, 5, 5, None),
    ("reset_done", 8192, 128, 5, 5, "compact_done + ptile_reset_tree_kernel"),
    ("reset_done", 1024, 32, 5, 5, "ptile_generate_kernel"),
    ("reset_done", 8192, 64, 8, 16, "compact_done + ptile_reset_tree_kernel"),
    ("reset", 257, 0, 8, 16, None),
]


def _generated_facts(obs, tab, n, max_rot, final, label):
    """Facts of every reset env that hold whatever the generator drew: a symplectic tableau, at most final_pauli_layers visible
    rotations, and -- when every active rotation is visible -- no visible rotation of weight <= 1 in the front layer, i.e. each one
    anticommutes with another visible rotation; success iff nothing is visible and the tableau is the identity."""
    d = 2 * n
    omega = np.zeros((d, d), np.int64)
    omega[:n, n:], omega[n:, :n] = np.eye(n, dtype=np.int64), np.eye(n, dtype=np.int64)
    rot = obs[:, :, d:].astype(np.int64)  # [E, 2n, max_rot]
    visible = rot.any(axis=1)  # (a present rotation is never all zero: weight 0 would panic at the initial clean)
    t = tab.reshape(-1, d, d).astype(np.int64)
    for e in range(len(obs)):
        assert ((t[e].T @ omega @ t[e]) % 2 == omega).all(), f"{label}: tableau of env {e} is not symplectic"
        cnt = int(visible[e].sum())
        assert cnt <= min(final, max_rot) and visible[e, :cnt].all(), (label, e)  # packed to the left, in node order
        if final <= max_rot:
            x, z = rot[e, :n, :cnt], rot[e, n:, :cnt]
            comm = (x.T @ z + z.T @ x) % 2
            for c in range(cnt):
                if int((x[:, c] | z[:, c]).sum()) <= 1:
                    assert comm[c].any(), f"{label}: env {e} rotation column {c} has weight <= 1 and nothing blocks it"
    return visible.any(axis=1)


@pytest.mark.parametrize("how,B,count,max_rot,final,want", GEN_CASES)
def test_device_generated_targets(how, B, count, max_rot, final, want):
    from qiskit_gym_amd.vec import VecEnv

    n = 20
    gs = line_gateset("pauli", n)
    cfg = dict(add_perms=False, track_solution=False, max_rotations=max_rot, final_pauli_layers=final, difficulty=96, pauli_diff_scale=4,
               depth_slope=1, max_depth=128)
    if want is not None:
        assert plan("pauli", n, RESET_DONE, batch=B, arg=count, num_actions=len(gs), **cfg) == want
    gv = VecEnv("pauli", n, gs, B, **cfg)
    gv.reset(0xC0DE)
    gv.sync()
    sel = np.arange(B)
    if how == "reset_done":
        before_tab = gv.get_state("u8").cpu().numpy()
        gv.step(_dev(np.zeros(B), torch.int32))  # one H on qubit 0 everywhere: what reset_done must overwrite
        done = np.zeros(B, bool)
        sel = np.sort(np.random.default_rng(B).choice(B, size=count, replace=False))
        done[sel] = True
        gv.done.copy_(_dev(done, torch.uint8))
        gv.reset_done(0xBEEF)
        gv.sync()
        keep = ~done
        after_tab = gv.get_state("u8").cpu().numpy()
        h = before_tab[keep].reshape(-1, 2 * n, 2 * n).copy()
        h[:, [0, n]] = h[:, [n, 0]]
        np.testing.assert_array_equal(after_tab[keep].reshape(-1, 2 * n, 2 * n), h, err_msg="envs not reset changed")
    obs = gv.observe().cpu().numpy()[sel]
    tab = gv.get_state("u8").cpu().numpy()[sel]
    depth, success = gv.depth.cpu().numpy()[sel], gv.success.cpu().numpy()[sel].astype(bool)
    any_visible = _generated_facts(obs, tab, n, max_rot, final, how)
    np.testing.assert_array_equal(depth, min(96, 128), err_msg="depth = min(slope * difficulty, max_depth)")
    identity = (tab.reshape(-1, 2 * n, 2 * n) == np.eye(2 * n, dtype=np.uint8)).all(axis=(1, 2))
    if final <= max_rot:
        np.testing.assert_array_equal(success, identity & ~any_visible, err_msg="success")
    else:
        assert not (success & any_visible).any()
    assert any_visible.mean() > 0.5  # the generator did draw rotations
