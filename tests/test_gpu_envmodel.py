"""Every kernel family the dispatcher picks (tests/test_dispatch.py's rows) against tests/envmodel.py, a model that shares no code
with the oracle: states, observations, reward bit patterns, flags, depth and masks after every step, solution logs at the end.
Each case first asserts that `plan()` routes its configuration to the kernel it means to exercise."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

from envmodel import Model  # noqa: E402
from test_dispatch import DEFAULT, FUSED, OBS_DENSE, OBS_PACKED, PLAIN, RESET_DONE, RESET_DONE_STEP, STATE_I64, STEP, TRACK_DENSE, plan  # noqa: E402
from util import f32_bits, grid_gateset, line_gateset, rng_actions  # noqa: E402


def _gateset(kind, n):
    """Line (or 3 x n/3 grid) gatesets, plus the two-qubit gates on one qubit twice the env kind accepts (state no-ops that still count
    in the metrics)."""
    if kind == "permutation":
        gs = grid_gateset("permutation", 3, n // 3) if n % 3 == 0 else line_gateset("permutation", n)
    else:
        gs = line_gateset(kind, n)
    q = n // 2
    return gs + [("SWAP", (q, q))] + ([] if kind == "permutation" else [("CX", (q, q))]) + ([("CZ", (q, q))] if kind == "clifford" else [])


def _dev(a, dtype):
    return torch.as_tensor(np.ascontiguousarray(a), device="cuda").to(dtype)


def _make(kind, n, B, cfg, weights=None):
    from qiskit_gym_amd.vec import VecEnv

    gs = _gateset(kind, n)
    cfg = dict(cfg, max_depth=cfg.get("max_depth", 128))
    gv = VecEnv(kind, n, gs, B, metrics_weights=weights, **cfg)
    m = Model(kind, n, gs, B, add_inverts=cfg.get("add_inverts", True), track_solution=cfg.get("track_solution", True),
              max_depth=cfg["max_depth"], depth_slope=cfg.get("depth_slope", 2), metrics_weights=weights)
    return gs, gv, m


def _expect(gv, m, label, dense=None, full=True):
    gv.sync()
    np.testing.assert_array_equal(f32_bits(gv.reward.cpu().numpy()), f32_bits(m.reward), err_msg=f"reward {label}")
    np.testing.assert_array_equal(gv.done.cpu().numpy(), m.is_final(), err_msg=f"done {label}")
    np.testing.assert_array_equal(gv.success.cpu().numpy(), m.success, err_msg=f"success {label}")
    np.testing.assert_array_equal(gv.depth.cpu().numpy(), m.depth, err_msg=f"depth {label}")
    _expect_state(gv, m, label, dense, full)
    np.testing.assert_array_equal(gv.masks().cpu().numpy(), m.masks(), err_msg=f"masks {label}")


def _expect_state(gv, m, label, dense=None, full=True):
    from qiskit_gym_amd.collector import expand_packed

    B = gv.batch
    obs = m.observe()
    np.testing.assert_array_equal(gv.observe().cpu().numpy().reshape(B, -1), obs, err_msg=f"observe {label}")
    if full:
        np.testing.assert_array_equal(gv.get_state("i64").cpu().numpy(), m.wire(), err_msg=f"state {label}")
        packed = expand_packed(gv.observe_packed(), gv.obs_shape_[1], torch.int8)
        np.testing.assert_array_equal(packed.cpu().numpy().reshape(B, -1), obs, err_msg=f"packed {label}")
    if dense is not None:
        np.testing.assert_array_equal(dense.cpu().numpy().reshape(B, -1), obs, err_msg=f"tracked dense {label}")


def _targets(m, rng, T0, nonsymplectic=False):
    """Each env's start: the model's state of its own random target (replayed by the even envs); with `nonsymplectic`, the odd envs get
    invertible matrices that are no Clifford (random row additions), which only a Gauss-Jordan inversion handles."""
    circs = rng.integers(0, m.A, size=(m.B, T0))
    start = m.state_of_circuit(circs)
    if nonsymplectic:
        d = start.shape[1]
        for _ in range(3 * d):
            i, j = rng.integers(0, d, size=2)
            if i != j:
                start[1::2, i] ^= start[1::2, j]
    return circs, start


def _actions(m, rng, circs, t, coins_on):
    """Even envs replay their target with zero coins (then act at random); odd envs act at random, out-of-range actions included."""
    B, A = m.B, m.A
    acts = rng.integers(0, A, size=B)
    if t < circs.shape[1]:
        acts[::2] = circs[::2, t]
    if t % 4 == 2:
        acts[1::14] = A
        acts[3::22] = A + 3
        acts[5::26] = -1
    coins = rng.integers(0, 2, size=B) if coins_on else np.zeros(B, np.int64)
    coins[::2] = 0
    return acts, coins


def _replays_succeeded(first_gpu, first_model, reward_at, penalty_at, T0):
    """The replaying envs solve exactly at the step the model predicts (at or before their target's last gate), with reward 1 - penalty."""
    np.testing.assert_array_equal(first_gpu[::2], first_model[::2])
    assert (first_model[::2] <= T0).all()
    np.testing.assert_array_equal(f32_bits(reward_at[::2]), f32_bits(np.float32(1) - penalty_at[::2]))


def _expect_logs(gv, m, start, label):
    """The solution logs after a step: the model's own logs compose to its state (M = G(s) V G(s_inv)^-1, or the inverse while inverted),
    and the device's log s ++ reverse(s_inv) is the model's."""
    np.testing.assert_array_equal(m.logged_state(start), m.state, err_msg=f"log invariant {label}")
    sol, lens = gv.solutions(cap=m.max_depth)
    want = m.solutions()
    np.testing.assert_array_equal(lens, [len(w) for w in want], err_msg=f"log lengths {label}")
    for b in range(m.B):
        assert sol[b, : lens[b]].tolist() == want[b], (label, b)


STEP_CASES = [
    # kind, n, options, nonsymplectic, batch, steps, int64 actions, step kernel, fused kernel   (test_dispatch.STEPS)
    ("clifford", 16, PLAIN, 0, 4097, 12, False, "qm_step1_kernel", "qm_fused_lds_kernel"),
    ("clifford", 16, dict(PLAIN, track_solution=True), 0, 65, 14, True, "qm_step1_kernel", "qm_step_kernel"),
    ("clifford", 16, DEFAULT, 0, 1000, 14, False, "qm_inv2_kernel", "qm_step_kernel<inv>"),
    ("clifford", 16, DEFAULT, 1, 130, 12, True, "qm_step_kernel<gauss-jordan>", "qm_step_kernel<gauss-jordan>"),
    ("clifford", 5, DEFAULT, 0, 63, 16, False, "qm_inv2_kernel", "qm_step_kernel<inv>"),
    ("clifford", 24, PLAIN, 0, 65, 12, True, "q64_step1_kernel", "q64_fused_lds_kernel"),
    ("clifford", 24, DEFAULT, 0, 200, 12, False, "q64_inv2_kernel", "q64_step_kernel<inv>"),
    ("clifford", 24, DEFAULT, 1, 66, 10, True, "q64_step_kernel<gauss-jordan>", "q64_step_kernel<gauss-jordan>"),
    ("linear_function", 8, PLAIN, 0, 8192, 12, False, "word_step_kernel", "word_step_kernel"),
    ("linear_function", 24, PLAIN, 0, 1, 16, True, "qm_step1_kernel", "qm_fused_lds_kernel"),
    ("linear_function", 24, DEFAULT, 0, 300, 14, False, "lfd_step_kernel", "lfd_step_kernel"),
    ("linear_function", 48, PLAIN, 0, 65, 12, True, "q64_step1_kernel", "q64_fused_lds_kernel"),
    ("permutation", 9, PLAIN, 0, 4097, 16, False, "word_step_kernel", "word_step_kernel"),
    ("permutation", 27, PLAIN, 0, 63, 16, True, "permb_step1_kernel", "permb_step_kernel"),
    ("permutation", 27, DEFAULT, 0, 300, 16, False, "permb_step_kernel", "permb_step_kernel"),
    # the layout boundaries: the first 64-bit-row Clifford, the last 32-bit / first 64-bit LinearFunction rows, the last one-word /
    # first byte-per-entry permutation
    ("clifford", 17, PLAIN, 0, 65, 12, False, "q64_step1_kernel", "q64_fused_lds_kernel"),
    ("clifford", 17, DEFAULT, 0, 200, 12, True, "q64_inv2_kernel", "q64_step_kernel<inv>"),
    ("clifford", 17, DEFAULT, 1, 66, 10, False, "q64_step_kernel<gauss-jordan>", "q64_step_kernel<gauss-jordan>"),
    ("linear_function", 32, PLAIN, 0, 63, 12, False, "qm_step1_kernel", "qm_fused_lds_kernel"),
    ("linear_function", 33, PLAIN, 0, 65, 12, True, "q64_step1_kernel", "q64_fused_lds_kernel"),
    ("linear_function", 32, DEFAULT, 0, 100, 12, True, "lfd_step_kernel", "lfd_step_kernel"),
    ("linear_function", 33, DEFAULT, 0, 100, 12, False, "lfd_step_kernel", "lfd_step_kernel"),
    ("permutation", 16, PLAIN, 0, 4097, 16, True, "word_step_kernel", "word_step_kernel"),
    ("permutation", 17, PLAIN, 0, 65, 16, False, "permb_step1_kernel", "permb_step_kernel"),
    ("permutation", 16, DEFAULT, 0, 300, 16, False, "word_step_kernel", "word_step_kernel"),
    ("permutation", 17, DEFAULT, 0, 300, 16, True, "permb_step_kernel", "permb_step_kernel"),
]


def _step_ids(c):
    return f"{c[0]}{c[1]}-{c[7]}-{c[8]}-ns{c[3]}-B{c[4]}".replace("<", "_").replace(">", "")


@pytest.mark.parametrize("path", ["step", "graph", "fused"])
@pytest.mark.parametrize("kind,n,opts,nonsymp,B,T,act64,step_k,fused_k", STEP_CASES, ids=[_step_ids(c) for c in STEP_CASES])
def test_step_kernels_against_the_model(kind, n, opts, nonsymp, B, T, act64, step_k, fused_k, path):
    gs = _gateset(kind, n)
    A = len(gs)
    assert plan(kind, n, STEP, batch=B, nonsymplectic=nonsymp, num_actions=A, **opts) == step_k
    assert plan(kind, n, FUSED, batch=B, arg=T, nonsymplectic=nonsymp, num_actions=A, **opts) == fused_k
    _, gv, m = _make(kind, n, B, opts)
    rng = np.random.default_rng(n * 1000 + B + len(path))
    T0 = max(2, T // 2)
    circs, start = _targets(m, rng, T0, nonsymplectic=bool(nonsymp))
    m.set_state(m.wire(start))
    gv.set_state(m.wire(start))
    mode = plan(kind, n, TRACK_DENSE, batch=B, num_actions=A, **opts) if path == "step" else -3
    dense = gv.track_dense() if isinstance(mode, str) else None
    _expect(gv, m, "after set_state", dense)
    adt = torch.int64 if act64 else torch.int32
    coins_on = opts["add_inverts"]
    never = 10 ** 6
    first, first_gpu = np.full(B, never), np.full(B, never)
    reward_at, penalty_at = np.zeros(B, np.float32), np.zeros(B, np.float32)

    def model_step(a, c, t):
        nonlocal first
        m.step(a, c)
        hit = m.success & (first == never)
        first = np.where(hit, t + 1, first)
        reward_at[hit], penalty_at[hit] = m.reward[hit], m.penalty[hit]
        if opts["track_solution"]:
            np.testing.assert_array_equal(m.logged_state(start), m.state, err_msg=f"log invariant t={t}")

    if path == "step":
        for t in range(T):
            acts, coins = _actions(m, rng, circs, t, coins_on)
            model_step(acts, coins, t)
            gv.step(_dev(acts, adt), _dev(coins, torch.uint8) if coins_on else None)
            _expect(gv, m, f"t={t}", dense)
            first_gpu = np.where((gv.success.cpu().numpy() > 0) & (first_gpu == never), t + 1, first_gpu)
            if opts["track_solution"]:
                _expect_logs(gv, m, start, f"t={t}")
    else:
        acts, coins = zip(*[_actions(m, rng, circs, t, coins_on) for t in range(T)])
        acts, coins = np.stack(acts), np.stack(coins)
        rew = np.zeros((T, B), np.float32)
        fin = np.zeros((T, B), np.uint8)
        for t in range(T):
            model_step(acts[t], coins[t], t)
            rew[t], fin[t] = m.reward, m.is_final()
        rew_out = torch.zeros((T, B), dtype=torch.float32, device="cuda")
        fin_out = torch.zeros((T, B), dtype=torch.uint8, device="cuda")
        gv.rollout(_dev(acts, adt), fused=path == "fused", coins=_dev(coins, torch.uint8) if coins_on else None,
                   rewards_out=rew_out, dones_out=fin_out)
        gv.sync()
        np.testing.assert_array_equal(f32_bits(rew_out.cpu().numpy()), f32_bits(rew), err_msg="per-step rewards")
        np.testing.assert_array_equal(fin_out.cpu().numpy(), fin, err_msg="per-step dones")
        done_gpu = fin_out.cpu().numpy() > 0  # (episodes of max_depth 128 steps: done here is success)
        first_gpu = np.where(done_gpu.any(0), done_gpu.argmax(0) + 1, never)
        _expect(gv, m, "end")
    _replays_succeeded(first_gpu, first, reward_at, penalty_at, T0)
    if opts["track_solution"]:
        sol, lens = gv.solutions(cap=T + 1)
        want = m.solutions()
        assert lens.tolist() == [len(s) for s in want]
        for b in range(B):
            assert sol[b, : lens[b]].tolist() == want[b], b


def test_layer_weights_take_the_feature_kernels():
    w = {"n_cnots": 0.02, "n_layers_cnots": 0.3, "n_layers": 0.07, "n_gates": 0.0005}
    kind, n, B, T = "clifford", 16, 257, 12
    gs = _gateset(kind, n)
    assert plan(kind, n, STEP, batch=B, num_actions=len(gs), w_n_layers=0.1, **PLAIN) == "qm_step1_kernel"
    assert plan(kind, n, FUSED, batch=B, arg=T, num_actions=len(gs), w_n_layers=0.1, **PLAIN) == "qm_step_kernel"
    _, gv, m = _make(kind, n, B, PLAIN, weights=w)
    _, fv, _ = _make(kind, n, B, PLAIN, weights=w)
    rng = np.random.default_rng(1)
    circs, start = _targets(m, rng, 6)
    for h in (m, gv, fv):
        h.set_state(m.wire(start))
    acts = np.stack([_actions(m, rng, circs, t, False)[0] for t in range(T)])
    rew = np.zeros((T, B), np.float32)
    for t in range(T):
        m.step(acts[t])
        rew[t] = m.reward
        gv.step(_dev(acts[t], torch.int32))
        _expect(gv, m, f"t={t}")
    rew_out = torch.zeros((T, B), dtype=torch.float32, device="cuda")
    fv.rollout(_dev(acts, torch.int32), fused=True, rewards_out=rew_out)
    fv.sync()
    np.testing.assert_array_equal(f32_bits(rew_out.cpu().numpy()), f32_bits(rew))


def _draws(seed, envs, B, diff, A):
    """rng_actions of the listed envs only, scattered into [diff, B]."""
    out = np.zeros((diff, B), np.int64)
    if len(envs):
        out[:, envs] = rng_actions(seed, np.asarray(envs), diff, A)
    return out


RESET_CASES = [
    # kind, n, batch, difficulty, finished envs -> scramble path   (test_dispatch.RESETS)
    ("clifford", 16, 65536, 256, 512, "scramble_tree"),
    ("clifford", 16, 65536, 256, 4097, "scramble_flat"),
    ("clifford", 16, 65536, 63, 512, "scramble_coop"),
    ("clifford", 16, 1024, 256, 1024, "scramble_tree"),
    ("clifford", 16, 63, 256, 1, "scramble_flat"),
    ("linear_function", 12, 65536, 256, 512, "scramble_tree"),
    ("clifford", 24, 65536, 256, 512, "scramble_tree64"),
    ("clifford", 24, 65536, 32, 4000, "scramble_flat"),
    ("linear_function", 8, 65536, 64, 512, "word_init_kernel"),
    ("permutation", 9, 65536, 16, 512, "word_init_kernel"),
    ("permutation", 27, 65536, 64, 512, "init_kernel"),
]


@pytest.mark.parametrize("kind,n,B,diff,count,want", RESET_CASES)
def test_reset_done_paths_against_the_model(kind, n, B, diff, count, want):
    cfg = dict(difficulty=diff, add_perms=False, track_solution=False, add_inverts=False, depth_slope=2)
    gs = _gateset(kind, n)
    A = len(gs)
    assert plan(kind, n, RESET_DONE, batch=B, arg=count, num_actions=A, **cfg) == want
    _, gv, m = _make(kind, n, B, cfg)
    rng = np.random.default_rng(B + count + diff)
    start = m.product(rng.integers(0, A, size=(B, 4)).tolist())  # (a start the set_state can carry cheaply for 65 536 envs)
    m.set_state(m.wire(start))
    gv.set_state(m.wire(start), fmt="i64" if kind == "permutation" else "u8")
    m.reset_with(_draws(1, np.flatnonzero(m.is_final()), B, diff, A), mask=m.is_final())
    gv.reset_done(1)  # (an env whose start happens to be solved is final: it is reset here)
    done = np.zeros(B, bool)
    done[rng.choice(B, size=count, replace=False)] = True
    gv.done.copy_(_dev(done, torch.uint8))  # the caller ends these episodes
    seed = 77 + diff
    gv.reset_done(seed)
    m.reset_with(_draws(seed, np.flatnonzero(done), B, diff, A), mask=done)
    small = B <= 4097
    _expect_state(gv, m, "after reset_done", full=small)
    for t in range(2):
        acts = rng.integers(0, A, size=B)
        m.step(acts)
        gv.step(_dev(acts, torch.int32))
        gv.sync()
        np.testing.assert_array_equal(f32_bits(gv.reward.cpu().numpy()), f32_bits(m.reward), err_msg=f"reward t={t}")
        np.testing.assert_array_equal(gv.done.cpu().numpy(), m.is_final(), err_msg=f"done t={t}")
        np.testing.assert_array_equal(gv.depth.cpu().numpy(), m.depth, err_msg=f"depth t={t}")
    _expect_state(gv, m, "end", full=small)


def test_reset_and_reset_with_against_the_model():
    kind, n, B, diff = "clifford", 16, 4097, 40
    cfg = dict(difficulty=diff, add_perms=False, track_solution=True, add_inverts=True)
    gs = _gateset(kind, n)
    _, gv, m = _make(kind, n, B, cfg)
    gv.reset(5)
    m.reset_with(rng_actions(5, B, diff, len(gs)))
    _expect(gv, m, "reset(seed)")
    draws = np.random.default_rng(2).integers(0, len(gs), size=(diff, B))
    gv.reset_with(_dev(draws, torch.int32))
    m.reset_with(draws)
    _expect(gv, m, "reset_with")


RDS_CASES = [
    # kind, n, options, difficulty, num_actions override -> one-launch kernel   (test_dispatch.test_reset_done_step_in_one_launch)
    ("clifford", 16, PLAIN, 256, "qm_reset_step_kernel"),
    ("linear_function", 24, PLAIN, 256, "qm_reset_step_kernel"),
    ("clifford", 24, PLAIN, 256, "q64_reset_step_kernel"),
    ("linear_function", 40, PLAIN, 256, "q64_reset_step_kernel"),
    ("clifford", 16, DEFAULT, 256, "qm_reset_inv2_step_kernel"),
    ("clifford", 7, DEFAULT, 256, "qm_reset_inv2_step_kernel"),
    ("linear_function", 8, PLAIN, 64, "word_reset_step_kernel"),
    ("linear_function", 8, DEFAULT, 64, "word_reset_step_kernel"),
    ("permutation", 9, DEFAULT, 16, "word_reset_step_kernel"),
]


@pytest.mark.parametrize("kind,n,opts,diff,want", RDS_CASES)
def test_reset_done_step_kernels_against_the_model(kind, n, opts, diff, want):
    B, T = 1000, 14
    cfg = dict(opts, difficulty=diff, max_depth=5, depth_slope=2)
    gs = _gateset(kind, n)
    A = len(gs)
    assert str(plan(kind, n, RESET_DONE_STEP, batch=B, num_actions=A, **cfg)).startswith(want)
    _, gv, m = _make(kind, n, B, cfg)
    rng = np.random.default_rng(n + diff)
    circs, start = _targets(m, rng, 3)
    m.set_state(m.wire(start))
    gv.set_state(m.wire(start))
    coins_on = opts["add_inverts"]
    for t in range(T):  # episodes end on success (the replaying envs) or at depth 0: 5 steps, max_depth, also after a reset
        acts, coins = _actions(m, rng, circs, t, coins_on)
        seed = 300 + t
        done = m.is_final()
        m.reset_with(_draws(seed, np.flatnonzero(done), B, diff, A), mask=done)
        m.step(acts, coins)
        gv.reset_done_step(seed, _dev(acts, torch.int32), _dev(coins, torch.uint8) if coins_on else None)
        _expect(gv, m, f"t={t}", full=t == T - 1)
    if opts["track_solution"]:
        sol, lens = gv.solutions(cap=T + 1)
        want_s = m.solutions()
        for b in range(B):
            assert sol[b, : lens[b]].tolist() == want_s[b], b


OBS_CASES = [
    # kind, n, options, batch, dense observation path, packed path, i64 state path   (test_dispatch.test_observation_and_state_paths)
    ("clifford", 16, PLAIN, 64, "qm_dense_stream_kernel", "qm_pack_kernel", "row words / bit stream + streaming kernel"),
    ("clifford", 8, PLAIN, 63, "qm_dense_stream_kernel", None, "init / export kernel"),
    ("clifford", 5, PLAIN, 65, "qm_dense_stream_any_kernel", None, None),
    ("clifford", 12, PLAIN, 100, "qm_dense_stream_any_kernel", None, None),
    ("linear_function", 9, PLAIN, 65, "qm_dense_stream_any_kernel", None, None),
    ("linear_function", 32, PLAIN, 65, "qm_dense_stream_kernel", None, None),
    ("linear_function", 16, PLAIN, 65, "qm_dense_stream_kernel", None, None),
    ("clifford", 24, PLAIN, 63, "row words + expand", "export_kernel", "init / export kernel"),
    ("clifford", 24, PLAIN, 64, "row words + expand", "export_kernel", "row words / bit stream + streaming kernel"),
    ("linear_function", 24, DEFAULT, 64, "row words + expand", None, "row words / bit stream + streaming kernel"),
    ("linear_function", 8, PLAIN, 65, None, None, "init / export kernel"),
]


@pytest.mark.parametrize("kind,n,opts,B,dense_k,packed_k,state_k", OBS_CASES)
def test_observation_paths_against_the_model(kind, n, opts, B, dense_k, packed_k, state_k):
    gs = _gateset(kind, n)
    A = len(gs)
    for op, k in ((OBS_DENSE, dense_k), (OBS_PACKED, packed_k), (STATE_I64, state_k)):
        if k is not None:
            assert plan(kind, n, op, batch=B if op == STATE_I64 else 65536, num_actions=A, **opts) == k
    _, gv, m = _make(kind, n, B, opts)
    rng = np.random.default_rng(n + B)
    mode = plan(kind, n, TRACK_DENSE, batch=B, num_actions=A, **opts)
    dense = gv.track_dense() if isinstance(mode, str) else None
    circs, start = _targets(m, rng, 5)
    m.set_state(m.wire(start))
    gv.set_state(m.wire(start))
    _expect(gv, m, "set_state", dense)
    for t in range(4):
        acts, coins = _actions(m, rng, circs, t, opts["add_inverts"])
        m.step(acts, coins)
        gv.step(_dev(acts, torch.int32), _dev(coins, torch.uint8) if opts["add_inverts"] else None)
        _expect(gv, m, f"t={t}", dense)
