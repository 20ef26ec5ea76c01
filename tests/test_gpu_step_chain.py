"""The one-step kernel of the TILE layout (qm_step1_kernel) after its chain of dependent memory round trips was shortened: constant
workgroup size, front-of-chain arguments as leading kernel parameters, an unconditional (clamped) gate-entry load, both action widths
without a branch that waits, one store phase.  Every case is bit-exact against the CPU oracle: reward bit patterns, success, is_final,
depth, final state and observation.  Shapes are the smallest at which that code can go wrong (ragged grids around the 64-lane wave and
the 256-thread workgroup), not the workload's."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

from util import f32_bits, line_gateset, make_pair  # noqa: E402

PLAIN = dict(add_inverts=False, add_perms=False, track_solution=False)
I32_MIN, I32_MAX = -(2**31), 2**31 - 1


def _dev(a, dtype):
    return torch.as_tensor(np.ascontiguousarray(a), device="cuda").to(dtype)


def _per_env(kind, n):
    return {"clifford": 4 * n * n, "linear_function": n * n}[kind]


def _scramble(ov, gv, rng, n_draws, A):
    draws = rng.integers(0, A, size=(n_draws, gv.batch))
    ov.proto.difficulty = n_draws
    for i in range(ov.batch):
        ov.env(i).difficulty = n_draws
    gv.difficulty = n_draws
    ov.reset_with(draws)
    gv.reset_with(_dev(draws, torch.int32))
    return draws


def _for_oracle(acts):
    """The oracle steps int32 actions.  A value that fits goes in as it is; one that does not (int64 edge values) goes in as -1: every
    out-of-range action is the same no-op to an env that keeps no solution log."""
    acts = np.asarray(acts, dtype=np.int64)
    return np.where((acts >= I32_MIN) & (acts <= I32_MAX), acts, -1).astype(np.int32)


def _same_outputs(gv, want, label):
    r_o, s_o, f_o, d_o = want
    gv.sync()
    np.testing.assert_array_equal(f32_bits(gv.reward.cpu().numpy()), f32_bits(r_o), err_msg=f"reward {label}")
    np.testing.assert_array_equal(gv.success.cpu().numpy(), s_o, err_msg=f"success {label}")
    np.testing.assert_array_equal(gv.done.cpu().numpy(), f_o, err_msg=f"is_final {label}")
    np.testing.assert_array_equal(gv.depth.cpu().numpy(), d_o, err_msg=f"depth {label}")


def _same_state(ov, gv, kind, n, label):
    np.testing.assert_array_equal(gv.get_state("i64").cpu().numpy(), ov.get_state(_per_env(kind, n)), err_msg=f"state {label}")
    np.testing.assert_array_equal(gv.observe().cpu().numpy().reshape(gv.batch, -1), ov.observe_dense(), err_msg=f"obs {label}")


def _step_both(ov, gv, acts, A, dtype=torch.int32, label=""):
    want = ov.step(_for_oracle(acts))
    gv.step(_dev(acts, dtype))
    _same_outputs(gv, want, label)
    return want


def _mixed_actions(rng, A, B, t):
    acts = rng.integers(0, A, size=B)
    if t % 3 == 2:  # out-of-range actions on both sides, inside waves that also hold valid ones
        acts[::7] = A + 3
        acts[1::11] = -1
    return acts


# ---- ragged grids against the constant block size ------------------------------------------------------------------------------------
@pytest.mark.parametrize("B", [1, 63, 65, 255, 257, 300])
@pytest.mark.parametrize("kind,n", [("clifford", 16), ("linear_function", 12)])
def test_ragged_grids_and_saturating_depth(kind, n, B):
    gs = line_gateset(kind, n)
    A = len(gs)
    ov, gv = make_pair(kind, n, gs, B, max_depth=16, **PLAIN)
    rng = np.random.default_rng(100 * n + B)
    _scramble(ov, gv, rng, 3 * n, A)
    for t in range(24):  # past max_depth: depth saturates at 0 and stays there
        want = _step_both(ov, gv, _mixed_actions(rng, A, B, t), A, label=f"{kind}{n} B={B} t={t}")
    assert (want[3] == 0).all()
    _same_state(ov, gv, kind, n, f"{kind}{n} B={B}")


# ---- action edge values through the unconditional gate load --------------------------------------------------------------------------
@pytest.mark.parametrize("adt", ["int32", "int64"])
@pytest.mark.parametrize("kind,n", [("clifford", 16), ("linear_function", 12)])
def test_action_edge_values(kind, n, adt):
    gs = line_gateset(kind, n)
    A, B = len(gs), 130
    dtype = getattr(torch, adt)
    ov, gv = make_pair(kind, n, gs, B, max_depth=64, **PLAIN)
    rng = np.random.default_rng(7 + n)
    _scramble(ov, gv, rng, 3 * n, A)
    edges = [-1, A, A + 3, I32_MIN, I32_MAX]
    if adt == "int64":  # the low 32 bits alone are in range, the value is not
        edges += [2**32 + 5, -(2**32) + 5, 2**32, 2**63 - 1, -(2**63), 2**32 + A - 1]
    for t in range(len(edges) + 2):
        acts = rng.integers(0, A, size=B).astype(np.int64)
        bad = np.zeros(B, dtype=bool)
        if t < len(edges):
            bad[t % 5::5] = True  # a fifth of every wave, next to valid actions
            acts[bad] = edges[t]
        else:  # every edge value in one launch
            for k, e in enumerate(edges):
                acts[k::2 * len(edges)] = e
                bad[k::2 * len(edges)] = True
        state0, depth0 = gv.get_state("i64").cpu().numpy(), gv.depth.cpu().numpy().copy()
        want = _step_both(ov, gv, acts, A, dtype, label=f"{kind}{n} {adt} t={t}")
        # out of range: no row changes, no penalty (the reward is 1 or 0 exactly), depth is still used
        state1 = gv.get_state("i64").cpu().numpy()
        np.testing.assert_array_equal(state1[bad], state0[bad])
        assert set(np.unique(want[0][bad])) <= {0.0, 1.0}
        np.testing.assert_array_equal(gv.depth.cpu().numpy()[bad], np.maximum(depth0[bad] - 1, 0))
    _same_state(ov, gv, kind, n, f"{kind}{n} {adt}")


# ---- every instantiation that shares the body ----------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind,n", [("clifford", 3), ("clifford", 5), ("clifford", 8), ("clifford", 16), ("linear_function", 12), ("linear_function", 32)])
def test_sizes(kind, n):
    gs = line_gateset(kind, n)
    A, B = len(gs), 130
    ov, gv = make_pair(kind, n, gs, B, max_depth=10, **PLAIN)
    rng = np.random.default_rng(31 + n)
    _scramble(ov, gv, rng, 2 * n, A)
    for t in range(12):
        _step_both(ov, gv, _mixed_actions(rng, A, B, t), A, label=f"{kind}{n} t={t}")
    _same_state(ov, gv, kind, n, f"{kind}{n}")


WEIGHTS = {"n_cnots": 0.02, "n_layers_cnots": 0.3, "n_layers": 0.07, "n_gates": 0.0005}


@pytest.mark.parametrize("kind,n,cfg,dense", [
    ("clifford", 16, dict(PLAIN), False),                                                      # LIST
    ("linear_function", 12, dict(PLAIN), False),
    ("clifford", 16, dict(PLAIN, track_solution=True, metrics_weights=WEIGHTS), False),        # FEAT + LIST
    ("clifford", 16, dict(PLAIN), True),                                                       # LIST + DENSE
    ("clifford", 8, dict(PLAIN, track_solution=True, metrics_weights=WEIGHTS), True),          # FEAT + LIST + DENSE
])
def test_done_mask_through_a_following_reset_done(kind, n, cfg, dense):
    """A handle that uses reset_done: its steps record the envs that finish (LIST), and the reset that follows re-scrambles exactly those."""
    gs = line_gateset(kind, n)
    A, B, diff = len(gs), 300, 4
    ov, gv = make_pair(kind, n, gs, B, max_depth=3, difficulty=diff, **cfg)
    rng = np.random.default_rng(77 + n)
    _scramble(ov, gv, rng, diff, A)
    tracked = gv.track_dense() if dense else None
    resets = 0
    for t in range(12):
        want = _step_both(ov, gv, _mixed_actions(rng, A, B, t), A, label=f"{kind}{n} t={t}")
        if tracked is not None:
            assert torch.equal(tracked, gv.observe()), t
        done = want[2].astype(bool)
        if done.any():
            gv.reset_done(500 + t)
            ov.reset_seeded(500 + t, mask=done)
            resets += int(done.sum())
            _same_state(ov, gv, kind, n, f"{kind}{n} after reset_done t={t}")
            if tracked is not None:
                assert torch.equal(tracked, gv.observe()), t
    assert resets > B  # every env finished more than once on average: the mask was in use throughout
    if cfg.get("track_solution"):
        for e in (0, 63, 64, B - 1):
            assert gv.solution(e) == ov.env(e).solution(), e


@pytest.mark.parametrize("kind,n", [("clifford", 16), ("linear_function", 12)])
def test_solution_log_and_layer_weights(kind, n):
    gs = line_gateset(kind, n)
    A, B = len(gs), 130
    ov, gv = make_pair(kind, n, gs, B, max_depth=40, **dict(PLAIN, track_solution=True, metrics_weights=WEIGHTS))
    rng = np.random.default_rng(5 + n)
    _scramble(ov, gv, rng, 10, A)
    for t in range(16):
        acts = rng.integers(0, A, size=B)
        if t == 7:
            acts[::5] = A  # out of range: still logged (clifford.rs:334-340)
        _step_both(ov, gv, acts, A, label=f"{kind}{n} t={t}")
    _same_state(ov, gv, kind, n, f"{kind}{n}")
    for e in (0, 1, 64, B - 1):
        assert gv.solution(e) == ov.env(e).solution(), e


@pytest.mark.parametrize("n,B", [(8, 131), (16, 131), (16, 64)])
def test_tracked_dense_follows_every_step(n, B):
    gs = line_gateset("clifford", n)
    A = len(gs)
    ov, gv = make_pair("clifford", n, gs, B, max_depth=10, **PLAIN)
    rng = np.random.default_rng(900 + n + B)
    _scramble(ov, gv, rng, 2 * n, A)
    tracked = gv.track_dense()
    for t in range(12):
        _step_both(ov, gv, _mixed_actions(rng, A, B, t), A, label=f"dense {n}q t={t}")
        assert torch.equal(tracked, gv.observe()), t
        np.testing.assert_array_equal(tracked.cpu().numpy().reshape(B, -1), ov.observe_dense(), err_msg=f"tracked dense t={t}")


# ---- launch forms --------------------------------------------------------------------------------------------------------------------
def test_eager_ring_and_captured_graph_agree():
    kind, n, B, T, period, replays = "clifford", 16, 300, 5, 3, 3
    gs = line_gateset(kind, n)
    A = len(gs)
    rng = np.random.default_rng(2024)
    ov, eager = make_pair(kind, n, gs, B, max_depth=64, **PLAIN)
    from qiskit_gym_amd.vec import VecEnv

    ring, captured = (VecEnv(kind, n, gs, B, max_depth=64, **PLAIN) for _ in range(2))
    draws = _scramble(ov, eager, rng, 24, A)
    for e in (ring, captured):
        e.difficulty = 24
        e.reset_with(_dev(draws, torch.int32))
    host = rng.integers(0, A, size=(period, B))
    host[1, ::9] = A + 1
    acts = _dev(host, torch.int32)
    stream = torch.cuda.Stream()
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph, stream=stream):  # captured, not run
        for t in range(T):
            captured.step(acts[t % period])
    for rep in range(replays):
        for t in range(T):
            want = ov.step(_for_oracle(host[t % period]))
            eager.step(acts[t % period])
        ring.rollout_ring(acts, T)
        graph.replay()
        torch.cuda.synchronize()
        for name, e in (("eager", eager), ("ring", ring), ("captured", captured)):
            _same_outputs(e, want, f"{name} replay {rep}")
            _same_state(ov, e, kind, n, f"{name} replay {rep}")
        assert torch.equal(eager.get_state("packed"), ring.get_state("packed")) and torch.equal(eager.get_state("packed"), captured.get_state("packed"))


# ---- kernel clock attached -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("B", [300, 64])
def test_kernel_clock_attached(B):
    kind, n, T = "clifford", 16, 6
    gs = line_gateset(kind, n)
    A = len(gs)
    ov, gv = make_pair(kind, n, gs, B, max_depth=64, **PLAIN)
    rng = np.random.default_rng(11 + B)
    _scramble(ov, gv, rng, 24, A)
    host = rng.integers(0, A, size=(T, B))
    slots = gv.kernel_clock(T)
    gv.rollout(_dev(host, torch.int32), fused=False)
    for t in range(T):
        want = ov.step(host[t])
    _same_outputs(gv, want, "clocked")
    d = gv.kernel_durations_us(slots)
    assert len(d) == T and (d > 0).all(), d
    live = slots[:T, :, 1] != 0
    assert bool((live.sum(dim=1) >= (B + 63) // 64).all()), "every wave of every launch writes its record"
    assert bool((slots[:T, :, 1][live] >= slots[:T, :, 0][live]).all())
    gv.kernel_clock(0)
    _same_state(ov, gv, kind, n, "clocked")
