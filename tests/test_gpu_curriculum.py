"""A curriculum on a live handle: `env.difficulty = d` between resets, many times over, on ONE handle (the reference trainer raises
`env.difficulty` whenever the success rate crosses its threshold, rl/synthesis.py:128-133; set_difficulty only stores the number and
the next reset() reads it for the scramble length and the start depth, clifford.rs:296,311,317).

Difficulty picks the reset path at launch time -- trees from 64 draws, 16 lanes per env for short lists, one lane per env otherwise,
a thread per env for the first difficulties, one launch or two for reset_done_step, PauliEnv's tree -- and the done-list session, the
mask / list rotation and the tree grid's sizing carry over from one reset to the next.  Every test here walks one handle along a ladder
of difficulties that crosses those thresholds in both directions (and visits 0: no gate, depth 0, final at once) and compares EVERY
env, bit for bit, with the CPU oracle after every call; two families also with tests/envmodel.py.  `plan()` says which paths the
ladder visits before the walk starts."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")

from envmodel import Model  # noqa: E402
from oracle import OracleEnv, OracleVec  # noqa: E402
from test_dispatch import DEFAULT, PLAIN, RESET_DONE, RESET_DONE_STEP, plan  # noqa: E402
from test_gpu_envmodel import RDS_CASES, _draws  # noqa: E402
from util import f32_bits, grid_gateset, line_gateset, make_pair, oracle_cfg, oracle_envs, rng_actions, rng_draw, set_difficulty  # noqa: E402

# crosses 8 / 9 (the thread-per-env reset), 16 / 17 (the word layouts' draws per lane) and 63 / 64 (the trees) upwards and downwards;
# 256 is capped by max_depth = 128
LADDER = [1, 2, 8, 9, 16, 17, 63, 64, 65, 256, 70, 9, 8, 1]
# difficulty 0 (the reference accepts it: no gate, depth 0, final at once), on the short and then on the long list, and back up.  (The 5 first:
# the envs of the 1 before it have all finished -- episodes of two steps -- and would make the 0's short list a long one.)
LADDER_0 = LADDER + [5, 0, 0, 3]
PAULI_LADDER = [1, 2, 7, 8, 9, 15, 16, 17, 63, 64, 65, 256, 70, 9, 8, 1, 5, 0, 0, 3]  # pauli_diff_scale = 8: 7 / 8 and 15 / 16 change the target's size
POLICY_LADDER = [1, 3, 9, 64, 2]
PAULI = dict(max_rotations=5, pauli_diff_scale=8, add_perms=False, track_solution=False)
START = 40  # the difficulty the handles are built and first reset at: episodes of 80 steps, longer than any walk
PHI = 0x9E3779B9
M64 = 2**64 - 1


def _gateset(kind, n):
    if kind == "permutation":
        return grid_gateset("permutation", 3, n // 3)
    return line_gateset(kind, n)


def _per_env(kind, n):
    return {"clifford": 4 * n * n, "linear_function": n * n, "permutation": n}[kind]


def _dev(a, dtype):
    return torch.as_tensor(np.ascontiguousarray(a), device="cuda").to(dtype)


def _long_rungs(ladder):
    """Which rungs end the long list's episodes: every other one, the other way round after the ladder's top, so that the way down
    meets each threshold with the list the way up did not."""
    top = int(np.argmax(ladder))
    return [(i + (i > top)) % 2 == 1 for i in range(len(ladder))]


def _flags_of(envs, ids, flags=None):
    """reward bits, is_final, success and depth of the oracle envs `ids` (the others carried over from `flags`)."""
    if flags is None:
        flags = dict(reward=np.zeros(len(envs), np.uint32), done=np.zeros(len(envs), np.uint8), success=np.zeros(len(envs), np.uint8),
                     depth=np.zeros(len(envs), np.int64))
    else:
        flags = {k: v.copy() for k, v in flags.items()}
    for e in ids:
        o = envs[e]
        flags["reward"][e], flags["done"][e], flags["success"][e], flags["depth"][e] = o.reward_bits(), o.is_final(), o.success(), o.depth()
    return flags


def _step_flags(r, s, f, d):
    return dict(reward=f32_bits(r), done=np.asarray(f, np.uint8), success=np.asarray(s, np.uint8), depth=np.asarray(d, np.int64))


def _expect(gv, ov, flags, label, full=True, m=None):
    """The whole batch against the oracle (and the model): state, observation, reward bits, is_final, success, depth."""
    gv.sync()
    np.testing.assert_array_equal(f32_bits(gv.reward.cpu().numpy()), flags["reward"], err_msg=f"reward {label}")
    np.testing.assert_array_equal(gv.done.cpu().numpy(), flags["done"], err_msg=f"is_final {label}")
    np.testing.assert_array_equal(gv.success.cpu().numpy(), flags["success"], err_msg=f"success {label}")
    np.testing.assert_array_equal(gv.depth.cpu().numpy(), flags["depth"], err_msg=f"depth {label}")
    np.testing.assert_array_equal(gv.observe().cpu().numpy().reshape(gv.batch, -1), ov.observe_dense(), err_msg=f"observation {label}")
    state = None
    if full and gv.env_kind != "pauli":
        state = gv.get_state("i64").cpu().numpy()
        np.testing.assert_array_equal(state, ov.get_state(_per_env(gv.env_kind, gv.num_qubits)), err_msg=f"state {label}")
    if m is not None:
        np.testing.assert_array_equal(state, m.wire(), err_msg=f"model state {label}")
        np.testing.assert_array_equal(flags["reward"], f32_bits(m.reward), err_msg=f"model reward {label}")
        np.testing.assert_array_equal(flags["done"], m.is_final(), err_msg=f"model is_final {label}")
        np.testing.assert_array_equal(flags["success"], m.success, err_msg=f"model success {label}")
        np.testing.assert_array_equal(flags["depth"], m.depth, err_msg=f"model depth {label}")


def _actions(rng, B, A, t):
    """Random actions, some of them out of range (one past the end, further, negative: no-ops for the state that still use depth)."""
    acts = rng.integers(0, A, size=B)
    acts[1 + t::14] = A
    acts[3 + t::22] = A + 3
    acts[5 + t::26] = -1
    return acts


def _step(gv, ov, m, rng, A, t, coins_on):
    acts = _actions(rng, gv.batch, A, t)
    coins = rng.integers(0, 2, size=gv.batch) if coins_on else None
    flags = _step_flags(*ov.step(acts, coins))
    if m is not None:
        m.step(acts)
    return acts, coins, flags


def _expect_logs(gv, ov, cap):
    g_sol, g_len = gv.solutions(cap)
    o_sol, o_len = ov.solutions(cap)
    np.testing.assert_array_equal(g_len, o_len, err_msg="solution log lengths")
    np.testing.assert_array_equal(g_sol, o_sol, err_msg="solution logs")


TILE_PATHS = {"scramble_tree", "scramble_coop", "scramble_flat"}
PAULI_PATHS = {"compact_done + ptile_reset_tree_kernel", "compact_done + ptile_generate_kernel"}
A_CASES = [
    # kind, qubits, options, batch, (short list, long list), the reset paths the ladder must name, also against the model
    ("clifford", 16, PLAIN, 2048, (32, 1024), TILE_PATHS, True),      # TILE: coop below 64 draws and trees from 64 (short); thread per env up to 8
    ("clifford", 16, PLAIN, 8192, (32, 4097), TILE_PATHS, False),     #   draws, flat above, trees from 64 (long); 4 097: flat also from 64 draws
    ("clifford", 16, DEFAULT, 2048, (32, 1024), TILE_PATHS, False),   # add_inverts + solution log
    ("clifford", 24, PLAIN, 2048, (32, 1024), {"scramble_tree64", "scramble_coop", "scramble_flat"}, False),  # TILE64
    ("linear_function", 8, PLAIN, 2048, (32, 1024), {"word_init_kernel"}, True),    # one word per env: ceil(difficulty / 16) draws per lane
    ("linear_function", 24, DEFAULT, 2048, (32, 1024), {"init_kernel"}, False),     # LFD
    ("permutation", 9, PLAIN, 2048, (32, 1024), {"word_init_kernel"}, False),
    ("permutation", 27, PLAIN, 2048, (32, 1024), {"init_kernel"}, False),           # a byte per entry
    ("pauli", 20, PAULI, 4100, (32, 1024), PAULI_PATHS, False),                     # (lists are compacted, and short ones are trees, above 4 096 envs)
]


@pytest.mark.parametrize("kind,n,opts,B,counts,want,model", A_CASES, ids=[f"{c[0]}{c[1]}-{'default' if c[2] is DEFAULT else 'plain'}-B{c[3]}" for c in A_CASES])
def test_reset_done_along_the_ladder(kind, n, opts, B, counts, want, model):
    """set difficulty -> end some episodes (a short and a long list in turn) -> reset_done -> two steps, rung after rung on one handle."""
    gs = _gateset(kind, n)
    A = len(gs)
    ladder = PAULI_LADDER if kind == "pauli" else LADDER_0
    longs = _long_rungs(ladder)
    names = [plan(kind, n, RESET_DONE, batch=B, arg=counts[lg], num_actions=A, difficulty=d, **opts) for d, lg in zip(ladder, longs)]
    assert set(names) == want, list(zip(ladder, names))
    if B == 8192:  # the list longer than the trees take: one lane per env at 64 draws and more
        assert {nm for nm, d, lg in zip(names, ladder, longs) if lg and d >= 64} == {"scramble_flat"}
    cfg = dict(opts, difficulty=START, depth_slope=2, max_depth=128)
    ov, gv = make_pair(kind, n, gs, B, **cfg)
    envs = oracle_envs(ov)
    m = Model(kind, n, gs, B, add_inverts=False, track_solution=False, max_depth=128, depth_slope=2) if model else None
    gv.reset(3)
    ov.reset_seeded(3)
    if m is not None:
        m.reset_with(rng_actions(3, B, START, A))
    full = B <= 4100  # (the observation is the whole state of these kinds: the i64 export of 8 192 Clifford envs is 67 MB a time)
    flags = _flags_of(envs, range(B))
    _expect(gv, ov, flags, "reset(3)", full, m)
    rng = np.random.default_rng(n * 100 + B)
    coins_on = bool(opts.get("add_inverts", False))
    for i, (d, lg) in enumerate(zip(ladder, longs)):
        label = f"rung {i} (difficulty {d}, {'long' if lg else 'short'} list)"
        set_difficulty(ov, gv, d)
        done = flags["done"].astype(bool)  # the episodes that ended by themselves, and the caller ends these:
        done[rng.choice(B, size=counts[lg], replace=False)] = True
        ids = np.flatnonzero(done)
        before = gv.observe_packed().clone()
        gv.done.copy_(_dev(done, torch.uint8))
        seed = 500 + i
        gv.reset_done(seed)
        ov.reset_seeded(seed, mask=done)
        if kind != "pauli":  # the draws made in numpy, on fresh oracle envs built at this difficulty: the reset envs' states
            fresh = OracleVec(ov.proto, ids.size)
            fresh.reset_with(rng_actions(seed, ids, d, A))
            np.testing.assert_array_equal(ov.observe_dense()[ids], fresh.observe_dense(), err_msg=f"oracle {label}")
        if m is not None:
            m.reset_with(_draws(seed, ids, B, d, A), mask=done)
        flags = _flags_of(envs, ids, flags)
        np.testing.assert_array_equal(flags["depth"][ids], min(2 * d, 128), err_msg=f"start depth {label}")  # clifford.rs:317
        _expect(gv, ov, flags, f"after reset_done, {label}", full, m)
        live = _dev(~done, torch.bool)
        assert torch.equal(gv.observe_packed()[live], before[live]), f"a live env was touched, {label}"
        for t in range(2):
            acts, coins, flags = _step(gv, ov, m, rng, A, t, coins_on)
            gv.step(_dev(acts, torch.int32), _dev(coins, torch.uint8) if coins_on else None)
            _expect(gv, ov, flags, f"step {t}, {label}", full, m)
    if opts.get("track_solution"):
        _expect_logs(gv, ov, 128)


@pytest.mark.parametrize("kind,n,opts,_diff,want", RDS_CASES, ids=[f"{c[0]}{c[1]}-{'default' if c[2] is DEFAULT else 'plain'}" for c in RDS_CASES])
def test_reset_done_step_along_the_ladder(kind, n, opts, _diff, want):
    """reset_done_step, three per rung, with episodes of at most 6 steps: one launch or two is decided from the difficulty at every call
    (qgym_plan.hpp reset_step_pays), on a handle whose list and masks were left by the calls of the rung before."""
    B = 1000
    gs = _gateset(kind, n)
    A = len(gs)
    cfg = dict(opts, depth_slope=1, max_depth=6)
    names = [str(plan(kind, n, RESET_DONE_STEP, batch=B, num_actions=A, difficulty=d, **cfg)) for d in LADDER]
    if want == "word_reset_step_kernel":  # no list: one launch at every difficulty
        assert set(names) == {want}
    else:
        assert "two launches" in names and any(nm.startswith(want) for nm in names), names
        assert all(nm == "two launches" or nm.startswith(want) for nm in names), names
    ov, gv = make_pair(kind, n, gs, B, difficulty=5, **cfg)
    envs = oracle_envs(ov)
    gv.reset(3)
    ov.reset_seeded(3)
    flags = _flags_of(envs, range(B))
    _expect(gv, ov, flags, "reset(3)")
    rng = np.random.default_rng(n + 7)
    coins_on = bool(opts["add_inverts"])
    resets = 0
    for i, d in enumerate(LADDER):
        set_difficulty(ov, gv, d)
        for t in range(3):
            seed = 700 + 3 * i + t
            fin = flags["done"].astype(bool)
            resets += int(fin.sum())
            ov.reset_seeded(seed, mask=fin)
            acts, coins, flags = _step(gv, ov, None, rng, A, t, coins_on)
            gv.reset_done_step(seed, _dev(acts, torch.int32), _dev(coins, torch.uint8) if coins_on else None)
            _expect(gv, ov, flags, f"rung {i} (difficulty {d}), step {t}")
            # an env reset in this call starts at min(depth_slope * d, max_depth) and has taken one step
            np.testing.assert_array_equal(flags["depth"][fin], min(d, 6) - 1)
    assert resets > 3 * B
    if opts["track_solution"]:
        _expect_logs(gv, ov, 8)


@pytest.mark.parametrize("kind,n,opts", [("clifford", 16, DEFAULT), ("permutation", 27, PLAIN)])
def test_reset_and_reset_with_after_a_change(kind, n, opts):
    """reset(seed) draws the new number of gates; reset_with is refused with the old number of draws and accepted with the new one."""
    from qiskit_gym_amd import _lib

    B = 333
    gs = _gateset(kind, n)
    A = len(gs)
    ov, gv = make_pair(kind, n, gs, B, difficulty=5, depth_slope=2, max_depth=128, **opts)
    envs = oracle_envs(ov)
    rng = np.random.default_rng(n)
    coins_on = bool(opts["add_inverts"])
    for i, d in enumerate(LADDER_0):
        old = gv.difficulty
        set_difficulty(ov, gv, d)
        seed = 40 + i
        gv.reset(seed)
        ov.reset_with(rng_actions(seed, B, d, A))
        flags = _flags_of(envs, range(B))
        np.testing.assert_array_equal(flags["depth"], min(2 * d, 128))
        _expect(gv, ov, flags, f"reset(seed) at difficulty {d}")
        if old != d:
            with pytest.raises(_lib.QGymError, match=rf"exactly `difficulty` \({d}\) draws per env, got {old}"):
                gv.reset_with(_dev(rng.integers(0, A, size=(old, B)), torch.int32))
            _expect(gv, ov, flags, f"after the refused reset_with at difficulty {d}")  # nothing happened
        draws = rng.integers(0, A, size=(d, B))
        gv.reset_with(_dev(draws, torch.int32))
        ov.reset_with(draws)
        flags = _flags_of(envs, range(B))
        np.testing.assert_array_equal(flags["depth"], min(2 * d, 128))
        _expect(gv, ov, flags, f"reset_with at difficulty {d}")
        acts, coins, flags = _step(gv, ov, None, rng, A, 0, coins_on)
        gv.step(_dev(acts, torch.int32), _dev(coins, torch.uint8) if coins_on else None)
        _expect(gv, ov, flags, f"step at difficulty {d}")


# ---- the collector: the sampling kernel that steps and resets, and collections replayed from a graph ------------------------------------
KEYS = ("obs", "actions", "logp", "values", "rewards", "dones", "advantages")


def _collect(col, env, T, difficulty, depth_of, fused):
    """env.difficulty = d (where it differs), one collection, its outputs cloned; and, directly: every env reset in this collection
    started at this difficulty's depth -- after its last finished episode it was reset and has stepped to the collection's end."""
    if env.difficulty != difficulty:
        env.difficulty = difficulty
    assert env.difficulty == difficulty
    ro = col.collect(T)
    torch.cuda.synchronize()
    got = {k: getattr(ro, k).clone() for k in KEYS}
    dones = got["dones"].cpu().numpy() > 0
    depth = env.depth.cpu().numpy()
    last = T - 1 - np.argmax(dones[::-1], axis=0)  # the last step that ended an episode of the env (where any did)
    mid = dones.any(axis=0) & (last < T - 1)
    np.testing.assert_array_equal(depth[mid], depth_of(difficulty) - (T - 1 - last[mid]), err_msg=f"depth after a reset at difficulty {difficulty}")
    if fused:  # ... and the envs the last step finished have been reset by its own call
        np.testing.assert_array_equal(depth[dones[T - 1]], depth_of(difficulty))
    return got, int(mid.sum())


def _replay_on_the_oracle(kind, n, gs, cfg, B, seed, runs, depth_of):
    """The collector's trajectories on B oracle envs: `runs` = [(difficulty, outputs)], the collections in order.  Collector step number s
    resets the final envs with seed + PHI * (s + 1), `difficulty` draws (util.rng_actions), and throws the add_inverts coin with counter s."""
    A = len(gs)
    envs = [OracleEnv(kind, n, gs, **oracle_cfg(cfg)) for _ in range(B)]
    ids = np.arange(B, dtype=np.uint64)
    inverts = bool(cfg.get("add_inverts", False))
    s = 0
    for d, got in runs:
        acts, rew, done = got["actions"].cpu().numpy(), f32_bits(got["rewards"].cpu().numpy()), got["dones"].cpu().numpy()
        for o in envs:
            o.difficulty = d
        resets = 0
        for t in range(acts.shape[0]):
            draws = rng_actions((seed + PHI * (s + 1)) & M64, B, d, A)
            coins = (rng_draw(0x5EED0000C01F ^ 0x636F696E, ids, s) >> np.uint64(63)).astype(np.int64) if inverts else np.zeros(B, np.int64)
            for e, o in enumerate(envs):
                if o.is_final():  # (a fresh env is final: depth 1, solved)
                    o.reset_with(draws[:, e])
                    assert o.depth() == depth_of(d)
                    resets += 1
                o.step(int(acts[t, e]), int(coins[e]))
                assert o.reward_bits() == int(rew[t, e]) and int(o.is_final()) == int(done[t, e]), (d, t, e)
            s += 1
        assert resets > 0, f"no episode started at difficulty {d}"


@pytest.mark.parametrize("kind,n,inverts", [("clifford", 16, False), ("clifford", 16, True), ("linear_function", 12, False)])
def test_sampling_kernel_that_steps_and_resets_along_the_ladder(kind, n, inverts):
    """qg_vec_mid_head_sample_step_reset resets the envs it finishes itself, with the handle's difficulty at the call.  With the difficulty
    set before every collection the fused collector equals the separate launches bit for bit -- also for the envs whose episode ended in a
    collection's last step, which the fused call has restarted before the change -- and replays on the oracle."""
    from qiskit_gym_amd.collector import BasicPolicy, RolloutCollector
    from qiskit_gym_amd.vec import VecEnv

    B, T = 1000, 6
    gs = line_gateset(kind, n)
    A = len(gs)
    cfg = dict(add_inverts=inverts, add_perms=False, track_solution=inverts, depth_slope=1, max_depth=4)  # episodes of 1 .. 4 steps: resets at every rung
    depth_of = lambda d: min(d, 4)  # noqa: E731
    obs_size = 4 * n * n if kind == "clifford" else n * n
    runs = {}
    for fused in (True, False):
        env = VecEnv(kind, n, gs, B, **cfg)
        torch.manual_seed(3)
        pol = BasicPolicy(obs_size, A, embedding_size=128, common=256)
        col = RolloutCollector(env, pol, dtype=torch.bfloat16, seed=5, store_obs="packed", use_graph=False, use_bit_embedding=True,
                               use_fused_head=True, use_fused_step=fused)
        assert col.route.tail == "mid_head" and col.route.fused_step == fused
        runs[fused] = [_collect(col, env, T, d, depth_of, fused)[0] for d in POLICY_LADDER]
        env.sync()
    for k, d in enumerate(POLICY_LADDER):
        for name in KEYS:
            assert torch.equal(runs[True][k][name], runs[False][k][name]), (d, name)
    _replay_on_the_oracle(kind, n, gs, cfg, B, 5, list(zip(POLICY_LADDER, runs[True])), depth_of)


E_ROUTES = [
    # env kind, qubits, batch, policy dtype, options, (embedding, middle) features, observation store -> route tail, fused step
    ("clifford", 4, 160, "float32", dict(add_inverts=False, add_perms=False, track_solution=False), (64, 32), "dense", "heads_gemm", False),
    ("clifford", 16, 1000, "bfloat16", dict(add_inverts=False, add_perms=False, track_solution=False), (128, 256), "packed", "mid_head", True),
    ("pauli", 5, 160, "float32", dict(add_perms=False, track_solution=False, max_rotations=3, pauli_diff_scale=1), (64, 32), "dense", "heads_gemm", False),
]


@pytest.mark.parametrize("kind,n,B,dtype_name,opts,sizes,store,tail,fused", E_ROUTES, ids=[f"{c[0]}{c[1]}-{c[3]}-{c[7]}" for c in E_ROUTES])
def test_graph_collector_follows_the_difficulty(kind, n, B, dtype_name, opts, sizes, store, tail, fused):
    """use_graph=True captures reset_done and the sampling + step + reset call with the difficulty's scramble length, start depth and kernel
    choice as arguments: `env.difficulty = d` between collections must take effect in the next one, as it does eagerly."""
    from qiskit_gym_amd.collector import BasicPolicy, RolloutCollector
    from qiskit_gym_amd.vec import VecEnv

    T = 6
    # episodes of 6, 4 and 5 steps (unless solved): both changes find the envs finished in the collection's last step, and the collection after a
    # change resets them at its start and again in its middle
    d1, d2, d3 = 6, 4, 5
    plan_ = [d1, d2, d2, d3]
    gs = line_gateset(kind, n)
    cfg = dict(opts, depth_slope=1, max_depth=128, difficulty=d1)
    depth_of = lambda d: min(d, 128)  # noqa: E731
    rollouts = {}
    for mode in (False, True):
        env = VecEnv(kind, n, gs, B, **cfg)
        torch.manual_seed(3)
        pol = BasicPolicy(env.obs_shape_[0] * env.obs_shape_[1], len(gs), embedding_size=sizes[0], common=sizes[1])
        col = RolloutCollector(env, pol, dtype=getattr(torch, dtype_name), seed=21, store_obs=store, use_graph=mode)
        assert col.route.tail == tail and col.route.fused_step == fused
        got = [_collect(col, env, T, d, depth_of, fused) for d in plan_]
        env.sync()
        assert col.steps_done == len(plan_) * T
        assert got[1][1] > 0 and got[3][1] > 0, "no env was reset mid-collection after a change"
        rollouts[mode] = [g for g, _ in got]
    for k, d in enumerate(plan_):
        for name, eager in rollouts[False][k].items():
            if eager.dtype.is_floating_point:  # the GEMMs may pick different kernels under capture
                torch.testing.assert_close(rollouts[True][k][name], eager, atol=1e-4, rtol=1e-4, msg=lambda msg: f"call {k} (difficulty {d}) {name}: {msg}")
            else:
                assert torch.equal(rollouts[True][k][name], eager), (k, d, name)
    if kind != "pauli":
        _replay_on_the_oracle(kind, n, gs, cfg, B, 21, list(zip(plan_, rollouts[False])), depth_of)


# ---- the scalar surface: qg_env_set_difficulty / qg_env_get_difficulty, clones and the clone pool -----------------------------------------
def _episode(env, ora, rng, A, steps):
    """Random actions until is_final, on the scalar env and the oracle: the same observations, rewards and flags, `steps` steps unless solved."""
    assert env.observe() == ora.observe() and env.is_final() == ora.is_final() and env.success() == ora.success()
    taken = 0
    while not ora.is_final():
        a = int(rng.integers(0, A))
        env.step(a)
        ora.step(a)
        taken += 1
        assert env.observe() == ora.observe(), taken
        assert np.float32(env.reward()).view(np.uint32) == ora.reward_bits(), taken
        assert env.is_final() == ora.is_final() and env.success() == ora.success(), taken
    assert env.is_final() and (taken == steps or (ora.success() and taken < steps))


@pytest.mark.parametrize("kind,n", [("clifford", 5), ("permutation", 9)])
def test_scalar_env_difficulty_clone_and_pool(kind, n):
    from qiskit_gym_amd.envs.raw import RawEnv

    gs = _gateset(kind, n)
    A = len(gs)
    kw = dict(add_inverts=False, add_perms=False)
    okw = oracle_cfg(kw)
    rng = np.random.default_rng(n)

    def oracle_at(d, seed):  # a fresh oracle env built at `d`, reset with the draws of `seed` for env 0
        o = OracleEnv(kind, n, gs, difficulty=d, **okw)
        o.reset_with(rng_actions(seed, 1, d, A)[:, 0])
        return o

    env = RawEnv(kind, n, gs, seed=1, **kw)
    assert env.difficulty == 1
    for d, seed in ((4, 11), (9, 12), (0, 13), (2, 14)):  # up, down to no gate at all (final at once), up again: one env
        env.difficulty = d
        assert env.difficulty == d
        env.reset(seed)
        _episode(env, oracle_at(d, seed), rng, A, 2 * d)
    # clone() after a change carries the new difficulty
    env.difficulty = 6
    twin = env.clone(seed=2)
    assert twin.difficulty == 6
    twin.reset(15)
    _episode(twin, oracle_at(6, 15), rng, A, 12)
    # a handle from the clone pool has its previous owner's difficulty: the clone takes its source's
    stale = RawEnv(kind, n, gs, seed=3, **kw)
    stale.difficulty = 7
    del stale  # (into the pool: qg_env_destroy)
    proto = RawEnv(kind, n, gs, seed=4, **kw)
    proto.difficulty = 2
    pooled = proto.clone(seed=5)
    assert pooled.difficulty == 2 and proto.difficulty == 2
    pooled.reset(16)
    _episode(pooled, oracle_at(2, 16), rng, A, 4)
