"""The solution log at its capacity, and action values far outside the gateset, on every step kernel the dispatcher picks: against
tests/envmodel.py / tests/paulimodel.py for what a step computes and tests/logcap_model.py for what the log must hold.

With `track_solution` the log holds `max_depth` pushes per env (PauliEnv: plus one per rotation).  A push beyond that is dropped and
sets status bit 8 (QG_FAULT_SOLUTION_OVERFLOW) in the env's word; everything else a step computes goes on as in the reference.  The
cases run an episode of exactly `max_depth` logged steps (the last slot must be written), then step the finished envs once more (the
first push that must not be), in waves that hold overflowing envs beside clean ones.  Every comparison is exact.  Each case first
asserts through `qg_plan_query` that its configuration runs the kernel it names."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

from logcap_model import OVERFLOW_BIT, PushRecorder, reported  # noqa: E402
from paulimodel import PauliModel  # noqa: E402
from test_dispatch import DEFAULT, FUSED, LAYOUT, PLAIN, RESET_DONE_STEP, STEP, plan  # noqa: E402
from test_gpu_envmodel import _dev, _draws, _expect_state, _gateset, _make, _targets  # noqa: E402
from test_gpu_paulimodel import W_COUNTS, replay_target  # noqa: E402
from util import f32_bits, line_gateset  # noqa: E402

TRACK = dict(PLAIN, track_solution=True)
B = 130  # two full waves and a ragged third
CAP = 5  # max_depth of the capacity cases: the boundary is a handful of steps away

ROWS = [
    # kind, qubits, options, odd envs non-symplectic -> env.step() kernel, fused rollout kernel
    ("clifford", 16, TRACK, 0, "qm_step1_kernel", "qm_step_kernel"),
    ("clifford", 16, DEFAULT, 0, "qm_inv2_kernel", "qm_step_kernel<inv>"),
    ("clifford", 16, DEFAULT, 1, "qm_step_kernel<gauss-jordan>", "qm_step_kernel<gauss-jordan>"),
    ("clifford", 24, TRACK, 0, "q64_step1_kernel", "q64_step_kernel"),
    ("clifford", 24, DEFAULT, 0, "q64_inv2_kernel", "q64_step_kernel<inv>"),
    ("clifford", 17, DEFAULT, 1, "q64_step_kernel<gauss-jordan>", "q64_step_kernel<gauss-jordan>"),
    ("linear_function", 8, TRACK, 0, "word_step_kernel", "word_step_kernel"),
    ("linear_function", 8, DEFAULT, 0, "word_step_kernel", "word_step_kernel"),
    ("linear_function", 24, TRACK, 0, "qm_step1_kernel", "qm_step_kernel"),
    ("linear_function", 48, TRACK, 0, "q64_step1_kernel", "q64_step_kernel"),
    ("linear_function", 24, DEFAULT, 0, "lfd_step_kernel", "lfd_step_kernel"),
    ("linear_function", 48, DEFAULT, 0, "lfd_step_kernel", "lfd_step_kernel"),
    ("permutation", 9, TRACK, 0, "word_step_kernel", "word_step_kernel"),
    ("permutation", 9, DEFAULT, 0, "word_step_kernel", "word_step_kernel"),
    ("permutation", 27, TRACK, 0, "permb_step1_kernel", "permb_step_kernel"),
    ("permutation", 27, DEFAULT, 0, "permb_step_kernel", "permb_step_kernel"),
]
PAULI_ROWS = [
    # max_rotations -> layout, env.step() kernel, fused rollout kernel   (6 qubits; rmax = max_rotations + 2)
    (4, "PTILE-compact", "ptile_step1c_kernel", "ptile_step_kernel"),
    (10, "PTILE", "ptile_step1_kernel", "ptile_step_kernel"),
]


def _row_id(r):
    return f"{r[0]}{r[1]}-{'default' if r[2]['add_inverts'] else 'track'}-ns{r[3]}"


ROW_IDS = [_row_id(r) for r in ROWS]


def _expect(gv, m, label):
    """test_gpu_envmodel._expect without its sync(): after an overflow sync() raises, and everything else must still be the model's."""
    np.testing.assert_array_equal(f32_bits(gv.reward.cpu().numpy()), f32_bits(m.reward), err_msg=f"reward {label}")
    np.testing.assert_array_equal(gv.done.cpu().numpy(), m.is_final(), err_msg=f"done {label}")
    np.testing.assert_array_equal(gv.success.cpu().numpy(), m.success, err_msg=f"success {label}")
    np.testing.assert_array_equal(gv.depth.cpu().numpy(), m.depth, err_msg=f"depth {label}")
    _expect_state(gv, m, label)
    np.testing.assert_array_equal(gv.masks().cpu().numpy(), m.masks(), err_msg=f"masks {label}")


def _expect_log(gv, rec, cap, label):
    """Lengths and entries of every env's log against the recorder's first `cap` pushes; returns the lengths."""
    sol, lens = gv.solutions(cap=cap + 2)
    np.testing.assert_array_equal(lens, np.minimum(rec.counts(), cap), err_msg=f"log lengths {label}")
    want = rec.expected_log(cap)
    for b in range(rec.B):
        assert sol[b, : lens[b]].tolist() == want[b], (label, b)
    return lens


def _expect_overflow(gv, rec, cap, label):
    from qiskit_gym_amd._lib import QGymError

    np.testing.assert_array_equal(gv.faults(), rec.expected_faults(cap), err_msg=f"faults {label}")
    if rec.overflowed(cap).any():
        with pytest.raises(QGymError, match="solution log overflow"):
            gv.sync()
    else:
        gv.sync()


def _schedule(m, rng, circs, n_steps, coins_on, misses):
    """Actions and coins [n_steps, B], drawn before anything runs.  Even envs replay their target with zero coins, then act at random
    in range.  Odd envs act at random, with coins where add_inverts is on; the odd envs b = 1 (mod 6) are fed `misses` out-of-range
    actions each (-1, A, A + 3 in turn) at steps that differ from env to env, the last step among them."""
    A = m.A
    acts = rng.integers(0, A, size=(n_steps, B))
    T0 = circs.shape[1]
    acts[:T0, ::2] = circs[::2, :T0].T
    fed = np.zeros(B, bool)
    for b in range(1, B, 6):
        fed[b] = True
        for k in range(misses):
            acts[(b // 6 + 2 * k) % n_steps, b] = (-1, A, A + 3)[(b // 6 + k) % 3]
    coins = rng.integers(0, 2, size=(n_steps, B)) if coins_on else np.zeros((n_steps, B), np.int64)
    coins[:, ::2] = 0
    return acts, coins, fed


def _dry_counts(kind, A, acts):
    dry = PushRecorder(kind, B, A)
    for a in acts:
        dry.note(a)
    return dry.counts()


def _assert_waves_hold_both(kind, over, fed, label):
    """About the inputs, before any launch: every full wave holds at least 8 envs whose log overflows and, on PermutationEnv, at least 8
    that were fed an out-of-range action and must stay clean beside them."""
    for w in range(B // 64):
        wave = slice(64 * w, 64 * w + 64)
        assert over[wave].sum() >= 8, (label, w)
        if kind == "permutation":
            assert (fed & ~over)[wave].sum() >= 8, (label, w)


# ---- (a) exactly full, then one more ----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("path", ["step", "graph", "fused"])
@pytest.mark.parametrize("kind,n,opts,nonsymp,step_k,fused_k", ROWS, ids=ROW_IDS)
def test_exactly_full_then_one_more(kind, n, opts, nonsymp, step_k, fused_k, path):
    cap = CAP
    cfg = dict(opts, max_depth=cap)
    A = len(_gateset(kind, n))
    n_steps = cap + 1 if path == "step" else cap + 2
    assert plan(kind, n, STEP, batch=B, nonsymplectic=nonsymp, num_actions=A, **cfg) == step_k
    assert plan(kind, n, FUSED, batch=B, arg=n_steps, nonsymplectic=nonsymp, num_actions=A, **cfg) == fused_k
    _, gv, m = _make(kind, n, B, cfg)
    rng = np.random.default_rng(31 * n + len(path) + 7 * nonsymp)
    circs, start = _targets(m, rng, cap, nonsymplectic=bool(nonsymp))
    coins_on = opts["add_inverts"]
    # an env that misses n_steps - cap pushes ends with exactly cap of them: full by another route, and clean
    acts, coins, fed = _schedule(m, rng, circs, n_steps, coins_on, misses=n_steps - cap)
    counts = _dry_counts(kind, A, acts)
    over = counts > cap
    assert (_dry_counts(kind, A, acts[:cap]) <= cap).all()
    _assert_waves_hold_both(kind, over, fed, "inputs")
    if kind == "permutation":
        assert (counts[fed] == cap).all() and over[~fed].all()
    else:
        assert over.all()
    m.set_state(m.wire(start))
    gv.set_state(m.wire(start))
    assert (m.depth == cap).all()
    rec = PushRecorder(kind, B, A)
    adt = torch.int64 if n % 2 else torch.int32
    dev_coins = (lambda c: _dev(c, torch.uint8)) if coins_on else (lambda c: None)

    if path == "step":
        for t in range(cap):
            rec.note_model(m, acts[t])
            m.step(acts[t], coins[t])
            gv.step(_dev(acts[t], adt), dev_coins(coins[t]))
        # exactly full: the last slot is written, nothing is reported
        assert m.success[::2].all() and (m.depth == 0).all()  # (the replayed episodes are legal and max_depth steps long)
        np.testing.assert_array_equal(gv.faults(), np.zeros(B, np.uint32), err_msg="faults of a full log")
        gv.sync()
        full = _expect_log(gv, rec, cap, "full")
        np.testing.assert_array_equal(full, _dry_counts(kind, A, acts[:cap]))
        want = [[reported(v, kind) for v in s] for s in m.solutions()]
        assert rec.expected_log(cap) == want  # the recorder and the model agree while nothing is dropped
        _expect(gv, m, "full")
        # one more: dropped and reported, everything else as in the model
        rec.note_model(m, acts[cap])
        m.step(acts[cap], coins[cap])
        gv.step(_dev(acts[cap], adt), dev_coins(coins[cap]))
        _expect(gv, m, "one more")
        assert (m.depth == 0).all()
        lens = _expect_log(gv, rec, cap, "one more")
        np.testing.assert_array_equal(lens[rec.overflowed(cap)], full[rec.overflowed(cap)], err_msg="an overflowing env's length moved")
    else:
        rew, fin = np.zeros((n_steps, B), np.float32), np.zeros((n_steps, B), np.uint8)
        for t in range(n_steps):
            rec.note_model(m, acts[t])
            m.step(acts[t], coins[t])
            rew[t], fin[t] = m.reward, m.is_final()
        rew_out = torch.zeros((n_steps, B), dtype=torch.float32, device="cuda")
        fin_out = torch.zeros((n_steps, B), dtype=torch.uint8, device="cuda")
        gv.rollout(_dev(acts, adt), fused=path == "fused", coins=dev_coins(coins), rewards_out=rew_out, dones_out=fin_out)
        np.testing.assert_array_equal(f32_bits(rew_out.cpu().numpy()), f32_bits(rew), err_msg="per-step rewards")
        np.testing.assert_array_equal(fin_out.cpu().numpy(), fin, err_msg="per-step dones")
        _expect(gv, m, "end")
        _expect_log(gv, rec, cap, "end")
    np.testing.assert_array_equal(rec.overflowed(cap), over)
    _expect_overflow(gv, rec, cap, "end")


# ---- (b) a wave that holds both ---------------------------------------------------------------------------------------------------
ONE_LAUNCH = [
    # row of ROWS, difficulty, depth_slope -> the kernel reset_done_step runs as one launch
    (0, 1, 4, "qm_reset_step_kernel"),
    (3, 1, 4, "q64_reset_step_kernel"),
    (8, 1, 4, "qm_reset_step_kernel"),
    (9, 1, 4, "q64_reset_step_kernel"),
    (6, 1, 4, "word_reset_step_kernel"),
    (7, 1, 4, "word_reset_step_kernel"),
    (12, 1, 4, "word_reset_step_kernel"),
    (13, 1, 4, "word_reset_step_kernel"),
    # with add_inverts the one launch is taken from 64 scramble draws on (qgym_plan.hpp reset_step_pays): the fresh depth is then
    # max_depth itself, and the second episode still stays below the capacity because it starts at step 3
    (1, 64, 1, "qm_reset_inv2_step_kernel"),
]


def _mixed_wave(kind, n, opts, nonsymp, diff, slope, one_launch):
    cap = CAP
    cfg = dict(opts, max_depth=cap, difficulty=diff, depth_slope=slope)
    A = len(_gateset(kind, n))
    if one_launch is not None:
        assert str(plan(kind, n, RESET_DONE_STEP, batch=B, num_actions=A, **cfg)).startswith(one_launch)
    _, gv, m = _make(kind, n, B, cfg)
    rng = np.random.default_rng(17 * n + diff + 3 * nonsymp)
    circs, start = _targets(m, rng, 2, nonsymplectic=bool(nonsymp))  # the even envs solve within 2 steps
    coins_on = opts["add_inverts"]
    n_steps = cap + 1
    acts, coins, fed = _schedule(m, rng, circs, n_steps + 1, coins_on, misses=1)
    m.set_state(m.wire(start))
    gv.set_state(m.wire(start))
    rec = PushRecorder(kind, B, A)
    dev_coins = (lambda c: _dev(c, torch.uint8)) if coins_on else (lambda c: None)

    def model_reset(seed):
        done = m.is_final().copy()
        m.reset_with(_draws(seed, np.flatnonzero(done), B, diff, A), mask=done)
        rec.clear(done)
        return done

    def model_step(t):
        rec.note_model(m, acts[t])
        m.step(acts[t], coins[t])

    resets = 0
    for t in range(n_steps):
        if one_launch is not None and t < cap:  # the collection loop's call; the step past the capacity is a plain one
            resets += int(model_reset(300 + t)[::2].sum())
            model_step(t)
            gv.reset_done_step(300 + t, _dev(acts[t], torch.int32), dev_coins(coins[t]))
            continue
        if one_launch is None and t == 2:
            resets += int(model_reset(77)[::2].sum())
            gv.reset_done(77)
        model_step(t)
        gv.step(_dev(acts[t], torch.int32), dev_coins(coins[t]))
    assert resets >= B // 2  # every even env started a second episode
    over = rec.overflowed(cap)
    assert not over[::2].any()
    _assert_waves_hold_both(kind, over, fed, "inputs")
    # odd envs carry bit 8 and the truncated log, even envs 0 and the full log of their latest episode, lane beside lane
    _expect(gv, m, "past the capacity")
    _expect_log(gv, rec, cap, "past the capacity")
    _expect_overflow(gv, rec, cap, "past the capacity")
    # one more reset of the finished envs clears their words and logs
    done = m.is_final().copy()
    assert done[over].all()
    if one_launch is not None:
        model_reset(999)
        model_step(n_steps)
        gv.reset_done_step(999, _dev(acts[n_steps], torch.int32), dev_coins(coins[n_steps]))
    else:
        model_reset(999)
        gv.reset_done(999)
        assert (rec.counts()[done] == 0).all()
    faults = gv.faults()
    assert (faults[done] == 0).all() and not faults.any()
    gv.sync()
    _expect(gv, m, "after the last reset")
    _expect_log(gv, rec, cap, "after the last reset")


@pytest.mark.parametrize("kind,n,opts,nonsymp,step_k,fused_k", ROWS, ids=ROW_IDS)
def test_overflowing_and_fresh_envs_share_a_wave(kind, n, opts, nonsymp, step_k, fused_k):
    A = len(_gateset(kind, n))
    assert plan(kind, n, STEP, batch=B, nonsymplectic=nonsymp, num_actions=A, **dict(opts, max_depth=CAP, difficulty=1, depth_slope=4)) == step_k
    _mixed_wave(kind, n, opts, nonsymp, 1, 4, None)


@pytest.mark.parametrize("row,diff,slope,want", ONE_LAUNCH, ids=[f"{ROW_IDS[r[0]]}-{r[3]}" for r in ONE_LAUNCH])
def test_overflowing_and_fresh_envs_share_a_wave_reset_done_step(row, diff, slope, want):
    kind, n, opts, nonsymp, _, _ = ROWS[row]
    _mixed_wave(kind, n, opts, nonsymp, diff, slope, want)


# ---- (c) PauliEnv -----------------------------------------------------------------------------------------------------------------
def _pauli_config(max_rot, max_depth):
    return dict(add_perms=False, track_solution=True, max_rotations=max_rot, max_depth=max_depth, difficulty=max_depth // 2, depth_slope=2,
                pauli_layer_reward=0.0625, metrics_weights=W_COUNTS)


def _pauli_model(max_rot, max_depth, rng, n=6):
    """A PauliEnv model on targets that keep the full rmax = max_rotations + 2 rotations through the reset's clean, and the 6-gate circuits
    that solve them: three one-qubit gates, then CX(0, 1), CX(2, 3), CX(4, 5).  The rotations are the weight-1 Paulis that a CX of that
    layer spreads over both of its qubits (Z or Y on its first qubit, X or Y on its second, as the network evolves its rotations),
    conjugated by the circuit's inverse: all of weight 2 in the target, so the reset releases none (asserted); replaying the circuit
    releases those of a pair with the pair's CX."""
    gs = line_gateset("pauli", n)
    rmax = max_rot + 2
    cfg = _pauli_config(max_rot, max_depth)
    m = PauliModel(n, gs, B, **cfg)
    index = {g: a for a, g in enumerate(m.gateset)}
    layer = [index[("cx", (q, q + 1))] for q in range(0, n, 2)]
    one_q = [a for a, (_, qs) in enumerate(m.gateset) if len(qs) == 1]
    circs = np.concatenate([rng.choice(one_q, size=(B, 3)), np.tile(layer, (B, 1))], axis=1)
    pool = [(q, ax) for q in range(n) for ax in ((2, 3) if q % 2 == 0 else (1, 3))]  # (axis bits: 1 X, 2 Z, 3 Y)
    assert len(pool) >= rmax
    tabs, labs = [], []
    for b in range(B):
        picks = [pool[i] for i in rng.permutation(len(pool))[:rmax]]
        t, l = replay_target(m, circs[b], rmax, rng, paulis=picks)
        tabs.append(t)
        labs.append([x.lstrip("-") for x in l])  # (pauli_reset_from takes bare IXYZ strings)
    m.reset_from(tabs, labs)
    assert all(len(a) == rmax for a in m.active()) and (m.depth == max_depth).all()
    return gs, cfg, m, circs, rmax, tabs, labs


def _pauli_pair(max_rot, max_depth, rng):
    from qiskit_gym_amd.vec import VecEnv

    gs, cfg, m, circs, rmax, tabs, labs = _pauli_model(max_rot, max_depth, rng)
    gv = VecEnv("pauli", m.n, gs, B, **cfg)
    gv.pauli_reset_from(np.stack(tabs), labs)
    return gs, cfg, gv, m, circs, rmax


def _expect_pauli(gv, m, label):
    np.testing.assert_array_equal(f32_bits(gv.reward.cpu().numpy()), f32_bits(m.reward), err_msg=f"reward {label}")
    np.testing.assert_array_equal(gv.done.cpu().numpy(), m.is_final(), err_msg=f"done {label}")
    np.testing.assert_array_equal(gv.success.cpu().numpy(), m.success, err_msg=f"success {label}")
    np.testing.assert_array_equal(gv.depth.cpu().numpy(), m.depth, err_msg=f"depth {label}")
    np.testing.assert_array_equal(gv.get_state("i64").cpu().numpy(), m.tableau(), err_msg=f"tableau {label}")
    np.testing.assert_array_equal(gv.observe().cpu().numpy().reshape(B, -1), m.observe(), err_msg=f"observe {label}")


def _pauli_plans(max_rot, layout, step_k, fused_k, cfg, A, fused_steps):
    assert plan("pauli", 6, LAYOUT, batch=B, num_actions=A, **cfg) == layout
    assert plan("pauli", 6, STEP, batch=B, num_actions=A, **cfg) == step_k
    for T in fused_steps:
        assert plan("pauli", 6, FUSED, batch=B, arg=T, num_actions=A, **cfg) == fused_k


@pytest.mark.parametrize("path", ["step", "fused"])
@pytest.mark.parametrize("max_rot,layout,step_k,fused_k", PAULI_ROWS, ids=[f"r{r[0]}" for r in PAULI_ROWS])
def test_pauli_log_never_overflows_in_an_episode_and_truncates_at_whole_steps_after(max_rot, layout, step_k, fused_k, path):
    max_depth = 6
    rng = np.random.default_rng(max_rot + len(path))
    gs, cfg, gv, m, circs, rmax = _pauli_pair(max_rot, max_depth, rng)
    A = len(gs)
    cap = max_depth + rmax  # the documented capacity: max_depth steps plus one entry per rotation
    _pauli_plans(max_rot, layout, step_k, fused_k, cfg, A, (2, max_depth))
    _expect_pauli(gv, m, "entry")
    bounds = [{0} for _ in range(B)]  # the model's log lengths after whole steps

    def run(acts):
        """Steps [T, B] of in-range actions on the model and the device (one launch per step, or one fused rollout)."""
        for a in acts:
            m.step(a)
            for b in range(B):
                bounds[b].add(len(m.sol[b]))
        if path == "step":
            for a in acts:
                gv.step(_dev(a, torch.int32))
        else:
            gv.rollout(_dev(acts, torch.int32), fused=True)

    def device_logs():
        sol, lens = gv.solutions(cap=cap + 4)
        return [sol[b, : lens[b]].tolist() for b in range(B)], lens

    # an episode can never overflow: max_depth in-range steps, the even envs replaying their circuit, the odd ones acting at random
    acts = rng.integers(0, A, size=(max_depth, B))
    acts[:, ::2] = circs[::2].T
    run(acts)
    live = np.array([len(a) for a in m.active()])
    # about the inputs: the replaying envs released all rmax rotations and fill the log to its last slot; some others still hold rotations
    assert (live[::2] == 0).all() and m.success[::2].all() and (live[1::2] > 0).any()
    assert all(len(m.sol[b]) == cap for b in range(0, B, 2))
    np.testing.assert_array_equal(gv.faults(), np.zeros(B, np.uint32), err_msg="faults within an episode")
    gv.sync()
    _expect_pauli(gv, m, "episode")
    got, lens = device_logs()
    assert got == m.solutions() and (lens <= cap).all()

    # keep stepping in-range gates on the finished envs
    prev = np.zeros(B, np.uint32)
    for k in range((rmax + 4) // 2):
        run(rng.integers(0, A, size=(2, B)))
        _expect_pauli(gv, m, f"past the end {k}")
        faults = gv.faults()
        got, lens = device_logs()
        assert np.isin(faults, (0, OVERFLOW_BIT)).all() and (faults >= prev).all()  # nothing but bit 8, and it is sticky
        prev = faults
        for b in range(B):
            want = m.sol[b]
            if faults[b] == 0:
                assert got[b] == want, (k, b)
            else:  # a prefix made of whole steps (a gate entry with all its rotation entries), within the capacity
                assert lens[b] <= cap and got[b] == want[: lens[b]] and int(lens[b]) in bounds[b], (k, b)
            if len(want) > cap:
                assert faults[b] == OVERFLOW_BIT, (k, b)
    assert all(len(s) > cap for s in m.sol) and (prev == OVERFLOW_BIT).all()
    from qiskit_gym_amd._lib import QGymError

    with pytest.raises(QGymError, match="solution log overflow"):
        gv.sync()


# ---- (d) wild values --------------------------------------------------------------------------------------------------------------
def _wild_values(A, act64):
    if not act64:
        return [-1, A, -2**31, 2**31 - 1]
    return [-1, A, A + 3, 2**31 - 2, 2**31 - 1, 2**31, 2**32 - 2, 2**32 - 1, 2**32, 2**32 + 5, 2**32 + A - 1, -2**32 + 5, 2**63 - 1, -2**63]


def _wild_schedule(rng, A, act64, n_steps):
    """Actions [n_steps, B]: the envs b = 1 (mod 3) are fed the wild values in turn (every value in every wave at every step, valid
    actions in the lanes on both sides), the others act at random in range."""
    values = _wild_values(A, act64)
    acts = rng.integers(0, A, size=(n_steps, B)).astype(np.int64)
    wild = np.arange(B) % 3 == 1
    for t in range(n_steps):
        acts[t, wild] = [values[(b // 3 + t) % len(values)] for b in np.flatnonzero(wild)]
        for w in range(B // 64):
            assert set(values) <= set(acts[t, 64 * w: 64 * w + 64].tolist())
    return acts, wild, values


BITS_0_OR_1 = f32_bits(np.array([0, 1], np.float32))


@pytest.mark.parametrize("act64", [True, False], ids=["i64", "i32"])
@pytest.mark.parametrize("path", ["step", "fused"])
@pytest.mark.parametrize("kind,n,opts,nonsymp,step_k,fused_k", ROWS, ids=ROW_IDS)
def test_wild_action_values(kind, n, opts, nonsymp, step_k, fused_k, path, act64):
    cap, T = 16, 8  # nothing overflows
    cfg = dict(opts, max_depth=cap)
    A = len(_gateset(kind, n))
    assert plan(kind, n, STEP, batch=B, nonsymplectic=nonsymp, num_actions=A, **cfg) == step_k
    assert plan(kind, n, FUSED, batch=B, arg=T, nonsymplectic=nonsymp, num_actions=A, **cfg) == fused_k
    _, gv, m = _make(kind, n, B, cfg)
    rng = np.random.default_rng(13 * n + 2 * act64 + len(path) + 5 * nonsymp)
    _, start = _targets(m, rng, 4, nonsymplectic=bool(nonsymp))
    acts, wild, values = _wild_schedule(rng, A, act64, T)
    coins_on = opts["add_inverts"]
    coins = rng.integers(0, 2, size=(T, B)) if coins_on else np.zeros((T, B), np.int64)
    m.set_state(m.wire(start))
    gv.set_state(m.wire(start))
    rec = PushRecorder(kind, B, A)
    adt = torch.int64 if act64 else torch.int32
    dev_coins = (lambda c: _dev(c, torch.uint8)) if coins_on else (lambda c: None)
    rew, fin = np.zeros((T, B), np.float32), np.zeros((T, B), np.uint8)
    lens = np.zeros(B, np.int64)
    for t in range(T):
        rec.note_model(m, acts[t])
        m.step(acts[t], coins[t])
        rew[t], fin[t] = m.reward, m.is_final()
        assert np.isin(f32_bits(m.reward[wild]), BITS_0_OR_1).all()  # no gate, no penalty
        if path == "step":
            gv.step(_dev(acts[t], adt), dev_coins(coins[t]))
            gv.sync()
            _expect(gv, m, f"t={t}")
            now = _expect_log(gv, rec, cap, f"t={t}")
            if kind == "permutation":
                np.testing.assert_array_equal(now[wild], lens[wild], err_msg="an out-of-range action moved a PermutationEnv log")
            lens = now
    if path == "fused":
        rew_out = torch.zeros((T, B), dtype=torch.float32, device="cuda")
        fin_out = torch.zeros((T, B), dtype=torch.uint8, device="cuda")
        gv.rollout(_dev(acts, adt), fused=True, coins=dev_coins(coins), rewards_out=rew_out, dones_out=fin_out)
        gv.sync()
        np.testing.assert_array_equal(f32_bits(rew_out.cpu().numpy()), f32_bits(rew), err_msg="per-step rewards")
        np.testing.assert_array_equal(fin_out.cpu().numpy(), fin, err_msg="per-step dones")
        _expect(gv, m, "end")
        lens = _expect_log(gv, rec, cap, "end")
    np.testing.assert_array_equal(gv.faults(), np.zeros(B, np.uint32))
    if kind == "permutation":
        assert (lens[wild] == 0).all() and (lens[~wild] == T).all()
    else:
        assert (lens == T).all()
        assert rec.expected_log(cap) == [[reported(v, kind) for v in s] for s in m.solutions()]
        frames = {(a, inv) for b in np.flatnonzero(wild) for a, inv in rec.pushes[b]}
        for v in values:  # every value was logged, with add_inverts in both frames
            assert (v, False) in frames and ((v, True) in frames or not coins_on), v


@pytest.mark.parametrize("act64", [True, False], ids=["i64", "i32"])
@pytest.mark.parametrize("path", ["step", "fused"])
@pytest.mark.parametrize("max_rot,layout,step_k,fused_k", PAULI_ROWS, ids=[f"r{r[0]}" for r in PAULI_ROWS])
def test_wild_action_values_pauli(max_rot, layout, step_k, fused_k, path, act64):
    max_depth, T = 16, 8
    rng = np.random.default_rng(50 + max_rot + 2 * act64 + len(path))
    gs, cfg, gv, m, circs, rmax = _pauli_pair(max_rot, max_depth, rng)
    A = len(gs)
    _pauli_plans(max_rot, layout, step_k, fused_k, cfg, A, (T,))
    acts, wild, _ = _wild_schedule(rng, A, act64, T)
    replay = (np.arange(B) % 3 == 0) & (np.arange(B) % 2 == 0)
    acts[:6, replay] = circs[replay].T  # some envs release their rotations next to the wild lanes
    adt = torch.int64 if act64 else torch.int32
    rew, fin = np.zeros((T, B), np.float32), np.zeros((T, B), np.uint8)

    def expect_logs(label):
        sol, lens = gv.solutions(cap=max_depth + rmax)
        want = m.solutions()
        np.testing.assert_array_equal(lens, [len(w) for w in want], err_msg=f"log lengths {label}")
        for b in range(B):
            assert sol[b, : lens[b]].tolist() == want[b], (label, b)
        assert (lens[wild] == 0).all()  # PauliEnv logs in-range actions only

    for t in range(T):
        m.step(acts[t])
        rew[t], fin[t] = m.reward, m.is_final()
        assert np.isin(f32_bits(m.reward[wild]), BITS_0_OR_1).all()
        if path == "step":
            gv.step(_dev(acts[t], adt))
            gv.sync()
            _expect_pauli(gv, m, f"t={t}")
            expect_logs(f"t={t}")
    if path == "fused":
        rew_out = torch.zeros((T, B), dtype=torch.float32, device="cuda")
        fin_out = torch.zeros((T, B), dtype=torch.uint8, device="cuda")
        gv.rollout(_dev(acts, adt), fused=True, rewards_out=rew_out, dones_out=fin_out)
        gv.sync()
        np.testing.assert_array_equal(f32_bits(rew_out.cpu().numpy()), f32_bits(rew), err_msg="per-step rewards")
        np.testing.assert_array_equal(fin_out.cpu().numpy(), fin, err_msg="per-step dones")
        _expect_pauli(gv, m, "end")
        expect_logs("end")
    assert sum(e >= 0x80000000 for s in m.sol for e in s) >= rmax  # rotations were released and logged
    np.testing.assert_array_equal(gv.faults(), np.zeros(B, np.uint32))
