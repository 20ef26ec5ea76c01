"""The one-step kernel of the TILE layout has a straight-line form (qm_step1_straight_kernel) for the launches in which the host knows what the generic
kernel decides in every wave: int32 actions, a batch of whole waves, at most 256 actions, no rewards_seq / dones_seq, no kernel clock, no solution log,
done list or tracked observation (qgym_plan.hpp step1_straight; its conditions one by one: test_step1_straight_plan.py).  What can go wrong with that:

* the wrong form for a launch -- so every reason for falling back is run beside the straight form, on the same actions: batches of 1, 63 and 65 envs,
  int64 actions, rollout(..., rewards_out, dones_out), a kernel clock attached, 257 actions;
* a form cached with a graph outliving its reason -- rollout_ring replays before, while and after a kernel clock is attached;
* the 32-bit lane offsets and the whole-wave exit -- 64, 128, 256 and 320 envs: one wave, two waves, one workgroup, a last workgroup of one wave;
* the table's last lane -- a gateset of exactly 256 actions with every env taking the highest ids.

Every batch: 64 steps against the CPU oracle, computed once per (env, batch) and shared by every way of running them.  Actions are uniform over the range,
with -1 and A + 3 in some lanes of every step; a third of the lanes take a self-inverse gate twice in a row from the identity, so that success and is_final
flip in both directions, and depth reaches 0 inside the run.  After every step: reward bits, is_final, success, depth and the packed observation;
at the end every row."""
import functools

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

from util import f32_bits, line_gateset, make_pair  # noqa: E402

STEPS, T = 64, 8
ENVS = [("clifford", 16), ("clifford", 4), ("linear_function", 12)]
STRAIGHT = [64, 128, 256, 320]
GENERIC = [1, 63, 65]
SELF_INVERSE = ("H", "CX", "CZ", "SWAP")


def _dev(a, dtype=None):
    return torch.as_tensor(np.ascontiguousarray(a), device="cuda").to(dtype or torch.int32)


def _cfg(kind, n):
    difficulty = 1 if n == 4 else 2
    return dict(add_inverts=False, add_perms=False, track_solution=False, difficulty=difficulty, depth_slope=12, max_depth=40)


def _schedule(gs, B, difficulty, seed):
    """(draws [difficulty, B], acts [STEPS, B])."""
    rng = np.random.default_rng(seed)
    A = len(gs)
    inv = np.array([i for i, (g, _) in enumerate(gs) if g in SELF_INVERSE])
    lanes = np.arange(B)
    pair = lanes % 3 == 0
    draws = rng.integers(0, A, size=(difficulty, B))
    first = inv[rng.integers(0, len(inv), size=B)]
    draws[:, pair] = first[pair]  # difficulty 2: (a, a) -- the identity; 1: (a), undone by the first step
    acts = rng.integers(0, A, size=(STEPS, B))
    off = difficulty % 2
    if off:
        acts[0, pair] = first[pair]
    for t in range(off, STEPS - 1, 2):  # the pair lanes: a self-inverse gate twice -- or "no gate" twice
        a = inv[rng.integers(0, len(inv), size=B)]
        k = t // 2
        a = np.where((lanes + k) % 7 == 1, -1, np.where((lanes + k) % 7 == 2, A + 3, a))
        acts[t, pair] = a[pair]
        acts[t + 1, pair] = a[pair]
    for t in range(STEPS):
        acts[t, ~pair & ((lanes + t) % 7 == 1)] = -1
        acts[t, ~pair & ((lanes + t) % 7 == 2)] = A + 3
    return draws, acts


def _packed_of(ov, gv):
    """observe_packed: word r of an env = the bits of row r of its dense observation."""
    r, c = gv.obs_shape_
    dense = ov.observe_dense().reshape(gv.batch, r, c).astype(np.uint64)
    return (dense << np.arange(c, dtype=np.uint64)).sum(axis=2)


def _packed(gv):
    r, _ = gv.obs_shape_
    return gv.observe_packed().cpu().numpy().view({1: np.uint8, 4: np.uint32, 8: np.uint64}[gv.packed_word_bytes]).astype(np.uint64)[:, :r]


@functools.lru_cache(maxsize=None)
def _reference(kind, n, B, gs_key=None):
    """The oracle's 64 steps: per step (reward bits, success, is_final, depth, packed observation), and the rows at the end.  Never modified."""
    gs = _gateset(kind, n, gs_key)
    cfg = _cfg(kind, n)
    ov, gv = make_pair(kind, n, gs, B, **cfg)
    if gs_key is None:
        draws, acts = _schedule(gs, B, cfg["difficulty"], seed=100 * n + B)
    else:  # every env one of the four highest ids (the table's last dword in use)
        rng = np.random.default_rng(gs_key)
        draws, acts = rng.integers(0, len(gs), size=(cfg["difficulty"], B)), rng.integers(len(gs) - 4, len(gs), size=(STEPS, B))
    ov.reset_with(draws)
    steps = []
    for t in range(STEPS):
        r, s, f, d = ov.step(acts[t].astype(np.int32))
        steps.append((f32_bits(r).copy(), np.array(s), np.array(f), np.array(d), _packed_of(ov, gv)))
    d = 2 * n if kind == "clifford" else n
    ref = dict(gs=gs, cfg=cfg, draws=draws, acts=acts, steps=steps, state=ov.get_state(d * d).copy(), dense=ov.observe_dense().copy())
    if gs_key is None and B >= 63:  # the run does what the header says
        succ = np.stack([s[1] for s in steps]).astype(np.int8)
        fin = np.stack([s[2] for s in steps]).astype(np.int8)
        depth = np.stack([s[3] for s in steps])
        assert (np.diff(succ, axis=0) == 1).any() and (np.diff(succ, axis=0) == -1).any(), "success flips in both directions"
        assert (np.diff(fin, axis=0) == 1).any() and (np.diff(fin, axis=0) == -1).any(), "is_final flips in both directions"
        assert (depth[:8] > 0).all() and (depth[-8:] == 0).all(), "depth reaches 0 inside the run"
    return ref


def _gateset(kind, n, gs_key):
    gs = list(line_gateset(kind, n))
    if gs_key is None:
        return gs
    return [gs[i % len(gs)] for i in range(gs_key)]  # exactly gs_key actions: the set's entries repeated


def _fresh(kind, n, B, ref):
    from qiskit_gym_amd.vec import VecEnv

    gv = VecEnv(kind, n, ref["gs"], B, **ref["cfg"])
    gv.reset_with(_dev(ref["draws"]))
    return gv


def _same_step(gv, ref, t, label, packed=True):
    r, s, f, d, p = ref["steps"][t]
    gv.sync()
    np.testing.assert_array_equal(f32_bits(gv.reward.cpu().numpy()), r, err_msg=f"reward {label} t={t}")
    np.testing.assert_array_equal(gv.done.cpu().numpy(), f, err_msg=f"is_final {label} t={t}")
    np.testing.assert_array_equal(gv.success.cpu().numpy(), s, err_msg=f"success {label} t={t}")
    np.testing.assert_array_equal(gv.depth.cpu().numpy(), d, err_msg=f"depth {label} t={t}")
    if packed:
        np.testing.assert_array_equal(_packed(gv), p, err_msg=f"packed observation {label} t={t}")


def _same_end(gv, ref, label):
    np.testing.assert_array_equal(gv.get_state("i64").cpu().numpy(), ref["state"], err_msg=f"state {label}")
    np.testing.assert_array_equal(gv.observe().cpu().numpy().reshape(gv.batch, -1), ref["dense"], err_msg=f"obs {label}")


ALL = [(k, n, B) for k, n in ENVS for B in STRAIGHT + GENERIC]
# the other ways of running the same steps: every batch of the headline env, one straight and one generic batch of the others
SOME = [(k, n, B) for k, n in ENVS for B in STRAIGHT + GENERIC if (k, n) == ENVS[0] or B in (320, 65)]


@pytest.mark.parametrize("kind,n,B", ALL)
def test_step_by_step(kind, n, B):
    ref = _reference(kind, n, B)
    gv = _fresh(kind, n, B, ref)
    for t in range(STEPS):
        gv.step(_dev(ref["acts"][t]))
        _same_step(gv, ref, t, f"{kind}{n} B={B}")
    _same_end(gv, ref, f"{kind}{n} B={B}")


@pytest.mark.parametrize("kind,n,B", SOME)
def test_int64_actions_take_the_generic_form(kind, n, B):
    ref = _reference(kind, n, B)
    gv = _fresh(kind, n, B, ref)
    for t in range(STEPS):
        gv.step(_dev(ref["acts"][t], torch.int64))
        _same_step(gv, ref, t, f"int64 {kind}{n} B={B}", packed=(t % T == T - 1))
    _same_end(gv, ref, f"int64 {kind}{n} B={B}")


@pytest.mark.parametrize("kind,n,B", SOME)
def test_ring_replays(kind, n, B):
    """rollout_ring replays of 8 steps: the graph caches the form."""
    ref = _reference(kind, n, B)
    gv = _fresh(kind, n, B, ref)
    for rep in range(STEPS // T):
        gv.rollout_ring(_dev(ref["acts"][rep * T:(rep + 1) * T]), T)
        _same_step(gv, ref, rep * T + T - 1, f"ring {kind}{n} B={B}")
    _same_end(gv, ref, f"ring {kind}{n} B={B}")


@pytest.mark.parametrize("kind,n,B", SOME)
def test_rollout_with_sequence_outputs_takes_the_generic_form(kind, n, B):
    ref = _reference(kind, n, B)
    gv = _fresh(kind, n, B, ref)
    for rep in range(STEPS // T):
        rewards = torch.full((T, B), float("nan"), dtype=torch.float32, device="cuda")
        dones = torch.full((T, B), 7, dtype=torch.uint8, device="cuda")
        gv.rollout(_dev(ref["acts"][rep * T:(rep + 1) * T]), rewards_out=rewards, dones_out=dones)
        _same_step(gv, ref, rep * T + T - 1, f"rollout {kind}{n} B={B}")
        for t in range(T):
            np.testing.assert_array_equal(f32_bits(rewards[t].cpu().numpy()), ref["steps"][rep * T + t][0], err_msg=f"rewards_out rep={rep} t={t}")
            np.testing.assert_array_equal(dones[t].cpu().numpy(), ref["steps"][rep * T + t][2], err_msg=f"dones_out rep={rep} t={t}")
    _same_end(gv, ref, f"rollout {kind}{n} B={B}")


@pytest.mark.parametrize("kind,n,B", SOME)
def test_kernel_clock_attached_and_detached(kind, n, B):
    """Steps 0-15 without a clock, 16-31 with kernel_clock(8) attached (eight stamped launches, then eight with the slots used up), 32-63 detached again.
    The straight-line kernel has no clock: that the attached launches stamped their slots says the generic kernel ran them."""
    ref = _reference(kind, n, B)
    gv = _fresh(kind, n, B, ref)
    slots = None
    for t in range(STEPS):
        if t == 16:
            slots = gv.kernel_clock(8)
        if t == 32:
            gv.sync()
            stamps = slots.cpu().numpy()
            assert (stamps[:, 0, :] != 0).all(), "every attached launch stamps wave 0's record"
            assert (stamps[:, 0, 1] >= stamps[:, 0, 0]).all()
            gv.kernel_clock(0)
        gv.step(_dev(ref["acts"][t]))
        _same_step(gv, ref, t, f"clock {kind}{n} B={B}", packed=(t % T == T - 1))
    _same_end(gv, ref, f"clock {kind}{n} B={B}")
    assert np.array_equal(slots.cpu().numpy(), stamps), "no launch stamps a detached clock's slots"


@pytest.mark.parametrize("kind,n,B", SOME)
def test_ring_replays_across_a_kernel_clock(kind, n, B):
    """The same replays with a clock attached for replays 2 and 3: attaching and detaching drops the cached graphs (qg_vec_set_kernel_clock), so the
    graph captured with one form is never replayed for the other.  Replay 2's eight launches stamp the eight slots."""
    ref = _reference(kind, n, B)
    gv = _fresh(kind, n, B, ref)
    slots = None
    for rep in range(STEPS // T):
        if rep == 2:
            slots = gv.kernel_clock(T)
        if rep == 4:
            gv.sync()
            assert (slots[:, 0, :].cpu().numpy() != 0).all(), "the attached replay's launches stamp wave 0's record"
            gv.kernel_clock(0)
        gv.rollout_ring(_dev(ref["acts"][rep * T:(rep + 1) * T]), T)
        _same_step(gv, ref, rep * T + T - 1, f"ring+clock {kind}{n} B={B} rep={rep}")
    _same_end(gv, ref, f"ring+clock {kind}{n} B={B}")


@pytest.mark.parametrize("A", [256, 257])
@pytest.mark.parametrize("B", [128, 65])
def test_256_and_257_actions(A, B):
    """The 4-qubit set's entries repeated to exactly 256 actions (the table's last lane; straight form at 128 envs) and to 257 (generic form, groups from the
    gate entry); every env takes one of the four highest ids in every step."""
    kind, n = "clifford", 4
    ref = _reference(kind, n, B, A)
    assert len(ref["gs"]) == A
    gv = _fresh(kind, n, B, ref)
    for t in range(STEPS):
        gv.step(_dev(ref["acts"][t]))
        _same_step(gv, ref, t, f"A={A} B={B}")
    _same_end(gv, ref, f"A={A} B={B}")
    ring = _fresh(kind, n, B, ref)
    for rep in range(STEPS // T):
        ring.rollout_ring(_dev(ref["acts"][rep * T:(rep + 1) * T]), T)
    _same_step(ring, ref, STEPS - 1, f"ring A={A} B={B}")
    _same_end(ring, ref, f"ring A={A} B={B}")
