"""The one-step kernel of the TILE layout (qm_step1_kernel) takes the gate's two row groups from a table of one byte per action that a wave holds
across its lanes -- lane j the bytes of actions 4 j .. 4 j + 3, fetched by one permute -- so that the row loads leave before the gate entry has
arrived.  What can go wrong with that:

* the permute reads a lane that is not there: a wave at the batch's end has lanes without an env, which hold no table dword (such a wave takes the
  groups from the gate entry) -- so every batch size around a wave's and a workgroup's end is run with EVERY env taking the highest action ids
  (the dword of lane (A - 1) >> 2);
  Which path a case runs: only a wave with 64 envs takes the permute, so the batches of 1, 2 and 63 run the gate-entry path alone; at 64 every
  wave takes the permute; at 65, 255, 257 and 1 000 the whole waves take it and the last wave does not -- both paths in one launch;
* the table's edges: 1, 4, 5, 255, 256 actions, and 257, where every wave takes the groups from the gate entry;
* an action out of range (-1, A, A + 3, an int64 whose low half alone is in range) must be "no gate", not action 0's or a neighbour's groups;
* the groups themselves: qubits in one group (even and odd), in neighbouring groups in both operand orders, in groups of equal parity and far
  apart, two-qubit gates on equal qubits;
* every form of the kernel: plain, with a solution log, with the resident dense observation, with the done list, eager and from a graph.

Every case: 64 steps of seeded random actions, bit-exact against the CPU oracle after every step -- reward bit patterns, success (the kernel's
incremental `solved` mask), is_final, depth -- and the rows (state and dense observation) at four of the steps and at the end."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

from util import f32_bits, line_gateset, make_pair  # noqa: E402

PLAIN = dict(add_inverts=False, add_perms=False, track_solution=False)
STEPS = 64
ONE = {"clifford": ["H", "S", "Sdg", "SX", "SXdg"], "linear_function": []}
TWO = {"clifford": ["CX", "CZ", "SWAP"], "linear_function": ["CX", "SWAP"]}


def _dev(a, dtype=None):
    return torch.as_tensor(np.ascontiguousarray(a), device="cuda").to(dtype or torch.int32)


def _dim(kind, n):
    return 2 * n if kind == "clifford" else n


def _start(ov, gv, kind, n, rng, A, scramble):
    """Every env at the identity (success flips in the first steps), or scrambled by 2 n random gates."""
    if scramble:
        draws = rng.integers(0, A, size=(2 * n, gv.batch))
        ov.proto.difficulty = 2 * n
        for i in range(ov.batch):
            ov.env(i).difficulty = 2 * n
        gv.difficulty = 2 * n
        ov.reset_with(draws)
        gv.reset_with(_dev(draws))
    else:
        d = _dim(kind, n)
        states = np.tile(np.eye(d, dtype=np.int64).reshape(-1), (gv.batch, 1))
        ov.set_state(states)
        gv.set_state(states)


def _same_outputs(gv, want, label):
    r_o, s_o, f_o, d_o = want
    gv.sync()
    np.testing.assert_array_equal(f32_bits(gv.reward.cpu().numpy()), f32_bits(r_o), err_msg=f"reward {label}")
    np.testing.assert_array_equal(gv.success.cpu().numpy(), s_o, err_msg=f"success {label}")
    np.testing.assert_array_equal(gv.done.cpu().numpy(), f_o, err_msg=f"is_final {label}")
    np.testing.assert_array_equal(gv.depth.cpu().numpy(), d_o, err_msg=f"depth {label}")


def _same_rows(ov, gv, kind, n, label):
    d = _dim(kind, n)
    np.testing.assert_array_equal(gv.get_state("i64").cpu().numpy(), ov.get_state(d * d), err_msg=f"state {label}")
    np.testing.assert_array_equal(gv.observe().cpu().numpy().reshape(gv.batch, -1), ov.observe_dense(), err_msg=f"obs {label}")


def _actions(rng, A, B, mode):
    """[STEPS, B].  "random": uniform; "top": every env one of the (at most four) highest ids -- one table dword, the last one in use;
    "mixed": uniform with one lane in five out of range."""
    if mode == "top":
        return rng.integers(max(A - 4, 0), A, size=(STEPS, B))
    acts = rng.integers(0, A, size=(STEPS, B))
    if mode == "mixed":
        bad = rng.choice(np.array([-1, A, A + 3, A + 256, 2**31 - 1, -(2**31)]), size=(STEPS, B))
        acts = np.where(rng.integers(0, 5, size=(STEPS, B)) == 0, bad, acts)
    return acts


def _run(kind, n, gs, B, acts, *, seed, scramble, dtype=None, max_depth=40, cfg=PLAIN, after_step=None):
    ov, gv = make_pair(kind, n, gs, B, max_depth=max_depth, **cfg)
    _start(ov, gv, kind, n, np.random.default_rng(seed), len(gs), scramble)
    for t in range(acts.shape[0]):
        want = ov.step(acts[t].astype(np.int32))
        gv.step(_dev(acts[t], dtype))
        label = f"{kind}{n} A={len(gs)} B={B} t={t}"
        _same_outputs(gv, want, label)
        if t % 16 == 0 or t == acts.shape[0] - 1:
            _same_rows(ov, gv, kind, n, label)
        if after_step:
            after_step(ov, gv, t, want)
    return ov, gv


def _all_pairs_gateset(kind, n, A, seed):
    """A gateset of exactly A actions: the line's, then every other ordered pair of qubits (equal qubits too), shuffled."""
    gs = list(line_gateset(kind, n))
    have = set(gs)
    rest = [(g, (a, b)) for g in TWO[kind] for a in range(n) for b in range(n) if (g, (a, b)) not in have]
    order = np.random.default_rng(seed).permutation(len(rest))
    gs += [rest[i] for i in order]
    gs = [gs[i] for i in np.random.default_rng(seed + 1).permutation(len(gs))]
    assert len(gs) >= A
    return gs[:A]


# ---- batch sizes: a wave's and a workgroup's end, with the needed table dword in a lane past the batch's end ---------------------------------
@pytest.mark.parametrize("mode", ["random", "top"])
@pytest.mark.parametrize("B", [1, 2, 63, 64, 65, 255, 257, 1000])
def test_batch_sizes(B, mode):
    kind, n = "clifford", 16
    gs = line_gateset(kind, n)
    assert len(gs) == 170  # lane 42 holds the highest ids' bytes: past the end of the batches of 1 and 2, and of the last wave of 65, 257 and 1000
    rng = np.random.default_rng(1000 + B)
    _run(kind, n, gs, B, _actions(rng, len(gs), B, mode), seed=B, scramble=(B % 2 == 1))


# ---- action counts: the table's first dword, a dword's edge, the last lane, and the fallback ---------------------------------------------------
@pytest.mark.parametrize("A", [1, 4, 5, 255, 256, 257])
def test_action_counts(A):
    kind, n, B = "clifford", 16, 130  # two whole waves and a ragged one
    gs = _all_pairs_gateset(kind, n, A, seed=A)
    rng = np.random.default_rng(2000 + A)
    acts = _actions(rng, A, B, "mixed")
    acts[1::2] = rng.integers(0, A, size=acts[1::2].shape)  # (odd steps: every action in range)
    acts[3::8] = _actions(rng, A, B, "top")[3::8]
    _run(kind, n, gs, B, acts, seed=A, scramble=False)


def test_action_counts_linear_function():
    kind, n, B = "linear_function", 32, 130
    for A in (255, 256, 257):
        gs = _all_pairs_gateset(kind, n, A, seed=A)
        acts = _actions(np.random.default_rng(2100 + A), A, B, "mixed")[:32]
        _run(kind, n, gs, B, acts, seed=A, scramble=True)


# ---- out of range --------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("adt", ["int32", "int64"])
def test_out_of_range_actions(adt):
    """-1, A, A + 3 beside lanes in range; int64: values whose low half alone is in range (2^32 + k, -2^32 + k) -- all "no gate": the rows stay,
    depth and reward move.  Action 0 of this gateset spans two groups, so "no gate" taking action 0's groups would still be right only by the
    identity map on them; the neighbours' groups are checked by the state."""
    kind, n, B = "clifford", 16, 130
    gs = [("CX", (1, 2))] + list(line_gateset(kind, n))
    A = len(gs)
    rng = np.random.default_rng(3000)
    acts = rng.integers(0, A, size=(STEPS, B)).astype(np.int64)
    oor = [-1, A, A + 3]
    if adt == "int64":
        oor += [2**32 + 5, -(2**32) + 7, 2**32 * 3 + (A - 1), -(2**63) + 1]
    pick = rng.choice(np.array(oor, dtype=np.int64), size=(STEPS, B))
    acts = np.where(rng.integers(0, 3, size=(STEPS, B)) == 0, pick, acts)
    acts[5] = pick[5]  # a step in which no lane has a gate
    ov, gv = make_pair(kind, n, gs, B, max_depth=40, **PLAIN)
    _start(ov, gv, kind, n, rng, A, True)
    for t in range(STEPS):
        inside = (acts[t] >= 0) & (acts[t] < A)
        before = gv.get_state("i64").cpu().numpy()
        want = ov.step(np.where(inside, acts[t], -1).astype(np.int32))  # (the oracle takes int32: every value out of range is one "no gate")
        gv.step(_dev(acts[t], getattr(torch, adt)))
        _same_outputs(gv, want, f"oor {adt} t={t}")
        after = gv.get_state("i64").cpu().numpy()
        np.testing.assert_array_equal(after[~inside], before[~inside], err_msg=f"rows of the envs without a gate, t={t}")
        if t % 16 == 0 or t == STEPS - 1:
            _same_rows(ov, gv, kind, n, f"oor {adt} t={t}")


# ---- gatesets ------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind,n", [("clifford", 3), ("clifford", 4), ("clifford", 16), ("linear_function", 9), ("linear_function", 32)])
def test_line_gatesets(kind, n):
    B = 130
    gs = line_gateset(kind, n)
    rng = np.random.default_rng(4000 + n)
    _run(kind, n, gs, B, _actions(rng, len(gs), B, "mixed"), seed=n, scramble=(kind == "linear_function"))


@pytest.mark.parametrize("kind,n", [("clifford", 16), ("linear_function", 32), ("linear_function", 12)])
def test_groups_of_equal_parity_far_apart_and_both_operand_orders(kind, n):
    """Edges (0,4), (1,9), (2,3) and (1,2), (5,6), (3,4), each in both orders, and two-qubit gates on equal qubits.  CliffordEnv (two qubits a
    group): groups 0|2, 0|4 (equal parity), 1|1 (one odd group), 0|1 and 2|3 (neighbours), 1|2 (neighbours, the odd one first).
    LinearFunctionEnv (four rows a group): 0|1, 0|2, 0|0, 0|0, 1|1, 0|1."""
    B = 130
    edges = [(0, 4), (1, 9), (2, 3), (1, 2), (5, 6), (3, 4)]
    gs = []
    for a, b in edges:
        for g in TWO[kind]:
            gs += [(g, (a, b)), (g, (b, a))]
    gs += [(g, (q, q)) for g in TWO[kind] for q in (0, 3, n - 1)]
    gs += [(g, (q,)) for g in ONE[kind] for q in (0, 1, 2, 3, n - 1)]
    rng = np.random.default_rng(4100 + n)
    acts = _actions(rng, len(gs), B, "random")
    acts[7] = (np.arange(B) * 7) % len(gs)  # neighbouring lanes: neighbouring actions
    _run(kind, n, gs, B, acts, seed=n, scramble=True)


# ---- the kernel's forms -----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind,n,B", [("clifford", 16, 130), ("linear_function", 9, 65)])
def test_solution_log_form(kind, n, B):
    """FEAT (track_solution): the log holds max_depth entries, one per step."""
    gs = line_gateset(kind, n)
    rng = np.random.default_rng(5000 + n)
    acts = _actions(rng, len(gs), B, "random")
    acts[3::8] = _actions(rng, len(gs), B, "top")[3::8]
    ov, gv = _run(kind, n, gs, B, acts, seed=n, scramble=True, max_depth=STEPS, cfg=dict(PLAIN, track_solution=True))
    for e in (0, 1, 63, 64, B - 1):
        assert gv.solution(e) == ov.env(e).solution(), e


@pytest.mark.parametrize("kind,n,B", [("clifford", 8, 65), ("clifford", 16, 130), ("linear_function", 32, 131)])
def test_tracked_dense_form(kind, n, B):
    """DENSE: the resident dense observation follows every step (B = 131: the last env has no partner lane)."""
    gs = line_gateset(kind, n)
    rng = np.random.default_rng(5100 + n)
    acts = _actions(rng, len(gs), B, "mixed")
    acts[3::8] = _actions(rng, len(gs), B, "top")[3::8]
    ov, gv = make_pair(kind, n, gs, B, max_depth=40, **PLAIN)
    _start(ov, gv, kind, n, rng, len(gs), True)
    tracked = gv.track_dense()
    for t in range(STEPS):
        want = ov.step(acts[t].astype(np.int32))
        gv.step(_dev(acts[t]))
        _same_outputs(gv, want, f"dense {kind}{n} t={t}")
        np.testing.assert_array_equal(tracked.cpu().numpy().reshape(B, -1), ov.observe_dense(), err_msg=f"tracked dense t={t}")
    _same_rows(ov, gv, kind, n, "dense, end")


@pytest.mark.parametrize("kind,n,B", [("clifford", 16, 130), ("clifford", 16, 2), ("linear_function", 12, 65)])
def test_done_list_form(kind, n, B):
    """LIST: a handle on which reset_done is in use -- a reset_done after every fourth step."""
    gs = line_gateset(kind, n)
    rng = np.random.default_rng(5200 + n + B)
    acts = _actions(rng, len(gs), B, "random")
    acts[2::4] = _actions(rng, len(gs), B, "top")[2::4]
    resets = [0]

    def after_step(ov, gv, t, want):
        done = want[2].astype(bool)
        if t % 4 == 3 and done.any():
            gv.reset_done(800 + t)
            ov.reset_seeded(800 + t, mask=done)
            resets[0] += int(done.sum())
            _same_rows(ov, gv, kind, n, f"after reset_done t={t}")

    _run(kind, n, gs, B, acts, seed=n, scramble=True, max_depth=5, cfg=dict(PLAIN, difficulty=2), after_step=after_step)
    assert resets[0] >= B


@pytest.mark.parametrize("B", [2, 130])
def test_eager_and_graph_replays_agree(B):
    """The same 64 steps eager and as rollout_ring replays (eight of eight steps): the oracle's outputs after each replay, the same rows at the end."""
    kind, n, T = "clifford", 16, 8
    gs = line_gateset(kind, n)
    rng = np.random.default_rng(5300 + B)
    host = _actions(rng, len(gs), B, "mixed")
    host[3::8] = _actions(rng, len(gs), B, "top")[3::8]
    ov, eager = _run(kind, n, gs, B, host, seed=B, scramble=True)
    ov2, ring = make_pair(kind, n, gs, B, max_depth=40, **PLAIN)
    _start(ov2, ring, kind, n, np.random.default_rng(B), len(gs), True)
    for rep in range(STEPS // T):
        block = host[rep * T:(rep + 1) * T]
        for t in range(T):
            want = ov2.step(block[t].astype(np.int32))
        ring.rollout_ring(_dev(block), T)
        _same_outputs(ring, want, f"replay {rep}")
    _same_rows(ov2, ring, kind, n, "graph, end")
    assert torch.equal(eager.get_state("i64"), ring.get_state("i64"))
    for name in ("reward", "done", "success", "depth"):
        assert torch.equal(getattr(eager, name), getattr(ring, name)), name
