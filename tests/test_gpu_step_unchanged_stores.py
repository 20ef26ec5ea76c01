"""The one-step kernel of the TILE layout (qm_step1_kernel) stores depth, done and success only where the step changes them.  What can go
wrong with that: a value that changed is not stored (a compare against something other than what memory held), a store under a partial
execution mask reaches the wrong lanes.  The last test holds the kernel's two row groups to the oracle lane by lane -- qubits in one
group, in two, equal qubits -- whichever way the second group is fetched (fetching it only where it is another group was measured and
rejected, EXPERIMENTS.md round 9).  Every case is bit-exact against the CPU oracle after every step: reward bit patterns, success,
is_final, depth, state and observation.  B = 65 and 130: more than one wave, a ragged last one."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

from util import f32_bits, line_gateset, make_pair  # noqa: E402

PLAIN = dict(add_inverts=False, add_perms=False, track_solution=False)
SHAPES = [("clifford", 4), ("clifford", 16), ("linear_function", 12)]
BATCHES = [65, 130]


def _dev(a, dtype=None):
    return torch.as_tensor(np.ascontiguousarray(a), device="cuda").to(dtype or torch.int32)


def _dim(kind, n):
    return 2 * n if kind == "clifford" else n


def _from_identity(ov, gv, kind, n):
    """set_state: every env at the identity, depth = max_depth."""
    d = _dim(kind, n)
    states = np.tile(np.eye(d, dtype=np.int64).reshape(-1), (gv.batch, 1))
    ov.set_state(states)
    gv.set_state(states)


def _scramble(ov, gv, rng, n_draws, A):
    draws = rng.integers(0, A, size=(n_draws, gv.batch))
    ov.proto.difficulty = n_draws
    for i in range(ov.batch):
        ov.env(i).difficulty = n_draws
    gv.difficulty = n_draws
    ov.reset_with(draws)
    gv.reset_with(_dev(draws))


def _same_outputs(gv, want, label, done=None, depth=None):
    r_o, s_o, f_o, d_o = want
    gv.sync()
    np.testing.assert_array_equal(f32_bits(gv.reward.cpu().numpy()), f32_bits(r_o), err_msg=f"reward {label}")
    np.testing.assert_array_equal(gv.success.cpu().numpy(), s_o, err_msg=f"success {label}")
    np.testing.assert_array_equal(gv.done.cpu().numpy(), f_o if done is None else done, err_msg=f"is_final {label}")
    np.testing.assert_array_equal(gv.depth.cpu().numpy(), d_o if depth is None else depth, err_msg=f"depth {label}")


def _same_state(ov, gv, kind, n, label):
    d = _dim(kind, n)
    np.testing.assert_array_equal(gv.get_state("i64").cpu().numpy(), ov.get_state(d * d), err_msg=f"state {label}")
    np.testing.assert_array_equal(gv.observe().cpu().numpy().reshape(gv.batch, -1), ov.observe_dense(), err_msg=f"obs {label}")


def _same_packed(ov, gv, label):
    """observe_packed: word r of an env = the bits of row r of its dense observation."""
    r, c = gv.obs_shape_
    dense = ov.observe_dense().reshape(gv.batch, r, c).astype(np.uint64)
    want = (dense << np.arange(c, dtype=np.uint64)).sum(axis=2)
    got = gv.observe_packed().cpu().numpy().view({1: np.uint8, 4: np.uint32, 8: np.uint64}[gv.packed_word_bytes]).astype(np.uint64)
    np.testing.assert_array_equal(got[:, :r], want, err_msg=f"packed obs {label}")


def _step(ov, gv, kind, n, acts, dtype=None, label=""):
    want = ov.step(np.asarray(acts, dtype=np.int32))
    gv.step(_dev(acts, dtype))
    _same_outputs(gv, want, label)
    _same_state(ov, gv, kind, n, label)
    return want


def _pairs(kind, n, gs):
    """(gate, inverse) action pairs that leave the identity and return to it: both qubit parities, qubits in one group and in two."""
    def a(name, *q):
        return gs.index((name, tuple(q)))
    if kind == "clifford":  # groups of two qubits
        singles = [("H", "H"), ("S", "Sdg"), ("Sdg", "S"), ("SX", "SXdg"), ("SXdg", "SX")]
        pairs = [(a(x, q), a(y, q)) for x, y in singles for q in (0, n - 1)]
        doubles, edges = ["CX", "CZ", "SWAP"], [(0, 1), (1, 0), (1, 2), (2, 1), (n - 2, n - 1)]
    else:  # groups of four rows
        pairs, doubles, edges = [], ["CX", "SWAP"], [(4, 5), (5, 4), (3, 4), (4, 3), (n - 2, n - 1)]
    return pairs + [(a(g, *e), a(g, *e)) for g in doubles for e in edges]


def _lanes(kind, n, gs, B):
    pairs = _pairs(kind, n, gs)
    gate = np.array([pairs[e % len(pairs)][0] for e in range(B)])
    inverse = np.array([pairs[e % len(pairs)][1] for e in range(B)])
    return gate, inverse


# ---- success, done and depth in both directions, next to lanes that keep theirs --------------------------------------------------------
CHANGES = [(k, n, B, False, "int32") for k, n in SHAPES for B in BATCHES] + [
    ("clifford", 16, 130, True, "int32"), ("clifford", 4, 65, True, "int64"), ("linear_function", 12, 65, False, "int64"),
    ("linear_function", 12, 130, True, "int32")]


@pytest.mark.parametrize("kind,n,B,track,adt", CHANGES)
def test_success_done_and_depth_change_both_ways(kind, n, B, track, adt):
    """Three kinds of lane, interleaved (env e is of kind e % 3), from the identity at depth max_depth:
      0: gate, inverse, gate, nothing x 4, inverse     success 0 1 0 0 0 0 0 1
      1: nothing, gate, inverse, nothing x 5           success 1 0 1 1 1 1 1 1
      2: gate, nothing x 7                             success 0 throughout; done follows depth alone
    "nothing" is an out-of-range action: only depth and reward change.  Without a solution log max_depth is 3: depth goes 1 -> 0 in the
    third step, done with it, and both stay for five more steps.  With one (the FEAT instantiation; the log holds max_depth entries)
    max_depth is 8 and depth reaches 0 in the last step."""
    gs = line_gateset(kind, n)
    A, md = len(gs), 8 if track else 3
    ov, gv = make_pair(kind, n, gs, B, max_depth=md, **dict(PLAIN, track_solution=track))
    _from_identity(ov, gv, kind, n)
    gate, inverse = _lanes(kind, n, gs, B)
    cls = np.arange(B) % 3
    oor = np.full(B, A + 3)
    plan = {0: [gate, inverse, gate, oor, oor, oor, oor, inverse], 1: [oor, gate, inverse] + [oor] * 5, 2: [gate] + [oor] * 7}
    success = {0: [0, 1, 0, 0, 0, 0, 0, 1], 1: [1, 0, 1, 1, 1, 1, 1, 1], 2: [0] * 8}
    dtype = getattr(torch, adt)
    for t in range(8):
        acts = np.select([cls == 0, cls == 1, cls == 2], [plan[0][t], plan[1][t], plan[2][t]])
        state0 = gv.get_state("i64").cpu().numpy()
        before = (gv.success.cpu().numpy().copy(), gv.done.cpu().numpy().copy())
        _, s, f, d = _step(ov, gv, kind, n, acts, dtype, label=f"{kind}{n} B={B} t={t}")
        # the scenario is what the docstring says (the oracle's outputs)
        for c in range(3):
            assert (s[cls == c] == success[c][t]).all(), (t, c)
        assert (d == max(md - t - 1, 0)).all() and (f == (s | (d == 0))).all(), t
        nothing = acts == A + 3
        np.testing.assert_array_equal(gv.get_state("i64").cpu().numpy()[nothing], state0[nothing])
        if t > 0 and d[0] > 0:  # an out-of-range action while depth is above 0: success and done as they were
            np.testing.assert_array_equal(s[nothing], before[0][nothing])
            np.testing.assert_array_equal(f[nothing], before[1][nothing])
    if track:
        for e in (0, 1, 2, 64, B - 1):
            assert gv.solution(e) == ov.env(e).solution(), e


# ---- memory that a caller overwrote ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("B", BATCHES)
@pytest.mark.parametrize("kind,n", SHAPES)
def test_stale_done_success_and_depth(kind, n, B):
    """env.done, env.success and env.depth overwritten from torch before every step: all ones (bytes of 0xFF, then of 1), all zeros, and
    patterns that differ per lane.  After the step done and success are the oracle's for every env and depth is max(written - 1, 0).
    done depends on depth, so a step writes depths that end at 0 exactly when the oracle's depth does (max_depth 4: from the fourth step),
    and the oracle's depth is put back after the steps that wrote others."""
    gs = line_gateset(kind, n)
    A = len(gs)
    ov, gv = make_pair(kind, n, gs, B, max_depth=4, **PLAIN)
    _from_identity(ov, gv, kind, n)
    gate, inverse = _lanes(kind, n, gs, B)
    e = np.arange(B)
    oor = np.full(B, A + 3)
    written = [  # (done, success, depth)
        (np.full(B, 255), np.full(B, 255), 7 + e),
        (np.zeros(B), np.zeros(B), 1000 - e),
        (e & 1, (e >> 1) & 1, 2 + e % 5),
        (np.ones(B), np.ones(B), np.ones(B)),           # the oracle's depth goes 1 -> 0 here
        (np.zeros(B), np.zeros(B), np.zeros(B)),
        ((e >> 1) & 1, e & 1, e & 1),
    ]
    for t, (w_done, w_success, w_depth) in enumerate(written):
        # even envs: gate, inverse, gate, ...; odd envs: nothing, then gate, inverse, ... -- so both outputs take both values in every wave
        acts = np.where(e % 2 == 0, gate if t % 2 == 0 else inverse, oor if t == 0 else (gate if t % 2 == 1 else inverse))
        gv.done.copy_(_dev(w_done, torch.uint8))
        gv.success.copy_(_dev(w_success, torch.uint8))
        gv.depth.copy_(_dev(w_depth, torch.int32))
        want = ov.step(acts.astype(np.int32))
        gv.step(_dev(acts))
        expect_depth = np.maximum(w_depth.astype(np.int64) - 1, 0).astype(np.int32)
        assert ((expect_depth == 0) == (want[3] == 0)).all(), "the test's own depths"
        _same_outputs(gv, want, f"{kind}{n} B={B} t={t}", depth=expect_depth)
        _same_state(ov, gv, kind, n, f"{kind}{n} B={B} t={t}")
        assert len(np.unique(want[1])) == 2, "both values of success in the batch"
        gv.depth.copy_(_dev(want[3], torch.int32))


def test_neighbouring_lanes_change_different_outputs():
    """One step in which, lane by lane, depth alone changes, or success alone, or done alone, or nothing at all: partial execution masks on each
    of the three conditional stores.  Depth differs from env to env only after a reset_done or a caller's write; here it is written (odd envs 0, even envs 5), so done
    is checked as the oracle's success or depth == 0, the oracle's own rule (is_final)."""
    kind, n, B = "clifford", 16, 130
    gs = line_gateset(kind, n)
    A = len(gs)
    ov, gv = make_pair(kind, n, gs, B, max_depth=9, **PLAIN)
    _from_identity(ov, gv, kind, n)
    gate, inverse = _lanes(kind, n, gs, B)
    e = np.arange(B)
    oor = np.full(B, A + 3)
    # kinds of four lanes: solved / unsolved before the mixed steps
    _step(ov, gv, kind, n, np.where(e % 4 < 2, oor, gate), label="setup")
    for t, acts in enumerate([np.select([e % 4 == 0, e % 4 == 1, e % 4 == 2, e % 4 == 3], [oor, gate, oor, inverse]),
                              np.select([e % 4 == 0, e % 4 == 1, e % 4 == 2, e % 4 == 3], [gate, oor, inverse, oor]),
                              oor]):
        w_depth = np.where((e + (t == 2)) % 2 == 1, 0, 5).astype(np.int32)  # (the last step: an unsolved env's depth 4 -> 0, done alone changes)
        gv.depth.copy_(_dev(w_depth))
        want = ov.step(acts.astype(np.int32))
        gv.step(_dev(acts))
        expect_depth = np.maximum(w_depth - 1, 0)
        _same_outputs(gv, want, f"mixed t={t}", done=want[1] | (expect_depth == 0), depth=expect_depth)
        _same_state(ov, gv, kind, n, f"mixed t={t}")
        assert len(np.unique(want[1][:64])) == 2, "both values of success in a wave"


# ---- the other launch forms and instantiations -----------------------------------------------------------------------------------------
def test_graph_replay():
    """rollout_ring: the same launches from a cached graph; success and done flip between its steps and between its replays."""
    kind, n, B, T = "clifford", 16, 130, 3
    gs = line_gateset(kind, n)
    A = len(gs)
    ov, gv = make_pair(kind, n, gs, B, max_depth=7, **PLAIN)
    _from_identity(ov, gv, kind, n)
    gate, inverse = _lanes(kind, n, gs, B)
    e = np.arange(B)
    host = np.stack([np.where(e % 2 == 0, gate, A + 3), np.where(e % 2 == 0, inverse, gate), np.where(e % 2 == 0, A + 3, inverse)])
    acts = _dev(host)
    for rep in range(3):  # depth 7 -> 0 in the third replay's first step
        for t in range(T):
            want = ov.step(host[t].astype(np.int32))
        gv.rollout_ring(acts, T)
        _same_outputs(gv, want, f"replay {rep}")
        _same_state(ov, gv, kind, n, f"replay {rep}")
    assert (want[3] == 0).all() and want[1].all()


@pytest.mark.parametrize("kind,n,B", [("clifford", 16, 130), ("linear_function", 12, 65)])
def test_done_list_form_with_reset_done(kind, n, B):
    """LIST: a handle on which reset_done is in use.  After a reset_done the envs it reset are at full depth beside envs at depth 0."""
    gs = line_gateset(kind, n)
    A, diff = len(gs), 2
    ov, gv = make_pair(kind, n, gs, B, max_depth=3, difficulty=diff, **PLAIN)
    rng = np.random.default_rng(90 + n)
    _scramble(ov, gv, rng, diff, A)
    gate, inverse = _lanes(kind, n, gs, B)
    e, resets = np.arange(B), 0
    for t in range(12):
        acts = np.select([(e + t) % 3 == 0, (e + t) % 3 == 1, (e + t) % 3 == 2], [gate, inverse, np.full(B, A + 3)])
        _, _, fin, _ = _step(ov, gv, kind, n, acts, label=f"list {kind}{n} t={t}")
        done = fin.astype(bool)
        if done.any() and t % 2 == 1:  # every other step: some envs stay done, at depth 0, for a step
            gv.reset_done(700 + t)
            ov.reset_seeded(700 + t, mask=done)
            resets += int(done.sum())
            _same_state(ov, gv, kind, n, f"list after reset_done t={t}")
    assert resets > B


@pytest.mark.parametrize("n,B", [(16, 65), (8, 130)])
def test_tracked_dense_form(n, B):
    """DENSE: the resident dense observation follows every step."""
    kind = "clifford"
    gs = line_gateset(kind, n)
    A = len(gs)
    ov, gv = make_pair(kind, n, gs, B, max_depth=3, **PLAIN)
    _from_identity(ov, gv, kind, n)
    tracked = gv.track_dense()
    gate, inverse = _lanes(kind, n, gs, B)
    e = np.arange(B)
    for t in range(6):
        acts = np.select([(e + t) % 3 == 0, (e + t) % 3 == 1, (e + t) % 3 == 2], [gate, inverse, np.full(B, A + 3)])
        _step(ov, gv, kind, n, acts, label=f"dense {n}q t={t}")
        assert torch.equal(tracked, gv.observe()), t
        np.testing.assert_array_equal(tracked.cpu().numpy().reshape(B, -1), ov.observe_dense(), err_msg=f"tracked dense t={t}")


# ---- the two row groups: one group, two groups, equal qubits, by lane --------------------------------------------------------------------
def _group_gateset(kind, n):
    """Gates on qubits of one group, on qubits of two, and two-qubit gates on equal qubits, in turn -- so that neighbouring lanes differ."""
    per, doubles = (2, ["CX", "CZ", "SWAP"]) if kind == "clifford" else (4, ["CX", "SWAP"])
    gs = []
    for k in range(n // per):
        lo = per * k
        for g in doubles:
            gs.append((g, (lo, lo + 1)))                      # one group
            if lo + per < n:
                gs.append((g, (lo + per - 1, lo + per)))      # two groups
                gs.append((g, (lo + per, lo + per - 1)))
            gs.append((g, (lo + 1, lo)))
            gs.append((g, (lo + 1, lo + 1)))                  # equal qubits
        if kind == "clifford":
            gs += [("H", (lo,)), ("S", (lo + 1,))]
    return gs


@pytest.mark.parametrize("kind,n,B", [("clifford", 16, 130), ("clifford", 4, 65), ("linear_function", 12, 65), ("linear_function", 12, 130)])
def test_same_group_and_cross_group_gates_by_lane(kind, n, B):
    gs = _group_gateset(kind, n)
    A = len(gs)
    ov, gv = make_pair(kind, n, gs, B, max_depth=A + 8, **PLAIN)
    _scramble(ov, gv, np.random.default_rng(40 + n + B), 3 * n, A)
    e = np.arange(B)
    for t in range(min(A, 40)):
        _step(ov, gv, kind, n, (3 * t + e) % A, label=f"groups {kind}{n} t={t}")
        _same_packed(ov, gv, f"groups {kind}{n} t={t}")
