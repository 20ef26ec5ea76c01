"""tests/beammodel.py, the CPU restatement the GPU beam search is compared with, checked on its own: its selection against a brute-force
sort of hand-made cases (ties, masked actions, dead slots, fewer candidates than slots), and a whole model search on a 3-qubit oracle env
under a table policy, every returned solution replayed on a fresh oracle env."""
import numpy as np
import pytest

from beammodel import beam_search, select
from oracle import OracleEnv
from util import line_gateset

NINF, NAN = -np.inf, np.nan


def brute_force(logp, cum, live, W, A):
    """The rules of qg_beam_select spelled out one candidate at a time."""
    B = len(cum)
    parent, actions, cum_out, live_out = list(range(B)), [A] * B, [np.float32(NINF)] * B, [0] * B
    for g in range(B // W):
        cands = []
        for b in range(g * W, (g + 1) * W):
            if not live[b]:
                continue
            for a in range(A):
                s = np.float32(np.float32(cum[b]) + np.float32(logp[b][a]))
                if np.isnan(s) or s == np.float32(NINF):
                    continue
                cands.append((-float(s), b, a, s))
        cands.sort(key=lambda c: c[:3])
        for j, (_, b, a, s) in enumerate(cands[:W]):
            parent[g * W + j], actions[g * W + j], cum_out[g * W + j], live_out[g * W + j] = b, a, s, 1
    return parent, actions, cum_out, live_out


def agree(logp, cum, live, W, A):
    logp = np.asarray(logp, dtype=np.float32)
    got = select(logp, np.asarray(cum, dtype=np.float32), np.asarray(live), W, A)
    want = brute_force(logp, cum, live, W, A)
    assert got[0].tolist() == want[0] and got[1].tolist() == want[1]
    assert got[2].view(np.uint32).tolist() == [int(np.float32(x).view(np.uint32)) for x in want[2]]
    assert got[3].tolist() == want[3]
    return got


def test_selection_by_hand():
    # one group of two beams, three actions: scores 0.5+[-1,-2,-3], 0+[-1.5,-0.5,-9]
    p, a, c, l = agree([[-1, -2, -3], [-1.5, -0.5, -9]], [0.5, 0.0], [1, 1], 2, 3)
    assert p.tolist() == [0, 1] and a.tolist() == [0, 1] and c.tolist() == [-0.5, -0.5]  # a tie: slot 0 before slot 1
    # ties inside a slot go by action; a column past A (ld > A) is not read
    p, a, c, l = agree([[-1, -1, -1, 99], [-1, -1, -1, 99]], [0, 0], [1, 1], 2, 3)
    assert p.tolist() == [0, 0] and a.tolist() == [0, 1]
    # -0.0 and +0.0 tie (slot order decides) and keep their own bits
    p, a, c, l = agree([[-0.0, -5], [0.0, -5]], [-0.0, 0.0], [1, 1], 2, 2)
    assert p.tolist() == [0, 1] and c.view(np.uint32).tolist() == [0x80000000, 0]


def test_masked_actions_dead_slots_and_short_groups():
    # -inf and NaN entries do not exist; a dead slot contributes nothing whatever its row holds; a +inf score is an ordinary (best) one
    logp = [[NINF, -1, NAN], [5, 5, 5], [-2, np.inf, NINF], [NAN, NAN, NAN]]
    p, a, c, l = agree(logp, [0, 0, 0, 0], [1, 0, 1, 1], 4, 3)
    assert p.tolist() == [2, 0, 2, 3] and a.tolist() == [1, 1, 0, 3] and l.tolist() == [1, 1, 1, 0]
    assert c.tolist()[:3] == [np.inf, -1, -2] and c[3] == NINF
    # a cum of -inf or NaN removes the slot's candidates; a group without candidates is all filler; groups are independent
    logp = [[-1, -2], [-1, -2], [-3, -4], [-1, -2]]
    p, a, c, l = agree(logp, [NINF, NAN, 0, 7], [1, 1, 0, 1], 2, 2)
    assert p.tolist() == [0, 1, 3, 3] and a.tolist() == [2, 2, 0, 1] and l.tolist() == [0, 0, 1, 1]
    # width 1 is the greedy choice, lowest action among equals
    p, a, c, l = agree([[-3, -1, -1]], [0], [1], 1, 3)
    assert a.tolist() == [1]


@pytest.mark.parametrize("W,A", [(1, 3), (2, 5), (4, 3), (8, 7)])
def test_selection_against_the_brute_force_on_quantised_scores(W, A):
    rng = np.random.default_rng(W * 100 + A)
    for _ in range(20):
        B = W * int(rng.integers(1, 5))
        logp = rng.choice(np.array([-0.5, -1.0, -1.5, NINF, NAN, 0.0, -0.0], dtype=np.float32), size=(B, A + 2), p=[0.3, 0.25, 0.2, 0.1, 0.05, 0.05, 0.05])
        cum = rng.choice(np.array([0.0, -0.5, -1.0, NINF], dtype=np.float32), size=B, p=[0.4, 0.3, 0.25, 0.05])
        live = rng.random(B) < 0.7
        agree(logp, cum, live, W, A)


def _make(kind, n, gs, max_depth, difficulty=1):
    return OracleEnv(kind, n, gs, add_inverts=0, add_perms=0, track_solution=1, difficulty=difficulty, depth_slope=2, max_depth=max_depth)


def test_model_search_on_a_three_qubit_env_returns_solutions_that_replay():
    n, max_depth = 3, 6
    gs = line_gateset("clifford", n)
    A = len(gs)
    rng = np.random.default_rng(3)
    table = np.log(rng.dirichlet(np.ones(A), size=64)).astype(np.float32)  # a table policy: the observation's weight picks the row

    def logp_of(t, envs):
        out = np.zeros((len(envs), A), dtype=np.float32)
        for b, env in enumerate(envs):
            if env is not None:
                out[b] = table[int(np.asarray(env.dense_obs()).sum()) % 64]
        return out

    targets, states = [], []
    for k in range(12):
        env = _make("clifford", n, gs, max_depth, difficulty=1 + k % 3)
        if k:  # target 0 is the identity: solved on arrival
            env.reset_with(rng.integers(0, A, size=1 + k % 3))
        state = env.get_state().tolist()
        env = _make("clifford", n, gs, max_depth)
        env.set_state(state)
        targets.append(env)
        states.append(state)
    W = 32  # >= A: after one step every one-gate continuation is in the beam, so every one-gate target is solved
    sols = beam_search(targets, W, A, max_depth, logp_of)
    assert sols[0] == []
    for k, (state, sol) in enumerate(zip(states, sols)):
        if k % 3 == 0:
            assert sol is not None, k
        if sol is None:
            continue
        env = _make("clifford", n, gs, max_depth)
        env.set_state(state)
        for a in sol:
            assert not env.success()
            env.step(int(a))
        assert env.success() and env.solution() == sol and len(sol) <= max_depth
    assert sum(s is not None for s in sols) >= 5
    assert beam_search(targets, W, A, max_depth, logp_of) == sols  # the targets were cloned, not stepped; no randomness
    assert beam_search(targets, 1, A, max_depth, logp_of)[0] == []  # width 1 follows the table's best action only
