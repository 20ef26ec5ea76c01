"""The definition of a symmetry view (include/qgym.h, "Twists, batched"), proved on the CPU oracle before any kernel relies on it.

Twist t of a CliffordEnv / LinearFunctionEnv / PermutationEnv is (obs_perms[t], act_perms[t]) (symmetry.rs:205-295).  With
    view_t(obs)[i] = obs[obs_perms[t][i]]                 (a gather)
    real action of an action a chosen on the view = act_perms[t][a]      (pauli.rs:596)
the defining property is equivariance: for every state s, twist t and action a
    view_t(observe(step(s, act_perms[t][a]))) == observe(step(set_state(view_t(observe(s))), a)).
Checked here for the three kinds, every twist and every action, on random reachable states of graphs with non-involutive automorphisms
(ring6: the rotations; star5: the 3- and 4-cycles of its leaves; grid3x3: the quarter turns) -- for an involution gather and scatter are the
same map and prove nothing.  The scatter form, view[obs_perms[t][i]] = obs[i], is shown to FAIL on ring6: the gather form is the definition."""
import numpy as np
import pytest

from oracle import OracleEnv
from qiskit_gym_amd.envs.gateset import gateset_from_coupling_map
from test_oracle_symmetry import GRAPHS
from util import ALLOWED

KINDS = ["clifford", "linear_function", "permutation"]
N_STATES = 3


def gather(obs, perm):
    return obs[perm]


def scatter(obs, perm):
    out = np.empty_like(obs)
    out[perm] = obs
    return out


def wire_state(kind, n, dense):
    """Env::set_state's Vec<i64> of a flat dense observation (clifford.rs:299-304: the entries; permutation.rs:168-173: the set column of
    each row)."""
    if kind == "permutation":
        rows = dense.reshape(n, n)
        assert (rows.sum(axis=1) == 1).all(), "a view of a permutation matrix is a permutation matrix"
        return rows.argmax(axis=1).astype(np.int64)
    return dense.astype(np.int64)


def violations(kind, graph, view):
    """(state, twist, action) triples at which `view` is not equivariant, and the number tried."""
    n, edges = GRAPHS[graph]
    gs = gateset_from_coupling_map(edges, None, ALLOWED[kind])[1]
    env = OracleEnv(kind, n, gs, add_perms=1, add_inverts=0, max_depth=64, difficulty=3 * n)
    obs_perms, act_perms = (np.asarray(x, dtype=np.int64) for x in env.twists())
    A = env.num_actions()
    rng = np.random.default_rng(sum(map(ord, kind + graph)))
    bad, tried = [], 0
    real, viewed = env.clone(), env.clone()
    for s in range(N_STATES):
        env.reset_with(rng.integers(0, A, size=3 * n))  # a random reachable state
        obs = env.dense_obs().reshape(-1)
        start = wire_state(kind, n, obs)
        for t in range(len(obs_perms)):
            seen = wire_state(kind, n, view(obs, obs_perms[t]))
            for a in range(A):
                real.set_state(start)
                real.step(int(act_perms[t][a]))
                viewed.set_state(seen)
                viewed.step(a)
                tried += 1
                if not np.array_equal(view(real.dense_obs().reshape(-1), obs_perms[t]), viewed.dense_obs().reshape(-1)):
                    bad.append((s, t, a))
    return bad, tried


def non_involutions(graph, kind):
    n, edges = GRAPHS[graph]
    gs = gateset_from_coupling_map(edges, None, ALLOWED[kind])[1]
    obs_perms = np.asarray(OracleEnv(kind, n, gs, add_perms=1).twists()[0])
    return sum(1 for p in obs_perms if not np.array_equal(p[p], np.arange(p.size)))


@pytest.mark.parametrize("graph", ["ring6", "star5", "grid3x3", "line5"])
@pytest.mark.parametrize("kind", KINDS)
def test_gather_view_is_equivariant(kind, graph):
    bad, tried = violations(kind, graph, gather)
    assert tried > 0 and bad == [], f"{len(bad)} of {tried} (state, twist, action) triples break equivariance, first {bad[:5]}"


@pytest.mark.parametrize("kind", KINDS)
def test_the_graphs_have_non_involutive_twists(kind):
    assert non_involutions("ring6", kind) == 4  # the rotations by 1, 2, 4 and 5 places (by 3 and the six reflections are involutions)
    assert non_involutions("star5", kind) == 24 - 10  # S4 has the identity and 9 involutions
    assert non_involutions("grid3x3", kind) == 2  # the quarter turns
    assert non_involutions("line5", kind) == 0


@pytest.mark.parametrize("kind", KINDS)
def test_scatter_view_is_not_equivariant(kind):
    """The other direction is a different map wherever a twist is not an involution, and there it fails: the header records the gather."""
    bad, tried = violations(kind, "ring6", scatter)
    assert bad, "the scatter form holds as well: the two forms would not be told apart by this graph"
    n, edges = GRAPHS["ring6"]
    gs = gateset_from_coupling_map(edges, None, ALLOWED[kind])[1]
    obs_perms = np.asarray(OracleEnv(kind, n, gs, add_perms=1).twists()[0])
    involution = [bool(np.array_equal(p[p], np.arange(p.size))) for p in obs_perms]
    assert all(not involution[t] for _, t, _ in bad), "the scatter form may only fail at a non-involutive twist"
