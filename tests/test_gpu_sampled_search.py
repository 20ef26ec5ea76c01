"""The sampled and the greedy search of `BatchedSynthesis.solve` against the CPU model of tests/searchmodel.py, draw by draw, on the torch
forward and on the policy-layer kernels, alone and under symmetry views.

The model is driven with the device's own numbers.  Torch path: a recording module keeps the input and the f32 logits of every forward call,
a stand-in on `synthesis.sample_actions` the (seed, counter, actions) of every draw, a stand-in on `VecEnv.step` the actions the env was
handed.  Kernel path: the kernels leave no logits in memory, so stand-ins on `synthesis.mid_head_sample` / `mid_head_logp` call the real
function with the search's arguments and then `mid_head_logp` once more on the same operands for the rows of log-probabilities (the race
and the arg-max do not change under a per-row shift).  Every live draw is checked against the model's own f64 race (searchmodel.py says how
an unclear one is treated), the model's envs then take the device's actions, and at the end solutions and `last_stats` must be the model's.
And the switch of `fast=None` to the kernels at 4 096 envs."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")

from oracle import OracleEnv  # noqa: E402
from sampling_cases import entry_threshold  # noqa: E402
from searchmodel import MARKER, SearchModel, views_of  # noqa: E402
from test_gpu_beam import Recorder, clifford16_case, oracle_kwargs, pauli_case  # noqa: E402
from test_gpu_synthesis import make, replay, targets  # noqa: E402

UNCLEAR_CAP = 0.01  # of a case's live draws: the cap of test_gpu_sampling_edges.py
# The draws are the search's, the seed is the test's.  The 16-qubit policy is untrained: of its 20 targets one or two gates from solved, 8 searches
# of 5 steps find hardly any, and seed 2 is one whose draws solve three of them (the model alone, on a CPU forward of the same policy).
SEEDS = {"clifford-3q": 5, "linear-function-5q": 5, "permutation-9q": 5, "clifford-16q": 2, "pauli-3q": 5}


class InputRecorder(Recorder):
    """`Recorder`, keeping the input of every forward call and the f32 logits themselves as well."""

    def __init__(self, inner):
        super().__init__(inner)
        self.x, self.logits = [], []

    def forward(self, x):
        logits, value = self.inner(x)
        self.x.append(x.float().cpu().numpy())
        self.logits.append(logits.float().cpu().numpy())
        return logits, value


def golden(name, seed):
    """24 targets at difficulty 20 and the identity, for one of the reference's trained policies."""
    kind, cfg, gateset, syn = make(name)
    states = targets(kind, cfg, gateset, 24, 20, seed)
    states.append(OracleEnv(kind, cfg["num_qubits"], gateset, add_inverts=0, add_perms=0).get_state().tolist())  # solved on arrival
    return syn.env, syn._policy, states, None


CASES = {
    "clifford-3q": lambda: golden("clifford_3q_custom", 1),
    "linear-function-5q": lambda: golden("lf_5_line", 3),
    "permutation-9q": lambda: golden("perm_square_3x3", 4),
    "clifford-16q": clifford16_case,
    "pauli-3q": pauli_case,
}

CALLS = [  # case, solve's arguments
    ("clifford-3q", dict(num_searches=16)),
    ("clifford-3q", dict(deterministic=True)),
    ("clifford-3q", dict(num_searches=16, fast=True)),
    ("clifford-3q", dict(deterministic=True, fast=True)),
    ("linear-function-5q", dict(num_searches=5, twists=2)),  # 5 mod 2 != 0
    ("linear-function-5q", dict(deterministic=True, twists=2)),
    ("linear-function-5q", dict(num_searches=5, twists=2, twist_kernels=True)),
    ("linear-function-5q", dict(deterministic=True, twists=2, twist_kernels=True)),
    ("permutation-9q", dict(num_searches=12, twists=8)),  # wraps past V
    ("permutation-9q", dict(num_searches=3, twists=8)),  # S < V
    ("permutation-9q", dict(deterministic=True, twists=8)),
    ("permutation-9q", dict(num_searches=12, twists=8, twist_kernels=True)),
    ("clifford-16q", dict(num_searches=8)),
    ("pauli-3q", dict(num_searches=64, fast=False)),
    ("pauli-3q", dict(num_searches=64, fast=True)),
]


def call_id(call):
    case, kw = call
    return case + "-" + "-".join(f"{k}={v}" for k, v in kw.items())


def oracle_targets(gym, states, raw):
    kind, n, gs = gym.env_kind, gym.config["num_qubits"], gym.config["gateset"]
    out = []
    for m in range(len(states)):
        env = OracleEnv(kind, n, gs, **oracle_kwargs(gym))
        if raw is not None:
            env.pauli_reset_from(*raw[m])
        else:
            env.set_state(states[m])
        out.append(env)
    return out


def recorded_search(monkeypatch, gym, policy, states, seed, kw):
    """`solve(states, **kw)` with the stand-ins in place.  Returns (solutions, last_stats, per step: the f32 rows the search chose from,
    the actions chosen on the views (None where the path does not show them), the actions the env was handed; the inputs of the forward
    calls, or None on the kernels)."""
    from qiskit_gym_amd import synthesis
    from qiskit_gym_amd.vec import VecEnv

    on_kernels = bool(kw.get("fast") or kw.get("twist_kernels"))
    rows, chosen, counters, stepped = [], [], [], []
    real_step, real_draw, real_sample, real_logp = VecEnv.step, synthesis.sample_actions, synthesis.mid_head_sample, synthesis.mid_head_logp

    def step(self, actions, coins=None):
        stepped.append(actions.cpu().numpy().astype(np.int64))
        return real_step(self, actions, coins)

    def draw(logits, seed, counter, *a, **k):
        out = real_draw(logits, seed, counter, *a, **k)
        counters.append((seed, counter))
        chosen.append(out[0].cpu().numpy().astype(np.int64))
        return out

    def own_rows(h, packed_mid, mid_features, packed_head, num_actions):
        return real_logp(h, packed_mid, mid_features, packed_head, num_actions, want_rows=True)[0].cpu().numpy()  # outputs of its own

    def sample(h, packed_mid, mid_features, packed_head, num_actions, seed, counter, **k):
        out = real_sample(h, packed_mid, mid_features, packed_head, num_actions, seed, counter, **k)
        counters.append((seed, counter))
        chosen.append(out[0].cpu().numpy().astype(np.int64))  # before `untwist_actions` rewrites the buffer in place
        rows.append(own_rows(h, packed_mid, mid_features, packed_head, num_actions))
        return out

    def logp(h, packed_mid, mid_features, packed_head, num_actions, **k):
        out = real_logp(h, packed_mid, mid_features, packed_head, num_actions, **k)
        chosen.append(out[1].cpu().numpy().astype(np.int64))
        rows.append(own_rows(h, packed_mid, mid_features, packed_head, num_actions))
        return out

    rec = None if on_kernels else InputRecorder(policy)
    syn = synthesis.BatchedSynthesis(gym, policy if on_kernels else rec, seed=seed)
    with monkeypatch.context() as m:
        m.setattr(VecEnv, "step", step)
        m.setattr(synthesis, "sample_actions", draw)
        m.setattr(synthesis, "mid_head_sample", sample)
        m.setattr(synthesis, "mid_head_logp", logp)
        sols = syn.solve(states, **kw)
    stats = dict(syn.last_stats)
    assert stats["kernels"] is on_kernels
    steps = stats["steps"]
    if not on_kernels:
        rows = rec.logits
        if kw.get("deterministic"):
            chosen = [None] * steps  # `argmax` on the module's logits: the env's side shows the choice
    assert len(rows) == len(chosen) == len(stepped) == steps
    if not kw.get("deterministic"):
        assert counters == [(seed, t) for t in range(steps)]
    return sols, stats, rows, chosen, stepped, None if on_kernels else rec.x


@pytest.mark.parametrize("call", CALLS, ids=call_id)
def test_search_against_the_model_draw_by_draw(monkeypatch, call):
    case, kw = call
    gym, policy, states, raw = CASES[case]()
    sols, stats, rows, chosen, stepped, inputs = recorded_search(monkeypatch, gym, policy, states, SEEDS[case], kw)

    kind, n, gs = gym.env_kind, gym.config["num_qubits"], gym.config["gateset"]
    A, T, M = len(gs), gym.config["max_depth"], len(states)
    greedy, on_kernels = bool(kw.get("deterministic")), inputs is None
    views = None
    if "twists" in kw:
        views = views_of(OracleEnv(kind, n, gs, add_inverts=0, add_perms=1))[: kw["twists"]]
        assert stats["views"] == len(views) == kw["twists"]
    else:
        assert "views" not in stats
    S = (1 if views is None else len(views)) if greedy else max(1, kw["num_searches"])
    assert stats["targets"] == M and stats["searches"] == S
    # the kernels take the lowest index among equal maxima; `torch.argmax` promises no order
    model = SearchModel(oracle_targets(gym, states, raw), S, A, T, seed=SEEDS[case], greedy=greedy, views=views, threshold=entry_threshold("mid_small"),
                        lowest_on_ties=on_kernels)
    assert entry_threshold("sample_f32") == entry_threshold("mid_small") == entry_threshold("mid_big") == model.threshold
    for t in range(stats["steps"]):
        assert not model.ended, f"the search went on after step {t}"
        if inputs is not None:  # every env, the finished ones too: a parked env does not move
            np.testing.assert_array_equal(inputs[t], model.observations(), err_msg=f"the policy's input at step {t}")
        model.step(rows[t], chosen[t], stepped[t])
    assert model.ended, f"the search stopped after {stats['steps']} steps, the model goes on"
    want, want_stats = model.result()
    share = model.unclear / max(model.live_draws, 1)
    print(f"{call_id(call)}: {model.unclear} of {model.live_draws} live draws unclear ({share:.4%}); steps {stats['steps']} of {T}, every env "
          f"finished after {model.all_finished_at}; solved {stats['solved']} of {M}, searches solved {stats['searches_solved']:.4f}, "
          f"mean gates {stats['mean_gates']:.3f}")
    assert sols == want
    for key in ("steps", "solved", "mean_gates"):
        assert stats[key] == want_stats[key], key
    # the device's mean is one f32 division (or multiplication by 1 / B) of an exact count: within one f32 spacing of the quotient
    assert abs(stats["searches_solved"] - want_stats["searches_solved"]) <= np.spacing(np.float32(want_stats["searches_solved"]))
    assert share <= UNCLEAR_CAP and (greedy or model.live_draws > 0)
    assert stats["solved"] >= 2  # nothing is compared empty
    if raw is None:
        assert sols[-1] == []  # the identity: solved on arrival
        cfg = dict(num_qubits=n, depth_slope=gym.config["depth_slope"], max_depth=T)
        for state, sol in zip(states, sols):
            if sol is not None:
                assert replay(kind, cfg, gs, state, sol).success()
    if case == "clifford-16q":
        assert stats["steps"] == T == 5 and any(s is None for s in sols)  # T is no multiple of 8, and most searches fail
    if case == "pauli-3q":
        assert any(any(a >= MARKER for a in s) for s in sols if s is not None)  # a winner's log carries a rotation marker: the replay is checked
    if call in CALLS[:2]:  # the last env finishes between two looks at `finished`: `steps`, and the cut of the actions, are the rounded-up value
        k = model.all_finished_at
        assert k is not None and k % 8 != 0 and stats["steps"] == -(-k // 8) * 8 < T


def confirm(gym, states, sols, some):
    kind, gs = gym.env_kind, gym.config["gateset"]
    cfg = dict(num_qubits=gym.config["num_qubits"], depth_slope=gym.config["depth_slope"], max_depth=gym.config["max_depth"])
    checked = 0
    for m in some:
        if sols[m] is not None:
            env = replay(kind, cfg, gs, states[m], sols[m])
            assert env.success() and env.solution() == sols[m]
            checked += 1
    assert checked >= len(some) // 2


def test_fast_none_switches_to_the_kernels_at_4096_envs():
    """fast=None: the torch forward below 4 096 envs, the kernels from there on where they apply, the torch forward where they do not."""
    kind, cfg, gateset, syn = make("clifford_3q_custom")
    tg = targets(kind, cfg, gateset, 65, 20, 11)
    sols = syn.solve(tg, num_searches=63)  # 65 * 63 = 4 095
    assert syn.last_stats["kernels"] is False and syn.last_stats["searches"] == 63 and len(sols) == 65
    confirm(syn.env, tg, sols, range(0, 65, 13))
    sols = syn.solve(tg[:64], num_searches=64)  # 4 096
    assert syn.last_stats["kernels"] is True and len(sols) == 64
    confirm(syn.env, tg, sols, range(0, 64, 13))
    assert syn.solve(tg[:64], num_searches=64, fast=False) is not None and syn.last_stats["kernels"] is False  # and not against the caller's word
    kind, cfg, gateset, syn = make("lf_5_line")  # one-word layout: the kernels do not apply
    tg = targets(kind, cfg, gateset, 64, 20, 12)
    sols = syn.solve(tg, num_searches=64)
    assert syn.last_stats["kernels"] is False and len(sols) == 64
    confirm(syn.env, tg, sols, range(0, 64, 13))
