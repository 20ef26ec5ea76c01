"""`qg_beam_advance` (collector.beam_advance) on the device against tests/beambound_model.py bit for bit and, without the bound, against the
tensor-library lines of the beam search it replaces; `BatchedSynthesis.solve(..., beam_width=W, bound="stop")` against the search without
the bound, solution for solution; `bound="prune"` against the CPU model search driven by the same log-probabilities."""
import functools

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")

from beambound_model import advance, beam_search_bounded  # noqa: E402
from oracle import OracleEnv  # noqa: E402
from test_gpu_beam import Recorder, golden_case, oracle_kwargs, pauli_case  # noqa: E402

NINF = np.float32(-np.inf)
# sums of one of each are exact in f32 and repeat: equal returns, and r + 1 == best, are frequent
RET_IN = np.array([0.0, -0.0, -0.25, -0.5, -0.75], dtype=np.float32)
REWARD = np.array([0.0, -0.0, -0.25, 0.75, 1.0, 0.5], dtype=np.float32)
BEST = np.array([NINF, 0.0, 0.25, 0.5, 0.75, 1.0], dtype=np.float32)
MODES = (None, "stop", "prune")
PLANTS = 7


def plant(kind, sl, x, W):
    """One of the hand-made rows of tests/test_beambound_model.py written over the group whose slots are `sl`, at any width."""
    g = sl.start // W
    x["live"][sl], x["done"][sl], x["success"][sl] = 1, 0, 0
    x["ret_in"][sl], x["best"][g], x["found"][g] = 0.0, 0.25, 1
    x["parent"][sl] = np.arange(sl.start, sl.stop)
    if kind == 0:  # every slot solved with the same return: the lowest slot wins
        x["reward"][sl], x["success"][sl], x["done"][sl] = 0.75, 1, 1
    elif kind == 1:  # the results equal best: the winner stays
        x["reward"][sl], x["success"][sl], x["done"][sl], x["best"][g] = 0.75, 1, 1, 0.75
    elif kind == 2:  # r + 1 == best exactly, in every slot: all hopeless
        x["reward"][sl], x["best"][g] = -0.25, 0.75
    elif kind == 3:  # no winner yet: never bounded, whatever best holds
        x["reward"][sl], x["best"][g], x["found"][g] = -0.75, 1.0, 0
    elif kind == 4:  # ended without success
        x["reward"][sl], x["done"][sl] = -0.5, 1
    elif kind == 5:  # all dead; nothing of a dead slot is read
        x["live"][sl], x["success"][sl], x["done"][sl], x["reward"][sl] = 0, 1, 1, 1.0
        x["parent"][sl] = -1
    else:  # -0.0 in slot 0 against +0.0 behind it, all solved
        x["ret_in"][sl], x["reward"][sl], x["success"][sl], x["done"][sl], x["best"][g] = 0.0, 0.0, 1, 1, NINF
        x["ret_in"][sl.start], x["reward"][sl.start] = -0.0, -0.0


def make_inputs(rng, W, groups, first_plant):
    B = groups * W
    x = dict(parent=(np.arange(B) // W * W + rng.integers(0, W, size=B)).astype(np.int32), ret_in=rng.choice(RET_IN, size=B), reward=rng.choice(REWARD, size=B),
             success=(rng.random(B) < 0.3).astype(np.uint8), done=(rng.random(B) < 0.15).astype(np.uint8), live=(rng.random(B) < 0.75).astype(np.uint8),
             best=rng.choice(BEST, size=groups), bounded=rng.integers(0, 5, size=groups).astype(np.int32))
    x["done"] |= x["success"]  # as the envs do; the planted rows and the random ones below cover the other combinations
    odd = rng.random(B) < 0.05
    x["done"][odd] ^= 1
    far = rng.random(B) < 0.1  # a parent is a batch-wide index
    x["parent"][far] = rng.integers(0, B, size=int(far.sum()))
    x["parent"][x["live"] == 0] = rng.choice(np.array([-1, B, 2**31 - 1], dtype=np.int32), size=int((x["live"] == 0).sum()))  # not read
    x["found"] = ((x["best"] != NINF) ^ (rng.random(groups) < 0.1)).astype(np.uint8)
    for k in range(min(groups, PLANTS - first_plant)):
        plant(first_plant + k, slice(k * W, (k + 1) * W), x, W)
    return x


def on_device(x):
    return {k: torch.as_tensor(v, device="cuda") for k, v in x.items()}


def run_kernel(d, W, mode, bonus=1.0, skip=None, **out):
    """On copies of the in/out operands; returns what `advance` returns."""
    from qiskit_gym_amd.collector import beam_advance

    B = d["parent"].numel()
    live, best, found, bounded = d["live"].clone(), d["best"].clone(), d["found"].clone(), d["bounded"].clone()
    ret, win_src, group_live = beam_advance(d["parent"], d["ret_in"], d["reward"], d["success"], d["done"], live, best, found, W, B if skip is None else skip,
                                            bonus, mode, bounded=bounded, **out)
    torch.cuda.synchronize()
    return ret, live, best, found, win_src, group_live, bounded


def expect_equal(got, want, label):
    names = ("ret_out", "live", "best", "found", "win_src", "group_live", "bounded")
    for name, g, w in zip(names, got, want):
        g = g.cpu().numpy()
        if name in ("ret_out", "best"):
            np.testing.assert_array_equal(g.view(np.uint32), np.asarray(w, dtype=np.float32).view(np.uint32), err_msg=f"{name} bits {label}")
        else:
            np.testing.assert_array_equal(g.astype(np.int64), np.asarray(w).astype(np.int64), err_msg=f"{name} {label}")


def model(x, W, mode, bonus=1.0, skip=None):
    return advance(x["parent"], x["ret_in"], x["reward"], x["success"], x["done"], x["live"], x["best"], x["found"], W, len(x["parent"]) if skip is None else skip,
                   bonus, mode, x["bounded"])


@pytest.mark.parametrize("groups", [1, 3, 257])  # 257: the last workgroup is partly filled
@pytest.mark.parametrize("W", [1, 2, 16, 64])
def test_kernel_against_the_model_bit_for_bit(W, groups):
    rng = np.random.default_rng(1000 * W + groups)
    seen_bound = seen_tie = 0
    for first_plant in range(0, PLANTS, groups):  # few groups: one launch per batch of planted rows
        x = make_inputs(rng, W, groups, first_plant)
        d = on_device(x)
        none = model(x, W, None)
        for mode in MODES:
            want = model(x, W, mode)
            expect_equal(run_kernel(d, W, mode), want, f"mode {mode} plants from {first_plant}")
            expect_equal(run_kernel(d, W, mode, skip=-3), model(x, W, mode, skip=-3), f"mode {mode} skip -3")
            seen_bound += int((want[6] - x["bounded"]).sum())
            # bonus = +inf: the bound ends nothing
            expect_equal(run_kernel(d, W, mode, bonus=float("inf")), none, f"mode {mode} bonus inf")
            assert model(x, W, mode, bonus=np.inf)[1].tolist() == none[1].tolist()
        r, best = none[0].reshape(groups, W), x["best"]
        seen_tie += int(((r + np.float32(1.0) == best[:, None]) & (x["live"].reshape(groups, W) != 0)).sum())
    assert seen_bound > 0 and seen_tie > 0  # the inputs reach the bound, and r + bonus == best occurs


def test_the_launch_replayed_from_a_graph():
    from qiskit_gym_amd.collector import beam_advance

    W, groups = 16, 257
    B = groups * W
    rng = np.random.default_rng(5)
    x = make_inputs(rng, W, groups, 0)
    bufs = on_device(x)
    outs = dict(ret_out=torch.empty(B, device="cuda"), win_src=torch.empty(groups, dtype=torch.int32, device="cuda"),
                group_live=torch.empty(groups, dtype=torch.uint8, device="cuda"))
    graph = None
    for round_ in range(3):
        if round_:
            x = make_inputs(rng, W, groups, 0)
            for k, v in x.items():
                bufs[k].copy_(torch.as_tensor(v))
        for o in outs.values():
            o.zero_()
        if graph is None:
            torch.cuda.synchronize()
            graph = torch.cuda.CUDAGraph()
            with torch.cuda.graph(graph):
                beam_advance(bufs["parent"], bufs["ret_in"], bufs["reward"], bufs["success"], bufs["done"], bufs["live"], bufs["best"], bufs["found"], W, B, 1.0,
                             "stop", bounded=bufs["bounded"], **outs)
            for k, v in x.items():  # (capture runs nothing; the in/out operands are as they were, but make that plain)
                bufs[k].copy_(torch.as_tensor(v))
        graph.replay()
        torch.cuda.synchronize()
        got = (outs["ret_out"], bufs["live"], bufs["best"], bufs["found"], outs["win_src"], outs["group_live"], bufs["bounded"])
        expect_equal(got, model(x, W, "stop"), f"replay {round_}")
    del graph


def _winner(solved, ret):
    score = torch.where(solved, ret, torch.full(ret.shape, -float("inf"), device=ret.device))
    return score, score.argmax(dim=1)


@pytest.mark.parametrize("W,groups", [(1, 300), (4, 1024), (16, 257), (64, 33)])
def test_mode_none_against_the_torch_lines_it_replaces(W, groups):
    """The search runs the kernel in every mode now: the torch lines below, with this file's `_winner`, are the only restatement left of
    what `bound=None` once ran per step."""
    M, B = groups, groups * W
    rng = np.random.default_rng(W + groups)
    x = make_inputs(rng, W, groups, 0)
    x["parent"] = np.where(x["live"] != 0, x["parent"], np.arange(B)).astype(np.int32)  # the torch gather reads every slot's parent
    x["found"] = (x["best"] != NINF).astype(np.uint8)
    d = on_device(x)
    parent, ret, live, best, found = d["parent"], d["ret_in"], d["live"], d["best"], d["found"].bool()
    reward, success, done = d["reward"], d["success"], d["done"]
    group = torch.arange(M, dtype=torch.int32, device="cuda")
    nowhere = torch.full((M,), B, dtype=torch.int32, device="cuda")
    got = run_kernel(d, W, None)
    # ---- the lines of BatchedSynthesis._beam_search between `oth.step(act)` and the merge, as they stood for bound=None
    live_in = live
    ret = ret[parent.long()] + reward
    solved = (live.bool() & success.bool()).view(M, W)
    live = live & (1 - done)
    score, j = _winner(solved, ret.view(M, W))
    val = score.gather(1, j.view(M, 1)).view(M)
    better = val > best
    src = torch.where(better, group * W + j.to(torch.int32), nowhere)
    best = torch.where(better, val, best)
    found |= better
    # ----
    torch.cuda.synchronize()
    on = live_in.bool()
    assert torch.equal(got[0].view(torch.int32)[on], ret.view(torch.int32)[on])  # bit for bit, on the live slots
    assert torch.equal(got[1], live) and torch.equal(got[2].view(torch.int32), best.view(torch.int32)) and torch.equal(got[3].bool(), found)
    assert torch.equal(got[4], src)
    assert torch.equal(got[5].long(), live.view(M, W).long().sum(dim=1)) and torch.equal(got[6], d["bounded"])
    assert int(better.sum()) > 0 and int((~better).sum()) > 0


# ---- the search -----------------------------------------------------------------------------------------------------------------------------
SOLVES = {  # policy, W, further arguments
    "clifford-W1": ("clifford_3q_custom", 1, {}), "clifford-W4": ("clifford_3q_custom", 4, {}),
    "linear-function-W1": ("lf_5_line", 1, {}), "linear-function-W4": ("lf_5_line", 4, {}),
    "permutation-W1": ("perm_square_3x3", 1, {}), "permutation-W4": ("perm_square_3x3", 4, {}),
    "clifford-W4-merge": ("clifford_3q_custom", 4, {"merge_duplicates": True}), "clifford-W4-fast": ("clifford_3q_custom", 4, {"fast": True}),
    "linear-function-W4-twists": ("lf_5_line", 4, {"twists": 2}),  # the line's mirror image: two (target, view) groups per target
    "linear-function-W4-twist-kernels": ("lf_5_line", 4, {"twists": 2, "twist_kernels": True}),
}


@functools.lru_cache(maxsize=None)
def both_searches(case):
    from qiskit_gym_amd.synthesis import BatchedSynthesis

    name, W, kw = SOLVES[case]
    gym, policy, states, _ = golden_case(name, 64, 4, 11)
    syn = BatchedSynthesis(gym, policy, seed=1)
    plain = syn.solve(states, beam_width=W, **kw)
    plain_stats = dict(syn.last_stats)
    stop = syn.solve(states, beam_width=W, bound="stop", **kw)
    return plain, plain_stats, stop, dict(syn.last_stats), int(gym.config["max_depth"])


@pytest.mark.parametrize("case", sorted(SOLVES))
def test_stop_returns_what_the_search_without_it_returns(case):
    plain, plain_stats, stop, stats, T = both_searches(case)
    print(case, plain_stats, stats)
    assert stop == plain
    assert stats["solved"] == plain_stats["solved"] >= 60 and stats["mean_gates"] == plain_stats["mean_gates"]
    assert stats["steps"] <= plain_stats["steps"] <= T
    assert stats["bound"] == "stop" and stats["bounded"] >= 0
    loose = ("bound", "bounded", "steps", "merged", "revisits")  # a search that ends sooner merges less
    assert {k: v for k, v in stats.items() if k not in loose} == {k: v for k, v in plain_stats.items() if k not in loose}
    assert set(stats) == set(plain_stats) | {"bound", "bounded"}
    assert "bound" not in plain_stats and "bounded" not in plain_stats
    assert stats.get("views") == SOLVES[case][2].get("twists") and stats.get("kernels", False) == ("fast" in case or "kernels" in case)


def test_stop_ends_a_search_before_max_depth():
    runs = [both_searches(case) for case in sorted(SOLVES)]
    assert any(stats["steps"] < T for _, _, _, stats, T in runs)
    assert any(stats["steps"] < plain_stats["steps"] and stats["bounded"] > 0 for _, plain_stats, _, stats, _ in runs)


@pytest.mark.parametrize("name", ["clifford_3q_custom", "lf_5_line"])
def test_prune_against_the_model_on_the_same_log_probabilities(name):
    from qiskit_gym_amd.synthesis import BatchedSynthesis

    W = 4
    gym, policy, states, _ = golden_case(name, 24, 4, 7)
    kind, n, gs = gym.env_kind, gym.config["num_qubits"], gym.config["gateset"]
    A, T = len(gs), gym.config["max_depth"]
    rec = Recorder(policy)
    syn = BatchedSynthesis(gym, rec, seed=1)
    sols = syn.solve(states, beam_width=W, bound="prune")
    stats = syn.last_stats
    assert set(stats) == {"beam_width", "targets", "steps", "solved", "mean_gates", "bound", "bounded"} and stats["bound"] == "prune"
    assert stats["steps"] == len(rec.logp) <= T
    okw = oracle_kwargs(gym)

    def fresh(m):
        env = OracleEnv(kind, n, gs, **okw)
        env.set_state(states[m])
        return env

    trace = {}
    want = beam_search_bounded([fresh(m) for m in range(len(states))], W, A, T, lambda t, envs: rec.logp[t], "prune", trace=trace)
    print(name, stats, "model steps", trace["steps"], "model bounded", int(trace["bounded"].sum()))
    assert sols == want
    assert stats["bounded"] == int(trace["bounded"].sum()) > 0
    assert sols[-1] == [] and stats["solved"] == sum(s is not None for s in sols) >= 20
    for m, sol in enumerate(sols):  # every solution, replayed on the oracle from its target, solves it with exactly those gates
        if sol is not None:
            env = fresh(m)
            for a in sol:
                assert not env.success()
                env.step(int(a))
            assert env.success() and env.solution() == sol


def test_solve_checks_the_bound_argument():
    import qiskit_gym_amd.envs as envs
    from qiskit_gym_amd.synthesis import BatchedSynthesis

    gym, policy, states, _ = golden_case("clifford_3q_custom", 8, 4, 3)
    syn = BatchedSynthesis(gym, policy, seed=1)
    before = syn.solve(states, beam_width=4)
    keys = set(syn.last_stats)
    assert keys == {"beam_width", "targets", "steps", "solved", "mean_gates"}
    with pytest.raises(ValueError, match="beam_width"):
        syn.solve(states, bound="stop")
    with pytest.raises(ValueError, match="bound"):
        syn.solve(states, beam_width=4, bound="halt")
    assert syn.solve(states, beam_width=4, bound="stop") == before and syn.last_stats["bound"] == "stop"
    assert syn.solve(states, beam_width=4) == before and set(syn.last_stats) == keys  # a bounded search in between changes nothing
    assert syn.solve(states, beam_width=4, bound=None) == before and set(syn.last_stats) == keys

    cfg = gym.config
    neg = envs.CliffordGym(cfg["num_qubits"], cfg["gateset"], depth_slope=cfg["depth_slope"], max_depth=cfg["max_depth"], metrics_weights={"n_gates": -0.0001})
    syn = BatchedSynthesis(neg, policy, seed=1)
    with pytest.raises(ValueError, match="cannot exceed 1"):
        syn.solve(states, beam_width=4, bound="stop")
    assert len(syn.solve(states, beam_width=4)) == len(states)  # the search without the bound takes any weights
    zero = envs.CliffordGym(cfg["num_qubits"], cfg["gateset"], depth_slope=cfg["depth_slope"], max_depth=cfg["max_depth"], metrics_weights={"n_gates": 0.0})
    assert len(BatchedSynthesis(zero, policy, seed=1).solve(states, beam_width=4, bound="prune")) == len(states)

    pgym, ppolicy, pstates, _ = pauli_case()
    with pytest.raises(ValueError, match="PauliGym"):
        BatchedSynthesis(pgym, ppolicy, seed=1).solve(pstates, beam_width=4, bound="stop")


def test_beam_advance_checks_its_operands():
    from qiskit_gym_amd import _lib
    from qiskit_gym_amd.collector import beam_advance

    def call(B=8, W=2, mode="stop", **kw):
        M = max(1, B // W)
        t = dict(parent=torch.zeros(B, dtype=torch.int32, device="cuda"), ret_in=torch.zeros(B, device="cuda"), reward=torch.zeros(B, device="cuda"),
                 success=torch.zeros(B, dtype=torch.uint8, device="cuda"), done=torch.zeros(B, dtype=torch.uint8, device="cuda"),
                 live=torch.ones(B, dtype=torch.uint8, device="cuda"), best=torch.zeros(M, device="cuda"), found=torch.zeros(M, dtype=torch.uint8, device="cuda"))
        out = {k: kw.pop(k) for k in ("ret_out", "win_src", "group_live", "bounded") if k in kw}
        t.update(kw)
        if out.get("ret_out") == "alias":
            out["ret_out"] = t["ret_in"]
        return beam_advance(t["parent"], t["ret_in"], t["reward"], t["success"], t["done"], t["live"], t["best"], t["found"], W, B, 1.0, mode, **out)

    ret, win_src, group_live = call()
    torch.cuda.synchronize()
    assert ret.tolist() == [0.0] * 8 and win_src.tolist() == [8] * 4 and group_live.tolist() == [2] * 4
    with pytest.raises(ValueError, match="parent"):
        call(parent=torch.zeros(8, dtype=torch.int64, device="cuda"))  # wrong dtype
    with pytest.raises(ValueError, match="reward"):
        call(reward=torch.zeros(8, dtype=torch.float64, device="cuda"))
    with pytest.raises(ValueError, match="best"):
        call(best=torch.zeros(8, device="cuda"))  # wrong length: one entry per group
    with pytest.raises(ValueError, match="done"):
        call(done=torch.zeros(7, dtype=torch.uint8, device="cuda"))
    with pytest.raises(ValueError, match="bounded"):
        call(bounded=torch.zeros(4, dtype=torch.int64, device="cuda"))
    with pytest.raises(ValueError, match="ret_in"):
        call(ret_in=torch.zeros(16, device="cuda")[::2])  # not contiguous
    with pytest.raises(ValueError, match="alias"):
        call(ret_out="alias")
    with pytest.raises(ValueError, match="groups"):
        call(B=9)
    with pytest.raises(ValueError, match="mode"):
        call(mode="halt")
    with pytest.raises(_lib.QGymError) as e:
        call(B=130, W=65)  # wider than a wave
    assert e.value.status == -3
    ret, win_src, group_live = call(B=64, W=64)  # the widest group
    torch.cuda.synchronize()
    assert group_live.tolist() == [64]
