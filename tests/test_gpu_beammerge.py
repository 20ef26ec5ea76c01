"""Merging of duplicate and revisited states on the device: `qg_beam_merge` (collector.beam_merge) against the numpy restatement of its rules
bit for bit, over three successive calls on one history per case; and `BatchedSynthesis.solve(..., beam_width=W, merge_duplicates=True)`
against the CPU model search of tests/beammerge_model.py driven by the same log-probabilities, every returned solution replayed on the
oracle."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")

from beammerge_model import beam_search_merged, merge, state_key  # noqa: E402
from beammodel import beam_search  # noqa: E402
from oracle import OracleEnv  # noqa: E402
from test_gpu_beam import Recorder, clifford16_case, golden_case, oracle_kwargs, pauli_case  # noqa: E402
from test_gpu_synthesis import replay  # noqa: E402

NINF, NAN = np.float32(-np.inf), np.float32(np.nan)
CUMS = np.array([0.0, -0.0, -0.5, -1.0, -3.0, NINF, NAN], dtype=np.float32)  # few values: ties are frequent; the last two have no order word
NP_DT = {1: np.uint8, 4: np.uint32, 8: np.uint64}
CALLS = 3


def make_calls(rng, W, n, wb, groups):
    """Three calls' inputs.  Every slot's row comes from its group's pool of about W / 2 distinct rows, the same pool in every call: duplicates
    within a call and hits on the history of the calls before; about a quarter of the slots is dead."""
    B = groups * W
    P = max(2, W // 2)
    hi = 1 << (8 * wb)
    pool = rng.integers(0, hi, size=(groups, P, n), dtype=np.uint64, endpoint=False).astype(NP_DT[wb])
    pool[:, :, 0] = np.arange(P, dtype=NP_DT[wb])  # (P <= 32) distinct rows within a pool, whatever the draw
    if n > 1:
        pool[:, 0, 1:] = 0  # zero words are in the case
    calls = []
    for _ in range(CALLS):
        pick = rng.integers(0, P, size=(groups, W))
        words = pool[np.arange(groups)[:, None], pick].reshape(B, n)
        cum = rng.choice(CUMS, size=B, p=[0.2, 0.15, 0.2, 0.2, 0.15, 0.05, 0.05])
        live = (rng.random(B) < 0.75).astype(np.uint8)
        calls.append((np.ascontiguousarray(words), cum, live))
    return calls


def to_dev(words, cum, live):
    wb = words.dtype.itemsize
    return (torch.as_tensor(words.view({1: np.uint8, 4: np.int32, 8: np.int64}[wb]), device="cuda"), torch.as_tensor(cum, device="cuda"),
            torch.as_tensor(live, device="cuda"))


CASES = [  # W, words_per_env, word_bytes, groups, seen_cap (None: 3 * W, never full)
    (1, 1, 8, 3, None), (8, 6, 4, 5, None), (16, 9, 1, 4, None), (33, 32, 4, 70, None), (64, 64, 8, 2, None), (64, 256, 1, 2, None),
    (8, 6, 4, 5, 3),  # a pool of 4 rows per group and room for 3 keys: the history saturates
    (8, 64, 4, 5, None), (9, 57, 4, 5, None),  # 512 and 513 words per group: the last shape of one wave, the first of four (test_search_dispatch.py)
]


@pytest.mark.parametrize("W,n,wb,groups,cap", CASES, ids=[f"W{c[0]}-n{c[1]}-b{c[2]}-G{c[3]}" + (f"-cap{c[4]}" if c[4] else "") for c in CASES])
def test_kernel_against_the_model_bit_for_bit(W, n, wb, groups, cap):
    from qiskit_gym_amd.collector import beam_merge, beam_seen

    rng = np.random.default_rng(W * 1000 + n * 10 + wb + groups)
    calls = make_calls(rng, W, n, wb, groups)
    full = cap is None
    cap = CALLS * W if full else cap
    B = groups * W

    # the model first, and what the case has to contain
    seen_m = [[] for _ in range(groups)]
    want, total = [], np.zeros((groups, 2), dtype=np.uint32)
    for c, (words, cum, live) in enumerate(calls):
        live_out, keys, dropped = merge(words, cum, live, W, seen_m, cap)
        total += dropped
        want.append((live_out, keys, total.copy()))
        assert c == 0 or dropped[:, 0].sum() >= 1, "no revisit in a later call"
        assert dropped[:, 0].sum() + dropped[:, 1].sum() + live_out.sum() <= live.sum()
    assert sum(w[0].sum() for w in want) >= 1 and (W == 1 or total[:, 1].sum() >= 1)
    if full:
        assert max(len(h) for h in seen_m) < cap
    else:  # a group was offered more keys than its history holds
        offered = [len({int(k) for w in want for k, keep in zip(w[1][g * W:(g + 1) * W], w[0][g * W:(g + 1) * W]) if keep}) for g in range(groups)]
        assert max(offered) > cap and max(len(h) for h in seen_m) == cap

    seen = beam_seen(groups, cap, "cuda")
    dropped = torch.zeros((groups, 2), dtype=torch.int32, device="cuda")
    keys = torch.empty(B, dtype=torch.int64, device="cuda")
    for c, call in enumerate(calls):
        words_d, cum_d, live_d = to_dev(*call)
        live_out = beam_merge(words_d, cum_d, live_d, W, seen, cap, keys=keys, dropped=dropped)
        torch.cuda.synchronize()
        np.testing.assert_array_equal(keys.cpu().numpy().view(np.uint64), want[c][1], err_msg=f"keys, call {c}")
        np.testing.assert_array_equal(live_out.cpu().numpy(), want[c][0], err_msg=f"live_out, call {c}")
        np.testing.assert_array_equal(dropped.cpu().numpy().view(np.uint32), want[c][2], err_msg=f"dropped, call {c}")
        assert live_out.data_ptr() != live_d.data_ptr()

    # without a history, and without the optional outputs: the last call merged within itself
    words, cum, live = calls[-1]
    live_out = beam_merge(*to_dev(words, cum, live), W)
    torch.cuda.synchronize()
    np.testing.assert_array_equal(live_out.cpu().numpy(), merge(words, cum, live, W)[0], err_msg="no history")


@pytest.mark.parametrize("cap", [512, 513])
def test_a_long_history_with_small_words(cap):
    """W 8, 6 words per env -- a group's 48 words would go to one wave -- with room for 512 keys (one wave: the last capacity that takes it)
    and for 513 (four waves, because of the history alone).  100 calls of mostly new rows: the history grows past 512 keys where there is
    room, so the threads' shares of it are dozens of keys each and a revisited key lies anywhere in it, and saturates at 512 where not."""
    from qiskit_gym_amd.collector import beam_merge, beam_seen

    W, n, groups, calls = 8, 6, 3, 100
    B = groups * W
    rng = np.random.default_rng(cap)
    seen_m, total = [[] for _ in range(groups)], np.zeros((groups, 2), dtype=np.uint32)
    seen = beam_seen(groups, cap, "cuda")
    dropped = torch.zeros((groups, 2), dtype=torch.int32, device="cuda")
    keys = torch.empty(B, dtype=torch.int64, device="cuda")
    rows = rng.integers(0, 1 << 32, size=(calls, B, n), dtype=np.uint64).astype(np.uint32)
    rows[:, :, 0] = np.arange(calls * B, dtype=np.uint32).reshape(calls, B)  # no two rows alike, whatever the draw
    revisits = late = 0
    for c in range(calls):
        words = rows[c].copy()
        for slot in np.nonzero(rng.random(B) < 0.12)[0]:  # a row its group has met: in an earlier call, anywhere in the history, or in this one
            back = int(rng.integers(0, c + 1))
            words[slot] = rows[back, slot // W * W + int(rng.integers(0, W))] if back < c else words[slot // W * W]
        cum = rng.choice(CUMS, size=B, p=[0.2, 0.15, 0.2, 0.2, 0.15, 0.05, 0.05])
        live = (rng.random(B) < 0.9).astype(np.uint8)
        held = [len(h) for h in seen_m]
        live_want, keys_want, d = merge(words, cum, live, W, seen_m, cap)
        total += d
        revisits += int(d[:, 0].sum())
        late += int(d[:, 0].sum()) if min(held) > 448 else 0  # revisits found in a history of hundreds of keys
        live_out = beam_merge(*to_dev(words, cum, live), W, seen, cap, keys=keys, dropped=dropped)
        torch.cuda.synchronize()
        np.testing.assert_array_equal(keys.cpu().numpy().view(np.uint64), keys_want, err_msg=f"keys, call {c}")
        np.testing.assert_array_equal(live_out.cpu().numpy(), live_want, err_msg=f"live_out, call {c}")
        np.testing.assert_array_equal(dropped.cpu().numpy().view(np.uint32), total, err_msg=f"dropped, call {c}")
    got = seen.cpu().numpy().view(np.uint64).reshape(groups, cap + 1)
    for g in range(groups):  # the history itself: the number of keys held, then the keys in the order they came
        assert got[g, 0] == len(seen_m[g]) and got[g, 1 : 1 + len(seen_m[g])].tolist() == seen_m[g], g
    assert revisits >= 20 and late >= 1 and total[:, 1].sum() >= 1
    assert [len(h) for h in seen_m] == [cap] * groups if cap == 512 else min(len(h) for h in seen_m) > 512


def test_the_launch_replayed_from_a_graph_with_the_memset_inside():
    """Clearing the history and two merges on it, captured once and replayed on new contents of the same buffers, give the eager result."""
    from qiskit_gym_amd.collector import beam_merge, beam_seen

    W, n, wb, groups = 16, 9, 4, 33
    B, cap = groups * W, 2 * W
    rng = np.random.default_rng(7)
    seen = beam_seen(groups, cap, "cuda")
    bufs = [dict(words=torch.empty((B, n), dtype=torch.int32, device="cuda"), cum=torch.empty(B, dtype=torch.float32, device="cuda"),
                 live=torch.empty(B, dtype=torch.uint8, device="cuda"), live_out=torch.empty(B, dtype=torch.uint8, device="cuda"),
                 keys=torch.empty(B, dtype=torch.int64, device="cuda")) for _ in range(2)]
    dropped = torch.empty((groups, 2), dtype=torch.int32, device="cuda")

    def launch():
        seen.zero_()  # a memset on the stream
        dropped.zero_()
        for b in bufs:
            beam_merge(b["words"], b["cum"], b["live"], W, seen, cap, keys=b["keys"], dropped=dropped, live_out=b["live_out"])

    graph = None
    for round_ in range(2):
        calls = make_calls(rng, W, n, wb, groups)[:2]
        for b, call in zip(bufs, calls):
            for name, t in zip(("words", "cum", "live"), to_dev(*call)):
                b[name].copy_(t)
        seen_m, total, want = [[] for _ in range(groups)], np.zeros((groups, 2), dtype=np.uint32), []
        for words, cum, live in calls:
            live_out, keys, d = merge(words, cum, live, W, seen_m, cap)
            total += d
            want.append((live_out, keys))
        assert total[:, 0].sum() >= 1 and total[:, 1].sum() >= 1
        if graph is None:
            torch.cuda.synchronize()
            graph = torch.cuda.CUDAGraph()
            with torch.cuda.graph(graph):
                launch()
        for how, run in (("replay", graph.replay), ("eager", launch)):
            for b in bufs:
                b["live_out"].fill_(7)
                b["keys"].zero_()
            run()
            torch.cuda.synchronize()
            for b, (live_out, keys) in zip(bufs, want):
                np.testing.assert_array_equal(b["live_out"].cpu().numpy(), live_out, err_msg=f"{how} {round_}")
                np.testing.assert_array_equal(b["keys"].cpu().numpy().view(np.uint64), keys, err_msg=f"{how} {round_}")
            np.testing.assert_array_equal(dropped.cpu().numpy().view(np.uint32), total, err_msg=f"{how} {round_}")
    del graph


def test_beam_merge_checks_its_arguments():
    from qiskit_gym_amd import _lib
    from qiskit_gym_amd.collector import beam_merge, beam_seen
    from qiskit_gym_amd.vec import _stream_ptr

    L = _lib.load()
    assert L.qg_beam_seen_bytes(0, 5) == 0 and L.qg_beam_seen_bytes(3, 5) >= 3 * 5 * 8

    def call(B, n, W, dtype=torch.int32, **kw):
        return beam_merge(torch.zeros((B, n), dtype=dtype, device="cuda"), torch.zeros(B, device="cuda"), torch.ones(B, dtype=torch.uint8, device="cuda"), W, **kw)

    with pytest.raises(_lib.QGymError) as e:
        call(130, 4, 65)  # wider than a wave
    assert e.value.status == -3
    with pytest.raises(_lib.QGymError) as e:
        call(2, 257, 2, torch.int64)  # 2056 bytes per env
    assert e.value.status == -3
    with pytest.raises(ValueError):
        call(9, 4, 2)  # not whole groups
    with pytest.raises(ValueError):
        call(4, 4, 2, torch.int16)  # no such word size
    with pytest.raises(ValueError):
        call(4, 4, 2, seen=beam_seen(2, 5, "cuda"), seen_cap=6)  # the history was made for another capacity
    live = torch.ones(4, dtype=torch.uint8, device="cuda")
    with pytest.raises(_lib.QGymError) as e:  # the output aliasing its input
        beam_merge(torch.zeros((4, 4), dtype=torch.int32, device="cuda"), torch.zeros(4, device="cuda"), live, 2, live_out=live)
    assert e.value.status == -1

    # the C entry point itself: every refusal comes before a launch, so the pointers that are passed are never read
    words, cum, out = torch.zeros((4, 4), dtype=torch.int32, device="cuda"), torch.zeros(4, device="cuda"), torch.zeros(4, dtype=torch.uint8, device="cuda")
    seen = beam_seen(2, 5, "cuda")
    good = dict(words=words.data_ptr(), wb=4, n=4, groups=2, W=2, cum=cum.data_ptr(), live=live.data_ptr(), seen=None, cap=0, out=out.data_ptr())

    def raw(**kw):
        a = dict(good, **kw)
        return L.qg_beam_merge(a["words"], a["wb"], a["n"], a["groups"], a["W"], a["cum"], a["live"], a["seen"], a["cap"], a["out"], None, None, _stream_ptr())

    for bad in (dict(words=None), dict(cum=None), dict(live=None), dict(out=None), dict(wb=2), dict(wb=0), dict(n=0), dict(W=0), dict(out=live.data_ptr()),
                dict(seen=seen.data_ptr(), cap=0), dict(words=words.data_ptr() + 2)):
        assert raw(**bad) == -1, bad
        assert L.qg_last_error()
    assert raw(W=65) == -3 and raw(wb=8, n=257) == -3
    assert raw(groups=0) == 0 and raw() == 0 and raw(seen=seen.data_ptr(), cap=5) == 0

    # the largest supported group: 64 slots of 2048 bytes, all different, all kept
    W, n = 64, 256
    rows = torch.arange(W * n, dtype=torch.int64, device="cuda").view(W, n)
    keys = torch.empty(W, dtype=torch.int64, device="cuda")
    kept = beam_merge(rows, torch.zeros(W, device="cuda"), torch.ones(W, dtype=torch.uint8, device="cuda"), W, keys=keys)
    torch.cuda.synchronize()
    assert kept.cpu().numpy().all()
    got = keys.cpu().numpy().view(np.uint64)
    assert int(got[0]) == state_key(rows[0].cpu().numpy()) and int(got[-1]) == state_key(rows[-1].cpu().numpy()) and len(set(got.tolist())) == W


# ---- the search -----------------------------------------------------------------------------------------------------------------------------
SEARCHES = {
    "clifford-3q-W8": (lambda: golden_case("clifford_3q_custom", 24, 20, 1), 8),
    "clifford-16q-W32": (clifford16_case, 32),
    "linear-function-5q-W4": (lambda: golden_case("lf_5_line", 24, 20, 3), 4),
    "permutation-9q-W16": (lambda: golden_case("perm_square_3x3", 24, 20, 4), 16),
}


@pytest.mark.parametrize("case", sorted(SEARCHES))
def test_merged_search_against_the_model_on_the_same_log_probabilities(case):
    from qiskit_gym_amd.synthesis import BatchedSynthesis

    build, W = SEARCHES[case]
    gym, policy, states, _ = build()
    kind, n, gs = gym.env_kind, gym.config["num_qubits"], gym.config["gateset"]
    A, T = len(gs), gym.config["max_depth"]
    rec = Recorder(policy)
    syn = BatchedSynthesis(gym, rec, seed=1)
    sols = syn.solve(states, beam_width=W, merge_duplicates=True)
    stats = syn.last_stats
    assert set(stats) == {"beam_width", "targets", "steps", "solved", "mean_gates", "merged", "revisits"} and stats["beam_width"] == W
    assert stats["solved"] == sum(s is not None for s in sols) and stats["steps"] == len(rec.logp) <= T

    okw = oracle_kwargs(gym)

    def fresh(m):
        env = OracleEnv(kind, n, gs, **okw)
        env.set_state(states[m])
        return env

    model_stats: dict = {}
    want = beam_search_merged([fresh(m) for m in range(len(states))], W, A, T, lambda t, envs: rec.logp[t], stats=model_stats)
    print(case, stats, "model", model_stats, "solved", sum(s is not None for s in want))
    assert sols == want
    assert (stats["merged"], stats["revisits"]) == (model_stats["merged"], model_stats["revisits"])
    assert sols[-1] == []  # the identity: solved on arrival
    if case == "clifford-3q-W8":  # H and CX undo themselves and H gates on different qubits commute: both kinds of drop within two steps
        assert stats["merged"] >= 1 and stats["revisits"] >= 1

    solved = 0
    for m, sol in enumerate(sols):  # every solution, replayed on the oracle from its target, solves it with exactly those gates
        if sol is None:
            continue
        solved += 1
        env = fresh(m)
        for a in sol:
            assert not env.success()
            env.step(int(a))
        assert env.success() and env.solution() == sol
        cfg = dict(num_qubits=n, depth_slope=gym.config["depth_slope"], max_depth=T)
        assert replay(kind, cfg, gs, states[m], sol).success()
    assert solved >= 2, stats
    n_logp = len(rec.logp)
    assert syn.solve(states, beam_width=W, merge_duplicates=True) == sols and len(rec.logp) == 2 * n_logp  # no randomness; a fresh history per call


def test_merge_duplicates_is_refused_for_pauli_and_without_a_beam():
    from qiskit_gym_amd.synthesis import BatchedSynthesis

    gym, policy, states, _ = pauli_case()
    syn = BatchedSynthesis(gym, policy, seed=1)
    with pytest.raises(ValueError, match="PauliGym"):
        syn.solve(states, beam_width=4, merge_duplicates=True)
    gym, policy, states, _ = golden_case("clifford_3q_custom", 4, 20, 6)
    with pytest.raises(ValueError, match="beam_width"):
        BatchedSynthesis(gym, policy, seed=1).solve(states, merge_duplicates=True)


def test_without_the_option_the_beam_search_is_what_it_was():
    from qiskit_gym_amd.synthesis import BatchedSynthesis

    W = 8
    gym, policy, states, _ = golden_case("clifford_3q_custom", 16, 20, 6)
    kind, n, gs = gym.env_kind, gym.config["num_qubits"], gym.config["gateset"]
    rec = Recorder(policy)
    syn = BatchedSynthesis(gym, rec, seed=5)
    a = syn.solve(states, beam_width=W)
    keys = set(syn.last_stats)
    assert keys == {"beam_width", "targets", "steps", "solved", "mean_gates"}
    logp = list(rec.logp)
    okw = oracle_kwargs(gym)
    targets = []
    for s in states:
        env = OracleEnv(kind, n, gs, **okw)
        env.set_state(s)
        targets.append(env)
    assert a == beam_search(targets, W, len(gs), gym.config["max_depth"], lambda t, envs: logp[t])  # the unmerged model, as before
    assert syn.solve(states, beam_width=W, merge_duplicates=False) == a and set(syn.last_stats) == keys
    merged = syn.solve(states, beam_width=W, merge_duplicates=True)
    assert set(syn.last_stats) == keys | {"merged", "revisits"}
    assert syn.solve(states, beam_width=W) == a and set(syn.last_stats) == keys  # a merged search in between changes nothing
    assert sum(s is not None for s in merged) >= 2
