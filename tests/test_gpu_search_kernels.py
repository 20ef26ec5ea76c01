"""`BatchedSynthesis.solve(..., fast=True)` in the two deterministic modes: the greedy and the beam search on the policy-layer kernels
(`embed` / `embed_words` -> `mid_head_logp`).  The kernel is pinned by test_gpu_head_logp.py; here the plumbing: every solution replays on
the oracle, the searches are reproducible and equal to loops written from the public pieces, they solve about what the torch path
solves, and without `fast` nothing changed."""
import numpy as np
import pytest

from beammodel import select
from oracle import OracleEnv
from test_gpu_beam import oracle_kwargs, pauli_case
from test_gpu_synthesis import make, replay, targets

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")

NAME = "clifford_3q_custom"
_CASE = {}


def case():
    """The committed TILE-layout policy, 64 targets of 24 scramble gates (as test_gpu_synthesis.py), and the torch path's results on them."""
    if not _CASE:
        kind, cfg, gateset, syn = make(NAME)
        tg = targets(kind, cfg, gateset, 64, 24, 2)
        _CASE.update(kind=kind, cfg=cfg, gateset=gateset, syn=syn, tg=tg)
    return _CASE


def torch_result(key, **kw):
    """`solve(fast=False, **kw)` on the case's targets, computed once."""
    c = case()
    if key not in c:
        sols = c["syn"].solve(c["tg"], fast=False, **kw)
        c[key] = (sols, dict(c["syn"].last_stats))
    return c[key]


def check_valid(sols):
    c = case()
    for state, sol in zip(c["tg"], sols):
        if sol is not None:
            env = replay(c["kind"], c["cfg"], c["gateset"], state, sol)
            assert env.success() and env.solution() == sol
    return sum(s is not None for s in sols)


def operands(c, vec):
    """The kernels' operands from the public packing calls, for one handle."""
    from qiskit_gym_amd.collector import pack_embedding, pack_head, pack_mid
    pol = c["syn"]._policy
    w, b, A = pol.fused_heads()
    return (pack_embedding(vec, pol.embeddings.weight), pol.embeddings.bias.detach().float().contiguous(), pack_mid(pol.common.weight, pol.common.bias),
            pack_head(w, b, A, A, after_mid=True), pol.embeddings.out_features, pol.common.out_features)


def test_greedy_on_the_kernels():
    c = case()
    syn, tg = c["syn"], c["tg"]
    sols = syn.solve(tg, deterministic=True, fast=True)
    stats = dict(syn.last_stats)
    assert stats["kernels"] is True and stats["searches"] == 1
    solved = check_valid(sols)
    assert solved == stats["solved"]
    assert syn.solve(tg, deterministic=True, fast=True) == sols
    ref, ref_stats = torch_result("greedy", deterministic=True)
    assert ref_stats["kernels"] is False
    print(f"greedy: solved fast {solved} / torch {ref_stats['solved']} of {len(tg)}; mean gates {stats['mean_gates']:.2f} / {ref_stats['mean_gates']:.2f}")
    assert solved >= 0.9 * ref_stats["solved"]  # bf16 products may flip near-ties either way

    # the same search as a loop over the public pieces: set_state once, then embed -> mid_head_logp -> step
    from qiskit_gym_amd.collector import embed, mid_head_logp
    M = len(tg)
    vec = syn.env.vec(M, add_inverts=False, add_perms=False, track_solution=False)
    first, b1, mid, head, hidden, common = operands(c, vec)
    vec.set_state(np.asarray(tg, dtype=np.int64), fmt="i64")
    A, T = vec.num_actions(), int(c["cfg"]["max_depth"])
    finished = vec.success.bool().clone()
    solved_at = torch.where(finished, 0, -1)
    acts = torch.full((T, M), A, dtype=torch.int32, device=vec.device)
    for t in range(T):
        h1 = embed(vec, first, b1, hidden, relu=True)
        act = mid_head_logp(h1, mid, common, head, A, want_rows=False)[1].to(torch.int32)
        acts[t] = torch.where(finished, torch.full_like(act, A), act)
        vec.step(acts[t])
        solved_at = torch.where(~finished & vec.success.bool(), t + 1, solved_at)
        finished |= vec.done.bool()
    vec.sync()
    a, n = acts.cpu().numpy(), solved_at.cpu().numpy()
    vec.close()
    assert sols == [a[:n[m], m].tolist() if n[m] >= 0 else None for m in range(M)]


def beam_loop(c, W):
    """The beam search of `solve(beam_width=W)` without merging, from mid_head_logp + beammodel.select (numpy) + copy_envs + step."""
    from qiskit_gym_amd.collector import embed, mid_head_logp
    syn, tg = c["syn"], c["tg"]
    M, T = len(tg), int(c["cfg"]["max_depth"])
    mk = lambda batch: syn.env.vec(batch, add_inverts=False, add_perms=False, track_solution=True)  # noqa: E731
    cur, oth, win = mk(M * W), mk(M * W), mk(M)
    ops = {id(v): operands(c, v) for v in (cur, oth)}
    A, dev = cur.num_actions(), cur.device
    win.set_state(np.asarray(tg, dtype=np.int64), fmt="i64")
    cur.copy_envs(win, torch.arange(M, dtype=torch.int32, device=dev).repeat_interleave(W))
    found = win.success.bool().cpu().numpy().copy()
    best = np.where(found, 0.0, -np.inf).astype(np.float32)
    live = np.zeros((M, W), dtype=np.uint8)
    live[:, 0] = ~found
    live = live.reshape(-1)
    cum, ret = np.zeros(M * W, dtype=np.float32), np.zeros(M * W, dtype=np.float32)
    for t in range(T):
        first, b1, mid, head, hidden, common = ops[id(cur)]
        rows = mid_head_logp(embed(cur, first, b1, hidden, relu=True), mid, common, head, A)[0]
        parent, act, cum, live = select(rows.cpu().numpy(), cum, live, W, A)
        oth.copy_envs(cur, torch.from_numpy(parent.astype(np.int32)).to(dev))
        oth.step(torch.from_numpy(act.astype(np.int32)).to(dev))
        oth.sync()
        ret = (ret[parent] + oth.reward.cpu().numpy()).astype(np.float32)
        solved = (live.astype(bool) & oth.success.bool().cpu().numpy()).reshape(M, W)
        live = live & (1 - oth.done.cpu().numpy())
        score = np.where(solved, ret.reshape(M, W), -np.inf)
        j = score.argmax(axis=1)
        val = score[np.arange(M), j]
        better = val > best
        src = np.where(better, np.arange(M) * W + j, M * W).astype(np.int32)
        win.copy_envs(oth, torch.from_numpy(src).to(dev))
        best, found = np.where(better, val, best).astype(np.float32), found | better
        cur, oth = oth, cur
        if not live.any():
            break
    win.sync()
    sols, lens = win.solutions(T + 64)
    out = [[int(x) for x in sols[m, :lens[m]]] if found[m] else None for m in range(M)]
    for v in (cur, oth, win):
        v.close()
    return out


@pytest.mark.parametrize("merge", [False, True])
@pytest.mark.parametrize("W", [1, 4])
def test_beam_on_the_kernels(W, merge):
    c = case()
    syn, tg = c["syn"], c["tg"]
    sols = syn.solve(tg, beam_width=W, merge_duplicates=merge, fast=True)
    stats = dict(syn.last_stats)
    assert stats["kernels"] is True and stats["beam_width"] == W
    solved = check_valid(sols)
    assert solved == stats["solved"]
    assert syn.solve(tg, beam_width=W, merge_duplicates=merge, fast=True) == sols
    ref, ref_stats = torch_result(("beam", W, merge), beam_width=W, merge_duplicates=merge)
    assert "kernels" not in ref_stats
    print(f"beam W={W} merge={merge}: solved fast {solved} / torch {ref_stats['solved']} of {len(tg)}; "
          f"mean gates {stats['mean_gates']:.2f} / {ref_stats['mean_gates']:.2f}")
    assert solved >= 0.9 * ref_stats["solved"]
    if W == 4 and not merge:
        assert sols == beam_loop(c, W)


def test_without_fast_nothing_changed():
    c = case()
    syn, tg = c["syn"], c["tg"]
    g = syn.solve(tg, deterministic=True)
    assert set(syn.last_stats) == {"kernels", "targets", "searches", "steps", "solved", "searches_solved", "mean_gates"} and syn.last_stats["kernels"] is False
    assert g == torch_result("greedy", deterministic=True)[0]
    b = syn.solve(tg, beam_width=4)
    assert set(syn.last_stats) == {"beam_width", "targets", "steps", "solved", "mean_gates"}
    assert b == torch_result(("beam", 4, False), beam_width=4, merge_duplicates=False)[0]


def test_the_two_search_handles_pack_the_same_first_layer():
    """The beam search packs the first layer once per handle (the packing goes through the handle); both come out equal, and the shared
    middle layer and head are packed once."""
    c = case()
    syn = c["syn"]
    syn.solve(c["tg"][:8], beam_width=2, fast=True)
    cur, oth, _ = syn._beam.vecs
    a, b = syn._beam.first[cur], syn._beam.first[oth]
    assert set(syn._beam.first) == {cur, oth} and a.route == b.route == "state"
    assert a.weight is not b.weight and torch.equal(a.weight, b.weight)
    before = (syn._packed.mid, syn._packed.head)
    syn.solve(c["tg"][:8], beam_width=2, fast=True)  # both handles again: the same first layers, and the one middle layer and head
    assert syn._beam.first[cur] is a and syn._beam.first[oth] is b
    assert syn._packed.mid is before[0] and syn._packed.head is before[1]


def test_an_in_place_weight_update_reaches_every_packed_layer():
    """The packed operands are a snapshot of the policy.  After an in-place update a handle that exists and a handle made afterwards both
    search with the new weights in every layer -- what a fresh BatchedSynthesis on the updated policy returns -- never with a new first
    layer in front of the old middle layer and head."""
    from qiskit_gym_amd.synthesis import BatchedSynthesis

    tg = case()["tg"]
    _, _, _, syn = make(NAME)  # a policy of its own: the shared case keeps its weights
    before = syn.solve(tg[:16], deterministic=True, fast=True)
    assert any(s is not None for s in before)
    with torch.no_grad():  # the head prefers what it avoided
        syn._policy.policy_head.weight.mul_(-1.0)
        syn._policy.policy_head.bias.mul_(-1.0)
    new_handle = syn.solve(tg[:8], deterministic=True, fast=True)
    old_handle = syn.solve(tg[:16], deterministic=True, fast=True)
    fresh = BatchedSynthesis(syn.env, syn._policy, seed=5)
    assert new_handle == fresh.solve(tg[:8], deterministic=True, fast=True)
    assert old_handle == fresh.solve(tg[:16], deterministic=True, fast=True)
    assert old_handle != before and old_handle[:8] == new_handle


def test_fast_where_the_kernels_do_not_apply():
    kind, cfg, gateset, syn = make("lf_5_line")
    tg = targets(kind, cfg, gateset, 4, 8, 1)
    for kw in (dict(deterministic=True), dict(beam_width=2), dict(num_searches=4)):
        with pytest.raises(ValueError):
            syn.solve(tg, fast=True, **kw)
    c = case()
    for kw in (dict(deterministic=True), dict(beam_width=2)):
        with pytest.raises(ValueError):
            c["syn"].solve(c["tg"][:4], fast=True, twists=2, **kw)


def test_pauli_beam_on_the_kernels():
    """PauliGym 3q, random BasicPolicy: the first layer reads the packed observation words (`embed_words`); whatever is returned replays
    on the oracle with its rotation markers."""
    from qiskit_gym_amd.envs.gyms import decode_pauli_solution
    from qiskit_gym_amd.synthesis import BatchedSynthesis

    gym, policy, states, raw = pauli_case()
    kind, n, gs = gym.env_kind, gym.config["num_qubits"], gym.config["gateset"]
    syn = BatchedSynthesis(gym, policy, seed=1)
    sols = syn.solve(states, beam_width=2, fast=True)
    assert syn.last_stats["kernels"] is True
    assert syn._beam.first[syn._beam.vecs[0]].route == "words"
    assert syn.solve(states, beam_width=2, fast=True) == sols
    okw = oracle_kwargs(gym)
    for m, sol in enumerate(sols):
        if sol is None:
            continue
        env = OracleEnv(kind, n, gs, **okw)
        env.pauli_reset_from(*raw[m])
        for a in sol:
            if a < 0x80000000:
                assert not env.success()
                env.step(int(a))
        assert env.success() and env.solution() == sol
        dec = decode_pauli_solution(sol)
        assert [d[1] for d in dec if d[0] == "gate"] == [a for a in sol if a < 0x80000000]
    print("pauli beam W=2 fast:", syn.last_stats)
    # 64 beams hold all 49 two-gate sequences: the neighbour targets are solved whatever the policy prefers, each by releasing its rotation
    wide = syn.solve(states, beam_width=64, fast=True)
    assert syn.last_stats["kernels"] is True and syn.last_stats["solved"] >= 2
    assert any(a >= 0x80000000 for sol in wide if sol is not None for a in sol)
    for m, sol in enumerate(wide):
        if sol is not None:
            env = OracleEnv(kind, n, gs, **okw)
            env.pauli_reset_from(*raw[m])
            for a in sol:
                if a < 0x80000000:
                    env.step(int(a))
            assert env.success() and env.solution() == sol
