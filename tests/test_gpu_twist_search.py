"""`BatchedSynthesis.solve(twists=V, twist_kernels=True)`: the searches under symmetry views on the policy-layer kernels
(`observe_twisted_words` -> `embed_words` -> `mid_head_sample` / `mid_head_logp` -> `untwist_actions` -> `step`).  The kernels are pinned
by test_gpu_twist_words.py, test_gpu_embed_words.py and test_gpu_head_logp.py; here the plumbing, on the three committed policies -- among
them the 5 x 5 and the 9 x 9 byte-word observation that `fast=True` does not reach: every solution replays on the oracle, the searches are
reproducible, they solve about what the torch path solves under the same views, the greedy search equals a loop written from the public
pieces, an in-place weight update is followed, and the argument errors."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")

from test_gpu_synthesis import make  # noqa: E402
from test_gpu_vec_twists import all_views, confirm, search_setup  # noqa: E402
from test_reference_policies import MODELS  # noqa: E402
from util import line_gateset  # noqa: E402

MODES = {"greedy": dict(deterministic=True), "beam2": dict(beam_width=2), "beam4_merged": dict(beam_width=4, merge_duplicates=True),
         "sampled8": dict(num_searches=8)}
_TORCH = {}


def torch_path(name, mode):
    """`solve(twists=V)` on the torch forward, on the same targets: computed once per (policy, mode)."""
    if (name, mode) not in _TORCH:
        _, _, _, syn, tg = search_setup(name)
        sols = syn.solve(tg, twists=len(all_views(name)), **MODES[mode])
        _TORCH[name, mode] = (sols, dict(syn.last_stats))
    return _TORCH[name, mode]


@pytest.mark.parametrize("mode", sorted(MODES))
@pytest.mark.parametrize("name", sorted(MODELS))
def test_twisted_searches_on_the_kernels(name, mode):
    _, _, _, syn, tg = search_setup(name)
    V = len(all_views(name))
    sols = syn.solve(tg, twists=V, twist_kernels=True, **MODES[mode])
    stats = dict(syn.last_stats)
    assert len(sols) == len(tg)
    confirm(name, sols)  # real, untwisted actions: each replays to success on the oracle with solution() == sol
    solved = sum(s is not None for s in sols)
    assert solved == stats["solved"] and stats["kernels"] is True
    ref, ref_stats = torch_path(name, mode)
    assert stats["views"] == ref_stats["views"] == V
    assert ref_stats.get("kernels", False) is False
    assert syn.solve(tg, twists=V, twist_kernels=True, **MODES[mode]) == sols
    print(f"{name} {mode} V={V}: solved kernels {solved} / torch {ref_stats['solved']} of {len(tg)}; "
          f"mean gates {stats['mean_gates']:.2f} / {ref_stats['mean_gates']:.2f}")
    assert ref_stats["solved"] >= len(tg) // 2  # the comparison below is not vacuous
    assert solved >= 0.9 * ref_stats["solved"]  # bf16 products may flip near-ties either way (the margin of test_gpu_search_kernels.py)


@pytest.mark.parametrize("name", sorted(MODELS))
def test_greedy_equals_a_loop_over_the_public_pieces(name):
    """set_state once, then observe_twisted_words -> embed_words -> mid_head_logp -> untwist_actions -> step; env m * V + s sees view s, a
    target's winner is its best return, the lowest view among equals."""
    from qiskit_gym_amd.collector import embed_words, mid_head_logp, pack_embed_words, pack_head, pack_mid

    _, cfg, _, syn, tg = search_setup(name)
    views = all_views(name)
    V, M = len(views), len(tg)
    sols = syn.solve(tg, deterministic=True, twists=V, twist_kernels=True)
    vec = syn.env.vec(M * V, add_inverts=False, add_perms=True, track_solution=False)
    pol = syn._policy
    rows, cols = vec.obs_shape_
    rows_out = rows + rows % 2
    w1 = pol.embeddings.weight.detach()
    first = pack_embed_words(torch.nn.functional.pad(w1, (0, cols)) if rows % 2 else w1, rows_out, cols)
    b1 = pol.embeddings.bias.detach().float().contiguous()
    w, b, A = pol.fused_heads()
    mid, head = pack_mid(pol.common.weight, pol.common.bias), pack_head(w, b, A, A, after_mid=True)
    hidden, common = pol.embeddings.out_features, pol.common.out_features
    obs_perms = vec.twists()[0]
    index = [-1] + [obs_perms.index(o) for o, _ in views[1:]]  # view 0: no twist
    tw = torch.tensor(index, dtype=torch.int32, device=vec.device).repeat(M).contiguous()
    vec.set_state(np.repeat(np.asarray(tg, dtype=np.int64), V, axis=0), fmt="i64")
    T = int(cfg["max_depth"])
    finished = vec.success.bool().clone()
    solved_at = torch.where(finished, 0, -1)
    ret = torch.zeros(M * V, dtype=torch.float32, device=vec.device)
    acts = torch.full((T, M * V), A, dtype=torch.int32, device=vec.device)
    for t in range(T):
        h1 = embed_words(vec.observe_twisted_words(tw), cols, first, b1, hidden, relu=True)
        act = mid_head_logp(h1, mid, common, head, A, want_rows=False)[1].to(torch.int32)
        act = vec.untwist_actions(act, tw)
        acts[t] = torch.where(finished, torch.full_like(act, A), act)
        vec.step(acts[t])
        ret += torch.where(~finished, vec.reward, torch.zeros_like(ret))
        solved_at = torch.where(~finished & vec.success.bool(), t + 1, solved_at)
        finished |= vec.done.bool()
    vec.sync()
    score = torch.where(solved_at >= 0, ret, torch.full_like(ret, -float("inf"))).view(M, V)
    best = (torch.arange(M, device=vec.device) * V + score.argmax(dim=1)).cpu().numpy()
    a, n = acts.cpu().numpy(), solved_at.cpu().numpy()
    vec.close()
    assert sols == [a[: n[e], e].tolist() if n[e] >= 0 else None for e in best]
    assert sum(s is not None for s in sols) >= M // 2


def test_an_in_place_weight_update_is_repacked():
    """The packed first layer of the views is a snapshot of the weights: after an in-place `add_` the search returns what a fresh
    BatchedSynthesis on the updated policy returns, and not what it returned before."""
    from qiskit_gym_amd.synthesis import BatchedSynthesis

    name = "lf_5_line"
    tg = search_setup(name)[4][:16]
    _, _, _, syn = make(name)  # a policy of its own: the shared one keeps its weights
    kw = dict(deterministic=True, twists=2, twist_kernels=True)
    before = syn.solve(tg, **kw)
    assert any(s is not None for s in before)
    g = torch.Generator(device="cpu").manual_seed(3)
    with torch.no_grad():
        w = syn._policy.embeddings.weight
        w.add_((torch.randn(w.shape, generator=g) * 2.0 * w.abs().max().item()).to(w.device))
    after = syn.solve(tg, **kw)
    fresh = BatchedSynthesis(syn.env, syn._policy, seed=5)
    assert after == fresh.solve(tg, **kw)
    assert after != before


def test_twist_kernels_argument_errors():
    from qiskit_gym_amd.collector import BasicPolicy
    from qiskit_gym_amd.envs import PauliGym
    from qiskit_gym_amd.synthesis import BatchedSynthesis

    _, _, _, syn, tg = search_setup("lf_5_line")
    modes = (dict(deterministic=True), dict(beam_width=2), dict(num_searches=4))
    for kw in modes:
        with pytest.raises(ValueError):
            syn.solve(tg[:4], twist_kernels=True, **kw)  # without twists
        with pytest.raises(ValueError):
            syn.solve(tg[:4], twists=2, twist_kernels=True, fast=True, **kw)
    with pytest.raises(ValueError):
        syn.solve(tg[:4], fast=True, twist_kernels=True)
    gs = line_gateset("pauli", 2)
    gym = PauliGym(2, gs, max_rotations=3, max_depth=12, difficulty=1)
    r, c = gym.obs_shape()
    pauli = BatchedSynthesis(gym, BasicPolicy(r * c, len(gs)), seed=3)
    for kw in modes[:2]:
        with pytest.raises(ValueError):
            pauli.solve([[0] * (1 + 16)], twists=2, twist_kernels=True, **kw)

    class Other(torch.nn.Module):  # not a BasicPolicy
        def __init__(self, inner):
            super().__init__()
            self.inner = inner

        def forward(self, x):
            return self.inner(x)

    other = BatchedSynthesis(syn.env, Other(syn._policy), seed=5)
    narrow = BatchedSynthesis(syn.env, BasicPolicy(25, len(syn.env.config["gateset"]), embedding_size=64), seed=5)  # a hidden size the first layer does not take
    for bad in (other, narrow):
        for kw in modes:
            with pytest.raises(ValueError, match="twist_kernels=True needs"):
                bad.solve(tg[:4], twists=2, twist_kernels=True, **kw)
        assert len(bad.solve(tg[:4], twists=2, deterministic=True)) == 4  # the torch path takes them
    # more than 64 columns: a row of the view does not fit a 64-bit word.  No env with twists is that wide (CliffordGym ends at 32 qubits,
    # 64 columns), so the operands are asked for a handle-shaped stand-in
    import types

    from qiskit_gym_amd.policy_kernels import first_layer

    wide = BatchedSynthesis(syn.env, BasicPolicy(4 * 66, 8).cuda(), seed=1)
    stand_in = types.SimpleNamespace(obs_shape_=(4, 66), packed_words_per_env=4)
    with pytest.raises(ValueError, match="a row of the view is one 64-bit word"):  # the shared function: the packer's reason
        first_layer(stand_in, wide._policy.embeddings.weight, ("views",))
    with pytest.raises(ValueError, match=r"twist_kernels=True needs .* \(a row of the view is one 64-bit word\)"):  # the searches' wording around it
        wide._first_layer(stand_in, {}, views=True)
