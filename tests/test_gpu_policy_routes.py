"""The operands the collector and the searches share (`qiskit_gym_amd/policy_kernels.py`) and the route a `RolloutCollector` decides on in
its constructor.  Objects are constructed only, at 64 envs: no collection runs here -- every tail and every first-layer route runs end to
end against the oracle in test_gpu_collector.py, test_gpu_search_kernels.py and test_gpu_search_modes.py."""
import pytest

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")

from test_gpu_synthesis import targets  # noqa: E402
from util import line_gateset  # noqa: E402

B = 64


def handle(kind, n, **kw):
    from qiskit_gym_amd.vec import VecEnv

    gs = line_gateset(kind, n)
    if kind != "pauli":
        kw.setdefault("add_inverts", False)
    return VecEnv(kind, n, gs, B, add_perms=False, track_solution=False, difficulty=3, **kw), len(gs)


def basic(env, A, embedding_size, common):
    from qiskit_gym_amd.collector import BasicPolicy

    torch.manual_seed(7)
    return BasicPolicy(env.obs_shape_[0] * env.obs_shape_[1], A, embedding_size=embedding_size, common=common)


# (env kind, qubits, env keywords, (embedding_size, common), dtype, store_obs, collector switches) -> (first, tail, fused_step), as the
# constructor before `route` existed set its private attributes.  common=32 fails pack_head's in_features % 64, common=64 pack_mid's 256
# output features; the two words lines have an even row count and embedding_size % 128 == 0, which `pack_embed_words` asks for.
ROUTES = [
    ("clifford", 4, {}, (64, 32), "float32", "dense", {}, ("dense", "heads_gemm", False)),
    ("clifford", 4, {}, (64, 32), "bfloat16", "packed", {}, ("state", "heads_gemm", False)),
    ("clifford", 4, {}, (128, 64), "bfloat16", "packed", {}, ("state", "head", False)),
    ("clifford", 4, {}, (128, 256), "bfloat16", "packed", {}, ("state", "mid_head", True)),
    ("clifford", 4, {}, (128, 256), "bfloat16", "packed", dict(use_fused_step=False), ("state", "mid_head", False)),
    ("clifford", 4, {}, (128, 256), "bfloat16", "packed", dict(use_fused_head=False), ("state", "heads_gemm", False)),
    ("clifford", 4, {}, (128, 256), "bfloat16", "packed", dict(use_bit_embedding=False), ("dense", "mid_head", True)),
    ("clifford", 4, dict(add_inverts=True), (128, 256), "bfloat16", "packed", {}, ("state", "mid_head", True)),
    ("linear_function", 12, dict(add_inverts=False), (128, 256), "bfloat16", "packed", {}, ("state", "mid_head", True)),
    ("linear_function", 12, dict(add_inverts=True), (128, 256), "bfloat16", "packed", {}, ("state", "mid_head", False)),
    ("linear_function", 6, {}, (128, 256), "bfloat16", "packed", {}, ("dense", "mid_head", False)),
    ("clifford", 18, {}, (128, 256), "bfloat16", "packed", {}, ("words", "mid_head", False)),
    ("clifford", 18, {}, (128, 256), "bfloat16", "dense", {}, ("dense", "mid_head", False)),
    ("pauli", 6, dict(max_rotations=4), (128, 64), "bfloat16", "packed", {}, ("words", "head", False)),
]


@pytest.mark.parametrize("kind,n,env_kw,shape,dtype_name,store_obs,switches,want", ROUTES)
def test_the_route_the_constructor_decides_on(kind, n, env_kw, shape, dtype_name, store_obs, switches, want):
    from qiskit_gym_amd.collector import CollectorRoute, RolloutCollector

    env, A = handle(kind, n, **env_kw)
    col = RolloutCollector(env, basic(env, A, *shape), dtype=getattr(torch, dtype_name), seed=1, store_obs=store_obs, **switches)
    assert col.route == CollectorRoute(*want)
    with pytest.raises(Exception):  # frozen: decided once
        col.route.first = "dense"
    env.close()


def test_the_route_of_a_policy_that_is_no_basic_policy():
    """The `Tiny` module of test_collector_runs_pauli_and_generic_policies on its PauliGym handle."""
    from qiskit_gym_amd.collector import CollectorRoute, RolloutCollector

    env, A = handle("pauli", 5, max_rotations=3, depth_slope=1)
    rows, cols = env.obs_shape_

    class Tiny(torch.nn.Module):
        def __init__(self):
            super().__init__()
            self.body = torch.nn.Linear(rows * cols, 48)
            self.pi = torch.nn.Linear(48, A)
            self.v = torch.nn.Linear(48, 1)

        def forward(self, x):
            h = torch.tanh(self.body(x))
            return self.pi(h), self.v(h).squeeze(-1)

    col = RolloutCollector(env, Tiny(), dtype=torch.float32, seed=3)
    assert col.route == CollectorRoute("dense", "module", False) and col.operands is None
    env.close()


def buffers(ops, first):
    return {"w": ops.w, "b": ops.b, "bias": ops.bias, "mid": ops.mid, "head": ops.head, "first": first.weight}


def packed_bytes(name, t, ops):
    """The bytes of buffer `name` that its packer writes: all of them, but for the packed head -- that buffer is whole 16 KiB chunks
    (`qg_policy_head_packed_bytes`) of which `qg_policy_pack_head` writes the (K / 16 + 1) k-steps x tiles x 64 lanes x 8 bf16 of its layout;
    what lies past them is whatever the allocator left there, in every head ever packed, and no kernel's result depends on it."""
    raw = t.contiguous().view(-1).view(torch.uint8)
    if name != "head":
        return raw
    written = (ops.w.shape[1] // 16 + 1) * ((ops.A + 1 + 31) // 32) * 64 * 8 * 2
    assert 0 < written <= raw.numel() < written + 16384
    return raw[:written]


@pytest.mark.parametrize("n,route", [(4, "state"), (18, "words")])
def test_repack_is_in_place_and_complete(n, route):
    """`PolicyOperands.repack_` after an in-place update of every parameter: no buffer moved, and every buffer holds the bytes of
    operands built fresh from the updated policy."""
    from qiskit_gym_amd.policy_kernels import PolicyOperands, first_layer

    env, A = handle("clifford", n)
    pol = basic(env, A, 128, 256).to(device=env.device, dtype=torch.bfloat16)
    ops, first = PolicyOperands(pol), first_layer(env, pol.embeddings.weight)
    assert first.route == route and ops.mid is not None and ops.head is not None and ops.why is None
    held = buffers(ops, first)
    where = {k: t.data_ptr() for k, t in held.items()}
    stale = {k: t.clone() for k, t in held.items()}
    with torch.no_grad():
        for p in pol.parameters():
            p.mul_(0.5)
    ops.repack_(pol, first, env)
    assert buffers(ops, first).keys() == where.keys() and all(t is held[k] and t.data_ptr() == where[k] for k, t in buffers(ops, first).items())
    fresh = buffers(PolicyOperands(pol), first_layer(env, pol.embeddings.weight))
    for k, t in held.items():
        assert t.dtype == fresh[k].dtype and t.shape == fresh[k].shape, k
        assert torch.equal(packed_bytes(k, t, ops), packed_bytes(k, fresh[k], ops)), k
        assert not torch.equal(t, stale[k]), k  # the update reached it
    env.close()


def test_the_collector_and_the_searches_pack_the_same_bytes():
    """One `BasicPolicy` on a CliffordGym 4q handle: the operands a `RolloutCollector` holds and the snapshot of a `BatchedSynthesis`
    after a `fast=True` solve are byte-equal in the middle layer, the head and the first layer's bias -- both are `PolicyOperands`."""
    from qiskit_gym_amd.collector import RolloutCollector
    from qiskit_gym_amd.envs import CliffordGym
    from qiskit_gym_amd.policy_kernels import PolicyOperands
    from qiskit_gym_amd.synthesis import BatchedSynthesis

    n = 4
    gs = line_gateset("clifford", n)
    cfg = dict(num_qubits=n, depth_slope=2, max_depth=16)
    gym = CliffordGym(n, gs, depth_slope=cfg["depth_slope"], max_depth=cfg["max_depth"])
    vec = gym.vec(B, add_inverts=False, add_perms=False, track_solution=False)
    syn = BatchedSynthesis(gym, basic(vec, len(gs), 128, 256), dtype=torch.bfloat16, seed=1)
    syn.solve(targets("clifford", cfg, gs, 8, 4, 1), num_searches=2, fast=True)
    assert syn.last_stats["kernels"] is True
    col = RolloutCollector(vec, syn._policy, dtype=torch.bfloat16, seed=1, store_obs="packed")
    assert col.route.tail == "mid_head" and isinstance(col.operands, PolicyOperands) and isinstance(syn._packed, PolicyOperands)
    for name in ("mid", "head", "bias"):
        a, b = getattr(col.operands, name), getattr(syn._packed, name)
        assert a is not b and a.dtype == b.dtype and a.shape == b.shape, name
        assert torch.equal(packed_bytes(name, a, col.operands), packed_bytes(name, b, col.operands)), name
    vec.close()
