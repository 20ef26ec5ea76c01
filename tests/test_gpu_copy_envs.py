"""qg_vec_copy_envs (VecEnv.copy_envs), the batched Env::clone, on every dispatch row: mid-episode envs are copied with random sources
(repeats included) across handles, within one handle, and from a captured hipGraph.  Each copy must hold its source's state, and then
step like an oracle clone() of the source under the same actions and coins, with an auto-reset collection loop running for twice
max_depth: reward bits, flags, depth, observations (the tracked dense one too) and solution logs after every step.  The first
reset_done after the copy must reset exactly the envs the oracle calls final, although a step before the copy had left its own list."""
import zlib

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

from oracle import OracleEnv  # noqa: E402
from test_dispatch import LAYOUT, TRACK_DENSE, plan  # noqa: E402
from util import f32_bits, line_gateset, oracle_cfg, rng_actions  # noqa: E402

WEIGHTS = dict(n_cnots=0.01, n_layers_cnots=0.25, n_layers=0.125, n_gates=0.001)
PLAIN = dict(add_inverts=False, track_solution=False)
FULL = dict(add_inverts=True, track_solution=True)
FULL_NO_INV = dict(add_inverts=False, track_solution=True)  # LinearFunctionEnv with add_inverts is the LFD layout ...
INV = dict(add_inverts=True, track_solution=False)           # ... and without it is no LFD

# kind, qubits, layout, options of the plain and the full run (the full run adds layer weights)
ROWS = [
    ("clifford", 8, "TILE", PLAIN, FULL), ("clifford", 16, "TILE", PLAIN, FULL), ("linear_function", 16, "TILE", PLAIN, FULL_NO_INV),
    ("linear_function", 32, "TILE", PLAIN, FULL_NO_INV),
    ("clifford", 24, "TILE64", PLAIN, FULL), ("clifford", 32, "TILE64", PLAIN, FULL), ("linear_function", 48, "TILE64", PLAIN, FULL_NO_INV),
    ("linear_function", 64, "TILE64", PLAIN, FULL_NO_INV),
    ("linear_function", 5, "LF8", PLAIN, FULL), ("permutation", 9, "PERM", PLAIN, FULL), ("permutation", 20, "PERMB", PLAIN, FULL),
    ("permutation", 256, "PERMB", PLAIN, FULL),
    ("linear_function", 12, "LFD", INV, FULL), ("linear_function", 40, "LFD", INV, FULL),
    ("pauli", 3, "PTILE-compact", PLAIN, FULL), ("pauli", 26, "PTILE", PLAIN, FULL), ("pauli", 6, "PTILE", PLAIN, FULL),
]
PAULI_ROT = {3: 3, 26: 5, 6: 12}  # max_rotations: compact, wide by qubits, wide by rotations


def _case(kind, n, layout, plain, full, weighted):
    opts = dict(full if weighted else plain)
    cfg = dict(opts, add_perms=False, max_depth=10)
    if kind == "pauli":
        cfg.update(max_rotations=PAULI_ROT[n], difficulty=6, pauli_diff_scale=2, depth_slope=1, pauli_layer_reward=0.0625)
        cfg.pop("add_inverts")
    else:
        cfg.update(difficulty=4, depth_slope=2)
    weights = WEIGHTS if weighted else None
    assert plan(kind, n, LAYOUT, batch=128, metrics_weights=weights, **cfg) == layout
    return cfg, weights


class Side:
    """One VecEnv and its B oracle envs, driven together."""

    def __init__(self, kind, n, gs, B, cfg, weights, gv=None):
        from qiskit_gym_amd.vec import VecEnv

        self.kind, self.cfg, self.B = kind, cfg, B
        self.gv = gv if gv is not None else VecEnv(kind, n, gs, B, metrics_weights=weights, **cfg)
        ocfg = oracle_cfg(cfg)
        self.envs = [OracleEnv(kind, n, gs, metrics_weights=weights, **ocfg) for _ in range(B)]
        self.A = len(gs)
        self.dense = None

    def reset_all(self, seed):
        if self.kind == "pauli":
            self.gv.reset(seed)
            for e, o in enumerate(self.envs):
                o.pauli_reset_seeded(seed, e)
        else:
            draws = rng_actions(seed, self.B, self.cfg["difficulty"], self.A)
            self.gv.reset_with(torch.as_tensor(draws, device="cuda", dtype=torch.int32))
            for e, o in enumerate(self.envs):
                o.reset_with([int(a) for a in draws[:, e]])

    def reset_done(self, seed):
        """qg_vec_reset_done(seed) and the oracle's reset of the envs it calls final, with the same counter-RNG draws."""
        final = np.array([o.is_final() for o in self.envs], dtype=bool)
        self.gv.reset_done(seed)
        for e in np.nonzero(final)[0]:
            if self.kind == "pauli":
                self.envs[e].pauli_reset_seeded(seed, int(e))
            else:
                self.envs[e].reset_with([int(a) for a in rng_actions(seed, [int(e)], self.cfg["difficulty"], self.A)[:, 0]])
        return final

    def step(self, acts, coins):
        self.gv.step(torch.as_tensor(acts, device="cuda", dtype=torch.int32),
                     torch.as_tensor(coins, device="cuda", dtype=torch.uint8) if coins is not None else None)
        for o, a, c in zip(self.envs, acts, coins if coins is not None else np.zeros(self.B, dtype=np.uint8)):
            o.step(int(a), int(c))

    def expect(self, label):
        gv, envs = self.gv, self.envs
        gv.sync()
        np.testing.assert_array_equal(f32_bits(gv.reward.cpu().numpy()), np.array([o.reward_bits() for o in envs], dtype=np.uint32), err_msg=f"reward {label}")
        np.testing.assert_array_equal(gv.done.cpu().numpy(), [int(o.is_final()) for o in envs], err_msg=f"done {label}")
        np.testing.assert_array_equal(gv.success.cpu().numpy(), [int(o.success()) for o in envs], err_msg=f"success {label}")
        np.testing.assert_array_equal(gv.depth.cpu().numpy(), [o.depth() for o in envs], err_msg=f"depth {label}")
        obs = np.stack([np.asarray(o.dense_obs()).reshape(-1) for o in envs])
        if self.dense is not None:  # (before observe(): a full observation does not refresh the tracked one)
            np.testing.assert_array_equal(self.dense.cpu().numpy().reshape(self.B, -1), obs, err_msg=f"tracked dense {label}")
        np.testing.assert_array_equal(gv.observe().cpu().numpy().reshape(self.B, -1), obs, err_msg=f"observe {label}")
        if self.cfg.get("track_solution"):
            cap = self.cfg["max_depth"] + 40
            sols, lens = gv.solutions(cap)
            for e, o in enumerate(envs):
                want = o.solution()
                assert int(lens[e]) == len(want), f"solution length {label} env {e}"
                assert [int(x) for x in sols[e, : lens[e]]] == [int(x) for x in want], f"solution {label} env {e}"


def _actions(rng, side, src_of=None, src_acts=None, src_coins=None):
    acts = rng.integers(0, side.A, size=side.B)
    coins = rng.integers(0, 2, size=side.B).astype(np.uint8) if side.cfg.get("add_inverts") else None
    if src_of is not None:  # a copy takes the action (and the coin) its source takes
        for d, s in src_of.items():
            acts[d] = src_acts[s]
            if coins is not None:
                coins[d] = src_coins[s]
    return acts, coins


@pytest.mark.parametrize("how", ["cross", "same", "graph"])
@pytest.mark.parametrize("weighted", [False, True], ids=["plain", "inverts-track-layers"])
@pytest.mark.parametrize("kind,n,layout,plain,full", ROWS, ids=[f"{r[0]}-{r[1]}" for r in ROWS])
def test_copies_step_like_oracle_clones(kind, n, layout, plain, full, weighted, how):
    cfg, weights = _case(kind, n, layout, plain, full, weighted)
    gs = line_gateset(kind, n)
    rng = np.random.default_rng(zlib.crc32(f"{kind}{n}{weighted}{how}".encode()))
    src = Side(kind, n, gs, 130, cfg, weights)
    dst = src if how == "same" else Side(kind, n, gs, 100, cfg, weights)
    sides = [src] if dst is src else [src, dst]
    for k, side in enumerate(sides):
        side.reset_all(11 + k)
    if dst.kind != "pauli" and plan(kind, n, TRACK_DENSE, batch=dst.B, metrics_weights=weights, **cfg) in ("in-step", "refresh"):
        dst.dense = dst.gv.track_dense()
    # mid-episode, with reset_done in use so that the step right before the copy leaves its finishers as a list / mask.  Across handles
    # the sources run a whole episode (most of them are final when copied) and the destinations three steps (few are): a reset_done that
    # read the destination's stale list would miss the copies
    depth0 = min(cfg["depth_slope"] * cfg["difficulty"], cfg["max_depth"])
    n_pre = {id(src): 3 if how == "same" else depth0, id(dst): 3}
    for t in range(depth0):
        for side in sides:
            if t < n_pre[id(side)]:
                side.reset_done(100 + t)
                side.step(*_actions(rng, side))
    for side in sides:
        side.expect("before the copy")

    if how == "same":
        perm = rng.permutation(src.B)
        d_idx = perm[:50]
        s_idx = rng.choice(perm[50:], size=d_idx.size)
    else:
        d_idx = rng.permutation(dst.B)[:80]
        s_idx = rng.integers(0, src.B, size=d_idx.size)
    s_idx[:4] = s_idx[4]  # a source copied several times
    if how == "graph":
        s_dev = torch.as_tensor(s_idx.astype(np.int32), device="cuda")
        d_dev = torch.as_tensor(d_idx.astype(np.int32), device="cuda")
        torch.cuda.synchronize()
        g = torch.cuda.CUDAGraph()
        with torch.cuda.graph(g):
            dst.gv.copy_envs(src.gv, s_dev, d_dev)
        g.replay()
    else:
        dst.gv.copy_envs(src.gv, s_idx, d_idx)
    clones = {int(d): src.envs[int(s)].clone() for d, s in zip(d_idx, s_idx)}
    for d, o in clones.items():
        dst.envs[d] = o
    dst.expect("after the copy")
    if how == "graph":
        del g
    state_src, state_dst = src.gv.get_state("i64").cpu().numpy(), dst.gv.get_state("i64").cpu().numpy()
    np.testing.assert_array_equal(state_dst[d_idx], state_src[s_idx], err_msg="state of the copies")

    # the first reset_done after the copy: exactly the envs the oracle calls final (not the list the step before the copy left)
    final = dst.reset_done(500)
    if how != "same":
        assert final[d_idx].sum() > final.sum() // 2, "most copies are final"
    dst.expect("reset_done after the copy")

    # then the copies and their sources, and the oracle clones, under the same actions and coins for 2 * max_depth steps
    src_of = {int(d): int(s) for d, s in zip(d_idx, s_idx)}
    for t in range(2 * cfg["max_depth"]):
        if t:
            for side in sides:
                side.reset_done(600 + t)
        sa, sc = _actions(rng, src)
        if dst is src:
            for d, s in src_of.items():  # (sources are never destinations within one handle)
                sa[d] = sa[s]
                if sc is not None:
                    sc[d] = sc[s]
            src.step(sa, sc)
        else:
            src.step(sa, sc)
            dst.step(*_actions(rng, dst, src_of, sa, sc))
        for side in sides:
            side.expect(f"step {t} after the copy")


def test_copy_envs_checks_its_arguments():
    from qiskit_gym_amd import _lib
    from qiskit_gym_amd.vec import VecEnv

    gs = line_gateset("clifford", 4)
    a = VecEnv("clifford", 4, gs, 70, add_inverts=False)
    b = VecEnv("clifford", 4, gs, 70, add_inverts=True)
    with pytest.raises(_lib.QGymError):  # other constructor arguments
        a.copy_envs(b, [0])
    with pytest.raises(ValueError):
        a.copy_envs(a, [1, 2], [3, 3])  # a destination repeats
    with pytest.raises(ValueError):
        a.copy_envs(a, [1, 2], [2, 5])  # env 2 is both
    with pytest.raises(ValueError):
        a.copy_envs(a, [70], [0])  # out of range
    a.copy_envs(a, [], [])  # nothing to do
    a.sync()
