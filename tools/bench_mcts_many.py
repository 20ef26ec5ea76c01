"""The tree searches of BatchedSynthesis with K leaves per tree and round of launches, `solve(num_mcts_searches=N, mcts_leaves=K,
virtual_loss=v)`, beside the same searches at K = 1 -- the code path as it was, in the same process -- with the reference's trained policies
(tests/golden/policies): per row time per solve (every call made twice, the second timed: a host clock around a solve that ends in a
synchronise), rounds and launch groups per decision, solved targets, mean gates, mean nodes per decision and `idle`; every 8th answer is
replayed on the oracle.  Rows: N in {8, 32, 100} x K in {1, 4, 8, 16, 32}, K <= N, x virtual_loss in {0, 1} (K = 1: 0 only), deterministic
and sampled with S = 8, with fast=True where the policy-layer kernels take the env (CliffordGym), and with reuse_tree at N = 32.
A "launch group" is one call of the search loop -- select, clone, step, forward pass, clone back, backup: six per round whatever K -- plus
the four of the root pass and the decision; the forward pass is several launches on the torch forward and two on the kernels.
A record, not a gate.  Run on the GPU box: python tools/bench_mcts_many.py [--targets 1024] [--difficulty 20] [--only NAME] [--json FILE]"""
import argparse
import json
import os
import sys
import time

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

from test_reference_policies import MODELS, load  # noqa: E402

import qiskit_gym_amd.envs as envs  # noqa: E402
from qiskit_gym_amd.synthesis import BatchedSynthesis, policy_from_reference_state_dict  # noqa: E402

GYMS = {"clifford": "CliffordGym", "linear_function": "LinearFunctionGym", "permutation": "PermutationGym"}
NAMES = ("clifford_3q_custom", "lf_5_line", "perm_square_3x3")
SIMS, LEAVES, LOSSES = (8, 32, 100), (1, 4, 8, 16, 32), (0.0, 1.0)


def gym_of(name):
    cfg, gateset, w = load(name)
    kind = MODELS[name]
    gym = getattr(envs, GYMS[kind])(cfg["num_qubits"], gateset, depth_slope=cfg["depth_slope"], max_depth=cfg["max_depth"])
    return kind, cfg, gateset, gym, policy_from_reference_state_dict(w)


def drop_handles(syn):
    for held in list(syn._held):  # the pools of one shape are large: drop them before the next
        for vec in syn._held.pop(held).vecs:
            vec.close()


def table(M: int, difficulty: int, names, sims, out):
    from test_gpu_synthesis import replay

    for name in names:
        kind, cfg, gateset, gym, policy = gym_of(name)
        syn = BatchedSynthesis(gym, policy, seed=1)
        v = gym.vec(M, add_inverts=False, add_perms=False, track_solution=False, difficulty=difficulty)
        v.reset(3)  # targets: random scrambles made on the device, read back in the set_state wire format
        states = v.get_state("i64").cpu().numpy()
        v.close()
        rcfg = dict(num_qubits=cfg["num_qubits"], depth_slope=cfg["depth_slope"], max_depth=cfg["max_depth"])
        shapes = [("deterministic", dict(deterministic=True), sims), ("sampled S=8", dict(num_searches=8, mcts_sampled=True), sims)]
        if kind == "clifford":
            shapes += [("deterministic fast", dict(deterministic=True, fast=True), sims), ("sampled S=8 fast", dict(num_searches=8, mcts_sampled=True, fast=True), sims)]
        shapes += [("deterministic reuse", dict(deterministic=True, reuse_tree=True), (32,)), ("sampled S=8 reuse", dict(num_searches=8, mcts_sampled=True, reuse_tree=True), (32,))]
        for what, base, Ns in shapes:
            for N in Ns:
                for K in LEAVES:
                    if K > N:
                        continue
                    for vl in LOSSES if K > 1 else (0.0,):
                        kw = dict(base, num_mcts_searches=N)
                        if K > 1:  # K = 1: the call as it was, without the keywords
                            kw.update(mcts_leaves=K, virtual_loss=vl)
                        try:
                            syn.solve(states, **kw)  # the handles of this batch shape, every code path
                        except ValueError as e:  # the forest limit
                            print(f"{name} x {M}, {what}, N={N}, K={K}: not run: {e}", flush=True)
                            break
                        torch.cuda.synchronize()
                        t0 = time.perf_counter()
                        sols = syn.solve(states, **kw)
                        torch.cuda.synchronize()
                        dt = time.perf_counter() - t0
                        st = syn.last_stats
                        rounds = st.get("rounds", N)
                        groups = 6 * rounds + (0 if "reuse" in st else 4) + 1
                        checked = [replay(kind, rcfg, gateset, states[m].tolist(), sols[m]).success() for m in range(0, M, 8) if sols[m] is not None]
                        row = dict(policy=name, targets=M, difficulty=difficulty, search=what, N=N, K=K, virtual_loss=vl, ms=dt * 1e3, rounds=rounds,
                                   launch_groups=groups, decisions=st["steps"], solved=st["solved"], mean_gates=st["mean_gates"], nodes=st["nodes"],
                                   idle=st.get("idle", st.get("refused", 0)), replayed=[sum(checked), len(checked)])
                        out.append(row)
                        print(f"{name} x {M} (difficulty {difficulty}), {what}, N={N}, K={K}, virtual_loss={vl}: {dt * 1e3:.1f} ms per solve, {rounds} rounds and "
                              f"{groups} launch groups per decision, {st['steps']} decisions, solved {st['solved']}/{M}, mean gates {st['mean_gates']:.3f}, "
                              f"nodes {st['nodes']:.2f}, idle {row['idle']}; {sum(checked)} of {len(checked)} replayed answers solve their target", flush=True)
                    drop_handles(syn)


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--targets", type=int, default=1024)
    ap.add_argument("--difficulty", type=int, default=20)
    ap.add_argument("--only", choices=NAMES, action="append", help="these policies alone")
    ap.add_argument("--sims", type=int, action="append", help="these N alone")
    ap.add_argument("--json", help="the rows, as JSON, into this file as well")
    args = ap.parse_args()
    assert torch.cuda.is_available(), "needs the GPU"
    rows = []
    try:
        table(args.targets, args.difficulty, args.only or NAMES, tuple(args.sims) if args.sims else SIMS, rows)
    finally:
        if args.json:
            with open(args.json, "w") as fh:
                json.dump(rows, fh, indent=1)
