#!/usr/bin/env python3
"""End-to-end example: AlphaZero-style self-play training on LinearFunctionGym with everything on one MI355X.

Collection is `BatchedSynthesis.self_play`: the targets are generated on the device (states=None), every episode is a sampled tree
search (PUCT, N simulations per decision, the move drawn from the root's visit counts), every decision is logged on the device and
packed by `az_pack` into (observation, pi, z, action) samples.  The update below is plain torch: cross-entropy of the policy head
against the visit distribution pi plus the squared error of the value head against the return to go z,

    loss = -(pi * log_softmax(logits)).sum(-1).mean() + vf_coef * (value - z)**2 .mean()

The trainers themselves are out of this repo's scope (the reference's is twisterl.rl.AZ); this script only shows
that the self-play samples are what a learner needs: the share of self-play episodes that end in success goes up.

    python examples/az_linear_function.py [--qubits 4] [--difficulty 5] [--iters 12] [--seed 0]

The search is kept small -- 16 simulations per decision, four leaves per round (EXPERIMENTS section 22: keep `mcts_leaves` well below N);
with 8 simulations one seed in three did not learn within 12 iterations (EXPERIMENTS section 23).
"""
import argparse
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import torch

from qiskit_gym_amd.collector import BasicPolicy
from qiskit_gym_amd.envs import LinearFunctionGym
from qiskit_gym_amd.synthesis import BatchedSynthesis


def train(qubits=4, difficulty=5, episodes=2048, iters=12, simulations=16, leaves=4, epochs=4, minibatches=4, lr=1e-3, vf_coef=0.5, seed=0,
          log=print, return_policy=False):
    """Returns per iteration the share of that iteration's self-play episodes that ended in success."""
    torch.manual_seed(seed)
    edges = [(i, i + 1) for i in range(qubits - 1)] + [(i + 1, i) for i in range(qubits - 1)]
    gym = LinearFunctionGym.from_coupling_map(edges, difficulty=difficulty, max_depth=32, add_inverts=False, add_perms=False)
    rows, cols = gym.obs_shape()
    policy = BasicPolicy(rows * cols, len(gym.config["gateset"]), embedding_size=256, common=128)
    syn = BatchedSynthesis(gym, policy, seed=seed)
    opt = torch.optim.Adam(policy.parameters(), lr=lr)
    history = []
    for it in range(iters):
        t0 = time.perf_counter()
        syn.seed = seed * 7919 + it  # other draws, and (reset_seed) other targets, every iteration
        batch = syn.self_play(num_episodes=episodes, difficulty=difficulty, reset_seed=seed * 7919 + it, num_mcts_searches=simulations,
                              mcts_leaves=leaves)
        t1 = time.perf_counter()
        # the batch's tensors belong to the self-play handles (the next call writes them again): all of them are consumed before it
        obs, pi, z = batch.dense_obs(torch.float32), batch.pi, batch.z
        for _ in range(epochs):
            perm = torch.randperm(batch.n, device=obs.device)
            for mb in perm.chunk(minibatches):
                logits, value = policy(obs[mb])
                loss = -(pi[mb] * torch.log_softmax(logits, dim=-1)).sum(-1).mean() + vf_coef * (value - z[mb]).pow(2).mean()
                opt.zero_grad(set_to_none=True)
                loss.backward()
                opt.step()
        rate = batch.stats["episodes_solved"]
        history.append(rate)
        log(f"iter {it:3d}: {episodes} episodes, {batch.n:6d} samples, solved {rate:6.1%}, mean length {float(batch.lengths.float().mean()):5.2f}, "
            f"loss {loss.item():.4f}, self-play {t1 - t0:.2f} s, update {time.perf_counter() - t1:.2f} s")
    return (history, gym, policy) if return_policy else history


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--qubits", type=int, default=4)
    ap.add_argument("--difficulty", type=int, default=5)
    ap.add_argument("--iters", type=int, default=12)
    ap.add_argument("--episodes", type=int, default=2048)
    ap.add_argument("--simulations", type=int, default=16)
    ap.add_argument("--leaves", type=int, default=4)
    ap.add_argument("--seed", type=int, default=0)
    a = ap.parse_args()
    train(qubits=a.qubits, difficulty=a.difficulty, iters=a.iters, episodes=a.episodes, simulations=a.simulations, leaves=a.leaves, seed=a.seed)
