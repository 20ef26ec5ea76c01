"""The two deterministic searches of BatchedSynthesis on the torch forward (fast=False: three library GEMMs, log_softmax) and on the
policy-layer kernels (fast=True: embed -> mid_head_logp), same targets, same process: ms per solve, steps, solved targets, mean gates for
the greedy search and beam widths 4 / 16 with and without merge_duplicates on clifford_3q_custom (the committed policy on a TILE layout),
and beam width 4 on CliffordGym 16q with a seeded random BasicPolicy.  Then the kernel alone: mid_head_logp with and without rows beside
mid_head_sample at 1 024 and 65 536 envs, 170 actions, on device events.  A record, not a gate.
Run on the GPU box: python tools/bench_search_kernels.py [--targets 1024] [--reps 3]"""
import argparse
import os
import sys
import time

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

from test_reference_policies import MODELS, load  # noqa: E402

import qiskit_gym_amd.envs as envs  # noqa: E402
from qiskit_gym_amd.collector import BasicPolicy, mid_head_logp, mid_head_sample, pack_head, pack_mid  # noqa: E402
from qiskit_gym_amd.envs.gateset import gateset_from_coupling_map, line_edges  # noqa: E402
from qiskit_gym_amd.synthesis import BatchedSynthesis, policy_from_reference_state_dict  # noqa: E402


def device_targets(gym, M, difficulty):
    v = gym.vec(M, add_inverts=False, add_perms=False, track_solution=False, difficulty=difficulty)
    v.reset(3)  # random scrambles made on the device, read back in the set_state wire format
    states = v.get_state("i64").cpu().numpy()
    v.close()
    return states


def timed(syn, states, reps, **kw):
    syn.solve(states, **kw)  # builds the handles of this batch shape, warms the library
    torch.cuda.synchronize()
    best = float("inf")
    for _ in range(reps):
        t0 = time.perf_counter()
        syn.solve(states, **kw)
        torch.cuda.synchronize()
        best = min(best, time.perf_counter() - t0)
    return best, dict(syn.last_stats)


def table(label, syn, states, runs, reps):
    for name, kw in runs:
        for fast in (False, True):
            dt, st = timed(syn, states, reps, fast=fast, **kw)
            print(f"{label} x {len(states)} targets, {name}, fast={fast}: {dt * 1e3:.1f} ms per solve (best of {reps}), {st['steps']} steps, "
                  f"{dt * 1e6 / max(1, st['steps']):.0f} us per step, solved {st['solved']}/{len(states)}, mean gates {st['mean_gates']:.2f}", flush=True)


def kernel_times(reps=50):
    A, K1, F = 170, 512, 256
    g = torch.Generator(device="cuda")
    g.manual_seed(3)
    w2 = (torch.randn((F, K1), device="cuda", generator=g) * (2.0 / K1) ** 0.5).to(torch.bfloat16)
    w3 = (torch.randn((A + 1, F), device="cuda", generator=g) * (2.0 / F) ** 0.5).to(torch.bfloat16)
    pm, ph = pack_mid(w2, None), pack_head(w3, None, A, A, after_mid=True)
    for B in (1024, 65536):
        h1 = torch.randn((B, K1), device="cuda", generator=g).clamp_min(0).to(torch.bfloat16)
        rows = torch.empty((B, 172), dtype=torch.float32, device="cuda")
        act = torch.empty(B, dtype=torch.int32, device="cuda")
        f = torch.empty((3, B), dtype=torch.float32, device="cuda")
        calls = {"mid_head_sample": lambda: mid_head_sample(h1, pm, F, ph, A, 1, 2, actions=act, logp=f[0], entropy=f[1], values=f[2]),
                 "mid_head_logp rows on": lambda: mid_head_logp(h1, pm, F, ph, A, logp_rows=rows, actions=act, best_logp=f[0], entropy=f[1], values=f[2]),
                 "mid_head_logp rows off": lambda: mid_head_logp(h1, pm, F, ph, A, want_rows=False, actions=act, best_logp=f[0], entropy=f[1], values=f[2])}
        us = {k: [] for k in calls}
        for _ in range(5):  # alternating: the three see the same clocks
            for k, fn in calls.items():
                fn()
                torch.cuda.synchronize()
                a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                a.record()
                for _ in range(reps):
                    fn()
                b.record()
                torch.cuda.synchronize()
                us[k].append(a.elapsed_time(b) * 1e3 / reps)
        print(f"{B} envs, A = {A}, K1 = {K1}: " + ", ".join(f"{k} {sorted(v)[len(v) // 2]:.1f} us" for k, v in us.items()) + f" (median of 5 x {reps} back-to-back launches)",
              flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--targets", type=int, default=1024)
    ap.add_argument("--reps", type=int, default=3)
    a = ap.parse_args()
    print(torch.cuda.get_device_name(0), flush=True)
    cfg, gateset, w = load("clifford_3q_custom")
    gym = getattr(envs, "CliffordGym")(cfg["num_qubits"], gateset, depth_slope=cfg["depth_slope"], max_depth=cfg["max_depth"])
    assert MODELS["clifford_3q_custom"] == "clifford"
    syn = BatchedSynthesis(gym, policy_from_reference_state_dict(w), seed=1)
    runs = [("greedy", dict(deterministic=True))]
    runs += [(f"beam_width={W} merge={m}", dict(beam_width=W, merge_duplicates=m)) for W in (4, 16) for m in (False, True)]
    table("clifford_3q_custom", syn, device_targets(gym, a.targets, 24), runs, a.reps)
    n, gs = gateset_from_coupling_map(line_edges(16, True), None, ["H", "S", "Sdg", "SX", "SXdg", "CX", "CZ", "SWAP"])
    gym16 = envs.CliffordGym(n, gs, max_depth=40)
    torch.manual_seed(16)
    syn16 = BatchedSynthesis(gym16, BasicPolicy(4 * n * n, len(gs)), seed=1)
    table("CliffordGym 16q (random policy)", syn16, device_targets(gym16, a.targets, 8), [("beam_width=4 merge=False", dict(beam_width=4))], a.reps)
    kernel_times()


if __name__ == "__main__":
    main()
