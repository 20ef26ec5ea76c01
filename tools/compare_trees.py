"""Parent against branch for a Python-only refactor of the collector or the searches (EXPERIMENTS.md sections 14 and 15): import
`qiskit_gym_amd` from the tree given with --tree (a checkout of either commit; both load the same built library), run fixed
workloads and dump what they return.  Two dumps are then compared with --compare.

  --what collector   every parametrisation of the five tests of tests/test_gpu_collector.py, same shapes, seeds and switches (and CliffordGym
                     18q with the 256-feature middle layer: the words route in front of the one-kernel tail): three
                     `collect` calls with `p.mul_(0.5)` on every parameter between them, eager and under hipGraph; SHA-256 of every
                     `Rollout` field of every call and of `env.get_state("packed")` and `env.depth` at the end
  --what searches    one `BatchedSynthesis` per policy running every mode in a row: solutions and `last_stats`, or the ValueError text
  --what routes      the route of every line of tests/test_gpu_policy_routes.py::ROUTES (read from the private attributes on a tree
                     whose collector has no `route`)
  --what launches N  two `collect(8)` calls of configuration N (0: CliffordGym 16q x 1 024 envs, defaults; 1: the same with
                     use_fused_step=False; 2: CliffordGym 18q x 1 024 envs, packed), to run under `rocprofv3 --kernel-trace --stats`
  --compare A B [A2] per case the fields whose hashes differ between dumps A and B; with A2, a second dump of A's tree, a case with a
                     library GEMM between observation and draw is held to A against A2 instead of to identity.  Exit status 1 on a miss."""
import argparse
import hashlib
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FIELDS = ("obs", "actions", "logp", "entropy", "values", "rewards", "dones", "advantages", "returns", "last_values")


def route_of(col):
    if hasattr(col, "route"):
        return [col.route.first, col.route.tail, bool(col.route.fused_step)]
    first = "state" if col._embed is not None else "words" if col._embed_words is not None else "dense"
    tail = "module" if col._heads is None else "mid_head" if col._mid is not None else "head" if col._head is not None else "heads_gemm"
    return [first, tail, bool(col._fused_step)]


def sha(t):
    import torch

    return hashlib.sha256(t.detach().contiguous().view(torch.uint8).cpu().numpy().tobytes()).hexdigest()


def collector_cases():
    """(name, env kind, qubits, env keywords, B, T, policy (torch seed, shape or "tiny"), collector keywords)"""
    out = []
    for store, dt in (("dense", "float32"), ("packed", "float32"), ("packed", "bfloat16"), ("dense", "bfloat16")):
        out.append((f"trajectories-{store}-{dt}", "clifford", 4, dict(add_inverts=False, track_solution=False, difficulty=2), 192, 24, (0, (64, 32)),
                    dict(dtype=dt, seed=77, gamma=0.99, gae_lambda=0.9, store_obs=store, use_bit_embedding=True, use_fused_head=True)))
    for store in ("dense", "packed"):
        out.append((f"generic-{store}", "pauli", 5, dict(track_solution=False, max_rotations=3, difficulty=4, depth_slope=1), 96, 12, (1, "tiny"),
                    dict(dtype="float32", seed=3, store_obs=store)))
    for kind, n, kw in (("clifford", 4, dict(add_inverts=True)), ("linear_function", 6, dict(add_inverts=False)), ("pauli", 5, dict(max_rotations=3, depth_slope=1))):
        out.append((f"graph-{kind}{n}", kind, n, dict(track_solution=False, difficulty=3, **kw), 160, 6, (3, (64, 32)), dict(dtype="float32", seed=21)))
    for kind, n, inv, B in (("clifford", 6, False, 256), ("linear_function", 12, True, 256), ("linear_function", 12, True, 9000)):
        out.append((f"bits-{kind}{n}-B{B}", kind, n, dict(add_inverts=inv, track_solution=False, difficulty=3), B, 5, (5, (128, 64)),
                    dict(dtype="bfloat16", seed=9, store_obs="packed", use_bit_embedding=True, use_fused_head=True)))
    for kind, n, kw in (("pauli", 6, dict(max_rotations=4, depth_slope=1)), ("clifford", 18, dict(add_inverts=False))):
        out.append((f"words-{kind}{n}", kind, n, dict(track_solution=False, difficulty=3, **kw), 300, 5, (5, (128, 64)),
                    dict(dtype="bfloat16", seed=9, store_obs="packed", use_bit_embedding=True, use_fused_head=True)))
    # beyond the tests' list: the words route in front of the one-kernel tail, which they do not pair
    out.append(("words-mid_head-clifford18", "clifford", 18, dict(add_inverts=False, track_solution=False, difficulty=3), 300, 5, (5, (128, 256)),
                dict(dtype="bfloat16", seed=9, store_obs="packed")))
    for kind, n, B, inv in (("clifford", 5, 1000, False), ("clifford", 16, 1000, False), ("linear_function", 12, 1000, False), ("clifford", 5, 9000, False),
                            ("linear_function", 20, 8193, False), ("clifford", 16, 1000, True), ("clifford", 7, 333, True), ("clifford", 12, 8200, True)):
        for fused in (True, False):
            out.append((f"step-{kind}{n}-B{B}-inv{int(inv)}-fused{int(fused)}", kind, n, dict(add_inverts=inv, track_solution=inv, difficulty=2), B, 12, (3, (128, 256)),
                        dict(dtype="bfloat16", seed=5, store_obs="packed", use_bit_embedding=True, use_fused_head=True, use_fused_step=fused)))
    return out


def build_collector(kind, n, env_kw, B, policy, col_kw, use_graph):
    import torch
    from qiskit_gym_amd.collector import BasicPolicy, RolloutCollector
    from qiskit_gym_amd.vec import VecEnv
    from util import line_gateset

    gs = line_gateset(kind, n)
    env = VecEnv(kind, n, gs, B, add_perms=False, **env_kw)
    rows, cols = env.obs_shape_
    seed, shape = policy
    torch.manual_seed(seed)
    if shape == "tiny":
        class Tiny(torch.nn.Module):
            def __init__(self):
                super().__init__()
                self.body = torch.nn.Linear(rows * cols, 48)
                self.pi = torch.nn.Linear(48, len(gs))
                self.v = torch.nn.Linear(48, 1)

            def forward(self, x):
                h = torch.tanh(self.body(x))
                return self.pi(h), self.v(h).squeeze(-1)

        pol = Tiny()
    else:
        pol = BasicPolicy(rows * cols, len(gs), embedding_size=shape[0], common=shape[1])
    kw = dict(col_kw)
    kw["dtype"] = getattr(torch, kw["dtype"])
    return env, RolloutCollector(env, pol, use_graph=use_graph, **kw)


def dump_collector():
    import torch

    out = {}
    for name, kind, n, env_kw, B, T, policy, col_kw in collector_cases():
        for use_graph in (False, True):
            env, col = build_collector(kind, n, env_kw, B, policy, col_kw, use_graph)
            fields = {}
            for call in range(3):
                ro = col.collect(T)
                torch.cuda.synchronize()
                for f in FIELDS:
                    v = getattr(ro, f)
                    fields[f"{call}.{f}"] = None if v is None else sha(v)
                with torch.no_grad():
                    for p in col.policy.parameters():
                        p.mul_(0.5)
            env.sync()
            fields["end.state"], fields["end.depth"] = sha(env.get_state("packed")), sha(env.depth)
            route = route_of(col)
            out[f"{name}-{'graph' if use_graph else 'eager'}"] = {"route": route, "library_gemm": not (route[0] in ("state", "words") and route[1] == "mid_head"),
                                                                 "steps_done": col.steps_done, "fields": fields}
            del col
            env.close()
    return out


def dump_routes():
    import torch
    from test_gpu_policy_routes import ROUTES, basic, handle
    from qiskit_gym_amd.collector import RolloutCollector

    out = {}
    for kind, n, env_kw, shape, dt, store, switches, want in ROUTES:
        env, A = handle(kind, n, **env_kw)
        col = RolloutCollector(env, basic(env, A, *shape), dtype=getattr(torch, dt), seed=1, store_obs=store, **switches)
        out[f"{kind}{n} {env_kw} {shape} {dt} {store} {switches}"] = {"route": route_of(col), "table": list(want)}
        env.close()
    return out


def dump_searches(M):
    from test_gpu_beam import pauli_case
    from test_gpu_synthesis import make
    from qiskit_gym_amd.synthesis import BatchedSynthesis

    modes = [dict(num_searches=4), dict(num_searches=8), dict(deterministic=True), dict(beam_width=2), dict(beam_width=2, merge_duplicates=True),
             dict(beam_width=4), dict(beam_width=4, merge_duplicates=True), dict(beam_width=4, bound="stop"), dict(beam_width=4, bound="prune"),
             dict(beam_width=4, merge_duplicates=True, bound="stop")]
    out = {}

    def run(label, syn, states, calls):
        for kw in calls:
            try:
                sols = syn.solve(states, **kw)
                out[f"{label} {kw}"] = {"solutions": sols, "last_stats": dict(syn.last_stats)}
            except ValueError as e:
                out[f"{label} {kw}"] = {"ValueError": str(e)}

    for name in ("clifford_3q_custom", "lf_5_line", "perm_square_3x3"):
        _, _, _, syn = make(name)
        syn.seed = 1
        v = syn.env.vec(M, add_inverts=False, add_perms=False, track_solution=False, difficulty=24)
        v.reset(3)  # random scrambles made on the device, read back in the set_state wire format
        states = v.get_state("i64").cpu().numpy()
        v.close()
        calls = [dict(m, **f) for m in modes for f in ({}, dict(fast=True))]
        for V in (2, 64):  # 64: cut to the view count the coupling map has
            calls += [dict(m, twists=V, **k) for m in modes for k in ({}, dict(twist_kernels=True))]
        run(name, syn, states, calls)
    gym, policy, states, _ = pauli_case()
    run("pauli", BatchedSynthesis(gym, policy, seed=1), states, [dict(m, **f) for m in modes if not m.get("merge_duplicates") for f in ({}, dict(fast=True))])
    return out


def launches(which):
    import torch

    kind, n, env_kw, col_kw = [("clifford", 16, {}, {}), ("clifford", 16, {}, dict(use_fused_step=False)), ("clifford", 18, {}, dict(store_obs="packed"))][which]
    env, col = build_collector(kind, n, env_kw, 1024, (1, (512, 256)), dict(dtype="bfloat16", seed=1, **col_kw), False)
    for _ in range(2):
        col.collect(8)
    torch.cuda.synchronize()
    env.sync()
    print("route", route_of(col))


def compare(a, b, a2):
    A, B = json.load(open(a)), json.load(open(b))
    A2 = json.load(open(a2)) if a2 else None
    bad = 0
    if A.keys() != B.keys():
        print("case lists differ:", sorted(set(A) ^ set(B)))
        bad += 1
    for case in sorted(A.keys() & B.keys()):
        x, y = A[case], B[case]
        if "fields" not in x:
            if x != y:
                print(f"DIFFERS {case}: {json.dumps(x)[:200]} | {json.dumps(y)[:200]}")
                bad += 1
            continue
        diff = sorted(k for k in x["fields"] if x["fields"][k] != y["fields"].get(k))
        own = sorted(k for k in x["fields"] if A2 is not None and x["fields"][k] != A2[case]["fields"].get(k))
        head = {k: (x[k], y[k]) for k in ("route", "steps_done") if x[k] != y[k]}
        ok = not head and (not diff or (x["library_gemm"] and set(diff) <= set(own)))
        if diff or own or head:
            print(f"{'within A against A2' if ok else 'DIFFERS'} {case} route {x['route']}: A/B {diff or head} A/A2 {own}")
        bad += not ok
    print(f"{len(A)} cases, {bad} misses")
    return 1 if bad else 0


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--tree", default=ROOT)
    ap.add_argument("--what", choices=("collector", "searches", "routes", "launches"))
    ap.add_argument("--config", type=int, default=0)
    ap.add_argument("--targets", type=int, default=1024)
    ap.add_argument("--out")
    ap.add_argument("--compare", nargs="+")
    args = ap.parse_args()
    if args.compare:
        sys.exit(compare(args.compare[0], args.compare[1], args.compare[2] if len(args.compare) > 2 else None))
    tree = os.path.abspath(args.tree)
    sys.path.insert(0, os.path.join(ROOT, "tests"))  # the tests' helpers: gatesets, committed policies
    sys.path.insert(0, tree)
    import qiskit_gym_amd

    assert os.path.dirname(os.path.dirname(os.path.abspath(qiskit_gym_amd.__file__))) == tree, qiskit_gym_amd.__file__
    if args.what == "launches":
        return launches(args.config)
    out = {"collector": dump_collector, "routes": dump_routes, "searches": lambda: dump_searches(args.targets)}[args.what]()
    text = json.dumps(out, indent=1, sort_keys=True)
    if args.out:
        with open(args.out, "w") as f:
            f.write(text)
    print(f"{args.what} from {tree}: {len(out)} cases, {len(text)} bytes, sha256 {hashlib.sha256(text.encode()).hexdigest()}")
    if args.what == "routes":
        for k, v in out.items():
            print("  ", "ok      " if v["route"] == v["table"] else "DISAGREE", v["route"], k)


if __name__ == "__main__":
    main()
