// qm_step1.hpp -- the body of the one-step kernel of the TILE layout (CliffordEnv N <= 16, LinearFunctionEnv 8 < N <= 32, no add_inverts),
// shared by qm_step1_kernel (kernels_qm_step1.hip), the step lanes of qm_reset_step_kernel (kernels_qm.hip) and by the policy kernel that samples an action and steps its env in the same launch
// (mid_head_sample_kernel, kernels_policy.hip).  Reference: Clifford::step rust/src/envs/clifford.rs:321-347.
#pragma once

#include "device_common.hpp"

namespace qg {

#define QM_IDENTITY 0x8421u

template <bool HAS_Z>
__device__ inline void qm_group_get(const uint32_t (&u)[4], uint32_t q, uint32_t &x, uint32_t &z) {
    const uint32_t o = 0u - (q & 1u);
    if constexpr (HAS_Z) {  // {X[2g], Z[2g], X[2g+1], Z[2g+1]}
        x = (u[2] & o) | (u[0] & ~o);
        z = (u[3] & o) | (u[1] & ~o);
    } else {                // rows 4g .. 4g+3
        const uint32_t h = 0u - ((q >> 1) & 1u);
        const uint32_t lo = (u[1] & o) | (u[0] & ~o), hi = (u[3] & o) | (u[2] & ~o);
        x = (hi & h) | (lo & ~h);
        z = 0u;
    }
}
template <bool HAS_Z>
__device__ inline void qm_group_put(uint32_t (&u)[4], uint32_t q, uint32_t x, uint32_t z) {
    if constexpr (HAS_Z) {
        const uint32_t o = 0u - (q & 1u);
        u[0] = (u[0] & o) | (x & ~o); u[1] = (u[1] & o) | (z & ~o);
        u[2] = (x & o) | (u[2] & ~o); u[3] = (z & o) | (u[3] & ~o);
    } else {
#pragma unroll
        for (uint32_t k = 0; k < 4; ++k) u[k] = (q & 3u) == k ? x : u[k];
    }
}

// The fields the front of the one-step chain reads -- the action, depth and bad-mask loads, the gate entry behind the action, the rows behind the
// gate entry.  qm_step1_kernel (kernels_qm_step1.hip) takes them as leading kernel parameters of their own (14 dwords: what the kernel-argument preload
// delivers in SGPRs at wave start, no scalar load in front of the first vector load); every other caller fills them from its StepArgs.
struct Step1Front {
    const void *actions;
    int32_t *depth;
    uint32_t *bad;
    const GateEntry *gates;
    void *state;
    uint64_t B;
    uint32_t flags, num_actions;
};
__device__ inline Step1Front step1_front(const StepArgs &a) { return Step1Front{a.actions, a.depth, a.bad, a.gates, a.state, a.B, a.flags, a.num_actions}; }

// QG_STEP1_ABLATE (development, tools/build_variant.sh; EXPERIMENTS.md round 6) puts one avoidable round trip back: bit 0 -- the front in its old
// order (action, then depth and bad, then the gate entry behind the in_range branch), bit 1 -- a wait for the row stores in front of the output
// stores, bit 2 -- blockDim.x instead of the constant block size (kernels_qm_step1.hip)
// Round 7 (EXPERIMENTS.md): bit 3 -- the gate's arithmetic as the compiler makes it from selects and compares (and the "no gate" branch around the
// rows), bit 4 -- the tile base and the output addresses wherever the compiler computes them (and the gate entry's load behind its branch),
// bit 5 -- the kernel clock's record count fetched at the kernel's end (below, beside the pinned statement).  Bits 3 and 4 each undo two things that
// only work together -- the masks need the rows' wait in one block with their decode, the early addresses need the gate entry's load outside a
// branch -- so a variant measures the pair
#ifndef QG_STEP1_ABLATE
#define QG_STEP1_ABLATE 0
#endif

// The gate word decoded into full-word 0 / -1 masks, and the two qubits' rows moved through them with one instruction per select and per term:
// bit_select (v_bfi_b32 / v_bitop3_b32) and xor_and (v_bitop3_b32, device_common.hpp).  The masks depend on the gate entry alone: qm_step1_body
// computes them while the row loads fly.  Written with the builtins on purpose -- from plain mask arithmetic the compiler goes back to
// v_and -> v_cmp_ne -> v_cndmask -> v_xor per term, three to four instructions each, all behind the rows' arrival.
// An address that went through an integer or an `asm` operand has lost its address space: dereferenced as it is it becomes a flat_ instruction
// (slower, and counted with the scalar loads).  These put it back.
template <class T>
using global_ptr = __attribute__((address_space(1))) T *;
typedef uint32_t u32x4 __attribute__((ext_vector_type(4)));
__device__ inline uint4 global_load4(const uint4 *p) {
    const u32x4 v = *(global_ptr<const u32x4>)p;
    return make_uint4(v.x, v.y, v.z, v.w);
}
__device__ inline void global_store4(uint4 *p, const uint4 &v) { *(global_ptr<u32x4>)p = u32x4{v.x, v.y, v.z, v.w}; }
template <class T>
__device__ inline void global_store(uintptr_t at, T v) { *(global_ptr<T>)at = v; }

__device__ inline uint32_t gate_bit_mask(uint32_t ops, uint32_t bit) { return (uint32_t)__builtin_amdgcn_sbfe((int32_t)ops, bit, 1u); }  // v_bfe_i32
template <bool HAS_Z>
struct GateMasks {
    uint32_t m[16];   // m[4 k + i]: matrix bit M[k][i], in = {x0, z0, x1, z1}
    uint32_t o0, o1;  // the qubit's parity (HAS_Z: which half of its group; else bit 0 of its place among the group's four rows)
    uint32_t h0, h1;  // !HAS_Z: bit 1 of that place
    uint32_t same;    // both qubits in one group
    __device__ inline GateMasks(uint32_t ops, uint32_t g0, uint32_t g1) {
#pragma unroll
        for (uint32_t i = 0; i < 16; ++i) m[i] = gate_bit_mask(ops, 10u + i);
        o0 = gate_bit_mask(ops, 0u); o1 = gate_bit_mask(ops, 5u);
        h0 = HAS_Z ? 0u : gate_bit_mask(ops, 1u); h1 = HAS_Z ? 0u : gate_bit_mask(ops, 6u);
        same = 0u - (uint32_t)(g0 == g1);
    }
    __device__ inline void pin() {  // (compiler only: the masks are values in registers from here on, not expressions to be folded into their uses)
        asm volatile("" : "+v"(m[0]), "+v"(m[1]), "+v"(m[2]), "+v"(m[3]), "+v"(m[4]), "+v"(m[5]), "+v"(m[6]), "+v"(m[7]), "+v"(m[8]), "+v"(m[9]),
                          "+v"(m[10]), "+v"(m[11]), "+v"(m[12]), "+v"(m[13]), "+v"(m[14]), "+v"(m[15]));
        asm volatile("" : "+v"(o0), "+v"(o1), "+v"(h0), "+v"(h1), "+v"(same));
    }
    __device__ inline uint32_t get(const uint4 &u, uint32_t o, uint32_t h, uint32_t &z) const {
        if constexpr (HAS_Z) {  // {X[2g], Z[2g], X[2g+1], Z[2g+1]}
            z = bit_select(o, u.w, u.y);
            return bit_select(o, u.z, u.x);
        } else {                // rows 4g .. 4g+3
            z = 0u;
            return bit_select(h, bit_select(o, u.w, u.z), bit_select(o, u.y, u.x));
        }
    }
    __device__ inline uint32_t mix(uint32_t k, uint32_t x0, uint32_t z0, uint32_t x1, uint32_t z1) const {  // out_k = xor_i M[k][i] * in_i
        uint32_t o = m[4 * k] & x0;
        if constexpr (HAS_Z) o = xor_and(o, m[4 * k + 1], z0);
        o = xor_and(o, m[4 * k + 2], x1);
        if constexpr (HAS_Z) o = xor_and(o, m[4 * k + 3], z1);
        return o;
    }
};
// ... the put-back: `e` = the qubit's parity mask (HAS_Z) / its four place masks
template <bool HAS_Z>
__device__ inline void gate_put(uint4 &u, const uint32_t (&e)[4], uint32_t x, uint32_t z) {
    if constexpr (HAS_Z) {
        u.x = bit_select(e[0], u.x, x); u.y = bit_select(e[0], u.y, z);
        u.z = bit_select(e[0], x, u.z); u.w = bit_select(e[0], z, u.w);
    } else {
        u.x = bit_select(e[0], x, u.x); u.y = bit_select(e[1], x, u.y);
        u.z = bit_select(e[2], x, u.z); u.w = bit_select(e[3], x, u.w);
    }
}

// The env's action for the one-step kernels in two halves, so that no wait sits inside the width's branch: action_issue only chooses the load
// instruction (a uniform branch on a flag that sits in an SGPR), action_value extends the sign behind whatever the caller issues in between --
// those loads then fly with the action (load_action's i32 arm waits for its load inside the branch).  An int64 action keeps all 64 bits: one
// whose low half alone is in range stays out of range.
__device__ inline void action_issue(const void *actions, uint64_t idx, bool act64, int32_t &lo, int32_t &hi) {
    hi = 0;
    if (act64) {
        const int64_t v = reinterpret_cast<const int64_t *>(actions)[idx];
        lo = (int32_t)v;
        hi = (int32_t)(v >> 32);
    } else {
        lo = reinterpret_cast<const int32_t *>(actions)[idx];
    }
}
__device__ inline int64_t action_value(int32_t lo, int32_t hi, bool act64) {
    hi = act64 ? hi : lo >> 31;
    return (int64_t)(((uint64_t)(uint32_t)hi << 32) | (uint64_t)(uint32_t)lo);
}

// One env.step() of env `env`: gathers the gate's <= 2 row groups from the env's tile (G groups of
// 1 KiB), applies the gate's 4x4 GF(2) map, scatters, updates the incremental solved mask, depth, reward, done, success (and the
// solution log / layer metrics when FEAT).  Returns is_final.
// `act_in`: the env's action when the caller holds it in a register (the policy kernel), or null: load it from f.actions.
// The dependent memory round trips of a lane are four: {action, depth, bad} issued back to back, the action first -- the gate entry (unconditional,
// clamped index: an out-of-range action reads entry 0 and is given "no gate, penalty 0" afterwards, clifford.rs:324) needs the action alone; the
// <= 2 row groups; every store.  depth and bad are pinned where the gate entry is consumed: left alone the compiler sinks their first use below the
// row stores and waits there for ALL outstanding memory operations -- the output stores then leave only after the row stores have been acknowledged.
// D16 > 0 (qg_vec_track_dense; the matrix has D = 16 * D16 rows, no padding slots): the rows the gate rewrote also go to the env's
// dense int8 observation -- <= 4 rows of D bytes instead of the D * D bytes a full qg_vec_observe_dense writes.
// `alone`: the neighbouring lane does not run this body with the neighbouring env (the reset's lanes in qm_reset_step_kernel): the dense rows are
// then written by this lane alone.
// PLAIN_FRONT: the front and back as the compiler orders them by itself -- action, then depth and bad, then the gate entry behind the in_range branch,
// nothing pinned.  The policy kernel (mid_head_sample_kernel) keeps it: it holds the action in a register, sits at its register limit, and the
// pinned form costs two of its instantiations one VGPR more.
// PLAIN_BACK: the gate's arithmetic and the addresses as the compiler makes them from selects and compares, nothing computed ahead of its use
// (the body before round 7).  The mask form keeps ~25 more values in registers across the rows' wait: the fused reset+step kernels
// (qm_reset_step_kernel, whose reset workgroups share the SIMDs with these lanes) would drop from 7-8 waves per SIMD to 4-6 with it, so they keep this one.
template <bool HAS_Z, bool FEAT, int D16 = 0, bool PLAIN_FRONT = false, bool PLAIN_BACK = PLAIN_FRONT>
__device__ inline bool qm_step1_body(const Step1Front &f, const StepArgs &a, uint32_t G, uint64_t env, const int64_t *act_in, bool alone = false) {
    static_assert(PLAIN_BACK || !PLAIN_FRONT, "the mask arithmetic is placed against the pinned front");
    constexpr bool NEW_ALU = !PLAIN_BACK && !(QG_STEP1_ABLATE & 8), EARLY_ADDR = !PLAIN_BACK && !(QG_STEP1_ABLATE & (16 | 1));
    const uint32_t lane = (uint32_t)env & (QG_WAVE - 1);
    uint4 *tile = reinterpret_cast<uint4 *>(f.state) + (env >> 6) * (uint64_t)(G * 64);
    uint4 *tile_lane = tile + lane;  // EARLY_ADDR: the env's place in its tile, in registers before the gate entry is there
    auto group_at = [&](uint32_t grp) { return EARLY_ADDR ? tile_lane + grp * 64 : tile + (grp * 64 + lane); };
    // the addresses of the five per-env outputs (as integers: the two sequence arrays may be null)
    uintptr_t out_reward = 0, out_done = 0, out_success = 0, out_rseq = 0, out_dseq = 0;
    auto output_addresses = [&] {
        out_reward = reinterpret_cast<uintptr_t>(a.reward + env); out_done = reinterpret_cast<uintptr_t>(a.done + env);
        out_success = reinterpret_cast<uintptr_t>(a.success + env);
        out_rseq = reinterpret_cast<uintptr_t>(a.rewards_seq) + 4u * env; out_dseq = reinterpret_cast<uintptr_t>(a.dones_seq) + env;
    };
    int64_t act;
    int32_t depth, sol_n;
    uint32_t bad0;
    bool in_range;
    GateEntry g = GateEntry{QM_IDENTITY << 10, 0.0f};  // "no gate", penalty 0: what an out-of-range action selects (clifford.rs:324)
    if constexpr (PLAIN_FRONT) {
        act = act_in ? *act_in : load_action(f.actions, env, f.flags & F_ACT64);
        depth = f.depth[env];
        bad0 = f.bad[env];
        sol_n = (FEAT && (f.flags & F_TRACK)) ? a.sol_len[env * 2] : 0;
        in_range = act >= 0 && act < (int64_t)f.num_actions;  // gateset.get(action) (clifford.rs:324)
        if (in_range) g = f.gates[act];
    } else {
        int32_t act_lo = 0, act_hi = 0;
        if (!act_in) action_issue(f.actions, env, f.flags & F_ACT64, act_lo, act_hi);
#if QG_STEP1_ABLATE & 1  // the front in its old order
        act = act_in ? *act_in : action_value(act_lo, act_hi, f.flags & F_ACT64);
        __builtin_amdgcn_sched_barrier(0);
#endif
        depth = f.depth[env];
        bad0 = f.bad[env];
        sol_n = (FEAT && (f.flags & F_TRACK)) ? a.sol_len[env * 2] : 0;
#if QG_STEP1_ABLATE & 1
        asm volatile("" : "+v"(bad0));
        in_range = (uint64_t)act < (uint64_t)f.num_actions;
        if (in_range) g = f.gates[act];
#else
        // what depends on `env` alone is computed here, under these loads: the env's place in its tile now (`state` is a preloaded argument), the
        // output addresses under the gate entry's load below -- not between the gate entry's arrival and the row loads, or in front of the stores
        if constexpr (EARLY_ADDR) asm volatile("" : "+v"(tile_lane));
        __builtin_amdgcn_sched_barrier(0);  // (compiler only: the loads above are issued before anything uses the action -- the gate entry's load waits for it alone)
        act = act_in ? *act_in : action_value(act_lo, act_hi, f.flags & F_ACT64);
        in_range = (uint64_t)act < (uint64_t)f.num_actions;  // gateset.get(action) (clifford.rs:324): 0 <= act < num_actions
        if constexpr (EARLY_ADDR) {
            uint32_t gi = in_range ? (uint32_t)act : 0u;
            asm volatile("" : "+v"(gi));  // (compiler only: the load stays unconditional, in one block with what runs under it)
            const GateEntry entry = f.gates[gi];
            __builtin_amdgcn_sched_barrier(0);
            output_addresses();
            asm volatile("" : "+v"(out_reward), "+v"(out_done), "+v"(out_success), "+v"(out_rseq), "+v"(out_dseq));
            if (in_range) g = entry;
        } else {
            const GateEntry entry = f.gates[in_range ? act : 0];
            if (in_range) g = entry;
        }
#endif
        // the gate entry, depth and bad are all here: no later wait for a load.  The StepArgs fields the back of the chain reads are asked for here too:
        // their scalar loads are issued at the top, fly with the vector loads and have long arrived -- left alone the compiler fetches a field right
        // before its first use, a cold scalar line between the rows and the stores
        asm volatile("" : "+v"(g.ops), "+v"(g.penalty), "+v"(depth), "+v"(bad0)
                     : "s"(a.N), "s"(a.rewards_seq), "s"(a.dones_seq), "s"(a.reward), "s"(a.done), "s"(a.success));
#if !(QG_STEP1_ABLATE & 32)  // ... and the kernel clock's record count: left alone it is a cold scalar load, waited for, in every wave's last instructions
        if constexpr (!PLAIN_BACK) asm volatile("" : : "s"(a.kclk_waves));
#endif
        depth = depth > 0 ? depth - 1 : 0;  // clifford.rs:342
    }
    if constexpr (NEW_ALU && !EARLY_ADDR) output_addresses();
    uint32_t bad = bad0, fault = 0;
    float penalty = 0.0f, r_solved = 0.0f, r_open = 0.0f;
    uint32_t fin_open = 0;  // NEW_ALU: is_final of an env that is not solved
    uint32_t drow[4] = {0, 0, 0, 0}, dword[4] = {0, 0, 0, 0}, dchg = 0;  // D16: the rows the gate changed (bit k of dchg: entry k)
    if constexpr (NEW_ALU) {
        // No branch around the rows: "no gate" (an out-of-range action, a two-qubit gate on equal qubits) is the identity map on qubit 0 -- its rows are
        // rewritten as they are and `bad` keeps its bit (`live`) -- so the chain from the gate entry to the stores is one block.  Between the issue of
        // the row loads and their arrival: the masks, the identity patterns, the cleared `bad`.  Behind it: 4 selects, 16 terms, 12 merges (HAS_Z).
        penalty = g.penalty;  // (out of range: 0)
        const bool layered = FEAT && (f.flags & F_LAYERS) && in_range;
        LayerTxn lt;
        if (layered) lt = layers_begin(layer_rec(a.layers, env, 2 * a.N + 2), a.N, a.descs[act]);  // its loads fly with the state's
        constexpr uint32_t gsh = HAS_Z ? 1u : 2u;
        const uint32_t ops = g.ops, q0 = ops & 31u, q1 = (ops >> 5) & 31u, g0 = q0 >> gsh, g1 = q1 >> gsh;
        uint4 *pa = group_at(g0), *pb = group_at(g1);
        uint4 ua = global_load4(pa), ub = global_load4(pb);
        __builtin_amdgcn_sched_barrier(0);  // (compiler only: everything down to the next one stands between the loads and their wait)
        GateMasks<HAS_Z> gm(ops, g0, g1);
        uint32_t e0[4], e1[4];  // the put-back's masks: gate_put
#pragma unroll
        for (uint32_t k = 0; k < 4; ++k) {
            e0[k] = HAS_Z ? gm.o0 : 0u - (uint32_t)((q0 & 3u) == k);
            e1[k] = HAS_Z ? gm.o1 : 0u - (uint32_t)((q1 & 3u) == k);
        }
        const uint32_t live = 0u - (uint32_t)(((ops >> 10) & 0xFFFFu) != QM_IDENTITY);
        const uint32_t zb = 1u << a.N;
        uint32_t ix0 = 1u << q0, ix1 = 1u << q1, iz0 = zb << q0, iz1 = zb << q1;  // the identity's rows of the two qubits
        // `bad`: the two qubits' bits cleared here, set again behind the rows as min(difference, 1) << q -- no compare, no select.  "No gate" keeps
        // both bits (`live`); q0's value wins when q0 == q1, as below
        uint32_t set0 = live & 1u, set1 = set0 & (uint32_t)(q0 != q1);
        uint32_t bad_rest = bad0 & ~((set0 << q0) | (set1 << q1));
        r_solved = 1.0f - penalty; r_open = 0.0f - penalty;  // clifford.rs:345-346, both outcomes
        fin_open = (uint32_t)(depth == 0);
        const bool apart = g0 != g1;
        gm.pin();
        if constexpr (!HAS_Z) asm volatile("" : "+v"(e0[0]), "+v"(e0[1]), "+v"(e0[2]), "+v"(e0[3]), "+v"(e1[0]), "+v"(e1[1]), "+v"(e1[2]), "+v"(e1[3]));
        asm volatile("" : "+v"(ix0), "+v"(ix1), "+v"(iz0), "+v"(iz1), "+v"(set0), "+v"(set1), "+v"(bad_rest), "+v"(r_solved), "+v"(r_open),
                          "+v"(depth), "+v"(fin_open));
        __builtin_amdgcn_sched_barrier(0);
        uint32_t z0, z1;
        const uint32_t x0 = gm.get(ua, gm.o0, gm.h0, z0), x1 = gm.get(ub, gm.o1, gm.h1, z1);
        const uint32_t nx0 = gm.mix(0, x0, z0, x1, z1), nx1 = gm.mix(2, x0, z0, x1, z1);
        const uint32_t nz0 = HAS_Z ? gm.mix(1, x0, z0, x1, z1) : 0u, nz1 = HAS_Z ? gm.mix(3, x0, z0, x1, z1) : 0u;
        // q1's rows first, then q0's (q0's value wins when q0 == q1, as in qm_apply)
        gate_put<HAS_Z>(ub, e1, nx1, nz1);
        ua.x = bit_select(gm.same, ub.x, ua.x); ua.y = bit_select(gm.same, ub.y, ua.y);
        ua.z = bit_select(gm.same, ub.z, ua.z); ua.w = bit_select(gm.same, ub.w, ua.w);
        gate_put<HAS_Z>(ua, e0, nx0, nz0);
        // (one group: q0's store carries q1's rows too.  Storing them twice, to spare this branch, measured 0.17 us per step SLOWER at 65 536 envs:
        // 47 % of the line gateset's actions stay in one group, and the launch ends when its stores have drained -- EXPERIMENTS.md round 7)
        if (apart) global_store4(pb, ub);
        global_store4(pa, ua);
        if constexpr (D16 > 0) {  // the rows that changed: stored below ("no gate" changes none)
            drow[0] = q0; dword[0] = nx0; dchg |= (uint32_t)(nx0 != x0);
            drow[1] = a.N + q0; dword[1] = nz0; dchg |= (uint32_t)(HAS_Z && nz0 != z0) << 1;
            drow[2] = q1; dword[2] = nx1; dchg |= (uint32_t)(q1 != q0 && nx1 != x1) << 2;
            drow[3] = a.N + q1; dword[3] = nz1; dchg |= (uint32_t)(HAS_Z && q1 != q0 && nz1 != z1) << 3;
        }
        const uint32_t d0 = HAS_Z ? xor_or(nx0, ix0, nz0 ^ iz0) : nx0 ^ ix0, d1 = HAS_Z ? xor_or(nx1, ix1, nz1 ^ iz1) : nx1 ^ ix1;
        bad = bad_rest | (min(d0, set0) << q0) | (min(d1, set1) << q1);
        if (layered) {
            penalty = layers_commit(lt, a.w);
            r_solved = 1.0f - penalty; r_open = 0.0f - penalty;
        }
    } else if (in_range) {
        penalty = g.penalty;
        const bool layered = FEAT && (f.flags & F_LAYERS);
        LayerTxn lt;
        if (layered) lt = layers_begin(layer_rec(a.layers, env, 2 * a.N + 2), a.N, a.descs[act]);  // its loads fly with the state's
        const uint32_t q0 = g.ops & 31u, q1 = (g.ops >> 5) & 31u, m = (g.ops >> 10) & 0xFFFFu;
        if (m != QM_IDENTITY) {  // "no gate" (e.g. a two-qubit gate on equal qubits) changes nothing
            constexpr uint32_t gsh = HAS_Z ? 1u : 2u;
            const uint32_t g0 = q0 >> gsh, g1 = q1 >> gsh;
            const uint4 va = EARLY_ADDR ? global_load4(group_at(g0)) : tile[g0 * 64 + lane], vb = EARLY_ADDR ? global_load4(group_at(g1)) : tile[g1 * 64 + lane];
            uint32_t ua[4] = {va.x, va.y, va.z, va.w}, ub[4] = {vb.x, vb.y, vb.z, vb.w};
            uint32_t x0, z0, x1, z1;
            qm_group_get<HAS_Z>(ua, q0, x0, z0);
            qm_group_get<HAS_Z>(ub, q1, x1, z1);
            auto mix = [&](uint32_t k) -> uint32_t {  // out_k = xor_i M[k][i] * in_i
                const uint32_t b = m >> (4 * k);
                uint32_t o = ((0u - (b & 1u)) & x0) ^ ((0u - ((b >> 2) & 1u)) & x1);
                if (HAS_Z) o ^= ((0u - ((b >> 1) & 1u)) & z0) ^ ((0u - ((b >> 3) & 1u)) & z1);
                return o;
            };
            const uint32_t nx0 = mix(0), nx1 = mix(2), nz0 = HAS_Z ? mix(1) : 0u, nz1 = HAS_Z ? mix(3) : 0u;
            // q1's rows first, then q0's (q0's value wins when q0 == q1, as in qm_apply)
            qm_group_put<HAS_Z>(ub, q1, nx1, nz1);
            const bool same = g0 == g1;
#pragma unroll
            for (int k = 0; k < 4; ++k) ua[k] = same ? ub[k] : ua[k];
            qm_group_put<HAS_Z>(ua, q0, nx0, nz0);
            if constexpr (EARLY_ADDR) {
                if (!same) global_store4(group_at(g1), make_uint4(ub[0], ub[1], ub[2], ub[3]));
                global_store4(group_at(g0), make_uint4(ua[0], ua[1], ua[2], ua[3]));
            } else {
                if (!same) tile[g1 * 64 + lane] = make_uint4(ub[0], ub[1], ub[2], ub[3]);
                tile[g0 * 64 + lane] = make_uint4(ua[0], ua[1], ua[2], ua[3]);
            }
            if constexpr (D16 > 0) {  // the rows that changed (S rewrites one of a qubit's two rows, CX two of four, ...): stored below
                drow[0] = q0; dword[0] = nx0; dchg |= (uint32_t)(nx0 != x0);
                drow[1] = a.N + q0; dword[1] = nz0; dchg |= (uint32_t)(HAS_Z && nz0 != z0) << 1;
                drow[2] = q1; dword[2] = nx1; dchg |= (uint32_t)(q1 != q0 && nx1 != x1) << 2;
                drow[3] = a.N + q1; dword[3] = nz1; dchg |= (uint32_t)(HAS_Z && q1 != q0 && nz1 != z1) << 3;
            }
            const uint32_t zb = 1u << a.N;
            const uint32_t b1 = (uint32_t)(nx1 != (1u << q1) || (HAS_Z && nz1 != (zb << q1)));
            const uint32_t b0 = (uint32_t)(nx0 != (1u << q0) || (HAS_Z && nz0 != (zb << q0)));
            bad = (bad & ~(1u << q1)) | (b1 << q1);
            bad = (bad & ~(1u << q0)) | (b0 << q0);
        }
        if (layered) penalty = layers_commit(lt, a.w);
    }
    // qg_vec_track_dense: matrix row r, column c of env e at dense[(e * D + r) * D + c] (clifford.rs:361-368, adapters.py:50-54)
    if constexpr (D16 == 2) {
        // The two lanes of a pair (2k, 2k + 1: neighbouring envs) write one 32-byte row together, 16 bytes each, so that a store
        // instruction's lanes cover whole rows: per-lane rows (two 16-byte stores 16 bytes apart from ONE lane) measured 5.28 us per step at
        // 65 536 envs, this form 4.83 (3.11 without the dense observation).  Every lane that runs this body reaches this point; a pair lane
        // that does not (past the batch's odd end) reads as "no row" -- update_dpp keeps `old` = 0 for a disabled source lane -- and the
        // env it leaves without a partner writes its rows alone.
        const bool solo = alone || (env ^ 1ull) >= f.B;
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            if (solo && ((dchg >> k) & 1u)) dense_row_store<2>(a.dense, env, drow[k], dword[k]);
            const uint32_t mine = (!solo && ((dchg >> k) & 1u)) ? (drow[k] | 0x80000000u) : 0u;
#pragma unroll
            for (int par = 0; par < 2; ++par) {  // quad_perm [0, 0, 2, 2] / [1, 1, 3, 3]: the even / odd lane's entry on both lanes of the pair
                const uint32_t r = par ? (uint32_t)__builtin_amdgcn_update_dpp(0, (int)mine, 0xF5, 0xF, 0xF, false)
                                       : (uint32_t)__builtin_amdgcn_update_dpp(0, (int)mine, 0xA0, 0xF, 0xF, false);
                const uint32_t w = par ? (uint32_t)__builtin_amdgcn_update_dpp(0, (int)dword[k], 0xF5, 0xF, 0xF, false)
                                       : (uint32_t)__builtin_amdgcn_update_dpp(0, (int)dword[k], 0xA0, 0xF, 0xF, false);
                const uint64_t e = (env & ~1ull) | (uint64_t)par;
                const uint32_t half = lane & 1u;
                if (r >> 31) *reinterpret_cast<uint4 *>(a.dense + (e * 32u + (r & 31u)) * 32u + 16u * half) = expand16_i8(w >> (16u * half));
            }
        }
    } else if constexpr (D16 == 1) {  // 16-byte rows: one store each
#pragma unroll
        for (int k = 0; k < 4; ++k)
            if ((dchg >> k) & 1u) dense_row_store<1>(a.dense, env, drow[k], dword[k]);
    }
    if (FEAT && (f.flags & F_TRACK)) {  // clifford.rs:334-340
        if ((uint32_t)sol_n < a.sol_cap) sol_at(a, env, (uint32_t)sol_n++) = sol_word_framed(act, false);
        else fault |= 8u;
    }
#if QG_STEP1_ABLATE & 2  // the wait that stood between the row stores and the output stores
    if constexpr (!PLAIN_FRONT) asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
#endif
    if constexpr (PLAIN_FRONT) depth = depth > 0 ? depth - 1 : 0;  // clifford.rs:342
    const bool solved = bad == 0;       // clifford.rs:344
    const float achieved = solved ? 1.0f : 0.0f;
    if constexpr (NEW_ALU || EARLY_ADDR) {
        const float reward = NEW_ALU ? (solved ? r_solved : r_open) : achieved - penalty;  // clifford.rs:345-346
        const uint32_t fin = NEW_ALU ? (solved ? 1u : fin_open) : (uint32_t)(depth == 0 || solved);  // is_final (clifford.rs:353)
        if (a.rewards_seq) global_store(out_rseq, reward);
        if (a.dones_seq) global_store(out_dseq, (uint8_t)fin);
        if (bad != bad0) f.bad[env] = bad;
        f.depth[env] = depth;
        global_store(out_reward, reward);
        global_store(out_done, (uint8_t)fin);
        global_store(out_success, (uint8_t)solved);
        if (FEAT && (f.flags & F_TRACK)) a.sol_len[env * 2] = sol_n;
        if (FEAT && fault) atomicOr(&a.error[env], fault);
        return fin != 0;
    } else {
        const float reward = achieved - penalty;  // clifford.rs:345-346
        if (a.rewards_seq) a.rewards_seq[env] = reward;
        if (a.dones_seq) a.dones_seq[env] = (uint8_t)(depth == 0 || solved);
        if (bad != bad0) f.bad[env] = bad;
        f.depth[env] = depth;
        a.reward[env] = reward;
        a.done[env] = (uint8_t)(depth == 0 || solved);  // is_final (clifford.rs:353)
        a.success[env] = (uint8_t)solved;
        if (FEAT && (f.flags & F_TRACK)) a.sol_len[env * 2] = sol_n;
        if (FEAT && fault) atomicOr(&a.error[env], fault);
        return depth == 0 || solved;
    }
}
// ... for the policy kernel: the action in a register, the front from its StepArgs, the body's order left to the compiler
template <bool HAS_Z, bool FEAT, int D16 = 0>
__device__ inline bool qm_step1_body(const StepArgs &a, uint32_t G, uint64_t env, int64_t act, bool alone = false) {
    return qm_step1_body<HAS_Z, FEAT, D16, true>(step1_front(a), a, G, env, &act, alone);
}


// qg_vec_track_dense with add_inverts (N = 16): the envs of this wave whose matrix was inverted in this step, one after the other -- every lane
// writes its 16 bytes of the env's contiguous 1 KiB from the rows qm_inv2_body parked in `dense_lds` ([env of the wave][row], pitch 33).
// Call from all 64 lanes; `env0` = the wave's first env, `whole` false on lanes without an env.
__device__ inline void qm_inv2_dense_flush(int8_t *dense, const uint32_t *dense_lds, uint64_t env0, bool whole) {
    const uint32_t lane = threadIdx.x & (QG_WAVE - 1);
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
    __builtin_amdgcn_wave_barrier();
    uint64_t todo = __ballot(whole && !(lane & 1u));  // bit 2 * slot per inverted env of this wave
    while (todo) {  // wave-uniform
        const uint32_t sl = ((uint32_t)__ffsll((long long)todo) - 1u) >> 1;
        todo &= todo - 1ull;
        const uint32_t w = dense_lds[sl * 33u + (lane >> 1)];
        reinterpret_cast<uint4 *>(dense + (env0 + sl) * 1024u)[lane] = expand16_i8(w >> (16u * (lane & 1u)));
    }
}

// ---- the reference-default step of CliffordEnv N <= 16 (add_inverts), two lanes per env: see kernels_qm.hip for the discussion ----
#define QM_FLAG_INVERTED 1u
#define QM_FLAG_SYMPLECTIC 2u

// Balanced select tree: each level blends pairs with an all-ones/all-zeros lane mask, (hi & m) | (lo & ~m) = one v_bfi_b32; written
// as bit arithmetic on purpose: a `b ? t[2k+1] : t[2k]` select gets folded by the compiler into a runtime-indexed (scratch) array read.
template <int n>
__device__ inline uint32_t tree_select(const uint32_t (&t)[n], uint32_t q) {
    if constexpr (n == 1) {
        return t[0];
    } else {
        constexpr int m = (n + 1) / 2;
        uint32_t u[m];
        const uint32_t mb = 0u - (q & 1u);
#pragma unroll
        for (int k = 0; k < m; ++k) u[k] = (2 * k + 1 < n) ? ((t[2 * k + 1] & mb) | (t[2 * k] & ~mb)) : t[2 * k];
        return tree_select<m>(u, q >> 1);
    }
}

__device__ inline uint32_t qm_pair_swap(uint32_t v) {  // the partner lane's value (lanes 2e, 2e+1): DPP quad_perm [1, 0, 3, 2]
    return (uint32_t)__builtin_amdgcn_update_dpp(0, (int)v, 0xB1, 0xF, 0xF, false);
}

// GS: the env's 16-byte groups (two qubits each) as a compile-time constant, or 0: `groups` at run time (the policy kernel).
// `env`, `h`: this lane's env and half (lanes 2e, 2e + 1 of a wave hold env e); `act`: the env's action, or null: load it from a.actions.
// Returns is_final (on both lanes).
// DENSE (qg_vec_track_dense, N = 16): `dense_lds` = 32 x 33 words of LDS owned by this wave; the env's dense int8 observation follows the step --
// the whole 1 KiB when the coin inverted the matrix (the wave's inverted envs one after the other, every lane 16 bytes of a contiguous 1 KiB),
// else the rows of the gate's qubits.
// The whole-env part needs all 64 lanes of the wave: the body only parks the rows (and reports `whole`), the kernel calls qm_inv2_dense_flush
// from EVERY lane afterwards, the ones past the batch's end included.
template <int GS, bool FEAT, bool DENSE = false>
__device__ inline bool qm_inv2_body(const StepArgs &a, uint32_t groups, uint64_t env, uint32_t h, const int64_t *act_in, uint32_t *dense_lds = nullptr,
                                    bool *dense_whole = nullptr) {
    const int G = GS ? GS : (int)groups;
    const uint32_t N = a.N;
    uint4 *tile = reinterpret_cast<uint4 *>(a.state) + (env >> 6) * (uint64_t)(G * 64) + (env & 63u);
    // every load that does not depend on another one is issued here, the rows first (the longest transfers), so that the whole
    // kernel pays two memory round trips: this batch, and the gate entry behind the action
    uint4 grp[4];
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        grp[k] = make_uint4(0u, 0u, 0u, 0u);
        if (k < G && (h == 0 || k + 4 < G)) grp[k] = tile[(uint32_t)(4 * h + k) * 64u];
    }
    int32_t depth = a.depth[env];
    uint32_t iflags = a.inverted[env];
    uint32_t coin = a.coins ? a.coins[env] : 0u;
    int32_t sol_n = (FEAT && (a.flags & F_TRACK)) ? a.sol_len[env * 2] : 0;
    int32_t sol_b = (FEAT && (a.flags & F_TRACK)) ? a.sol_len[env * 2 + 1] : 0;
    const int64_t act = act_in ? *act_in : load_action(a.actions, env, a.flags & F_ACT64);
    const bool in_range = act >= 0 && act < (int64_t)a.num_actions;  // gateset.get(action) (clifford.rs:324)
    GateEntry g = a.gates[in_range ? act : 0];  // unconditional (clamped) load: nothing else waits behind a branch
    if (!in_range) g = GateEntry{QM_IDENTITY << 10, 0.0f};
    if (!a.coins) coin = (uint32_t)(rng_draw(a.seed ^ 0x636F696Eull, a.env_base + env, step_clock(a)) >> 63);  // runs under the loads
    // this lane's 8 qubits: xs[j] = X row of qubit 8h + j, zs[j] = its Z row (stored words: bit c = logical column c)
    uint32_t xs[8], zs[8];
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        xs[2 * k] = grp[k].x; zs[2 * k] = grp[k].y; xs[2 * k + 1] = grp[k].z; zs[2 * k + 1] = grp[k].w;
    }
    uint32_t fault = 0;
    float penalty = g.penalty;
    if (FEAT && (a.flags & F_LAYERS) && in_range && h == 0) penalty = layers_penalty(layer_rec(a.layers, env, 2 * N + 2), N, a.descs[act], a.w);

    // ---- apply_gate_to_state (clifford.rs:331): the 4x4 GF(2) map on {X[q0], Z[q0], X[q1], Z[q1]} --------------------------
    uint32_t dirty = 0;  // this lane's groups that changed (bit k: group 4h + k)
    const uint32_t q0 = g.ops & 31u, q1 = (g.ops >> 5) & 31u, m = (g.ops >> 10) & 0xFFFFu;
    const bool own0 = (q0 >> 3) == h, own1 = (q1 >> 3) == h;
    {
        uint32_t x0 = own0 ? tree_select<8>(xs, q0 & 7u) : 0u, z0 = own0 ? tree_select<8>(zs, q0 & 7u) : 0u;
        uint32_t x1 = own1 ? tree_select<8>(xs, q1 & 7u) : 0u, z1 = own1 ? tree_select<8>(zs, q1 & 7u) : 0u;
        x0 |= qm_pair_swap(x0); z0 |= qm_pair_swap(z0);  // the lane that does not own the qubit contributes zero
        x1 |= qm_pair_swap(x1); z1 |= qm_pair_swap(z1);
        auto mix = [&](uint32_t k) -> uint32_t {  // out_k = xor_i M[k][i] * in_i
            const uint32_t b = m >> (4 * k);
            return ((0u - (b & 1u)) & x0) ^ ((0u - ((b >> 1) & 1u)) & z0) ^ ((0u - ((b >> 2) & 1u)) & x1) ^ ((0u - ((b >> 3) & 1u)) & z1);
        };
        const uint32_t nx0 = mix(0), nz0 = mix(1), nx1 = mix(2), nz1 = mix(3);
        if (m != QM_IDENTITY) {
#pragma unroll
            for (int j = 0; j < 8; ++j) {  // q1's rows first, then q0's (q0's value wins when q0 == q1, as in qm_apply)
                const bool h1 = own1 && (q1 & 7u) == (uint32_t)j, h0 = own0 && (q0 & 7u) == (uint32_t)j;
                uint32_t vx = xs[j], vz = zs[j];
                vx = h1 ? nx1 : vx; vz = h1 ? nz1 : vz;
                vx = h0 ? nx0 : vx; vz = h0 ? nz0 : vz;
                xs[j] = vx; zs[j] = vz;
            }
            if (own0) dirty |= 1u << ((q0 & 7u) >> 1);
            if (own1) dirty |= 1u << ((q1 & 7u) >> 1);
        }
    }

    if (FEAT && (a.flags & F_TRACK) && h == 0) {  // clifford.rs:334-340: entries in push order, bit 31 = pushed to solution_inv
        if ((uint32_t)(sol_n + sol_b) < a.sol_cap) {
            const bool inv_frame = iflags & QM_FLAG_INVERTED;
            sol_at(a, env, (uint32_t)(sol_n + sol_b)) = sol_word_framed(act, inv_frame);
            if (inv_frame) ++sol_b;
            else ++sol_n;
        } else {
            fault |= 8u;
        }
    }
    depth = depth > 0 ? depth - 1 : 0;  // clifford.rs:342

    // ---- maybe_random_invert (clifford.rs:262-270) ----------------------------------------------------------------------------
    if (coin & 1u) {  // both lanes of a pair take the same branch
        if (iflags & QM_FLAG_SYMPLECTIC) {
            uint32_t w[16];  // local index i = 8 t + j  <->  v = 16 t + 8 h + j
            const uint32_t xm = N >= 16 ? 0xFFFFu : ((1u << N) - 1u);
#pragma unroll
            for (int j = 0; j < 8; ++j) {
                w[j] = xs[j];
                w[8 + j] = zs[j];
            }
            if (N < 16) {  // logical Z columns N .. 2N-1 move to bit positions 16 .. 16+N-1
#pragma unroll
                for (int i = 0; i < 16; ++i) w[i] = (w[i] & xm) | (((w[i] >> N) & xm) << 16);
            }
            // stages 4, 2, 1: word pairs (i, i + d) of this lane
#pragma unroll
            for (int st = 0; st < 3; ++st) {
                const int d = 4 >> st;
                const uint32_t mlo = st == 0 ? 0x0F0F0F0Fu : st == 1 ? 0x33333333u : 0x55555555u;
#pragma unroll
                for (int i = 0; i < 16; ++i) {
                    if ((i & d) == 0) {
                        const uint32_t lo = w[i], hi = w[i + d];
                        w[i] = (lo & mlo) | ((hi & mlo) << d);
                        w[i + d] = ((lo >> d) & mlo) | (hi & ~mlo);
                    }
                }
            }
            // stage 8: the partner lane holds the other word of every pair; byte 1 / 3 of the low word <-> byte 0 / 2 of the high word
            const uint32_t sel8 = h ? 0x03070105u : 0x06020400u;
#pragma unroll
            for (int i = 0; i < 16; ++i) w[i] = __builtin_amdgcn_perm(qm_pair_swap(w[i]), w[i], sel8);
            // stage 16 + Omega: inv[v] = rot16(T[v ^ 16])
#pragma unroll
            for (int j = 0; j < 8; ++j) {
                const uint32_t lo = w[j], hi = w[8 + j];
                w[j] = __builtin_amdgcn_perm(hi, lo, 0x03020706u);      // {hi.hi16, lo.hi16}
                w[8 + j] = __builtin_amdgcn_perm(hi, lo, 0x01000504u);  // {hi.lo16, lo.lo16}
            }
            if (N < 16) {
#pragma unroll
                for (int i = 0; i < 16; ++i) w[i] = (w[i] & xm) | (((w[i] >> 16) & xm) << N);
            }
#pragma unroll
            for (int j = 0; j < 8; ++j) {
                xs[j] = w[j];
                zs[j] = w[8 + j];
            }
            iflags ^= QM_FLAG_INVERTED;
            dirty = 0xFu;
        } else {
            fault |= QG_FAULT_BAD_STATE;  // unreachable: the host launches the Gauss-Jordan variant whenever such an env may exist
        }
    }

    // ---- solved (clifford.rs:344), reward (:345-346) ----------------------------------------------------------------------------
    uint32_t diff = 0;
#pragma unroll
    for (int j = 0; j < 8; ++j) {
        const uint32_t q = 8u * h + (uint32_t)j;
        const bool real = q < N;
        diff |= xs[j] ^ (real ? 1u << q : 0u);
        diff |= zs[j] ^ (real ? (1u << N) << q : 0u);
    }
    diff |= qm_pair_swap(diff);
    const bool solved = diff == 0;
    const float achieved = solved ? 1.0f : 0.0f;
    const float reward = achieved - penalty;

#pragma unroll
    for (int k = 0; k < 4; ++k)
        if (((dirty >> k) & 1u) && k < G && (h == 0 || k + 4 < G))
            tile[(uint32_t)(4 * h + k) * 64u] = make_uint4(xs[2 * k], zs[2 * k], xs[2 * k + 1], zs[2 * k + 1]);
    if constexpr (DENSE) {  // N = 16: matrix row r of env e at dense[(e * 32 + r) * 32] (clifford.rs:361-368, adapters.py:50-54)
        const uint32_t lane = threadIdx.x & (QG_WAVE - 1), slot = lane >> 1;
        const bool whole = dirty == 0xFu;  // the inversion rewrote every row (both lanes of the pair agree)
        if (whole) {
#pragma unroll
            for (int j = 0; j < 8; ++j) {
                dense_lds[slot * 33u + 8u * h + (uint32_t)j] = xs[j];
                dense_lds[slot * 33u + 16u + 8u * h + (uint32_t)j] = zs[j];
            }
        }
        *dense_whole = whole;
        if (!whole && m != QM_IDENTITY) {  // the gate's rows only (this lane's share of them)
            if (own0) {
                dense_row_store<2>(a.dense, env, q0, tree_select<8>(xs, q0 & 7u));
                dense_row_store<2>(a.dense, env, 16u + q0, tree_select<8>(zs, q0 & 7u));
            }
            if (own1 && q1 != q0) {
                dense_row_store<2>(a.dense, env, q1, tree_select<8>(xs, q1 & 7u));
                dense_row_store<2>(a.dense, env, 16u + q1, tree_select<8>(zs, q1 & 7u));
            }
        }
    }
    if (h == 0) {
        if (a.rewards_seq) a.rewards_seq[env] = reward;
        if (a.dones_seq) a.dones_seq[env] = (uint8_t)(depth == 0 || solved);
        a.depth[env] = depth;
        a.reward[env] = reward;
        a.done[env] = (uint8_t)(depth == 0 || solved);  // is_final (clifford.rs:353)
        a.success[env] = (uint8_t)solved;
        if (FEAT && (a.flags & F_TRACK)) {
            a.sol_len[env * 2] = sol_n;
            a.sol_len[env * 2 + 1] = sol_b;
        }
        a.inverted[env] = (uint8_t)iflags;
        if (fault) atomicOr(&a.error[env], fault);
    }
    return depth == 0 || solved;
}

}  // namespace qg
