// qm_step1.hpp -- one env.step() of the TILE layout (CliffordEnv N <= 16, LinearFunctionEnv 8 < N <= 32, no add_inverts), one lane per env, in its
// forms: qm_step1_mask_body for qm_step1_kernel (kernels_qm_step1.hip), qm_step1_straight_body for qm_step1_straight_kernel (the same file: the mask body
// without the choices the host has made before the launch), qm_step1_plain_body for the step lanes of qm_reset_step_kernel (kernels_qm.hip)
// and for the policy kernel that samples an action and steps its env in the same launch (mid_head_sample_kernel, kernels_policy.hip).
// Reference: Clifford::step rust/src/envs/clifford.rs:321-347.
// The two bodies share no arithmetic on purpose: with helper lambdas in common five instantiations moved by one VGPR and one took 20 B of scratch
// (EXPERIMENTS.md round 7).  That holds for the parts that read alike too -- the tracked-dense tail, the solution-log push, the plain `mix`: each of
// them, made one function, changes the code of some instantiation (profiles/r08/CODEGEN.md), so each body writes them out.
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

// The gate word decoded into full-word 0 / -1 masks, and the two qubits' rows moved through them with one instruction per select and per term:
// bit_select (v_bfi_b32 / v_bitop3_b32) and xor_and (v_bitop3_b32, device_common.hpp).  The masks depend on the gate entry alone: qm_step1_mask_body
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

// One env.step() of env `env`, as qm_step1_kernel runs it: gathers the gate's <= 2 row groups from the env's tile (G groups of 1 KiB), applies the
// gate's 4x4 GF(2) map, scatters, updates the incremental solved mask, depth, reward, done, success (and the solution log / layer metrics when
// FEAT).  Returns is_final.
// D16 > 0 (qg_vec_track_dense; the matrix has D = 16 * D16 rows, no padding slots): the rows the gate rewrote also go to the env's
// dense int8 observation -- <= 4 rows of D bytes instead of the D * D bytes a full qg_vec_observe_dense writes.
// The dependent memory round trips of a lane are four: {action, depth, bad, done, success} issued back to back, the action first -- the gate entry (unconditional,
// clamped index: an out-of-range action reads entry 0 and is given "no gate, penalty 0" afterwards, clifford.rs:324) needs the action alone; the
// <= 2 row groups; every store.  Three where the wave holds the gates' group bytes across its lanes (F_GROUP_LANES, below): the row loads then leave behind a
// permute, and the gate entry flies beside them.  depth and bad are pinned where the gate entry is consumed: left alone the compiler sinks their first use below the
// row stores and waits there for ALL outstanding memory operations -- the output stores then leave only after the row stores have been acknowledged.
// Between those waits a lone wave pays every instruction, so the gate's arithmetic runs on lane masks (GateMasks) decoded while the row loads fly,
// and what depends on `env` alone is computed under the earlier loads.  Everything here depends on statement order.
template <bool HAS_Z, bool FEAT, int D16>
__device__ inline bool qm_step1_mask_body(const Step1Front &f, const StepArgs &a, uint32_t G, uint64_t env, uint64_t wave_envs) {
    const uint32_t lane = (uint32_t)env & (QG_WAVE - 1);
    uint4 *tile = reinterpret_cast<uint4 *>(f.state) + (env >> 6) * (uint64_t)(G * 64);
    uint4 *tile_lane = tile + lane;  // the env's place in its tile, in registers before the gate entry is there
    int32_t act_lo = 0, act_hi = 0;
    action_issue(f.actions, env, f.flags & F_ACT64, act_lo, act_hi);
    // Whether this wave takes the gate's groups across its lanes (below): the flag, and all 64 lanes with an env.  One SGPR, one uniform branch.
    uint32_t group_lanes = ((uint32_t)__builtin_popcountll(wave_envs) >> 6) & (f.flags / F_GROUP_LANES);
    asm volatile("" : "+s"(group_lanes));
    // ... then the group bytes of four actions, lane j holding those of actions 4 j .. 4 j + 3 (the table lies behind the gate table: gate_group_bytes,
    // qgym_plan.hpp; 64 dwords whatever num_actions is, so every lane's load is in bounds): with the first trip, from an address that depends on the lane alone
    // (by every wave, also one that does not use it: the load under the branch measured 0.03 us per step slower at 65 536 envs)
    const uint32_t gtab = reinterpret_cast<const uint32_t *>(f.gates + f.num_actions)[lane];
    int32_t depth0 = f.depth[env];
    uint32_t bad0 = f.bad[env];
    // done and success as memory holds them (a caller may have written either): the stores below leave only where the step changes them.  Two
    // byte loads behind the action, 64 B per wave each; they arrive ahead of the gate entry, so no wait is theirs.  Their addresses come from
    // StepArgs, not from the preloaded arguments: (compiler only) the barrier keeps that scalar wait behind the issue of depth and bad
    __builtin_amdgcn_sched_barrier(0);
    uint32_t done0 = a.done[env], success0 = a.success[env];
    int32_t sol_n = (FEAT && (f.flags & F_TRACK)) ? a.sol_len[env * 2] : 0;
    // what depends on `env` alone is computed here, under these loads: the env's place in its tile now (`state` is a preloaded argument), the
    // output addresses under the row loads below -- not between the action's arrival and the row loads, or in front of the stores
    asm volatile("" : "+v"(tile_lane));
    // (the StepArgs fields the rest of the chain reads are asked for here, with done's and success's: one batch of scalar loads, one wait -- none of
    // their cold lines is fetched behind the action's arrival)
    asm volatile("" : : "s"(a.N), "s"(a.rewards_seq), "s"(a.dones_seq), "s"(a.reward), "s"(a.kclk_waves));
    __builtin_amdgcn_sched_barrier(0);  // (compiler only: the loads above are issued before anything uses the action -- the gate entry's load waits for it alone)
    const int64_t act = action_value(act_lo, act_hi, f.flags & F_ACT64);
    const bool in_range = (uint64_t)act < (uint64_t)f.num_actions;  // gateset.get(action) (clifford.rs:324): 0 <= act < num_actions
    uint32_t gi = in_range ? (uint32_t)act : 0u;
    asm volatile("" : "+v"(gi));  // (compiler only: the load stays unconditional, in one block with what runs under it)
    const GateEntry entry = f.gates[gi];
    __builtin_amdgcn_sched_barrier(0);
    // The row loads need the gate's two groups and nothing else of its entry.  Where the wave holds the group bytes across its lanes (F_GROUP_LANES:
    // num_actions <= 256, and every lane of the wave live -- a lane past the batch's end has not loaded its dword, and a permute reads 0 from a lane
    // that is switched off) one ds_bpermute_b32 by act >> 2 and two v_bfe give them ~100 cycles behind the action: the gate entry's load flies beside
    // the row loads, not in front of them.  Otherwise (a uniform branch) the groups come from the entry, behind its wait, as before round 10.
    constexpr uint32_t gsh = HAS_Z ? 1u : 2u;
    uint32_t g0, g1;
    if (__builtin_expect(group_lanes != 0u, 1)) {
        uint32_t gb = (uint32_t)__builtin_amdgcn_ds_bpermute((int)(gi & ~3u), (int)gtab);
        gb = in_range ? gb : 0u;  // out of range: "no gate" on qubit 0, groups 0 / 0
        const uint32_t sh = (gi << 3) & 24u;
        g0 = __builtin_amdgcn_ubfe(gb, sh, 4u); g1 = __builtin_amdgcn_ubfe(gb, sh + 4u, 4u);
    } else {
        // (compiler only: a value of its own -- written as the select below, that select and the gate entry's wait are hoisted in front of this branch)
        uint32_t ops_e = entry.ops;
        asm volatile("" : "+v"(ops_e));
        ops_e = in_range ? ops_e : 0u;
        g0 = (ops_e & 31u) >> gsh; g1 = ((ops_e >> 5) & 31u) >> gsh;
    }
    uint4 *pa = tile_lane + g0 * 64, *pb = tile_lane + g1 * 64;
    // (both groups by every lane, also where they are one: the second load under the execution mask of the lanes with two groups -- no request
    // from the others, which then take `ub` from `ua` behind the wait -- measured 0.09 us per step SLOWER at 65 536 envs: six instructions more in
    // front of the second load, four selects behind the wait, one wait for both groups.  EXPERIMENTS.md round 9)
    uint4 ua = global_load4(pa), ub = global_load4(pb);
    __builtin_amdgcn_sched_barrier(0);  // (compiler only: everything down to the next one stands between the loads and their wait)
    // the addresses of the five per-env outputs (as integers: the two sequence arrays may be null)
    uintptr_t out_reward = reinterpret_cast<uintptr_t>(a.reward + env), out_done = reinterpret_cast<uintptr_t>(a.done + env);
    uintptr_t out_success = reinterpret_cast<uintptr_t>(a.success + env);
    uintptr_t out_rseq = reinterpret_cast<uintptr_t>(a.rewards_seq) + 4u * env, out_dseq = reinterpret_cast<uintptr_t>(a.dones_seq) + env;
    asm volatile("" : "+v"(out_reward), "+v"(out_done), "+v"(out_success), "+v"(out_rseq), "+v"(out_dseq));
    GateEntry g = GateEntry{QM_IDENTITY << 10, 0.0f};  // "no gate", penalty 0: what an out-of-range action selects (clifford.rs:324)
    if (in_range) g = entry;
    // the gate entry, depth and bad are all here: no later wait for a load.  The StepArgs fields the back of the chain reads are asked for here too:
    // their scalar loads are issued at the top, fly with the vector loads and have long arrived -- left alone the compiler fetches a field right
    // before its first use, a cold scalar line between the rows and the stores
    asm volatile("" : "+v"(g.ops), "+v"(g.penalty), "+v"(depth0), "+v"(bad0)
                 : "s"(a.N), "s"(a.rewards_seq), "s"(a.dones_seq), "s"(a.reward), "s"(a.done), "s"(a.success));
    asm volatile("" : "+v"(done0), "+v"(success0));  // ... and the two old bytes, pinned here with depth and bad: their first use is behind the row stores
    asm volatile("" : : "s"(a.kclk_waves));  // ... and the kernel clock's record count: left alone a cold scalar load, waited for, in every wave's last instructions
    int32_t depth = depth0 > 0 ? depth0 - 1 : 0;  // clifford.rs:342
    uint32_t bad = bad0, fault = 0;
    // (declared ahead of their values on purpose: declared where they are computed, the compiler pairs r_solved and r_open the other way round)
    float penalty = g.penalty, r_solved = 0.0f, r_open = 0.0f;  // (out of range: 0)
    uint32_t fin_open = 0;  // is_final of an env that is not solved
    uint32_t drow[4] = {0, 0, 0, 0}, dword[4] = {0, 0, 0, 0}, dchg = 0;  // D16: the rows the gate changed (bit k of dchg: entry k)
    // No branch around the rows: "no gate" (an out-of-range action, a two-qubit gate on equal qubits) is the identity map on qubit 0 -- its rows are
    // rewritten as they are and `bad` keeps its bit (`live`) -- so the chain from the gate entry to the stores is one block.  Between the issue of
    // the row loads and their arrival: the masks, the identity patterns, the cleared `bad`.  Behind it: 4 selects, 16 terms, 12 merges (HAS_Z).
    const bool layered = FEAT && (f.flags & F_LAYERS) && in_range;
    LayerTxn lt;
    if (layered) lt = layers_begin(layer_rec(a.layers, env, 2 * a.N + 2), a.N, a.descs[act]);  // its loads fly with the state's
    const uint32_t ops = g.ops, q0 = ops & 31u, q1 = (ops >> 5) & 31u;
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
    // 128 of the line gateset's 170 actions (75 %) stay in one group, and the launch ends when its stores have drained -- EXPERIMENTS.md round 7.
    // The two stores split by the group's parity instead -- no 128-byte line asked for twice, 47.3 line requests a wave instead of 56.1 -- measured
    // no faster: EXPERIMENTS.md round 10)
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
    // qg_vec_track_dense: matrix row r, column c of env e at dense[(e * D + r) * D + c] (clifford.rs:361-368, adapters.py:50-54)
    if constexpr (D16 == 2) {
        // The two lanes of a pair (2k, 2k + 1: neighbouring envs) write one 32-byte row together, 16 bytes each, so that a store
        // instruction's lanes cover whole rows: per-lane rows (two 16-byte stores 16 bytes apart from ONE lane) measured 5.28 us per step at
        // 65 536 envs, this form 4.83 (3.11 without the dense observation).  Every lane that runs this body reaches this point; a pair lane
        // that does not (past the batch's odd end) reads as "no row" -- update_dpp keeps `old` = 0 for a disabled source lane -- and the
        // env it leaves without a partner writes its rows alone.
        const bool solo = (env ^ 1ull) >= f.B;
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
    const bool solved = bad == 0;       // clifford.rs:344
    const float reward = solved ? r_solved : r_open;  // clifford.rs:345-346
    const uint32_t fin = solved ? 1u : fin_open;  // is_final (clifford.rs:353)
    if (a.rewards_seq) global_store(out_rseq, reward);
    if (a.dones_seq) global_store(out_dseq, (uint8_t)fin);
    if (bad != bad0) f.bad[env] = bad;
    // depth, done and success leave only where the step changed what memory held (an env at depth 0 keeps all three; success and done change on
    // well under 1 % of a rollout's steps): the launch ends when its stores have drained, and three of a step's seven stores were these.
    // rewards_seq and dones_seq above are a log: always written
    if (depth != depth0) f.depth[env] = depth;
    global_store(out_reward, reward);
    if (fin != done0) global_store(out_done, (uint8_t)fin);
    if ((uint32_t)solved != success0) global_store(out_success, (uint8_t)solved);
    if (FEAT && (f.flags & F_TRACK)) a.sol_len[env * 2] = sol_n;
    if (FEAT && fault) atomicOr(&a.error[env], fault);
    return fin != 0;
}

// A lane's element of a per-env array as "uniform base + 32-bit lane offset": the base stays in an SGPR pair, the offset is one VGPR that every array of
// the same element size shares (global_load / global_store with an saddr operand) -- no 64-bit per-lane address is built.  `byte_off` is zero-extended.
typedef uint32_t u32x2 __attribute__((ext_vector_type(2)));
template <class T>
__device__ inline T lane_load(const void *base, uint32_t byte_off) { return *(global_ptr<const T>)((global_ptr<const char>)base + byte_off); }
template <class T>
__device__ inline void lane_store(void *base, uint32_t byte_off, T v) {
    // (compiler only: the offset's zero extension stands in the store's own basic block -- extended in an earlier block, as for the loads, the store is
    // selected with a 64-bit per-lane address made by one more vector add)
    asm volatile("" : "+v"(byte_off));
    *(global_ptr<T>)((global_ptr<char>)base + byte_off) = v;
}

// qm_step1_mask_body for the launches in which the host has made every choice that body makes from values uniform over the launch (qgym_plan.hpp
// step1_straight; qm_step1_straight_kernel): int32 actions, every wave whole and taking the gate's groups across its lanes, no rewards_seq / dones_seq, no
// solution log, layer metrics, done list or dense observation.  Same loads, same stores, same arithmetic, same order -- and the same results, bit for bit --
// without the arms not taken, and with every per-lane address a 32-bit offset (`env`, 4 * env, the lane's place in its tile) from a base held in SGPRs.
// A body of its own for the reason given at the top of this file: shared helpers move the generic instantiations' code.  Statement order is load-bearing
// here as there.
template <bool HAS_Z>
__device__ inline void qm_step1_straight_body(const Step1Front &f, const StepArgs &a, uint32_t G, uint32_t env) {
    // The action's load is the head of the chain, and what stands in front of its issue is what round 11 measured as cost (profiles/r11/NUMBERS.md: the
    // generic kernel has 21 instructions there, the action's 64-bit address and the width's branch among them; putting those back alone gave the whole gain
    // away).  So it is the body's first instruction but one: its offset, then the load -- (compiler only) the barrier keeps the table's address arithmetic and
    // the other loads behind it.
    const uint32_t at4 = env << 2;                                    // the env's 4-byte elements
    const int32_t act = lane_load<int32_t>(f.actions, at4);
    __builtin_amdgcn_sched_barrier(0);
    const uint32_t lane = env & (QG_WAVE - 1);
    uint32_t at_tile = (env >> 6) * (G * 1024u) + (lane << 4);        // the env's place in its tile (G groups of 1 KiB), group 0
    // the group bytes of four actions, lane j holding those of actions 4 j .. 4 j + 3 (gate_group_bytes, qgym_plan.hpp)
    const uint32_t gtab = lane_load<uint32_t>(f.gates + f.num_actions, lane << 2);
    int32_t depth0 = lane_load<int32_t>(f.depth, at4);
    uint32_t bad0 = lane_load<uint32_t>(f.bad, at4);
    // done and success as memory holds them; their bases come from StepArgs, not from the preloaded arguments: (compiler only) the barrier keeps that
    // scalar wait behind the issue of depth and bad
    __builtin_amdgcn_sched_barrier(0);
    uint32_t done0 = lane_load<uint8_t>(a.done, env), success0 = lane_load<uint8_t>(a.success, env);
    asm volatile("" : "+v"(at_tile));
    // (the StepArgs fields the back of the chain reads are asked for here, in the batch of done's and success's: none of their cold lines behind the action)
    asm volatile("" : : "s"(a.N), "s"(a.reward));
    __builtin_amdgcn_sched_barrier(0);  // (compiler only: the loads above are issued before anything uses the action)
    // The gate entry's index clamped by one v_min_u32: an action out of range (negative ones are large as unsigned) reads "entry" num_actions -- the first
    // eight bytes of the group table, which lies directly behind the gate table in the same allocation -- and is given "no gate" below whatever it read.
    // A compare and a select in its place cost two instructions and two hazard waits between the action's arrival and the entry's load.
    const uint32_t gi = min((uint32_t)act, f.num_actions);
    const u32x2 entry = lane_load<u32x2>(f.gates, gi << 3);  // GateEntry {ops, penalty}; flies beside the row loads
    __builtin_amdgcn_sched_barrier(0);
    // the gate's two groups: one ds_bpermute_b32 by act >> 2 and two v_bfe behind the action (every lane of the wave holds its dword).  The entry's load
    // stays in front of the permute: behind it the step measured 0.02 us slower (the masks made from the entry are the longer arm under the rows' trip)
    uint32_t gb = (uint32_t)__builtin_amdgcn_ds_bpermute((int)(gi & ~3u), (int)gtab);
    const bool in_range = (uint32_t)act < f.num_actions;  // gateset.get(action) (clifford.rs:324): 0 <= act < num_actions
    gb = in_range ? gb : 0u;  // out of range: "no gate" on qubit 0, groups 0 / 0
    const uint32_t sh = (gi << 3) & 24u;
    const uint32_t g0 = __builtin_amdgcn_ubfe(gb, sh, 4u), g1 = __builtin_amdgcn_ubfe(gb, sh + 4u, 4u);
    const uint32_t at_a = at_tile + (g0 << 10), at_b = at_tile + (g1 << 10);
    const u32x4 va = lane_load<u32x4>(f.state, at_a), vb = lane_load<u32x4>(f.state, at_b);
    uint4 ua = make_uint4(va.x, va.y, va.z, va.w), ub = make_uint4(vb.x, vb.y, vb.z, vb.w);
    __builtin_amdgcn_sched_barrier(0);  // (compiler only: everything down to the next one stands between the loads and their wait)
    uint32_t g_ops = in_range ? entry.x : QM_IDENTITY << 10;  // "no gate", penalty 0: what an out-of-range action selects (clifford.rs:324)
    float g_penalty = in_range ? __uint_as_float(entry.y) : 0.0f;
    // the gate entry, depth and bad are all here: no later wait for a load
    asm volatile("" : "+v"(g_ops), "+v"(g_penalty), "+v"(depth0), "+v"(bad0) : "s"(a.N), "s"(a.reward), "s"(a.done), "s"(a.success));
    asm volatile("" : "+v"(done0), "+v"(success0));  // ... and the two old bytes: their first use is behind the row stores
    int32_t depth = depth0 > 0 ? depth0 - 1 : 0;  // clifford.rs:342
    float r_solved = 0.0f, r_open = 0.0f;
    uint32_t fin_open = 0;  // is_final of an env that is not solved
    const uint32_t ops = g_ops, q0 = ops & 31u, q1 = (ops >> 5) & 31u;
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
    uint32_t set0 = live & 1u, set1 = set0 & (uint32_t)(q0 != q1);  // `bad`: as in qm_step1_mask_body
    uint32_t bad_rest = bad0 & ~((set0 << q0) | (set1 << q1));
    r_solved = 1.0f - g_penalty; r_open = 0.0f - g_penalty;  // clifford.rs:345-346, both outcomes
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
    if (apart) lane_store(f.state, at_b, u32x4{ub.x, ub.y, ub.z, ub.w});  // (one group: q0's store carries q1's rows too)
    lane_store(f.state, at_a, u32x4{ua.x, ua.y, ua.z, ua.w});
    const uint32_t d0 = HAS_Z ? xor_or(nx0, ix0, nz0 ^ iz0) : nx0 ^ ix0, d1 = HAS_Z ? xor_or(nx1, ix1, nz1 ^ iz1) : nx1 ^ ix1;
    const uint32_t bad = bad_rest | (min(d0, set0) << q0) | (min(d1, set1) << q1);
    const bool solved = bad == 0;       // clifford.rs:344
    const float reward = solved ? r_solved : r_open;  // clifford.rs:345-346
    const uint32_t fin = solved ? 1u : fin_open;  // is_final (clifford.rs:353)
    if (bad != bad0) lane_store(f.bad, at4, bad);
    // depth, done and success leave only where the step changed what memory held (qm_step1_mask_body)
    if (depth != depth0) lane_store(f.depth, at4, depth);
    lane_store(a.reward, at4, reward);
    if (fin != done0) lane_store(a.done, env, (uint8_t)fin);
    if ((uint32_t)solved != success0) lane_store(a.success, env, (uint8_t)solved);
}

// The same step with the gate's arithmetic and the addresses as the compiler makes them from selects and compares, nothing computed ahead of its
// use (the body before round 7); same results.  The mask form keeps ~25 more values in registers across the rows' wait: the fused reset+step kernels
// (qm_reset_step_kernel, whose reset workgroups share the SIMDs with these lanes) would drop from 7-8 waves per SIMD to 4-6 with it, so they keep this one.
// PINNED_FRONT: the front of qm_step1_mask_body's chain (round 6) -- the lane loads its own action (`act` is ignored), {action, depth, bad} are
// issued back to back, the gate entry's load is unconditional and depth and bad are pinned where it is consumed.  Otherwise `act` is the env's action,
// held in a register, and the front is as the compiler orders it by itself -- depth and bad, then the gate entry behind the in_range branch, nothing
// pinned: the policy kernel (mid_head_sample_kernel) sits at its register limit, and the pinned form costs two of its instantiations one VGPR more.
// `alone`: the neighbouring lane does not run this body with the neighbouring env (the reset's lanes in qm_reset_step_kernel): the dense rows are
// then written by this lane alone.
template <bool HAS_Z, bool FEAT, int D16, bool PINNED_FRONT>
__device__ inline bool qm_step1_plain_body(const Step1Front &f, const StepArgs &a, uint32_t G, uint64_t env, int64_t act, bool alone) {
    const uint32_t lane = (uint32_t)env & (QG_WAVE - 1);
    uint4 *tile = reinterpret_cast<uint4 *>(f.state) + (env >> 6) * (uint64_t)(G * 64);
    int32_t depth, sol_n;
    uint32_t bad0;
    bool in_range;
    GateEntry g = GateEntry{QM_IDENTITY << 10, 0.0f};  // "no gate", penalty 0: what an out-of-range action selects (clifford.rs:324)
    if constexpr (PINNED_FRONT) {
        int32_t act_lo = 0, act_hi = 0;
        action_issue(f.actions, env, f.flags & F_ACT64, act_lo, act_hi);
        depth = f.depth[env];
        bad0 = f.bad[env];
        sol_n = (FEAT && (f.flags & F_TRACK)) ? a.sol_len[env * 2] : 0;
        __builtin_amdgcn_sched_barrier(0);  // (compiler only: the loads above are issued before anything uses the action -- the gate entry's load waits for it alone)
        act = action_value(act_lo, act_hi, f.flags & F_ACT64);
        in_range = (uint64_t)act < (uint64_t)f.num_actions;  // gateset.get(action) (clifford.rs:324): 0 <= act < num_actions
        const GateEntry entry = f.gates[in_range ? act : 0];
        if (in_range) g = entry;
        // the gate entry, depth and bad are all here: no later wait for a load, and the StepArgs fields the back reads are asked for (see qm_step1_mask_body)
        asm volatile("" : "+v"(g.ops), "+v"(g.penalty), "+v"(depth), "+v"(bad0)
                     : "s"(a.N), "s"(a.rewards_seq), "s"(a.dones_seq), "s"(a.reward), "s"(a.done), "s"(a.success));
        depth = depth > 0 ? depth - 1 : 0;  // clifford.rs:342
    } else {
        depth = f.depth[env];
        bad0 = f.bad[env];
        sol_n = (FEAT && (f.flags & F_TRACK)) ? a.sol_len[env * 2] : 0;
        in_range = act >= 0 && act < (int64_t)f.num_actions;  // gateset.get(action) (clifford.rs:324)
        if (in_range) g = f.gates[act];
    }
    uint32_t bad = bad0, fault = 0;
    float penalty = 0.0f;
    uint32_t drow[4] = {0, 0, 0, 0}, dword[4] = {0, 0, 0, 0}, dchg = 0;  // D16: the rows the gate changed (bit k of dchg: entry k)
    if (in_range) {
        penalty = g.penalty;
        const bool layered = FEAT && (f.flags & F_LAYERS);
        LayerTxn lt;
        if (layered) lt = layers_begin(layer_rec(a.layers, env, 2 * a.N + 2), a.N, a.descs[act]);  // its loads fly with the state's
        const uint32_t q0 = g.ops & 31u, q1 = (g.ops >> 5) & 31u, m = (g.ops >> 10) & 0xFFFFu;
        if (m != QM_IDENTITY) {  // "no gate" (e.g. a two-qubit gate on equal qubits) changes nothing
            constexpr uint32_t gsh = HAS_Z ? 1u : 2u;
            const uint32_t g0 = q0 >> gsh, g1 = q1 >> gsh;
            const uint4 va = tile[g0 * 64 + lane], vb = tile[g1 * 64 + lane];
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
            if (!same) tile[g1 * 64 + lane] = make_uint4(ub[0], ub[1], ub[2], ub[3]);
            tile[g0 * 64 + lane] = make_uint4(ua[0], ua[1], ua[2], ua[3]);
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
    if constexpr (D16 == 2) {
        // (lane pairs write whole 32-byte rows, as in qm_step1_mask_body; a lane whose partner is past the batch's end or being reset writes alone)
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
    if constexpr (!PINNED_FRONT) depth = depth > 0 ? depth - 1 : 0;  // clifford.rs:342
    const bool solved = bad == 0;       // clifford.rs:344
    const float achieved = solved ? 1.0f : 0.0f;
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
// ... for the policy kernel: the action in a register, the front from its StepArgs
template <bool HAS_Z, bool FEAT>
__device__ inline bool qm_step1_body(const StepArgs &a, uint32_t G, uint64_t env, int64_t act) {
    return qm_step1_plain_body<HAS_Z, FEAT, 0, false>(step1_front(a), a, G, env, act, false);
}

}  // namespace qg
