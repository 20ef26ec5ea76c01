// kernels_qm_step1.hip -- qm_step1_kernel, the one-step kernel of the TILE layout without add_inverts (env.step(): the headline), in a translation
// unit of its own: the Makefile builds this file alone with the kernel-argument preload (-mllvm -amdgpu-kernarg-preload-count=16), which applies to
// every kernel of a translation unit that has leading scalar or pointer parameters.  Layout and the other TILE kernels: kernels_qm.hip.
#include "device_common.hpp"
#include "qgym_plan.hpp"
#include "qm_step1.hpp"

namespace qg {

// threads per workgroup of the one-step launch: the kernel and qm_step1 below share it, so the kernel never reads blockDim.x (a hidden kernel
// argument: one more scalar load in front of the first vector load)
constexpr uint32_t QM_STEP1_BLOCK = 256;  // 64- and 128-thread blocks measured no faster

// One step per launch without holding the matrix (the env.step() path without add_inverts).  A gate
// touches the rows of <= 2 qubits (CliffordEnv) / <= 2 rows (LinearFunctionEnv), i.e. <= 2 of the env's
// 16-byte groups: they are gathered and scattered at per-lane addresses, and `solved` comes from the
// incrementally kept `bad` mask (bit j: qubit j's rows / row j differ from the identity's).  ~3x fewer
// instructions than the register-resident kernel, which at one wave per SIMD is what a step costs;
// measured 3.77 -> 3.15 us per step at B = 65 536 and 34.9 -> 30.0 us at B = 2^20 (CliffordEnv 16q).
//
// At one wave per SIMD nothing overlaps a lane's memory round trips, so their number is what the kernel costs (EXPERIMENTS.md round 6).  Round 6 left
// four (the form before round 10, and still the path of a wave without F_GROUP_LANES; today's chain: the round 10 paragraph below):
// {action, depth, bad} -> gate entry -> row groups -> every store (qm_step1_mask_body, qm_step1.hpp).  What the front of that chain
// reads comes as the kernel's leading parameters -- 14 dwords, the most the preload delivers in SGPRs beside the kernarg pointer -- so the first vector
// loads are issued without a scalar load in front of them; the rest of StepArgs follows by value and is fetched while those loads fly (one batch,
// waited for where the gate entry is consumed: a cold scalar line must not surface between the rows and the stores).  On firmware
// that does not preload, the compiler's compatibility prologue loads the same SGPRs first: correct, without the gain.
// Between those waits a lone wave pays every instruction (1.3-3 ns each: EXPERIMENTS.md round 7, round 2's issue microbenchmark), so the body keeps
// them few where nothing hides them: the gate word is decoded into 0 / -1 lane masks while the row loads fly, the rows go through one v_bitop3_b32 per select, merge and
// term of the 4x4 GF(2) map, `bad` is updated by shifts, "no gate" takes no branch, and what depends on the env's index alone (its place in the
// tile, the output addresses) is computed under the first loads and under the gate entry's.  The headline instantiation
// <16, true, false, false, false>: first row wait -> last output store 143 -> 68 instructions, gate entry's arrival -> row loads 28 -> 12,
// 269 -> 216 in all (profiles/r07/qm_step1_listing.txt); 2.817 -> 2.677 us per step at B = 65 536, 1.41 -> 1.24 us on the kernel's own clock
// (profiles/r07/NUMBERS.md).
// The launch ends when its stores have drained, and written bytes cost more than instructions (round 7: a second row store of the same 16 bytes,
// +0.17 us).  So depth, done and success -- three of a step's seven stores -- leave only in the lanes where the step changed what memory held: depth
// against the value the step loaded anyway, done and success against two byte loads issued with the first trip (64 B per wave each; a caller may
// have written either array, so nothing derived stands in for them).  An env at depth 0 stores none of the three; in a rollout success and done
// change on well under 1 % of the steps.  11 instructions more behind the row stores, 2-3 VGPRs more; written bytes 46.8 -> 41.1 B per env (PMC),
// 2.675 -> 2.613 us per step at B = 65 536 (profiles/r09/NUMBERS.md; the kernel's own clock rises 1.24 -> 1.29 us: the gain is the launch boundary).
// Asking for the second row group only in the lanes whose qubits sit in two groups was 0.09 us SLOWER and is not done (EXPERIMENTS.md round 9).
// Round 10 took the gate entry out of the chain: the row loads need its two groups only, and those come from one byte per action held across the wave's
// lanes (one ds_bpermute_b32; F_GROUP_LANES and a wave with 64 live lanes, else the old path by a uniform branch) -- {action, table dword, depth, bad, done,
// success} -> row groups -> every store, the gate entry flying beside the rows.  2.617 -> 2.557 us per step at B = 65 536, 1.285 -> 1.225 us on the kernel's own
// clock (profiles/r10/NUMBERS.md).  Launches of more than three workgroups per compute unit keep the old path (qgym_plan.hpp group_lanes_pays): the gain shrinks
// as waves share a SIMD and hide each other's trips, is nil at 3.5 workgroups per CU, and at four the permute costs 1.9 %.  So does a wave with fewer than
// 64 envs -- a batch's last wave, every wave of a batch under 64.
// LIST: also record the envs that finish, one bit each in StepArgs::done_mask (F_DONE_LIST; its own instantiation: the plain kernel's code stays as it is)
// DENSE (qg_vec_track_dense, N == NXP, D % 16 == 0): the rows the gate rewrote also go to the resident dense int8 observation
template <int NXP, bool HAS_Z, bool FEAT, bool LIST = false, bool DENSE = false>
__global__ __launch_bounds__(QM_STEP1_BLOCK) void qm_step1_kernel(const void *actions, int32_t *depth, uint32_t *bad, const GateEntry *gates, void *state,
                                                                   uint64_t B, uint32_t flags, uint32_t num_actions, StepArgs a) {
    KernelClock kclk(a.kclk, a.kclk_waves, QM_STEP1_BLOCK);  // device_common.hpp
    constexpr int R = HAS_Z ? 2 * NXP : NXP, G = R / 4;  // row slots and 16-byte groups per env (QmRows, kernels_qm.hip)
    constexpr int D16 = DENSE ? R / 16 : 0;
    const Step1Front f{actions, depth, bad, gates, state, B, flags, num_actions};
    const uint64_t env = (uint64_t)blockIdx.x * QM_STEP1_BLOCK + threadIdx.x;
    // the wave's lanes that have an env (the others do not run the body: only a wave with all 64 takes the gate's groups across lanes)
    const uint64_t wave_envs = __builtin_amdgcn_ballot_w64(env < B);
    if constexpr (LIST) {  // every thread reaches the wave's ballot
        bool fin = false;
        if (env < B) fin = qm_step1_mask_body<HAS_Z, FEAT, D16>(f, a, G, env, wave_envs);  // qm_step1.hpp
        done_mask_store(a.done_mask, B, fin, env, a.done_epoch);
    } else {
        if (env >= B) return;
        (void)qm_step1_mask_body<HAS_Z, FEAT, D16>(f, a, G, env, wave_envs);  // qm_step1.hpp
    }
}

// The straight-line form (round 11; F_STEP1_STRAIGHT, chosen per launch by qgym_plan.hpp step1_straight): the kernel above decides in every wave of every
// launch what the host knows before the launch -- the action width, whether the wave takes the gate's groups across lanes, whether the two sequence
// arrays are null, whether a kernel clock is attached -- and builds ten 64-bit per-lane addresses with vector arithmetic.  A launch with int32 actions,
// B % 64 == 0, num_actions <= 256, group_lanes_pays, no rewards_seq / dones_seq, no kernel clock attached, and none of FEAT, LIST, DENSE runs this kernel
// instead: one action load, the permute unconditional, no sequence stores, no KernelClock (neither a.kclk nor a.kclk_waves is read; nothing between the last
// output store and s_endpgm), and every per-lane address a shared 32-bit offset from an SGPR base (qm_step1_straight_body, qm_step1.hpp).  Every other
// launch -- a handle with a kernel clock, rollout(..., rewards_out=...), int64 actions, a ragged batch, more than 256 actions, more than three workgroups
// per compute unit -- runs the kernel above exactly as before.  The leading parameters are the same 14 dwords (flags is not read).
// What that is worth, measured part by part (profiles/r11/NUMBERS.md): the branch, the sequence code and the clock nothing that can be told from the spread
// (they are gone because under that predicate they cannot run); everything in front of the action's load and right behind its arrival, all of it.  The
// action's load is the head of the lane's chain, so it is issued first -- 5 instructions from the entry where the kernel above has 21 -- and the entry's index
// behind it is one v_min_u32 (qm_step1_straight_body).  260 -> 175 instructions, 71 -> 54 VGPRs (profiles/r11/qm_step1_listing.txt); 2.555 -> 2.512 us per step
// at B = 65 536 (two more sessions 2.564 -> 2.518, 2.562 -> 2.516), the same vector loads and the same stored bytes.
template <int NXP, bool HAS_Z>
__global__ __launch_bounds__(QM_STEP1_BLOCK) void qm_step1_straight_kernel(const void *actions, int32_t *depth, uint32_t *bad, const GateEntry *gates, void *state,
                                                                            uint64_t B, uint32_t flags, uint32_t num_actions, StepArgs a) {
    constexpr int R = HAS_Z ? 2 * NXP : NXP, G = R / 4;
    const Step1Front f{actions, depth, bad, gates, state, B, flags, num_actions};
    const uint32_t env = blockIdx.x * QM_STEP1_BLOCK + threadIdx.x;
    if (env >= (uint32_t)B) return;  // B % 64 == 0: a wave leaves as a whole or not at all
    qm_step1_straight_body<HAS_Z>(f, a, G, env);  // qm_step1.hpp
}

template <int NXP, bool HAS_Z>
static hipError_t launch_step1(const StepArgs &a, hipStream_t s) {
    const dim3 grid((unsigned)((a.B + QM_STEP1_BLOCK - 1) / QM_STEP1_BLOCK)), block(QM_STEP1_BLOCK);
    const bool feat = a.flags & (F_TRACK | F_LAYERS);
    const bool list = a.flags & F_DONE_LIST;
    if (a.flags & F_STEP1_STRAIGHT) {  // (the plan sets it only without FEAT, LIST and DENSE)
        if (feat || list || a.dense || a.rewards_seq || a.dones_seq || a.kclk || (a.flags & F_ACT64) || a.B % 64u) return hipErrorInvalidValue;
        hipLaunchKernelGGL((qm_step1_straight_kernel<NXP, HAS_Z>), grid, block, 0, s, a.actions, a.depth, a.bad, a.gates, a.state, a.B, a.flags, a.num_actions, a);
        return hipGetLastError();
    }
#define QM_STEP1_LAUNCH(...) \
    hipLaunchKernelGGL((qm_step1_kernel<NXP, HAS_Z, __VA_ARGS__>), grid, block, 0, s, a.actions, a.depth, a.bad, a.gates, a.state, a.B, a.flags, a.num_actions, a)
    constexpr int R = HAS_Z ? 2 * NXP : NXP;
    if constexpr (R % 16 == 0) {
        if (a.dense) {  // qg_vec_track_dense (the host passes it for N == NXP only)
            if (feat && list) QM_STEP1_LAUNCH(true, true, true);
            else if (feat) QM_STEP1_LAUNCH(true, false, true);
            else if (list) QM_STEP1_LAUNCH(false, true, true);
            else QM_STEP1_LAUNCH(false, false, true);
            return hipGetLastError();
        }
    }
    if (feat && list) QM_STEP1_LAUNCH(true, true);
    else if (feat) QM_STEP1_LAUNCH(true);
    else if (list) QM_STEP1_LAUNCH(false, true);
    else QM_STEP1_LAUNCH(false);
#undef QM_STEP1_LAUNCH
    return hipGetLastError();
}

hipError_t qm_step1(const StepArgs &a, uint32_t nxp, bool has_z, hipStream_t s) {
    if (!a.B) return hipSuccess;
    if (has_z) {
        switch (nxp) {
        case 4: return launch_step1<4, true>(a, s);
        case 8: return launch_step1<8, true>(a, s);
        case 12: return launch_step1<12, true>(a, s);
        case 16: return launch_step1<16, true>(a, s);
        }
    } else {
        switch (nxp) {
        case 4: return launch_step1<4, false>(a, s);
        case 8: return launch_step1<8, false>(a, s);
        case 12: return launch_step1<12, false>(a, s);
        case 16: return launch_step1<16, false>(a, s);
        case 20: return launch_step1<20, false>(a, s);
        case 24: return launch_step1<24, false>(a, s);
        case 28: return launch_step1<28, false>(a, s);
        case 32: return launch_step1<32, false>(a, s);
        }
    }
    return hipErrorInvalidValue;
}

}  // namespace qg
