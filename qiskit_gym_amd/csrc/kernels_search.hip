// kernels_search.hip -- the device-side steps of a beam search over a policy's log-probabilities: qg_beam_select, then qg_beam_merge (which
// beams of a target hold a state the target has already got) and, at the end of this file, qg_beam_advance (returns, winners, and which
// beams can still beat their target's winner).
//
// qg_beam_select: the selection step.  From the W beams x A actions
// of one target pick the W best continuations as (parent env, action) pairs, the operands of qg_vec_copy_envs and qg_vec_step, without
// leaving the device.  The rules are stated in include/qgym.h; tests/beammodel.py restates them in numpy.
//
// One workgroup per group.  A candidate is the flat index i = slot * A + action of its group; its rank is decided by ONE 64-bit key
//   key(i) = order(score) << 32 | (0xFFFFFFFF - i)       order: f32 -> uint32, monotone, -0 = +0, 0 = "no such candidate"
// so "score descending, then slot, then action ascending" is "key descending", and keys of different candidates differ: whatever way the
// candidates are dealt to lanes and waves, the W largest keys are the same W candidates in the same order.
//   1. every thread computes order(score) of its candidates (i = tid, tid + NT, ...: consecutive lanes, consecutive LDS words) into LDS and
//      keeps its largest key;
//   2. every wave extracts the W largest keys of ITS candidates: W rounds of a 64-lane max (cross-lane, no LDS, no barrier); the lane that
//      owned the round's winner looks for its next key below it (its own LDS words only);
//   3. one barrier, then the NW sorted lists (NW * W <= NT keys) are merged by counting: the thread that holds key k writes output slot
//      #{keys > k} if that is below W.
// Plain vector loads and stores only.
#include <hip/hip_fp16.h>

#include "device_common.hpp"
#include "qgym_host.hpp"

namespace qg {

using plan::BEAM_MAX_CAND;
using plan::BEAM_MAX_WIDTH;
using plan::BEAM_MAX_WAVES;  // the waves of a launch: qgym_plan.hpp beam_select_waves

struct BeamArgs {
    const void *logp;
    const float *cum;
    const uint8_t *live;
    uint32_t *parent;
    void *actions;
    float *cum_out;
    uint8_t *live_out;
    uint64_t ld;
    uint32_t A, W, n;  // n = W * A
    int32_t act64;
};

template <typename LT>
__device__ inline float beam_to_float(LT v);
template <>
__device__ inline float beam_to_float<float>(float v) { return v; }
template <>
__device__ inline float beam_to_float<uint16_t>(uint16_t v) { return __uint_as_float((uint32_t)v << 16); }  // bf16
template <>
__device__ inline float beam_to_float<__half>(__half v) { return __half2float(v); }

// larger score <=> larger word; NaN and -inf (a masked action) have no word; every other score's word is >= 0x00800000
__device__ inline uint32_t beam_order(float score) {
    if (score != score || score == -__builtin_huge_valf()) return 0u;
    uint32_t u = __float_as_uint(score);
    if (u == 0x80000000u) u = 0u;  // -0 ties with +0
    return (u & 0x80000000u) ? ~u : (u | 0x80000000u);
}
__device__ inline uint64_t beam_key(uint32_t order, uint32_t i) { return ((uint64_t)order << 32) | (uint64_t)(0xFFFFFFFFu - i); }

__device__ inline uint64_t wave_max_u64(uint64_t v) {
#pragma unroll
    for (int off = 32; off >= 1; off >>= 1) {
        const uint32_t hi = (uint32_t)__shfl_xor((int)(uint32_t)(v >> 32), off, 64), lo = (uint32_t)__shfl_xor((int)(uint32_t)v, off, 64);
        const uint64_t o = ((uint64_t)hi << 32) | lo;
        v = o > v ? o : v;
    }
    return v;
}

template <typename LT>
__global__ __launch_bounds__(64 * BEAM_MAX_WAVES) void beam_select_kernel(const BeamArgs a) {
    extern __shared__ uint64_t beam_lds[];
    const uint32_t tid = threadIdx.x, NT = blockDim.x, lane = tid & (QG_WAVE - 1), wave = tid >> 6, NW = NT >> 6;
    uint64_t *merged = beam_lds;                                         // [NW][W] each wave's keys, descending, 0 = none
    uint32_t *order = reinterpret_cast<uint32_t *>(beam_lds + NW * a.W);  // [n]
    const uint64_t slot0 = (uint64_t)blockIdx.x * a.W;                    // the group's first env
    const LT *logp = reinterpret_cast<const LT *>(a.logp);

    // 1. scores.  (slot, action) of candidate i without a division per candidate: i advances by NT = qs * A + qa
    uint32_t s = tid / a.A, act = tid - s * a.A;
    const uint32_t qs = NT / a.A, qa = NT - qs * a.A;
    uint64_t cur = 0;  // this thread's largest key not yet extracted
    for (uint32_t i = tid; i < a.n; i += NT) {
        uint32_t o = 0;
        if (a.live[slot0 + s]) o = beam_order(a.cum[slot0 + s] + beam_to_float<LT>(logp[(slot0 + s) * a.ld + act]));
        order[i] = o;
        if (o) {
            const uint64_t k = beam_key(o, i);
            cur = k > cur ? k : cur;
        }
        act += qa;
        s += qs;
        if (act >= a.A) {
            act -= a.A;
            s += 1;
        }
    }

    // 2. the wave's W largest keys; lane r keeps the r-th.  A thread's keys leave in descending order, so "not yet extracted" = "below the
    // last one extracted from this thread"
    uint64_t mine = 0;
    for (uint32_t r = 0; r < a.W; ++r) {
        const uint64_t m = wave_max_u64(cur);
        if (m == 0) break;  // (the same in every lane)
        if (lane == r) mine = m;
        if (cur == m) {
            uint64_t next = 0;
            for (uint32_t i = tid; i < a.n; i += NT) {
                const uint32_t o = order[i];
                const uint64_t k = beam_key(o, i);
                if (o && k < m && k > next) next = k;
            }
            cur = next;
        }
    }
    if (lane < a.W) merged[wave * a.W + lane] = mine;
    __syncthreads();

    // 3. merge by counting
    const uint32_t L = NW * a.W;  // <= NT
    const uint64_t k = tid < L ? merged[tid] : 0;
    uint32_t rank = 0, n_cand = 0;
    for (uint32_t j = 0; j < L; ++j) {
        const uint64_t o = merged[j];
        n_cand += o != 0;
        rank += o > k;
    }
    if (k && rank < a.W) {
        const uint32_t i = 0xFFFFFFFFu - (uint32_t)k;
        const uint32_t ps = i / a.A, pa = i - ps * a.A;
        const uint64_t p = slot0 + ps, out = slot0 + rank;
        a.parent[out] = (uint32_t)p;
        if (a.act64) reinterpret_cast<int64_t *>(a.actions)[out] = (int64_t)pa;
        else reinterpret_cast<int32_t *>(a.actions)[out] = (int32_t)pa;
        a.cum_out[out] = a.cum[p] + beam_to_float<LT>(logp[p * a.ld + pa]);  // the same single f32 addition as in 1.
        a.live_out[out] = 1;
    }
    if (tid < a.W && tid >= n_cand) {  // fewer candidates than slots: the rest hold no beam
        const uint64_t out = slot0 + tid;
        a.parent[out] = (uint32_t)out;
        if (a.act64) reinterpret_cast<int64_t *>(a.actions)[out] = (int64_t)a.A;
        else reinterpret_cast<int32_t *>(a.actions)[out] = (int32_t)a.A;  // out of range: "no gate" (clifford.rs:324)
        a.cum_out[out] = -__builtin_huge_valf();
        a.live_out[out] = 0;
    }
}

// ---- qg_beam_merge ---------------------------------------------------------------------------------------------------------------------------
// One workgroup per group; the rules are stated in include/qgym.h, tests/beammerge_model.py restates them in numpy.
//   1. salt[i] = splitmix64(i + 1) of every word index into LDS, once for the group's W envs;
//   2. every wave hashes whole envs (wave, wave + NW, ...): lane l sums splitmix64(w_i ^ salt[i]) over i = l, l + 64, ... (consecutive lanes,
//      consecutive words), a 64-lane wrapping sum (cross-lane, no LDS) closes the key.  The sum wraps, so the deal does not show in the key;
//   3. the group's history -- [0] = number of keys held, [1 ..] = the keys in the order they came -- is dealt to the threads; each compares
//      its keys with the W slot keys (LDS broadcast reads) and flags the slots it meets;
//   4. lane s of wave 0 decides slot s: no order word / revisit / duplicate (one pass over the W slots: a slot is a duplicate when another
//      remaining slot with its key has the larger (order word, lower slot)); survivors take consecutive places of the history by a ballot.
// One workgroup owns a group's history and counters for the whole launch: plain vector loads and stores, no atomics.
constexpr uint32_t MERGE_MAX_ENV_BYTES = 2048;
using plan::MERGE_WAVES;  // the waves of a launch: qgym_plan.hpp beam_merge_waves

struct MergeArgs {
    const void *words;
    const float *cum;
    const uint8_t *live;
    uint64_t *seen;  // [n_groups][1 + cap], or nullptr
    uint8_t *live_out;
    uint64_t *keys_out;  // or nullptr
    uint32_t *dropped;   // [n_groups][2], or nullptr
    uint64_t cap;
    uint32_t W, n;  // n = words per env
};

__host__ __device__ inline uint64_t merge_key_close(uint32_t n, uint64_t sum) {
    const uint64_t k = splitmix64((uint64_t)n ^ sum);
    return k ? k : 0x9E3779B97F4A7C15ull;  // 0 is the history's "empty"
}

__device__ inline uint64_t wave_sum_u64(uint64_t v) {
#pragma unroll
    for (int off = 32; off >= 1; off >>= 1) {
        const uint32_t hi = (uint32_t)__shfl_xor((int)(uint32_t)(v >> 32), off, 64), lo = (uint32_t)__shfl_xor((int)(uint32_t)v, off, 64);
        v += ((uint64_t)hi << 32) | lo;
    }
    return v;
}

template <typename WT>
__global__ __launch_bounds__(64 * MERGE_WAVES) void beam_merge_kernel(const MergeArgs a) {
    extern __shared__ uint64_t merge_lds[];
    const uint32_t tid = threadIdx.x, NT = blockDim.x, lane = tid & (QG_WAVE - 1), wave = tid >> 6, NW = NT >> 6;
    uint64_t *salt = merge_lds;                                  // [n]
    uint64_t *keys = merge_lds + a.n;                            // [W]
    uint32_t *ord = reinterpret_cast<uint32_t *>(keys + a.W);    // [W] order word of a slot still in the running, else 0
    uint32_t *hit = ord + a.W;                                   // [W] != 0: the slot's key is in the history
    const uint64_t slot0 = (uint64_t)blockIdx.x * a.W;           // the group's first env
    const WT *words = reinterpret_cast<const WT *>(a.words) + slot0 * a.n;

    // 1.
    for (uint32_t i = tid; i < a.n; i += NT) salt[i] = splitmix64((uint64_t)i + 1);
    if (tid < a.W) hit[tid] = 0;
    __syncthreads();

    // 2.
    for (uint32_t s = wave; s < a.W; s += NW) {
        uint64_t sum = 0;
        for (uint32_t i = lane; i < a.n; i += QG_WAVE) sum += splitmix64((uint64_t)words[(uint64_t)s * a.n + i] ^ salt[i]);
        sum = wave_sum_u64(sum);
        if (lane == 0) keys[s] = merge_key_close(a.n, sum);
    }
    __syncthreads();

    // 3.
    uint64_t *seen = a.seen ? a.seen + (uint64_t)blockIdx.x * (a.cap + 1) : nullptr;
    uint64_t held = 0;
    if (seen) {
        held = seen[0] < a.cap ? seen[0] : a.cap;  // (a buffer that was never cleared cannot send the scan out of bounds)
        for (uint64_t j = tid; j < held; j += NT) {
            const uint64_t h = seen[1 + j];
            for (uint32_t s = 0; s < a.W; ++s)
                if (keys[s] == h) hit[s] = 1;
        }
    }
    uint32_t o = 0;
    if (tid < a.W && a.live[slot0 + tid]) o = beam_order(a.cum[slot0 + tid]);
    __syncthreads();
    const bool revisit = tid < a.W && o && hit[tid];
    if (tid < a.W) ord[tid] = revisit ? 0u : o;
    __syncthreads();

    // 4.
    if (wave != 0) return;
    const bool in = tid < a.W && o && !revisit;
    bool dup = false;
    uint64_t k = 0;
    if (tid < a.W) {
        k = keys[tid];
        if (in)
            for (uint32_t j = 0; j < a.W; ++j) {
                const uint32_t oj = ord[j];
                dup |= oj && keys[j] == k && (oj > o || (oj == o && j < tid));
            }
    }
    const bool keep = in && !dup;
    const uint64_t kept = __ballot(keep);
    const uint32_t n_rev = (uint32_t)__popcll(__ballot(revisit)), n_dup = (uint32_t)__popcll(__ballot(dup));
    if (tid < a.W) {
        a.live_out[slot0 + tid] = keep ? 1 : 0;
        if (a.keys_out) a.keys_out[slot0 + tid] = k;
    }
    if (seen) {
        const uint64_t place = held + (uint64_t)__popcll(kept & ((1ull << lane) - 1ull));  // survivors in ascending slot order
        if (keep && place < a.cap) seen[1 + place] = k;
        const uint64_t total = held + (uint64_t)__popcll(kept);
        if (lane == 0) seen[0] = total < a.cap ? total : a.cap;
    }
    if (a.dropped && lane == 0) {
        a.dropped[2 * (uint64_t)blockIdx.x] += n_rev;
        a.dropped[2 * (uint64_t)blockIdx.x + 1] += n_dup;
    }
}

// ---- qg_beam_advance -------------------------------------------------------------------------------------------------------------------------
// One WAVE per group, lane s = slot s, ADVANCE_WAVES groups per workgroup (the waves of the last workgroup past n_groups leave at once); the
// rules are stated in include/qgym.h, tests/beambound_model.py restates them in numpy.  Every lane of a group's wave stays to the end -- the
// lanes past the width hold "not live" -- so the cross-lane steps see all 64:
//   - the pick is one 64-lane max of key = order(r) << 32 | ~slot over the solved slots (qg_beam_select's order word and key: -0 = +0, the
//     lowest slot among equals, the same whatever lane a slot sits in); the winner's own r comes back by a lane read;
//   - "is any slot hopeful", the beams ended and the group's live count are ballots.
// One wave owns its group's best, found, win_src, group_live and bounded entries for the whole launch: plain vector loads and stores, no
// atomics, no LDS, no barrier.  r + bonus is an f32 addition of its own (the file is built without contraction, and there is no product).
constexpr uint32_t ADVANCE_WAVES = 4;

struct AdvanceArgs {
    const int32_t *parent;
    const float *ret_in, *reward;
    const uint8_t *success, *done;
    uint8_t *live;
    float *best;
    uint8_t *found;
    float *ret_out;
    int32_t *win_src;
    uint8_t *group_live;
    int32_t *bounded;  // or nullptr
    uint64_t n_groups;
    uint32_t W, batch;  // batch = n_groups * W
    int32_t skip, mode;
    float bonus;
};

__global__ __launch_bounds__(64 * ADVANCE_WAVES) void beam_advance_kernel(const AdvanceArgs a) {
    const uint32_t lane = threadIdx.x & (QG_WAVE - 1), wave = threadIdx.x >> 6;
    const uint64_t g = (uint64_t)blockIdx.x * ADVANCE_WAVES + wave;
    if (g >= a.n_groups) return;  // (the whole wave)
    const bool in = lane < a.W;
    const uint64_t b = g * a.W + lane;  // < batch where `in`

    // 1. returns
    bool lv = in && a.live[b] != 0, solved = false, ended = false;
    float r = 0.0f;
    if (lv) {
        const uint32_t p = (uint32_t)a.parent[b];
        // a parent outside the batch is outside the contract: it is not followed
        r = (p < a.batch ? a.ret_in[p] : __builtin_nanf("")) + a.reward[b];
        solved = a.success[b] != 0;
        ended = a.done[b] != 0;
    }
    if (in) a.ret_out[b] = r;
    float best = a.best[g];  // (one address per wave)
    bool found = a.found[g] != 0;

    // 2. the group's winner
    const uint32_t o = solved ? beam_order(r) : 0u;  // NaN and -inf have no word: such a result is never > best
    const uint64_t top = wave_max_u64(o ? beam_key(o, lane) : 0ull);
    const uint32_t j = top ? 0xFFFFFFFFu - (uint32_t)top : 0u;
    const float rj = __shfl(r, (int)j, 64);
    const bool better = top != 0 && rj > best;
    if (better) {
        best = rj;
        found = true;
    }
    if (lane == 0) {
        a.win_src[g] = better ? (int32_t)(g * a.W + j) : a.skip;
        if (better) {
            a.best[g] = rj;
            a.found[g] = 1;
        }
    }

    // 3. beams that ended leave
    lv = lv && !ended;

    // 4. the bound
    uint32_t n_bounded = 0;
    if (a.mode != 0 && found) {
        const bool hopeful = lv && (r + a.bonus > best);
        const uint64_t hopefuls = __ballot(hopeful), lives = __ballot(lv);
        if (a.mode == 2 || hopefuls == 0) {
            n_bounded = (uint32_t)__popcll(lives & ~hopefuls);
            lv = hopeful;
        }
    }
    if (in) a.live[b] = lv ? 1 : 0;

    // 5.
    const uint32_t n_live = (uint32_t)__popcll(__ballot(lv));
    if (lane == 0) {
        a.group_live[g] = (uint8_t)n_live;
        if (a.bounded && n_bounded) a.bounded[g] += (int32_t)n_bounded;
    }
}

}  // namespace qg

using namespace qg;

extern "C" int qg_beam_select(const void *logp_dev, int logp_dtype, uint64_t ld, uint32_t num_actions, uint64_t n_groups, uint32_t width,
                              const float *cum_dev, const uint8_t *live_dev, uint32_t *parent_dev, void *actions_dev, int action_dtype,
                              float *cum_out_dev, uint8_t *live_out_dev, void *stream) {
    if (!logp_dev || !cum_dev || !live_dev || !parent_dev || !actions_dev || !cum_out_dev || !live_out_dev) return set_error(QG_ERR_INVALID, "null argument");
    if (num_actions == 0 || width == 0 || ld < num_actions) return set_error(QG_ERR_INVALID, "bad shape: width and num_actions must be positive, ld >= num_actions");
    if (action_dtype != QG_ACT_I32 && action_dtype != QG_ACT_I64) return set_error(QG_ERR_INVALID, "bad action dtype");
    if (logp_dtype != QG_DT_F32 && logp_dtype != QG_DT_BF16 && logp_dtype != QG_DT_F16) return set_error(QG_ERR_INVALID, "logp dtype must be f32, bf16 or f16");
    if (cum_out_dev == cum_dev || live_out_dev == live_dev) return set_error(QG_ERR_INVALID, "input and output arrays may not alias");
    if (width > BEAM_MAX_WIDTH || (uint64_t)width * num_actions > BEAM_MAX_CAND)
        return set_error(QG_ERR_UNSUPPORTED, "beam_select: width <= %u and width * num_actions <= %u supported", BEAM_MAX_WIDTH, BEAM_MAX_CAND);
    if (n_groups > 0x7FFFFFFFull || n_groups * width > 0xFFFFFFFFull) return set_error(QG_ERR_UNSUPPORTED, "beam_select: too many envs for 32-bit parent indices");
    if (n_groups == 0) return QG_OK;
    BeamArgs a;
    a.logp = logp_dev;
    a.cum = cum_dev;
    a.live = live_dev;
    a.parent = parent_dev;
    a.actions = actions_dev;
    a.cum_out = cum_out_dev;
    a.live_out = live_out_dev;
    a.ld = ld;
    a.A = num_actions;
    a.W = width;
    a.n = width * num_actions;
    a.act64 = action_dtype == QG_ACT_I64;
    const uint32_t waves = plan::beam_select_waves(a.n);  // the result does not depend on it
    const dim3 grid((unsigned)n_groups), block(64u * waves);
    const size_t lds = (size_t)waves * width * sizeof(uint64_t) + (size_t)a.n * sizeof(uint32_t);  // <= 4 KiB + 56 KiB
    hipStream_t s = (hipStream_t)stream;
    switch (logp_dtype) {
    case QG_DT_F32: hipLaunchKernelGGL(beam_select_kernel<float>, grid, block, lds, s, a); break;
    case QG_DT_BF16: hipLaunchKernelGGL(beam_select_kernel<uint16_t>, grid, block, lds, s, a); break;
    default: hipLaunchKernelGGL(beam_select_kernel<__half>, grid, block, lds, s, a); break;
    }
    HIP_TRY(hipGetLastError());
    return QG_OK;
}

extern "C" size_t qg_beam_seen_bytes(uint64_t n_groups, uint64_t seen_cap) { return (size_t)(n_groups * (seen_cap + 1) * sizeof(uint64_t)); }

extern "C" int qg_beam_merge(const void *words_dev, int word_bytes, uint32_t words_per_env, uint64_t n_groups, uint32_t width, const float *cum_dev,
                             const uint8_t *live_dev, void *seen_dev, uint64_t seen_cap, uint8_t *live_out_dev, uint64_t *keys_out_dev,
                             uint32_t *dropped_dev, void *stream) {
    if (!words_dev || !cum_dev || !live_dev || !live_out_dev) return set_error(QG_ERR_INVALID, "null argument");
    if (word_bytes != 1 && word_bytes != 4 && word_bytes != 8) return set_error(QG_ERR_INVALID, "word_bytes must be 1, 4 or 8");
    if (words_per_env == 0 || width == 0) return set_error(QG_ERR_INVALID, "bad shape: width and words_per_env must be positive");
    if (seen_dev && seen_cap == 0) return set_error(QG_ERR_INVALID, "a history needs seen_cap >= 1");
    if (live_out_dev == live_dev) return set_error(QG_ERR_INVALID, "input and output arrays may not alias");
    if (((uintptr_t)words_dev % (uintptr_t)word_bytes) || ((uintptr_t)seen_dev % 8) || ((uintptr_t)keys_out_dev % 8))
        return set_error(QG_ERR_INVALID, "words, history and keys must be aligned to their element size");
    if (width > BEAM_MAX_WIDTH || (uint64_t)words_per_env * (uint64_t)word_bytes > MERGE_MAX_ENV_BYTES)
        return set_error(QG_ERR_UNSUPPORTED, "beam_merge: width <= %u and words_per_env * word_bytes <= %u supported", BEAM_MAX_WIDTH, MERGE_MAX_ENV_BYTES);
    if (n_groups > 0x7FFFFFFFull || seen_cap > 0xFFFFFFFFull) return set_error(QG_ERR_UNSUPPORTED, "beam_merge: n_groups < 2^31 and seen_cap < 2^32 supported");
    if (n_groups == 0) return QG_OK;
    MergeArgs a;
    a.words = words_dev;
    a.cum = cum_dev;
    a.live = live_dev;
    a.seen = reinterpret_cast<uint64_t *>(seen_dev);
    a.live_out = live_out_dev;
    a.keys_out = keys_out_dev;
    a.dropped = dropped_dev;
    a.cap = seen_dev ? seen_cap : 0;
    a.W = width;
    a.n = words_per_env;
    const uint32_t waves = plan::beam_merge_waves(width, words_per_env, a.cap);  // the result does not depend on it
    const dim3 grid((unsigned)n_groups), block(64u * waves);
    const size_t lds = ((size_t)words_per_env + width) * sizeof(uint64_t) + (size_t)width * 2 * sizeof(uint32_t);  // <= 16 KiB + 1 KiB
    hipStream_t s = (hipStream_t)stream;
    switch (word_bytes) {
    case 1: hipLaunchKernelGGL(beam_merge_kernel<uint8_t>, grid, block, lds, s, a); break;
    case 4: hipLaunchKernelGGL(beam_merge_kernel<uint32_t>, grid, block, lds, s, a); break;
    default: hipLaunchKernelGGL(beam_merge_kernel<uint64_t>, grid, block, lds, s, a); break;
    }
    HIP_TRY(hipGetLastError());
    return QG_OK;
}

extern "C" int qg_beam_advance(uint64_t n_groups, uint32_t width, const int32_t *parent_dev, const float *ret_in_dev, const float *reward_dev,
                               const uint8_t *success_dev, const uint8_t *done_dev, uint8_t *live_dev, float *best_dev, uint8_t *found_dev,
                               float *ret_out_dev, int32_t *win_src_dev, uint8_t *group_live_dev, int32_t *bounded_dev, int32_t skip, float bonus,
                               int mode, void *stream) {
    if (!parent_dev || !ret_in_dev || !reward_dev || !success_dev || !done_dev || !live_dev || !best_dev || !found_dev || !ret_out_dev || !win_src_dev ||
        !group_live_dev)
        return set_error(QG_ERR_INVALID, "null argument");
    if (width == 0) return set_error(QG_ERR_INVALID, "bad shape: width must be positive");
    if (mode != QG_BOUND_NONE && mode != QG_BOUND_STOP && mode != QG_BOUND_PRUNE) return set_error(QG_ERR_INVALID, "mode must be 0 (none), 1 (stop) or 2 (prune)");
    if (ret_out_dev == ret_in_dev) return set_error(QG_ERR_INVALID, "input and output arrays may not alias");
    if (((uintptr_t)parent_dev % 4) || ((uintptr_t)ret_in_dev % 4) || ((uintptr_t)reward_dev % 4) || ((uintptr_t)best_dev % 4) || ((uintptr_t)ret_out_dev % 4) ||
        ((uintptr_t)win_src_dev % 4) || ((uintptr_t)bounded_dev % 4))
        return set_error(QG_ERR_INVALID, "32-bit arrays must be aligned to their element size");
    if (width > BEAM_MAX_WIDTH) return set_error(QG_ERR_UNSUPPORTED, "beam_advance: width <= %u supported", BEAM_MAX_WIDTH);
    if (n_groups * width > 0x7FFFFFFFull || n_groups > 0x7FFFFFFFull) return set_error(QG_ERR_UNSUPPORTED, "beam_advance: too many envs for 32-bit env indices");
    if (n_groups == 0) return QG_OK;
    AdvanceArgs a;
    a.parent = parent_dev;
    a.ret_in = ret_in_dev;
    a.reward = reward_dev;
    a.success = success_dev;
    a.done = done_dev;
    a.live = live_dev;
    a.best = best_dev;
    a.found = found_dev;
    a.ret_out = ret_out_dev;
    a.win_src = win_src_dev;
    a.group_live = group_live_dev;
    a.bounded = bounded_dev;
    a.n_groups = n_groups;
    a.W = width;
    a.batch = (uint32_t)(n_groups * width);
    a.skip = skip;
    a.mode = mode;
    a.bonus = bonus;
    const dim3 grid((unsigned)((n_groups + ADVANCE_WAVES - 1) / ADVANCE_WAVES)), block(64u * ADVANCE_WAVES);
    hipLaunchKernelGGL(beam_advance_kernel, grid, block, 0, (hipStream_t)stream, a);
    HIP_TRY(hipGetLastError());
    return QG_OK;
}
