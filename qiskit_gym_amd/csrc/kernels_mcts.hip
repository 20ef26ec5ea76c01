// kernels_mcts.hip -- the tree of a PUCT search (MCTS) over a policy's priors and values: qg_mcts_select (one descent per tree: which node to
// expand, by which action), qg_mcts_backup (link the new node, carry its value to the root; in mode QG_MCTS_ROOT: start a tree) and
// qg_mcts_decide (the root's visit counts and the move they give: the most visited action, or one drawn in proportion to the counts) and
// qg_mcts_rebase (between two decisions: the chosen move's subtree becomes the tree, in place).  The rules are stated in include/qgym.h;
// tests/mctsmodel.py, tests/mctssample_model.py and tests/mctsreuse_model.py restate them in numpy and the kernels agree with them bit for bit.
//
// qg_mcts_select_many and qg_mcts_backup_many are the first two for k descents per tree and launch (virtual visits between the descents);
// tests/mctsmany_model.py restates them.  What a pair shares is written once, in inline functions: a level's loads, scoring and lane read
// (mcts_level_*), the new node's stores and the walk to the root (mcts_new_node, mcts_walk_up); the four kernels stay four.
//
// The forest is a struct of plain arrays (qg_mcts_forest): per (tree, node) parent, reward, value, visits, wsum, terminal; per (tree, node,
// action) child and prior; per tree n_nodes.  One WAVE per tree in every kernel, several trees per workgroup; a wave owns its tree for the
// whole launch: plain vector loads and stores, no atomics, no barrier between waves.
//
// qg_mcts_decide.  The same lanes over the root's actions.  The draw needs the sums n_0 + ... + n_a in ACTION order: the slices k are consecutive
// blocks of 64 actions, so that is an inclusive scan over the lanes per slice (six __shfl_up steps) plus the totals of the slices before it, all
// in integers -- the result does not depend on the launch geometry.  No LDS: a root has few children, each count is one load behind the child row.
//
// qg_mcts_select.  The lanes cover the actions of the node the descent stands on (action lane + 64 k, k < 4).  A level's score needs the
// node's child and prior rows and, per expanded edge, the child's visits and wsum: the second would be a dependent memory trip behind the
// first.  So the wave first copies its tree's (visits, wsum) pairs -- n_nodes of them, at most cap -- into LDS, one trip for the whole
// tree; after that a level is ONE dependent trip to memory (child row, prior row, the node's value and terminal flag, all addressed by the
// node alone) and LDS reads.  The arg-max is qg_beam_advance's: one 64-lane max of key = order(score) << 32 | ~action (-0 = +0, the lowest
// action among equals, a NaN has no word), the winner's child index comes back by a lane read.
//
// Arithmetic: every operation of the score is one IEEE f32 operation, round to nearest -- the file is built with -ffp-contract=off, and
// `/` and __builtin_sqrtf are the correctly rounded division and square root of this build (hipcc's default
// -fhip-fp32-correctly-rounded-divide-sqrt; f32 denormals are kept on gfx950).  __fsqrt_rn is NOT used: without OCML_BASIC_ROUNDED_OPERATIONS
// it is the native, approximate square root.
//
// Every loop is bounded by the data's own size -- a descent makes at most cap levels, a backup walk at most cap steps, and both also move
// strictly (a child's index is above its parent's): an index read from the forest is range-checked before it is used, and a check that fails
// ends that tree's work for the call (leaf = -1, which qg_mcts_backup skips).
#include "device_common.hpp"
#include "qgym_host.hpp"

namespace qg {

// the launch geometry -- trees per workgroup, the rebase's slices of 64 actions -- and the limits: qgym_plan.hpp
using plan::MCTS_MAX_ACTIONS;
using plan::MCTS_MAX_CAP;
using plan::MCTS_WAVES;

// larger score <=> larger word; a NaN has no word (0); every other score's word is >= 0x007FFFFF
__device__ inline uint32_t mcts_order(float score) {
    if (score != score) return 0u;
    uint32_t u = __float_as_uint(score);
    if (u == 0x80000000u) u = 0u;  // -0 ties with +0
    return (u & 0x80000000u) ? ~u : (u | 0x80000000u);
}

__device__ inline uint64_t mcts_wave_max(uint64_t v) {
#pragma unroll
    for (int off = 32; off >= 1; off >>= 1) {
        const uint32_t hi = (uint32_t)__shfl_xor((int)(uint32_t)(v >> 32), off, 64), lo = (uint32_t)__shfl_xor((int)(uint32_t)v, off, 64);
        const uint64_t o = ((uint64_t)hi << 32) | lo;
        v = o > v ? o : v;
    }
    return v;
}

// One level of a descent, as both selection kernels make it.  What the wave holds of node x after the level's one trip to memory -- everything
// in it is addressed by x alone: the lane's entries of the child and prior rows (action lane + 64 k), the node's value and terminal flag.
struct MctsLevel {
    int32_t c[4];
    float p[4];
    float vx;
    bool term;
};

__device__ inline MctsLevel mcts_level_load(const qg_mcts_forest &f, uint64_t base, uint32_t x, uint32_t lane) {
    MctsLevel l;
    const uint64_t row = (base + x) * f.num_actions;
    l.term = f.terminal[base + x] != 0;
    l.vx = f.value[base + x];
#pragma unroll
    for (uint32_t k = 0; k < 4; ++k) {
        const uint32_t ac = lane + QG_WAVE * k;
        l.c[k] = ac < f.num_actions ? f.child[row + ac] : -1;
        l.p[k] = ac < f.num_actions ? f.prior[row + ac] : 0.0f;
    }
    return l;
}

// The lane's best candidate at node x (visits_x of them so far, n nodes in the tree), as key = order(score) << 32 | ~action, 0: none; `st` is
// the wave's LDS copy of (visits, wsum); bit k of `taken`: the lane's action of slice k is no candidate.  `bad`: a child index that is no node
// of this tree, or no step down.
__device__ inline uint64_t mcts_level_key(const MctsLevel &l, const uint2 *st, uint32_t visits_x, uint32_t x, uint32_t n, uint32_t A, float C, uint32_t lane,
                                          uint32_t taken, bool &bad) {
    const float sq = __builtin_sqrtf((float)(int32_t)visits_x);
    uint64_t key = 0;
    bool wrong = false;  // (a local, handed out once at the end: EXPERIMENTS.md section 24)
#pragma unroll
    for (uint32_t k = 0; k < 4; ++k) {
        const uint32_t ac = lane + QG_WAVE * k;
        if (ac >= A || ((taken >> k) & 1u)) continue;
        float q = l.vx;
        int32_t na = 0;
        if (l.c[k] >= 0) {
            if ((uint32_t)l.c[k] >= n || (uint32_t)l.c[k] <= x) {
                wrong = true;
                continue;
            }
            const uint2 s = st[l.c[k]];
            na = (int32_t)s.x;
            q = __uint_as_float(s.y) / (float)na;
        }
        const float u = ((C * l.p[k]) * sq) / (float)(1 + na);
        const uint32_t o = mcts_order(q + u);
        const uint64_t kk = ((uint64_t)o << 32) | (uint64_t)(0xFFFFFFFFu - ac);
        if (o && kk > key) key = kk;
    }
    bad = wrong;
    return key;
}

// the child under action `best`, by a read of the lane that holds it; < 0: an unexpanded edge
__device__ inline int32_t mcts_level_child(const MctsLevel &l, uint32_t best) {
    const uint32_t k = best >> 6;
    const int32_t mine = k == 0 ? l.c[0] : k == 1 ? l.c[1] : k == 2 ? l.c[2] : l.c[3];
    return __shfl(mine, (int)(best & (QG_WAVE - 1)), 64);
}

struct SelectArgs {
    qg_mcts_forest f;
    const uint8_t *finished;  // or nullptr
    int32_t *src, *dst, *act, *leaf;
    float C;
    uint32_t waves;
};

__global__ __launch_bounds__(64 * MCTS_WAVES) void mcts_select_kernel(const SelectArgs a) {
    extern __shared__ uint2 mcts_lds[];  // [waves][cap]: (visits, bits of wsum) of the wave's tree
    const qg_mcts_forest &f = a.f;
    const uint32_t lane = threadIdx.x & (QG_WAVE - 1), wave = threadIdx.x >> 6;
    const uint64_t m = (uint64_t)blockIdx.x * a.waves + wave;
    if (m >= f.n_trees) return;  // (the whole wave)
    const uint32_t cap = f.cap, A = f.num_actions;
    const uint64_t base = m * cap;                    // the tree's node 0, and its env in the pool
    const int32_t none = (int32_t)(f.n_trees * cap);  // out of range for the pool: qg_vec_copy_envs skips it
    uint2 *st = mcts_lds + (size_t)wave * cap;

    uint32_t x = 0;
    int32_t leaf = -1, act = (int32_t)A, dst = none;
    const uint32_t n = (uint32_t)f.n_nodes[m];
    const bool run = !(a.finished && a.finished[m] != 0) && n >= 1 && n <= cap;
    if (run) {
        for (uint32_t j = lane; j < n; j += QG_WAVE) st[j] = make_uint2((uint32_t)f.visits[base + j], __float_as_uint(f.wsum[base + j]));
        __builtin_amdgcn_wave_barrier();  // the wave reads what its other lanes wrote: LDS keeps a wave's accesses in order
        for (uint32_t level = 0; level < cap; ++level) {
            const MctsLevel l = mcts_level_load(f, base, x, lane);
            if (l.term) {  // the descent ends on a terminal node: nothing is expanded
                leaf = (int32_t)x;
                break;
            }
            bool bad;
            const uint64_t key = mcts_level_key(l, st, st[x].x, x, n, A, a.C, lane, 0u, bad);
            if (__ballot(bad)) break;  // leaf stays -1: the tree's work ends here
            const uint64_t top = mcts_wave_max(key);
            if (top == 0) {  // no candidate (every score a NaN): nothing to expand
                leaf = (int32_t)x;
                break;
            }
            const uint32_t best = 0xFFFFFFFFu - (uint32_t)top;
            const int32_t next = mcts_level_child(l, best);
            if (next < 0) {  // an unexpanded edge: the new node is n_nodes, if the tree has room
                if (n < cap) {
                    leaf = (int32_t)n;
                    dst = (int32_t)(base + n);
                    act = (int32_t)best;
                }
                break;
            }
            x = (uint32_t)next;  // x < next < n: at most cap - 1 steps down
        }
    }
    if (lane == 0) {
        a.src[m] = (int32_t)(base + x);
        a.dst[m] = dst;
        a.act[m] = act;
        a.leaf[m] = leaf;
    }
}

struct BackupArgs {
    qg_mcts_forest f;
    const int32_t *src, *dst, *act, *leaf;
    const float *logp, *values, *reward;
    const uint8_t *done;  // mode ROOT: or nullptr
    uint64_t ld;
    int32_t mode;
};

// the rows of node `node`: no child yet, prior = expf(logp)
__device__ inline void mcts_open_node(const qg_mcts_forest &f, uint64_t node, const float *logp, uint32_t lane) {
    for (uint32_t ac = lane; ac < f.num_actions; ac += QG_WAVE) {
        f.child[node * f.num_actions + ac] = -1;
        f.prior[node * f.num_actions + ac] = expf(logp[ac]);
    }
}

// the per-node fields of the new node j of the tree at `base`, the child of node x: one lane's stores
__device__ inline void mcts_new_node(const qg_mcts_forest &f, uint64_t base, int64_t j, int64_t x, float reward, float value, bool term) {
    f.parent[base + j] = (int32_t)x;
    f.reward[base + j] = reward;
    f.value[base + j] = value;
    f.visits[base + j] = 0;
    f.wsum[base + j] = 0.0f;
    f.terminal[base + j] = term ? 1 : 0;
}

// The walk from node y to the root with the leaf's value g, on one lane -- the lane that stored every field it loads, its stores in program order
// before these loads: one trip per level, every address is y's.  A parent that is no step up ends it, and the root is then not counted.
__device__ inline void mcts_walk_up(const qg_mcts_forest &f, uint64_t base, uint32_t y, float g) {
    for (uint32_t step = 0; step < f.cap && y != 0; ++step) {
        const int32_t up = f.parent[base + y];
        g = f.reward[base + y] + g;
        f.visits[base + y] += 1;
        f.wsum[base + y] += g;
        if (up < 0 || (uint32_t)up >= y) return;
        y = (uint32_t)up;
    }
    if (y == 0) f.visits[base] += 1;
}

__global__ __launch_bounds__(64 * MCTS_WAVES) void mcts_backup_kernel(const BackupArgs a) {
    const qg_mcts_forest &f = a.f;
    const uint32_t lane = threadIdx.x & (QG_WAVE - 1), wave = threadIdx.x >> 6;
    const uint64_t m = (uint64_t)blockIdx.x * MCTS_WAVES + wave;
    if (m >= f.n_trees) return;  // (the whole wave)
    const uint32_t cap = f.cap, A = f.num_actions;
    const uint64_t base = m * cap;
    const float *logp = a.logp + m * a.ld;

    if (a.mode == QG_MCTS_ROOT) {
        const bool term = a.done && a.done[m] != 0;
        mcts_open_node(f, base, logp, lane);
        if (lane == 0) {
            f.parent[base] = -1;
            f.reward[base] = 0.0f;
            f.value[base] = term ? 0.0f : a.values[m];
            f.visits[base] = 1;
            f.wsum[base] = 0.0f;
            f.terminal[base] = term ? 1 : 0;
            f.n_nodes[m] = 1;
        }
        return;
    }

    const int32_t leaf = a.leaf[m];
    uint32_t n = (uint32_t)f.n_nodes[m];
    if (leaf < 0 || n < 1 || n > cap) return;  // no simulation that counts
    const uint32_t ac = (uint32_t)a.act[m];
    const bool expand = ac < A;
    float g;  // the leaf's value
    if (expand) {
        const int64_t x = (int64_t)a.src[m] - (int64_t)base, j = (int64_t)a.dst[m] - (int64_t)base;
        // the new node is n_nodes, below cap, the child of a node of this tree by an edge that has none
        if (x < 0 || x >= (int64_t)n || j != (int64_t)n || j >= (int64_t)cap || leaf != (int32_t)j) return;
        if (f.child[(base + (uint64_t)x) * A + ac] != -1) return;
        const bool term = a.done[m] != 0;
        g = term ? 0.0f : a.values[m];
        mcts_open_node(f, base + (uint64_t)j, logp, lane);
        if (lane == 0) {
            mcts_new_node(f, base, j, x, a.reward[m], g, term);
            f.child[(base + (uint64_t)x) * A + ac] = (int32_t)j;
            f.n_nodes[m] = (int32_t)(n + 1);
        }
        n += 1;
    } else {
        if ((uint32_t)leaf >= n) return;
        g = f.value[base + (uint32_t)leaf];
    }
    if (lane == 0) mcts_walk_up(f, base, (uint32_t)leaf, g);
}

struct SelectManyArgs {
    qg_mcts_forest f;
    const uint8_t *finished;  // or nullptr
    int32_t *src, *dst, *act, *leaf;
    float C, vloss;
    uint32_t waves, k, stride;
};

// k descents per tree in one launch, one after another on the tree's statistics (qg_mcts_select_many).  The LDS copy of (visits, wsum) that
// mcts_select_kernel makes is the overlay: as a descent leaves a node, lane 0 adds the virtual visit there (and takes virtual_loss from its
// wsum, the root's excepted) -- LDS keeps a wave's accesses in order, so the next read of any lane sees it.  The edges chosen for expansion
// so far live in registers, pair e in lane e (stride <= 64): at a node that some pair names, the pairs are read lane by lane and the lane
// that holds the action drops it from its candidates.  The four outputs of descent i are kept in lane i and stored once, at the end, so a
// call writes entries 0 .. stride - 1 of every array.  Nothing is written into the forest.
__global__ __launch_bounds__(64 * MCTS_WAVES) void mcts_select_many_kernel(const SelectManyArgs a) {
    extern __shared__ uint2 mcts_lds[];  // [waves][cap]: (visits, bits of wsum) of the wave's tree, with this call's virtual visits
    const qg_mcts_forest &f = a.f;
    const uint32_t lane = threadIdx.x & (QG_WAVE - 1), wave = threadIdx.x >> 6;
    const uint64_t m = (uint64_t)blockIdx.x * a.waves + wave;
    if (m >= f.n_trees) return;  // (the whole wave)
    const uint32_t cap = f.cap, A = f.num_actions;
    const uint64_t base = m * cap;
    const int32_t none = (int32_t)(f.n_trees * cap);
    uint2 *st = mcts_lds + (size_t)wave * cap;

    // lane i: the outputs of descent i -- a refused one until it is made
    int32_t o_src = (int32_t)base, o_dst = none, o_act = (int32_t)A, o_leaf = -1;
    int32_t pend_x = -1;    // lane e: the e-th edge chosen for expansion, (node, action)
    uint32_t pend_a = 0;
    uint32_t grown = 0;     // edges chosen so far
    const uint32_t n = (uint32_t)f.n_nodes[m];
    bool run = !(a.finished && a.finished[m] != 0) && n >= 1 && n <= cap;
    if (run) {
        for (uint32_t j = lane; j < n; j += QG_WAVE) st[j] = make_uint2((uint32_t)f.visits[base + j], __float_as_uint(f.wsum[base + j]));
        __builtin_amdgcn_wave_barrier();
    }
    for (uint32_t i = 0; i < a.k && run; ++i) {
        uint32_t x = 0;
        int32_t leaf = -1, act = (int32_t)A, dst = none;
        for (uint32_t level = 0; level < cap; ++level) {
            const MctsLevel l = mcts_level_load(f, base, x, lane);
            const uint2 sx = st[x];  // x < n
            __builtin_amdgcn_wave_barrier();  // every lane has read the node's pair before lane 0 changes it
            // the descent stands on x once, and everything it reads of x it has read: the virtual visit
            const uint2 after = make_uint2(sx.x + 1u, x != 0 ? __float_as_uint(__uint_as_float(sx.y) - a.vloss) : sx.y);
            if (l.term) {  // the descent ends on a terminal node: nothing is expanded
                if (lane == 0) st[x] = after;
                leaf = (int32_t)x;
                break;
            }
            // the edges of x that an earlier descent of this call chose: no candidates
            uint32_t taken = 0;
            for (uint64_t hit = __ballot(pend_x == (int32_t)x); hit; hit &= hit - 1) {  // at most 64 pairs
                const uint32_t pa = (uint32_t)__shfl((int)pend_a, (int)__builtin_ctzll(hit), 64);
                if ((pa & (QG_WAVE - 1)) == lane) taken |= 1u << (pa >> 6);
            }
            bool bad;
            const uint64_t key = mcts_level_key(l, st, sx.x, x, n, A, a.C, lane, taken, bad);
            if (__ballot(bad)) {  // leaf stays -1, and the tree's work ends here: no later descent is made
                run = false;
                break;
            }
            __builtin_amdgcn_wave_barrier();  // the children's pairs are read
            if (lane == 0) st[x] = after;
            const uint64_t top = mcts_wave_max(key);
            if (top == 0) {  // no candidate left: nothing to expand
                leaf = (int32_t)x;
                break;
            }
            const uint32_t best = 0xFFFFFFFFu - (uint32_t)top;
            const int32_t next = mcts_level_child(l, best);
            if (next < 0) {  // an unexpanded edge: the new node is n_nodes + the edges chosen before, if the tree has room
                if (n + grown < cap) {  // (grown <= 64: no overflow)
                    leaf = (int32_t)(n + grown);
                    dst = (int32_t)(base + n + grown);
                    act = (int32_t)best;
                    if (lane == grown) {
                        pend_x = (int32_t)x;
                        pend_a = best;
                    }
                    grown += 1;
                }
                break;
            }
            x = (uint32_t)next;  // x < next < n: at most cap - 1 steps down
        }
        __builtin_amdgcn_wave_barrier();  // lane 0's virtual visits before the next descent's reads
        if (lane == i) {
            o_src = (int32_t)(base + x);
            o_dst = dst;
            o_act = act;
            o_leaf = leaf;
        }
    }
    if (lane < a.stride) {
        const uint64_t at = m * a.stride + lane;
        a.src[at] = o_src;
        a.dst[at] = o_dst;
        a.act[at] = o_act;
        a.leaf[at] = o_leaf;
    }
}

struct BackupManyArgs {
    qg_mcts_forest f;
    const int32_t *src, *dst, *act, *leaf;
    const float *logp, *values, *reward;
    const uint8_t *done;
    uint64_t ld;
    uint32_t k, stride;
};

// mcts_backup_kernel's QG_MCTS_BACKUP body k times per tree, entry m * stride + i in turn, n_nodes in a register (qg_mcts_backup_many).
// A later entry reads what an earlier one of the same launch stored, so every such location has ONE lane that stores and loads it, and what
// that lane reads is handed to the others by a lane read: child[x][a] belongs to lane a % 64 (the row of a new node and the link into it),
// every per-node field and the walk to lane 0.  A lane's own stores are in program order before its loads.
__global__ __launch_bounds__(64 * MCTS_WAVES) void mcts_backup_many_kernel(const BackupManyArgs a) {
    const qg_mcts_forest &f = a.f;
    const uint32_t lane = threadIdx.x & (QG_WAVE - 1), wave = threadIdx.x >> 6;
    const uint64_t m = (uint64_t)blockIdx.x * MCTS_WAVES + wave;
    if (m >= f.n_trees) return;  // (the whole wave)
    const uint32_t cap = f.cap, A = f.num_actions;
    const uint64_t base = m * cap;
    const uint32_t n0 = (uint32_t)f.n_nodes[m];
    if (n0 < 1 || n0 > cap) return;  // no simulation that counts
    uint32_t n = n0;
    for (uint32_t i = 0; i < a.k; ++i) {
        const uint64_t e = m * a.stride + i;
        const int32_t leaf = a.leaf[e];
        if (leaf < 0) continue;
        const uint32_t ac = (uint32_t)a.act[e];
        const bool expand = ac < A;
        float g = 0.0f;  // the leaf's value: lane 0's
        if (expand) {
            const int64_t x = (int64_t)a.src[e] - (int64_t)base, j = (int64_t)a.dst[e] - (int64_t)base;
            // the new node is n_nodes, below cap, the child of a node of this tree by an edge that has none
            if (x < 0 || x >= (int64_t)n || j != (int64_t)n || j >= (int64_t)cap || leaf != (int32_t)j) continue;
            const uint32_t owner = ac & (QG_WAVE - 1);
            int32_t *edge = f.child + (base + (uint64_t)x) * A + ac;
            const int32_t had = __shfl(lane == owner ? *edge : 0, (int)owner, 64);
            if (had != -1) continue;
            const bool term = a.done[e] != 0;
            g = term ? 0.0f : a.values[e];
            mcts_open_node(f, base + (uint64_t)j, a.logp + e * a.ld, lane);
            if (lane == owner) *edge = (int32_t)j;
            if (lane == 0) mcts_new_node(f, base, j, x, a.reward[e], g, term);
            n += 1;
        } else if ((uint32_t)leaf >= n) {
            continue;
        }
        if (lane == 0) mcts_walk_up(f, base, (uint32_t)leaf, expand ? g : f.value[base + (uint32_t)leaf]);
    }
    if (lane == 0 && n != n0) f.n_nodes[m] = (int32_t)n;
}

struct DecideArgs {
    qg_mcts_forest f;
    const uint8_t *finished;  // or nullptr
    int32_t *move;
    int32_t *counts;  // or nullptr
    uint64_t counts_ld, seed, counter;
    int32_t mode;
};

__device__ inline uint64_t mcts_shfl64(uint64_t v, int src) {
    const uint32_t hi = (uint32_t)__shfl((int)(uint32_t)(v >> 32), src, 64), lo = (uint32_t)__shfl((int)(uint32_t)v, src, 64);
    return ((uint64_t)hi << 32) | lo;
}

// inclusive prefix sum over the 64 lanes, in lane order: six shifted additions
__device__ inline uint64_t mcts_wave_scan(uint64_t v, uint32_t lane) {
#pragma unroll
    for (int off = 1; off < 64; off <<= 1) {
        const uint32_t hi = (uint32_t)__shfl_up((int)(uint32_t)(v >> 32), off, 64), lo = (uint32_t)__shfl_up((int)(uint32_t)v, off, 64);
        if (lane >= (uint32_t)off) v += ((uint64_t)hi << 32) | lo;
    }
    return v;
}

// The decision after a decision's simulations: the root's visit counts, and the move they give -- the most visited action, or one drawn in
// proportion to the counts.  The lanes cover the root's actions as in the selection; the counts are one dependent trip behind the child row
// (the root's children are few, so no LDS copy of the tree pays here).  Nothing is written into the forest.
__global__ __launch_bounds__(64 * MCTS_WAVES) void mcts_decide_kernel(const DecideArgs a) {
    const qg_mcts_forest &f = a.f;
    const uint32_t lane = threadIdx.x & (QG_WAVE - 1), wave = threadIdx.x >> 6;
    const uint64_t m = (uint64_t)blockIdx.x * MCTS_WAVES + wave;
    if (m >= f.n_trees) return;  // (the whole wave)
    const uint32_t cap = f.cap, A = f.num_actions;
    const uint64_t base = m * cap;
    const bool fin = a.finished && a.finished[m] != 0;
    if (fin && !a.counts) {  // no gate, and nobody asks for the row
        if (lane == 0) a.move[m] = (int32_t)A;
        return;
    }

    const uint32_t n = (uint32_t)f.n_nodes[m];
    bool bad = n < 1 || n > cap;
    int32_t c[4];
#pragma unroll
    for (uint32_t k = 0; k < 4; ++k) {
        const uint32_t ac = lane + QG_WAVE * k;
        c[k] = (!bad && ac < A) ? f.child[base * A + ac] : -1;
    }
    uint32_t na[4];   // n_a
    bool grown[4];    // the edge has a child
#pragma unroll
    for (uint32_t k = 0; k < 4; ++k) {
        na[k] = 0;
        grown[k] = c[k] >= 0;
        if (!grown[k]) continue;
        if (c[k] == 0 || (uint32_t)c[k] >= n) {  // no child of this tree's root
            bad = true;
            continue;
        }
        const int32_t v = f.visits[base + (uint32_t)c[k]];
        if (v < 0) bad = true;
        else na[k] = (uint32_t)v;
    }
    if (__ballot(bad)) {  // the tree's work ends here: no move, a row of zeros
#pragma unroll
        for (uint32_t k = 0; k < 4; ++k) {
            na[k] = 0;
            grown[k] = false;
        }
    }
    if (a.counts) {
#pragma unroll
        for (uint32_t k = 0; k < 4; ++k) {
            const uint32_t ac = lane + QG_WAVE * k;
            if (ac < A) a.counts[m * a.counts_ld + ac] = (int32_t)na[k];
        }
    }
    if (fin) {
        if (lane == 0) a.move[m] = (int32_t)A;
        return;
    }

    uint32_t move = A;
    uint64_t total = 0;
    if (a.mode == QG_MCTS_SAMPLE) {
        uint64_t incl[4];  // the sums up to and including the lane's action, in action order: slice k holds actions 64 k .. 64 k + 63
#pragma unroll
        for (uint32_t k = 0; k < 4; ++k) {
            incl[k] = total;
            if (QG_WAVE * k >= A) continue;  // (the whole wave)
            incl[k] += mcts_wave_scan((uint64_t)na[k], lane);
            total = mcts_shfl64(incl[k], QG_WAVE - 1);
        }
        if (total != 0) {
            const uint64_t r = __umul64hi(rng_draw(a.seed ^ 0x6D637473ull, m, a.counter), total);  // r < total
#pragma unroll
            for (uint32_t k = 0; k < 4; ++k) {
                // the lowest action whose sum exceeds r: the one action with incl - n_a <= r < incl
                const uint64_t hit = __ballot(incl[k] > r && incl[k] - na[k] <= r);
                if (hit) move = QG_WAVE * k + (uint32_t)__builtin_ctzll(hit);
            }
        }
    }
    if (total == 0) {  // the most visited of the expanded edges, the lowest action among equals
        uint64_t key = 0;
#pragma unroll
        for (uint32_t k = 0; k < 4; ++k) {
            const uint64_t kk = ((uint64_t)na[k] << 32) | (uint64_t)(0xFFFFFFFFu - (lane + QG_WAVE * k));
            if (grown[k] && kk > key) key = kk;
        }
        const uint64_t top = mcts_wave_max(key);
        if (top != 0) move = 0xFFFFFFFFu - (uint32_t)top;
    }
    if (lane == 0) a.move[m] = (int32_t)move;
}

struct RebaseArgs {
    qg_mcts_forest f;
    const int32_t *move;
    const uint8_t *finished;  // or nullptr
    int32_t *env_src;
    uint32_t waves;
};

// The step between two decisions: the chosen move's subtree becomes the tree, in place.  Four passes per tree, all on its one wave:
//   1  the tree's parents into LDS (one trip);
//   2  per slice of 64 nodes, ascending: is the lane's node below c?  It walks its parents in LDS until it leaves the slice -- there the
//      answer is already in the table -- so at most 64 steps of a strictly falling index; the new index is the kept nodes so far plus the
//      kept lanes below this one (a ballot and a popcount);
//   3  the per-node fields, one node per lane, a slice per trip, and the LDS copy of the parents gives way to the list of the kept nodes;
//   4  the child and prior rows, ROWS kept nodes per trip (16 rows of up to 64 actions ... 4 rows of up to 256), the child entries renumbered
//      through the table.
// In place: a kept node's new index is below its old one and the order is kept, so with ascending nodes, and every load of a trip issued
// before its first store, a store never lands on a node still to be read.
template <uint32_t K>  // slices of 64 actions
__global__ __launch_bounds__(64 * MCTS_WAVES) void mcts_rebase_kernel(const RebaseArgs a) {
    constexpr uint32_t ROWS = plan::mcts_rebase_rows(K);
    extern __shared__ int32_t mcts_rebase_lds[];  // [waves][2][cap]: parent, later the kept nodes in order | new index, -1: not kept
    const qg_mcts_forest &f = a.f;
    const uint32_t lane = threadIdx.x & (QG_WAVE - 1), wave = threadIdx.x >> 6;
    const uint64_t m = (uint64_t)blockIdx.x * a.waves + wave;
    if (m >= f.n_trees) return;  // (the whole wave)
    const uint32_t cap = f.cap, A = f.num_actions;
    const uint64_t base = m * cap;
    const int32_t none = (int32_t)(f.n_trees * cap);
    int32_t *par = mcts_rebase_lds + (size_t)wave * 2 * cap, *idx = par + cap;
    int32_t *es = a.env_src + base;

    if (a.finished && a.finished[m] != 0) {  // the tree is left alone and copies nothing
        for (uint32_t j = lane; j < cap; j += QG_WAVE) es[j] = none;
        return;
    }
    const int32_t n_raw = f.n_nodes[m], mv = a.move[m];
    int32_t c = -1;
    if (n_raw >= 1 && (uint32_t)n_raw <= cap && mv >= 0 && (uint32_t)mv < A) c = f.child[base * A + (uint32_t)mv];
    if (!(c > 0 && c < n_raw)) {  // nothing to carry: every node keeps its env
        const uint32_t lim = n_raw < 1 ? 0u : (uint32_t)n_raw > cap ? cap : (uint32_t)n_raw;
        for (uint32_t j = lane; j < cap; j += QG_WAVE) es[j] = j < lim ? (int32_t)(base + j) : none;
        return;
    }
    const uint32_t n = (uint32_t)n_raw;

    for (uint32_t j = lane; j < n; j += QG_WAVE) par[j] = f.parent[base + j];
    __builtin_amdgcn_wave_barrier();  // the wave reads what its other lanes wrote: LDS keeps a wave's accesses in order

    uint32_t kept = 0;
    for (uint32_t s = 0; s < n; s += QG_WAVE) {
        const uint32_t j = s + lane;
        bool keep = j == (uint32_t)c;
        if (j > (uint32_t)c && j < n) {
            uint32_t y = j;
            for (uint32_t step = 0; step < QG_WAVE; ++step) {
                const int32_t p = par[y];
                if (p < c || (uint32_t)p >= y) break;  // the chain breaks, or passes below c
                if (p == c) {
                    keep = true;
                    break;
                }
                if ((uint32_t)p < s) {  // an earlier slice: settled
                    keep = idx[p] >= 0;
                    break;
                }
                y = (uint32_t)p;
            }
        }
        const uint64_t mask = __ballot(keep);
        if (j < n) idx[j] = keep ? (int32_t)(kept + (uint32_t)__popcll(mask & ((1ull << lane) - 1ull))) : -1;
        kept += (uint32_t)__popcll(mask);
        __builtin_amdgcn_wave_barrier();
    }

    for (uint32_t s = 0; s < n; s += QG_WAVE) {
        const uint32_t j = s + lane;
        const int32_t to = j < n ? idx[j] : -1;
        if (to >= 0) {
            const int32_t up = par[j];  // kept: c <= up < j, or j is c
            int32_t pa = to == 0 ? -1 : idx[up];
            float rw = f.reward[base + j], ws = f.wsum[base + j];
            const float va = f.value[base + j];
            const int32_t vi = f.visits[base + j];
            const uint8_t te = f.terminal[base + j];
            if (to == 0) rw = ws = 0.0f;  // the new root
            f.parent[base + to] = pa;
            f.reward[base + to] = rw;
            f.value[base + to] = va;
            f.visits[base + to] = vi;
            f.wsum[base + to] = ws;
            f.terminal[base + to] = te;
        }
        __builtin_amdgcn_wave_barrier();
        if (to >= 0) par[to] = (int32_t)j;  // to <= j, and nobody reads a parent at or below this slice again
    }
    __builtin_amdgcn_wave_barrier();

    for (uint32_t j0 = 0; j0 < kept; j0 += ROWS) {
        int32_t ch[ROWS][K];
        float pr[ROWS][K];
#pragma unroll
        for (uint32_t r = 0; r < ROWS; ++r) {
            const bool row = j0 + r < kept;
            const uint64_t from = (base + (uint32_t)(row ? par[j0 + r] : 0)) * A;
#pragma unroll
            for (uint32_t k = 0; k < K; ++k) {
                const uint32_t ac = lane + QG_WAVE * k;
                ch[r][k] = row && ac < A ? f.child[from + ac] : -1;
                pr[r][k] = row && ac < A ? f.prior[from + ac] : 0.0f;
            }
        }
#pragma unroll
        for (uint32_t r = 0; r < ROWS; ++r) {
#pragma unroll
            for (uint32_t k = 0; k < K; ++k) ch[r][k] = ch[r][k] >= 0 && (uint32_t)ch[r][k] < n ? idx[ch[r][k]] : -1;
        }
#pragma unroll
        for (uint32_t r = 0; r < ROWS; ++r) {
            const uint64_t to = (base + j0 + r) * A;
#pragma unroll
            for (uint32_t k = 0; k < K; ++k) {
                const uint32_t ac = lane + QG_WAVE * k;
                if (j0 + r < kept && ac < A) {
                    f.child[to + ac] = ch[r][k];
                    f.prior[to + ac] = pr[r][k];
                }
            }
        }
    }
    for (uint32_t j = lane; j < cap; j += QG_WAVE) es[j] = j < kept ? (int32_t)(base + (uint32_t)par[j]) : none;
    if (lane == 0) f.n_nodes[m] = (int32_t)kept;
}

static int mcts_check_forest(const qg_mcts_forest *f, const char *who) {
    if (!f) return set_error(QG_ERR_INVALID, "null argument");
    if (!f->parent || !f->reward || !f->value || !f->visits || !f->wsum || !f->terminal || !f->child || !f->prior || !f->n_nodes)
        return set_error(QG_ERR_INVALID, "%s: a forest array is null", who);
    if (f->cap < 2 || f->num_actions == 0) return set_error(QG_ERR_INVALID, "%s: bad shape: cap >= 2 (one search) and num_actions >= 1", who);
    if (((uintptr_t)f->parent % 4) || ((uintptr_t)f->reward % 4) || ((uintptr_t)f->value % 4) || ((uintptr_t)f->visits % 4) || ((uintptr_t)f->wsum % 4) ||
        ((uintptr_t)f->child % 4) || ((uintptr_t)f->prior % 4) || ((uintptr_t)f->n_nodes % 4))
        return set_error(QG_ERR_INVALID, "%s: 32-bit arrays must be aligned to their element size", who);
    if (f->num_actions > MCTS_MAX_ACTIONS || f->cap > MCTS_MAX_CAP)
        return set_error(QG_ERR_UNSUPPORTED, "%s: num_actions <= %u and cap <= %u supported", who, MCTS_MAX_ACTIONS, MCTS_MAX_CAP);
    if (f->n_trees > 0x7FFFFFFFull || f->n_trees * f->cap >= 0x7FFFFFFFull) return set_error(QG_ERR_UNSUPPORTED, "%s: too many nodes for 32-bit pool indices", who);
    return QG_OK;
}

// the four output arrays of a selection
static int mcts_check_picked(const int32_t *src, const int32_t *dst, const int32_t *act, const int32_t *leaf) {
    if (!src || !dst || !act || !leaf) return set_error(QG_ERR_INVALID, "null argument");
    if (((uintptr_t)src % 4) || ((uintptr_t)dst % 4) || ((uintptr_t)act % 4) || ((uintptr_t)leaf % 4))
        return set_error(QG_ERR_INVALID, "32-bit arrays must be aligned to their element size");
    return QG_OK;
}

// the operands of a backup; `link`: those of a simulation (the selection's four, reward and done) must be there too
static int mcts_check_operands(const qg_mcts_forest *f, bool link, const int32_t *src, const int32_t *dst, const int32_t *act, const int32_t *leaf,
                               const float *logp, uint64_t ld, const float *values, const float *reward, const uint8_t *done) {
    if (!logp || !values) return set_error(QG_ERR_INVALID, "null argument");
    if (link && (!src || !dst || !act || !leaf || !reward || !done)) return set_error(QG_ERR_INVALID, "null argument");
    if (ld < f->num_actions) return set_error(QG_ERR_INVALID, "bad shape: ld >= num_actions");
    if (((uintptr_t)src % 4) || ((uintptr_t)dst % 4) || ((uintptr_t)act % 4) || ((uintptr_t)leaf % 4) || ((uintptr_t)logp % 4) ||
        ((uintptr_t)values % 4) || ((uintptr_t)reward % 4))
        return set_error(QG_ERR_INVALID, "32-bit arrays must be aligned to their element size");
    return QG_OK;
}

static int mcts_check_many(const qg_mcts_forest *f, uint32_t k, uint32_t stride, const char *who) {
    if (k < 1 || k > stride || stride > plan::MCTS_MAX_LEAVES)
        return set_error(QG_ERR_INVALID, "%s: 1 <= k <= stride <= %u (a descent per lane of the tree's wave)", who, plan::MCTS_MAX_LEAVES);
    if (f->n_trees * stride >= 0x7FFFFFFFull) return set_error(QG_ERR_INVALID, "%s: n_trees * stride must stay below 2^31 - 1", who);
    return QG_OK;
}

}  // namespace qg

using namespace qg;

extern "C" size_t qg_mcts_forest_bytes(uint64_t n_trees, uint32_t cap, uint32_t num_actions) {
    return (size_t)(n_trees * cap * (21ull + 8ull * num_actions) + n_trees * 4ull);
}

extern "C" int qg_mcts_select(const qg_mcts_forest *forest, float c_puct, const uint8_t *finished_dev, int32_t *src_dev, int32_t *dst_dev, int32_t *act_dev,
                              int32_t *leaf_dev, void *stream) {
    if (const int rc = mcts_check_forest(forest, "mcts_select")) return rc;
    if (const int rc = mcts_check_picked(src_dev, dst_dev, act_dev, leaf_dev)) return rc;
    if (forest->n_trees == 0) return QG_OK;
    SelectArgs a;
    a.f = *forest;
    a.finished = finished_dev;
    a.src = src_dev;
    a.dst = dst_dev;
    a.act = act_dev;
    a.leaf = leaf_dev;
    a.C = c_puct;
    static_assert(sizeof(uint2) == plan::MCTS_LDS_NODE_BYTES, "a node's LDS copy");
    a.waves = plan::mcts_trees_per_workgroup(forest->cap);  // trees whose LDS copies fit one workgroup
    const dim3 grid((unsigned)((forest->n_trees + a.waves - 1) / a.waves)), block(64u * a.waves);
    hipLaunchKernelGGL(mcts_select_kernel, grid, block, (size_t)a.waves * forest->cap * sizeof(uint2), (hipStream_t)stream, a);
    HIP_TRY(hipGetLastError());
    return QG_OK;
}

extern "C" int qg_mcts_backup(const qg_mcts_forest *forest, int mode, const int32_t *src_dev, const int32_t *dst_dev, const int32_t *act_dev,
                              const int32_t *leaf_dev, const float *logp_dev, uint64_t ld, const float *values_dev, const float *reward_dev,
                              const uint8_t *done_dev, void *stream) {
    if (const int rc = mcts_check_forest(forest, "mcts_backup")) return rc;
    if (mode != QG_MCTS_ROOT && mode != QG_MCTS_BACKUP) return set_error(QG_ERR_INVALID, "mode must be 0 (root) or 1 (backup)");
    if (const int rc = mcts_check_operands(forest, mode == QG_MCTS_BACKUP, src_dev, dst_dev, act_dev, leaf_dev, logp_dev, ld, values_dev, reward_dev, done_dev)) return rc;
    if (forest->n_trees == 0) return QG_OK;
    BackupArgs a;
    a.f = *forest;
    a.src = src_dev;
    a.dst = dst_dev;
    a.act = act_dev;
    a.leaf = leaf_dev;
    a.logp = logp_dev;
    a.values = values_dev;
    a.reward = reward_dev;
    a.done = done_dev;
    a.ld = ld;
    a.mode = mode;
    const dim3 grid((unsigned)((forest->n_trees + MCTS_WAVES - 1) / MCTS_WAVES)), block(64u * MCTS_WAVES);
    hipLaunchKernelGGL(mcts_backup_kernel, grid, block, 0, (hipStream_t)stream, a);
    HIP_TRY(hipGetLastError());
    return QG_OK;
}

extern "C" int qg_mcts_select_many(const qg_mcts_forest *forest, float c_puct, float virtual_loss, uint32_t k, uint32_t stride, const uint8_t *finished_dev,
                                   int32_t *src_dev, int32_t *dst_dev, int32_t *act_dev, int32_t *leaf_dev, void *stream) {
    if (const int rc = mcts_check_forest(forest, "mcts_select_many")) return rc;
    if (const int rc = mcts_check_many(forest, k, stride, "mcts_select_many")) return rc;
    if (!(virtual_loss >= 0.0f) || virtual_loss > 3.402823466e+38f) return set_error(QG_ERR_INVALID, "mcts_select_many: virtual_loss must be finite and >= 0");
    if (const int rc = mcts_check_picked(src_dev, dst_dev, act_dev, leaf_dev)) return rc;
    if (forest->n_trees == 0) return QG_OK;
    SelectManyArgs a;
    a.f = *forest;
    a.finished = finished_dev;
    a.src = src_dev;
    a.dst = dst_dev;
    a.act = act_dev;
    a.leaf = leaf_dev;
    a.C = c_puct;
    a.vloss = virtual_loss;
    a.k = k;
    a.stride = stride;
    a.waves = plan::mcts_trees_per_workgroup(forest->cap);  // the overlay is qg_mcts_select's LDS copy: the same trees per workgroup
    const dim3 grid((unsigned)((forest->n_trees + a.waves - 1) / a.waves)), block(64u * a.waves);
    hipLaunchKernelGGL(mcts_select_many_kernel, grid, block, (size_t)a.waves * forest->cap * sizeof(uint2), (hipStream_t)stream, a);
    HIP_TRY(hipGetLastError());
    return QG_OK;
}

extern "C" int qg_mcts_backup_many(const qg_mcts_forest *forest, uint32_t k, uint32_t stride, const int32_t *src_dev, const int32_t *dst_dev,
                                   const int32_t *act_dev, const int32_t *leaf_dev, const float *logp_dev, uint64_t ld, const float *values_dev,
                                   const float *reward_dev, const uint8_t *done_dev, void *stream) {
    if (const int rc = mcts_check_forest(forest, "mcts_backup_many")) return rc;
    if (const int rc = mcts_check_many(forest, k, stride, "mcts_backup_many")) return rc;
    if (const int rc = mcts_check_operands(forest, true, src_dev, dst_dev, act_dev, leaf_dev, logp_dev, ld, values_dev, reward_dev, done_dev)) return rc;
    if (forest->n_trees == 0) return QG_OK;
    BackupManyArgs a;
    a.f = *forest;
    a.src = src_dev;
    a.dst = dst_dev;
    a.act = act_dev;
    a.leaf = leaf_dev;
    a.logp = logp_dev;
    a.values = values_dev;
    a.reward = reward_dev;
    a.done = done_dev;
    a.ld = ld;
    a.k = k;
    a.stride = stride;
    const dim3 grid((unsigned)((forest->n_trees + MCTS_WAVES - 1) / MCTS_WAVES)), block(64u * MCTS_WAVES);
    hipLaunchKernelGGL(mcts_backup_many_kernel, grid, block, 0, (hipStream_t)stream, a);
    HIP_TRY(hipGetLastError());
    return QG_OK;
}

extern "C" int qg_mcts_decide(const qg_mcts_forest *forest, int mode, uint64_t seed, uint64_t counter, const uint8_t *finished_dev, int32_t *move_dev,
                              int32_t *counts_dev, uint64_t counts_ld, void *stream) {
    if (const int rc = mcts_check_forest(forest, "mcts_decide")) return rc;
    if (mode != QG_MCTS_MOST_VISITED && mode != QG_MCTS_SAMPLE) return set_error(QG_ERR_INVALID, "mode must be 0 (most visited) or 1 (sample)");
    if (!move_dev) return set_error(QG_ERR_INVALID, "null argument");
    if (((uintptr_t)move_dev % 4) || ((uintptr_t)counts_dev % 4)) return set_error(QG_ERR_INVALID, "32-bit arrays must be aligned to their element size");
    if (counts_dev && counts_ld < forest->num_actions) return set_error(QG_ERR_INVALID, "bad shape: counts_ld >= num_actions");
    if (forest->n_trees == 0) return QG_OK;
    DecideArgs a;
    a.f = *forest;
    a.finished = finished_dev;
    a.move = move_dev;
    a.counts = counts_dev;
    a.counts_ld = counts_ld;
    a.seed = seed;
    a.counter = counter;
    a.mode = mode;
    const dim3 grid((unsigned)((forest->n_trees + MCTS_WAVES - 1) / MCTS_WAVES)), block(64u * MCTS_WAVES);
    hipLaunchKernelGGL(mcts_decide_kernel, grid, block, 0, (hipStream_t)stream, a);
    HIP_TRY(hipGetLastError());
    return QG_OK;
}

extern "C" int qg_mcts_rebase(const qg_mcts_forest *forest, const int32_t *move_dev, const uint8_t *finished_dev, int32_t *env_src_dev, void *stream) {
    if (const int rc = mcts_check_forest(forest, "mcts_rebase")) return rc;
    if (!move_dev || !env_src_dev) return set_error(QG_ERR_INVALID, "null argument");
    if (((uintptr_t)move_dev % 4) || ((uintptr_t)env_src_dev % 4)) return set_error(QG_ERR_INVALID, "32-bit arrays must be aligned to their element size");
    if (forest->n_trees == 0) return QG_OK;
    RebaseArgs a;
    a.f = *forest;
    a.move = move_dev;
    a.finished = finished_dev;
    a.env_src = env_src_dev;
    static_assert(2 * sizeof(int32_t) == plan::MCTS_LDS_NODE_BYTES, "a node's two table entries");
    a.waves = plan::mcts_trees_per_workgroup(forest->cap);  // trees whose two LDS tables fit one workgroup
    const dim3 grid((unsigned)((forest->n_trees + a.waves - 1) / a.waves)), block(64u * a.waves);
    const size_t lds = (size_t)a.waves * forest->cap * 2 * sizeof(int32_t);
    switch (plan::mcts_rebase_slices(forest->num_actions)) {
        case 1: hipLaunchKernelGGL(mcts_rebase_kernel<1>, grid, block, lds, (hipStream_t)stream, a); break;
        case 2: hipLaunchKernelGGL(mcts_rebase_kernel<2>, grid, block, lds, (hipStream_t)stream, a); break;
        case 3: hipLaunchKernelGGL(mcts_rebase_kernel<3>, grid, block, lds, (hipStream_t)stream, a); break;
        default: hipLaunchKernelGGL(mcts_rebase_kernel<4>, grid, block, lds, (hipStream_t)stream, a); break;
    }
    HIP_TRY(hipGetLastError());
    return QG_OK;
}
