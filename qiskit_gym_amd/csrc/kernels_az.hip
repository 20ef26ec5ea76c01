// kernels_az.hip -- qg_az_pack: the log of a finished batch of self-play episodes (per decision and episode the root's visit counts that
// qg_mcts_decide wrote, the real env's reward, the move, a live flag and optionally the packed observation) -> a dense batch of training
// samples for an AlphaZero-style learner: the live decisions compacted in (decision, episode) order, the counts normalised to pi, the
// undiscounted return to go as z.  The rules are stated in include/qgym.h; tests/azmodel.py restates them in numpy and the kernels agree
// with it bit for bit.  Like the search kernels this file knows no env and no policy.
//
// Four launches on one stream, no host read between them, no workgroup ever waits for another:
//   1  az_mark_kernel     a workgroup per CHUNK of 256 (t, e) items, a wave per 64 of them: the live flags in one coalesced load, then per
//                         live item the row of counts by the whole wave (four actions per lane, as in kernels_mcts.hip) -> total, bad.
//                         Lane l keeps item l's result; the row totals go to scratch (0: not valid), the numbers of valid and of bad
//                         items of the wave are a ballot and a popcount, of the workgroup a sum over LDS -> scratch, one pair per chunk.
//                         A dead item's row is never read: the counts log is the traffic, and a self-play log is mostly dead rows.
//   2  az_return_kernel   a lane per episode, t = T-1 .. 0: G = reward + G where live (one f32 addition; -ffp-contract=off), read and written
//                         coalesced across e.  Independent of 1.
//   3  az_scan_kernel     ONE workgroup: the exclusive prefix sums of the per-chunk valid counts, in place, 256 chunks per pass (a shifted-add
//                         scan within a wave, LDS across the waves, the running sum in a register), the sum of the bad counts, and n[3].
//   4  az_write_kernel    the geometry of 1: an item's rank = its chunk's offset + the valid items of the earlier waves of the workgroup (LDS)
//                         + the valid lanes below it (ballot, popcount).  index, z and move: a lane per item.  pi and the words: per valid
//                         item of rank < capacity the whole wave on its row -- the second and last read of a VALID row, nothing else is
//                         read twice.  A chunk whose offset is at or past capacity returns at once.
// Integer arithmetic decides everything but pi and z, so the result does not depend on the launch geometry; pi is one correctly rounded
// f32 division per entry (the plain `/` of this build, as in qg_mcts_select), z the f32 sums in the one order the rules give.
//
// A row's total: a row with a count < 0 or >= 2^24 is bad whatever the rest holds (the total of non-negative counts is at least each of
// them), and otherwise at most 256 counts below 2^24 sum to less than 2^32 -- so the 64-bit rule of the header is a u32 sum here.
#include "device_common.hpp"
#include "qgym_host.hpp"

namespace qg {

constexpr uint32_t AZ_WAVES = 4;                    // waves per workgroup of launches 1 and 4
constexpr uint32_t AZ_CHUNK = QG_WAVE * AZ_WAVES;   // items per workgroup: a lane per item
constexpr uint32_t AZ_SCAN_THREADS = 256;           // launch 3: chunks per pass
constexpr uint32_t AZ_RETURN_THREADS = 256;         // launch 2: episodes per workgroup
constexpr uint32_t AZ_MAX_ACTIONS = 256;            // four actions per lane
constexpr uint32_t AZ_MAX_WORD_BYTES = 2048;        // a sample's packed observation
constexpr uint32_t AZ_TOTAL_LIMIT = 1u << 24;       // f32(total) is exact below it

struct AzArgs {
    const int32_t *counts;
    const float *reward;
    const uint8_t *live;
    const int32_t *move;
    const void *words;  // or nullptr
    int32_t *n, *index, *move_out;
    float *z, *pi;
    void *words_out;
    uint32_t *tot;             // scratch [items]: the row's total, 0: no sample
    float *ret;                // scratch [items]: G(t, e) where live
    uint32_t *chunk_valid;     // scratch [chunks]: valid items, after launch 3 those of the chunks before
    uint32_t *chunk_bad;       // scratch [chunks]
    uint64_t counts_ld, pi_ld, capacity;
    uint32_t items, chunks, T, E, A, W, word_bytes;
};

__device__ inline uint32_t az_wave_sum(uint32_t v) {
#pragma unroll
    for (int off = 32; off >= 1; off >>= 1) v += (uint32_t)__shfl_xor((int)v, off, 64);
    return v;
}

__global__ __launch_bounds__(AZ_CHUNK) void az_mark_kernel(const AzArgs a) {
    __shared__ uint32_t part[AZ_WAVES][2];
    const uint32_t lane = threadIdx.x & (QG_WAVE - 1), wave = threadIdx.x >> 6;
    const uint64_t item = (uint64_t)blockIdx.x * AZ_CHUNK + threadIdx.x;  // < 2^31 + 256
    const bool alive = item < a.items && a.live[item] != 0;
    uint32_t my_tot = 0;
    bool my_bad = false;
    for (uint64_t todo = __ballot(alive); todo; todo &= todo - 1) {  // the wave's live items, one row each
        const uint32_t r = (uint32_t)__builtin_ctzll(todo);
        const int32_t *row = a.counts + (item - lane + r) * a.counts_ld;
        uint32_t sum = 0;
        bool bad = false;
#pragma unroll
        for (uint32_t k = 0; k < 4; ++k) {
            const uint32_t ac = lane + QG_WAVE * k;
            const int32_t c = ac < a.A ? row[ac] : 0;
            bad |= c < 0 || (uint32_t)c >= AZ_TOTAL_LIMIT;
            sum += (uint32_t)c;
        }
        const bool row_bad = __ballot(bad) != 0;
        const uint32_t total = row_bad ? 0u : az_wave_sum(sum);  // < 2^32: 256 counts below 2^24
        if (lane == r) {
            my_bad = row_bad || total >= AZ_TOTAL_LIMIT;
            my_tot = my_bad ? 0u : total;
        }
    }
    if (item < a.items) a.tot[item] = my_tot;
    const uint32_t valid = (uint32_t)__popcll(__ballot(my_tot != 0)), bads = (uint32_t)__popcll(__ballot(my_bad));
    if (lane == 0) {
        part[wave][0] = valid;
        part[wave][1] = bads;
    }
    __syncthreads();
    if (threadIdx.x == 0) {
        uint32_t v = 0, b = 0;
#pragma unroll
        for (uint32_t w = 0; w < AZ_WAVES; ++w) {
            v += part[w][0];
            b += part[w][1];
        }
        a.chunk_valid[blockIdx.x] = v;
        a.chunk_bad[blockIdx.x] = b;
    }
}

__global__ __launch_bounds__(AZ_RETURN_THREADS) void az_return_kernel(const AzArgs a) {
    const uint64_t e = (uint64_t)blockIdx.x * AZ_RETURN_THREADS + threadIdx.x;
    if (e >= a.E) return;
    float g = 0.0f;
    for (uint32_t t = a.T; t-- > 0;) {
        const uint64_t at = (uint64_t)t * a.E + e;
        if (a.live[at] != 0) {
            g = a.reward[at] + g;
            a.ret[at] = g;
        }
    }
}

__global__ __launch_bounds__(AZ_SCAN_THREADS) void az_scan_kernel(const AzArgs a) {
    constexpr uint32_t WAVES = AZ_SCAN_THREADS / QG_WAVE;
    __shared__ uint32_t part[WAVES][2];
    const uint32_t lane = threadIdx.x & (QG_WAVE - 1), wave = threadIdx.x >> 6;
    uint32_t before = 0, bad = 0;  // the valid and the bad items of the passes so far (at most items < 2^31)
    for (uint32_t c0 = 0; c0 < a.chunks; c0 += AZ_SCAN_THREADS) {
        const uint32_t c = c0 + threadIdx.x;
        const uint32_t v = c < a.chunks ? a.chunk_valid[c] : 0u;
        const uint32_t b = az_wave_sum(c < a.chunks ? a.chunk_bad[c] : 0u);
        uint32_t incl = v;  // inclusive sums over the lanes, in lane order
#pragma unroll
        for (int off = 1; off < 64; off <<= 1) {
            const uint32_t o = (uint32_t)__shfl_up((int)incl, off, 64);
            if (lane >= (uint32_t)off) incl += o;
        }
        if (lane == QG_WAVE - 1) {
            part[wave][0] = incl;
            part[wave][1] = b;
        }
        __syncthreads();
        uint32_t lower = 0, all = 0;
#pragma unroll
        for (uint32_t w = 0; w < WAVES; ++w) {
            if (w < wave) lower += part[w][0];
            all += part[w][0];
            bad += part[w][1];
        }
        if (c < a.chunks) a.chunk_valid[c] = before + lower + incl - v;
        before += all;
        __syncthreads();  // the table is read before the next pass writes it
    }
    if (threadIdx.x == 0) {
        a.n[0] = (int32_t)((uint64_t)before < a.capacity ? before : (uint32_t)a.capacity);
        a.n[1] = (int32_t)before;
        a.n[2] = (int32_t)bad;
    }
}

template <typename Word>
__device__ inline void az_copy_words(const void *from, void *to, uint64_t src_row, uint64_t dst_row, uint32_t W, uint32_t lane) {
    const Word *s = (const Word *)from + src_row * W;
    Word *d = (Word *)to + dst_row * W;
    for (uint32_t j = lane; j < W; j += QG_WAVE) d[j] = s[j];
}

__global__ __launch_bounds__(AZ_CHUNK) void az_write_kernel(const AzArgs a) {
    __shared__ uint32_t part[AZ_WAVES];
    const uint64_t first = a.chunk_valid[blockIdx.x];  // the rank of the chunk's first sample
    if (first >= a.capacity) return;                   // (the whole workgroup) ranks ascend: nothing of this chunk is written
    const uint32_t lane = threadIdx.x & (QG_WAVE - 1), wave = threadIdx.x >> 6;
    const uint64_t item = (uint64_t)blockIdx.x * AZ_CHUNK + threadIdx.x;
    const uint32_t tot = item < a.items ? a.tot[item] : 0u;
    const uint64_t mask = __ballot(tot != 0);
    if (lane == 0) part[wave] = (uint32_t)__popcll(mask);
    __syncthreads();
    uint64_t base = first;
#pragma unroll
    for (uint32_t w = 0; w < AZ_WAVES; ++w)
        if (w < wave) base += part[w];
    const uint64_t rank = base + (uint32_t)__popcll(mask & ((1ull << lane) - 1ull));
    if (tot != 0 && rank < a.capacity) {
        a.index[rank] = (int32_t)item;
        a.z[rank] = a.ret[item];
        a.move_out[rank] = a.move[item];
    }
    uint64_t at = base;  // the rank of the wave's next sample
    for (uint64_t todo = mask; todo && at < a.capacity; todo &= todo - 1, ++at) {
        const uint32_t r = (uint32_t)__builtin_ctzll(todo);
        const uint64_t src = item - lane + r;
        const float total = (float)__shfl((int)tot, (int)r, 64);  // exact: below 2^24
        const int32_t *row = a.counts + src * a.counts_ld;
        float *out = a.pi + at * a.pi_ld;
        int32_t c[4];
#pragma unroll
        for (uint32_t k = 0; k < 4; ++k) {
            const uint32_t ac = lane + QG_WAVE * k;
            c[k] = ac < a.A ? row[ac] : 0;
        }
#pragma unroll
        for (uint32_t k = 0; k < 4; ++k) {
            const uint32_t ac = lane + QG_WAVE * k;
            if (ac < a.A) out[ac] = (float)c[k] / total;
        }
        if (a.words) {
            if (a.word_bytes == 8) az_copy_words<uint64_t>(a.words, a.words_out, src, at, a.W, lane);
            else if (a.word_bytes == 4) az_copy_words<uint32_t>(a.words, a.words_out, src, at, a.W, lane);
            else az_copy_words<uint8_t>(a.words, a.words_out, src, at, a.W, lane);
        }
    }
}

static uint64_t az_chunks(uint64_t items) { return (items + AZ_CHUNK - 1) / AZ_CHUNK; }

}  // namespace qg

using namespace qg;

extern "C" size_t qg_az_pack_scratch_bytes(uint64_t T, uint64_t E) {
    if (T == 0 || E == 0 || T >= 0x7FFFFFFFull || E >= 0x7FFFFFFFull || T * E >= 0x7FFFFFFFull) return 0;
    return (size_t)(T * E * 8ull + az_chunks(T * E) * 8ull);
}

extern "C" int qg_az_pack(const int32_t *counts_dev, uint64_t counts_ld, const float *reward_dev, const uint8_t *live_dev, const int32_t *move_dev,
                          const void *words_dev, int word_bytes, uint32_t W, uint64_t T, uint64_t E, uint32_t num_actions, uint64_t capacity,
                          int32_t *n_dev, int32_t *index_dev, float *z_dev, int32_t *move_out_dev, float *pi_dev, uint64_t pi_ld, void *words_out_dev,
                          void *scratch_dev, void *stream) {
    if (!counts_dev || !reward_dev || !live_dev || !move_dev || !n_dev || !index_dev || !z_dev || !move_out_dev || !pi_dev || !scratch_dev)
        return set_error(QG_ERR_INVALID, "az_pack: null argument");
    if (T == 0 || E == 0 || num_actions == 0 || capacity == 0) return set_error(QG_ERR_INVALID, "az_pack: bad shape: T, E, num_actions and capacity >= 1");
    if (counts_ld < num_actions || pi_ld < num_actions) return set_error(QG_ERR_INVALID, "az_pack: bad shape: counts_ld and pi_ld >= num_actions");
    if (words_dev) {
        if (word_bytes != 1 && word_bytes != 4 && word_bytes != 8) return set_error(QG_ERR_INVALID, "az_pack: word_bytes must be 1, 4 or 8");
        if (!words_out_dev) return set_error(QG_ERR_INVALID, "az_pack: words_dev without words_out_dev");
        if (W == 0) return set_error(QG_ERR_INVALID, "az_pack: bad shape: W >= 1 with words_dev");
        if (((uintptr_t)words_dev % (unsigned)word_bytes) || ((uintptr_t)words_out_dev % (unsigned)word_bytes))
            return set_error(QG_ERR_INVALID, "az_pack: the words must be aligned to word_bytes");
    }
    if (((uintptr_t)counts_dev % 4) || ((uintptr_t)reward_dev % 4) || ((uintptr_t)move_dev % 4) || ((uintptr_t)n_dev % 4) || ((uintptr_t)index_dev % 4) ||
        ((uintptr_t)z_dev % 4) || ((uintptr_t)move_out_dev % 4) || ((uintptr_t)pi_dev % 4) || ((uintptr_t)scratch_dev % 4))
        return set_error(QG_ERR_INVALID, "az_pack: 32-bit arrays must be aligned to their element size");
    if (num_actions > AZ_MAX_ACTIONS) return set_error(QG_ERR_UNSUPPORTED, "az_pack: num_actions <= %u supported", AZ_MAX_ACTIONS);
    if (T >= 0x7FFFFFFFull || E >= 0x7FFFFFFFull || T * E >= 0x7FFFFFFFull) return set_error(QG_ERR_UNSUPPORTED, "az_pack: T * E must stay below 2^31 - 1");
    if (words_dev && (uint64_t)W * (uint64_t)word_bytes > AZ_MAX_WORD_BYTES)
        return set_error(QG_ERR_UNSUPPORTED, "az_pack: W * word_bytes <= %u supported", AZ_MAX_WORD_BYTES);
    AzArgs a;
    a.counts = counts_dev;
    a.reward = reward_dev;
    a.live = live_dev;
    a.move = move_dev;
    a.words = words_dev;
    a.n = n_dev;
    a.index = index_dev;
    a.move_out = move_out_dev;
    a.z = z_dev;
    a.pi = pi_dev;
    a.words_out = words_out_dev;
    a.items = (uint32_t)(T * E);
    a.chunks = (uint32_t)az_chunks(T * E);
    a.tot = (uint32_t *)scratch_dev;
    a.ret = (float *)(a.tot + a.items);
    a.chunk_valid = (uint32_t *)(a.ret + a.items);
    a.chunk_bad = a.chunk_valid + a.chunks;
    a.counts_ld = counts_ld;
    a.pi_ld = pi_ld;
    a.capacity = capacity;
    a.T = (uint32_t)T;
    a.E = (uint32_t)E;
    a.A = num_actions;
    a.W = words_dev ? W : 0u;
    a.word_bytes = words_dev ? (uint32_t)word_bytes : 0u;
    hipStream_t s = (hipStream_t)stream;
    hipLaunchKernelGGL(az_mark_kernel, dim3(a.chunks), dim3(AZ_CHUNK), 0, s, a);
    HIP_TRY(hipGetLastError());
    hipLaunchKernelGGL(az_return_kernel, dim3((unsigned)((E + AZ_RETURN_THREADS - 1) / AZ_RETURN_THREADS)), dim3(AZ_RETURN_THREADS), 0, s, a);
    HIP_TRY(hipGetLastError());
    hipLaunchKernelGGL(az_scan_kernel, dim3(1), dim3(AZ_SCAN_THREADS), 0, s, a);
    HIP_TRY(hipGetLastError());
    hipLaunchKernelGGL(az_write_kernel, dim3(a.chunks), dim3(AZ_CHUNK), 0, s, a);
    HIP_TRY(hipGetLastError());
    return QG_OK;
}
