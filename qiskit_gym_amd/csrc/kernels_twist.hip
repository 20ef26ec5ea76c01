// kernels_twist.hip -- symmetry views ("twists", Env::twists: clifford.rs:370-372, symmetry.rs:205-295) of a batch, on the device:
//
//   qg_twist_expand_packed / qg_vec_observe_twisted   packed observation -> dense {0,1} tensor seen through a per-env permutation of its entries
//   qg_twist_pack_words / qg_vec_observe_twisted_words   the same view as packed 64-bit row words, what qg_policy_embed_words reads
//   qg_untwist_actions                                 an action chosen on a view -> the real action
//
// The definition (include/qgym.h, proved on the oracle by tests/test_twist_views.py): view_t(obs)[i] = obs[obs_perms[t][i]], a gather; an
// action a chosen on the view is the real action act_perms[t][a].
//
// The view kernel knows no env: rows of packed words, a table of flat source indices.  It is write-bound like qg_expand_packed -- the dense
// output is 8x .. 64x the packed input -- so the mapping is the same: one thread produces one aligned 16-byte chunk of the output (16 / ES
// elements), a wave's store instruction writes 1 KiB contiguously.  What differs is the source of the bits: entry i of a chunk comes from
// bit (src % cols) of row (src / cols), src = obs_perms[t][i], anywhere in the env.  The envs of a workgroup therefore put their packed
// words (<= 2 KiB each) into LDS first, with coalesced loads, and every output entry is one LDS read at an arbitrary address; the table row
// of a chunk is 16 / ES consecutive int32 (16-byte loads; a twist's table is a few KiB and shared by every env that uses it: it stays in
// cache).  src / cols is a multiply-high by a host-made reciprocal (exact for src * cols < 2^32; the limits keep src below 2^19, cols <= 256).
#include "device_common.hpp"
#include "qgym_host.hpp"

namespace qg {

constexpr uint32_t TWIST_MAX_ENV_BYTES = 2048;  // packed words of one env (as qg_beam_merge)
constexpr uint32_t TWIST_BLOCK = 256;

struct TwistArgs {
    const void *packed;     // [B][rows] words
    const int32_t *perms;   // [K][obs]
    const int32_t *twist;   // [B]
    void *out;              // [B][obs] elements
    uint64_t B;
    uint32_t rows, cols, obs;  // obs = rows * cols
    uint32_t K;
    uint32_t recip;         // floor(2^32 / cols) + 1 (unused when cols == 1)
    uint32_t one;           // bit pattern of 1 in the output dtype
    uint32_t cpe;           // 16-byte chunks per env (chunk kernel)
    uint32_t epb;           // envs per workgroup (chunk and words kernels)
    uint32_t rows_out = 0;  // words kernel: 64-bit words per env of the output, rows .. rows_out are zero padding
};

// entry `src` (a flat index below obs) of an env whose words are at w[0 .. rows)
template <typename WT>
__device__ inline uint32_t twist_bit(const WT *w, uint32_t src, const TwistArgs &a) {
    const uint32_t row = a.cols == 1u ? src : __umulhi(src, a.recip);
    const uint32_t col = src - row * a.cols;
    if constexpr (sizeof(WT) == 1) return w[row] == col ? 1u : 0u;  // PermutationEnv rows: the byte is the set column
    else return (uint32_t)(w[row] >> col) & 1u;
}

// obs * ES a multiple of 16, `out` and `perms` 16-byte aligned: an env's output is cpe whole chunks
template <int ES, typename WT>
__global__ __launch_bounds__(TWIST_BLOCK) void twist_chunks_kernel(const TwistArgs a) {
    extern __shared__ uint64_t twist_lds[];
    constexpr uint32_t EPC = 16 / ES;
    WT *w = reinterpret_cast<WT *>(twist_lds);
    const uint32_t tid = threadIdx.x;
    const uint64_t env0 = (uint64_t)blockIdx.x * a.epb;
    const uint32_t n_env = (uint32_t)(a.B - env0 < a.epb ? a.B - env0 : a.epb);  // the grid has no workgroup past the batch
    const WT *src_words = reinterpret_cast<const WT *>(a.packed) + env0 * a.rows;
    for (uint32_t i = tid; i < n_env * a.rows; i += TWIST_BLOCK) w[i] = src_words[i];
    __syncthreads();
    uint4 *out = reinterpret_cast<uint4 *>(a.out) + env0 * a.cpe;
    for (uint32_t c = tid; c < n_env * a.cpe; c += TWIST_BLOCK) {
        const uint32_t le = c / a.cpe, i0 = (c - le * a.cpe) * EPC;
        const uint32_t t = (uint32_t)a.twist[env0 + le];
        const WT *we = w + le * a.rows;
        uint32_t bits = 0;
        if (t < a.K) {
            const uint4 *tp = reinterpret_cast<const uint4 *>(a.perms + (uint64_t)t * a.obs + i0);
#pragma unroll
            for (uint32_t q = 0; q < EPC / 4; ++q) {
                const uint4 v = tp[q];
                const uint32_t s[4] = {v.x, v.y, v.z, v.w};
#pragma unroll
                for (uint32_t k = 0; k < 4; ++k)
                    if (s[k] < a.obs) bits |= twist_bit<WT>(we, s[k], a) << (4 * q + k);  // an entry outside the observation reads as 0
            }
        } else {  // no such twist: the env's own observation
#pragma unroll
            for (uint32_t k = 0; k < EPC; ++k) bits |= twist_bit<WT>(we, i0 + k, a) << k;
        }
        out[c] = expand_chunk<ES>(bits, a.one);
    }
}

// any shape / alignment: one thread per element, the words read through the cache
template <typename T, typename WT>
__global__ __launch_bounds__(TWIST_BLOCK) void twist_elems_kernel(const TwistArgs a, uint64_t total) {
    const uint64_t gid = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (gid >= total) return;
    uint64_t env;
    if (total <= 0xFFFFFFFFull) env = (uint32_t)gid / a.obs;  // 32-bit division: the 64-bit one costs more than the rest of the thread
    else env = gid / a.obs;
    const uint32_t i = (uint32_t)(gid - env * a.obs);
    const uint32_t t = (uint32_t)a.twist[env];
    const uint32_t src = t < a.K ? (uint32_t)a.perms[(uint64_t)t * a.obs + i] : i;
    const WT *w = reinterpret_cast<const WT *>(a.packed) + env * a.rows;
    const uint32_t bit = src < a.obs ? twist_bit<WT>(w, src, a) : 0u;
    reinterpret_cast<T *>(a.out)[gid] = (T)(bit * a.one);
}

// The view as packed words: out[e][r] bit c = entry obs_perms[t][r * cols + c] of env e, a packed -> packed gather.  A workgroup takes epb
// whole envs, their words and twist indices in LDS; its output is one stream of n_env * rows_out words, cut into runs of 64.  A wave makes a
// run: word i of it is one __ballot -- lane c < cols reads its table entry (cols consecutive ints: coalesced, the table stays in cache),
// then its bit from LDS -- and lane i keeps that ballot, so the run leaves as one 512-byte store.  Every index is clamped instead of
// branched on; the compiler re-forms the branches all the same, so a ballot waits for its own table load (EXPERIMENTS.md section 13 has the
// measurement and the next step).  Nothing depends on the geometry: epb only groups envs.
template <typename WT>
__global__ __launch_bounds__(TWIST_BLOCK) void twist_words_kernel(const TwistArgs a) {
    extern __shared__ uint64_t twist_lds[];
    WT *w = reinterpret_cast<WT *>(twist_lds);
    const uint32_t tid = threadIdx.x, lane = tid & 63u;
    const uint64_t env0 = (uint64_t)blockIdx.x * a.epb;
    const uint32_t n_env = (uint32_t)(a.B - env0 < a.epb ? a.B - env0 : a.epb);  // the grid has no workgroup past the batch
    uint32_t *tw = reinterpret_cast<uint32_t *>(twist_lds + ((size_t)a.epb * a.rows * sizeof(WT) + 7u) / 8u);
    const WT *src_words = reinterpret_cast<const WT *>(a.packed) + env0 * a.rows;
    for (uint32_t i = tid; i < n_env * a.rows; i += TWIST_BLOCK) w[i] = src_words[i];
    for (uint32_t i = tid; i < n_env; i += TWIST_BLOCK) tw[i] = (uint32_t)a.twist[env0 + i];
    __syncthreads();
    const uint32_t total = n_env * a.rows_out;  // <= max(256, rows_out) (twist_words_impl)
    uint64_t *out = reinterpret_cast<uint64_t *>(a.out) + env0 * a.rows_out;
    const bool col = lane < a.cols;
    for (uint32_t g0 = (tid >> 6) * 64u; g0 < total; g0 += TWIST_BLOCK) {
        uint32_t le = g0 / a.rows_out, r = g0 - le * a.rows_out;
        uint64_t kept = 0;
#pragma unroll 8
        for (uint32_t i = 0; i < 64u; ++i) {
            const bool valid = col && g0 + i < total && r < a.rows;  // past the stream, a pad word, a lane past the columns: 0
            const uint32_t e = valid ? le : 0u, i0 = valid ? r * a.cols + lane : 0u;
            const uint32_t t = tw[e];
            const uint32_t entry = (uint32_t)a.perms[(uint64_t)(t < a.K ? t : 0u) * a.obs + i0];
            const uint32_t src = t < a.K ? entry : i0;  // no such twist: the env's own observation
            const bool ok = valid && src < a.obs;       // an entry outside the observation reads as 0
            const uint32_t bit = twist_bit<WT>(w + e * a.rows, ok ? src : 0u, a);
            const uint64_t word = __ballot(ok && bit != 0u);
            kept = lane == i ? word : kept;
            if (++r == a.rows_out) {
                r = 0;
                ++le;
            }
        }
        if (g0 + lane < total) out[g0 + lane] = kept;
    }
}

struct UntwistArgs {
    const void *actions;
    const int32_t *perms;  // [K][A]
    const int32_t *twist;  // [B]
    void *out;
    uint64_t B;
    uint32_t A, K;
};

template <typename AT>
__global__ __launch_bounds__(TWIST_BLOCK) void untwist_kernel(const UntwistArgs a) {
    const uint64_t e = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (e >= a.B) return;
    AT act = reinterpret_cast<const AT *>(a.actions)[e];
    const uint32_t t = (uint32_t)a.twist[e];
    if (t < a.K && act >= 0 && act < (AT)a.A) act = (AT)a.perms[(uint64_t)t * a.A + (uint32_t)act];
    reinterpret_cast<AT *>(a.out)[e] = act;
}

template <int ES, typename WT>
static void launch_chunks(const TwistArgs &a, hipStream_t s) {
    const uint64_t grid = (a.B + a.epb - 1) / a.epb;
    const size_t lds = ((size_t)a.epb * a.rows * sizeof(WT) + 7u) & ~(size_t)7u;  // <= 32 KiB + 2 KiB (twist_expand_impl)
    hipLaunchKernelGGL((twist_chunks_kernel<ES, WT>), dim3((unsigned)grid), dim3(TWIST_BLOCK), lds, s, a);
}
template <typename T, typename WT>
static void launch_elems(const TwistArgs &a, hipStream_t s) {
    const uint64_t total = a.B * a.obs;
    hipLaunchKernelGGL((twist_elems_kernel<T, WT>), dim3((unsigned)((total + TWIST_BLOCK - 1) / TWIST_BLOCK)), dim3(TWIST_BLOCK), 0, s, a, total);
}
template <typename WT>
static void launch_twist(const TwistArgs &a, uint32_t es, bool chunks, hipStream_t s) {
    if (chunks) {
        if (es == 1) launch_chunks<1, WT>(a, s);
        else if (es == 2) launch_chunks<2, WT>(a, s);
        else launch_chunks<4, WT>(a, s);
    } else {
        if (es == 1) launch_elems<uint8_t, WT>(a, s);
        else if (es == 2) launch_elems<uint16_t, WT>(a, s);
        else launch_elems<uint32_t, WT>(a, s);
    }
}

int twist_expand_impl(const void *packed_dev, int word_bytes, uint64_t batch, uint32_t rows, uint32_t cols, const int32_t *obs_perms_dev,
                      uint32_t n_twists, const int32_t *twist_idx_dev, void *out_dev, int out_dtype, hipStream_t s) {
    if (!packed_dev || !obs_perms_dev || !twist_idx_dev || !out_dev) return set_error(QG_ERR_INVALID, "null argument");
    uint32_t es = 0, one = 0;
    switch (out_dtype) {
    case QG_DT_I8: es = 1; one = 1u; break;
    case QG_DT_BF16: es = 2; one = 0x3F80u; break;
    case QG_DT_F16: es = 2; one = 0x3C00u; break;
    case QG_DT_F32: es = 4; one = 0x3F800000u; break;
    default: return set_error(QG_ERR_INVALID, "unknown output dtype %d", out_dtype);
    }
    if (word_bytes != 1 && word_bytes != 4 && word_bytes != 8) return set_error(QG_ERR_INVALID, "word_bytes must be 1, 4 or 8");
    if (batch == 0 || rows == 0 || cols == 0 || n_twists == 0) return set_error(QG_ERR_INVALID, "bad shape: batch, rows, cols and n_twists must be positive");
    if ((word_bytes != 1 && cols > (uint32_t)word_bytes * 8u) || (word_bytes == 1 && cols > 256u))
        return set_error(QG_ERR_INVALID, "cols does not fit the packed word");
    if (((uintptr_t)packed_dev % (uintptr_t)word_bytes) || ((uintptr_t)obs_perms_dev % 4) || ((uintptr_t)twist_idx_dev % 4) || ((uintptr_t)out_dev % es))
        return set_error(QG_ERR_INVALID, "words, tables and output must be aligned to their element size");
    if ((uint64_t)rows * (uint64_t)word_bytes > TWIST_MAX_ENV_BYTES)
        return set_error(QG_ERR_UNSUPPORTED, "twist_expand_packed: rows * word_bytes <= %u supported", TWIST_MAX_ENV_BYTES);
    const uint32_t obs = rows * cols;  // <= 2048 * 256
    if (batch > 0x7FFFFFFFull || (uint64_t)n_twists * obs > 0x7FFFFFFFull)
        return set_error(QG_ERR_UNSUPPORTED, "twist_expand_packed: batch < 2^31 and n_twists * rows * cols < 2^31 supported");
    TwistArgs a;
    a.packed = packed_dev;
    a.perms = obs_perms_dev;
    a.twist = twist_idx_dev;
    a.out = out_dev;
    a.B = batch;
    a.rows = rows;
    a.cols = cols;
    a.obs = obs;
    a.K = n_twists;
    a.recip = cols > 1u ? (uint32_t)(0x100000000ull / cols) + 1u : 0u;
    a.one = one;
    const bool chunks = ((uint64_t)obs * es) % 16u == 0 && (((uintptr_t)out_dev | (uintptr_t)obs_perms_dev) & 15u) == 0;
    a.cpe = chunks ? obs * es / 16u : 0u;
    // a workgroup takes whole envs, about one chunk per thread: cpe >= rows * es / 16 >= the env's bytes / 128, so the words of its envs are at
    // most 256 / cpe * 2 KiB <= 32 KiB of LDS (one env's 2 KiB when cpe >= 256)
    a.epb = chunks ? (a.cpe >= TWIST_BLOCK ? 1u : TWIST_BLOCK / a.cpe) : 0u;
    if (!chunks && (batch * obs + TWIST_BLOCK - 1) / TWIST_BLOCK > 0x7FFFFFFFull)
        return set_error(QG_ERR_UNSUPPORTED, "twist_expand_packed: an output that is not made of 16-byte chunks is limited to 2^39 elements");
    switch (word_bytes) {
    case 1: launch_twist<uint8_t>(a, es, chunks, s); break;
    case 4: launch_twist<uint32_t>(a, es, chunks, s); break;
    default: launch_twist<uint64_t>(a, es, chunks, s); break;
    }
    HIP_TRY(hipGetLastError());
    return QG_OK;
}

template <typename WT>
static void launch_words(const TwistArgs &a, hipStream_t s) {
    const uint64_t grid = (a.B + a.epb - 1) / a.epb;
    const size_t lds = (((size_t)a.epb * a.rows * sizeof(WT) + 7u) & ~(size_t)7u) + (size_t)a.epb * sizeof(uint32_t);  // <= 2 KiB + 1 KiB
    hipLaunchKernelGGL((twist_words_kernel<WT>), dim3((unsigned)grid), dim3(TWIST_BLOCK), lds, s, a);
}

int twist_words_impl(const void *packed_dev, int word_bytes, uint64_t batch, uint32_t rows, uint32_t cols, const int32_t *obs_perms_dev,
                     uint32_t n_twists, const int32_t *twist_idx_dev, uint64_t *out_dev, uint32_t rows_out, hipStream_t s) {
    if (!packed_dev || !obs_perms_dev || !twist_idx_dev || !out_dev) return set_error(QG_ERR_INVALID, "null argument");
    if (word_bytes != 1 && word_bytes != 4 && word_bytes != 8) return set_error(QG_ERR_INVALID, "word_bytes must be 1, 4 or 8");
    if (batch == 0 || rows == 0 || cols == 0 || n_twists == 0 || rows_out == 0)
        return set_error(QG_ERR_INVALID, "bad shape: batch, rows, cols, n_twists and rows_out must be positive");
    if ((word_bytes != 1 && cols > (uint32_t)word_bytes * 8u) || (word_bytes == 1 && cols > 256u))
        return set_error(QG_ERR_INVALID, "cols does not fit the packed word");
    if (((uintptr_t)packed_dev % (uintptr_t)word_bytes) || ((uintptr_t)obs_perms_dev % 4) || ((uintptr_t)twist_idx_dev % 4) || ((uintptr_t)out_dev % 8))
        return set_error(QG_ERR_INVALID, "words and tables must be aligned to their element size, the output to 8 bytes");
    if (cols > 64u) return set_error(QG_ERR_UNSUPPORTED, "twist_pack_words: cols <= 64 supported (a row of the view is one 64-bit word)");
    if ((uint64_t)rows * (uint64_t)word_bytes > TWIST_MAX_ENV_BYTES)
        return set_error(QG_ERR_UNSUPPORTED, "twist_pack_words: rows * word_bytes <= %u supported", TWIST_MAX_ENV_BYTES);
    if (rows_out < rows || rows_out > 2u * rows + 2u) return set_error(QG_ERR_UNSUPPORTED, "twist_pack_words: rows <= rows_out <= 2 * rows + 2 supported");
    const uint32_t obs = rows * cols;  // <= 2048 * 64
    if (batch > 0x7FFFFFFFull || (uint64_t)n_twists * obs > 0x7FFFFFFFull)
        return set_error(QG_ERR_UNSUPPORTED, "twist_pack_words: batch < 2^31 and n_twists * rows * cols < 2^31 supported");
    TwistArgs a{};
    a.packed = packed_dev;
    a.perms = obs_perms_dev;
    a.twist = twist_idx_dev;
    a.out = out_dev;
    a.B = batch;
    a.rows = rows;
    a.cols = cols;
    a.obs = obs;
    a.K = n_twists;
    a.recip = cols > 1u ? (uint32_t)(0x100000000ull / cols) + 1u : 0u;
    a.rows_out = rows_out;
    // a workgroup takes whole envs, about one run of 64 words per wave: at most 256 envs, and rows * word_bytes <= 8 * rows_out, so the words
    // of its envs are at most 256 / rows_out * 8 * rows_out = 2 KiB of LDS (one env's 2 KiB when rows_out >= 256), their twist indices 1 KiB
    a.epb = rows_out >= TWIST_BLOCK ? 1u : TWIST_BLOCK / rows_out;
    switch (word_bytes) {
    case 1: launch_words<uint8_t>(a, s); break;
    case 4: launch_words<uint32_t>(a, s); break;
    default: launch_words<uint64_t>(a, s); break;
    }
    HIP_TRY(hipGetLastError());
    return QG_OK;
}

}  // namespace qg

using namespace qg;

extern "C" int qg_twist_expand_packed(const void *packed_dev, int word_bytes, uint64_t batch, uint32_t rows, uint32_t cols, const int32_t *obs_perms_dev,
                                      uint32_t n_twists, const int32_t *twist_idx_dev, void *out_dev, int out_dtype, void *stream) {
    return twist_expand_impl(packed_dev, word_bytes, batch, rows, cols, obs_perms_dev, n_twists, twist_idx_dev, out_dev, out_dtype, (hipStream_t)stream);
}

extern "C" int qg_twist_pack_words(const void *packed_dev, int word_bytes, uint64_t batch, uint32_t rows, uint32_t cols, const int32_t *obs_perms_dev,
                                   uint32_t n_twists, const int32_t *twist_idx_dev, uint64_t *out_dev, uint32_t rows_out, void *stream) {
    return twist_words_impl(packed_dev, word_bytes, batch, rows, cols, obs_perms_dev, n_twists, twist_idx_dev, out_dev, rows_out, (hipStream_t)stream);
}

extern "C" int qg_untwist_actions(const void *actions_dev, int action_dtype, uint64_t batch, uint32_t num_actions, const int32_t *act_perms_dev,
                                  uint32_t n_twists, const int32_t *twist_idx_dev, void *out_dev, void *stream) {
    if (!actions_dev || !act_perms_dev || !twist_idx_dev || !out_dev) return set_error(QG_ERR_INVALID, "null argument");
    if (action_dtype != QG_ACT_I32 && action_dtype != QG_ACT_I64) return set_error(QG_ERR_INVALID, "bad action dtype");
    if (batch == 0 || num_actions == 0 || n_twists == 0) return set_error(QG_ERR_INVALID, "bad shape: batch, num_actions and n_twists must be positive");
    if (num_actions > 0x7FFFFFFFu || batch > 0x7FFFFFFFull * TWIST_BLOCK)
        return set_error(QG_ERR_UNSUPPORTED, "untwist_actions: num_actions < 2^31 and batch < 2^39 supported");
    UntwistArgs a;
    a.actions = actions_dev;
    a.perms = act_perms_dev;
    a.twist = twist_idx_dev;
    a.out = out_dev;
    a.B = batch;
    a.A = num_actions;
    a.K = n_twists;
    const dim3 grid((unsigned)((batch + TWIST_BLOCK - 1) / TWIST_BLOCK)), block(TWIST_BLOCK);
    if (action_dtype == QG_ACT_I64) hipLaunchKernelGGL(untwist_kernel<int64_t>, grid, block, 0, (hipStream_t)stream, a);
    else hipLaunchKernelGGL(untwist_kernel<int32_t>, grid, block, 0, (hipStream_t)stream, a);
    HIP_TRY(hipGetLastError());
    return QG_OK;
}
