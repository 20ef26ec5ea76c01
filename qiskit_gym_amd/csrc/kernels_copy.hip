// kernels_copy.hip -- qg_vec_copy_envs: the batched Env::clone (clifford.rs:179, linear_function.rs:154 and permutation.rs:29
// derive(Clone); pauli.rs:307-337).  Env dst_idx[i] becomes a copy of env src_idx[i]: every resident buffer the env owns -- the state's
// regions (qgym_plan.hpp copy_layout), depth, reward, flags, fault word, `bad` mask, solution log, layer records, PauliEnv's
// current_perm_idx -- is a set of rows of 64 lanes (CopyRegionArgs), so one gather kernel walks them all: workgroup row y = one region,
// thread = one copied env.  Lanes of consecutive entries with consecutive destinations store to consecutive addresses; the sources may lie
// anywhere.  Plain vector loads and stores only.
#include "device_common.hpp"

namespace qg {

template <uint32_t W>
__device__ inline void copy_lane(char *dst, const char *src) {
    if constexpr (W == 16) {
        *reinterpret_cast<uint4 *>(dst) = *reinterpret_cast<const uint4 *>(src);
    } else if constexpr (W == 12) {
        const uint32_t *s = reinterpret_cast<const uint32_t *>(src);
        uint32_t *d = reinterpret_cast<uint32_t *>(dst);
        const uint32_t a = s[0], b = s[1], c = s[2];
        d[0] = a; d[1] = b; d[2] = c;
    } else if constexpr (W == 8) {
        *reinterpret_cast<uint2 *>(dst) = *reinterpret_cast<const uint2 *>(src);
    } else if constexpr (W == 4) {
        *reinterpret_cast<uint32_t *>(dst) = *reinterpret_cast<const uint32_t *>(src);
    } else {
        *dst = *src;
    }
}

template <uint32_t W>
__device__ inline void copy_rows(const CopyRegionArgs &r, uint64_t s, uint64_t d) {
    const char *src = r.src + (s >> 6) * r.tile_bytes + (s & 63u) * W;
    char *dst = r.dst + (d >> 6) * r.tile_bytes + (d & 63u) * W;
    for (uint32_t k = 0; k < r.rows; ++k) copy_lane<W>(dst + k * r.pitch_dst, src + k * r.pitch_src);
}

// TILE state with a tracked dense observation: each 16-byte group holds row slots 4g .. 4g+3; slot -> matrix row as kernels_qm.hip lays them
// out (CliffordEnv: X row j in slot 2j, Z row N + j in slot 2j + 1), row r of env e at dense[(e * D + r) * D] (qg_vec_track_dense)
template <int D16>
__device__ inline void copy_tile_dense(const CopyArgs &a, uint64_t s, uint64_t d) {
    const CopyRegionArgs &r = a.r[0];
    const uint4 *src = reinterpret_cast<const uint4 *>(r.src + (s >> 6) * r.tile_bytes) + (s & 63u);
    uint4 *dst = reinterpret_cast<uint4 *>(r.dst + (d >> 6) * r.tile_bytes) + (d & 63u);
    for (uint32_t g = 0; g < r.rows; ++g) {
        const uint4 q = src[g * 64u];
        dst[g * 64u] = q;
        const uint32_t w[4] = {q.x, q.y, q.z, q.w};
#pragma unroll
        for (uint32_t k = 0; k < 4; ++k) {
            const uint32_t slot = 4u * g + k;
            const uint32_t row = a.has_z ? ((slot & 1u) ? a.N + (slot >> 1) : slot >> 1) : slot;
            dense_row_store<D16>(a.dense, d, row, w[k]);
        }
    }
}

__global__ __launch_bounds__(256) void copy_envs_kernel(const CopyArgs a) {
    const uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= a.n) return;
    const uint64_t s = a.src_idx[i];
    const uint64_t d = a.dst_idx ? (uint64_t)a.dst_idx[i] : i;
    if (s >= a.B_src || d >= a.B_dst) return;
    const CopyRegionArgs &r = a.r[blockIdx.y];
    if (blockIdx.y == 0 && a.dense) {
        if (a.D == 16) copy_tile_dense<1>(a, s, d);
        else copy_tile_dense<2>(a, s, d);
        return;
    }
    switch (r.w) {
    case 16: copy_rows<16>(r, s, d); break;
    case 12: copy_rows<12>(r, s, d); break;
    case 8: copy_rows<8>(r, s, d); break;
    case 4: copy_rows<4>(r, s, d); break;
    default: copy_rows<1>(r, s, d); break;
    }
}

hipError_t copy_envs(const CopyArgs &a, hipStream_t s) {
    if (!a.n || !a.n_regions) return hipSuccess;
    const dim3 grid((unsigned)((a.n + 255) / 256), a.n_regions), block(256);
    hipLaunchKernelGGL(copy_envs_kernel, grid, block, 0, s, a);
    return hipGetLastError();
}

}  // namespace qg
