// Device-only: the owner-computes node sum shared by the gather kernels of kernels_assembly.hip and kernels_explicit.hip.
#pragma once
#include "load_row.hpp"

namespace femcy {

// Half a wavefront (32 lanes) owns a node: thread t of the grid is lane sub = t & 31 of node a = t >> 5, so a launch needs
// node_gather_grid(nn, block) workgroups.
inline unsigned node_gather_grid(int32_t nn, int block) { return (unsigned)(((int64_t)nn * 32 + block - 1) / block); }

// sum[0..W) = the sum over node a's incident rows k = ne_ptr[a] .. ne_ptr[a + 1] - 1 of the W doubles at src + ne_idx[k] * W
// (ne_idx = e * npe + la: the row of a per-element record).  Lane sub takes the rows sub, sub + 32, ... in ascending order,
// one load_row each (W = 1: one 8-byte load) side by side instead of one dependent load chain; the partial sums are combined
// by a fixed xor tree over the 32 lanes: no atomics, the same bits on every run.  Every level adds the same two values in both
// lanes of a pair, so the tree leaves the same bits in all 32 lanes.  All 32 lanes of a node must call it, a >= nn included
// (those sum nothing).
template <int W>
__device__ __forceinline__ void node_gather(int32_t a, int sub, int32_t nn, const int32_t* __restrict__ ne_ptr,
                                            const int32_t* __restrict__ ne_idx, const double* __restrict__ src,
                                            double (&sum)[W]) {
#pragma unroll
    for (int c = 0; c < W; ++c) sum[c] = 0.0;
    if (a < nn) {
        const int32_t k1 = ne_ptr[a + 1];
        for (int32_t k = ne_ptr[a] + sub; k < k1; k += 32) {
            if constexpr (W == 1) {
                sum[0] += src[ne_idx[k]];
            } else {
                double rv[W];
                load_row<W>(src + (int64_t)ne_idx[k] * W, rv);
#pragma unroll
                for (int c = 0; c < W; ++c) sum[c] += rv[c];
            }
        }
    }
#pragma unroll
    for (int o = 16; o > 0; o >>= 1)
#pragma unroll
        for (int c = 0; c < W; ++c) sum[c] += __shfl_xor(sum[c], o, 32);
}

}  // namespace femcy
