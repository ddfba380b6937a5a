// Tagged-granule exchange between the workgroups of one persistent launch (k_pcg_persist, k_probe_exchange).
// A granule is one naturally aligned 16-byte {f64 value, u64 tag} written by ONE sc1 store (observed untorn on
// gfx950, MI355X_MICROARCH.md "Valid forms": R2); the tag is a launch-wide round number (1, 2, 3, ...; the arrays are
// zeroed before the launch), so a granule validates itself: no counter, no flag, no re-arming.  A workgroup may write
// round k + 1 of an array only after every workgroup has read round k of it -- the callers rotate arrays so that an
// exchange in between guarantees that.  Every sweep is bounded; TAG_POISON releases everybody with the same verdict.
#pragma once
#include <hip/hip_runtime.h>
#include "wave_reduce.hpp"

#if defined(__HIP_DEVICE_COMPILE__) && !defined(__gfx950__) && !defined(__gfx942__)
#error "the sc1-only hand-off protocols of the one-launch PCG kernels are validated for gfx942 / gfx950 only"
#endif

namespace femcy {

typedef unsigned int u32x2 __attribute__((ext_vector_type(2)));
typedef unsigned int u32x4 __attribute__((ext_vector_type(4)));
constexpr int AUX_SC1 = 16;     // gfx940+ buffer cache-policy bit 4: sc1 = write-through store / L2-served load
constexpr unsigned long long TAG_POISON = ~0ull;

__device__ __forceinline__ void granule_store(const __amdgpu_buffer_rsrc_t rs, int idx, double v, unsigned long long tag) {
    u32x4 w;
    w.x = (unsigned)__double2loint(v);
    w.y = (unsigned)__double2hiint(v);
    w.z = (unsigned)tag;
    w.w = (unsigned)(tag >> 32);
    __builtin_amdgcn_raw_buffer_store_b128(w, rs, idx * 16, 0, AUX_SC1);
}
// ONE wave sweeps: NV granules per workgroup, stored [G][NV]; lane sweeps workgroups lane, lane + 64, ...; sums /
// maxima in a fixed order (the same in every workgroup).  op[v]: 0 = sum, 1 = max.  Returns false on poison or
// time-out (the caller's workgroup then poisons its own granules, which every other sweep sees).
//
// A sweep is ONE load round trip: the SWEEP_ROWS * NV loads of a chunk (SWEEP_ROWS rows of 64 workgroups = 256
// workgroups, the whole grid of a 256-CU device) are issued back to back into registers and examined behind a single
// wait.  Written as `for (k = lane; k < G; k += 64)` the loop is divergent with a run-time trip count, the compiler
// keeps it rolled with s_waitcnt vmcnt(0) behind every load, and a sweep of 256 workgroups is four DEPENDENT sc1
// round trips -- paid once more, in full, after the last granule has become visible.  A lane whose workgroup index is
// >= G loads a clamped, in-range granule and a select discards it: it counts as "tag matches" and leaves the lane's
// sum / maximum as it is.  The order of combination is what it was (per lane ascending k, then across the wave).
constexpr int SWEEP_ROWS = 4;
template <int NV>
__device__ __forceinline__ bool granule_sweep(const __amdgpu_buffer_rsrc_t rs, int base, int G, unsigned long long tag,
                                              uint32_t spin_limit, double (&out)[NV], const int (&op)[NV]) {
    const int lane = threadIdx.x & 63;
    uint32_t spins = 0;
    for (;;) {
        double acc[NV];
#pragma unroll
        for (int v = 0; v < NV; ++v) acc[v] = 0.0;
        bool ok = true, poison = false;
        for (int k0 = 0; k0 < G; k0 += 64 * SWEEP_ROWS) {          // wave-uniform; a second chunk only when G > 256
            u32x4 w[SWEEP_ROWS][NV];
#pragma unroll
            for (int j = 0; j < SWEEP_ROWS; ++j) {
                const int kc = min(k0 + 64 * j + lane, G - 1);
#pragma unroll
                for (int v = 0; v < NV; ++v)
                    w[j][v] = __builtin_amdgcn_raw_buffer_load_b128(rs, (base + kc * NV + v) * 16, 0, AUX_SC1);
            }
#pragma unroll
            for (int j = 0; j < SWEEP_ROWS; ++j) {
                const bool in = k0 + 64 * j + lane < G;
#pragma unroll
                for (int v = 0; v < NV; ++v) {
                    const unsigned long long t = ((unsigned long long)w[j][v].w << 32) | w[j][v].z;
                    ok = ok && (!in || t == tag);
                    poison = poison || (in && t == TAG_POISON);
                    const double val = __hiloint2double((int)w[j][v].y, (int)w[j][v].x);
                    const double comb = op[v] ? fmax(acc[v], val) : acc[v] + val;
                    acc[v] = in ? comb : acc[v];
                }
            }
        }
        if (__any(poison)) return false;
        if (__all(ok)) {
#pragma unroll
            for (int v = 0; v < NV; ++v) out[v] = op[v] ? wave_max(acc[v]) : wave_sum(acc[v]);
            return true;
        }
        // the re-poll, measured with femcy_probe_exchange(2000, 1) on the one-round-trip sweep (2.14-2.18 us per exchange,
        // spread of repeated runs 0.04): without this sleep 2.16 -- no gain; a second sweep issued while the first is
        // in flight (examined behind s_waitcnt vmcnt(N) on the older half) 2.29-2.30 -- slower, twice the poll traffic
        __builtin_amdgcn_s_sleep(1);      // 64 cycles between sweeps
        if (++spins > spin_limit) return false;
    }
}

}  // namespace femcy
