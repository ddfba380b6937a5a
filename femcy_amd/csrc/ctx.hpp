// Internal state of one femcy context (one HIP device + one stream).  Not part of the ABI.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <stdlib.h>
#include <mutex>
#include <string>
#include <vector>
#include "../../include/femcy.h"
#include "api_checks.hpp"   // set_error, FEMCY_REQUIRE and what the entry points refuse
#include "element_math.hpp" // ExplicitClock, Amplitude

namespace femcy {

#define FEMCY_HIP(call)                                                                         \
    do {                                                                                        \
        hipError_t _e = (call);                                                                 \
        if (_e != hipSuccess) {                                                                 \
            femcy::set_error("%s failed: %s (%s:%d)", #call, hipGetErrorString(_e), __FILE__, __LINE__); \
            return FEMCY_EHIP;                                                                  \
        }                                                                                       \
    } while (0)

// Every device allocation of the library goes through dmalloc.  FEMCY_DEBUG_POISON=1 (environment, read once) fills
// each one with 0xFF bytes (a NaN as f64, -1 as i32) before it is used: a kernel that reads memory nobody wrote -- which a
// fresh process hides, because fresh device memory is zero, and a long-lived one does not, because the allocator hands
// freed blocks back -- then fails deterministically: the race / uninitialised-read check of the -m gpu suite
// (tools/records/r05_gpu2.sh).  In that mode a fill that cannot be issued or completed is an allocation failure, not a
// silently unpoisoned buffer.
// A fill of device memory that HAS LANDED when the call returns.  hipMemset on the null stream is asynchronous for device
// memory and the context streams are non-blocking (they do not order behind the null stream): a zero-fill issued by
// femcy_build_pattern could still be running when the first assembly kernel of the context stream wrote the same
// buffer, and zeroed what the kernel had just written -- the "NaN after 1 iteration" of round 5 (a K with 160 empty rows ->
// 1 / 0 in the Jacobi vector), reproduced and bisected in round 6 (profiles/r06_nan_hunt.txt).  The fill runs on a
// non-blocking stream of its own ON THE DEVICE OF THE ALLOCATION (several ranks of one process hold one device each; a
// device-wide synchronisation would deadlock against their co-dependent persistent kernels) and is synchronised here.
inline hipError_t dfill_sync(void* p, int value, size_t bytes) {
    if (!bytes) return hipSuccess;
#ifdef FEMCY_TEST_LATE_FILL     /* the behaviour before the fix, for tests/test_gpu_regressions.py to be shown failing on */
    return hipMemset(p, value, bytes);
#endif
    constexpr int MAXDEV = 64;
    static hipStream_t fill_stream[MAXDEV] = {};
    static std::mutex mu;
    int dev = -1;
    hipError_t e = hipGetDevice(&dev);
    if (e == hipSuccess && (dev < 0 || dev >= MAXDEV)) e = hipErrorInvalidDevice;
    hipStream_t st = nullptr;
    if (e == hipSuccess) {
        std::lock_guard<std::mutex> lock(mu);
        if (!fill_stream[dev]) e = hipStreamCreateWithFlags(&fill_stream[dev], hipStreamNonBlocking);
        st = fill_stream[dev];
    }
    if (e == hipSuccess) e = hipMemsetAsync(p, value, bytes, st);
    if (e == hipSuccess) e = hipStreamSynchronize(st);
    return e;
}

inline hipError_t dmalloc(void** p, size_t bytes) {
    static const bool poison = [] {
        const char* e = getenv("FEMCY_DEBUG_POISON");
        return e && e[0] && e[0] != '0';
    }();
    const hipError_t rc = hipMalloc(p, bytes);
    if (rc != hipSuccess || !poison || !bytes) return rc;
    // (the fill must have LANDED before the caller's first copy into the new buffer: index arrays of -1 and a memory fault
    // that was the checker's own)
    const hipError_t e = dfill_sync(*p, 0xFF, bytes);
    if (e != hipSuccess) {
        (void)hipFree(*p);
        *p = nullptr;
    }
    return e;
}
template <class T>
inline hipError_t dmalloc(T** p, size_t bytes) {
    return dmalloc(reinterpret_cast<void**>(p), bytes);
}

// Move-only owner of one device allocation: every device buffer of the backend is one (the members of Ctx, of the objects
// it hands out by id, of the direct solver's state, and the scratch of single calls).  The memory is released when the
// owner goes or is given a new allocation, so whoever drops one while kernels may still read it synchronises the stream
// first (femcy_ctx_destroy states the order for a whole context).  It reads as the pointer it owns -- kernel arguments,
// arithmetic, null tests; where a type is deduced from the argument (hipExtLaunchKernelGGL, ?: against nullptr,
// reinterpret_cast) say get().  A failed allocation leaves it null with capacity 0, never the address it held before.
template <class T>
class DevBuf {
    T* p_ = nullptr;
    size_t cap_ = 0;   // bytes

public:
    DevBuf() = default;
    DevBuf(DevBuf&& o) noexcept : p_(o.p_), cap_(o.cap_) { o.p_ = nullptr, o.cap_ = 0; }
    DevBuf& operator=(DevBuf&& o) noexcept {
        if (this != &o) {
            reset();
            p_ = o.p_, cap_ = o.cap_;
            o.p_ = nullptr, o.cap_ = 0;
        }
        return *this;
    }
    ~DevBuf() { reset(); }
    void reset() {
        if (p_) (void)hipFree(p_);
        p_ = nullptr, cap_ = 0;
    }
    hipError_t alloc(size_t bytes) {
        reset();
        const hipError_t e = dmalloc(&p_, bytes);
        if (e != hipSuccess) p_ = nullptr;
        else cap_ = bytes;
        return e;
    }
    // a new allocation (the contents go) only if the buffer holds fewer than `bytes`; *grew says which it was
    hipError_t grow(size_t bytes, bool* grew = nullptr) {
        const bool g = !p_ || bytes > cap_;
        if (grew) *grew = g;
        return g ? alloc(bytes) : hipSuccess;
    }
    // take over an allocation of `bytes` that did not come from dmalloc (hipFree releases it all the same)
    void adopt(T* p, size_t bytes) {
        reset();
        p_ = p, cap_ = p ? bytes : 0;
    }
    T* get() const { return p_; }
    size_t capacity() const { return cap_; }
    operator T*() const { return p_; }
    T* operator->() const { return p_; }
};

// The two ways device memory is obtained.  dev_alloc: `count` elements (at least one), anew, or with `grew` only if the
// buffer is too small (*grew: whether it was); `zero` fills what was allocated with zeros, landed on return (dfill_sync).
// dev_upload: a new buffer holding `bytes` of host memory.  After a failure the buffer is null.  An allocation that fails is
// FEMCY_ENOMEM with the text below, or `nomem` for the sites that have always reported it as a HIP error.
template <class T>
inline int dev_alloc(DevBuf<T>& d, size_t count, bool zero = true, bool* grew = nullptr, int nomem = FEMCY_ENOMEM) {
    const size_t bytes = (count ? count : 1) * sizeof(T);
    bool fresh = true;
    const hipError_t e = grew ? d.grow(bytes, &fresh) : d.alloc(bytes);
    if (grew) *grew = fresh;
    if (e != hipSuccess) {
        set_error("dmalloc(%zu bytes) failed: %s", bytes, hipGetErrorString(e));
        return nomem;
    }
    if (zero && fresh) FEMCY_HIP(dfill_sync(d.get(), 0, bytes));
    return FEMCY_OK;
}
template <class T>
inline int dev_upload(DevBuf<T>& d, const void* h, size_t bytes) {
    FEMCY_HIP(d.alloc(bytes > 8 ? bytes : 8));
    if (bytes) FEMCY_HIP(hipMemcpy(d.get(), h, bytes, hipMemcpyHostToDevice));
    return FEMCY_OK;
}
template <class T>
inline int dev_upload(DevBuf<T>& d, const std::vector<T>& h) {
    return dev_upload(d, h.data(), h.size() * sizeof(T));
}

// FEMCY_TUNE_PAIRS default: XCD-contiguous (1) + 8 rows per wave (2) + Morton chunk order (32) + 3 chunks per wave (128):
// 113-115 us on the 1 M-DOF CPE8 beam against 126 with all bits clear (profiles/r06_asm_cpe8_knobs.txt)
constexpr int FEMCY_PAIRS_DEFAULT = 163;
constexpr int SLICE = 64;           // nodes per SELL slice = one wavefront
constexpr int MAX_PARTIALS = 4096;  // upper bound on per-launch reduction partials

// Position of entry k (= r*dm + c) of the dm x dm block stored in block-row `row` for lane `lane`.
// Entries are interleaved in pairs, [row][k/2][lane][k%2] with the odd last entry (dm = 3: k = 8) as a
// trailing [lane] plane, so that a lane reads/writes two consecutive doubles per instruction: a wavefront
// moves 1 KiB per 16-byte load (4 + one 8-byte load per 3x3 block instead of 9 8-byte loads).
template <int DM>
__host__ __device__ __forceinline__ int64_t kv_index(int64_t row, int k, int lane) {
    constexpr int DD = DM * DM, NP = DD / 2;
    const int64_t base = row * (int64_t)(DD * SLICE);
    return (k < 2 * NP) ? base + (k >> 1) * (2 * SLICE) + lane * 2 + (k & 1) : base + NP * (2 * SLICE) + lane;
}
inline int64_t kv_index_rt(int dm, int64_t row, int k, int lane) {
    return dm == 3 ? kv_index<3>(row, k, lane) : kv_index<2>(row, k, lane);
}

// device-side scalar state of a PCG solve (conjugateGradientSolver.py:103-127)
struct PcgState {
    double rMr[2];   // r.M.r, double-buffered by iteration parity
    double r0;       // max|r0|
    double rmax;     // max|r| after the last completed iteration
    double dAd;      // multi-rank: reduced d.Ad
    double alpha;    // step length of the running iteration (k_update_xr -> k_update_d)
    double eps;      // stopping tolerance of this solve (kept on the device so that kernel arguments are
                     // solve-independent and a burst of iterations can be replayed from a hipGraph)
    int32_t iters;   // completed iterations (written by k_update_d, read by k_update_xr of the next iteration)
    int32_t it_k3;   // iteration index handed from k_update_xr to k_update_d
    int32_t done;    // 0 running, 1 converged, 2 NaN/breakdown: written by k_update_d, tested by k_spmv / k_update_xr
    int32_t skip;    // `done` as k_update_xr saw it, handed to the k_update_d of the same iteration
};

// contiguous slice range of each XCD for the SpMV (balanced by stored blocks), passed by value
struct XcdRanges {
    int32_t start[9];
};
// workgroups per XCD of a product whose longest XCD range holds `per` tasks: `cap` (the knob) or `cap_auto` (spmv_split)
inline int32_t spmv_bpx(int32_t per, int32_t cap, int32_t cap_auto) {
    if (cap <= 0) cap = cap_auto;
    return per < 1 ? 1 : (per < cap ? per : cap);
}

struct EventPair {
    hipEvent_t a, b;
};

struct Ctx {
    int device = 0;
    hipStream_t stream = nullptr;

    // ---- mesh / element / material
    int32_t nn = 0, dm = 0, ne = 0, npe = 0, nGP = 0, voigt = 0, s = 0;
    int64_t n = 0;
    std::vector<int32_t> h_elems;
    DevBuf<double> d_nodes;
    DevBuf<int32_t> d_elems;
    DevBuf<double> d_dN;
    DevBuf<double> d_w;
    DevBuf<double> d_C;
    int32_t mat_kind = -1;
    double mat_params[4] = {0, 0, 0, 0};
    double h_C[36] = {0};             // host copy of C (the consistent tangent reads lambda, mu from it)
    bool C_is_cubic = false;          // dm = 3: C has the cubic pattern (c11, c12, c44; kblock_cubic3)
    double cubic[3] = {0, 0, 0};
    bool have_mesh = false, have_element = false, have_material = false, have_pattern = false;
    bool dN_sums_to_zero = false;     // element tables satisfy sum_a dN_a = 0 (partition of unity)

    // ---- blocked SELL-64 matrix (lane = node, diagonal block in slot 0)
    int32_t nslices = 0;
    DevBuf<int32_t> d_asm_order;   // row-centric assembly (rows4): slices by decreasing work (workgroup b takes entry b)
    XcdRanges xcd{};                  // SpMV: slice range per XCD
    int32_t spmv_grid = 0;            // 8 * max blocks per XCD
    int32_t spmv_wps = 1;             // wavefronts per slice (1, 2 or 4)
    bool spmv_nt = false;             // matrix stream with non-temporal loads (matrix larger than the Infinity Cache)
    bool vec_nt = false;              // PCG vector kernels with non-temporal accesses
    int opt_vec_nt = -1;              // -1 auto (same rule as the matrix stream), 0 / 1 forced (test knob 103)
    int opt_spmv_nt = -1;             // -1 auto, 0 / 1 forced (test knob 102)
    int spmv_keep_permille = 0;       // NT SpMV: share of every XCD's slice range kept on the default cache policy
    int opt_spmv_keep = -1;           // -1 auto (235 MB of the matrix), else per mille (tuning knob 110)
    int32_t spmv_bpx_cap = 0;         // SpMV workgroups per XCD (larger slice ranges are looped in the kernel); 0 = by the
                                      // size of the matrix (spmv_cap_auto), FEMCY_TUNE_SPMV_WG_PER_XCD fixes it
    int32_t spmv_cap_auto = 256;      // spmv_split: 512 for long ranges of a large matrix, else 256
    int32_t opt_spmv_rot = -1;        // FEMCY_TUNE_SPMV_ROT: -1 = by the spread of the row lengths (spmv_split), 64 = balanced lists
    int32_t spmv_rot = 0;             // rotation of the product's rounds against each other (k_spmv), 0 = none
    DevBuf<int32_t> d_spmv_perm;   // [8][spmv_perm_rounds][workgroups per XCD] balanced task lists (spmv_split), or nullptr
    int32_t spmv_perm_rounds = 0;
    int64_t stored_rows = 0;          // sum over slices of slice_len (in block rows of 64 lanes)
    int64_t nnzb = 0;
    int32_t max_row_blocks = 0, max_node_elems = 0;
    std::vector<int32_t> h_slice_len, h_rowlen, h_bcol, h_pos;
    std::vector<int64_t> h_slice_off;
    DevBuf<int32_t> d_slice_len;
    DevBuf<int64_t> d_slice_off;
    DevBuf<int32_t> d_rowlen;      // [nn] blocks per node (indexed by node)
    DevBuf<int32_t> d_pos;         // [nn] node -> storage position (slice*64 + lane): SELL-C-sigma row order
    DevBuf<int32_t> d_node_of;     // [nslices*64] storage position -> node, -1 for padding lanes
    int32_t sell_sigma = 4096;        // sorting window (nodes); 64 = natural order.  (32768 measured -1 % ... +1 % per PCG
                                      // iteration inside bench.py on the C3D4 and C3D10 plates: no reason to move it)
    DevBuf<int32_t> d_bcol;        // [stored_rows*64]
    DevBuf<double> d_Kvals;        // [stored_rows*dm*dm*64]
    DevBuf<uint16_t> d_slotj;      // [ne*npe*npe] element-local (a,b) -> slot j in row of node a
    DevBuf<int32_t> d_ctr_ptr;     // [stored_rows*64+1] contributions per stored block
    DevBuf<int32_t> d_ctr;         // [ne*npe*npe] packed (e*npe+la)*npe+lb
    DevBuf<int32_t> d_tpos;        // [stored_rows*64] position of the transposed block (b,a) if a < b; p on the
                                      // diagonal; -2 if a > b (the mirror lane stores it); -1 padding
    DevBuf<int32_t> d_ne_ptr;      // [nn+1] node -> incident elements
    DevBuf<int32_t> d_ne_idx;      // [ne*npe] packed e*npe+la
    // pair lists of FEMCY_ASM_PAIRS (pattern.cpp: ensure_pairs, built on first use): per chunk of 16 (or 8) consecutive storage
    // positions the (row, incident element) pairs in (row, ascending element) order -- code e*npe+la and row inside the chunk;
    // 3-D: in step order, the s-th element of every row of the chunk, padded to whole steps
    std::vector<int32_t> h_node_of, h_ne_ptr, h_ne_idx;   // what they are built from (build_pattern: PAIRS families only)
    DevBuf<int32_t> d_pr_ptr;      // PairBatch descriptors (32 B) in PROCESSING order
    DevBuf<int32_t> d_pr_unit;     // [units + 1] first batch of every wavefront's unit of chunks
    DevBuf<int32_t> d_pr_code;     // [ne*npe + 64] row inside the chunk << 27 | e*npe+la
    int64_t pairs_serial = -1;        // pattern_serial * 64 + rows per chunk the lists were built for
    int tune_pairs = FEMCY_PAIRS_DEFAULT;   // FEMCY_TUNE_PAIRS (kernels_assembly.hip)

    // ---- Gauss-point fields
    DevBuf<double> d_dsdx;
    DevBuf<double> d_vol;
    DevBuf<double> d_F;
    DevBuf<double> d_sigma;
    DevBuf<double> d_strain;
    DevBuf<double> d_mises;
    DevBuf<double> d_energy;
    DevBuf<double> d_fe;           // [ne][npe][dm] per-element nodal forces of the last femcy_internal_force
    // The force evaluation of a Newton residual does not store F and sigma (at 1 M C3D4 they are 143 of the 334 MB the
    // element pass would write, and nothing on the solve path reads them).  The reference's post-processing reads
    // "the stress of the last force evaluation", so that state is kept as a copy of the displacement it was made
    // with (8 n bytes) and F / sigma are recomputed from it when somebody asks (ensure_gp_stress).
    bool gp_lazy = false;
    DevBuf<double> d_u_lazy;

    // ---- vectors
    DevBuf<double> d_vec[FEMCY_VEC_COUNT];
    DevBuf<double> d_r, d_d, d_M, d_Ad;
    DevBuf<double> d_part1;        // [MAX_PARTIALS] d.Ad partials (SpMV launch)
    DevBuf<double> d_part2;        // [2*MAX_PARTIALS] (r.M.r, max|r|) partials
    DevBuf<PcgState> d_state;
    PcgState* h_state = nullptr;      // pinned
    char* h_stage = nullptr;          // pinned staging area for small host -> device payloads (stage_h2d)
    size_t stage_cap = 0, stage_used = 0;
    double* h_scalar = nullptr;       // pinned scratch for reductions
    DevBuf<int32_t> d_idx_scratch;
    DevBuf<double> d_val_scratch;

    // ---- hipGraph of one poll-burst of PCG iterations (single rank, timing off)
    hipGraphExec_t pcg_graph = nullptr;
    const double* pcg_graph_x = nullptr;
    int pcg_graph_iters = 0, pcg_graph_g = 0, pcg_graph_np1 = 0;
    int opt_graph = 1;
    // ---- persistent one-launch PCG for systems of one wavefront-task per SIMD (k_pcg_persist)
    int opt_persist = 1;              // FEMCY_OPT_PCG_PERSIST
    // limit on the STREAMED part of the matrix in the persistent PCG.  Rounds 2-4: 240 MiB (the Infinity Cache), from a
    // round-2 measurement (124 k C3D10, 280 MB streamed: 99-103 us here against 93 with three launches).  Re-measured in
    // round 5 with the round-4 kernel (nt stream, tagged granules, storage-order d, 16 + 8 byte gathers): 61.0 us
    // against 78.0 (profiles/r05_persist_hbm_c3d10.txt) -- the rule was stale.  What bounds the kernel is the vector
    // layout (<= 4 slices per wave), not the matrix: no byte limit by default any more (test knob: option 114)
    int64_t persist_max_bytes = (int64_t)1 << 40;
    int opt_persist_rj = 4;           // block rows per slice kept in registers (test knob 105)
    int opt_persist_wgs = 0;          // test knob 107: workgroups of the launch (0 = one per CU; more than that cannot
                                      // be co-resident, the barrier times out and the solve falls back)
    int opt_persist_l2rows = 1;       // FEMCY_TUNE_PERSIST_L2_ROWS: default-policy streamed rows per slice (VAR & 1)
    int opt_persist_variant = -1;     // FEMCY_TUNE_PERSIST_VARIANT bits (-1 = defaults)
    int opt_persist_dbg = 0;          // timing experiments only (test knob 106): skip parts of the iteration
    int opt_persist_lds = -1;         // block rows per wave kept in LDS (-1: as many as fit; test knob 104)
    int persist_cus = 0;              // compute units of the device
    bool persist_failed = false;      // a grid barrier timed out once: do not try again on this context
    bool small_failed = false;        // the same for k_pcg_small
    int opt_skip_occupancy = 0;       // FEMCY_TUNE_SKIP_OCCUPANCY_CHECK
    uint32_t barrier_spin_limit = 1u << 20;   // polls (s_sleep 1 each, ~0.3 us) before a grid barrier gives up: ~0.5 s
    DevBuf<int32_t> d_persist_assign;   // [waves][SPW] slices of each wave (LPT-balanced per XCD range), -1 = none
    std::vector<int64_t> persist_assign_key;
    int64_t pattern_serial = 0;       // bumped by femcy_build_pattern
    DevBuf<double> d_persist;      // d double buffer, partials, granules, barrier counters
    // ---- three-launch PCG with its vectors in storage order (single rank)
    DevBuf<int32_t> d_bcolp;       // block columns as storage positions (PCG with its vectors in storage order)
    int64_t bcolp_serial = -1;
    int opt_pos_space = 1;            // FEMCY_OPT_PCG_STORAGE_ORDER: the three-kernel PCG of a single rank keeps r, d, M, Ad, x
                                      // in storage order (gathers of neighbouring lanes then hit neighbouring addresses)
    DevBuf<double> d_posb;         // right-hand side / solution in storage order
    DevBuf<double> d_posx;
    int opt_node_order = 1;           // FEMCY_OPT_NODE_ORDER: 0 = rows sorted inside windows of the caller's numbering,
                                      // 1 (default) = inside windows of the best of a few coordinate orders if it beats the
                                      // caller's numbering by 10 % (measured on the pattern), 2 + k = forced: coordinate order k
    int node_order_used = 0;          // 0 natural, 1 + k = coordinate order k (femcy_pattern_info)
    double node_order_cost[8] = {0};  // mean 128-byte lines per wave gather, natural first (diagnostics)
    std::vector<double> h_nodes;      // host copy of the coordinates (femcy_set_mesh) for the ordering
    DevBuf<char> d_probe;          // femcy_probe_stream's buffer
    // ---- one-launch PCG for small systems (k_pcg_small)
    int opt_small_rr = -1;            // test knob 108: block rows per wave of the small-system PCG kept in registers
    int opt_small = 1;                // FEMCY_OPT_PCG_SMALL
    int small_max_lds = 65536;        // LDS a workgroup may allocate (device attribute, femcy_ctx_create)
    int small_max_wg = 128;           // workgroups that are certainly co-resident at one per CU
    DevBuf<double> d_small;        // Ad double buffer, d.Ad partials, barrier counter
    int ew_cap = 512;                 // FEMCY_OPT_EW_GRID

    // ---- device-resident DOF lists of *Boundary blocks
    struct DofSet { DevBuf<int32_t> d_dofs; DevBuf<double> d_vals; int32_t k = 0; };
    std::vector<DofSet> dofsets;

    // ---- device-resident *Dsload surfaces (femcy_loadset_*)
    struct LoadSet {
        int32_t nft = 0, nfn = 0, nip = 0, nload = 0, nnode = 0;
        DevBuf<int32_t> d_ft_nodes, d_elem, d_ft, d_node, d_ptr, d_slot;
        DevBuf<double> d_N, d_dN, d_normal, d_weight, d_contrib, d_dir;
    };
    std::vector<LoadSet> loadsets;

    // ---- device-resident body loads (femcy_bodyload_*): the nodal weights m_a of one element selection
    struct BodyLoad { DevBuf<double> d_m; int32_t nsel = 0; };
    std::vector<BodyLoad> bodyloads;

    // ---- device-resident thermal loads (femcy_thermal_*): the load vector at scale 1 of one nodal temperature change,
    // and what the stress correction reads again (the temperatures, the shape functions at the Gauss points, and the
    // stress of full restraint per unit temperature change, alpha * C : eps_th, as a full row-major tensor)
    struct ThermalStress { double s[9]; };
    struct Thermal { DevBuf<double> d_f, d_dT, d_N; ThermalStress ts{}; };
    std::vector<Thermal> thermals;
    // ---- device-resident consistent mass (femcy_mass_*): one scalar per stored block, in d_bcol's [block row][lane] layout
    struct Mass { DevBuf<double> d_m; };
    std::vector<Mass> masses;
    // ---- explicit dynamics (femcy_lumped_mass_*, femcy_explicit_*): the HRZ-lumped nodal masses [nn], and an integrator =
    // the inverse mass per scalar DOF [n] with 0 on the constrained DOFs + the lumped mass it was made from
    // An automatic run (femcy_explicit_auto_*) also reads the element shares me [ne][npe] the nodal masses were summed from,
    // and keeps its clock (element_math.hpp: ExplicitClock) and the partial maxima of the bound kernel [ceil(ne / 256)] on
    // the device; both are allocated by the first call that needs them.
    // d_scale [ne]: the cumulative factors of femcy_lumped_mass_scale, allocated by its first call (none yet: all 1)
    struct LumpedMass { DevBuf<double> d_m, d_me, d_scale; double rho = 0.0; };
    std::vector<LumpedMass> lumped_masses;
    struct Explicit {
        DevBuf<double> d_minv, d_bpart;
        DevBuf<ExplicitClock> d_clock;
        int32_t lumped = -1;
        bool auto_begun = false;
        double s_C = 0.0;
        double alpha = 0.0, b1 = 0.0, b2 = 0.0, Md = 0.0;      // femcy_explicit_set_damping; all 0: the undamped launches
        bool damped() const { return alpha != 0.0 || b1 != 0.0 || b2 != 0.0; }
        bool bulk() const { return b1 != 0.0 || b2 != 0.0; }
        // prescribed motion (femcy_explicit_set_motion): the DOF-set ids the integrator holds, the compact list of moved
        // DOFs (d_mdof, d_mval, d_mcurve [nmoved]), the per-DOF position in it or -1 (d_mslot [n]) and the curves (d_amp);
        // nmoved = 0: no motion, the launches of an integrator that never had one
        std::vector<int32_t> held;
        DevBuf<int32_t> d_mslot, d_mdof, d_mcurve;
        DevBuf<double> d_mval;
        DevBuf<Amplitude> d_amp;
        int32_t nmoved = 0;
        // the clock of a fixed run: steps taken since femcy_explicit_start, and the (t_base, n_base, dt) of
        // explicit_fixed_time (element_math.hpp)
        int64_t n_done = 0, n_base = 0;
        double t_base = 0.0, dt_prev = 0.0;
        // the energy balance (femcy_explicit_energy_enable): asked for / running since a start; the forces of the last
        // kicked state (d_efint, d_ealpha [n]) and one slot of EN_SLOT doubles per wavefront of the node-pass grid
        // (explicit_energy_slots), all allocated by the first enable; off: the launches of an integrator that never had it
        bool energy_want = false, energy_on = false;
        DevBuf<double> d_efint, d_ealpha, d_eslot;
        // rigid walls (femcy_explicit_set_wall): they travel in the kernel arguments; walls.n = 0: none, the launches of an
        // integrator that never had one.  wall_kappa: the sum of their penalties, what the element bound adds
        ExplicitWalls walls{};
        double wall_kappa() const {
            double k = 0.0;
            for (int32_t w = 0; w < walls.n; ++w) k += walls.kappa[w];
            return k;
        }
    };
    std::vector<Explicit> explicits;
    std::vector<Amplitude> amplitudes;   // femcy_amplitude_create; dropped where integrators are
    int64_t K_serial = -1;            // pattern_serial of the last successful assembly: K holds a matrix when they agree
    bool post_small = false;         // sigma / mises hold femcy_compute_strain_stress(large = 0), not yet corrected

    // ---- options / timing
    int opt_assembly = FEMCY_ASM_AUTO;
    int asm_used = -1;                // the mode the last assembly ran, AUTO resolved (femcy_get_assembly_used)
    int opt_tangent = 0;              // FEMCY_OPT_TANGENT
    int opt_poll = 32;
    int opt_timing = 0;               // 0 off, 1 every launch, k > 1: every k-th SpMV launch
    int64_t spmv_count = 0;
    int opt_timing_fence = 1;
    int opt_spmv_variant = 0;
    femcy_timing_t timing{};
    std::vector<EventPair> ev_pool;
    struct Pending { int cls; size_t ev; };
    std::vector<Pending> ev_pending;
    size_t ev_next = 0;

    // ---- multi-rank
    int32_t rank = 0, nranks = 1;
    int64_t n_global = 0;             // DOFs of the un-partitioned system (sum of owned DOFs over the ranks)
    void* comm = nullptr;             // ncclComm_t, the in-process group (comm_local) or the shared-memory group
    int comm_kind = 0;                // COMM_*
    bool comm_local = false;
    uint64_t comm_token = 0;
    int32_t niface_local = 0, niface_global = 0;
    DevBuf<int32_t> d_iface_dof;
    DevBuf<int32_t> d_iface_slot;
    DevBuf<int32_t> d_slot2dof;    // [niface_global] local DOF of each global interface slot, -1 if not held
    DevBuf<uint8_t> d_owner;
    DevBuf<double> d_commbuf;      // [niface_global + 8]
    DevBuf<double> d_gather;       // [nranks*2]

    // ---- persistent PCG across ranks (kernels_pcg_persist.hip "persistent PCG across ranks"): this rank's mailbox,
    // the peers' mailboxes as mapped on this device, the per-position interface table
    DevBuf<unsigned long long> d_mbox;
    bool mbox_finegrained = false;
    std::vector<unsigned long long*> h_peer_mbox;   // [nranks], own entry = d_mbox
    std::vector<void*> ipc_opened;                  // mappings to close
    DevBuf<unsigned long long*> d_peer_tab;         // device copy of h_peer_mbox
    DevBuf<int32_t> d_mr_tab;                    // [nslices * 64][4]
    std::vector<int32_t> h_nb_dofs;                 // host copy of the neighbour DOF lists
    bool persist_multi_local = false;               // this rank could take the path
    bool persist_multi = false;                     // ... and every rank agreed (femcy_comm_persist_agree)
    bool persist_multi_failed = false;              // a solve timed out: the RCCL loop for the next solves
    int persist_multi_fallbacks = 0;                // ... counted here; the one-launch path is retried after PERSIST_MULTI_RETRY
    int opt_persist_multi = 1;                      // FEMCY_OPT_PCG_PERSIST_MULTI
    uint32_t solve_serial = 0;

    // ---- overlapped iteration (neighbour exchange): interface slices first, their exchange on a second stream
    // while the interior slices are multiplied
    hipStream_t comm_stream = nullptr;
    hipEvent_t ev_iface = nullptr, ev_xchg = nullptr;
    int opt_overlap = 1;              // FEMCY_OPT_OVERLAP
    bool split_ready = false;
    std::vector<int32_t> h_iface_dof; // host copy of the local interface DOFs (femcy_comm_init)
    DevBuf<int32_t> d_split_list;  // [nslices] slices holding an interface node first, then the others
    int32_t n_if_slices = 0;

    // ---- neighbour exchange (femcy_comm_set_neighbours): the alternative to the packed all-reduce
    int exchange = 0;                 // FEMCY_OPT_EXCHANGE: 0 packed all-reduce, 1 neighbour send/recv
    std::vector<int32_t> h_nb_rank, h_nb_ptr;   // neighbours (ascending) and their segments of the send / recv buffers
    DevBuf<int32_t> d_nb_dofs;     // [nb_total] local DOF of every send entry
    DevBuf<double> d_nb_send;      // [nb_total]
    DevBuf<double> d_nb_recv;      // [nb_total]
    DevBuf<int32_t> d_if_ptr;      // [niface_local+1] per local interface DOF (order of d_iface_dof): its
    DevBuf<int32_t> d_if_src;      //   contributions in ascending rank order; src = recv index, -1 = own value
};

template <>
inline bool vec_allocated(const Ctx* c, int v) {
    return c->d_vec[v] != nullptr;
}

enum { COMM_NONE = 0, COMM_RCCL = 1, COMM_LOCAL = 2, COMM_SHM = 3 };
// timing classes
enum { T_GEOM = 0, T_ASM = 1, T_FORCE = 2, T_SPMV = 3, T_PCG = 4, T_PERSIST = 5 };
size_t timing_begin(Ctx* c, int cls);
EventPair* timing_acquire(Ctx* c, int cls);   // registers a pair without recording (hipExtLaunchKernel fills it)
void timing_end(Ctx* c, size_t h);
void timing_collect(Ctx* c);

// pattern.cpp
int build_pattern(Ctx* c);
void spmv_split(Ctx* c);
// kernels_*.hip (host launchers)
// what the element pass leaves in memory: current-configuration gradients + det J w (always computed), the
// deformation gradient, the Cauchy stress, the per-element nodal forces
enum : unsigned { GEOM_DSDX = 1, GEOM_F = 2, GEOM_SIGMA = 4, GEOM_FE = 8 };
// gd (a damped explicit step with bulk viscosity, what includes GEOM_FE): the element pass adds the bulk-viscosity pressure
// at v_{n+1/2} = v + h/2 a from d_v, d_a (d_a null: the start, v_0 alone), h from the argument or, with d_clk, the device
// clock's h_next
struct GeomDamping {
    const double *d_v, *d_a;
    const ExplicitClock* d_clk;
    double h;
    double alpha, b1, b2, Md, rho0;      // element_math.hpp: ExplicitDamping
};
int launch_geom(Ctx* c, const double* d_u, unsigned what, const GeomDamping* gd = nullptr);
int ensure_gp_stress(Ctx* c);   // F / sigma of the last force evaluation, recomputed on demand (see Ctx::gp_lazy)
int launch_post(Ctx* c, int large);
int launch_energy(Ctx* c);
int launch_energy_small(Ctx* c);   // d_energy = sigma : eps / 2 of the infinitesimal strain of d_F
int launch_extrapolate(Ctx* c, const double* d_E, const double* d_field, int width, int comp, double* d_out);
int launch_energy_sum(Ctx* c, double* total);
int launch_assemble(Ctx* c);
int launch_nodal_force(Ctx* c, double* d_f);
int launch_neumann(Ctx* c, const Ctx::LoadSet& ls, double traction, bool along_normal, double* d_rhs, bool add);
void launch_node_sum(Ctx* c, const double* d_src, double* d_m);   // d_m [nn] = node sums of d_src [ne][npe]; only enqueues
int launch_body_weights(Ctx* c, const double* d_N, const uint8_t* d_mask_or_null, double* d_we, double* d_m);
int launch_body_apply(Ctx* c, const double* d_m, const double* b, bool add, double* d_f);
int launch_thermal_force(Ctx* c, const Ctx::Thermal& th, double* d_fe);
int launch_thermal_apply(Ctx* c, const double* d_funit, double scale, bool add, double* d_f);
int launch_thermal_post(Ctx* c, const Ctx::Thermal& th, double scale);
// consistent mass: element pass (rho |det J| w at the mass rule's points) into d_vq [ne][nq] (scratch of the caller), then one
// scalar per stored block into d_m [stored_rows * 64]
int launch_mass_blocks(Ctx* c, int32_t nq, const double* d_Nq, const double* d_dNq, const double* d_wq, double rho,
                       double* d_vq, double* d_m);
// d_y = [d_y +] scale (M (x) I) d_x (d_y may be null); d_partials != null: per-workgroup partials of x . (M x), count in *np
int launch_mass_spmv(Ctx* c, const double* d_m, const double* d_x, double* d_y, double scale, bool add, double* d_partials,
                     int* np);
int launch_mass_add_to_K(Ctx* c, const double* d_m, double cc, bool overwrite);
int launch_mass_energy(Ctx* c, const double* d_m, const double* d_v, double* out);
int launch_newmark_predict(Ctx* c, const double* u, const double* v, const double* a, double* out, double c0, double c1,
                           double c2);
int launch_newmark_update(Ctx* c, const double* un, const double* u, double* v, double* a, double beta, double gamma,
                          double dt);
// explicit dynamics (kernels_explicit.hip).  Lumped mass: element pass into d_me [ne][npe] (scratch of the caller), node sums
// into d_m [nn].  launch_explicit_minv: d_minv [n] = 1 / m of the DOF's node.  launch_explicit_node follows an element pass
// that left d_fe (launch_geom with GEOM_FE): mode XN_START = a_0, XN_KICK = one kick, XN_KICK_DRIFT = kick + the drift to the
// next state (element_math.hpp), with the node sums of d_fe never stored.  launch_explicit_drift: the first drift of a call.
// Both take the increment h and the load scale from the arguments when d_clk is null (a fixed step), and from the device
// clock of an automatic run otherwise (scale and h are then ignored).  All of them only enqueue.
int launch_lumped_mass(Ctx* c, int32_t nq, const double* d_Nq, const double* d_dNq, const double* d_wq, double rho,
                       double* d_me, double* d_m);
int launch_explicit_minv(Ctx* c, const double* d_m, double* d_minv);
int launch_explicit_drift(Ctx* c, const ExplicitClock* d_clk, double h);
// mv (femcy_explicit_set_motion; null: none, today's instantiations with today's arguments): the tables of the moved DOFs
// and, for a fixed step, the time t of the state being kicked and t_drift the drift reaches (an automatic run reads both
// from the clock).  launch_explicit_place: u, v, a (what: MOVE_* of element_math.hpp) of the moved DOFs at t, or with d_clk
// at the clock's t_next unless its h_next = 0.
struct ExplicitMotion {
    const int32_t *d_slot, *d_dof, *d_curve;
    const double* d_val;
    const Amplitude* d_amp;
    int32_t nmoved;
    double t, t_drift;
};
// en (femcy_explicit_energy_enable; null: none, today's instantiations with today's arguments): the energy variant of the
// node pass, which also adds the step's four work addends into the wavefront's slot of d_slot [explicit_energy_slots(c)]
// [EN_SLOT] and leaves the state's forces in d_fint / d_falpha [n]; d_m [nn] the lumped mass.  launch_explicit_energy_sum:
// out[FEMCY_EN_*] = the slots summed in a fixed order, fetched (synchronises).
constexpr int EN_SLOT = 8;      // the four sums, the load scale and the time of the last kicked state, padding to 64 B
struct ExplicitEnergy {
    const double* d_m;
    double *d_fint, *d_falpha, *d_slot;
};
int explicit_energy_slots(const Ctx* c);
// wl (femcy_explicit_set_wall; null: none, today's instantiations with today's arguments): the wall variant of either node
// pass, which also reads the node coordinates and u in every mode and adds wall_accel (element_math.hpp) to the kick.
// launch_explicit_wall_get: out[0..4) of femcy_explicit_wall_get for wall k from vec[DOF], fetched (synchronises).
int launch_explicit_node(Ctx* c, const double* d_minv, const double* d_f, const ExplicitClock* d_clk, double scale, double h,
                         int mode, double alpha = 0.0, const ExplicitMotion* mv = nullptr, const ExplicitEnergy* en = nullptr,
                         const ExplicitWalls* wl = nullptr);
int launch_explicit_wall_get(Ctx* c, const ExplicitWalls& wl, int k, const double* d_m, const double* d_minv, double* out);
int launch_explicit_energy_sum(Ctx* c, const double* d_slot, double* out);
int launch_explicit_place(Ctx* c, const ExplicitMotion& mv, const ExplicitClock* d_clk, double t, int what);
int launch_explicit_energy(Ctx* c, const double* d_m, const double* d_v, double* out);   // 1/2 sum m v^2, fixed order
// max over the rows i with minv_i != 0 of minv_i sum_j |K_ij| (Gershgorin bound on the spectrum of M_L^-1 K)
int launch_rowabs_bound(Ctx* c, const double* d_minv, double* out);
// element-by-element increment.  launch_explicit_bound: the workgroup maxima of omega_e^2 at d_u into d_part
// [explicit_bound_partials(c)], recomputed from the mesh.  _bound_max: their maximum, fetched (synchronises).  _clock: their
// maximum + one tick of the device clock.  All but _bound_max only enqueue.
int explicit_bound_partials(const Ctx* c);
// gd: omega_eff,e^2 with the damping of gd at v_{n+1/2}, formed as the element pass forms it; kappa: the sum of the wall
// penalties, added to omega_e^2 before that (0: none)
int launch_explicit_bound(Ctx* c, const double* d_u, const double* d_me, double s_C, double* d_part,
                          const GeomDamping* gd = nullptr, double kappa = 0.0);
int launch_explicit_bound_max(Ctx* c, const double* d_part, double* out);
int launch_explicit_clock(Ctx* c, const double* d_part, ExplicitClock* d_clk);
// fixed mass scaling (femcy_lumped_mass_scale).  launch_mass_total: the sum of d_m [nn] in a fixed order, fetched.
// launch_mass_scale_factors: d_fac [ne] = k_e from omega_e^2 at u = 0 with the shares d_me, its partials into d_part
// [3 explicit_bound_partials(c)], and out[0..3) = max omega_e^2 (NaN as infinity), max k_e (anything but a finite positive
// factor as infinity), the number of k_e != 1; measure: out[0] alone and d_fac is not written.  Both synchronise.
// launch_mass_scale_apply: d_me[e][:] *= d_fac[e], d_cum[e] = (first ? 1 : d_cum[e]) d_fac[e], d_m = node sums; only enqueues.
int launch_mass_total(Ctx* c, const double* d_m, double* out);
int launch_mass_scale_factors(Ctx* c, const double* d_me, double s_C, double w2max, double factor, double tau, int type,
                              bool measure, double* d_fac, double* d_part, double* out);
int launch_mass_scale_apply(Ctx* c, const double* d_fac, bool first, double* d_me, double* d_cum, double* d_m);
// pos_space: x and y are in STORAGE order (entry p * dm + c belongs to the node at storage position p = slice * 64 + lane;
// the padding lanes of the last slice hold zeros) -- the form the three-kernel PCG runs in since round 4
int launch_spmv(Ctx* c, const double* d_x, double* d_y, double* d_partials, int* nblocks_out, bool pos_space = false);
// part 1 / 2 of the split product: the slices holding interface nodes / all others (partials go to
// d_partials[part_off ...]); split_prepare builds the slice list once per pattern + communicator
int launch_spmv_part(Ctx* c, int part, const double* d_x, double* d_y, double* d_partials, int part_off, int* nblocks_out);
int split_prepare(Ctx* c);
bool coresident(Ctx* c, const void* fn, int block, size_t lds, int grid);
int probe_stream(Ctx* c, int64_t bytes, int32_t reps, int32_t mode, double* us_per_pass, int64_t* bytes_per_pass);
int probe_exchange(Ctx* c, int32_t rounds, int32_t form, double* us_per_exchange);
int probe_mailbox(Ctx* c, int32_t rounds, double* us_per_round);
int probe_spmv(Ctx* c, int32_t reps, int32_t storage_order, double* us_per_launch);
int spmv_public_storage_order(Ctx* c, const double* d_x, double* d_y);   // femcy_spmv through the storage-order kernel
int64_t persist_streamed_bytes(Ctx* c);
// FEMCY_ASM_PAIRS (kernels_assembly.hip) is instantiated for C3D8, C3D6 and the 2-D families
inline bool pairs_hex(const Ctx* c) { return c->dm == 3 && c->npe == 8 && c->nGP == 8; }
inline bool pairs_wedge(const Ctx* c) { return c->dm == 3 && c->npe == 6 && c->nGP == 6; }
inline bool pairs_instantiated(const Ctx* c) {
    return pairs_hex(c) || pairs_wedge(c) ||
           (c->dm == 2 && ((c->npe == 8 && c->nGP == 4) || (c->npe == 6 && c->nGP == 3) || (c->npe == 4 && c->nGP == 4) ||
                           (c->npe == 3 && c->nGP == 1)));
}
int ensure_pairs(Ctx* c, int rows_per_chunk, bool spatial_order, int chunks_per_wave);   // pattern.cpp: d_pr_unit / d_pr_ptr / d_pr_code for the current pattern
int ensure_pos_vectors(Ctx* c);   // d_posb / d_posx (storage-order right-hand side / solution) + d_bcolp
int ensure_bcolp(Ctx* c);   // d_bcolp = pos[bcol]: block columns as storage positions
int pcg_persist_solve(Ctx* c, const double* d_b, double* d_x, double eps, int32_t maxit, bool* handled);
int launch_dirichlet_zero(Ctx* c, const int32_t* d_dofs, int32_t k, double* d_resid_or_null);
int pcg_solve(Ctx* c, const double* d_b, double* d_x, double eps, int32_t maxit, int32_t* iters, double* r0,
              double* rmax);
int vec_fill(Ctx* c, double* d, double v, int64_t n);
int vec_sub(Ctx* c, double* dc, const double* da, const double* db);
int vec_axpy(Ctx* c, double* da, const double* db, double cc, const double* dd);
int vec_scale(Ctx* c, double* d, double s);
int vec_sumsq(Ctx* c, const double* d, double* out);
int vec_absmax(Ctx* c, const double* d, double* out);
int vec_scatter(Ctx* c, double* d, const int32_t* d_idx, const double* d_vals, int32_t k);
int vec_scatter_const(Ctx* c, double* d, const int32_t* d_idx, double val, int32_t k);
int vec_scatter_add(Ctx* c, double* d, const int32_t* d_idx, double val, int32_t k);
int ensure_scratch(Ctx* c, int64_t k);
// comm.cpp
int comm_unique_id(void* id128);
int comm_local_id(void* id128);
int comm_shm_id(void* id128, int64_t cap_doubles);
int comm_allgather_host(Ctx* c, const void* send, int32_t bytes, void* recv);
int comm_init(Ctx* c, int32_t rank, int32_t nranks, const void* id128);
int comm_allreduce_sum(Ctx* c, double* d_buf, int64_t count);
int comm_allgather(Ctx* c, const double* d_send, double* d_recv, int64_t count);
int comm_neighbour_exchange(Ctx* c, hipStream_t stream);   // d_nb_send segments -> neighbours, their segments -> d_nb_recv
int comm_register_neighbours(Ctx* c);  // in-process transport: publish this rank's segment table
int comm_destroy(Ctx* c);
int comm_mailbox_export(Ctx* c, void* blob256);
int comm_mailbox_import(Ctx* c, int32_t nblobs, const void* blobs);
int comm_persist_agree(Ctx* c, int32_t* enabled);
bool persist_pattern_fits(Ctx* c);
int iface_sum(Ctx* c, double* d_v);
int scalar_across_ranks(Ctx* c, double* d_val, int mode, double* out);
void pcg_graph_reset(Ctx* c);

}  // namespace femcy

struct femcy_ctx {
    femcy::Ctx c;
};
