// C ABI entry points of libfemcy_hip.so (declared in include/femcy.h).  Thin argument checking and
// resource management around the launchers in kernels_*.hip / pattern.cpp / comm.cpp.
#include <algorithm>
#include <cmath>
#include <cstdarg>
#include <chrono>
#include <cstdio>
#include <cstring>
#include <utility>
#include "ctx.hpp"
#include "element_dispatch.hpp"
#include "element_math.hpp"
#include "direct.hpp"
#include "motion_tables.hpp"

namespace femcy {

static thread_local char g_err[1024] = "";

void set_error(const char* fmt, ...) {
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(g_err, sizeof(g_err), fmt, ap);
    va_end(ap);
}

// the objects a context hands out by id, dropped when the mesh they were made on goes; their buffers go with them (DevBuf),
// so the streams are drained by the caller
static void drop_objects(Ctx* c) {
    c->dofsets.clear();
    c->loadsets.clear();
    c->bodyloads.clear();
    c->thermals.clear();
    c->masses.clear();
    c->lumped_masses.clear();
    c->explicits.clear();
    c->amplitudes.clear();
}

// Right-hand side of a stored load: apply(dst, add) writes this rank's share of it into dst (add: adds it) and is called
// once.  Multi-rank: every rank evaluates its own elements, so the load is summed over the interface -- when it is added
// to a vector, alone in TMP1 first.  `who` names the caller in the refusal.
template <class Apply>
static int apply_load(Ctx* c, const char* who, int rhs_vec, bool add, Apply&& apply) {
    FEMCY_REQUIRE(!add || !c->comm || rhs_vec != FEMCY_VEC_TMP1, "%s on several ranks sums the interface through vector "
                  "TMP1: it cannot be the right-hand side", who);
    double* rhs = c->d_vec[rhs_vec];
    int rc;
    if (add && c->comm) {
        double* tmp = c->d_vec[FEMCY_VEC_TMP1];
        if ((rc = apply(tmp, false))) return rc;
        if ((rc = iface_sum(c, tmp))) return rc;
        return vec_axpy(c, rhs, rhs, 1.0, tmp);
    }
    if ((rc = apply(rhs, add))) return rc;
    if (add) return FEMCY_OK;
    return iface_sum(c, rhs);
}

int ensure_scratch(Ctx* c, int64_t k) {
    const size_t cap = (size_t)std::max<int64_t>(k, 1024);
    bool grew;
    int rc;
    if ((rc = dev_alloc(c->d_idx_scratch, cap, false, &grew))) return rc;
    return dev_alloc(c->d_val_scratch, cap, false, &grew);
}

// Small host -> device payloads (the values of a prescribed-displacement block, index lists of a scatter) go through a
// pinned staging area: the caller's buffer is copied on the host, the device copy is asynchronous, and the call does
// not have to wait for the stream (a pageable hipMemcpyAsync + hipStreamSynchronize costs ~40 us per call; a deck run
// issues tens of thousands of them).  The area is a bump allocator: when it is full the stream is drained once.
static int stage_h2d(Ctx* c, void* dst, const void* src, size_t bytes) {
    constexpr size_t CAP = (size_t)1 << 20;
    if (bytes > CAP / 4) {                                  // large payloads: plain copy, synchronous for the caller
        FEMCY_HIP(hipMemcpyAsync(dst, src, bytes, hipMemcpyHostToDevice, c->stream));
        FEMCY_HIP(hipStreamSynchronize(c->stream));
        return FEMCY_OK;
    }
    if (!c->h_stage) {
        FEMCY_HIP(hipHostMalloc((void**)&c->h_stage, CAP, hipHostMallocDefault));
        c->stage_cap = CAP;
        c->stage_used = 0;
    }
    const size_t need = (bytes + 63) & ~(size_t)63;
    if (c->stage_used + need > c->stage_cap) {
        FEMCY_HIP(hipStreamSynchronize(c->stream));         // every copy that reads the area has finished
        c->stage_used = 0;
    }
    char* slot = c->h_stage + c->stage_used;
    c->stage_used += need;
    std::memcpy(slot, src, bytes);
    FEMCY_HIP(hipMemcpyAsync(dst, slot, bytes, hipMemcpyHostToDevice, c->stream));
    return FEMCY_OK;
}

// ------------------------------------------------------------------------------------- timing
static size_t timing_slot(Ctx* c, int cls) {
    if (!c->opt_timing) return (size_t)-1;
    if (c->ev_next >= c->ev_pool.size()) {
        EventPair p;
        if (hipEventCreate(&p.a) != hipSuccess || hipEventCreate(&p.b) != hipSuccess) return (size_t)-1;
        c->ev_pool.push_back(p);
    }
    size_t h = c->ev_next++;
    c->ev_pending.push_back({cls, h});
    return h;
}
size_t timing_begin(Ctx* c, int cls) {
    size_t h = timing_slot(c, cls);
    if (h != (size_t)-1) (void)hipEventRecord(c->ev_pool[h].a, c->stream);
    return h;
}
EventPair* timing_acquire(Ctx* c, int cls) {
    size_t h = timing_slot(c, cls);
    return h == (size_t)-1 ? nullptr : &c->ev_pool[h];
}
void timing_end(Ctx* c, size_t h) {
    if (h == (size_t)-1) return;
    (void)hipEventRecord(c->ev_pool[h].b, c->stream);
}
void timing_collect(Ctx* c) {
    if (c->ev_pending.empty()) return;
    (void)hipStreamSynchronize(c->stream);
    for (auto& p : c->ev_pending) {
        float ms = 0.f;
        if (hipEventElapsedTime(&ms, c->ev_pool[p.ev].a, c->ev_pool[p.ev].b) != hipSuccess) continue;
        switch (p.cls) {
            case T_GEOM: c->timing.geom_ms += ms; c->timing.geom_launches++; break;
            case T_ASM: c->timing.assemble_ms += ms; c->timing.assemble_launches++; break;
            case T_FORCE: c->timing.force_ms += ms; c->timing.force_launches++; break;
            case T_SPMV: c->timing.spmv_ms += ms; c->timing.spmv_launches++; break;
            case T_PCG: c->timing.pcg_ms += ms; break;
            case T_PERSIST: c->timing.persist_ms += ms; c->timing.persist_launches++; break;
        }
    }
    c->ev_pending.clear();
    c->ev_next = 0;
}

// element pass of a force evaluation: gradients + per-element nodal forces; F / sigma stay un-stored (gp_lazy)
int force_pass(Ctx* c, const double* d_u, const GeomDamping* gd = nullptr) {
    c->post_small = false;                           // sigma is about to be the stress of this evaluation (now or lazily)
    if (c->opt_tangent == 1) {                       // the consistent tangent reads F and sigma right away
        c->gp_lazy = false;
        return launch_geom(c, d_u, GEOM_DSDX | GEOM_F | GEOM_SIGMA | GEOM_FE, gd);
    }
    int rc = launch_geom(c, d_u, GEOM_DSDX | GEOM_FE, gd);
    if (rc) return rc;
    FEMCY_HIP(hipMemcpyAsync(c->d_u_lazy, d_u, sizeof(double) * c->n, hipMemcpyDeviceToDevice, c->stream));
    c->gp_lazy = true;
    return FEMCY_OK;
}

int ensure_gp_stress(Ctx* c) {
    if (!c->gp_lazy) return FEMCY_OK;
    c->gp_lazy = false;
    return launch_geom(c, c->d_u_lazy, GEOM_F | GEOM_SIGMA);
}

}  // namespace femcy

using namespace femcy;

#define CTX_OR_FAIL(ctx)                            \
    FEMCY_REQUIRE((ctx), TEXT_NULL_CONTEXT);                        \
    Ctx* c = &(ctx)->c;                             \
    if (hipSetDevice(c->device) != hipSuccess) {    \
        femcy::set_error("hipSetDevice(%d) failed", c->device); \
        return FEMCY_EHIP;                          \
    }

// device -> host, landed on return
static int download(Ctx* c, void* dst, const void* src, size_t bytes) {
    FEMCY_HIP(hipMemcpyAsync(dst, src, bytes, hipMemcpyDeviceToHost, c->stream));
    FEMCY_HIP(hipStreamSynchronize(c->stream));
    return FEMCY_OK;
}

// The tail the femcy_*_create calls of the element-pass objects share: wait for the kernels (they read scratch the caller
// releases when it returns), name the failure, keep the object, hand out its id.  `failed`: the text when the kernels failed;
// `what`: the object in the out-of-memory text.
template <class T>
static int finish_create(Ctx* c, int rc, std::vector<T>& objects, T& obj, const char* failed, const char* what, int32_t* id_out) {
    if (!rc && hipStreamSynchronize(c->stream) != hipSuccess) {
        set_error("%s", failed);
        rc = FEMCY_EHIP;
    }
    if (rc) {
        if (rc == FEMCY_ENOMEM) set_error("out of device memory for %s on %d elements", what, c->ne);
        return rc;
    }
    objects.push_back(std::move(obj));
    *id_out = (int32_t)objects.size() - 1;
    return FEMCY_OK;
}

extern "C" {

const char* femcy_last_error(void) { return g_err; }
int femcy_version(void) { return 100; }

int femcy_ctx_create(int device, femcy_ctx** out) {
    FEMCY_REQUIRE(out, TEXT_CTX_OUT_NULL);
    *out = nullptr;
    int count = 0;
    hipError_t e = hipGetDeviceCount(&count);
    if (e != hipSuccess || count <= 0) {
        set_error("no HIP device available (%s); libfemcy_hip has no CPU path", e == hipSuccess ? "count = 0" : hipGetErrorString(e));
        return FEMCY_EHIP;
    }
    if (device < 0 || device >= count) {
        set_error("device %d out of range (have %d)", device, count);
        return FEMCY_EINVAL;
    }
    FEMCY_HIP(hipSetDevice(device));
    femcy_ctx* ctx = new (std::nothrow) femcy_ctx();
    if (!ctx) return FEMCY_ENOMEM;
    Ctx* c = &ctx->c;
    c->device = device;
    hipError_t se = hipStreamCreateWithFlags(&c->stream, hipStreamNonBlocking);
    if (se != hipSuccess) {
        set_error("hipStreamCreate failed: %s", hipGetErrorString(se));
        delete ctx;
        return FEMCY_EHIP;
    }
    int rc = FEMCY_OK;
    // + a zero slot behind each partial array (read by out-of-range lanes of the PCG kernels, never written)
    if ((rc = dev_alloc(c->d_part1, (size_t)MAX_PARTIALS + 8)) || (rc = dev_alloc(c->d_part2, (size_t)2 * MAX_PARTIALS + 8)) ||
        (rc = dev_alloc(c->d_state, 1))) {
        delete ctx;
        return rc;
    }
    if (hipHostMalloc((void**)&c->h_state, sizeof(PcgState), hipHostMallocDefault) != hipSuccess ||
        hipHostMalloc((void**)&c->h_scalar, 4096, hipHostMallocDefault) != hipSuccess) {
        set_error("hipHostMalloc failed");
        delete ctx;
        return FEMCY_ENOMEM;
    }
    {
        int lds = 0, cus = 0;
        if (hipDeviceGetAttribute(&lds, hipDeviceAttributeMaxSharedMemoryPerBlock, device) == hipSuccess && lds > 0)
            c->small_max_lds = lds;
        if (hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, device) == hipSuccess && cus > 0)
            c->small_max_wg = std::max(1, cus / 2);   // one workgroup per CU with half the chip to spare
        c->persist_cus = cus;
    }
    *out = ctx;
    return FEMCY_OK;
}

int femcy_ctx_destroy(femcy_ctx* ctx) {
    if (!ctx) return FEMCY_OK;
    Ctx* c = &ctx->c;
    (void)hipSetDevice(c->device);
    if (c->stream) (void)hipStreamSynchronize(c->stream);
    // every stream of the context is drained BEFORE the first buffer is freed (round-6 audit: the exchange stream was
    // synchronised after the frees; its work is ordered behind events of the main stream, so nothing was in flight in
    // practice, but a freed block may be handed to another context at once)
    if (c->comm_stream) (void)hipStreamSynchronize(c->comm_stream);
    comm_destroy(c);
    pcg_graph_reset(c);
    direct_release(c);
    if (c->ev_iface) (void)hipEventDestroy(c->ev_iface);
    if (c->ev_xchg) (void)hipEventDestroy(c->ev_xchg);
    if (c->h_state) (void)hipHostFree(c->h_state);
    if (c->h_stage) (void)hipHostFree(c->h_stage);
    if (c->h_scalar) (void)hipHostFree(c->h_scalar);
    for (auto& p : c->ev_pool) {
        (void)hipEventDestroy(p.a);
        (void)hipEventDestroy(p.b);
    }
    // The one place that orders the device frees of a context.  Every buffer is a DevBuf -- a member of Ctx or of an object
    // it handed out by id -- and all of them go HERE, with `delete`: the context's device current, both streams drained,
    // after comm_destroy / pcg_graph_reset / direct_release (the peers' mappings, the graph and the factorisation that read
    // them are gone), and before either stream is destroyed -- which is why the stream handles outlive the context.
    const hipStream_t stream = c->stream, comm_stream = c->comm_stream;
    delete ctx;
    if (comm_stream) (void)hipStreamDestroy(comm_stream);
    if (stream) (void)hipStreamDestroy(stream);
    return FEMCY_OK;
}

int femcy_set_option(femcy_ctx* ctx, int option, int64_t value) {
    CTX_OR_FAIL(ctx);
    FEMCY_TRY(check_option(c, option, value));
    switch (option) {
        case FEMCY_OPT_ASSEMBLY:
            FEMCY_REQUIRE(value >= FEMCY_ASM_GATHER && value <= FEMCY_ASM_PAIRS, "bad assembly mode %lld", (long long)value);
            FEMCY_REQUIRE(value != 7, "assembly mode 7 is retired");
            c->opt_assembly = (int)value;
            break;
        case FEMCY_OPT_DIRECT_MAX_BYTES:
            return direct_set_max_bytes(c, value);
        case FEMCY_OPT_PCG_POLL:
            FEMCY_REQUIRE(value >= 1, "poll interval must be >= 1");
            c->opt_poll = (int)value;
            break;
        case FEMCY_OPT_TIMING:
            if (!value) timing_collect(c);
            c->opt_timing = value < 0 ? 0 : (int)value;
            break;
        case FEMCY_OPT_EW_GRID:
            FEMCY_REQUIRE(value >= 1 && value <= MAX_PARTIALS, "element-wise grid cap out of range");
            pcg_graph_reset(c);
            c->ew_cap = (int)value;
            break;
        case FEMCY_TUNE_SPMV_WG_PER_XCD:   /* test knob: SpMV workgroups per XCD (1 forces the in-kernel loop on small meshes) */
            FEMCY_REQUIRE(value >= 0 && value <= 512, "workgroups per XCD: 0 (by the size of the range) or 1 .. 512");
            c->spmv_bpx_cap = (int32_t)value;
            if (c->have_pattern) {
                pcg_graph_reset(c);
                spmv_split(c);
            }
            break;
        case FEMCY_OPT_EXCHANGE:
            FEMCY_REQUIRE(value == 0 || value == 1, "exchange: 0 (all-reduce) or 1 (neighbour send/recv)");
            FEMCY_REQUIRE(value == 0 || c->d_if_ptr, "femcy_comm_set_neighbours must come first");
            c->exchange = (int)value;
            break;
        case FEMCY_OPT_PCG_PERSIST:
            FEMCY_REQUIRE(value >= 0 && value <= 2, "persistent PCG: 0 (off), 1 (auto) or 2 (whenever the slices fit)");
            c->opt_persist = (int)value;
            c->persist_failed = false;
            break;
        case FEMCY_TUNE_PERSIST_LDS_ROWS:   /* test knob: block rows per wave of the persistent PCG kept in LDS (-1 = as many as fit) */
            FEMCY_REQUIRE(value >= -1 && value <= 64, "resident block rows out of range");
            c->opt_persist_lds = (int)value;
            break;
        case FEMCY_TUNE_SPMV_KEEP:   /* tuning: per-mille of every XCD's slice range that keeps the default cache policy in the NT SpMV */
            FEMCY_REQUIRE(value >= -1 && value <= 1000, "per-mille out of range (-1 = auto)");
            c->opt_spmv_keep = (int)value;
            if (c->have_pattern) {
                pcg_graph_reset(c);
                spmv_split(c);
            }
            break;
        case FEMCY_TUNE_SMALL_REG_ROWS:   /* test knob: register-resident block rows per wave of the small-system PCG (-1 = a wave's share) */
            FEMCY_REQUIRE(value >= -1 && value <= 64, "register-resident rows out of range");
            c->opt_small_rr = (int)value;
            break;
        case FEMCY_TUNE_PERSIST_WGS:   /* test knob: workgroups of the persistent PCG (0 = one per CU) -- exercises the barrier time-out */
            FEMCY_REQUIRE(value >= 0 && value <= 4096, "workgroup count out of range");
            c->opt_persist_wgs = (int)value;
            c->persist_failed = false;
            break;
        case FEMCY_TUNE_SKIP_OCCUPANCY_CHECK:
            c->opt_skip_occupancy = value ? 1 : 0;
            c->persist_failed = c->small_failed = false;
            break;
        case FEMCY_TUNE_BARRIER_SPIN_LIMIT:
            FEMCY_REQUIRE(value >= 0 && value <= (1ll << 30), "spin limit out of range");
            c->barrier_spin_limit = (uint32_t)value;
            c->persist_failed = c->small_failed = false;
            break;
        case FEMCY_OPT_PCG_PERSIST_MULTI:
            FEMCY_REQUIRE(value == 0 || value == 1, "persistent multi-rank PCG: 0 (off) or 1 (when every rank agreed)");
            c->opt_persist_multi = (int)value;
            c->persist_multi_failed = false;
            break;
        case FEMCY_TUNE_DIRECT_UPDATE:
            return direct_set_update_variant(c, value);
        case FEMCY_TUNE_SPMV_ROT:
            FEMCY_REQUIRE(value >= -1 && value <= 64, "SpMV task lists: -1 (by the spread of the row lengths), 0 (plain), 1 .. 63 (rounds rotated), 64 (balanced by the host)");
            c->opt_spmv_rot = (int32_t)value;
            if (c->have_pattern) {
                pcg_graph_reset(c);
                spmv_split(c);
            }
            break;
        case FEMCY_TUNE_PAIRS:
            if (value == -1) value = FEMCY_PAIRS_DEFAULT;
            FEMCY_REQUIRE(value >= 0 && value < 1024 && ((value >> 1) & 3) <= 1 && ((value >> 3) & 3) <= 2, "PAIRS assembly knobs: -1 (default) or bit 0 "
                          "XCD-contiguous, bits 1-2 rows per wave (0: 16, 1: 8), bits 3-4 steps in flight - 2 (0..2), bit 5 Morton order, "
                          "bits 6-9 chunks per wave - 1");
            c->tune_pairs = (int)value;
            break;
        case FEMCY_TUNE_PERSIST_MAX_MB:
            FEMCY_REQUIRE(value >= 0 && value <= (1 << 20), "streamed-matrix limit of the persistent PCG: 0 (none) .. 2^20 MiB");
            c->persist_max_bytes = value == 0 ? ((int64_t)1 << 40) : ((int64_t)value << 20);
            break;
        case FEMCY_TUNE_PERSIST_L2_ROWS:
            FEMCY_REQUIRE(value >= 0 && value <= 64, "rows out of range");
            c->opt_persist_l2rows = (int)value;
            break;
        case FEMCY_TUNE_PERSIST_VARIANT:
            FEMCY_REQUIRE(value >= -1 && value <= 15 && (value < 8 || value == 14), "variant bits: -1 (default), 0..7 or 14");
            c->opt_persist_variant = (int)value;
            break;
        case FEMCY_TUNE_PERSIST_PROBE:   /* timing experiments: bit 0 no streamed rows, 1 no LDS rows, 2 no register rows, 3 no barrier wait */
#ifdef FEMCY_PERSIST_PROBE
            c->opt_persist_dbg = (int)value;
            break;
#else
            FEMCY_REQUIRE(value == 0 || value == 16, "option 106: the work-skipping timing switches (bits 0-3) exist only in a "
                                                     "-DFEMCY_PERSIST_PROBE build; 16 (no prefetch during the barriers) is always available");
            c->opt_persist_dbg = (int)value;
            break;
#endif
        case FEMCY_TUNE_PERSIST_REG_ROWS:   /* test knob: block rows per slice of the persistent PCG kept in registers (0, 4 or 5) */
            FEMCY_REQUIRE(value == 0 || value == 4 || value == 5, "register-resident block rows: 0, 4 or 5");
            c->opt_persist_rj = (int)value;
            break;
        case FEMCY_OPT_PCG_SMALL:
            FEMCY_REQUIRE(value == 0 || value == 1, "small-system PCG: 0 (off) or 1 (auto)");
            c->opt_small = (int)value;
            c->small_failed = false;
            break;
        case FEMCY_OPT_OVERLAP:
            FEMCY_REQUIRE(value == 0 || value == 1, "overlap: 0 (one stream) or 1 (exchange overlapped with the interior product)");
            c->opt_overlap = (int)value;
            break;
        case FEMCY_OPT_TANGENT:
            c->opt_tangent = (int)value;
            break;
        case FEMCY_TUNE_VEC_NT:   /* test knob: PCG vector kernels with non-temporal loads / stores */
            FEMCY_REQUIRE(value >= -1 && value <= 1, "non-temporal switch must be -1, 0 or 1");
            c->opt_vec_nt = (int)value;
            if (c->have_pattern) {
                pcg_graph_reset(c);
                spmv_split(c);
            }
            break;
        case FEMCY_TUNE_SPMV_NT:   /* test knob: SpMV matrix loads non-temporal (-1 auto: matrix larger than the Infinity Cache) */
            FEMCY_REQUIRE(value >= -1 && value <= 1, "non-temporal switch must be -1, 0 or 1");
            c->opt_spmv_nt = (int)value;
            if (c->have_pattern) {
                pcg_graph_reset(c);
                spmv_split(c);
            }
            break;
        case FEMCY_TUNE_TIMING_FENCE:   /* debugging knob: empty kernel before a sampled SpMV dispatch */
            c->opt_timing_fence = value ? 1 : 0;
            break;
        case FEMCY_OPT_SELL_SIGMA:
            c->sell_sigma = (int32_t)value;
            break;
        case FEMCY_OPT_PCG_STORAGE_ORDER:
            FEMCY_REQUIRE(value == 0 || value == 1, "storage-order PCG: 0 (node order) or 1");
            pcg_graph_reset(c);
            c->opt_pos_space = (int)value;
            break;
        case FEMCY_OPT_NODE_ORDER:
            c->opt_node_order = (int)value;
            break;
        case FEMCY_OPT_PCG_GRAPH:
            FEMCY_REQUIRE(value >= 0 && value <= 2, "graph mode must be 0 (off), 1 (auto) or 2 (always)");
            c->opt_graph = (int)value;
            break;
        case FEMCY_OPT_SPMV_VARIANT:
            FEMCY_REQUIRE(value == 0 || value == 1 || value == 2 || value == 4, "wavefronts per slice: 0 (auto), 1, 2 or 4");
            c->opt_spmv_variant = (int)value;
            if (c->have_pattern) {
                pcg_graph_reset(c);
                spmv_split(c);
            }
            break;
        default:
            set_error(TEXT_UNKNOWN_OPTION, option);
            return FEMCY_EINVAL;
    }
    return FEMCY_OK;
}

int femcy_sync(femcy_ctx* ctx) {
    CTX_OR_FAIL(ctx);
    FEMCY_HIP(hipStreamSynchronize(c->stream));
    return FEMCY_OK;
}

// ------------------------------------------------------------------------- problem definition
int femcy_set_mesh(femcy_ctx* ctx, int32_t nn, int32_t dm, const double* nodes, int32_t ne, int32_t npe,
                   const int32_t* elems) {
    CTX_OR_FAIL(ctx);
    FEMCY_TRY(check_set_mesh(nn, dm, nodes, ne, npe, elems));
    FEMCY_REQUIRE(!c->comm, "the mesh of a context cannot change once a communicator is attached");
    FEMCY_HIP(hipStreamSynchronize(c->stream));
    // a new mesh invalidates everything that was defined on the old one
    drop_objects(c);
    c->post_small = false;
    c->have_material = false;
    c->nn = nn; c->dm = dm; c->ne = ne; c->npe = npe;
    c->n = (int64_t)nn * dm;
    c->h_elems.assign(elems, elems + (int64_t)ne * npe);
    c->h_nodes.assign(nodes, nodes + (int64_t)nn * dm);
    int rc;
    if ((rc = dev_alloc(c->d_nodes, (size_t)nn * dm, false))) return rc;
    if ((rc = dev_alloc(c->d_elems, (size_t)ne * npe, false))) return rc;
    FEMCY_HIP(hipMemcpy(c->d_nodes, nodes, sizeof(double) * nn * dm, hipMemcpyHostToDevice));
    FEMCY_HIP(hipMemcpy(c->d_elems, elems, sizeof(int32_t) * (size_t)ne * npe, hipMemcpyHostToDevice));
    // vectors are padded (zero) so that double2 kernels may touch one element past n
    const size_t nalloc = (size_t)((c->n + 63) / 64 * 64 + 64);
    for (auto& v : c->d_vec)
        if ((rc = dev_alloc(v, nalloc))) return rc;
    // the PCG work vectors also hold the storage-order form (whole slices of 64 nodes)
    const size_t palloc = std::max(nalloc, (size_t)((int64_t)(nn + SLICE - 1) / SLICE * SLICE * dm + 64));
    if ((rc = dev_alloc(c->d_r, palloc)) || (rc = dev_alloc(c->d_d, palloc)) || (rc = dev_alloc(c->d_M, palloc)) ||
        (rc = dev_alloc(c->d_Ad, palloc)) || (rc = dev_alloc(c->d_u_lazy, nalloc)))
        return rc;
    c->gp_lazy = false;
    pcg_graph_reset(c);
    c->have_mesh = true;
    c->have_element = c->have_pattern = false;
    return FEMCY_OK;
}

int femcy_set_element(femcy_ctx* ctx, int32_t nGP, const double* dN, const double* w, int32_t voigt_kind) {
    CTX_OR_FAIL(ctx);
    FEMCY_TRY(check_set_element(c, nGP, dN, w, voigt_kind));
    FEMCY_HIP(hipStreamSynchronize(c->stream));
    c->nGP = nGP;
    c->voigt = voigt_kind;
    // partition of unity of the plugin's shape functions, as far as the kernels see it: sum_a dN_a = 0 at every Gauss
    // point (enables the row-sum diagonal of the assembly; a plugin that violates it keeps the plain sum)
    c->dN_sums_to_zero = true;
    for (int32_t g = 0; g < nGP; ++g)
        for (int32_t d = 0; d < c->dm; ++d) {
            double sum = 0.0, mag = 0.0;
            for (int32_t a = 0; a < c->npe; ++a) {
                const double v = dN[((size_t)g * c->npe + a) * c->dm + d];
                sum += v;
                mag += std::fabs(v);
            }
            if (std::fabs(sum) > 1e-13 * std::max(mag, 1e-300)) c->dN_sums_to_zero = false;
        }
    c->s = (c->dm == 2) ? 3 : 6;
    int rc;
    if ((rc = dev_alloc(c->d_dN, (size_t)nGP * c->npe * c->dm, false))) return rc;
    if ((rc = dev_alloc(c->d_w, (size_t)nGP, false))) return rc;
    FEMCY_HIP(hipMemcpy(c->d_dN, dN, sizeof(double) * nGP * c->npe * c->dm, hipMemcpyHostToDevice));
    FEMCY_HIP(hipMemcpy(c->d_w, w, sizeof(double) * nGP, hipMemcpyHostToDevice));
    const size_t ngp = (size_t)c->ne * nGP;
    if ((rc = dev_alloc(c->d_dsdx, ngp * c->npe * c->dm)) || (rc = dev_alloc(c->d_vol, ngp)) ||
        (rc = dev_alloc(c->d_F, ngp * c->dm * c->dm)) || (rc = dev_alloc(c->d_sigma, ngp * c->dm * c->dm)) ||
        (rc = dev_alloc(c->d_strain, ngp * c->dm * c->dm)) || (rc = dev_alloc(c->d_mises, ngp)) ||
        (rc = dev_alloc(c->d_fe, (size_t)c->ne * c->npe * c->dm)) ||
        (rc = dev_alloc(c->d_energy, ngp)))
        return rc;
    c->have_element = true;
    c->post_small = false;
    c->gp_lazy = false;
    return FEMCY_OK;
}

int femcy_set_material(femcy_ctx* ctx, int32_t kind, const double* C, const double* params, int32_t nparams) {
    CTX_OR_FAIL(ctx);
    FEMCY_TRY(check_set_material(c, kind, C, params, nparams));
    // F / sigma "of the last force evaluation" are kept lazily (Ctx::gp_lazy): materialise them with the material they
    // were evaluated with before it changes
    if (c->gp_lazy && c->have_material && c->have_element) {
        int rcl = ensure_gp_stress(c);
        if (rcl) return rcl;
    }
    FEMCY_HIP(hipStreamSynchronize(c->stream));
    const int s = (c->dm == 2) ? 3 : 6;
    int rc;
    if ((rc = dev_alloc(c->d_C, (size_t)s * s, false))) return rc;
    FEMCY_HIP(hipMemcpy(c->d_C, C, sizeof(double) * s * s, hipMemcpyHostToDevice));
    for (int i = 0; i < s * s; ++i) c->h_C[i] = C[i];
    c->mat_kind = kind;
    // cubic pattern of a 6 x 6 C (exact comparisons: anything else takes the dense-pattern evaluation)
    c->C_is_cubic = false;
    if (s == 6) {
        const double c11 = C[0], c12 = C[1], c44 = C[3 * 6 + 3];
        bool ok = true;
        for (int i = 0; i < 6 && ok; ++i)
            for (int j = 0; j < 6 && ok; ++j) {
                const double want = (i == j) ? (i < 3 ? c11 : c44) : ((i < 3 && j < 3) ? c12 : 0.0);
                ok = C[i * 6 + j] == want;
            }
        c->C_is_cubic = ok;
        c->cubic[0] = c11; c->cubic[1] = c12; c->cubic[2] = c44;
    }
    for (int i = 0; i < 4; ++i) c->mat_params[i] = (i < nparams) ? params[i] : 0.0;
    c->have_material = true;
    c->post_small = false;
    return FEMCY_OK;
}

int femcy_build_pattern(femcy_ctx* ctx) {
    CTX_OR_FAIL(ctx);
    FEMCY_TRY(check_have_mesh(c));
    FEMCY_HIP(hipStreamSynchronize(c->stream));
    pcg_graph_reset(c);
    int rc = build_pattern(c);
    if (rc) return rc;
    c->split_ready = false;
    c->pattern_serial++;
    c->have_pattern = true;
    return FEMCY_OK;
}

int femcy_get_assembly_used(femcy_ctx* ctx, int32_t* mode) {
    CTX_OR_FAIL(ctx);
    FEMCY_TRY(check_get_assembly_used(c, mode));
    *mode = c->asm_used;
    return FEMCY_OK;
}

int femcy_get_pattern_info(femcy_ctx* ctx, femcy_pattern_info* out) {
    CTX_OR_FAIL(ctx);
    FEMCY_REQUIRE(c->have_pattern && out, TEXT_PATTERN_NOT_BUILT);
    out->n = c->n;
    out->nnzb = c->nnzb;
    out->nnz = c->nnzb * c->dm * c->dm;
    out->max_row_blocks = c->max_row_blocks;
    out->ell_width = c->max_row_blocks * c->dm;
    out->stored_blocks = c->stored_rows * SLICE;
    out->nslices = c->nslices;
    out->max_node_elems = c->max_node_elems;
    return FEMCY_OK;
}

int femcy_get_node_order(femcy_ctx* ctx, int32_t* used, double* lines) {
    CTX_OR_FAIL(ctx);
    FEMCY_REQUIRE(c->have_pattern, TEXT_PATTERN_NOT_BUILT);
    if (used) *used = c->node_order_used;
    if (lines)
        for (int k = 0; k < 7; ++k) lines[k] = c->node_order_cost[k];
    return FEMCY_OK;
}

// ---------------------------------------------------------------------------- vector plumbing
int femcy_vec_upload(femcy_ctx* ctx, int vec, const double* src, int64_t n) {
    CTX_OR_FAIL(ctx);
    FEMCY_TRY(check_vec_transfer(c, "upload", vec, src, n));
    FEMCY_HIP(hipMemcpyAsync(c->d_vec[vec], src, sizeof(double) * n, hipMemcpyHostToDevice, c->stream));
    FEMCY_HIP(hipStreamSynchronize(c->stream));
    return FEMCY_OK;
}
int femcy_vec_download(femcy_ctx* ctx, int vec, double* dst, int64_t n) {
    CTX_OR_FAIL(ctx);
    FEMCY_TRY(check_vec_transfer(c, "download", vec, dst, n));
    return download(c, dst, c->d_vec[vec], sizeof(double) * n);
}
int femcy_vec_fill(femcy_ctx* ctx, int vec, double value) {
    CTX_OR_FAIL(ctx);
    VEC_OR_FAIL(vec);
    return vec_fill(c, c->d_vec[vec], value, c->n);
}
int femcy_vec_copy(femcy_ctx* ctx, int dst, int src) {
    CTX_OR_FAIL(ctx);
    VEC_OR_FAIL(dst);
    VEC_OR_FAIL(src);
    if (dst == src) return FEMCY_OK;
    FEMCY_HIP(hipMemcpyAsync(c->d_vec[dst], c->d_vec[src], sizeof(double) * c->n, hipMemcpyDeviceToDevice, c->stream));
    return FEMCY_OK;
}
int femcy_vec_scatter(femcy_ctx* ctx, int vec, const int32_t* idx, const double* vals, int32_t k) {
    CTX_OR_FAIL(ctx);
    VEC_OR_FAIL(vec);
    if (k == 0) return FEMCY_OK;
    FEMCY_TRY(check_vec_scatter(c, idx, vals, k));
    int rc = ensure_scratch(c, k);
    if (rc) return rc;
    // host buffers are only borrowed for the call: staged (the scratch lists are reused by the next scatter, which the
    // stream orders behind this one)
    if ((rc = stage_h2d(c, c->d_idx_scratch, idx, sizeof(int32_t) * k))) return rc;
    if ((rc = stage_h2d(c, c->d_val_scratch, vals, sizeof(double) * k))) return rc;
    return vec_scatter(c, c->d_vec[vec], c->d_idx_scratch, c->d_val_scratch, k);
}
int femcy_vec_sub(femcy_ctx* ctx, int cv, int a, int b) {
    CTX_OR_FAIL(ctx);
    VEC_OR_FAIL(cv); VEC_OR_FAIL(a); VEC_OR_FAIL(b);
    return vec_sub(c, c->d_vec[cv], c->d_vec[a], c->d_vec[b]);
}
int femcy_vec_axpy(femcy_ctx* ctx, int a, int b, double cc, int d) {
    CTX_OR_FAIL(ctx);
    VEC_OR_FAIL(a); VEC_OR_FAIL(b); VEC_OR_FAIL(d);
    return vec_axpy(c, c->d_vec[a], c->d_vec[b], cc, c->d_vec[d]);
}
int femcy_vec_scale(femcy_ctx* ctx, int vec, double s) {
    CTX_OR_FAIL(ctx);
    VEC_OR_FAIL(vec);
    return vec_scale(c, c->d_vec[vec], s);
}
int femcy_vec_norm(femcy_ctx* ctx, int vec, double* rms) {
    CTX_OR_FAIL(ctx);
    VEC_OR_FAIL(vec);
    FEMCY_REQUIRE(rms, TEXT_NULL_OUTPUT);
    double ss = 0.0;
    int rc = vec_sumsq(c, c->d_vec[vec], &ss);
    if (rc) return rc;
    *rms = std::sqrt(ss / (double)(c->comm ? c->n_global : c->n));   // RMS over the whole system
    return FEMCY_OK;
}
int femcy_vec_absmax(femcy_ctx* ctx, int vec, double* out) {
    CTX_OR_FAIL(ctx);
    VEC_OR_FAIL(vec);
    FEMCY_REQUIRE(out, TEXT_NULL_OUTPUT);
    return vec_absmax(c, c->d_vec[vec], out);
}

// -------------------------------------------------------------------------------- the hot path
int femcy_assemble_K(femcy_ctx* ctx, int u_vec) {
    CTX_OR_FAIL(ctx);
    READY_OR_FAIL();
    c->asm_used = -1;                          // femcy_get_assembly_used: nothing ran until the assembly succeeds
    const double* du = nullptr;
    if (u_vec >= 0) {
        VEC_OR_FAIL(u_vec);
        du = c->d_vec[u_vec];
    }
    // the consistent tangent needs F and sigma of this state: the element pass then also evaluates the material
    // (sigma is then no longer what femcy_compute_strain_stress(large = 0) left: femcy_thermal_stress must not correct it)
    if (c->opt_tangent == 1) c->gp_lazy = c->post_small = false;
    int rc = launch_geom(c, du, c->opt_tangent == 1 ? (GEOM_DSDX | GEOM_F | GEOM_SIGMA) : GEOM_DSDX);
    if (rc) return rc;
    if ((rc = launch_assemble(c))) return rc;
    c->K_serial = c->pattern_serial;
    return FEMCY_OK;
}

int femcy_internal_force(femcy_ctx* ctx, int u_vec, int f_vec) {
    CTX_OR_FAIL(ctx);
    READY_OR_FAIL();
    VEC_OR_FAIL(u_vec);
    VEC_OR_FAIL(f_vec);
    int rc = force_pass(c, c->d_vec[u_vec]);
    if (rc) return rc;
    if ((rc = launch_nodal_force(c, c->d_vec[f_vec]))) return rc;
    return iface_sum(c, c->d_vec[f_vec]);      // multi-rank: forces of the elements other ranks hold (no-op otherwise)
}

int femcy_residual_and_K(femcy_ctx* ctx, int u_vec, int f_vec) {
    CTX_OR_FAIL(ctx);
    READY_OR_FAIL();
    c->asm_used = -1;                          // femcy_get_assembly_used: nothing ran until the assembly succeeds
    VEC_OR_FAIL(u_vec);
    VEC_OR_FAIL(f_vec);
    // ONE element pass for both halves of a Newton residual evaluation: the internal force and the matrix are
    // evaluated on the same displacement, so the gradients the force pass leaves are the ones the assembly reads
    int rc = force_pass(c, c->d_vec[u_vec]);
    if (rc) return rc;
    if ((rc = launch_nodal_force(c, c->d_vec[f_vec]))) return rc;
    if ((rc = iface_sum(c, c->d_vec[f_vec]))) return rc;
    if ((rc = launch_assemble(c))) return rc;
    c->K_serial = c->pattern_serial;
    return FEMCY_OK;
}

// the checked DOFs (and values) of a Dirichlet call into the scratch lists
static int stage_dofs(Ctx* c, const int32_t* dofs, const double* vals, int32_t k) {
    if (k == 0) return FEMCY_OK;
    int rc = ensure_scratch(c, k);
    if (rc) return rc;
    FEMCY_HIP(hipMemcpyAsync(c->d_idx_scratch, dofs, sizeof(int32_t) * k, hipMemcpyHostToDevice, c->stream));
    if (vals) FEMCY_HIP(hipMemcpyAsync(c->d_val_scratch, vals, sizeof(double) * k, hipMemcpyHostToDevice, c->stream));
    return FEMCY_OK;
}

int femcy_apply_dirichlet_linear(femcy_ctx* ctx, const int32_t* dofs, const double* vals, int32_t k, int rhs_vec) {
    CTX_OR_FAIL(ctx);
    READY_OR_FAIL();
    VEC_OR_FAIL(rhs_vec);
    if (k == 0 && !c->comm) return FEMCY_OK;
    FEMCY_TRY(check_dirichlet_linear(c, dofs, vals, k, rhs_vec));
    int rc = stage_dofs(c, dofs, vals, k);
    if (rc) return rc;
    // multi-rank: the elimination below is collective (other ranks may hold prescribed values even if this one
    // holds none), so it always runs
    bool any = c->comm != nullptr;
    for (int32_t i = 0; i < k; ++i) any = any || (vals[i] != 0.0);
    if (any) {
        // rhs -= K s  (s = prescribed values, 0 elsewhere): column-wise elimination through one SpMV with
        // the not-yet-modified matrix, equal to the reference's per-entry rhs[j] -= s*K[j][i] by symmetry
        double* s = c->d_vec[FEMCY_VEC_TMP0];
        double* Ks = c->d_vec[FEMCY_VEC_TMP1];
        if ((rc = vec_fill(c, s, 0.0, c->n))) return rc;
        if ((rc = vec_scatter(c, s, c->d_idx_scratch, c->d_val_scratch, k))) return rc;
        if ((rc = launch_spmv(c, s, Ks, nullptr, nullptr))) return rc;
        if ((rc = iface_sum(c, Ks))) return rc;
        if ((rc = vec_sub(c, c->d_vec[rhs_vec], c->d_vec[rhs_vec], Ks))) return rc;
    }
    if ((rc = vec_scatter(c, c->d_vec[rhs_vec], c->d_idx_scratch, c->d_val_scratch, k))) return rc;
    if ((rc = launch_dirichlet_zero(c, c->d_idx_scratch, k, nullptr))) return rc;
    FEMCY_HIP(hipStreamSynchronize(c->stream));
    return FEMCY_OK;
}

int femcy_apply_dirichlet_newton(femcy_ctx* ctx, const int32_t* dofs, int32_t k, int residual_vec) {
    CTX_OR_FAIL(ctx);
    READY_OR_FAIL();
    VEC_OR_FAIL(residual_vec);
    if (k == 0) return FEMCY_OK;
    FEMCY_TRY(check_dirichlet_newton(c, dofs, k));
    int rc = stage_dofs(c, dofs, nullptr, k);
    if (rc) return rc;
    if ((rc = launch_dirichlet_zero(c, c->d_idx_scratch, k, c->d_vec[residual_vec]))) return rc;
    FEMCY_HIP(hipStreamSynchronize(c->stream));
    return FEMCY_OK;
}

int femcy_dofset_create(femcy_ctx* ctx, const int32_t* dofs, int32_t k, int32_t* id_out) {
    CTX_OR_FAIL(ctx);
    FEMCY_TRY(check_dofset_create(c, dofs, k, id_out));
    Ctx::DofSet ds;
    ds.k = k;
    FEMCY_HIP(ds.d_dofs.alloc(std::max<size_t>(k, 1) * sizeof(int32_t)));
    FEMCY_HIP(ds.d_vals.alloc(std::max<size_t>(k, 1) * sizeof(double)));
    if (k) FEMCY_HIP(hipMemcpy(ds.d_dofs.get(), dofs, sizeof(int32_t) * k, hipMemcpyHostToDevice));
    c->dofsets.push_back(std::move(ds));
    *id_out = (int32_t)c->dofsets.size() - 1;
    return FEMCY_OK;
}

int femcy_dofset_dirichlet_newton(femcy_ctx* ctx, int32_t id, int residual_vec) {
    CTX_OR_FAIL(ctx);
    READY_OR_FAIL();
    VEC_OR_FAIL(residual_vec);
    FEMCY_OBJECT_OR_FAIL(ds, c->dofsets, id, "dofset");
    return launch_dirichlet_zero(c, ds.d_dofs.get(), ds.k, c->d_vec[residual_vec]);
}

int femcy_dofset_fill(femcy_ctx* ctx, int32_t id, int vec, double value) {
    CTX_OR_FAIL(ctx);
    VEC_OR_FAIL(vec);
    FEMCY_OBJECT_OR_FAIL(ds, c->dofsets, id, "dofset");
    return vec_scatter_const(c, c->d_vec[vec], ds.d_dofs.get(), value, ds.k);
}

int femcy_dofset_add(femcy_ctx* ctx, int32_t id, int vec, double value) {
    CTX_OR_FAIL(ctx);
    VEC_OR_FAIL(vec);
    FEMCY_OBJECT_OR_FAIL(ds, c->dofsets, id, "dofset");
    return vec_scatter_add(c, c->d_vec[vec], ds.d_dofs.get(), value, ds.k);
}

int femcy_dofset_scatter(femcy_ctx* ctx, int32_t id, int vec, const double* vals) {
    CTX_OR_FAIL(ctx);
    VEC_OR_FAIL(vec);
    FEMCY_OBJECT_OR_FAIL(ds, c->dofsets, id, "dofset");
    if (ds.k == 0) return FEMCY_OK;
    FEMCY_REQUIRE(vals, TEXT_NULL_VALUES);
    int rc = stage_h2d(c, ds.d_vals.get(), vals, sizeof(double) * ds.k);   // the host buffer is only borrowed for the call
    if (rc) return rc;
    return vec_scatter(c, c->d_vec[vec], ds.d_dofs.get(), ds.d_vals.get(), ds.k);
}

int femcy_dofset_dirichlet_linear(femcy_ctx* ctx, int32_t id, double value, int rhs_vec) {
    CTX_OR_FAIL(ctx);
    READY_OR_FAIL();
    VEC_OR_FAIL(rhs_vec);
    FEMCY_OBJECT_OR_FAIL(ds, c->dofsets, id, "dofset");
    FEMCY_TRY(check_rhs_not_scratch(rhs_vec));
    if (ds.k == 0 && !c->comm) return FEMCY_OK;
    int rc;
    if (value != 0.0) {   // rhs -= K s with s = value on the block's DOFs (see femcy_apply_dirichlet_linear); collective
        double* s = c->d_vec[FEMCY_VEC_TMP0];
        double* Ks = c->d_vec[FEMCY_VEC_TMP1];
        if ((rc = vec_fill(c, s, 0.0, c->n))) return rc;
        if ((rc = vec_scatter_const(c, s, ds.d_dofs.get(), value, ds.k))) return rc;
        if ((rc = launch_spmv(c, s, Ks, nullptr, nullptr))) return rc;
        if ((rc = iface_sum(c, Ks))) return rc;
        if ((rc = vec_sub(c, c->d_vec[rhs_vec], c->d_vec[rhs_vec], Ks))) return rc;
    }
    if ((rc = vec_scatter_const(c, c->d_vec[rhs_vec], ds.d_dofs.get(), value, ds.k))) return rc;
    return launch_dirichlet_zero(c, ds.d_dofs.get(), ds.k, nullptr);
}

// ------------------------------------------------------------------------------- Neumann load sets
int femcy_loadset_create(femcy_ctx* ctx, int32_t nft, int32_t nfn, int32_t nip, const int32_t* ft_nodes,
                         const double* ft_N, const double* ft_dN, const double* ft_normal, const double* ft_weight,
                         int32_t nload, const int32_t* load_elem, const int32_t* load_ft, int32_t* id_out) {
    CTX_OR_FAIL(ctx);
    FEMCY_TRY(check_loadset_create(c, nft, nfn, nip, ft_nodes, ft_N, ft_dN, ft_normal, ft_weight, nload, load_elem, load_ft,
                                   id_out));
    // loaded nodes and, per node, its contribution slots (facet * nfn + facet node) in ascending order
    const size_t nslot = (size_t)nload * nfn;
    std::vector<int32_t> slot_node(nslot), order(nslot);
    for (int32_t l = 0; l < nload; ++l)
        for (int32_t f = 0; f < nfn; ++f)
            slot_node[(size_t)l * nfn + f] = c->h_elems[(size_t)load_elem[l] * c->npe + ft_nodes[(size_t)load_ft[l] * nfn + f]];
    for (size_t i = 0; i < nslot; ++i) order[i] = (int32_t)i;
    std::stable_sort(order.begin(), order.end(), [&](int32_t a, int32_t b) { return slot_node[a] < slot_node[b]; });
    std::vector<int32_t> ld_node, ld_ptr;
    for (size_t i = 0; i < nslot; ++i) {
        if (i == 0 || slot_node[order[i]] != slot_node[order[i - 1]]) {
            ld_node.push_back(slot_node[order[i]]);
            ld_ptr.push_back((int32_t)i);
        }
    }
    ld_ptr.push_back((int32_t)nslot);

    Ctx::LoadSet ls;
    ls.nft = nft; ls.nfn = nfn; ls.nip = nip; ls.nload = nload; ls.nnode = (int32_t)ld_node.size();
    int rc = FEMCY_OK;
    const size_t tip = (size_t)nft * nip;
    if (!rc) rc = dev_upload(ls.d_ft_nodes, ft_nodes, sizeof(int32_t) * nft * nfn);
    if (!rc) rc = dev_upload(ls.d_N, ft_N, sizeof(double) * tip * c->npe);
    if (!rc) rc = dev_upload(ls.d_dN, ft_dN, sizeof(double) * tip * c->npe * c->dm);
    if (!rc) rc = dev_upload(ls.d_normal, ft_normal, sizeof(double) * tip * c->dm);
    if (!rc) rc = dev_upload(ls.d_weight, ft_weight, sizeof(double) * tip);
    if (!rc) rc = dev_upload(ls.d_elem, load_elem, sizeof(int32_t) * nload);
    if (!rc) rc = dev_upload(ls.d_ft, load_ft, sizeof(int32_t) * nload);
    if (!rc) rc = dev_upload(ls.d_node, ld_node.data(), sizeof(int32_t) * ld_node.size());
    if (!rc) rc = dev_upload(ls.d_ptr, ld_ptr.data(), sizeof(int32_t) * ld_ptr.size());
    if (!rc) rc = dev_upload(ls.d_slot, order.data(), sizeof(int32_t) * nslot);
    if (!rc && ls.d_contrib.alloc(std::max<size_t>(nslot, 1) * c->dm * sizeof(double)) != hipSuccess) rc = FEMCY_ENOMEM;
    if (!rc && ls.d_dir.alloc(3 * sizeof(double)) != hipSuccess) rc = FEMCY_ENOMEM;
    if (rc) {
        if (rc == FEMCY_ENOMEM) set_error("out of device memory for a load set of %d facets", nload);
        return rc;
    }
    c->loadsets.push_back(std::move(ls));
    *id_out = (int32_t)c->loadsets.size() - 1;
    return FEMCY_OK;
}

static int loadset_neumann(Ctx* c, int32_t id, double traction, const double* direction, int rhs_vec, bool add) {
    VEC_OR_FAIL(rhs_vec);
    FEMCY_OBJECT_OR_FAIL(ls, c->loadsets, id, "load set");
    return apply_load(c, "femcy_loadset_neumann_add", rhs_vec, add, [&](double* dst, bool add_to) -> int {
        if (direction) {
            FEMCY_HIP(hipMemcpyAsync(ls.d_dir.get(), direction, sizeof(double) * c->dm, hipMemcpyHostToDevice, c->stream));
            FEMCY_HIP(hipStreamSynchronize(c->stream));   // the host buffer is only borrowed for the call
        }
        return launch_neumann(c, ls, traction, direction == nullptr, dst, add_to);
    });
}

int femcy_loadset_neumann(femcy_ctx* ctx, int32_t id, double traction, const double* direction, int rhs_vec) {
    CTX_OR_FAIL(ctx);
    return loadset_neumann(c, id, traction, direction, rhs_vec, false);
}

int femcy_loadset_neumann_add(femcy_ctx* ctx, int32_t id, double traction, const double* direction, int rhs_vec) {
    CTX_OR_FAIL(ctx);
    return loadset_neumann(c, id, traction, direction, rhs_vec, true);
}

// ----------------------------------------------------------------------------------- body loads
int femcy_bodyload_create(femcy_ctx* ctx, const double* N, int32_t nsel, const int32_t* sel_elems, int32_t* id_out) {
    CTX_OR_FAIL(ctx);
    std::vector<uint8_t> mask;
    FEMCY_TRY(check_bodyload_create(c, N, nsel, sel_elems, id_out, mask));
    Ctx::BodyLoad bl;
    bl.nsel = sel_elems ? nsel : c->ne;
    DevBuf<double> d_N, d_we;      // the tables and the element records are scratch of this call
    DevBuf<uint8_t> d_mask;
    int rc = dev_upload(d_N, N, sizeof(double) * c->nGP * c->npe);
    if (!rc && sel_elems) rc = dev_upload(d_mask, mask.data(), mask.size());
    if (!rc && d_we.alloc(sizeof(double) * (size_t)c->ne * c->npe) != hipSuccess) rc = FEMCY_ENOMEM;
    if (!rc && bl.d_m.alloc(sizeof(double) * (size_t)c->nn) != hipSuccess) rc = FEMCY_ENOMEM;
    if (!rc) rc = launch_body_weights(c, d_N.get(), d_mask.get(), d_we.get(), bl.d_m.get());
    return finish_create(c, rc, c->bodyloads, bl, "body load: the weight kernels failed", "a body load", id_out);
}

int femcy_bodyload_weights(femcy_ctx* ctx, int32_t id, double* out) {
    CTX_OR_FAIL(ctx);
    FEMCY_OBJECT_OR_FAIL(bl, c->bodyloads, id, "body load");
    FEMCY_REQUIRE(out, TEXT_NULL_OUTPUT);
    return download(c, out, bl.d_m.get(), sizeof(double) * c->nn);
}

int femcy_bodyload_apply(femcy_ctx* ctx, int32_t id, const double* b, int rhs_vec, int32_t add) {
    CTX_OR_FAIL(ctx);
    FEMCY_TRY(check_bodyload_apply(c, id, b, rhs_vec));
    const Ctx::BodyLoad& bl = c->bodyloads[id];
    return apply_load(c, "femcy_bodyload_apply with add", rhs_vec, add != 0,
                      [&](double* dst, bool add_to) { return launch_body_apply(c, bl.d_m.get(), b, add_to, dst); });
}

// --------------------------------------------------------------------------------- thermal loads
int femcy_thermal_create(femcy_ctx* ctx, const double* N, double alpha, const double* dT, int32_t* id_out) {
    CTX_OR_FAIL(ctx);
    FEMCY_TRY(check_thermal_create(c, N, alpha, dT, id_out));
    Ctx::Thermal th;
    dispatch_dm(c->dm, [&](auto dm) {
        constexpr int DM = dm();
        double s[DM][DM];
        thermal_unit_stress<DM>(c->mat_kind, c->h_C, c->mat_params[1], s);
        for (int i = 0; i < DM * DM; ++i) th.ts.s[i] = alpha * s[i / DM][i % DM];
    });
    DevBuf<double> d_fe;           // the element records are scratch of this call
    int rc = dev_upload(th.d_N, N, sizeof(double) * c->nGP * c->npe);
    if (!rc) rc = dev_upload(th.d_dT, dT, sizeof(double) * (size_t)c->nn);
    if (!rc && d_fe.alloc(sizeof(double) * (size_t)c->ne * c->npe * c->dm) != hipSuccess) rc = FEMCY_ENOMEM;
    if (!rc && th.d_f.alloc(sizeof(double) * (size_t)c->n) != hipSuccess) rc = FEMCY_ENOMEM;
    if (!rc) rc = launch_thermal_force(c, th, d_fe.get());
    return finish_create(c, rc, c->thermals, th, "thermal load: the force kernels failed", "a thermal load", id_out);
}

int femcy_thermal_force(femcy_ctx* ctx, int32_t id, double* out) {
    CTX_OR_FAIL(ctx);
    FEMCY_OBJECT_OR_FAIL(th, c->thermals, id, "thermal load");
    FEMCY_REQUIRE(out, TEXT_NULL_OUTPUT);
    return download(c, out, th.d_f.get(), sizeof(double) * c->n);
}

int femcy_thermal_apply(femcy_ctx* ctx, int32_t id, double scale, int rhs_vec, int32_t add) {
    CTX_OR_FAIL(ctx);
    VEC_OR_FAIL(rhs_vec);
    FEMCY_OBJECT_OR_FAIL(th, c->thermals, id, "thermal load");
    return apply_load(c, "femcy_thermal_apply with add", rhs_vec, add != 0,
                      [&](double* dst, bool add_to) { return launch_thermal_apply(c, th.d_f.get(), scale, add_to, dst); });
}

int femcy_thermal_stress(femcy_ctx* ctx, int32_t id, double scale) {
    CTX_OR_FAIL(ctx);
    FEMCY_TRY(check_thermal_stress(c, id));
    c->post_small = false;
    return launch_thermal_post(c, c->thermals[id], scale);
}

// ------------------------------------------------------------------------------ implicit dynamics
#define SINGLE_RANK_OR_FAIL(name) \
    FEMCY_REQUIRE(!c->comm, name ": the consistent mass is not available on several ranks (femcy_comm_init has run)")

int femcy_mass_create(femcy_ctx* ctx, int32_t nq, const double* Nq, const double* dNq, const double* wq, double rho,
                      int32_t* id_out) {
    CTX_OR_FAIL(ctx);
    SINGLE_RANK_OR_FAIL("femcy_mass_create");
    FEMCY_TRY(check_mass_rule(c, "femcy_mass_create", nq, Nq, dNq, wq, rho, id_out));
    Ctx::Mass ms;
    DevBuf<double> d_Nq, d_dNq, d_wq, d_vq;     // the tables and the element records are scratch of this call
    const size_t npos = (size_t)c->stored_rows * SLICE;
    int rc = dev_upload(d_Nq, Nq, sizeof(double) * nq * c->npe);
    if (!rc) rc = dev_upload(d_dNq, dNq, sizeof(double) * nq * c->npe * c->dm);
    if (!rc) rc = dev_upload(d_wq, wq, sizeof(double) * nq);
    if (!rc && d_vq.alloc(sizeof(double) * (size_t)c->ne * nq) != hipSuccess) rc = FEMCY_ENOMEM;
    if (!rc && ms.d_m.alloc(std::max<size_t>(sizeof(double) * npos, 8)) != hipSuccess) rc = FEMCY_ENOMEM;
    if (!rc) rc = launch_mass_blocks(c, nq, d_Nq.get(), d_dNq.get(), d_wq.get(), rho, d_vq.get(), ms.d_m.get());
    return finish_create(c, rc, c->masses, ms, "mass: the assembly kernels failed", "a mass matrix", id_out);
}

int femcy_mass_get(femcy_ctx* ctx, int32_t id, double* vals) {
    CTX_OR_FAIL(ctx);
    SINGLE_RANK_OR_FAIL("femcy_mass_get");
    FEMCY_OBJECT_OR_FAIL(ms, c->masses, id, "mass object");
    FEMCY_REQUIRE(vals, TEXT_NULL_OUTPUT);
    std::vector<double> m((size_t)c->stored_rows * SLICE);
    FEMCY_TRY(download(c, m.data(), ms.d_m.get(), sizeof(double) * m.size()));
    int64_t w = 0;
    std::vector<std::pair<int32_t, int32_t>> order;
    for (int32_t a = 0; a < c->nn; ++a) {       // the block order of femcy_get_K_bsr
        const int64_t off = c->h_slice_off[c->h_pos[a] / SLICE];
        const int lane = c->h_pos[a] % SLICE, L = c->h_rowlen[a];
        order.clear();
        for (int j = 0; j < L; ++j) order.push_back({c->h_bcol[(off + j) * SLICE + lane], j});
        std::sort(order.begin(), order.end());
        for (auto& pr : order) vals[w++] = m[(off + pr.second) * SLICE + lane];
    }
    return FEMCY_OK;
}

int femcy_mass_apply(femcy_ctx* ctx, int32_t id, int x_vec, int y_vec, double scale, int32_t add) {
    CTX_OR_FAIL(ctx);
    SINGLE_RANK_OR_FAIL("femcy_mass_apply");
    FEMCY_TRY(check_mass_apply(c, id, x_vec, y_vec));
    return launch_mass_spmv(c, c->masses[id].d_m.get(), c->d_vec[x_vec], c->d_vec[y_vec], scale, add != 0, nullptr, nullptr);
}

int femcy_mass_add_to_K(femcy_ctx* ctx, int32_t id, double cc, int32_t overwrite) {
    CTX_OR_FAIL(ctx);
    SINGLE_RANK_OR_FAIL("femcy_mass_add_to_K");
    FEMCY_TRY(check_mass_add_to_K(c, id, cc));
    return launch_mass_add_to_K(c, c->masses[id].d_m.get(), cc, overwrite != 0);
}

int femcy_mass_kinetic_energy(femcy_ctx* ctx, int32_t id, int v_vec, double* out) {
    CTX_OR_FAIL(ctx);
    SINGLE_RANK_OR_FAIL("femcy_mass_kinetic_energy");
    VEC_OR_FAIL(v_vec);
    FEMCY_OBJECT_OR_FAIL(ms, c->masses, id, "mass object");
    FEMCY_REQUIRE(out, TEXT_NULL_OUTPUT);
    return launch_mass_energy(c, ms.d_m.get(), c->d_vec[v_vec], out);
}

int femcy_newmark_predict(femcy_ctx* ctx, int u_vec, int v_vec, int a_vec, int out_vec, double c0, double c1, double c2) {
    CTX_OR_FAIL(ctx);
    FEMCY_TRY(check_newmark_predict(c, u_vec, v_vec, a_vec, out_vec));
    return launch_newmark_predict(c, c->d_vec[u_vec], c->d_vec[v_vec], c->d_vec[a_vec], c->d_vec[out_vec], c0, c1, c2);
}

int femcy_newmark_update(femcy_ctx* ctx, int u_new_vec, int u_vec, int v_vec, int a_vec, double beta, double gamma,
                         double dt) {
    CTX_OR_FAIL(ctx);
    FEMCY_TRY(check_newmark_update(c, u_new_vec, u_vec, v_vec, a_vec, beta, gamma, dt));
    return launch_newmark_update(c, c->d_vec[u_new_vec], c->d_vec[u_vec], c->d_vec[v_vec], c->d_vec[a_vec], beta, gamma, dt);
}

// ------------------------------------------------------------------------------ explicit dynamics
#define EXPLICIT_SINGLE_RANK_OR_FAIL(name) \
    FEMCY_REQUIRE(!c->comm, name ": explicit dynamics is not available on several ranks (femcy_comm_init has run)")

int femcy_lumped_mass_create(femcy_ctx* ctx, int32_t nq, const double* Nq, const double* dNq, const double* wq, double rho,
                             int32_t* id_out) {
    CTX_OR_FAIL(ctx);
    EXPLICIT_SINGLE_RANK_OR_FAIL("femcy_lumped_mass_create");
    FEMCY_TRY(check_mass_rule(c, "femcy_lumped_mass_create", nq, Nq, dNq, wq, rho, id_out));
    Ctx::LumpedMass lm;
    DevBuf<double> d_Nq, d_dNq, d_wq;           // the tables are scratch of this call
    DevBuf<double>& d_me = lm.d_me;             // the element shares stay: the element-by-element increment divides by them
    int rc = dev_upload(d_Nq, Nq, sizeof(double) * nq * c->npe);
    if (!rc) rc = dev_upload(d_dNq, dNq, sizeof(double) * nq * c->npe * c->dm);
    if (!rc) rc = dev_upload(d_wq, wq, sizeof(double) * nq);
    if (!rc && d_me.alloc(sizeof(double) * (size_t)c->ne * c->npe) != hipSuccess) rc = FEMCY_ENOMEM;
    if (!rc && lm.d_m.alloc(sizeof(double) * (size_t)c->nn) != hipSuccess) rc = FEMCY_ENOMEM;
    lm.rho = rho;                               // rho_0 of the bulk viscosity (femcy_explicit_set_damping)
    if (!rc) rc = launch_lumped_mass(c, nq, d_Nq.get(), d_dNq.get(), d_wq.get(), rho, d_me.get(), lm.d_m.get());
    return finish_create(c, rc, c->lumped_masses, lm, "lumped mass: the kernels failed", "a lumped mass", id_out);
}

int femcy_lumped_mass_get(femcy_ctx* ctx, int32_t id, double* out) {
    CTX_OR_FAIL(ctx);
    EXPLICIT_SINGLE_RANK_OR_FAIL("femcy_lumped_mass_get");
    FEMCY_OBJECT_OR_FAIL(lm, c->lumped_masses, id, "lumped mass");
    FEMCY_REQUIRE(out, TEXT_NULL_OUTPUT);
    return download(c, out, lm.d_m.get(), sizeof(double) * c->nn);
}

// Set-up, synchronising: the total mass, the factors (FEMCY_MS_UNIFORM: a measuring pass first, its maximum comes back as an
// argument), and only once the host has seen that omega_e^2 and every factor are finite and positive the apply pass, the
// node sums and the total again.  The estimate of a call without dt serves that test alone and takes s_C = 1.
int femcy_lumped_mass_scale(femcy_ctx* ctx, int32_t lumped_id, double s_C, double factor, double dt, int32_t type,
                            double* mass_before, double* mass_after, int64_t* n_scaled, double* factor_max) {
    CTX_OR_FAIL(ctx);
    READY_OR_FAIL();
    EXPLICIT_SINGLE_RANK_OR_FAIL("femcy_lumped_mass_scale");
    FEMCY_TRY(check_lumped_mass_scale(c, lumped_id, s_C, factor, dt, type, mass_before, mass_after, n_scaled, factor_max));
    Ctx::LumpedMass& lm = c->lumped_masses[lumped_id];
    const int np = explicit_bound_partials(c);
    const bool first = !lm.d_scale.get();
    DevBuf<double> d_fac, d_part, d_scale;      // scratch of this call; d_scale moves to lm with the first apply pass
    if (d_fac.alloc(sizeof(double) * (size_t)c->ne) != hipSuccess || d_part.alloc(sizeof(double) * 3 * (size_t)np) != hipSuccess ||
        (first && d_scale.alloc(sizeof(double) * (size_t)c->ne) != hipSuccess)) {
        set_error("out of device memory for the mass scaling of %d elements", c->ne);
        return FEMCY_ENOMEM;
    }
    const double sc = dt != 0.0 ? s_C : 1.0;
    double res[3] = {0.0, 0.0, 0.0}, w2max = 0.0, m0 = 0.0, m1 = 0.0;
    int rc = launch_mass_total(c, lm.d_m.get(), &m0);
    if (!rc && dt != 0.0 && type == FEMCY_MS_UNIFORM) {
        rc = launch_mass_scale_factors(c, lm.d_me.get(), sc, 0.0, factor, dt, type, true, d_fac.get(), d_part.get(), res);
        w2max = res[0];
    }
    if (!rc && std::isfinite(w2max))
        rc = launch_mass_scale_factors(c, lm.d_me.get(), sc, w2max, factor, dt, type, false, d_fac.get(), d_part.get(), res);
    if (rc) {
        (void)hipStreamSynchronize(c->stream);      // the scratch goes: nothing may still write it
        return rc;
    }
    if (!std::isfinite(w2max) || !std::isfinite(res[0]) || !std::isfinite(res[1])) {
        set_error("femcy_lumped_mass_scale: an element frequency or a factor is not finite and positive (max omega_e^2 = %g, "
                  "max factor = %g): a broken element; the lumped mass is unchanged", std::isfinite(w2max) ? res[0] : w2max,
                  res[1]);
        return FEMCY_ENUMERIC;
    }
    rc = launch_mass_scale_apply(c, d_fac.get(), first, lm.d_me.get(), first ? d_scale.get() : lm.d_scale.get(), lm.d_m.get());
    if (first) lm.d_scale = std::move(d_scale);
    if (!rc) rc = launch_mass_total(c, lm.d_m.get(), &m1);
    if (rc) {
        (void)hipStreamSynchronize(c->stream);
        return rc;
    }
    *mass_before = m0;
    *mass_after = m1;
    *n_scaled = (int64_t)res[2];
    *factor_max = res[1];
    return FEMCY_OK;
}

int femcy_lumped_mass_get_scaling(femcy_ctx* ctx, int32_t lumped_id, double* out) {
    CTX_OR_FAIL(ctx);
    EXPLICIT_SINGLE_RANK_OR_FAIL("femcy_lumped_mass_get_scaling");
    FEMCY_OBJECT_OR_FAIL(lm, c->lumped_masses, lumped_id, "lumped mass");
    FEMCY_REQUIRE(out, TEXT_NULL_OUTPUT);
    if (!lm.d_scale.get()) {
        std::fill(out, out + c->ne, 1.0);
        return FEMCY_OK;
    }
    return download(c, out, lm.d_scale.get(), sizeof(double) * c->ne);
}

int femcy_explicit_create(femcy_ctx* ctx, int32_t lumped_id, int32_t ndofsets, const int32_t* dofset_ids, int32_t* id_out) {
    CTX_OR_FAIL(ctx);
    EXPLICIT_SINGLE_RANK_OR_FAIL("femcy_explicit_create");
    FEMCY_TRY(check_explicit_create(c, lumped_id, ndofsets, dofset_ids, id_out));
    const Ctx::LumpedMass& lm = c->lumped_masses[lumped_id];
    Ctx::Explicit ex;
    ex.lumped = lumped_id;
    ex.held.assign(dofset_ids, dofset_ids + ndofsets);
    if (ex.d_minv.alloc(sizeof(double) * (size_t)c->n) != hipSuccess) {
        set_error("out of device memory for the inverse mass of %lld DOF", (long long)c->n);
        return FEMCY_ENOMEM;
    }
    int rc = launch_explicit_minv(c, lm.d_m.get(), ex.d_minv.get());
    for (int32_t k = 0; !rc && k < ndofsets; ++k) {
        const Ctx::DofSet& ds = c->dofsets[dofset_ids[k]];
        rc = vec_scatter_const(c, ex.d_minv.get(), ds.d_dofs.get(), 0.0, ds.k);
    }
    if (rc) {
        (void)hipStreamSynchronize(c->stream);      // ex goes: nothing may still write its buffer
        return rc;
    }
    c->explicits.push_back(std::move(ex));
    *id_out = (int32_t)c->explicits.size() - 1;
    return FEMCY_OK;
}

// what the damped kernels of an integrator take: v and a (start: a null, v_{-1/2} := v_0 and vec[ACC] is not read), the
// increment of the drift that led to the state from h or, in an automatic run, from the clock
static GeomDamping damping_of(const Ctx* c, const Ctx::Explicit& ex, const ExplicitClock* clk, double h, bool start) {
    return {c->d_vec[FEMCY_VEC_VEL], start ? nullptr : c->d_vec[FEMCY_VEC_ACC], start ? nullptr : clk, h, ex.alpha, ex.b1, ex.b2,
            ex.Md, c->lumped_masses[ex.lumped].rho};
}

int femcy_explicit_set_damping(femcy_ctx* ctx, int32_t id, double alpha, double b1, double b2, double M_d) {
    CTX_OR_FAIL(ctx);
    EXPLICIT_SINGLE_RANK_OR_FAIL("femcy_explicit_set_damping");
    FEMCY_TRY(check_explicit_set_damping(c, id, alpha, b1, b2, M_d));
    Ctx::Explicit& ex = c->explicits[id];
    ex.alpha = alpha;
    ex.b1 = b1;
    ex.b2 = b2;
    ex.Md = M_d;
    return FEMCY_OK;
}

int femcy_amplitude_create(femcy_ctx* ctx, int32_t kind, int32_t npts, const double* t, const double* A, int32_t* id_out) {
    CTX_OR_FAIL(ctx);
    EXPLICIT_SINGLE_RANK_OR_FAIL("femcy_amplitude_create");
    FEMCY_TRY(check_amplitude_create(kind, npts, t, A, id_out));
    Amplitude am{};
    am.kind = kind;
    am.npts = npts;
    std::copy(t, t + npts, am.t);
    std::copy(A, A + npts, am.A);
    c->amplitudes.push_back(am);
    *id_out = (int32_t)c->amplitudes.size() - 1;
    return FEMCY_OK;
}

// Set-up, synchronising: the DOF lists of the sets come back from the device, the tables are built on the host
// (motion_tables.hpp) and replace the integrator's once nothing can still read the old ones.
int femcy_explicit_set_motion(femcy_ctx* ctx, int32_t id, int32_t nsets, const int32_t* dofset_ids, const double* values,
                              const int32_t* amplitude_ids) {
    CTX_OR_FAIL(ctx);
    EXPLICIT_SINGLE_RANK_OR_FAIL("femcy_explicit_set_motion");
    FEMCY_TRY(check_explicit_set_motion(c, id, nsets, dofset_ids, values, amplitude_ids));
    Ctx::Explicit& ex = c->explicits[id];
    std::vector<std::vector<int32_t>> sets((size_t)nsets);
    for (int32_t k = 0; k < nsets; ++k) {
        const Ctx::DofSet& ds = c->dofsets[dofset_ids[k]];
        sets[k].resize((size_t)ds.k);
        if (ds.k) FEMCY_TRY(download(c, sets[k].data(), ds.d_dofs.get(), sizeof(int32_t) * (size_t)ds.k));
    }
    const MotionTables mt = motion_tables(c->n, sets, values, amplitude_ids, c->amplitudes);
    FEMCY_HIP(hipStreamSynchronize(c->stream));
    ex.nmoved = 0;
    ex.d_mslot.reset(), ex.d_mdof.reset(), ex.d_mcurve.reset(), ex.d_mval.reset(), ex.d_amp.reset();
    if (mt.dof.empty()) return FEMCY_OK;
    int rc = dev_upload(ex.d_mslot, mt.slot);
    if (!rc) rc = dev_upload(ex.d_mdof, mt.dof);
    if (!rc) rc = dev_upload(ex.d_mcurve, mt.curve);
    if (!rc) rc = dev_upload(ex.d_mval, mt.val);
    if (!rc) rc = dev_upload(ex.d_amp, mt.amp);
    if (rc) return rc;
    ex.nmoved = (int32_t)mt.dof.size();
    return FEMCY_OK;
}

// the motion tables of an integrator for the launchers, at the times t and t_drift of a fixed step
static ExplicitMotion motion_of(const Ctx::Explicit& ex, double t, double t_drift) {
    return {ex.d_mslot.get(), ex.d_mdof.get(), ex.d_mcurve.get(), ex.d_mval.get(), ex.d_amp.get(), ex.nmoved, t, t_drift};
}

// the energy balance of an integrator for the launchers (femcy_explicit_energy_enable)
static ExplicitEnergy energy_of(const Ctx* c, const Ctx::Explicit& ex) {
    return {c->lumped_masses[ex.lumped].d_m.get(), ex.d_efint.get(), ex.d_ealpha.get(), ex.d_eslot.get()};
}

int femcy_explicit_energy_enable(femcy_ctx* ctx, int32_t id, int32_t on) {
    CTX_OR_FAIL(ctx);
    EXPLICIT_SINGLE_RANK_OR_FAIL("femcy_explicit_energy_enable");
    FEMCY_TRY(check_object(c->explicits, id, "explicit integrator"));
    Ctx::Explicit& ex = c->explicits[id];
    if (!on) {
        ex.energy_want = ex.energy_on = false;
        return FEMCY_OK;
    }
    const size_t nslot = (size_t)explicit_energy_slots(c) * EN_SLOT;
    if ((!ex.d_efint.get() && ex.d_efint.alloc(sizeof(double) * (size_t)c->n) != hipSuccess) ||
        (!ex.d_ealpha.get() && ex.d_ealpha.alloc(sizeof(double) * (size_t)c->n) != hipSuccess) ||
        (!ex.d_eslot.get() && ex.d_eslot.alloc(sizeof(double) * nslot) != hipSuccess)) {
        set_error("out of device memory for the energy balance of %lld DOF", (long long)c->n);
        return FEMCY_ENOMEM;
    }
    ex.energy_want = true;
    return FEMCY_OK;
}

int femcy_explicit_energy_get(femcy_ctx* ctx, int32_t id, double* out) {
    CTX_OR_FAIL(ctx);
    EXPLICIT_SINGLE_RANK_OR_FAIL("femcy_explicit_energy_get");
    FEMCY_TRY(check_explicit_energy_get(c, id, out));
    return launch_explicit_energy_sum(c, c->explicits[id].d_eslot.get(), out);
}

int femcy_explicit_set_wall(femcy_ctx* ctx, int32_t id, int32_t nwalls, const double* point, const double* normal,
                            const double* kappa) {
    CTX_OR_FAIL(ctx);
    EXPLICIT_SINGLE_RANK_OR_FAIL("femcy_explicit_set_wall");
    ExplicitWalls w{};
    FEMCY_TRY(check_explicit_set_wall(c, id, nwalls, point, normal, kappa, w));
    c->explicits[id].walls = w;                     // they travel in the kernel arguments: nothing on the device to replace
    return FEMCY_OK;
}

int femcy_explicit_wall_get(femcy_ctx* ctx, int32_t id, int32_t wall, double* out) {
    CTX_OR_FAIL(ctx);
    EXPLICIT_SINGLE_RANK_OR_FAIL("femcy_explicit_wall_get");
    FEMCY_TRY(check_explicit_wall_get(c, id, wall, out));
    const Ctx::Explicit& ex = c->explicits[id];
    return launch_explicit_wall_get(c, ex.walls, wall, c->lumped_masses[ex.lumped].d_m.get(), ex.d_minv.get(), out);
}

int femcy_explicit_start(femcy_ctx* ctx, int32_t id, int rhs_vec, double scale) {
    CTX_OR_FAIL(ctx);
    READY_OR_FAIL();
    EXPLICIT_SINGLE_RANK_OR_FAIL("femcy_explicit_start");
    FEMCY_TRY(check_explicit_start(c, id, rhs_vec, scale));
    Ctx::Explicit& ex = c->explicits[id];
    ex.n_done = ex.n_base = 0;                      // the clock of a fixed run: t = 0
    ex.t_base = ex.dt_prev = 0.0;
    const ExplicitMotion mv = motion_of(ex, 0.0, 0.0);
    int rc = ex.nmoved ? launch_explicit_place(c, mv, nullptr, 0.0, MOVE_U | MOVE_V | MOVE_A) : FEMCY_OK;
    if (rc) return rc;
    const GeomDamping gd = damping_of(c, ex, nullptr, 0.0, true);
    rc = force_pass(c, c->d_vec[FEMCY_VEC_DOF], ex.bulk() ? &gd : nullptr);
    if (rc) return rc;
    ex.energy_on = ex.energy_want;                  // the start zeroes the sums and records the forces of state 0
    const ExplicitEnergy en = energy_of(c, ex);
    return launch_explicit_node(c, ex.d_minv.get(), c->d_vec[rhs_vec], nullptr, scale, 0.0, XN_START, ex.alpha,
                                ex.nmoved ? &mv : nullptr, ex.energy_on ? &en : nullptr, ex.walls.n ? &ex.walls : nullptr);
}

// nsteps steps from a started state: the first drift, then per step the element pass and the node pass (kick, and the drift
// to the next state unless it is the last).  A fixed run (clk null) takes the increment dt and the load scale
// scale0 + k dscale from the caller; an automatic one bounds the element frequencies and ticks its device clock between the
// two passes, and the node pass reads both from the clock.
static int explicit_steps(Ctx* c, const Ctx::Explicit& ex, ExplicitClock* clk, int rhs_vec, int32_t nsteps, double dt,
                          double scale0, double dscale) {
    if (nsteps == 0) return FEMCY_OK;
    double* u = c->d_vec[FEMCY_VEC_DOF];
    const double* me = c->lumped_masses[ex.lumped].d_me.get();
    // damping (femcy_explicit_set_damping): the damped element pass only with bulk viscosity, the damped bound with any
    // coefficient; with none of them set these are the launches of an undamped integrator
    const GeomDamping gd = damping_of(c, ex, clk, dt, false);
    const GeomDamping *gd_geom = ex.bulk() ? &gd : nullptr, *gd_bound = ex.damped() ? &gd : nullptr;
    // motion (femcy_explicit_set_motion): a fixed run hands every launch the times of its own clock (time_of), an automatic
    // one reads the device clock; without it these are the launches of an integrator that never had one
    const bool moved = ex.nmoved != 0;
    auto time_of = [&](int32_t k) { return explicit_fixed_time(ex.t_base, ex.n_base, ex.n_done + k, dt); };
    ExplicitMotion mv = motion_of(ex, 0.0, 0.0);
    // energy balance (femcy_explicit_energy_enable): the energy variant of the node pass, the same number of launches
    const ExplicitEnergy en = energy_of(c, ex);
    int rc = launch_explicit_drift(c, clk, dt);
    if (!rc && moved) rc = launch_explicit_place(c, mv, clk, clk ? 0.0 : time_of(1), MOVE_U);
    for (int32_t k = 1; !rc && k <= nsteps; ++k) {
        if (moved && !clk) mv.t = time_of(k), mv.t_drift = time_of(k + 1);
        // the element pass of force_pass without its per-call copy of u: the lazy state is set once, below
        if ((rc = launch_geom(c, u, GEOM_DSDX | GEOM_FE, gd_geom))) break;
        if (clk) {
            if ((rc = launch_explicit_bound(c, u, me, ex.s_C, ex.d_bpart.get(), gd_bound, ex.wall_kappa()))) break;
            if ((rc = launch_explicit_clock(c, ex.d_bpart.get(), clk))) break;
        }
        rc = launch_explicit_node(c, ex.d_minv.get(), c->d_vec[rhs_vec], clk, scale0 + k * dscale, dt,
                                  k < nsteps ? XN_KICK_DRIFT : XN_KICK, ex.alpha, moved ? &mv : nullptr,
                                  ex.energy_on ? &en : nullptr, ex.walls.n ? &ex.walls : nullptr);
    }
    if (rc) return rc;
    // post-processing reads "the stress of the last force evaluation": that of the last state (the last step did not drift)
    FEMCY_HIP(hipMemcpyAsync(c->d_u_lazy, u, sizeof(double) * c->n, hipMemcpyDeviceToDevice, c->stream));
    c->gp_lazy = true;
    c->post_small = false;
    return FEMCY_OK;
}

int femcy_explicit_advance(femcy_ctx* ctx, int32_t id, int rhs_vec, int32_t nsteps, double dt, double scale0, double dscale) {
    CTX_OR_FAIL(ctx);
    READY_OR_FAIL();
    EXPLICIT_SINGLE_RANK_OR_FAIL("femcy_explicit_advance");
    FEMCY_TRY(check_explicit_advance(c, id, rhs_vec, nsteps, dt, scale0, dscale));
    Ctx::Explicit& ex = c->explicits[id];
    if (nsteps && dt != ex.dt_prev) {               // another increment: the clock counts on from the time it has reached
        ex.t_base = explicit_fixed_time(ex.t_base, ex.n_base, ex.n_done, ex.dt_prev);
        ex.n_base = ex.n_done;
        ex.dt_prev = dt;
    }
    const int rc = explicit_steps(c, ex, nullptr, rhs_vec, nsteps, dt, scale0, dscale);
    if (!rc) ex.n_done += nsteps;
    return rc;
}

int femcy_explicit_kinetic_energy(femcy_ctx* ctx, int32_t id, int v_vec, double* out) {
    CTX_OR_FAIL(ctx);
    EXPLICIT_SINGLE_RANK_OR_FAIL("femcy_explicit_kinetic_energy");
    FEMCY_OBJECT_OR_FAIL(ex, c->explicits, id, "explicit integrator");
    VEC_OR_FAIL(v_vec);
    FEMCY_REQUIRE(out, TEXT_NULL_OUTPUT);
    return launch_explicit_energy(c, c->lumped_masses[ex.lumped].d_m.get(), c->d_vec[v_vec], out);
}

int femcy_explicit_stable_dt(femcy_ctx* ctx, int32_t id, double* dt, double* omega_bound) {
    CTX_OR_FAIL(ctx);
    EXPLICIT_SINGLE_RANK_OR_FAIL("femcy_explicit_stable_dt");
    FEMCY_OBJECT_OR_FAIL(ex, c->explicits, id, "explicit integrator");
    FEMCY_REQUIRE(dt && omega_bound, TEXT_NULL_OUTPUT);
    FEMCY_REQUIRE(c->have_pattern && c->K_serial == c->pattern_serial, TEXT_ASSEMBLE_FIRST);
    double w2 = 0.0;
    int rc = launch_rowabs_bound(c, ex.d_minv.get(), &w2);
    if (rc) return rc;
    *omega_bound = std::sqrt(w2);
    *dt = 2.0 / *omega_bound;
    return FEMCY_OK;
}

// ---- element-by-element increment (*Dynamic, explicit, element by element)
// the buffers an integrator allocates on first use: the partial maxima of the bound kernel, the clock
static int explicit_auto_buffers(Ctx* c, Ctx::Explicit& ex) {
    if (!ex.d_bpart.get() && ex.d_bpart.alloc(sizeof(double) * (size_t)explicit_bound_partials(c)) != hipSuccess) {
        set_error("out of device memory for the element bound of %d elements", c->ne);
        return FEMCY_ENOMEM;
    }
    if (!ex.d_clock.get() && ex.d_clock.alloc(sizeof(ExplicitClock)) != hipSuccess) {
        set_error("out of device memory for the clock of an explicit integrator");
        return FEMCY_ENOMEM;
    }
    return FEMCY_OK;
}

int femcy_explicit_element_bound(femcy_ctx* ctx, int32_t id, int u_vec, double s_C, double* omega) {
    CTX_OR_FAIL(ctx);
    READY_OR_FAIL();
    EXPLICIT_SINGLE_RANK_OR_FAIL("femcy_explicit_element_bound");
    FEMCY_TRY(check_explicit_element_bound(c, id, u_vec, s_C, omega));
    Ctx::Explicit& exm = c->explicits[id];
    int rc = explicit_auto_buffers(c, exm);
    if (rc) return rc;
    const GeomDamping gd = damping_of(c, exm, nullptr, 0.0, true);      // v_{1/2} := vec[VEL]
    rc = launch_explicit_bound(c, c->d_vec[u_vec], c->lumped_masses[exm.lumped].d_me.get(), s_C, exm.d_bpart.get(),
                               exm.damped() ? &gd : nullptr, exm.wall_kappa());
    if (rc) return rc;
    double w2 = 0.0;
    if ((rc = launch_explicit_bound_max(c, exm.d_bpart.get(), &w2))) return rc;
    *omega = std::sqrt(w2);
    return FEMCY_OK;
}

int femcy_explicit_auto_begin(femcy_ctx* ctx, int32_t id, int rhs_vec, double s_C, double scale_factor, double T,
                              int32_t ramp) {
    CTX_OR_FAIL(ctx);
    READY_OR_FAIL();
    EXPLICIT_SINGLE_RANK_OR_FAIL("femcy_explicit_auto_begin");
    FEMCY_TRY(check_explicit_auto_begin(c, id, rhs_vec, s_C, scale_factor, T));
    Ctx::Explicit& exm = c->explicits[id];
    int rc = explicit_auto_buffers(c, exm);
    if (rc) return rc;
    ExplicitClock clk{};
    clk.T = T;
    clk.sf = scale_factor;
    clk.s_C = s_C;
    clk.h_min = INFINITY;
    clk.ramp = ramp ? 1 : 0;
    if ((rc = stage_h2d(c, exm.d_clock.get(), &clk, sizeof(clk)))) return rc;
    const double* u = c->d_vec[FEMCY_VEC_DOF];
    const ExplicitMotion mv = motion_of(exm, 0.0, 0.0);                 // the clock is at t = 0 when the node pass reads it
    if (exm.nmoved && (rc = launch_explicit_place(c, mv, nullptr, 0.0, MOVE_U | MOVE_V | MOVE_A))) return rc;
    const GeomDamping gd = damping_of(c, exm, nullptr, 0.0, true);      // v_{-1/2} := v_0, vec[ACC] is not read
    if ((rc = force_pass(c, u, exm.bulk() ? &gd : nullptr))) return rc;
    if ((rc = launch_explicit_bound(c, u, c->lumped_masses[exm.lumped].d_me.get(), s_C, exm.d_bpart.get(),
                                    exm.damped() ? &gd : nullptr, exm.wall_kappa())))
        return rc;
    if ((rc = launch_explicit_clock(c, exm.d_bpart.get(), exm.d_clock.get()))) return rc;   // t = 0, the first h
    exm.energy_on = exm.energy_want;                                    // as femcy_explicit_start
    const ExplicitEnergy en = energy_of(c, exm);
    if ((rc = launch_explicit_node(c, exm.d_minv.get(), c->d_vec[rhs_vec], exm.d_clock.get(), 0.0, 0.0, XN_START, exm.alpha,
                                   exm.nmoved ? &mv : nullptr, exm.energy_on ? &en : nullptr,
                                   exm.walls.n ? &exm.walls : nullptr)))
        return rc;
    exm.auto_begun = true;
    exm.s_C = s_C;
    return FEMCY_OK;
}

int femcy_explicit_auto_advance(femcy_ctx* ctx, int32_t id, int rhs_vec, int32_t nsteps) {
    CTX_OR_FAIL(ctx);
    READY_OR_FAIL();
    EXPLICIT_SINGLE_RANK_OR_FAIL("femcy_explicit_auto_advance");
    FEMCY_TRY(check_explicit_auto_advance(c, id, rhs_vec, nsteps));
    const Ctx::Explicit& ex = c->explicits[id];
    return explicit_steps(c, ex, ex.d_clock.get(), rhs_vec, nsteps, 0.0, 0.0, 0.0);
}

int femcy_explicit_auto_state(femcy_ctx* ctx, int32_t id, double* t, double* h_last, double* h_min, int64_t* steps_done) {
    CTX_OR_FAIL(ctx);
    EXPLICIT_SINGLE_RANK_OR_FAIL("femcy_explicit_auto_state");
    FEMCY_TRY(check_explicit_auto_state(c, id, t, h_last, h_min, steps_done));
    ExplicitClock clk;
    FEMCY_TRY(download(c, &clk, c->explicits[id].d_clock.get(), sizeof(clk)));
    *t = clk.t;
    *h_last = clk.h_last;
    *h_min = clk.steps ? clk.h_min : 0.0;
    *steps_done = clk.steps;
    return FEMCY_OK;
}

int femcy_spmv(femcy_ctx* ctx, int x_vec, int y_vec) {
    CTX_OR_FAIL(ctx);
    FEMCY_TRY(check_two_vectors(c, x_vec, y_vec, TEXT_SPMV_IN_PLACE));
    // (node-order product.  Round 5 tried the PCG's storage-order kernel between two permutations here: 78.0 -> 75.7 us
    // per call on the C3D10 plate, 281 -> 329 us on the 8 M C3D4 plate, whose numbering gathers as well as storage order
    // does -- not adopted; profiles/r05_bench_c3d4_n1_public_spmv_storage_order.json)
    // round 6: ... except where the internal row order is a coordinate order of the library's choosing AND the vectors are
    // large -- the caller's numbering then gathers badly (C3D10 at k = 12: 868 us per call against 561 for the kernel)
    if (!c->comm && c->node_order_used != 0 && c->n >= 1500000) return spmv_public_storage_order(c, c->d_vec[x_vec], c->d_vec[y_vec]);
    int rc = launch_spmv(c, c->d_vec[x_vec], c->d_vec[y_vec], nullptr, nullptr);
    if (rc) return rc;
    if (c->comm) return iface_sum(c, c->d_vec[y_vec]);
    return FEMCY_OK;
}

int femcy_pcg(femcy_ctx* ctx, int b_vec, int x_vec, double eps, int32_t maxit, int32_t* iters, double* rmax0,
              double* rmax) {
    CTX_OR_FAIL(ctx);
    FEMCY_TRY(check_two_vectors(c, b_vec, x_vec, TEXT_PCG_IN_PLACE));
    // reference: at most n iterations -- n of the whole (un-partitioned) system, so that every rank stops at the same count
    if (maxit <= 0) maxit = (int32_t)std::min<int64_t>(c->comm ? c->n_global : c->n, INT32_MAX);
    return pcg_solve(c, c->d_vec[b_vec], c->d_vec[x_vec], eps, maxit, iters, rmax0, rmax);
}

int femcy_direct_solve(femcy_ctx* ctx, int b_vec, int x_vec, femcy_direct_info* info) {
    CTX_OR_FAIL(ctx);
    FEMCY_TRY(check_two_vectors(c, b_vec, x_vec, TEXT_DIRECT_IN_PLACE));
    return direct_solve(c, c->d_vec[b_vec], c->d_vec[x_vec], info);
}

int femcy_direct_plan(femcy_ctx* ctx, femcy_direct_info* info) {
    CTX_OR_FAIL(ctx);
    FEMCY_TRY(check_direct_plan(c, info));
    return direct_plan(c, info);
}

// ------------------------------------------------------------------------------ post-processing
int femcy_compute_strain_stress(femcy_ctx* ctx, int u_vec, int large) {
    CTX_OR_FAIL(ctx);
    FEMCY_REQUIRE(c->have_mesh && c->have_element && c->have_material, TEXT_NOT_DEFINED);
    VEC_OR_FAIL(u_vec);
    // get_deformation_gradient: F only -- dsdx, vol and (for nlgeom) the Cauchy stress of the last
    // constitutiveOfLargeDeform stay as they are, exactly as in the reference
    int rc = ensure_gp_stress(c);
    if (rc) return rc;
    if ((rc = launch_geom(c, c->d_vec[u_vec], GEOM_F))) return rc;
    c->post_small = false;
    if ((rc = launch_post(c, large ? 1 : 0))) return rc;
    c->post_small = !large;                    // what femcy_thermal_stress may correct, once
    return FEMCY_OK;
}

int femcy_elastic_energy(femcy_ctx* ctx, int u_vec, double* total) {
    CTX_OR_FAIL(ctx);
    FEMCY_REQUIRE(c->have_mesh && c->have_element && c->have_material && total, TEXT_NOT_DEFINED);
    VEC_OR_FAIL(u_vec);
    int rc = ensure_gp_stress(c);
    if (rc) return rc;
    if ((rc = launch_geom(c, c->d_vec[u_vec], GEOM_F))) return rc;
    if ((rc = launch_energy(c))) return rc;
    return launch_energy_sum(c, total);
}

int femcy_elastic_energy_small(femcy_ctx* ctx, int u_vec, double* total) {
    CTX_OR_FAIL(ctx);
    FEMCY_TRY(check_elastic_energy_small(c, u_vec, total));
    int rc = ensure_gp_stress(c);
    if (rc) return rc;
    if ((rc = launch_geom(c, c->d_vec[u_vec], GEOM_F))) return rc;
    if ((rc = launch_energy_small(c))) return rc;
    // the weights det J w of the UNDEFORMED mesh (the F pass left those of the displaced one)
    if ((rc = launch_geom(c, nullptr, GEOM_DSDX))) return rc;
    return launch_energy_sum(c, total);
}

int femcy_extrapolate(femcy_ctx* ctx, int gp_field, int comp, const double* E, double* out) {
    CTX_OR_FAIL(ctx);
    int width = 1;
    FEMCY_TRY(check_extrapolate(c, gp_field, comp, E, out, &width));
    const double* field = nullptr;
    switch (gp_field) {
        case FEMCY_GP_VOL: field = c->d_vol; break;
        case FEMCY_GP_MISES: field = c->d_mises; break;
        case FEMCY_GP_ENERGY: field = c->d_energy; break;
        case FEMCY_GP_F: field = c->d_F; break;
        case FEMCY_GP_SIGMA: field = c->d_sigma; break;
        case FEMCY_GP_STRAIN: field = c->d_strain; break;
        default: return FEMCY_EINVAL;             // not reached: check_extrapolate has refused everything else
    }
    if (gp_field == FEMCY_GP_F || gp_field == FEMCY_GP_SIGMA) {
        int rcl = ensure_gp_stress(c);
        if (rcl) return rcl;
    }
    DevBuf<double> tE, tout;   // freed on every return path, behind the synchronisation below
    const size_t nE = (size_t)c->npe * c->nGP, nout = (size_t)c->ne * c->npe;
    FEMCY_HIP(tE.alloc(nE * sizeof(double)));
    FEMCY_HIP(tout.alloc(nout * sizeof(double)));
    FEMCY_HIP(hipMemcpyAsync(tE, E, nE * sizeof(double), hipMemcpyHostToDevice, c->stream));
    int rc = launch_extrapolate(c, tE, field, width, comp, tout);
    if (!rc) FEMCY_HIP(hipMemcpyAsync(out, tout, nout * sizeof(double), hipMemcpyDeviceToHost, c->stream));
    FEMCY_HIP(hipStreamSynchronize(c->stream));
    return rc;
}

// ---------------------------------------------------------------------------------- inspection
static int download_K(Ctx* c, std::vector<double>& vals) {
    vals.resize((size_t)c->stored_rows * c->dm * c->dm * SLICE);
    FEMCY_HIP(hipStreamSynchronize(c->stream));
    FEMCY_HIP(hipMemcpy(vals.data(), c->d_Kvals, vals.size() * sizeof(double), hipMemcpyDeviceToHost));
    return FEMCY_OK;
}

int femcy_get_K_ell(femcy_ctx* ctx, int32_t* ij, double* A) {
    CTX_OR_FAIL(ctx);
    FEMCY_REQUIRE(c->have_pattern && ij && A, TEXT_GET_K);
    std::vector<double> vals;
    int rc = download_K(c, vals);
    if (rc) return rc;
    const int dm = c->dm, W = c->max_row_blocks * dm;
    for (int32_t a = 0; a < c->nn; ++a) {
        const int64_t off = c->h_slice_off[c->h_pos[a] / SLICE];
        const int lane = c->h_pos[a] % SLICE, L = c->h_rowlen[a];
        for (int r = 0; r < dm; ++r) {
            const int64_t i = (int64_t)a * dm + r;
            int32_t* row_ij = ij + i * (W + 1);
            double* row_A = A + i * W;
            row_ij[0] = L * dm;
            for (int t = 0; t < W; ++t) {
                row_ij[t + 1] = -1;
                row_A[t] = 0.0;
            }
            for (int j = 0; j < L; ++j)
                for (int cc = 0; cc < dm; ++cc) {
                    row_ij[1 + j * dm + cc] = c->h_bcol[(off + j) * SLICE + lane] * dm + cc;
                    row_A[j * dm + cc] = vals[kv_index_rt(dm, off + j, r * dm + cc, lane)];
                }
        }
    }
    return FEMCY_OK;
}

int femcy_get_K_bsr(femcy_ctx* ctx, int32_t* rowptr, int32_t* colidx, double* out) {
    CTX_OR_FAIL(ctx);
    FEMCY_REQUIRE(c->have_pattern && rowptr && colidx && out, TEXT_GET_K);
    std::vector<double> vals;
    int rc = download_K(c, vals);
    if (rc) return rc;
    const int dm = c->dm, bb = dm * dm;
    int64_t w = 0;
    rowptr[0] = 0;
    std::vector<std::pair<int32_t, int32_t>> order;
    for (int32_t a = 0; a < c->nn; ++a) {
        const int64_t off = c->h_slice_off[c->h_pos[a] / SLICE];
        const int lane = c->h_pos[a] % SLICE, L = c->h_rowlen[a];
        order.clear();
        for (int j = 0; j < L; ++j) order.push_back({c->h_bcol[(off + j) * SLICE + lane], j});
        std::sort(order.begin(), order.end());
        for (auto& pr : order) {
            colidx[w] = pr.first;
            for (int k = 0; k < bb; ++k) out[w * bb + k] = vals[kv_index_rt(dm, off + pr.second, k, lane)];
            ++w;
        }
        rowptr[a + 1] = (int32_t)w;
    }
    return FEMCY_OK;
}

int femcy_get_gp_field(femcy_ctx* ctx, int which, double* out) {
    CTX_OR_FAIL(ctx);
    FEMCY_TRY(check_get_gp_field(c, which, out));
    const size_t ngp = (size_t)c->ne * c->nGP;
    const double* src = nullptr;
    size_t count = 0;
    switch (which) {
        case FEMCY_GP_DSDX: src = c->d_dsdx; count = ngp * c->npe * c->dm; break;
        case FEMCY_GP_VOL: src = c->d_vol; count = ngp; break;
        case FEMCY_GP_F: src = c->d_F; count = ngp * c->dm * c->dm; break;
        case FEMCY_GP_SIGMA: src = c->d_sigma; count = ngp * c->dm * c->dm; break;
        case FEMCY_GP_STRAIN: src = c->d_strain; count = ngp * c->dm * c->dm; break;
        case FEMCY_GP_MISES: src = c->d_mises; count = ngp; break;
        case FEMCY_GP_ENERGY: src = c->d_energy; count = ngp; break;
        default: return FEMCY_EINVAL;             // not reached: check_get_gp_field has refused everything else
    }
    if (which == FEMCY_GP_F || which == FEMCY_GP_SIGMA) {
        int rcl = ensure_gp_stress(c);
        if (rcl) return rcl;
    }
    FEMCY_HIP(hipStreamSynchronize(c->stream));
    FEMCY_HIP(hipMemcpy(out, src, count * sizeof(double), hipMemcpyDeviceToHost));
    return FEMCY_OK;
}

int femcy_timing(femcy_ctx* ctx, femcy_timing_t* out) {
    CTX_OR_FAIL(ctx);
    FEMCY_REQUIRE(out, TEXT_NULL_OUTPUT);
    timing_collect(c);
    *out = c->timing;
    return FEMCY_OK;
}
int femcy_timing_reset(femcy_ctx* ctx) {
    CTX_OR_FAIL(ctx);
    timing_collect(c);
    c->timing = femcy_timing_t{};
    return FEMCY_OK;
}

// ------------------------------------------------------------------------------------ ceilings
int femcy_probe_stream(femcy_ctx* ctx, int64_t bytes, int32_t reps, int32_t mode, double* us_per_pass,
                       int64_t* bytes_per_pass) {
    CTX_OR_FAIL(ctx);
    FEMCY_REQUIRE(us_per_pass, "null output");
    return probe_stream(c, bytes, reps, mode, us_per_pass, bytes_per_pass);
}
int femcy_probe_exchange(femcy_ctx* ctx, int32_t rounds, int32_t form, double* us_per_exchange) {
    CTX_OR_FAIL(ctx);
    FEMCY_REQUIRE(us_per_exchange, "null output");
    return probe_exchange(c, rounds, form, us_per_exchange);
}
int femcy_probe_spmv(femcy_ctx* ctx, int32_t reps, int32_t storage_order, double* us_per_launch) {
    CTX_OR_FAIL(ctx);
    return probe_spmv(c, reps, storage_order, us_per_launch);
}
int femcy_probe_mailbox(femcy_ctx* ctx, int32_t rounds, double* us_per_round) {
    CTX_OR_FAIL(ctx);
    FEMCY_REQUIRE(us_per_round, "null output");
    return probe_mailbox(c, rounds, us_per_round);
}
int femcy_persist_streamed_bytes(femcy_ctx* ctx, int64_t* bytes) {
    CTX_OR_FAIL(ctx);
    FEMCY_REQUIRE(bytes, TEXT_NULL_OUTPUT);
    FEMCY_REQUIRE(c->have_pattern, "femcy_build_pattern must come first");
    *bytes = persist_streamed_bytes(c);
    return FEMCY_OK;
}

// ------------------------------------------------------------------------------------ multi-GPU
int femcy_comm_unique_id(void* id128) {
    if (!id128) {
        set_error("null id buffer");
        return FEMCY_EINVAL;
    }
    return comm_unique_id(id128);
}

int femcy_comm_local_id(void* id128) {
    if (!id128) {
        set_error("null id buffer");
        return FEMCY_EINVAL;
    }
    return comm_local_id(id128);
}

int femcy_comm_shm_id(void* id128, int64_t max_values) {
    if (!id128 || max_values < 0) {
        set_error("null id buffer / negative capacity");
        return FEMCY_EINVAL;
    }
    return comm_shm_id(id128, max_values);
}

int femcy_comm_allgather_host(femcy_ctx* ctx, const void* send, int32_t bytes, void* recv) {
    CTX_OR_FAIL(ctx);
    return comm_allgather_host(c, send, bytes, recv);
}

int femcy_comm_init(femcy_ctx* ctx, int32_t rank, int32_t nranks, const void* id128, int32_t niface_local,
                    const int32_t* iface_local_dofs, const int32_t* iface_global_slot, int32_t niface_global,
                    const uint8_t* owner) {
    CTX_OR_FAIL(ctx);
    FEMCY_TRY(check_have_mesh(c));
    FEMCY_REQUIRE(nranks >= 1 && nranks <= 512 && rank >= 0 && rank < nranks && id128, "bad rank/nranks");
    FEMCY_REQUIRE(niface_local >= 0 && niface_global >= niface_local, "bad interface sizes");
    FEMCY_REQUIRE(owner, "owner mask required");
    for (int32_t i = 0; i < niface_local; ++i) {
        FEMCY_REQUIRE(iface_local_dofs[i] >= 0 && iface_local_dofs[i] < c->n, "interface DOF out of range");
        FEMCY_REQUIRE(iface_global_slot[i] >= 0 && iface_global_slot[i] < niface_global, "interface slot out of range");
    }
    int rc = comm_init(c, rank, nranks, id128);
    if (rc) return rc;
    c->niface_local = niface_local;
    c->niface_global = niface_global;
    c->h_iface_dof.assign(iface_local_dofs, iface_local_dofs + niface_local);
    c->split_ready = false;
    if ((rc = dev_alloc(c->d_iface_dof, (size_t)std::max(niface_local, 1), false))) return rc;
    if ((rc = dev_alloc(c->d_iface_slot, (size_t)std::max(niface_local, 1), false))) return rc;
    if ((rc = dev_alloc(c->d_owner, (size_t)c->n + 64))) return rc;
    if ((rc = dev_alloc(c->d_commbuf, (size_t)niface_global + 8))) return rc;
    if ((rc = dev_alloc(c->d_gather, (size_t)nranks * 2 + 2))) return rc;
    {
        std::vector<int32_t> slot2dof((size_t)std::max(niface_global, 1), -1);
        for (int32_t i = 0; i < niface_local; ++i) {
            FEMCY_REQUIRE(slot2dof[iface_global_slot[i]] < 0, "interface slot %d listed twice", iface_global_slot[i]);
            slot2dof[iface_global_slot[i]] = iface_local_dofs[i];
        }
        if ((rc = dev_alloc(c->d_slot2dof, slot2dof.size(), false))) return rc;
        FEMCY_HIP(hipMemcpy(c->d_slot2dof, slot2dof.data(), sizeof(int32_t) * slot2dof.size(), hipMemcpyHostToDevice));
    }
    if (niface_local > 0) {
        FEMCY_HIP(hipMemcpy(c->d_iface_dof, iface_local_dofs, sizeof(int32_t) * niface_local, hipMemcpyHostToDevice));
        FEMCY_HIP(hipMemcpy(c->d_iface_slot, iface_global_slot, sizeof(int32_t) * niface_local, hipMemcpyHostToDevice));
    }
    FEMCY_HIP(hipMemcpy(c->d_owner, owner, (size_t)c->n, hipMemcpyHostToDevice));
    // DOF count of the whole system = owned DOFs summed over the ranks (first collective of the new communicator)
    double owned = 0.0;
    for (int64_t i = 0; i < c->n; ++i) owned += owner[i] ? 1.0 : 0.0;
    FEMCY_HIP(hipMemcpy(c->d_commbuf, &owned, sizeof(double), hipMemcpyHostToDevice));
    if ((rc = comm_allreduce_sum(c, c->d_commbuf, 1))) return rc;
    FEMCY_HIP(hipStreamSynchronize(c->stream));
    FEMCY_HIP(hipMemcpy(&owned, c->d_commbuf, sizeof(double), hipMemcpyDeviceToHost));
    c->n_global = (int64_t)(owned + 0.5);
    return FEMCY_OK;
}

int femcy_comm_info(femcy_ctx* ctx, int32_t* rank, int32_t* nranks, int64_t* n_global) {
    CTX_OR_FAIL(ctx);
    if (rank) *rank = c->comm ? c->rank : 0;
    if (nranks) *nranks = c->comm ? c->nranks : 1;
    if (n_global) *n_global = c->comm ? c->n_global : c->n;
    return FEMCY_OK;
}

int femcy_comm_set_neighbours(femcy_ctx* ctx, int32_t nnb, const int32_t* nb_rank, const int32_t* nb_ptr,
                              const int32_t* nb_dofs) {
    CTX_OR_FAIL(ctx);
    FEMCY_REQUIRE(c->comm, "femcy_comm_init must come first");
    FEMCY_REQUIRE(nnb >= 0 && (nnb == 0 || (nb_rank && nb_ptr && nb_dofs)), "bad neighbour lists");
    const int32_t total = nnb ? nb_ptr[nnb] : 0;
    for (int32_t k = 0; k < nnb; ++k) {
        FEMCY_REQUIRE(nb_rank[k] >= 0 && nb_rank[k] < c->nranks && nb_rank[k] != c->rank, "neighbour %d out of range", nb_rank[k]);
        FEMCY_REQUIRE(k == 0 || nb_rank[k] > nb_rank[k - 1], "neighbours must be listed in ascending rank order");
        FEMCY_REQUIRE(nb_ptr[k + 1] >= nb_ptr[k] && nb_ptr[0] == 0, "neighbour segments must be contiguous");
    }
    // per local interface DOF (in the order of iface_local_dofs): own value + one received value per sharing
    // neighbour, sorted by rank
    std::vector<int32_t> h_dof((size_t)std::max(c->niface_local, 1));
    if (c->niface_local) FEMCY_HIP(hipMemcpy(h_dof.data(), c->d_iface_dof, sizeof(int32_t) * c->niface_local, hipMemcpyDeviceToHost));
    std::vector<int32_t> where((size_t)c->n, -1);
    for (int32_t i = 0; i < c->niface_local; ++i) where[h_dof[i]] = i;
    std::vector<std::vector<std::pair<int32_t, int32_t>>> lists((size_t)c->niface_local);   // (rank, recv index)
    for (int32_t i = 0; i < c->niface_local; ++i) lists[i].push_back({c->rank, -1});
    for (int32_t k = 0; k < nnb; ++k)
        for (int32_t j = nb_ptr[k]; j < nb_ptr[k + 1]; ++j) {
            FEMCY_REQUIRE(nb_dofs[j] >= 0 && nb_dofs[j] < c->n && where[nb_dofs[j]] >= 0,
                          "DOF %d shared with rank %d is not an interface DOF of femcy_comm_init", nb_dofs[j], nb_rank[k]);
            lists[where[nb_dofs[j]]].push_back({nb_rank[k], j});
        }
    std::vector<int32_t> ptr((size_t)c->niface_local + 1, 0), src;
    for (int32_t i = 0; i < c->niface_local; ++i) {
        FEMCY_REQUIRE(lists[i].size() >= 2, "interface DOF %d is shared with no neighbour", h_dof[i]);
        std::sort(lists[i].begin(), lists[i].end());
        for (auto& pr : lists[i]) src.push_back(pr.second);
        ptr[i + 1] = (int32_t)src.size();
    }
    int rc;
    if ((rc = dev_alloc(c->d_nb_dofs, (size_t)std::max(total, 1), false)) ||
        (rc = dev_alloc(c->d_nb_send, (size_t)std::max(total, 1))) ||
        (rc = dev_alloc(c->d_nb_recv, (size_t)std::max(total, 1))) || (rc = dev_alloc(c->d_if_ptr, ptr.size(), false)) ||
        (rc = dev_alloc(c->d_if_src, std::max<size_t>(src.size(), 1), false)))
        return rc;
    if (total) FEMCY_HIP(hipMemcpy(c->d_nb_dofs, nb_dofs, sizeof(int32_t) * total, hipMemcpyHostToDevice));
    FEMCY_HIP(hipMemcpy(c->d_if_ptr, ptr.data(), sizeof(int32_t) * ptr.size(), hipMemcpyHostToDevice));
    if (!src.empty()) FEMCY_HIP(hipMemcpy(c->d_if_src, src.data(), sizeof(int32_t) * src.size(), hipMemcpyHostToDevice));
    c->h_nb_dofs.assign(nb_dofs, nb_dofs + total);
    c->persist_multi = c->persist_multi_local = false;
    c->h_nb_rank.assign(nb_rank, nb_rank + nnb);
    c->h_nb_ptr.assign(nb_ptr, nb_ptr + nnb + (nnb ? 1 : 0));
    if (c->h_nb_ptr.empty()) c->h_nb_ptr.push_back(0);
    return comm_register_neighbours(c);
}

int femcy_comm_mailbox_export(femcy_ctx* ctx, void* blob256) {
    CTX_OR_FAIL(ctx);
    FEMCY_REQUIRE(blob256, "null blob");
    return comm_mailbox_export(c, blob256);
}
int femcy_comm_mailbox_import(femcy_ctx* ctx, int32_t nblobs, const void* blobs) {
    CTX_OR_FAIL(ctx);
    FEMCY_REQUIRE(c->have_pattern, "femcy_build_pattern must come first");
    return comm_mailbox_import(c, nblobs, blobs);
}
int femcy_comm_persist_agree(femcy_ctx* ctx, int32_t* enabled) {
    CTX_OR_FAIL(ctx);
    FEMCY_REQUIRE(c->have_pattern, "femcy_build_pattern must come first");
    return comm_persist_agree(c, enabled);
}

int femcy_comm_tune(femcy_ctx* ctx, int32_t iters, int32_t* chosen, double* us) {
    CTX_OR_FAIL(ctx);
    FEMCY_REQUIRE(c->comm && c->d_if_ptr, "femcy_comm_init and femcy_comm_set_neighbours must come first");
    FEMCY_REQUIRE(iters >= 1 && chosen && us, "bad arguments");
    double* v = c->d_vec[FEMCY_VEC_TMP1];
    double* keep = c->d_vec[FEMCY_VEC_TMP0];
    const int saved = c->exchange;
    int rc;
    // cross-check on a non-trivial vector: v[i] = 1 + (i mod 7) / 8 on both paths
    std::vector<double> h((size_t)c->n), a((size_t)c->n), b((size_t)c->n);
    for (int64_t i = 0; i < c->n; ++i) h[i] = 1.0 + (double)(i % 7) / 8.0;
    FEMCY_HIP(hipMemcpy(keep, h.data(), sizeof(double) * c->n, hipMemcpyHostToDevice));
    bool same = true;
    for (int method = 0; method < 2; ++method) {
        c->exchange = method;
        FEMCY_HIP(hipMemcpyAsync(v, keep, sizeof(double) * c->n, hipMemcpyDeviceToDevice, c->stream));
        if ((rc = iface_sum(c, v))) { c->exchange = saved; return rc; }
        FEMCY_HIP(hipStreamSynchronize(c->stream));
        FEMCY_HIP(hipMemcpy(method ? b.data() : a.data(), v, sizeof(double) * c->n, hipMemcpyDeviceToHost));
    }
    for (int64_t i = 0; i < c->n; ++i) same = same && std::fabs(a[i] - b[i]) <= 1e-12 * std::fabs(a[i]);
    // timing on a zero vector (sums stay zero)
    double t_us[2] = {0.0, 0.0};
    double* slot = c->d_commbuf + c->niface_global;
    for (int method = 0; method < 2; ++method) {
        c->exchange = method;
        if ((rc = vec_fill(c, v, 0.0, c->n))) { c->exchange = saved; return rc; }
        FEMCY_HIP(hipMemsetAsync(slot, 0, sizeof(double), c->stream));
        for (int pass = 0; pass < 2; ++pass) {           // pass 0 warms the connections up
            FEMCY_HIP(hipStreamSynchronize(c->stream));
            const auto t0 = std::chrono::steady_clock::now();
            for (int32_t k = 0; k < (pass ? iters : 3); ++k) {
                if ((rc = iface_sum(c, v))) { c->exchange = saved; return rc; }
                if (method == 1 && (rc = comm_allreduce_sum(c, slot, 1))) { c->exchange = saved; return rc; }
            }
            FEMCY_HIP(hipStreamSynchronize(c->stream));
            if (pass) t_us[method] = std::chrono::duration<double, std::micro>(std::chrono::steady_clock::now() - t0).count() / iters;
        }
    }
    c->exchange = saved;
    // agree: maximum over the ranks of each time, and of the "differs" flag
    double pack[3] = {t_us[0], t_us[1], same ? 0.0 : 1.0};
    std::vector<double> all((size_t)c->nranks * 3);
    FEMCY_HIP(hipMemcpy(c->d_commbuf, pack, sizeof(pack), hipMemcpyHostToDevice));
    DevBuf<double> d_all;
    FEMCY_HIP(d_all.alloc(sizeof(double) * all.size()));
    rc = comm_allgather(c, c->d_commbuf, d_all, 3);
    if (!rc && hipStreamSynchronize(c->stream) != hipSuccess) rc = FEMCY_EHIP;
    if (!rc && hipMemcpy(all.data(), d_all, sizeof(double) * all.size(), hipMemcpyDeviceToHost) != hipSuccess) rc = FEMCY_EHIP;
    if (rc) return rc;
    double m0 = 0.0, m1 = 0.0, bad = 0.0;
    for (int r = 0; r < c->nranks; ++r) {
        m0 = std::max(m0, all[3 * r]);
        m1 = std::max(m1, all[3 * r + 1]);
        bad = std::max(bad, all[3 * r + 2]);
    }
    us[0] = m0;
    us[1] = bad > 0.0 ? -1.0 : m1;
    c->exchange = (bad == 0.0 && m1 < m0) ? 1 : 0;
    *chosen = c->exchange;
    return FEMCY_OK;
}

int femcy_iface_sum(femcy_ctx* ctx, int vec) {
    CTX_OR_FAIL(ctx);
    VEC_OR_FAIL(vec);
    return iface_sum(c, c->d_vec[vec]);
}

}  // extern "C"
