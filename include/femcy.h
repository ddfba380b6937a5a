/*
 * femcy.h -- C ABI of libfemcy_hip.so, the MI355X (gfx950) solve path behind FEMcy's Python surface.
 *
 * The reference (mo-hanxuan/FEMcy) has no FFI: its "operator API" is Python duck typing over Taichi
 * kernels.  Every entry point below names the reference kernel(s)/method(s) it replaces
 * (file:line relative to the reference checkout) -- this is exactly the set a ctypes binding of
 * `System_of_equations` / `ConjugateGradientSolver_rowMajor` needs (INTEGRATION.md shows the stub).
 *
 * Conventions
 *   - every function returns 0 on success, a negative FEMCY_E* code otherwise; the message is
 *     available from femcy_last_error() (thread-local).  The library never aborts or throws.
 *   - host pointers are caller-owned and only borrowed for the duration of the call.
 *   - device memory is library-owned inside the opaque femcy_ctx: one ctx = one HIP device + one
 *     stream.  A ctx is not thread-safe; different ctxs are independent.
 *   - all floating point is f64, all indices i32 (reference: main.py:11 default_fp=ti.f64).
 *   - DOF numbering: i = node*dm + component (stiffnessMtrx.py:179-180).
 *   - solver vectors (the reference's ti.fields rhs/dof/residual/...) live in HBM inside the ctx and
 *     are addressed by the femcy_vec ids below; femcy_vec_upload/_download move them across PCIe.
 */
#ifndef FEMCY_H
#define FEMCY_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

typedef struct femcy_ctx femcy_ctx;

enum femcy_status {
    FEMCY_OK = 0,
    FEMCY_EINVAL = -1,     /* bad argument / call order */
    FEMCY_EHIP = -2,       /* a HIP runtime call failed */
    FEMCY_ENOKERNEL = -3,  /* no kernel instantiation for this (npe, dm, nGP) / material */
    FEMCY_ENUMERIC = -4,   /* NaN/breakdown detected by a solver */
    FEMCY_ECOMM = -5,      /* RCCL failure / a rendezvous of the in-process group that did not complete */
    FEMCY_ENOMEM = -6
};

/* device-resident solver vectors, each of length n = nn*dm (stiffnessMtrx.py:33-34,55-56,95,113;
 * conjugateGradientSolver.py:20-29) */
enum femcy_vec {
    FEMCY_VEC_DOF = 0,       /* System_of_equations.dof                 */
    FEMCY_VEC_RHS = 1,       /* .rhs                                    */
    FEMCY_VEC_RESIDUAL = 2,  /* .residual_nodal_force                   */
    FEMCY_VEC_FORCE = 3,     /* .nodal_force                            */
    FEMCY_VEC_DU = 4,        /* .du                                     */
    FEMCY_VEC_DOF_OLD = 5,   /* .dof_old                                */
    FEMCY_VEC_X = 6,         /* ConjugateGradientSolver_rowMajor.x      */
    FEMCY_VEC_TMP0 = 7,
    FEMCY_VEC_TMP1 = 8,
    FEMCY_VEC_VEL = 9,       /* dynamics: nodal velocities               */
    FEMCY_VEC_ACC = 10,      /* dynamics: nodal accelerations            */
    FEMCY_VEC_COUNT = 11
};

/* Voigt pattern of the strain matrix B (element_zoo: strainMtrx) */
enum femcy_voigt { FEMCY_VOIGT_2D = 0 /* xx,yy,xy */, FEMCY_VOIGT_3D = 1 /* xx,yy,zz,xy,zx,yz */ };

/* material_zoo classes (reader/inp_info.py:294-316) */
enum femcy_material {
    FEMCY_MAT_LIN3D = 0,    /* linear_isotropic.py            params = {E, nu}  */
    FEMCY_MAT_PSTRAIN = 1,  /* linear_isotropic_plane_strain  params = {E, nu}  */
    FEMCY_MAT_PSTRESS = 2,  /* linear_isotropic_plane_stress  params = {E, nu}  */
    FEMCY_MAT_NEOHOOKE = 3  /* neo_hookean.py                 params = {C1, D1}; with dm = 2: plane strain
                               (extension, the reference has the 3-D form only)                          */
};

/* Gauss-point fields that can be downloaded for checking (stiffnessMtrx.py:40-61) */
enum femcy_gpfield {
    FEMCY_GP_DSDX = 0,   /* f64[ne][nGP][npe][dm] */
    FEMCY_GP_VOL = 1,    /* f64[ne][nGP]          */
    FEMCY_GP_F = 2,      /* f64[ne][nGP][dm][dm]  */
    FEMCY_GP_SIGMA = 3,  /* f64[ne][nGP][dm][dm]  */
    FEMCY_GP_STRAIN = 4, /* f64[ne][nGP][dm][dm]  (after femcy_compute_strain_stress) */
    FEMCY_GP_MISES = 5,  /* f64[ne][nGP]          */
    FEMCY_GP_ENERGY = 6  /* f64[ne][nGP] elastic energy density (after femcy_elastic_energy) */
};

/* assembly strategy (femcy_set_option FEMCY_OPT_ASSEMBLY) */
enum femcy_assembly {
    FEMCY_ASM_GATHER = 0, /* owner-computes: one lane per stored block, deterministic            */
    FEMCY_ASM_ATOMIC = 1, /* element scatter with f64 HW atomics (comparison / race check).  The host
                             backend reports this value for its serial element-by-element scatter (no atomics) */
    FEMCY_ASM_ROWS = 2,   /* one wavefront per matrix row, LDS reduction, deterministic           */
    FEMCY_ASM_AUTO = 3,   /* default: ROWS4 for C3D10 (ROWS2 / ROWS if its LDS does not fit), PAIRS for the 2-D quadratic
                             families, C3D8 and C3D6 (if its LDS does not fit: GATHER_SYM_ROWSUM for C3D6, ROWS for the
                             others), GATHER_SYM(_ROWSUM) otherwise */
    FEMCY_ASM_GATHER_SYM = 4, /* GATHER on the diagonal + upper blocks only, mirrored stores of K_ba = K_ab^T: 1.3x on C3D4 */
    FEMCY_ASM_GATHER_SYM_ROWSUM = 5, /* the same with the diagonal block from K_aa = -sum_{b != a} K_ab (partition of
                                unity, checked on the element tables); AUTO picks it for npe <= 4 */
    FEMCY_ASM_ROWS2 = 6,  /* ROWS with the element records staged in LDS, one workgroup per 64-row slice, row-sum
                             diagonal, geometric-sum blocks for cubic-pattern C: AUTO's choice for C3D10 until round 3;
                             instantiated for C3D10 and C3D4 tables whose gradients sum to zero */
    /* 7: retired (ROWS3) */
    FEMCY_ASM_ROWS4 = 8,  /* two rows per wavefront at a time (half a wave each, three incident elements per step, the
                             diagonal block computed like the others): round 3, C3D10; AUTO picks it there */
    FEMCY_ASM_PAIRS = 9   /* round 6: a wavefront owns 8 (or 16) adjacent rows of a slice; lanes = (row, incident element) pair x
                             column node, the element's whole record is read once per pair by coalesced 16-byte loads
                             (the row node's gradients come from the neighbouring lane), the geometric sums are reduced
                             in a wave-private LDS tile and the tile is written as 256-byte runs; any constant C.
                             2-D families, C3D8 and C3D6 (3 x 3 blocks; pair lists in step order, each step padded to
                             a multiple of the pairs per kernel step, so no two lanes of one LDS add hit the same word);
                             AUTO picks it for CPE6 / CPS6 / CPE8 / CPS8, C3D8 and C3D6 */
};

enum femcy_option {
    FEMCY_OPT_ASSEMBLY = 0,     /* enum femcy_assembly, default AUTO                           */
    FEMCY_OPT_PCG_POLL = 1,     /* iterations between host polls of the device "done" flag      */
    FEMCY_OPT_TIMING = 2,       /* 1 = time kernel classes with hipEvents (femcy_timing);       */
                                /* k > 1 = same, but only every k-th SpMV launch is sampled     */
    FEMCY_OPT_SPMV_VARIANT = 3, /* SpMV wavefronts per 64-node slice: 0 auto (by mean row length), 1, 2, 4 */
    FEMCY_OPT_EW_GRID = 4,      /* cap on workgroups of the element-wise PCG kernels (tuning)   */
    FEMCY_OPT_SELL_SIGMA = 6,   /* rows are sorted by length inside windows of this many nodes before slicing
                                   (SELL-C-sigma, default 4096; 64 = natural order); set before build_pattern */
    FEMCY_OPT_PCG_GRAPH = 5,    /* hipGraph replay of poll-bursts of PCG iterations: 0 off, 1 auto (default:
                                   below 2e5 DOF, where the loop is launch-bound), 2 always             */
    FEMCY_OPT_EXCHANGE = 8,     /* multi-rank interface exchange: 0 = all-reduce of the packed global interface vector
                                   (default), 1 = send/recv with the neighbouring ranks (needs
                                   femcy_comm_set_neighbours); femcy_comm_tune measures both and sets it */
    FEMCY_OPT_PCG_STORAGE_ORDER = 13, /* 1 (default): the three-launch PCG of a single rank keeps its vectors in the matrix's
                                   storage order (b permuted once, x permuted back at the end): lanes of a wavefront are
                                   rows of one length class in ascending order, so their gathers of d touch neighbouring
                                   addresses; 0 = node order (what multi-rank runs keep)                          */
    /* 15: retired (PCG_FUSED_UPDATE) */
    /* 16: retired (SPMV_FOOTPRINT) */
    FEMCY_OPT_DIRECT_MAX_BYTES = 17, /* femcy_direct_solve: largest band (bytes) it may allocate (default 48 GiB); a system
                                   whose band after reverse Cuthill-McKee is larger is refused with FEMCY_ENOMEM    */
    FEMCY_OPT_NODE_ORDER = 14,  /* internal row order of the matrix, set before femcy_build_pattern; vectors handed
                                   to / from the caller always keep the caller's numbering.  0 = rows sorted by length
                                   inside windows of the caller's numbering; 1 (default) = inside windows of the best of the
                                   lexicographic coordinate orders (one per axis permutation) if its measured gather cost
                                   (cache lines per wavefront gather, femcy_get_node_order) beats the caller's numbering
                                   by 10 % -- otherwise the caller's numbering; 2 + k = coordinate order k forced (tests).
                                   Measured: persistent PCG on C3D10 plates of 37 k / 72 k elements 31.8 -> 28.8 / 40.7 ->
                                   34.9 us per iteration; neutral for the three-launch PCG and the assemblies; the 1 M / 8 M
                                   C3D4 plates keep their numbering (profiles/r04_persist_node_order_c3d10.txt)      */
    FEMCY_OPT_PCG_PERSIST = 11, /* 1 (default): single-rank systems that fit one wavefront task per SIMD (3 x 3 blocks: up
                                   to ~7.8e5 DOF on MI355X; 2 x 2 blocks: up to ~1.05e6) and fill the chip 1.5 times over
                                   are solved by one persistent launch -- vectors and part of the matrix in registers,
                                   another part in LDS, the rest streamed (from the Infinity Cache or, since round 5, from
                                   HBM: FEMCY_TUNE_PERSIST_MAX_MB), grid-wide exchanges at the three synchronisation points
                                   of the recurrence; 2 = any system whose slices fit (tests); 0 = three launches per
                                   iteration */
    FEMCY_OPT_PCG_PERSIST_MULTI = 12, /* 1 (default): with a communicator attached, femcy_pcg keeps the one-launch
                                   persistent kernel on every rank and the ranks' kernels exchange the interface rows of
                                   Ad and the two scalar reductions through mailboxes in each other's HBM (written over
                                   xGMI by the peers' kernels) -- once the mailboxes are exchanged
                                   (femcy_comm_mailbox_export / _import) and EVERY rank agreed
                                   (femcy_comm_persist_agree).  0 = three launches + RCCL calls per iteration */
    FEMCY_OPT_PCG_SMALL = 10,   /* 1 (default): systems whose two work vectors fit the LDS of a workgroup (~1e4 DOF on
                                   MI355X) are solved by ONE persistent launch with one grid barrier per iteration
                                   instead of three launches per iteration; 0 = always the three-kernel loop */
    FEMCY_OPT_OVERLAP = 9,      /* multi-rank PCG with the neighbour exchange: 1 (default) = the slices that hold interface
                                   nodes are multiplied first and their exchange runs on a second stream while the
                                   interior slices are multiplied; 0 = everything on one stream */
    FEMCY_OPT_TANGENT = 7,      /* what femcy_assemble_K assembles.  0 (default) = the reference's matrix: B^T C B
                                   on the current configuration with the constant C (stiffnessMtrx.py:124-186).
                                   1 = the consistent tangent of femcy_internal_force: spatial elasticity tensor of
                                   the material at F (the updates the reference left commented out,
                                   neo_hookean.py:62-64, 79-81) + geometric stiffness (grad N_a . sigma . grad N_b) I.
                                   An EXTENSION outside the parity runs: Newton iterates differ from the
                                   reference's (they converge quadratically).  Isotropic 3-D, plane-strain and
                                   neo-Hookean materials; not available for plane stress.
                                   What it leaves behind: with 1, femcy_assemble_K(u) evaluates the material at vec[u], so
                                   afterwards FEMCY_GP_F and FEMCY_GP_SIGMA hold F and the Cauchy stress of the ASSEMBLED
                                   state (u_vec = -1: I and 0) and an earlier force evaluation's F / sigma, pending or
                                   read, are gone; with 0 the assembly leaves them those of the last force evaluation.
                                   vec[f] of that evaluation is not touched either way, and the next
                                   femcy_internal_force / femcy_residual_and_K makes F and sigma its own again,
                                   whatever the option was in between: every call reads the option as it is then.
                                   femcy_thermal_stress does not correct the stress such an assembly left. */

    /* ---- tuning and test knobs.  Not needed by a caller of the path; the tests and the tools under tools/ use them
     * to force code paths and to measure alternatives.  None of them changes results beyond summation order. */
    FEMCY_TUNE_TIMING_FENCE = 100,   /* 1 (default): an empty kernel precedes every SpMV dispatch that is timed with
                                        dispatch-attached events, so that the start stamp is not taken while the
                                        previous kernel drains                                                     */
    FEMCY_TUNE_SPMV_WG_PER_XCD = 101,/* SpMV workgroups per XCD; longer slice ranges are looped inside the kernel.  0 (default)
                                        = 512 where an XCD's range holds more than 512 tasks of a matrix beyond 512 MiB, else
                                        256 (round 6: 5 workgroups per CU are resident, the rest is handed out as CUs become
                                        free; 3 GB C3D10 product 597 -> 560 us, profiles/r06_spmv_rounds.txt); 1 forces the
                                        loop on small meshes (tests)                                               */
    FEMCY_TUNE_SPMV_NT = 102,        /* SpMV matrix stream non-temporal: -1 auto (stored matrix > 256 MiB), 0, 1    */
    FEMCY_TUNE_VEC_NT = 103,         /* PCG vector kernels non-temporal: -1 auto (vector > 12 MB), 0, 1             */
    FEMCY_TUNE_PERSIST_LDS_ROWS = 104,/* persistent PCG: block rows per wave kept in LDS (-1 = as many as fit)      */
    FEMCY_TUNE_PERSIST_REG_ROWS = 105,/* persistent PCG: block rows per slice kept in registers (0, 4 or 5)         */
    FEMCY_TUNE_PERSIST_PROBE = 106,  /* persistent PCG: 16 = no prefetch during the barriers.  Bits 0-3 (skip the
                                        streamed / LDS / register rows, skip the barrier wait: timing experiments
                                        that produce meaningless numbers) are accepted only by a library built with
                                        -DFEMCY_PERSIST_PROBE; the shipped library has no work-skipping path       */
    FEMCY_TUNE_PERSIST_WGS = 107,    /* persistent PCG: workgroups of the launch (0 = one per CU).  More than the
                                        occupancy query admits is refused before the launch; see femcy_pcg          */
    FEMCY_TUNE_SMALL_REG_ROWS = 108, /* small-system PCG: block rows per wave kept in registers (-1 = its share)    */
    FEMCY_TUNE_PERSIST_VARIANT = 109,/* persistent PCG variant bits (-1 = the default chosen by measurement, DESIGN.md
                                        section 3): 1 = non-temporal matrix stream (FEMCY_TUNE_PERSIST_L2_ROWS), 2 = the
                                        three grid-wide exchanges as tagged granules (one hop) instead of counters +
                                        data, 4 = d published in storage order (16 + 8 byte gathers instead of 3 x 8).
                                        The shipped library holds the default and 0 (round 2); all eight with
                                        -DFEMCY_PERSIST_ALL_VARIANTS */
    FEMCY_TUNE_SPMV_KEEP = 110,      /* NT SpMV: per-mille of every XCD's slice range that keeps the default cache
                                        policy (-1 auto = 235 MB of the matrix)                                     */
    FEMCY_TUNE_SKIP_OCCUPANCY_CHECK = 111,/* 1 = launch the persistent kernels without the co-residency check (tests
                                        of the barrier time-out and its fallback)                                   */
    FEMCY_TUNE_PERSIST_L2_ROWS = 113,/* persistent PCG with non-temporal matrix stream (variant bit 1): streamed block rows
                                        per slice that keep the default cache policy (they stay in the XCD's L2)     */
    FEMCY_TUNE_DIRECT_UPDATE = 115,  /* femcy_direct_solve, trailing tile update: -1 auto (default), 0 = VALU product, 1 = f64
                                        matrix cores (v_mfma_f64_16x16x4_f64), one tile pair per workgroup, 2 = matrix
                                        cores, 2 x 2 tile pairs per workgroup, 3 = 1 on two streams: the tiles the next panel
                                        needs first, the rest beside that panel (tests, comparison records)          */
    /* 116: retired (ROWS4_TILE) */
    /* 118: retired (ROWS4_ORDER) */
    FEMCY_TUNE_SPMV_ROT = 119,       /* SpMV task lists of the workgroups of an XCD.  0 = task b + i * (workgroups per XCD) in round i
                                        (rounds 1-5: always the same position of the length-sorted window); 1 .. 63 = the
                                        position advances by this many tasks per round; 64 = lists balanced by the host, round
                                        by round (the workgroup with the most work so far takes the shortest task of the
                                        round); -1 (default) = 64 where the rows of a window differ in length by more than a
                                        quarter and an XCD's range holds more than 512 tasks of a matrix beyond 512 MiB (C3D10
                                        at k >= 8: 3 GB product 596 -> 529 us together with knob 101), 0 elsewhere.  Changes the grouping of the d.Ad partial sums only
                                        (profiles/r06_spmv_rounds.txt) */
    FEMCY_TUNE_PAIRS = 117,          /* FEMCY_ASM_PAIRS: -1 = default (163), else bit 0 = workgroups take XCD-contiguous ranges of
                                        the processing order, bits 1-2 = rows per wavefront (0: 16, 1: 8), bits 3-4 = steps of
                                        element records in flight - 2 (0..2), bit 5 = chunks processed in Morton order of their
                                        centroids, bits 6-9 = chunks per wavefront - 1; the same bits of K whatever the value
                                        (profiles/r06_asm_cpe8_knobs.txt) */
    FEMCY_TUNE_PERSIST_MAX_MB = 114, /* persistent PCG: largest STREAMED part of the matrix (MiB) it takes; 0 = no limit
                                        (default since round 5: 61 against 78 us per iteration on the 124 k C3D10 plate
                                        whose 287 MB stream comes from HBM); rounds 2-4 used 240 (tests, comparison
                                        records)                                                                     */
    FEMCY_TUNE_BARRIER_SPIN_LIMIT = 112 /* polls (each ~0.3-1 us) before a grid barrier of the one-launch solvers gives
                                        up, poisons the exchange and the solve is redone by the three-kernel loop
                                        (default 2^20, about half a second; 0 provokes the fallback: tests)         */
};

typedef struct femcy_pattern_info {
    int64_t n;           /* scalar DOFs                                                */
    int64_t nnzb;        /* structural dm x dm blocks (node adjacency incl. diagonal)   */
    int64_t nnz;         /* nnzb*dm*dm                                                  */
    int32_t max_row_blocks;   /* max neighbours per node (reference: maxLen, stiffnessMtrx.py:80) */
    int32_t ell_width;        /* reference W = max_row_blocks*dm                          */
    int64_t stored_blocks;    /* blocks stored incl. SELL padding                         */
    int32_t nslices;
    int32_t max_node_elems;   /* reference nodeEles width (stiffnessMtrx.py:71)           */
} femcy_pattern_info;

typedef struct femcy_timing_t {
    /* accumulated since the last femcy_timing_reset; *_ms from hipEvents on the ctx stream */
    double geom_ms;      int64_t geom_launches;      /* get_dsdx_and_vol / F / sigma kernels; also the element and vector passes
                                                        of the body-load, thermal, mass and Newmark calls */
    double assemble_ms;  int64_t assemble_launches;  /* K assembly kernel                     */
    double force_ms;     int64_t force_launches;     /* nodal-force gather                    */
    double spmv_ms;      int64_t spmv_launches;      /* compute_Ad                            */
    double pcg_ms;       int64_t pcg_iters;          /* whole PCG solves (all kernels)        */
    double persist_ms;   int64_t persist_launches;   /* one-launch PCG (k_pcg_persist) alone  */
    int64_t persist_iters;                           /* CG iterations inside those launches   */
    int64_t solves_three, solves_small, solves_persist; /* PCG solves by path (always counted) */
    int64_t barrier_timeouts;                        /* one-launch solves abandoned at a grid barrier and redone by
                                                        the three-kernel loop (always counted)              */
} femcy_timing_t;

/* ------------------------------------------------------------------ life cycle / diagnostics */
int femcy_ctx_create(int device, femcy_ctx** out);
int femcy_ctx_destroy(femcy_ctx* ctx);
const char* femcy_last_error(void);
int femcy_version(void);
int femcy_set_option(femcy_ctx* ctx, int option, int64_t value);
int femcy_sync(femcy_ctx* ctx);                                   /* hipStreamSynchronize */

/* ----------------------------------------------------------------------- problem definition */
/* Body + System_of_equations.__init__ state (body.py:13-17, stiffnessMtrx.py:26-121).  Calling it again on a used
 * ctx starts over: element tables, material, pattern, DOF lists, load sets, body loads, mass objects, lumped masses,
 * explicit integrators and thermal loads of the old mesh are dropped. */
int femcy_set_mesh(femcy_ctx* ctx, int32_t nn, int32_t dm, const double* nodes /*[nn*dm]*/,
                   int32_t ne, int32_t npe, const int32_t* elems /*[ne*npe]*/);
/* table-driven element plugin: ELE.gaussPoints/gaussWeights/dshape_dnat (element_zoo modules) */
int femcy_set_element(femcy_ctx* ctx, int32_t nGP, const double* dN /*[nGP*npe*dm]*/,
                      const double* w /*[nGP]*/, int32_t voigt_kind);
/* material.C copied to every Gauss point by ddsdde_init (stiffnessMtrx.py:124-129) + sigma(F) kind */
int femcy_set_material(femcy_ctx* ctx, int32_t kind, const double* C /*[s*s]*/, const double* params,
                       int32_t nparams);
/* body.get_nodeEles/get_coElement_nodes + sparseIJ (body.py:165-194, stiffnessMtrx.py:70-89):
 * node adjacency -> blocked sliced-ELL matrix, element->slot map, node->element lists */
int femcy_build_pattern(femcy_ctx* ctx);
int femcy_get_pattern_info(femcy_ctx* ctx, femcy_pattern_info* out);
/* the femcy_assembly mode the last femcy_assemble_K / femcy_residual_and_K ran, after AUTO and the LDS fall-backs
 * resolved (the consistent tangent reports GATHER_SYM_ROWSUM / GATHER_SYM, the gather form it runs).  The host backend
 * has one assembly, a serial element-by-element scatter, and reports FEMCY_ASM_ATOMIC.  FEMCY_EINVAL before the first
 * assembly of the context, and after an assembly that was refused or failed. */
int femcy_get_assembly_used(femcy_ctx* ctx, int32_t* mode);
/* which row order femcy_build_pattern took (FEMCY_OPT_NODE_ORDER): used = 0 the caller's numbering, 1 + k = coordinate
 * order k; lines[0] = mean 128-byte cache lines per wavefront gather with the caller's numbering, lines[1 + k] = with
 * coordinate order k (0 where not evaluated) */
int femcy_get_node_order(femcy_ctx* ctx, int32_t* used /* nullable */, double* lines /*[7], nullable*/);

/* ------------------------------------------------------------------------- vector plumbing */
int femcy_vec_upload(femcy_ctx* ctx, int vec, const double* src, int64_t n);
int femcy_vec_download(femcy_ctx* ctx, int vec, double* dst, int64_t n);
int femcy_vec_fill(femcy_ctx* ctx, int vec, double value);                 /* field.fill()          */
int femcy_vec_copy(femcy_ctx* ctx, int dst, int src);                      /* field.copy_from()     */
int femcy_vec_scatter(femcy_ctx* ctx, int vec, const int32_t* idx, const double* vals, int32_t k);
                                                      /* dirichletBC_val, stiffnessMtrx.py:357-366 */
int femcy_vec_sub(femcy_ctx* ctx, int c, int a, int b);                    /* tiGadgets.py:5-9      */
int femcy_vec_axpy(femcy_ctx* ctx, int a, int b, double c, int d);         /* a = b + c*d, :12-16   */
int femcy_vec_scale(femcy_ctx* ctx, int vec, double s);                    /* tiGadgets.py:67-70    */
int femcy_vec_norm(femcy_ctx* ctx, int vec, double* rms);                  /* tiGadgets.py:28-37    */
int femcy_vec_absmax(femcy_ctx* ctx, int vec, double* out);                /* tiGadgets.py:19-25    */

/* --------------------------------------------------------------------------- the hot path */
/* get_dsdx_and_vol + assemble_stiffnessMtrx (stiffnessMtrx.py:132-150, 161-186) at x = X + vec[u];
 * u_vec = -1: the undeformed configuration (u = 0) */
int femcy_assemble_K(femcy_ctx* ctx, int u_vec);
/* assemble_nodal_force_GN (stiffnessMtrx.py:609-644): F (ref. config), sigma(F), dsdx/vol (current
 * config), node-parallel gather of dsdx . sigma * vol */
int femcy_internal_force(femcy_ctx* ctx, int u_vec, int f_vec);
/* One Newton residual evaluation: assemble_nodal_force_GN followed by get_dsdx_and_vol + assemble_stiffnessMtrx on
 * the same displacement (the pair the reference issues back to back at stiffnessMtrx.py:756-759, 779-783 and in
 * inside_relaxation) as ONE element pass: vec[f] = internal force, K = matrix at x = X + vec[u].  Same results as
 * femcy_internal_force + femcy_assemble_K; the second geometry pass and the F / sigma stores are gone (F and sigma
 * "of the last force evaluation" are recomputed when post-processing asks for them). */
int femcy_residual_and_K(femcy_ctx* ctx, int u_vec, int f_vec);
/* dirichletBC_linearEquations (stiffnessMtrx.py:279-307) for one *Boundary block, race-free */
int femcy_apply_dirichlet_linear(femcy_ctx* ctx, const int32_t* dofs, const double* vals, int32_t k, int rhs_vec);
/* dirichletBC_forNewtonMethod_kernel (stiffnessMtrx.py:317-341) */
int femcy_apply_dirichlet_newton(femcy_ctx* ctx, const int32_t* dofs, int32_t k, int residual_vec);
/* Device-resident copy of one *Boundary block's DOF list (node_set*dm + dof).  The reference keeps each node
 * set in a ti.field for the whole run (stiffnessMtrx.py:656-659); the femcy_dofset_* calls are the
 * femcy_apply_dirichlet_* / femcy_vec_scatter calls without the per-call upload and stream sync. */
int femcy_dofset_create(femcy_ctx* ctx, const int32_t* dofs, int32_t k, int32_t* id_out);
int femcy_dofset_dirichlet_newton(femcy_ctx* ctx, int32_t id, int residual_vec);
int femcy_dofset_dirichlet_linear(femcy_ctx* ctx, int32_t id, double value, int rhs_vec);
int femcy_dofset_fill(femcy_ctx* ctx, int32_t id, int vec, double value);       /* dirichletBC_val */
int femcy_dofset_scatter(femcy_ctx* ctx, int32_t id, int vec, const double* vals /*[k]*/);
/* *Cload: vec[dof] += value over the set (the entries of a set are distinct DOFs).  Several ranks: no exchange -- the
 * right-hand side holds the summed value on every rank that shares a node, so each rank adds the full value to its copy. */
int femcy_dofset_add(femcy_ctx* ctx, int32_t id, int vec, double value);
/* neumannBC (stiffnessMtrx.py:369-411) on the device.  A load set is the device-resident description of one
 * *Dsload surface: for each loaded facet its owning element (body.boundary[facet], body.py:197-216) and its
 * facet type = index into the element plugin's facet tables (facet_natural_coos / facet_point_weights /
 * facet_natural_normals keys, e.g. element_linear_tetrahedral.py:30-55), which are passed as plain arrays:
 *   ft_nodes [nft][nfn]            sorted local node ids of the facet (the dict key)
 *   ft_N     [nft][nip][npe]       shapeFunc at the facet integration points
 *   ft_dN    [nft][nip][npe][dm]   dshape_dnat there
 *   ft_normal[nft][nip][dm]        natural outward normals
 *   ft_weight[nft][nip]            facet point weights
 * femcy_loadset_neumann zero-fills vec[rhs] (reference :384) and writes the consistent nodal loads of
 * traction * (direction, or the outward unit normal n_nat (dx/dxi)^-1 / (|.| + 1e-30) when direction is NULL)
 * on the undeformed geometry; the facet size is |x1 - x0| (dm = 2) or the triangle area of the facet's first
 * three sorted nodes (dm = 3), as ELE.globalNormal computes it.  A 3-D facet of four nodes (a hexahedron face, a
 * wedge's quadrilateral face) instead weights each facet point by its surface Jacobian (Nanson):
 * da = |det J| |J^-T n_nat| w.  Sums per node run in a fixed order.
 * A load set has one facet arity (nfn, nip).  The C3D6 wedge has faces of both kinds -- S1 / S2 are triangles (nfn 3,
 * three points of weight 1/3), S3 / S4 / S5 quadrilaterals (nfn 4, 2 x 2 Gauss points) -- so a wedge surface is two load
 * sets: femcy_loadset_neumann on the triangle set, then femcy_loadset_neumann_add on the quadrilateral set.
 * femcy_loadset_neumann_add is femcy_loadset_neumann without the zero-fill: it adds the set's node sums to vec[rhs]
 * (several ranks: it sums its own loads over the interface in vector TMP1, which must then not be vec[rhs]). */
int femcy_loadset_create(femcy_ctx* ctx, int32_t nft, int32_t nfn, int32_t nip, const int32_t* ft_nodes,
                         const double* ft_N, const double* ft_dN, const double* ft_normal, const double* ft_weight,
                         int32_t nload, const int32_t* load_elem, const int32_t* load_ft, int32_t* id_out);
int femcy_loadset_neumann(femcy_ctx* ctx, int32_t id, double traction, const double* direction /*[dm] or NULL*/,
                          int rhs_vec);
int femcy_loadset_neumann_add(femcy_ctx* ctx, int32_t id, double traction, const double* direction /*[dm] or NULL*/,
                              int rhs_vec);
/* Body forces (*Dload GRAV / BX / BY / BZ; an extension, the reference has surface tractions only).  A body load is to a
 * volume force what a load set is to a *Dsload surface: a device-resident description built once.
 * femcy_bodyload_create computes, on the UNDEFORMED geometry, the nodal weights
 *   m_a = sum over the selected elements e and their Gauss points g of N_a(xi_g) |det J_g| w_g
 * with N [nGP][npe] = the plugin's shapeFunc at its Gauss points (dN and w are those of femcy_set_element); sel_elems =
 * NULL selects every element, otherwise nsel distinct element ids.  After femcy_set_element and femcy_build_pattern.
 * The consistent load vector of a uniform force b per unit volume is then exactly f[a*dm + i] = m_a * b[i]: a dead load on
 * the reference volume, which is also the gravity load under nlgeom (mass is conserved), so nothing is re-evaluated per
 * Newton step.  Element pass + owner-computes node sums in a fixed order: the same bits on every run.
 * femcy_bodyload_weights downloads m [nn].
 * femcy_bodyload_apply writes (add = 0) or adds (add != 0) m_a * b[i] to vec[rhs]; b [dm] is read during the call and
 * travels in the kernel arguments (no copy, no stream synchronisation).  The product is rounded before it is added.
 * Several ranks: each rank weighs its own elements; apply sums over the interface like femcy_loadset_neumann, and with
 * add through vector TMP1, which must then not be vec[rhs] (collective calls). */
int femcy_bodyload_create(femcy_ctx* ctx, const double* N /*[nGP][npe]*/, int32_t nsel,
                          const int32_t* sel_elems /*[nsel], NULL = every element*/, int32_t* id_out);
int femcy_bodyload_weights(femcy_ctx* ctx, int32_t id, double* out /*[nn]*/);
int femcy_bodyload_apply(femcy_ctx* ctx, int32_t id, const double* b /*[dm]*/, int rhs_vec, int32_t add);
/* Thermal loads (*Expansion + *Temperature; an extension, small strain only).  With nodal temperature changes dT_a the
 * temperature change at a Gauss point is dT_g = sum_a N_a(xi_g) dT_a (the element's own shape functions, mid-side nodes
 * included), the thermal strain is isotropic, eps_th = alpha dT_g I, and the stress of full restraint is
 * sigma_th = C : eps_th with C as femcy_set_material received it:
 *   FEMCY_MAT_LIN3D    eps_th = alpha dT (1,1,1,0,0,0)
 *   FEMCY_MAT_PSTRESS  eps_th = alpha dT (1,1,0) against the plane-stress C
 *   FEMCY_MAT_PSTRAIN  eps_zz = 0 is enforced: (1 + nu) alpha dT (1,1,0) against the plane-strain C, nu = params[1]
 *   FEMCY_MAT_NEOHOOKE refused
 * femcy_thermal_create evaluates, once, on the UNDEFORMED geometry, the consistent load at scale 1
 *   f[a*dm + i] = sum over elements e and Gauss points g of sum_j dN_a/dx_j sigma_th[i][j] |det J_g| w_g
 * with N [nGP][npe] = the plugin's shapeFunc at its Gauss points and dT [nn] (both are copied).  After
 * femcy_set_element, femcy_set_material (the material of this moment is the one the load keeps) and femcy_build_pattern.
 * Element pass + owner-computes node sums in a fixed order: the same bits on every run.  The load is linear in dT, so an
 * increment only scales it.  femcy_thermal_force downloads f [n] (several ranks: the sum over the rank's own elements).
 * femcy_thermal_apply writes (add = 0) or adds (add != 0) scale * f to vec[rhs]; scale travels in the kernel arguments (no
 * copy, no stream synchronisation), the product is rounded before it is added.  Several ranks: apply sums over the
 * interface like femcy_bodyload_apply, and with add through vector TMP1, which must then not be vec[rhs] (collective).
 * femcy_thermal_stress corrects the result of femcy_compute_strain_stress(large = 0), once per such call:
 * FEMCY_GP_SIGMA -= scale * sigma_th(dT_g) and FEMCY_GP_MISES is formed again by material kind (plane strain:
 * sigma_zz = nu (sigma_xx + sigma_yy) - E alpha dT_g scale).  FEMCY_GP_STRAIN stays the total strain.
 * Refused with FEMCY_EINVAL, the context stays usable: an unknown id, a neo-Hookean material, a null N or dT, a
 * non-finite alpha, femcy_thermal_stress without a preceding femcy_compute_strain_stress(large = 0).
 * Thermal loads are dropped where body loads are: femcy_set_mesh and femcy_ctx_destroy. */
int femcy_thermal_create(femcy_ctx* ctx, const double* N /*[nGP][npe]*/, double alpha, const double* dT /*[nn]*/,
                         int32_t* id_out);
int femcy_thermal_force(femcy_ctx* ctx, int32_t id, double* out /*[n]*/);
int femcy_thermal_apply(femcy_ctx* ctx, int32_t id, double scale, int rhs_vec, int32_t add);
int femcy_thermal_stress(femcy_ctx* ctx, int32_t id, double scale);
/* Implicit dynamics (*Dynamic; an extension, small strain, single rank).  A mass object is the CONSISTENT mass matrix of
 * the mesh in the matrix's own storage: one scalar per stored block,
 *   m_ab = sum over elements e and mass-rule points q of N_a(xi_q) N_b(xi_q) rho |det J_q| w_q,
 * in bcol's [block row][lane] layout (8 B where K has 8 dm^2; padding blocks hold 0); the matrix itself is M (x) I_dm.
 * femcy_mass_create works on the UNDEFORMED mesh with a rule of its own (the stiffness rule under-integrates N_a N_b):
 * Nq [nq][npe], dNq [nq][npe][dm], wq [nq] are the plugin's shape functions, natural derivatives and weights at the points
 * of its mass_rule() (nq <= 64), rho > 0 the density.  An element pass evaluates rho |det J_q| w_q (it does not read the
 * Gauss-point volumes of the stiffness rule), an owner-computes pass sums every stored block's contributions in ascending
 * (element, local node) order: no atomics, the same bits on every run, and m_ab == m_ba bit for bit.
 * After femcy_set_element and femcy_build_pattern.
 * femcy_mass_get downloads the nnzb scalars in the block order of femcy_get_K_bsr (rows ascending, columns ascending).
 * femcy_mass_apply: vec[y] = [vec[y] +] scale * (M (x) I) vec[x] (add != 0 adds); the launch shape and slice ranges are the
 * stiffness product's, scale travels in the kernel arguments; x and y must differ.
 * femcy_mass_add_to_K adds c * m_ab to the dm diagonal entries of every stored block of K (products rounded before they are
 * added); overwrite != 0 sets K := c * M (x) I instead (the initial-acceleration solve).  K is the matrix of the last
 * femcy_assemble_K, so the call belongs between the assembly and the Dirichlet treatment.
 * femcy_mass_kinetic_energy: *out = 1/2 v^T (M (x) I) v, reduced in a fixed order.
 * femcy_newmark_predict: vec[out] = c0 vec[u] + c1 vec[v] + c2 vec[a] in one pass; out may not be one of the three inputs
 * (FEMCY_EINVAL), the inputs may coincide with each other.
 * femcy_newmark_update: with u_new the solution at t + dt, in one pass and in place of vec[a] and vec[v],
 *   a_new = (u_new - u) / (beta dt^2) - v / (beta dt) - (1 / (2 beta) - 1) a,   v_new = v + dt ((1 - gamma) a + gamma a_new).
 * Refused with FEMCY_EINVAL, the context stays usable: an unknown id, a null table or output, nq outside 1 .. 64, a
 * non-finite or non-positive rho, beta <= 0, dt <= 0, a call before the pattern exists, and every mass call once
 * femcy_comm_init has run (several ranks are not supported; the host backend has one rank, its femcy_comm_init never
 * succeeds, so it has no such check).  Mass objects are dropped where body loads are:
 * femcy_set_mesh and femcy_ctx_destroy. */
int femcy_mass_create(femcy_ctx* ctx, int32_t nq, const double* Nq /*[nq][npe]*/, const double* dNq /*[nq][npe][dm]*/,
                      const double* wq /*[nq]*/, double rho, int32_t* id_out);
int femcy_mass_get(femcy_ctx* ctx, int32_t id, double* vals /*[nnzb], in femcy_get_K_bsr's block order*/);
int femcy_mass_apply(femcy_ctx* ctx, int32_t id, int x_vec, int y_vec, double scale, int32_t add);
int femcy_mass_add_to_K(femcy_ctx* ctx, int32_t id, double c, int32_t overwrite);
int femcy_mass_kinetic_energy(femcy_ctx* ctx, int32_t id, int v_vec, double* out);
int femcy_newmark_predict(femcy_ctx* ctx, int u_vec, int v_vec, int a_vec, int out_vec, double c0, double c1, double c2);
int femcy_newmark_update(femcy_ctx* ctx, int u_new_vec, int u_vec, int v_vec, int a_vec, double beta, double gamma,
                         double dt);
/* Explicit dynamics (*Dynamic, explicit; an extension, large deformation, single rank).  Central differences with a diagonal
 * mass, written as velocity Verlet so that u, v and a all belong to whole steps: with minv the inverse lumped mass per scalar
 * DOF (0 on constrained DOFs, which therefore keep u = v = a = 0), f the load vector at scale 1 and s_n the load scale,
 *   a_0     = minv o (s_0 f - f_int(u_0))
 *   u_{n+1} = u_n + h v_n + (h^2 / 2) a_n
 *   a_{n+1} = minv o (s_{n+1} f - f_int(u_{n+1}))
 *   v_{n+1} = v_n + (h / 2)(a_n + a_{n+1})
 * with f_int what femcy_internal_force computes (F, sigma(F), gradients of the current configuration, all four stress laws):
 * an explicit step is geometrically non-linear whatever the deck's nlgeom says.  No matrix, no solve.
 * femcy_lumped_mass_create: the nodal masses of the UNDEFORMED mesh by HRZ lumping over the plug-in's mass_rule() (the tables
 * femcy_mass_create takes, nq <= 64).  Per element, with vq = rho |det J_q| w_q:
 *   m_e = sum_q vq,   d_a = sum_q N_a(xi_q)^2 vq,   m_a^e = d_a m_e / sum_b d_b,
 * strictly positive for every family (row sums are negative at the corners of C3D10 / CPS6 / CPS8), m_e / npe on CPS3 /
 * C3D4.  Element pass + owner-computes node sums in ascending (element, local node) order: no atomics, the same bits on
 * every run.  After femcy_set_element and femcy_build_pattern.  femcy_lumped_mass_get downloads m [nn].
 * femcy_explicit_create: an integrator = minv [n] from a lumped mass, 0 on every DOF of the given DOF sets
 * (femcy_dofset_create ids).
 * The stepping calls work on vec[DOF] = u, vec[VEL] = v, vec[ACC] = a; vec[rhs] = f is only read and may be none of them.
 * femcy_explicit_start: vec[ACC] = a_0 from vec[DOF], at load scale `scale`.
 * femcy_explicit_advance: nsteps steps of size dt, the k-th new state (k = 1 .. nsteps) at load scale scale0 + k dscale.  A
 * step is two launches -- the element pass of femcy_internal_force and one node pass that sums the element forces, forms
 * a_new and v_new and moves u on to the next state, the node sums never reaching memory; the first move of a call is a vector
 * pass of its own and the last step of a call leaves u alone, so that u, v, a leave the call at the same time.  All launches
 * are enqueued without a host synchronisation and the scalars travel in the kernel arguments.  A run split into several
 * calls gives the bits of one call (provided the caller's scales agree bit for bit).  nsteps = 0 does nothing.  Afterwards
 * post-processing sees the last state as after femcy_internal_force.
 * femcy_explicit_kinetic_energy: *out = 1/2 sum_a m_a |v_a|^2, reduced in a fixed order.
 * femcy_explicit_stable_dt: Gershgorin's bound on the largest eigenvalue of M_L^-1 K for the K of the last femcy_assemble_K,
 *   omega_bound^2 = max over the unconstrained scalar rows i of minv_i sum_j |K_ij|   (one pass over the SELL storage + a
 * maximum reduction), and *dt = 2 / omega_bound, the stability limit of central differences for a linear system with that
 * spectrum.
 * Refused with FEMCY_EINVAL, the context stays usable: an unknown id, the refusals of femcy_mass_create, nsteps < 0, dt <= 0
 * or not finite, a scale that is not finite, rhs_vec one of DOF / VEL / ACC, femcy_explicit_stable_dt before an assembly on
 * the current pattern, and every one of these calls once femcy_comm_init has run (several ranks are not supported; the host
 * backend has one rank, its femcy_comm_init never succeeds, so it has no such check).  Lumped masses and integrators are
 * dropped where mass objects are: femcy_set_mesh and femcy_ctx_destroy. */
int femcy_lumped_mass_create(femcy_ctx* ctx, int32_t nq, const double* Nq /*[nq][npe]*/, const double* dNq /*[nq][npe][dm]*/,
                             const double* wq /*[nq]*/, double rho, int32_t* id_out);
int femcy_lumped_mass_get(femcy_ctx* ctx, int32_t id, double* out /*[nn]*/);
int femcy_explicit_create(femcy_ctx* ctx, int32_t lumped_id, int32_t ndofsets, const int32_t* dofset_ids /*[ndofsets]*/,
                          int32_t* id_out);
int femcy_explicit_start(femcy_ctx* ctx, int32_t id, int rhs_vec, double scale);
int femcy_explicit_advance(femcy_ctx* ctx, int32_t id, int rhs_vec, int32_t nsteps, double dt, double scale0, double dscale);
int femcy_explicit_kinetic_energy(femcy_ctx* ctx, int32_t id, int v_vec, double* out);
int femcy_explicit_stable_dt(femcy_ctx* ctx, int32_t id, double* dt, double* omega_bound);
/* The element-by-element increment (*Dynamic, explicit, element by element): the highest frequency is estimated from the
 * CURRENT configuration x = X + u in every step, element by element, and the increment and the clock stay on the device, so
 * that a batch of steps needs no host synchronisation and no matrix is ever assembled.  With m_a^e the element's own HRZ
 * share of the lumped mass, v_q = |det J_x(xi_q)| w_q at the stiffness rule's Gauss points, sigma_q the Cauchy stress of the
 * internal force at F_q and s_C = max eps:C:eps / eps:eps of the material's small-strain matrix (3 lambda + 2 mu in 3-D,
 * 2 lambda + 2 mu in plane strain, E / (1 - nu) in plane stress; neo-Hookean: the same with mu = 2 C1, kappa = 2 / D1),
 *   omega_e^2 = sum_q v_q (s_C + |sigma_q|_F) sum_a |grad_x N_a(xi_q)|^2 / m_a^e,   omega = sqrt(max_e omega_e^2),
 *   dt_stable = 2 / omega.
 * At u = 0 with a linear material omega >= the largest eigenfrequency of M_L^-1 K, by Cauchy-Schwarz on every element and
 * because M and K are sums over the elements; the |sigma|_F term bounds the geometric stiffness in the same way.  At finite
 * strain the material part is an ESTIMATE, not a proof -- the spatial tangent is not C -- and scale_factor is the margin.
 * femcy_explicit_element_bound: *omega at vec[u_vec], stand-alone (synchronises, like femcy_explicit_stable_dt).
 * femcy_explicit_auto_begin: t = 0 on the device, vec[ACC] = a_0 from vec[DOF] at load scale 1 (ramp = 0) or 0 (ramp = 1:
 * the scale is t / T throughout), and the first increment h_0 = min(scale_factor 2 / omega(u_0), T).
 * femcy_explicit_auto_advance: nsteps steps, enqueued without a host synchronisation.  A step is the element pass at the
 * new state, the element bound + one tick of the clock (h_{n+1} = min(scale_factor 2 / omega, T - t), exactly 0 once t >= T
 * or when omega is not finite; the step that takes the remainder sets t = T itself), and the node pass, which kicks with h_n
 * and drifts with h_{n+1}.  A step with h = 0 writes nothing: a batch that overshoots T ends in no-ops, bit for bit.  A run
 * split into several calls gives the bits of one call.
 * femcy_explicit_auto_state: the one synchronising read-back: the clock t, the last and the smallest non-zero increment
 * taken (0 before the first) and the number of real steps.
 * Refused with FEMCY_EINVAL as above; also s_C, scale_factor or T not finite and positive, and _advance / _state before
 * _begin. */
int femcy_explicit_element_bound(femcy_ctx* ctx, int32_t id, int u_vec, double s_C, double* omega);
int femcy_explicit_auto_begin(femcy_ctx* ctx, int32_t id, int rhs_vec, double s_C, double scale_factor, double T,
                              int32_t ramp);
int femcy_explicit_auto_advance(femcy_ctx* ctx, int32_t id, int rhs_vec, int32_t nsteps);
int femcy_explicit_auto_state(femcy_ctx* ctx, int32_t id, double* t, double* h_last, double* h_min, int64_t* steps_done);
/* Damping of an explicit integrator (*Bulk Viscosity: b1, b2; *Damping, alpha=): from the next stepping call on, and it may
 * be called between calls.  Both forces are evaluated at u_{n+1} with the LAGGED half-step velocity of the drift by h that
 * led there,
 *   v_{n+1/2} = fma(h / 2, a_n, v_n)                            (v_{-1/2} := v_0 at _start / _auto_begin: vec[ACC] is not read)
 *   a_{n+1}   = minv (s f - f_int(u_{n+1}) - f_bv(u_{n+1}, v_{n+1/2})) - alpha v_{n+1/2},   v_{n+1} = v_n + h/2 (a_n + a_{n+1}).
 * Bulk viscosity, at every Gauss point q of the stiffness rule on the current configuration (plane stress: in the plane):
 *   rate_q = sum_a v_{a,n+1/2} . grad_x N_a,   L_q = (max_a |grad_x N_a|^2)^(-1/2),   rho_q = rho_0 / det F_q,
 *   p_q    = b1 sqrt(rho_q M_d) L_q rate_q + rho_q (b2 L_q)^2 |rate_q| min(0, rate_q),
 *   fe[a] += grad_x N_a p_q vol_q,
 * with rho_0 the density of the lumped mass and M_d = rho c_d^2 the dilatational modulus.  The stored and recovered stress
 * never contains p_q.  The element-by-element estimate becomes omega_eff,e = omega_e (sqrt(1 + xi_e^2) + xi_e) with
 *   xi_e = alpha / (2 omega_e) + b1 + b2^2 max_q [L_q sqrt(rho_q / M_d) max(0, -rate_q)]
 * (femcy_explicit_element_bound stand-alone and _auto_begin take v_{1/2} := vec[VEL]); femcy_explicit_stable_dt is unchanged.
 * All four zero: the undamped launches and bits.  Refused with FEMCY_EINVAL, the context stays usable: an unknown id, a
 * value that is not finite or negative, M_d <= 0 while b1 or b2 is not zero, and once femcy_comm_init has run. */
int femcy_explicit_set_damping(femcy_ctx* ctx, int32_t id, double alpha, double b1, double b2, double M_d);
/* Prescribed motion (*Boundary, amplitude=NAME with *Amplitude): held DOFs that follow a curve in time instead of staying at
 * rest.  femcy_amplitude_create: one curve A(t) in step time from npts points (2 .. FEMCY_AMP_MAX_POINTS), t strictly
 * increasing.  Between two points, with xi = (t - t_k) / (t_{k+1} - t_k),
 *   FEMCY_AMP_TABULAR      A = A_k + (A_{k+1} - A_k) xi,  A' the slope of [t_k, t_{k+1}) (the right-hand one at a point), A'' = 0
 *   FEMCY_AMP_SMOOTH_STEP  A = A_k + (A_{k+1} - A_k) xi^3 (10 - 15 xi + 6 xi^2), A' and A'' from the same polynomial: both 0
 *                          at every point
 * and outside the table both are clamped: (A_0, 0, 0) for t <= t_0, (A_last, 0, 0) exactly for t >= t_last.
 * femcy_explicit_set_motion: every DOF of DOF set dofset_ids[k] moves as
 *   u = values[k] A_k(t),   v = values[k] A_k'(t),   a = values[k] A_k''(t),      A_k the curve amplitude_ids[k],
 * whatever force it gathers.  Every set must be one of the sets the integrator was created with (minv = 0 there), at most 4
 * distinct curves per integrator; where a DOF is in two sets, the later one wins.  Held sets that are not named stay at rest.
 * It takes effect from the next femcy_explicit_start / _auto_begin: both first place u, v and a of the moved DOFs at t = 0,
 * so that f_int(u_0) and the first increment estimate see the placed boundary.  In a step the node pass writes a and v of a
 * moved DOF at the time of the state being kicked and, where it drifts, u at the time the drift reaches; the first drift of a
 * call is followed by one small launch over the moved DOFs that does the same to u.  The step stays two launches.  The bulk
 * viscosity reads these v and a like any other, v_{n+1/2} = values[k] (A' + (h / 2) A''); a moved DOF takes no alpha force.
 * femcy_explicit_kinetic_energy counts the moved nodes with their mass; neither increment estimate changes.
 * Time: an automatic run reads its device clock.  A fixed run keeps a clock of its own: femcy_explicit_start sets it to 0,
 * step n is at t_base + (n - n_base) dt, and (t_base, n_base) is reset only when a call's dt differs from the previous
 * call's -- so a run split into several femcy_explicit_advance calls of the same dt still gives the bits of one call.
 * nsets = 0 removes the motion: the integrator is then launched exactly as without this call, the same bits.
 * Amplitudes are dropped where integrators are.  Refused with FEMCY_EINVAL, the context stays usable: an unknown id (curve,
 * integrator, DOF set), an unknown kind, npts outside 2 .. 16, t not strictly increasing, an entry or a value that is not
 * finite, null arguments, a set that is not one of the integrator's held sets, more than 4 distinct curves, and either call
 * once femcy_comm_init has run. */
#define FEMCY_AMP_MAX_POINTS 16
#define FEMCY_MOTION_MAX_CURVES 4
enum femcy_amplitude_kind { FEMCY_AMP_TABULAR = 0, FEMCY_AMP_SMOOTH_STEP = 1 };
int femcy_amplitude_create(femcy_ctx* ctx, int32_t kind, int32_t npts, const double* t /*[npts]*/, const double* A /*[npts]*/,
                           int32_t* id_out);
int femcy_explicit_set_motion(femcy_ctx* ctx, int32_t id, int32_t nsets, const int32_t* dofset_ids /*[nsets]*/,
                              const double* values /*[nsets]*/, const int32_t* amplitude_ids /*[nsets]*/);
/* Energy balance of an explicit run (*Energy Output): four work integrals, accumulated inside the node pass of every step
 * and kept on the device (the steps run in batches with no host synchronisation and leave only the last state).  State k has
 * the load scale s_k; du_k = u_{k+1} - u_k is h_k v_{k+1/2} on a free DOF (v_{k+1/2} = fma(h_k / 2, a_k, v_k), h_k the
 * increment of the drift the step applied), the curve's own difference values[.] (A(t_{k+1}) - A(t_k)) on a moved DOF and 0
 * on a held one.  The work of a force g is the trapezoid sum W_g = sum_k 1/2 du_k . (g_k + g_{k+1}) over the scalar DOFs:
 *   FEMCY_EN_LOAD      g_k = s_k f                              free and moved DOFs
 *   FEMCY_EN_INTERNAL  g_k = the node sum of fe at state k      the stress force plus the bulk-viscosity force, as the node
 *                                                               pass gathers it
 *   FEMCY_EN_ALPHA     g_k = alpha m v_{k-1/2}                  free DOFs: the force the damped kick subtracts, v_{-1/2} := v_0
 *   FEMCY_EN_BOUNDARY  g_k = R_k = m a_k + f_int,k - s_k f      moved DOFs only: what the support applies, the inertia of the
 *                                                               moved node included; m from the lumped mass
 * For a fixed increment h the update gives, on the free DOFs and in exact arithmetic,
 *   [KE - (h^2 / 8) a.M a]_N - [KE - (h^2 / 8) a.M a]_0 = W_LOAD - W_INTERNAL - W_ALPHA.
 * femcy_explicit_energy_enable: on != 0 takes effect from the next femcy_explicit_start / _auto_begin, which zero the four
 * sums and record the forces of state 0; every kick then adds the step that led to its state and records the forces of that
 * state (two vectors [n], allocated here), so a run split into several calls gives the bits of one call.  No launch is
 * added, no atomics: every wavefront of the node pass owns one slot and adds its partial sum in a fixed order; a step of an
 * automatic run that does nothing adds and writes nothing.  u, v and a are bit for bit those of a run without it.  on = 0:
 * the launches of an integrator that never had it, from the next stepping call.
 * femcy_explicit_energy_get: the one synchronising read-back, out[FEMCY_EN_*], the slots summed in a fixed order.
 * Refused with FEMCY_EINVAL, the context stays usable: an unknown id, a null output, _get while the balance is off or before
 * a start, and either call once femcy_comm_init has run. */
enum femcy_energy_term { FEMCY_EN_LOAD = 0, FEMCY_EN_INTERNAL = 1, FEMCY_EN_ALPHA = 2, FEMCY_EN_BOUNDARY = 3 };
int femcy_explicit_energy_enable(femcy_ctx* ctx, int32_t id, int32_t on);
int femcy_explicit_energy_get(femcy_ctx* ctx, int32_t id, double* out /*[4]*/);
/* Frictionless planar rigid walls (*Rigid Wall: an extension keyword in the spirit of LS-DYNA's planar rigid wall; Abaqus
 * needs an analytical rigid surface, a reference node, a contact pair and a surface interaction for the same thing).  Wall w
 * is a point p, a normal n into the free half space and a penalty kappa_w in 1/s^2; n is normalised and d = n . p formed
 * once on the host, by code both backends share.  At most FEMCY_WALL_MAX walls per integrator.  For node a at
 * x = X_a + u_a (one rounding per component) the gap is formed in exactly this order,
 *   g = fma(n[dm-1], x[dm-1], ... fma(n[0], x[0], -d)),
 * and the wall adds to the acceleration of every FREE scalar DOF i of the node (minv != 0)
 *   a_i += -kappa_w min(g, 0) n_i,          evaluated as  g < 0: a_i = fma(-kappa_w g, n_i, a_i)
 * -- the force -kappa_w m_a min(g, 0) n divided by the node's mass -- walls in ascending index order, after
 * minv (s f - f_int) and before the alpha term.  A wall that a node has not reached adds nothing at all, bit for bit.  Held
 * DOFs take no wall force and stay at rest; moved DOFs ignore it as they ignore every other force, but their u enters g.
 * The wall acts at femcy_explicit_start / _auto_begin as well: a_0 of a mesh that starts inside a wall contains it.  The
 * step stays two launches: the node pass reads X and u of its DOF and the lanes of a node exchange x inside their quad.
 * The wall is conservative, with the potential
 *   E_w = 1/2 kappa_w sum_a m_a min(g_a, 0)^2       (the lumped mass, scaled if it was scaled; nodes with a free DOF only),
 * so the energy balance needs no new accumulator: the wall force enters the kick but none of the four sums,
 * FEMCY_EN_INTERNAL keeps meaning the gathered fe, and the fixed-increment identity above becomes
 *   [KE + sum_w E_w - (h^2 / 8) a.M a]_N - [...]_0 = W_LOAD - W_INTERNAL - W_ALPHA      (all DOFs of contacting nodes free),
 * with E_w read from the state by femcy_explicit_wall_get.
 * Stable increment: write kappa = sum_w kappa_w.  On a contacting node wall w adds kappa_w m_a n n^T to the stiffness; in
 * the M-inner product that is kappa_w n n^T, positive semi-definite with largest eigenvalue kappa_w, so by Weyl's inequality
 * omega_c^2 <= omega^2 + kappa.  The element-by-element estimate (femcy_explicit_element_bound and the clock of an automatic
 * run) adds kappa to every element's omega_e^2 BEFORE the damping factor -- any element may touch a wall --; a caller of
 * femcy_explicit_stable_dt, which is unchanged, uses omega_c = sqrt(omega_bound^2 + kappa).
 * femcy_explicit_set_wall is meant to be called before femcy_explicit_start / _auto_begin, which put the wall force into
 * a_0.  The walls are kept in the integrator and travel in the kernel arguments, so a call between two stepping calls is
 * taken at once: the next kick and the next increment estimate see the new walls, while a of the current state still
 * holds the old ones.  nwalls = 0 removes the walls: the node pass is then launched exactly as without this call, the same
 * kernels with the same arguments, and the bound kernel -- which since the walls always takes the sum of the penalties as
 * one more argument -- gets 0 and adds nothing: the same bits.
 * femcy_explicit_wall_get: a synchronising read-back from vec[DOF], one pass over the nodes and a fixed-order reduction, no
 * atomics: out[0] = sum_a kappa_w m_a max(-g_a, 0), the normal force on the wall; out[1] = E_w; out[2] = the number of nodes
 * with g < 0; out[3] = max_a max(-g_a, 0).  out[0] and out[1] count the nodes with at least one free DOF.
 * Refused with FEMCY_EINVAL, the context stays usable: an unknown id, nwalls outside 0 .. FEMCY_WALL_MAX, null arguments, an
 * entry that is not finite, a normal of length 0, kappa <= 0, a wall index out of range or _get with no walls set, and
 * either call once femcy_comm_init has run.  Walls are dropped where integrators are. */
#define FEMCY_WALL_MAX 4
int femcy_explicit_set_wall(femcy_ctx* ctx, int32_t id, int32_t nwalls, const double* point /*[nwalls][dm]*/,
                            const double* normal /*[nwalls][dm]*/, const double* kappa /*[nwalls]*/);
int femcy_explicit_wall_get(femcy_ctx* ctx, int32_t id, int32_t wall, double* out /*[4]*/);
/* Fixed mass scaling (*Fixed Mass Scaling, whole model): the element shares m_a^e of a lumped mass are multiplied by one
 * factor k_e per element, before an integrator is made from it, and the nodal masses are summed again.  omega_e^2 above is
 * linear in 1 / m_a^e, so k_e divides it exactly and a target increment is met in closed form, in the project's own
 * estimate.  With omega_e^2 the UNDAMPED estimate at u = 0 from the element's current shares and s_C, dt_e = 2 / omega_e:
 *   factor = f alone                      k_e = f
 *   dt = tau, FEMCY_MS_BELOW_MIN          k_e = max(1, omega_e^2 tau^2 / 4)        only elements with dt_e < tau grow
 *   dt = tau, FEMCY_MS_SET_EQUAL_DT       k_e = omega_e^2 tau^2 / 4                every dt_e becomes tau; k_e < 1 lightens
 *   dt = tau, FEMCY_MS_UNIFORM            k_e = max_e omega_e^2 tau^2 / 4          one factor, the smallest dt_e becomes tau
 *   factor and dt                         factor first: omega_e^2 / f enters the dt rule, k_e is the product
 * (0 stands for "not given"; type is ignored without dt).  A second call compounds.  Afterwards femcy_lumped_mass_get
 * returns the scaled nodal masses, both increment estimates and the kinetic energy see them, and no stepping kernel changes.
 * *mass_before / *mass_after: the sum of the nodal masses in a fixed order, *n_scaled: elements with k_e != 1, *factor_max:
 * max_e k_e of this call.  femcy_lumped_mass_get_scaling: the cumulative k_e [ne], 1.0 before any call.
 * DEVIATION from Abaqus: rho_0 of the bulk viscosity stays the density the lumped mass was created with (Abaqus uses the
 * scaled density).  The lagged estimate xi_e = b1 + ... then overstates the damping fraction of a scaled element: the safe
 * side.  Body forces are the caller's and are not scaled either, as in Abaqus.
 * FEMCY_ENUMERIC, the lumped mass untouched: an omega_e^2 or a factor that is NaN, infinite or (the factor) not positive (a
 * broken element).  Refused with FEMCY_EINVAL, the context stays usable: an unknown id, null outputs, factor and dt both 0,
 * either negative or not finite, an unknown type, dt with s_C not finite and positive, a lumped mass that an integrator
 * already refers to (scale before femcy_explicit_create: minv is derived once), and once femcy_comm_init has run. */
enum femcy_mass_scaling { FEMCY_MS_BELOW_MIN = 0, FEMCY_MS_SET_EQUAL_DT = 1, FEMCY_MS_UNIFORM = 2 };
int femcy_lumped_mass_scale(femcy_ctx* ctx, int32_t lumped_id, double s_C, double factor /*0: none*/, double dt /*0: none*/,
                            int32_t type /*femcy_mass_scaling*/, double* mass_before, double* mass_after, int64_t* n_scaled,
                            double* factor_max);
int femcy_lumped_mass_get_scaling(femcy_ctx* ctx, int32_t lumped_id, double* out /*[ne]*/);
/* compute_Ad (conjugateGradientSolver.py:53-58): vec[y] = K vec[x] */
int femcy_spmv(femcy_ctx* ctx, int x_vec, int y_vec);
/* ConjugateGradientSolver_rowMajor.re_init + solve (conjugateGradientSolver.py:32-51, 103-127):
 * Jacobi-PCG, x0 = 0, stop when max|r| < eps*max|r0|, at most maxit iterations (reference: n). */
int femcy_pcg(femcy_ctx* ctx, int b_vec, int x_vec, double eps, int32_t maxit, int32_t* iters,
              double* rmax0, double* rmax);
/* solve_by_scipy (stiffnessMtrx.py:219-251: `spsolve` on the scipy matrix built from sparseIJ / sparseMtrx_rowMajor,
 * the branch solve_dof takes below 1e5 DOF): vec[x] = K^-1 vec[b] by a direct factorisation on the device.
 * The nodes are renumbered by reverse Cuthill-McKee (once per pattern), K is copied into lower band storage (tiles of
 * 32 x 32, one column panel after the other) and factored K = L S L^T, S = diag(+-1), without pivoting: Cholesky for
 * the positive definite K of a sound configuration (after the Dirichlet treatment, :279-341), and still a
 * factorisation when a diverging Newton iterate has made K indefinite (the reference's LU returns a solution there
 * too, and the increment driver's path depends on it).  Two triangular solves follow; then the residual b - K x is
 * formed with K itself and the solution refined (at most twice) while that pays.  vec[b] is left untouched.
 * FEMCY_ENUMERIC when a pivot is zero / not a number (info->singular_at) or the residual stays above 1e-8 max|b|
 * (elimination without pivoting lost the indefinite matrix): the caller treats it like a solver breakdown.
 * FEMCY_ENOMEM when the band does not fit the limit (FEMCY_OPT_DIRECT_MAX_BYTES).  FEMCY_ECOMM with a communicator
 * attached (the factorisation is single-rank; a partitioned run of a small system keeps the tight PCG of femcy_pcg). */
typedef struct femcy_direct_info {
    int64_t n;               /* scalar unknowns */
    int64_t band_bytes;      /* storage of the band */
    int32_t bandwidth;       /* sub-diagonals kept, in DOF */
    int32_t panels;          /* column panels of 32 DOF (0 on the host backend) */
    int32_t singular_at;     /* 0, or 1 + the row (band order) whose pivot was zero / not a number */
    int32_t negative_pivots; /* 0 = K was positive definite */
    int32_t refinements;     /* refinement steps taken (0 .. 2) */
    int32_t reserved;
    double residual;         /* max|b - K x| / max|b| of the returned x */
} femcy_direct_info;
int femcy_direct_solve(femcy_ctx* ctx, int b_vec, int x_vec, femcy_direct_info* info /* nullable */);
/* What femcy_direct_solve WOULD factor for the current pattern, without factoring: n, bandwidth (after reverse
 * Cuthill-McKee), panels and band_bytes are filled, everything else is zero.  The reference's switch between its two
 * solvers is a fixed DOF count (`solve_dof`, stiffnessMtrx.py:272-276); the host driver here also looks at the band --
 * n * bandwidth^2 flops against iterations * (matrix bytes / bandwidth of the memory) -- before it takes the direct
 * branch (femcy_amd/stiffnessMtrx.py, direct = "auto").  Never FEMCY_ENOMEM: a band beyond the limit is reported, not
 * refused. */
int femcy_direct_plan(femcy_ctx* ctx, femcy_direct_info* info);

/* ------------------------------------------------------------------------ post-processing */
/* compute_strain_stress (stiffnessMtrx.py:436-501): F at vec[u]; strain (infinitesimal, or Green when
 * large != 0); Cauchy stress by constitutiveOfSmallDeform when large == 0 (kept from the last
 * femcy_internal_force otherwise, as in the reference); von Mises stress by material type */
int femcy_compute_strain_stress(femcy_ctx* ctx, int u_vec, int large);
/* get_elasEng (stiffnessMtrx.py:592-606): F at vec[u], elasticEnergyDensity, sum(density * vol) with the
 * vol left by the last geometry pass (reference behaviour) */
int femcy_elastic_energy(femcy_ctx* ctx, int u_vec, double* total);
/* The strain energy of a LINEAR (small-strain) analysis: sum over the Gauss points of sigma : eps / 2 with the infinitesimal
 * strain eps = sym(F) - I at vec[u], sigma = constitutiveOfSmallDeform(eps), times det J w of the UNDEFORMED mesh, i.e.
 * u^T K u / 2 with the K of femcy_assemble_K(ctx, -1) up to rounding.  This is the energy the Newmark integrator conserves;
 * femcy_elastic_energy is the reference's energy of the Green strain and differs from it by the order of the strain.  The
 * call leaves the gradients and weights of the undeformed mesh behind (what femcy_assemble_K(ctx, -1) leaves) and the
 * density in FEMCY_GP_ENERGY.  A neo-Hookean material is refused with FEMCY_EINVAL. */
int femcy_elastic_energy_small(femcy_ctx* ctx, int u_vec, double* total);
/* ELE.extrapolate (element_zoo): out[e][a] = sum_g E[a][g] * field[e][g][comp]; E is npe x nGP */
int femcy_extrapolate(femcy_ctx* ctx, int gp_field, int comp, const double* E, double* out /*[ne*npe]*/);

/* --------------------------------------------------------------------- inspection (tests) */
/* the reference's sparseIJ / sparseMtrx_rowMajor layouts (stiffnessMtrx.py:78-94) */
int femcy_get_K_ell(femcy_ctx* ctx, int32_t* ij /*[n*(W+1)]*/, double* A /*[n*W]*/);
/* block-CSR with ascending columns: rowptr[nn+1], colidx[nnzb], vals[nnzb*dm*dm] */
int femcy_get_K_bsr(femcy_ctx* ctx, int32_t* rowptr, int32_t* colidx, double* vals);
int femcy_get_gp_field(femcy_ctx* ctx, int which, double* out);
int femcy_timing(femcy_ctx* ctx, femcy_timing_t* out);
int femcy_timing_reset(femcy_ctx* ctx);

/* ----------------------------------------------------- ceilings of the device (bench.py's roofline) */
/* What the one-launch PCG runs against, measured with the kernel's own launch shape and exchange code:
 * femcy_probe_stream: a read-only sweep of `bytes` (>= 1 MiB), `reps` passes inside one launch after a warm-up
 *   launch, 16-byte loads, XCD-contiguous ranges.  mode 0 = one workgroup of four waves per CU (the persistent
 *   kernel's shape), 1 = the same with non-temporal loads, 2 = eight workgroups per CU, 3 = mode 2 non-temporal.
 *   A buffer below ~200 MB is served by the Infinity Cache from the second pass on, a larger one by HBM.
 *   us_per_pass = microseconds per pass, bytes_per_pass = the bytes one pass reads (whole tiles only).
 * femcy_probe_exchange: one grid-wide exchange of an 8-byte value per workgroup (publish, synchronise, every
 *   workgroup sums all of them), averaged over `rounds` inside one launch.  form 0 = per-XCD counters + top counter
 *   + data (FEMCY_TUNE_PERSIST_VARIANT without bit 1), 1 = tagged 16-byte granules (bit 1).  The sums are checked.
 * femcy_persist_streamed_bytes: bytes of the matrix the persistent PCG streams per iteration on this context (stored
 *   block rows less the register- and LDS-resident ones), 0 when the system does not fit that kernel. */
int femcy_probe_stream(femcy_ctx* ctx, int64_t bytes, int32_t reps, int32_t mode, double* us_per_pass,
                       int64_t* bytes_per_pass /* nullable */);
int femcy_probe_exchange(femcy_ctx* ctx, int32_t rounds, int32_t form, double* us_per_exchange);
/* femcy_probe_spmv: `reps` launches of compute_Ad back to back between ONE pair of HIP events on the context's stream, on
 *   the PCG's own vectors, in the caller's node order (storage_order = 0) or in storage order (1, what the three-launch
 *   PCG of a single rank runs): microseconds from launch to launch = kernel + the boundary between dependent launches. */
int femcy_probe_spmv(femcy_ctx* ctx, int32_t reps, int32_t storage_order, double* us_per_launch);
/* femcy_probe_mailbox (collective, after femcy_comm_mailbox_import): one cross-rank reduction of the persistent
 *   multi-rank PCG -- a wave per rank writes its value into every rank's mailbox and polls its own, the solver's own
 *   code -- averaged over `rounds` inside one launch per rank: the mailbox round trip between the ranks' kernels, link
 *   (xGMI) latency included.  The sums are checked; FEMCY_ECOMM on a time-out. */
int femcy_probe_mailbox(femcy_ctx* ctx, int32_t rounds, double* us_per_round);
int femcy_persist_streamed_bytes(femcy_ctx* ctx, int64_t* bytes);

/* ------------------------------------------------------------------- multi-GPU (new work) */
/* 128-byte ncclUniqueId produced on rank 0 and broadcast by the host program */
int femcy_comm_unique_id(void* id128);
/* 128-byte id of an in-process group instead: the contexts that pass it to femcy_comm_init are driven by one host
 * thread each inside ONE process and exchange through host staging buffers (no RCCL; any devices, also all on
 * one).  Same kernels and call sequence as the RCCL transport -- it is how the multi-rank path is verified on a
 * single GPU.  A rendezvous that is not completed by all ranks within 60 s fails with FEMCY_ECOMM. */
int femcy_comm_local_id(void* id128);
/* 128-byte id of a shared-memory group: the ranks are PROCESSES of one host (any devices, also all on one -- which
 * RCCL refuses) that exchange through a POSIX shared-memory segment; same kernels and call sequence as the other
 * transports.  max_values = the longest vector one collective carries (doubles; the packed interface vector + 8 is
 * enough; at least 4096 are reserved).  Produced by one process and handed to the others by the host program (a
 * pipe, a file, the command line).  It exists so that the cross-process branches of the mailbox path below
 * (hipIpcGetMemHandle / hipIpcOpenMemHandle, kernels of different processes writing into each other's HBM) can run
 * on a one-GPU box; a rendezvous that is not completed within 60 s fails with FEMCY_ECOMM.  Up to 16 ranks. */
int femcy_comm_shm_id(void* id128, int64_t max_values);
/* element partition: this ctx holds one sub-mesh; iface_local_dofs[k] is the local scalar DOF that is
 * entry iface_global_slot[k] of the packed global interface vector (length niface_global), owner[i] = 1
 * if this rank counts local DOF i in dot products (exactly one rank per shared DOF). */
int femcy_comm_init(femcy_ctx* ctx, int32_t rank, int32_t nranks, const void* id128,
                    int32_t niface_local, const int32_t* iface_local_dofs, const int32_t* iface_global_slot,
                    int32_t niface_global, const uint8_t* owner /*[n]*/);
/* With a communicator attached every vector the API hands back is the assembled / replicated one: femcy_spmv,
 * femcy_internal_force and femcy_loadset_neumann sum their sub-assembled result over the interface, femcy_vec_norm
 * (RMS over the DOFs of the whole system) and femcy_vec_absmax count each shared DOF once and reduce over the
 * ranks, femcy_elastic_energy sums over the ranks, femcy_pcg's default iteration cap is the global DOF count.
 * These calls are therefore collective: every rank makes the same sequence of them.
 * femcy_comm_info: rank, ranks and the DOF count of the whole system (owned DOFs summed over the ranks; n and 1
 * rank without a communicator).
 * femcy_iface_sum: sum any other sub-assembled vector over the ranks sharing each interface DOF */
int femcy_comm_info(femcy_ctx* ctx, int32_t* rank, int32_t* nranks, int64_t* n_global);
/* Neighbour exchange, the alternative to the packed all-reduce: nb_rank[k] (ascending) shares the local DOFs
 * nb_dofs[nb_ptr[k] .. nb_ptr[k+1]) with this rank, listed in ascending GLOBAL DOF order on both sides.  Per exchange
 * each pair swaps its segment (ncclSend / ncclRecv in one group) and every interface DOF is summed in ascending rank
 * order, so all replicas get the same bits; d.Ad then travels in an 8-byte all-reduce of its own.  The z-slab
 * partitions have <= 2 neighbours per rank: 2 x 116 KB per exchange at 8 M elements instead of a 0.8 MB all-reduce. */
int femcy_comm_set_neighbours(femcy_ctx* ctx, int32_t nnb, const int32_t* nb_rank, const int32_t* nb_ptr,
                              const int32_t* nb_dofs);
/* collective: times `iters` interface exchanges with each method (the neighbour form including its extra scalar
 * all-reduce), checks that both give the same sums, takes the maximum over the ranks and selects the faster one
 * (FEMCY_OPT_EXCHANGE) on every rank alike.  us[0] / us[1] = microseconds per exchange (all-reduce / neighbour);
 * a failed cross-check keeps the all-reduce and reports us[1] = -1. */
int femcy_comm_tune(femcy_ctx* ctx, int32_t iters, int32_t* chosen, double* us /*[2]*/);
int femcy_iface_sum(femcy_ctx* ctx, int vec);
/* Persistent PCG across ranks (FEMCY_OPT_PCG_PERSIST_MULTI).  After femcy_comm_set_neighbours:
 *   femcy_comm_mailbox_export  allocates this rank's mailbox (fine-grained device memory the peers' kernels write
 *                              into) and describes it in a 256-byte blob: IPC handle, process id, device pointer,
 *                              neighbour segment table;
 *   (the host program hands every rank all blobs, in rank order -- torch.distributed all-gather, MPI, a list)
 *   femcy_comm_mailbox_import  maps the peers' mailboxes (same process: the pointer, with peer access between
 *                              devices; other processes: hipIpcOpenMemHandle) and builds the interface tables;
 *   femcy_comm_persist_agree   collective: enabled = 1 only if every rank can take the path (mailboxes mapped, every
 *                              interface node shared with exactly one other rank as in a slab partition, at most 8
 *                              neighbours, the pattern fits the persistent kernel).
 * femcy_pcg then takes the one-launch path on every rank alike; after each such solve the ranks agree through the
 * communicator whether it completed, and a solve that timed out anywhere is redone everywhere by the RCCL loop. */
int femcy_comm_mailbox_export(femcy_ctx* ctx, void* blob256);
/* collective helper for the step in the middle: `bytes` host bytes of every rank -> recv[nranks][bytes] on every rank,
 * through the context's own transport (no communicator: a copy) -- the host program needs no second communication
 * library to hand the blobs round */
int femcy_comm_allgather_host(femcy_ctx* ctx, const void* send, int32_t bytes, void* recv /*[nranks*bytes]*/);
int femcy_comm_mailbox_import(femcy_ctx* ctx, int32_t nblobs, const void* blobs /*[nranks][256]*/);
int femcy_comm_persist_agree(femcy_ctx* ctx, int32_t* enabled);

#ifdef __cplusplus
}
#endif
#endif /* FEMCY_H */
