// libfemcy_cpu.so: the C ABI of include/femcy.h on the HOST (C++17 + OpenMP) -- SURVEY.md 8b "a CPU implementation of the
// same ABI", BASELINE configs[0] "plumbing, no GPU".  The reference runs on the CPU by one line (main.py:11) and solves
// small systems on the host (stiffnessMtrx.py:219-251); this backend lets `python -m femcy_amd.main deck.inp` and the
// whole Python surface run on a box without a GPU.
//
// It is NOT the oracle (`oracle/` restates the reference as written and is test infrastructure) and it is never chosen
// silently: femcy_amd.backend loads it only when FEMCY_BACKEND=cpu is set.  The arithmetic of an element, a Gauss
// point, a facet is the SAME CODE the HIP kernels run (csrc/element_math.hpp); what differs is storage and schedule:
//   * K is block-CSR (dm x dm blocks, the diagonal block first, then ascending columns -- the slot order of the
//     device's SELL matrix, so the reference-layout exports agree entry for entry), rows contiguous in memory;
//   * assembly is owner-computes by matrix row (one OpenMP task per node, its incident elements in ascending order:
//     no atomics, bit-reproducible for any thread count);
//   * reductions are sums of fixed chunks (1024 entries / 128 matrix rows) combined in order: the same bits for any thread count;
//   * PCG is the reference recurrence (conjugateGradientSolver.py:103-127) with the device's conventions (r0 = 0 ->
//     0 iterations, NaN/Inf -> FEMCY_ENUMERIC), fused as far as the dependencies allow: SpMV + d.Ad in one pass,
//     x / r update + r.M.r + max|r| in one pass, d update in one pass.
// Multi-rank entry points return FEMCY_ECOMM (one process = the whole mesh); the device probes return FEMCY_EINVAL.
#include <omp.h>
#include <algorithm>
#include <chrono>
#include <cmath>
#include <cstdarg>
#include <cstdio>
#include <cstring>
#include <new>
#include <vector>
#include "../../include/femcy.h"
#include "../csrc/api_checks.hpp"
#include "../csrc/band_order.hpp"
#include "../csrc/element_dispatch.hpp"
#include "../csrc/element_math.hpp"
#include "../csrc/motion_tables.hpp"

using namespace femcy;

static thread_local char g_err[1024] = "";
void femcy::set_error(const char* fmt, ...) {
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(g_err, sizeof(g_err), fmt, ap);
    va_end(ap);
}

namespace {

double now_ms() {
    return std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now().time_since_epoch()).count();
}

constexpr int64_t CHUNK = 1024;   // reduction granule (vector entries): partial sums of fixed chunks, combined in order
constexpr int64_t NODE_CHUNK = 128;   // the same for loops over matrix rows (nodes)

struct DofSet {
    std::vector<int32_t> dofs;
};
struct LoadSet {
    int32_t nft, nfn, nip, nload;
    std::vector<int32_t> ft_nodes, elem, ft, node, ptr, slot;
    std::vector<double> N, dN, normal, weight, contrib;
};
struct BodyLoad {
    std::vector<double> m;   // [nn] nodal weights
};
struct Mass {
    std::vector<double> m;   // [blocks of the block-CSR matrix] one scalar per block, K's block order
};
struct LumpedMass {
    double rho = 0.0;        // the density it was created with: rho_0 of the bulk viscosity
    std::vector<double> m;   // [nn] HRZ-lumped nodal masses
    std::vector<double> me;  // [ne][npe] the element shares they were summed from (the element-by-element increment)
    std::vector<double> scale;  // [ne] cumulative factors of femcy_lumped_mass_scale; empty before its first call: all 1
};
struct Explicit {
    std::vector<double> minv;   // [n] inverse mass per scalar DOF, 0 on the constrained DOFs
    int32_t lumped;
    femcy::ExplicitClock clock{};   // femcy_explicit_auto_*
    bool auto_begun = false;
    double alpha = 0.0, b1 = 0.0, b2 = 0.0, Md = 0.0;      // femcy_explicit_set_damping; all 0: undamped
    bool damped() const { return alpha != 0.0 || b1 != 0.0 || b2 != 0.0; }
    bool bulk() const { return b1 != 0.0 || b2 != 0.0; }
    // femcy_explicit_set_motion: the DOF-set ids the integrator holds and the device's tables (csrc/motion_tables.hpp;
    // motion.dof empty: no motion), then the clock of a fixed run (csrc/element_math.hpp: explicit_fixed_time)
    std::vector<int32_t> held;
    femcy::MotionTables motion;
    bool moved() const { return !motion.dof.empty(); }
    int64_t n_done = 0, n_base = 0;
    double t_base = 0.0, dt_prev = 0.0;
    // femcy_explicit_energy_enable: asked for / running since a start; the four sums, the forces [n] of the last kicked
    // state with its load scale and time, and per-node scratch [nn][4] of one step's addends
    bool energy_want = false, energy_on = false;
    double en[4] = {0.0, 0.0, 0.0, 0.0}, en_s = 0.0, en_t = 0.0;
    std::vector<double> efint, ealpha, ew;
    // femcy_explicit_set_wall (csrc/element_math.hpp: ExplicitWalls; walls.n = 0: none) and the sum of the penalties
    femcy::ExplicitWalls walls{};
    double wall_kappa() const {
        double k = 0.0;
        for (int32_t w = 0; w < walls.n; ++w) k += walls.kappa[w];
        return k;
    }
};
// a damped element pass or bound (the device's GeomDamping): v, a (null: the start, v_{-1/2} := v_0) and hh = h / 2 of the
// drift that led to the state
struct HostDamping {
    const double *v, *a;
    double hh;
    femcy::ExplicitDamping d;
};
struct Thermal {
    std::vector<double> f, dT, N;  // [n] load at scale 1, [nn] temperature changes, [nGP][npe] shape functions
    double s[9];                    // stress of full restraint per unit temperature change, row-major tensor
};

}  // namespace

struct femcy_ctx {
    int32_t nn = 0, dm = 0, ne = 0, npe = 0, nGP = 0, s = 0;
    int64_t n = 0;
    std::vector<double> nodes, dN, w;
    std::vector<int32_t> elems;
    double h_C[36] = {0}, mat_params[4] = {0, 0, 0, 0}, cubic[3] = {0, 0, 0};
    int32_t mat_kind = -1;
    bool C_is_cubic = false, have_mesh = false, have_element = false, have_material = false, have_pattern = false;
    int asm_used = -1;                    // the mode the last assembly ran (femcy_get_assembly_used)
    // block-CSR matrix: row a = blocks rowptr[a] .. rowptr[a+1], diagonal first, then ascending columns
    std::vector<int64_t> rowptr;
    std::vector<int32_t> col;
    std::vector<double> K;
    std::vector<int64_t> eslot;          // [ne][npe][npe] element-local (a, b) -> block index
    std::vector<int32_t> ne_ptr, ne_idx; // node -> (element * npe + local index), ascending
    int32_t max_row_blocks = 0, max_node_elems = 0;
    // Gauss-point fields
    std::vector<double> dsdx, vol, F, sigma, strain, mises, energy, fe;
    std::vector<double> vec[FEMCY_VEC_COUNT], r, d, M, Ad;
    std::vector<DofSet> dofsets;
    std::vector<LoadSet> loadsets;
    std::vector<BodyLoad> bodyloads;
    std::vector<Thermal> thermals;
    std::vector<Mass> masses;
    std::vector<LumpedMass> lumped_masses;
    std::vector<Explicit> explicits;
    std::vector<femcy::Amplitude> amplitudes;   // femcy_amplitude_create; dropped where integrators are
    bool have_K = false;                  // K holds an assembled matrix of the current pattern (femcy_explicit_stable_dt)
    bool post_small = false;             // sigma / mises hold femcy_compute_strain_stress(large = 0), not yet corrected
    int opt_tangent = 0, opt_timing = 0;
    femcy_timing_t timing{};
    // femcy_direct_solve: band order of the current pattern (built on first use), storage limit
    BandOrder band_order;
    bool have_band_order = false;
    int64_t direct_max_bytes = (int64_t)48 << 30;
};

template <>
bool femcy::vec_allocated(const femcy_ctx* c, int v) {
    return !c->vec[v].empty();
}

namespace {

enum : unsigned { GEOM_DSDX = 1, GEOM_F = 2, GEOM_SIGMA = 4, GEOM_FE = 8 };

// get_dsdx_and_vol (stiffnessMtrx.py:132-150), get_deformation_gradient (:532-556), constitutiveOfLargeDeform and the
// per-element nodal forces of assemble_nodal_force_GN (:620-644): the element pass of the device's k_geom
// DAMPED: hd is set (a damped explicit step); the undamped pass carries nothing of it
template <int DM, bool DAMPED>
void geom_pass(femcy_ctx* c, const double* u, unsigned what, [[maybe_unused]] const HostDamping* hd) {
    const int npe = c->npe, nGP = c->nGP;
#pragma omp parallel for schedule(static)
    for (int32_t e = 0; e < c->ne; ++e) {
        double X[27][DM], U[27][DM], facc[27][DM];
        [[maybe_unused]] double Vh[DAMPED ? 27 : 1][DM];
        for (int a = 0; a < npe; ++a) {
            const int32_t nd = c->elems[(int64_t)e * npe + a];
            for (int i = 0; i < DM; ++i) {
                X[a][i] = c->nodes[(int64_t)nd * DM + i];
                U[a][i] = u ? u[(int64_t)nd * DM + i] : 0.0;
                facc[a][i] = 0.0;
                if constexpr (DAMPED) {
                    const double vi = hd->v[(int64_t)nd * DM + i];
                    Vh[a][i] = hd->a ? explicit_vhalf(vi, hd->a[(int64_t)nd * DM + i], hd->hh) : vi;
                }
            }
        }
        for (int g = 0; g < nGP; ++g) {
            const double* dNg = c->dN.data() + (size_t)g * npe * DM;
            double J[DM][DM], inv[DM][DM];
            for (int i = 0; i < DM; ++i)
                for (int j = 0; j < DM; ++j) {
                    double acc = 0.0;
                    for (int a = 0; a < npe; ++a) acc += (X[a][i] + U[a][i]) * dNg[a * DM + j];
                    J[i][j] = acc;
                }
            const double det = det_inv<DM>(J, inv);
            const int64_t gp = (int64_t)e * nGP + g;
            if (what & GEOM_DSDX) {
                double* out = c->dsdx.data() + gp * npe * DM;
                for (int a = 0; a < npe; ++a)
                    for (int j = 0; j < DM; ++j) {
                        double acc = 0.0;
                        for (int k = 0; k < DM; ++k) acc += dNg[a * DM + k] * inv[k][j];
                        out[a * DM + j] = acc;
                    }
                c->vol[gp] = det * c->w[g];
            }
            if (what & (GEOM_F | GEOM_SIGMA | GEOM_FE)) {
                double J0[DM][DM], inv0[DM][DM], F[DM][DM], sig[DM][DM];
                for (int i = 0; i < DM; ++i)
                    for (int j = 0; j < DM; ++j) {
                        double acc = 0.0;
                        for (int a = 0; a < npe; ++a) acc += X[a][i] * dNg[a * DM + j];
                        J0[i][j] = acc;
                        F[i][j] = 0.0;
                    }
                [[maybe_unused]] const double det0 = det_inv<DM>(J0, inv0);
                for (int a = 0; a < npe; ++a) {
                    double dsdX[DM];
                    for (int j = 0; j < DM; ++j) {
                        double acc = 0.0;
                        for (int k = 0; k < DM; ++k) acc += dNg[a * DM + k] * inv0[k][j];
                        dsdX[j] = acc;
                    }
                    for (int i = 0; i < DM; ++i)
                        for (int j = 0; j < DM; ++j) F[i][j] += U[a][i] * dsdX[j];
                }
                for (int i = 0; i < DM; ++i) F[i][i] += 1.0;
                if (what & GEOM_F)
                    for (int i = 0; i < DM; ++i)
                        for (int j = 0; j < DM; ++j) c->F[gp * DM * DM + i * DM + j] = F[i][j];
                if (what & (GEOM_SIGMA | GEOM_FE)) {
                    cauchy_large<DM>(c->mat_kind, c->h_C, c->mat_params[0], c->mat_params[1], F, sig);
                    if (what & GEOM_SIGMA)
                        for (int i = 0; i < DM; ++i)
                            for (int j = 0; j < DM; ++j) c->sigma[gp * DM * DM + i * DM + j] = sig[i][j];
                    if (what & GEOM_FE) {
                        const double vg = det * c->w[g];
                        if constexpr (DAMPED) {      // bulk viscosity: sigma + p I in the force accumulation only
                            double rate, gmax;
                            bulk_rate_point<0, DM>(npe, dNg, inv, &Vh[0][0], rate, gmax);
                            const double p = bulk_pressure(hd->d, rate, gmax, det / det0);
                            for (int i = 0; i < DM; ++i) sig[i][i] += p;
                        }
                        for (int a = 0; a < npe; ++a) {
                            double ga[DM];
                            for (int j = 0; j < DM; ++j) {
                                double acc = 0.0;
                                for (int k = 0; k < DM; ++k) acc += dNg[a * DM + k] * inv[k][j];
                                ga[j] = acc;
                            }
                            for (int i = 0; i < DM; ++i) {
                                double dsum = 0.0;
                                for (int j = 0; j < DM; ++j) dsum += ga[j] * sig[j][i];
                                facc[a][i] += dsum * vg;
                            }
                        }
                    }
                }
            }
        }
        if (what & GEOM_FE)
            for (int a = 0; a < npe; ++a)
                for (int i = 0; i < DM; ++i) c->fe[((int64_t)e * npe + a) * DM + i] = facc[a][i];
    }
}
void geom(femcy_ctx* c, const double* u, unsigned what, const HostDamping* hd = nullptr) {
    if (what & GEOM_SIGMA) c->post_small = false;
    const double t = c->opt_timing ? now_ms() : 0.0;
    if (hd) {
        if (c->dm == 3) geom_pass<3, true>(c, u, what, hd); else geom_pass<2, true>(c, u, what, hd);
    } else {
        if (c->dm == 3) geom_pass<3, false>(c, u, what, nullptr); else geom_pass<2, false>(c, u, what, nullptr);
    }
    if (c->opt_timing) {
        c->timing.geom_ms += now_ms() - t;
        c->timing.geom_launches++;
    }
}

// assemble_nodal_force_GN_kernel (stiffnessMtrx.py:620-644): per node, its incident elements in ascending order
void nodal_force(femcy_ctx* c, double* f) {
    const double t = c->opt_timing ? now_ms() : 0.0;
    const int dm = c->dm;
#pragma omp parallel for schedule(static)
    for (int32_t a = 0; a < c->nn; ++a) {
        double acc[3] = {0, 0, 0};
        for (int32_t k = c->ne_ptr[a]; k < c->ne_ptr[a + 1]; ++k)
            for (int i = 0; i < dm; ++i) acc[i] += c->fe[(int64_t)c->ne_idx[k] * dm + i];
        for (int i = 0; i < dm; ++i) f[(int64_t)a * dm + i] = acc[i];
    }
    if (c->opt_timing) {
        c->timing.force_ms += now_ms() - t;
        c->timing.force_launches++;
    }
}

// assemble_stiffnessMtrx (stiffnessMtrx.py:161-186): K_ab = sum_g B_a^T C B_b vol, owner-computes by row
template <int DM>
void assemble(femcy_ctx* c) {
    constexpr int DD = DM * DM;
    const int npe = c->npe, nGP = c->nGP;
    const bool consistent = c->opt_tangent == 1;
    const bool neo = c->mat_kind == FEMCY_MAT_NEOHOOKE;
    const int s = DM == 3 ? 6 : 3;
    const double lam = c->h_C[0 * s + 1], mu = c->h_C[(s - 1) * s + (s - 1)];
#pragma omp parallel for schedule(dynamic, 64)
    for (int32_t a = 0; a < c->nn; ++a) {
        double* row = c->K.data() + c->rowptr[a] * DD;
        std::fill(row, row + (c->rowptr[a + 1] - c->rowptr[a]) * DD, 0.0);
        for (int32_t k = c->ne_ptr[a]; k < c->ne_ptr[a + 1]; ++k) {
            const int32_t code = c->ne_idx[k];
            const int64_t e = code / npe;
            const int la = code - (int32_t)e * npe;
            for (int lb = 0; lb < npe; ++lb) {
                double blk[DD];
                for (int q = 0; q < DD; ++q) blk[q] = 0.0;
                for (int g = 0; g < nGP; ++g) {
                    const int64_t gp = e * nGP + g;
                    const double* ga = c->dsdx.data() + (gp * npe + la) * DM;
                    const double* gb = c->dsdx.data() + (gp * npe + lb) * DM;
                    if (consistent)
                        kblock_consistent<DM>(ga, gb, c->F.data() + gp * DD, c->sigma.data() + gp * DD, neo, lam, mu,
                                              c->mat_params[0], c->mat_params[1], c->vol[gp], blk);
                    else if (DM == 3 && c->C_is_cubic)
                        kblock_cubic3(ga, gb, c->cubic[0], c->cubic[1], c->cubic[2], c->vol[gp], reinterpret_cast<double(&)[9]>(blk));
                    else
                        kblock_add<DM>(ga, gb, c->h_C, c->vol[gp], blk);
                }
                double* dst = c->K.data() + c->eslot[((int64_t)e * npe + la) * npe + lb] * DD;
                for (int q = 0; q < DD; ++q) dst[q] += blk[q];
            }
        }
    }
}
int assemble_K(femcy_ctx* c) {
    c->asm_used = -1;
    if (c->opt_tangent == 1 && c->mat_kind == FEMCY_MAT_PSTRESS) {
        set_error("the consistent tangent is not available for plane stress");
        return FEMCY_EINVAL;
    }
    const double t = c->opt_timing ? now_ms() : 0.0;
    if (c->dm == 3) assemble<3>(c); else assemble<2>(c);
    c->asm_used = FEMCY_ASM_ATOMIC;      // one assembly here: owner-computes by row, no mode to choose
    c->have_K = true;
    if (c->opt_timing) {
        c->timing.assemble_ms += now_ms() - t;
        c->timing.assemble_launches++;
    }
    return FEMCY_OK;
}

// compute_Ad (conjugateGradientSolver.py:53-58); returns x.y when dot != nullptr (chunked: thread-count independent)
template <int DM>
void spmv_t(const femcy_ctx* c, const double* x, double* y, double* dot) {
    constexpr int DD = DM * DM;
    const int64_t nchunk = (c->nn + NODE_CHUNK - 1) / NODE_CHUNK;
    std::vector<double> part(dot ? (size_t)nchunk : 0, 0.0);
#pragma omp parallel for schedule(static)
    for (int64_t ch = 0; ch < nchunk; ++ch) {
        double pd = 0.0;
        const int32_t a1 = (int32_t)std::min<int64_t>(c->nn, (ch + 1) * NODE_CHUNK);
        for (int32_t a = (int32_t)(ch * NODE_CHUNK); a < a1; ++a) {
            double acc[DM];
            for (int r = 0; r < DM; ++r) acc[r] = 0.0;
            for (int64_t p = c->rowptr[a]; p < c->rowptr[a + 1]; ++p) {
                const double* b = c->K.data() + p * DD;
                const double* xv = x + (int64_t)c->col[p] * DM;
                for (int r = 0; r < DM; ++r)
                    for (int cc = 0; cc < DM; ++cc) acc[r] += b[r * DM + cc] * xv[cc];
            }
            for (int r = 0; r < DM; ++r) {
                y[(int64_t)a * DM + r] = acc[r];
                pd += x[(int64_t)a * DM + r] * acc[r];
            }
        }
        if (dot) part[ch] = pd;
    }
    if (dot) {
        double sum = 0.0;
        for (double v : part) sum += v;
        *dot = sum;
    }
}
void spmv(femcy_ctx* c, const double* x, double* y, double* dot) {
    const double t = c->opt_timing ? now_ms() : 0.0;
    if (c->dm == 3) spmv_t<3>(c, x, y, dot); else spmv_t<2>(c, x, y, dot);
    if (c->opt_timing) {
        c->timing.spmv_ms += now_ms() - t;
        c->timing.spmv_launches++;
    }
}

double nan_to_inf_abs(double r) {
    const double a = std::fabs(r);
    return (a != a) ? INFINITY : a;
}

// dirichletBC_forNewtonMethod_kernel / the matrix part of dirichletBC_linearEquations (stiffnessMtrx.py:279-341): rows
// and columns of the constrained DOFs zeroed, unit diagonal, optionally the residual entry zeroed
void dirichlet_zero(femcy_ctx* c, const int32_t* dofs, int32_t k, double* resid) {
    const int dm = c->dm, dd = dm * dm;
    for (int32_t q = 0; q < k; ++q) {   // serial: different constrained DOFs touch the same blocks
        const int32_t dof = dofs[q], a = dof / dm, r = dof % dm;
        for (int64_t p = c->rowptr[a]; p < c->rowptr[a + 1]; ++p) {
            for (int cc = 0; cc < dm; ++cc) c->K[p * dd + r * dm + cc] = 0.0;
            const int32_t b = c->col[p];
            int64_t pm = -1;
            if (b == a) {
                pm = p;
            } else {
                const int32_t* lo = c->col.data() + c->rowptr[b] + 1;
                const int32_t* hi = c->col.data() + c->rowptr[b + 1];
                const int32_t* it = std::lower_bound(lo, hi, a);
                if (it != hi && *it == a) pm = it - c->col.data();
            }
            if (pm >= 0)
                for (int cc = 0; cc < dm; ++cc) c->K[pm * dd + cc * dm + r] = 0.0;
        }
        c->K[c->rowptr[a] * dd + r * dm + r] = 1.0;
        if (resid) resid[dof] = 0.0;
    }
}

}  // namespace

#define CTX_OR_FAIL(ctx)     \
    FEMCY_REQUIRE((ctx), TEXT_NULL_CONTEXT); \
    femcy_ctx* c = (ctx)

extern "C" {

const char* femcy_last_error(void) { return g_err; }
int femcy_version(void) { return 100; }

int femcy_ctx_create(int device, femcy_ctx** out) {
    FEMCY_REQUIRE(out, TEXT_CTX_OUT_NULL);
    if (device != 0) {                              // one host = device 0 (the caller's bookkeeping stays honest)
        set_error("device %d out of range (the CPU backend has one device: 0)", device);
        return FEMCY_EINVAL;
    }
    *out = new (std::nothrow) femcy_ctx();
    if (!*out) return FEMCY_ENOMEM;
    return FEMCY_OK;
}
int femcy_ctx_destroy(femcy_ctx* ctx) {
    delete ctx;
    return FEMCY_OK;
}

int femcy_set_option(femcy_ctx* ctx, int option, int64_t value) {
    CTX_OR_FAIL(ctx);
    FEMCY_TRY(check_option(c, option, value));
    switch (option) {
        case FEMCY_OPT_TANGENT:
            c->opt_tangent = (int)value;
            return FEMCY_OK;
        case FEMCY_OPT_TIMING:
            c->opt_timing = value > 0 ? 1 : 0;
            return FEMCY_OK;
        // schedule / layout knobs of the device kernels: accepted, without effect on the host
        case FEMCY_OPT_ASSEMBLY: case FEMCY_OPT_PCG_POLL: case FEMCY_OPT_SPMV_VARIANT: case FEMCY_OPT_EW_GRID:
        case FEMCY_OPT_PCG_GRAPH: case FEMCY_OPT_PCG_PERSIST: case FEMCY_OPT_PCG_SMALL: case FEMCY_OPT_OVERLAP:
        case FEMCY_OPT_PCG_PERSIST_MULTI: case FEMCY_OPT_PCG_STORAGE_ORDER: case FEMCY_OPT_SELL_SIGMA: case FEMCY_OPT_NODE_ORDER:
            return FEMCY_OK;
        case FEMCY_OPT_DIRECT_MAX_BYTES:
            c->direct_max_bytes = value;
            return FEMCY_OK;
        default:
            if (option >= 100 && option <= 119) return FEMCY_OK;   // FEMCY_TUNE_*: device tuning knobs
            set_error(TEXT_UNKNOWN_OPTION, option);
            return FEMCY_EINVAL;
    }
}
int femcy_sync(femcy_ctx* ctx) {
    CTX_OR_FAIL(ctx);
    (void)c;
    return FEMCY_OK;
}

int femcy_set_mesh(femcy_ctx* ctx, int32_t nn, int32_t dm, const double* nodes, int32_t ne, int32_t npe,
                   const int32_t* elems) {
    CTX_OR_FAIL(ctx);
    FEMCY_TRY(check_set_mesh(nn, dm, nodes, ne, npe, elems));
    c->dofsets.clear();
    c->loadsets.clear();
    c->bodyloads.clear();
    c->thermals.clear();
    c->masses.clear();
    c->lumped_masses.clear();
    c->explicits.clear();
    c->amplitudes.clear();
    c->have_K = false;
    c->post_small = false;
    c->nn = nn; c->dm = dm; c->ne = ne; c->npe = npe;
    c->n = (int64_t)nn * dm;
    c->nodes.assign(nodes, nodes + (size_t)nn * dm);
    c->elems.assign(elems, elems + (size_t)ne * npe);
    for (auto& v : c->vec) v.assign((size_t)c->n, 0.0);
    c->r.assign((size_t)c->n, 0.0);
    c->d.assign((size_t)c->n, 0.0);
    c->M.assign((size_t)c->n, 0.0);
    c->Ad.assign((size_t)c->n, 0.0);
    c->have_mesh = true;
    c->have_material = c->have_element = c->have_pattern = false;
    return FEMCY_OK;
}

int femcy_set_element(femcy_ctx* ctx, int32_t nGP, const double* dN, const double* w, int32_t voigt_kind) {
    CTX_OR_FAIL(ctx);
    FEMCY_TRY(check_set_element(c, nGP, dN, w, voigt_kind));
    c->nGP = nGP;
    c->s = c->dm == 2 ? 3 : 6;
    c->dN.assign(dN, dN + (size_t)nGP * c->npe * c->dm);
    c->w.assign(w, w + nGP);
    const size_t ngp = (size_t)c->ne * nGP, dd = (size_t)c->dm * c->dm;
    c->dsdx.assign(ngp * c->npe * c->dm, 0.0);
    c->vol.assign(ngp, 0.0);
    c->F.assign(ngp * dd, 0.0);
    c->sigma.assign(ngp * dd, 0.0);
    c->strain.assign(ngp * dd, 0.0);
    c->mises.assign(ngp, 0.0);
    c->energy.assign(ngp, 0.0);
    c->fe.assign((size_t)c->ne * c->npe * c->dm, 0.0);
    c->have_element = true;
    c->post_small = false;
    return FEMCY_OK;
}

int femcy_set_material(femcy_ctx* ctx, int32_t kind, const double* C, const double* params, int32_t nparams) {
    CTX_OR_FAIL(ctx);
    FEMCY_TRY(check_set_material(c, kind, C, params, nparams));
    const int s = c->dm == 2 ? 3 : 6;
    for (int i = 0; i < s * s; ++i) c->h_C[i] = C[i];
    c->mat_kind = kind;
    c->C_is_cubic = false;
    if (s == 6) {   // cubic pattern (exact comparisons), as on the device
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

// body.get_nodeEles / get_coElement_nodes + sparseIJ (body.py:165-194, stiffnessMtrx.py:70-89)
int femcy_build_pattern(femcy_ctx* ctx) {
    CTX_OR_FAIL(ctx);
    FEMCY_TRY(check_have_mesh(c));
    const int32_t nn = c->nn, ne = c->ne, npe = c->npe;
    c->ne_ptr.assign((size_t)nn + 1, 0);
    for (int64_t k = 0; k < (int64_t)ne * npe; ++k) c->ne_ptr[c->elems[k] + 1]++;
    c->max_node_elems = 0;
    for (int32_t a = 0; a < nn; ++a) {
        c->max_node_elems = std::max(c->max_node_elems, c->ne_ptr[a + 1]);
        c->ne_ptr[a + 1] += c->ne_ptr[a];
    }
    c->ne_idx.resize((size_t)ne * npe);
    {
        std::vector<int32_t> cur(c->ne_ptr.begin(), c->ne_ptr.end() - 1);
        for (int64_t k = 0; k < (int64_t)ne * npe; ++k) c->ne_idx[cur[c->elems[k]]++] = (int32_t)k;   // ascending (e, la)
    }
    // node adjacency: diagonal first, then ascending
    std::vector<int32_t> rowlen((size_t)nn);
    std::vector<std::vector<int32_t>> rows((size_t)nn);
#pragma omp parallel
    {
        std::vector<int32_t> tmp;
#pragma omp for schedule(dynamic, 256)
        for (int32_t a = 0; a < nn; ++a) {
            tmp.clear();
            for (int32_t k = c->ne_ptr[a]; k < c->ne_ptr[a + 1]; ++k) {
                const int64_t e = c->ne_idx[k] / npe;
                for (int lb = 0; lb < npe; ++lb) tmp.push_back(c->elems[e * npe + lb]);
            }
            std::sort(tmp.begin(), tmp.end());
            tmp.erase(std::unique(tmp.begin(), tmp.end()), tmp.end());
            auto& row = rows[a];
            row.clear();
            row.push_back(a);
            for (int32_t b : tmp)
                if (b != a) row.push_back(b);
            rowlen[a] = (int32_t)row.size();
        }
    }
    c->rowptr.assign((size_t)nn + 1, 0);
    c->max_row_blocks = 0;
    for (int32_t a = 0; a < nn; ++a) {
        c->rowptr[a + 1] = c->rowptr[a] + rowlen[a];
        c->max_row_blocks = std::max(c->max_row_blocks, rowlen[a]);
    }
    const int64_t nnzb = c->rowptr[nn];
    c->col.resize((size_t)nnzb);
#pragma omp parallel for schedule(static)
    for (int32_t a = 0; a < nn; ++a) std::copy(rows[a].begin(), rows[a].end(), c->col.begin() + c->rowptr[a]);
    rows.clear();
    rows.shrink_to_fit();
    c->K.assign((size_t)nnzb * c->dm * c->dm, 0.0);
    c->eslot.resize((size_t)ne * npe * npe);
#pragma omp parallel for schedule(static)
    for (int32_t e = 0; e < ne; ++e)
        for (int la = 0; la < npe; ++la) {
            const int32_t a = c->elems[(int64_t)e * npe + la];
            const int32_t* lo = c->col.data() + c->rowptr[a];
            const int32_t* hi = c->col.data() + c->rowptr[a + 1];
            for (int lb = 0; lb < npe; ++lb) {
                const int32_t b = c->elems[(int64_t)e * npe + lb];
                const int64_t p = (b == a) ? c->rowptr[a] : (std::lower_bound(lo + 1, hi, b) - c->col.data());
                c->eslot[((int64_t)e * npe + la) * npe + lb] = p;
            }
        }
    c->have_pattern = true;
    c->have_band_order = false;
    c->have_K = false;
    return FEMCY_OK;
}

// one assembly here: a serial scatter element by element in ascending element order
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
    out->nnzb = c->rowptr[c->nn];
    out->nnz = out->nnzb * c->dm * c->dm;
    out->max_row_blocks = c->max_row_blocks;
    out->ell_width = c->max_row_blocks * c->dm;
    out->stored_blocks = out->nnzb;                 // block-CSR: no padding
    out->nslices = (c->nn + 63) / 64;
    out->max_node_elems = c->max_node_elems;
    return FEMCY_OK;
}
int femcy_get_node_order(femcy_ctx* ctx, int32_t* used, double* lines) {
    CTX_OR_FAIL(ctx);
    FEMCY_REQUIRE(c->have_pattern, TEXT_PATTERN_NOT_BUILT);
    if (used) *used = 0;                                  // the host backend keeps the caller's numbering (block CSR)
    if (lines)
        for (int k = 0; k < 7; ++k) lines[k] = 0.0;
    return FEMCY_OK;
}

// ---------------------------------------------------------------------------- vector plumbing
int femcy_vec_upload(femcy_ctx* ctx, int vec, const double* src, int64_t n) {
    CTX_OR_FAIL(ctx);
    FEMCY_TRY(check_vec_transfer(c, "upload", vec, src, n));
    std::memcpy(c->vec[vec].data(), src, sizeof(double) * n);
    return FEMCY_OK;
}
int femcy_vec_download(femcy_ctx* ctx, int vec, double* dst, int64_t n) {
    CTX_OR_FAIL(ctx);
    FEMCY_TRY(check_vec_transfer(c, "download", vec, dst, n));
    std::memcpy(dst, c->vec[vec].data(), sizeof(double) * n);
    return FEMCY_OK;
}
int femcy_vec_fill(femcy_ctx* ctx, int vec, double value) {
    CTX_OR_FAIL(ctx);
    VEC_OR_FAIL(vec);
    std::fill(c->vec[vec].begin(), c->vec[vec].end(), value);
    return FEMCY_OK;
}
int femcy_vec_copy(femcy_ctx* ctx, int dst, int src) {
    CTX_OR_FAIL(ctx);
    VEC_OR_FAIL(dst);
    VEC_OR_FAIL(src);
    if (dst != src) c->vec[dst] = c->vec[src];
    return FEMCY_OK;
}
int femcy_vec_scatter(femcy_ctx* ctx, int vec, const int32_t* idx, const double* vals, int32_t k) {
    CTX_OR_FAIL(ctx);
    VEC_OR_FAIL(vec);
    if (k == 0) return FEMCY_OK;
    FEMCY_TRY(check_vec_scatter(c, idx, vals, k));
    for (int32_t i = 0; i < k; ++i) c->vec[vec][idx[i]] = vals[i];
    return FEMCY_OK;
}
int femcy_vec_sub(femcy_ctx* ctx, int cv, int a, int b) {
    CTX_OR_FAIL(ctx);
    VEC_OR_FAIL(cv); VEC_OR_FAIL(a); VEC_OR_FAIL(b);
    double* pc = c->vec[cv].data();
    const double *pa = c->vec[a].data(), *pb = c->vec[b].data();
#pragma omp parallel for schedule(static)
    for (int64_t i = 0; i < c->n; ++i) pc[i] = pa[i] - pb[i];
    return FEMCY_OK;
}
int femcy_vec_axpy(femcy_ctx* ctx, int a, int b, double cc, int d) {
    CTX_OR_FAIL(ctx);
    VEC_OR_FAIL(a); VEC_OR_FAIL(b); VEC_OR_FAIL(d);
    double* pa = c->vec[a].data();
    const double *pb = c->vec[b].data(), *pd = c->vec[d].data();
#pragma omp parallel for schedule(static)
    for (int64_t i = 0; i < c->n; ++i) pa[i] = pb[i] + cc * pd[i];
    return FEMCY_OK;
}
int femcy_vec_scale(femcy_ctx* ctx, int vec, double s) {
    CTX_OR_FAIL(ctx);
    VEC_OR_FAIL(vec);
    for (double& v : c->vec[vec]) v *= s;
    return FEMCY_OK;
}
int femcy_vec_norm(femcy_ctx* ctx, int vec, double* rms) {
    CTX_OR_FAIL(ctx);
    VEC_OR_FAIL(vec);
    FEMCY_REQUIRE(rms, TEXT_NULL_OUTPUT);
    const double* p = c->vec[vec].data();
    const int64_t nchunk = (c->n + CHUNK - 1) / CHUNK;
    std::vector<double> part((size_t)nchunk);
#pragma omp parallel for schedule(static)
    for (int64_t ch = 0; ch < nchunk; ++ch) {
        double s = 0.0;
        const int64_t i1 = std::min(c->n, (ch + 1) * CHUNK);
        for (int64_t i = ch * CHUNK; i < i1; ++i) s += p[i] * p[i];
        part[ch] = s;
    }
    double ss = 0.0;
    for (double v : part) ss += v;
    *rms = std::sqrt(ss / (double)c->n);
    return FEMCY_OK;
}
int femcy_vec_absmax(femcy_ctx* ctx, int vec, double* out) {
    CTX_OR_FAIL(ctx);
    VEC_OR_FAIL(vec);
    FEMCY_REQUIRE(out, TEXT_NULL_OUTPUT);
    double m = 0.0;
    for (double v : c->vec[vec]) m = std::fmax(m, nan_to_inf_abs(v));
    *out = m;
    return FEMCY_OK;
}

// -------------------------------------------------------------------------------- the hot path
int femcy_assemble_K(femcy_ctx* ctx, int u_vec) {
    CTX_OR_FAIL(ctx);
    READY_OR_FAIL();
    const double* u = nullptr;
    if (u_vec >= 0) {
        VEC_OR_FAIL(u_vec);
        u = c->vec[u_vec].data();
    }
    geom(c, u, c->opt_tangent == 1 ? (GEOM_DSDX | GEOM_F | GEOM_SIGMA) : GEOM_DSDX);
    return assemble_K(c);
}
int femcy_internal_force(femcy_ctx* ctx, int u_vec, int f_vec) {
    CTX_OR_FAIL(ctx);
    READY_OR_FAIL();
    VEC_OR_FAIL(u_vec);
    VEC_OR_FAIL(f_vec);
    geom(c, c->vec[u_vec].data(), GEOM_DSDX | GEOM_F | GEOM_SIGMA | GEOM_FE);
    nodal_force(c, c->vec[f_vec].data());
    return FEMCY_OK;
}
int femcy_residual_and_K(femcy_ctx* ctx, int u_vec, int f_vec) {
    CTX_OR_FAIL(ctx);
    READY_OR_FAIL();
    VEC_OR_FAIL(u_vec);
    VEC_OR_FAIL(f_vec);
    geom(c, c->vec[u_vec].data(), GEOM_DSDX | GEOM_F | GEOM_SIGMA | GEOM_FE);
    nodal_force(c, c->vec[f_vec].data());
    return assemble_K(c);
}

// dirichletBC_linearEquations (stiffnessMtrx.py:279-307), race-free: rhs -= K s with the not yet modified matrix
static int dirichlet_linear(femcy_ctx* c, const int32_t* dofs, const double* vals, double value, int32_t k, int rhs_vec) {
    bool any = false;
    for (int32_t i = 0; i < k; ++i) any = any || ((vals ? vals[i] : value) != 0.0);
    double* rhs = c->vec[rhs_vec].data();
    if (any) {
        std::vector<double>& s = c->vec[FEMCY_VEC_TMP0];
        std::vector<double>& Ks = c->vec[FEMCY_VEC_TMP1];
        std::fill(s.begin(), s.end(), 0.0);
        for (int32_t i = 0; i < k; ++i) s[dofs[i]] = vals ? vals[i] : value;
        spmv(c, s.data(), Ks.data(), nullptr);
        for (int64_t i = 0; i < c->n; ++i) rhs[i] -= Ks[i];
    }
    for (int32_t i = 0; i < k; ++i) rhs[dofs[i]] = vals ? vals[i] : value;
    dirichlet_zero(c, dofs, k, nullptr);
    return FEMCY_OK;
}
int femcy_apply_dirichlet_linear(femcy_ctx* ctx, const int32_t* dofs, const double* vals, int32_t k, int rhs_vec) {
    CTX_OR_FAIL(ctx);
    READY_OR_FAIL();
    VEC_OR_FAIL(rhs_vec);
    if (k == 0) return FEMCY_OK;
    FEMCY_TRY(check_dirichlet_linear(c, dofs, vals, k, rhs_vec));
    return dirichlet_linear(c, dofs, vals, 0.0, k, rhs_vec);
}
int femcy_apply_dirichlet_newton(femcy_ctx* ctx, const int32_t* dofs, int32_t k, int residual_vec) {
    CTX_OR_FAIL(ctx);
    READY_OR_FAIL();
    VEC_OR_FAIL(residual_vec);
    if (k == 0) return FEMCY_OK;
    FEMCY_TRY(check_dirichlet_newton(c, dofs, k));
    dirichlet_zero(c, dofs, k, c->vec[residual_vec].data());
    return FEMCY_OK;
}
int femcy_dofset_create(femcy_ctx* ctx, const int32_t* dofs, int32_t k, int32_t* id_out) {
    CTX_OR_FAIL(ctx);
    FEMCY_TRY(check_dofset_create(c, dofs, k, id_out));
    DofSet ds;
    if (k) ds.dofs.assign(dofs, dofs + k);
    c->dofsets.push_back(ds);
    *id_out = (int32_t)c->dofsets.size() - 1;
    return FEMCY_OK;
}
int femcy_dofset_dirichlet_newton(femcy_ctx* ctx, int32_t id, int residual_vec) {
    CTX_OR_FAIL(ctx);
    READY_OR_FAIL();
    VEC_OR_FAIL(residual_vec);
    FEMCY_OBJECT_OR_FAIL(ds, c->dofsets, id, "dofset");
    dirichlet_zero(c, ds.dofs.data(), (int32_t)ds.dofs.size(), c->vec[residual_vec].data());
    return FEMCY_OK;
}
int femcy_dofset_dirichlet_linear(femcy_ctx* ctx, int32_t id, double value, int rhs_vec) {
    CTX_OR_FAIL(ctx);
    READY_OR_FAIL();
    VEC_OR_FAIL(rhs_vec);
    FEMCY_OBJECT_OR_FAIL(ds, c->dofsets, id, "dofset");
    FEMCY_TRY(check_rhs_not_scratch(rhs_vec));
    if (ds.dofs.empty()) return FEMCY_OK;
    return dirichlet_linear(c, ds.dofs.data(), nullptr, value, (int32_t)ds.dofs.size(), rhs_vec);
}
int femcy_dofset_fill(femcy_ctx* ctx, int32_t id, int vec, double value) {
    CTX_OR_FAIL(ctx);
    VEC_OR_FAIL(vec);
    FEMCY_OBJECT_OR_FAIL(ds, c->dofsets, id, "dofset");
    for (int32_t dof : ds.dofs) c->vec[vec][dof] = value;
    return FEMCY_OK;
}
int femcy_dofset_add(femcy_ctx* ctx, int32_t id, int vec, double value) {
    CTX_OR_FAIL(ctx);
    VEC_OR_FAIL(vec);
    FEMCY_OBJECT_OR_FAIL(ds, c->dofsets, id, "dofset");
    for (int32_t dof : ds.dofs) c->vec[vec][dof] += value;
    return FEMCY_OK;
}
int femcy_dofset_scatter(femcy_ctx* ctx, int32_t id, int vec, const double* vals) {
    CTX_OR_FAIL(ctx);
    VEC_OR_FAIL(vec);
    FEMCY_OBJECT_OR_FAIL(ds, c->dofsets, id, "dofset");
    if (ds.dofs.empty()) return FEMCY_OK;
    FEMCY_REQUIRE(vals, TEXT_NULL_VALUES);
    for (size_t i = 0; i < ds.dofs.size(); ++i) c->vec[vec][ds.dofs[i]] = vals[i];
    return FEMCY_OK;
}

// ------------------------------------------------------------------------------- Neumann load sets
int femcy_loadset_create(femcy_ctx* ctx, int32_t nft, int32_t nfn, int32_t nip, const int32_t* ft_nodes,
                         const double* ft_N, const double* ft_dN, const double* ft_normal, const double* ft_weight,
                         int32_t nload, const int32_t* load_elem, const int32_t* load_ft, int32_t* id_out) {
    CTX_OR_FAIL(ctx);
    FEMCY_TRY(check_loadset_create(c, nft, nfn, nip, ft_nodes, ft_N, ft_dN, ft_normal, ft_weight, nload, load_elem, load_ft,
                                   id_out));
    LoadSet ls;
    ls.nft = nft; ls.nfn = nfn; ls.nip = nip; ls.nload = nload;
    const size_t tip = (size_t)nft * nip, nslot = (size_t)nload * nfn;
    ls.ft_nodes.assign(ft_nodes, ft_nodes + (size_t)nft * nfn);
    ls.N.assign(ft_N, ft_N + tip * c->npe);
    ls.dN.assign(ft_dN, ft_dN + tip * c->npe * c->dm);
    ls.normal.assign(ft_normal, ft_normal + tip * c->dm);
    ls.weight.assign(ft_weight, ft_weight + tip);
    if (nload) {
        ls.elem.assign(load_elem, load_elem + nload);
        ls.ft.assign(load_ft, load_ft + nload);
    }
    // loaded nodes and, per node, its contribution slots (facet * nfn + facet node) in ascending order
    std::vector<int32_t> slot_node(nslot);
    ls.slot.resize(nslot);
    for (int32_t l = 0; l < nload; ++l)
        for (int32_t f = 0; f < nfn; ++f)
            slot_node[(size_t)l * nfn + f] = c->elems[(size_t)load_elem[l] * c->npe + ft_nodes[(size_t)load_ft[l] * nfn + f]];
    for (size_t i = 0; i < nslot; ++i) ls.slot[i] = (int32_t)i;
    std::stable_sort(ls.slot.begin(), ls.slot.end(), [&](int32_t a, int32_t b) { return slot_node[a] < slot_node[b]; });
    for (size_t i = 0; i < nslot; ++i)
        if (i == 0 || slot_node[ls.slot[i]] != slot_node[ls.slot[i - 1]]) {
            ls.node.push_back(slot_node[ls.slot[i]]);
            ls.ptr.push_back((int32_t)i);
        }
    ls.ptr.push_back((int32_t)nslot);
    ls.contrib.assign(std::max<size_t>(nslot, 1) * c->dm, 0.0);
    c->loadsets.push_back(std::move(ls));
    *id_out = (int32_t)c->loadsets.size() - 1;
    return FEMCY_OK;
}

// neumannBC (stiffnessMtrx.py:369-411); add: the node sums are added to rhs instead of a zero-filled rhs
static int loadset_neumann(femcy_ctx* c, int32_t id, double traction, const double* direction, int rhs_vec, bool add) {
    VEC_OR_FAIL(rhs_vec);
    FEMCY_TRY(check_object(c->loadsets, id, "load set"));
    LoadSet& ls = c->loadsets[id];
    double* rhs = c->vec[rhs_vec].data();
    if (!add) std::fill(rhs, rhs + c->n, 0.0);      // reference :384
    const int dm = c->dm;
#pragma omp parallel for schedule(static)
    for (int32_t l = 0; l < ls.nload; ++l) {
        const int32_t* en = c->elems.data() + (int64_t)ls.elem[l] * c->npe;
        double* out = ls.contrib.data() + (int64_t)l * ls.nfn * dm;
        if (dm == 3)
            neumann_facet<3>(c->npe, ls.nfn, ls.nip, c->nodes.data(), en, ls.ft[l], ls.ft_nodes.data(), ls.N.data(),
                             ls.dN.data(), ls.normal.data(), ls.weight.data(), traction, direction, out);
        else
            neumann_facet<2>(c->npe, ls.nfn, ls.nip, c->nodes.data(), en, ls.ft[l], ls.ft_nodes.data(), ls.N.data(),
                             ls.dN.data(), ls.normal.data(), ls.weight.data(), traction, direction, out);
    }
    for (size_t i = 0; i < ls.node.size(); ++i)
        for (int dd = 0; dd < dm; ++dd) {
            double s = 0.0;
            for (int32_t k = ls.ptr[i]; k < ls.ptr[i + 1]; ++k) s += ls.contrib[(int64_t)ls.slot[k] * dm + dd];
            double& dst = rhs[(int64_t)ls.node[i] * dm + dd];
            dst = add ? dst + s : s;
        }
    return FEMCY_OK;
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
}  // extern "C"
namespace {
// the element pass of the device's k_body_weights (csrc/element_math.hpp: body_weights_element), then the node sums in
// ascending (element, local node) order
template <int NPE, int DM>
void body_weights(femcy_ctx* c, const double* N, const uint8_t* mask, std::vector<double>& m) {
    std::vector<double> we((size_t)c->ne * NPE, 0.0);
#pragma omp parallel for schedule(static)
    for (int32_t e = 0; e < c->ne; ++e) {
        if (mask && !mask[e]) continue;
        double X[NPE][DM], w_e[NPE];
        for (int a = 0; a < NPE; ++a)
            for (int i = 0; i < DM; ++i) X[a][i] = c->nodes[(int64_t)c->elems[(int64_t)e * NPE + a] * DM + i];
        body_weights_element<NPE, DM>(X, c->nGP, c->dN.data(), N, c->w.data(), w_e);
        for (int a = 0; a < NPE; ++a) we[(size_t)e * NPE + a] = w_e[a];
    }
    m.assign((size_t)c->nn, 0.0);
#pragma omp parallel for schedule(static)
    for (int32_t a = 0; a < c->nn; ++a) {
        double s = 0.0;
        for (int32_t k = c->ne_ptr[a]; k < c->ne_ptr[a + 1]; ++k) s += we[c->ne_idx[k]];
        m[a] = s;
    }
}
}  // namespace
extern "C" {

int femcy_bodyload_create(femcy_ctx* ctx, const double* N, int32_t nsel, const int32_t* sel_elems, int32_t* id_out) {
    CTX_OR_FAIL(ctx);
    std::vector<uint8_t> mask;
    FEMCY_TRY(check_bodyload_create(c, N, nsel, sel_elems, id_out, mask));
    const uint8_t* mk = sel_elems ? mask.data() : nullptr;
    BodyLoad bl;
    if (!dispatch_element(c->npe, c->dm, [&](auto npe, auto dm) { body_weights<npe(), dm()>(c, N, mk, bl.m); }))
        return no_kernel(c, "body-load");
    c->bodyloads.push_back(std::move(bl));
    *id_out = (int32_t)c->bodyloads.size() - 1;
    return FEMCY_OK;
}
int femcy_bodyload_weights(femcy_ctx* ctx, int32_t id, double* out) {
    CTX_OR_FAIL(ctx);
    FEMCY_OBJECT_OR_FAIL(bl, c->bodyloads, id, "body load");
    FEMCY_REQUIRE(out, TEXT_NULL_OUTPUT);
    std::copy(bl.m.begin(), bl.m.end(), out);
    return FEMCY_OK;
}
int femcy_bodyload_apply(femcy_ctx* ctx, int32_t id, const double* b, int rhs_vec, int32_t add) {
    CTX_OR_FAIL(ctx);
    FEMCY_TRY(check_bodyload_apply(c, id, b, rhs_vec));
    const BodyLoad& bl = c->bodyloads[id];
    double* rhs = c->vec[rhs_vec].data();
    const int dm = c->dm;
    // the product is rounded before it is added (two passes: no fused multiply-add), as on the device
    std::vector<double> f((size_t)c->n);
    for (int32_t a = 0; a < c->nn; ++a)
        for (int i = 0; i < dm; ++i) f[(size_t)a * dm + i] = bl.m[a] * b[i];
    if (add)
        for (int64_t i = 0; i < c->n; ++i) rhs[i] += f[i];
    else
        std::copy(f.begin(), f.end(), rhs);
    return FEMCY_OK;
}

// --------------------------------------------------------------------------------- thermal loads
}  // extern "C"
namespace {
// the element pass of the device's k_thermal_force (csrc/element_math.hpp: thermal_force_element), then the node sums in
// ascending (element, local node) order
template <int NPE, int DM>
void thermal_force(femcy_ctx* c, Thermal& th) {
    double s[DM][DM];
    for (int i = 0; i < DM; ++i)
        for (int j = 0; j < DM; ++j) s[i][j] = th.s[i * DM + j];
    std::vector<double> fe((size_t)c->ne * NPE * DM, 0.0);
#pragma omp parallel for schedule(static)
    for (int32_t e = 0; e < c->ne; ++e) {
        double X[NPE][DM], T[NPE], f_e[NPE * DM];
        for (int a = 0; a < NPE; ++a) {
            const int32_t nd = c->elems[(int64_t)e * NPE + a];
            for (int i = 0; i < DM; ++i) X[a][i] = c->nodes[(int64_t)nd * DM + i];
            T[a] = th.dT[nd];
        }
        thermal_force_element<NPE, DM>(X, T, c->nGP, c->dN.data(), th.N.data(), c->w.data(), s, f_e);
        for (int q = 0; q < NPE * DM; ++q) fe[(size_t)e * NPE * DM + q] = f_e[q];
    }
    th.f.assign((size_t)c->n, 0.0);
#pragma omp parallel for schedule(static)
    for (int32_t a = 0; a < c->nn; ++a)
        for (int i = 0; i < DM; ++i) {
            double acc = 0.0;
            for (int32_t k = c->ne_ptr[a]; k < c->ne_ptr[a + 1]; ++k) acc += fe[(size_t)c->ne_idx[k] * DM + i];
            th.f[(size_t)a * DM + i] = acc;
        }
}
}  // namespace
extern "C" {

int femcy_thermal_create(femcy_ctx* ctx, const double* N, double alpha, const double* dT, int32_t* id_out) {
    CTX_OR_FAIL(ctx);
    FEMCY_TRY(check_thermal_create(c, N, alpha, dT, id_out));
    Thermal th;
    th.N.assign(N, N + (size_t)c->nGP * c->npe);
    th.dT.assign(dT, dT + (size_t)c->nn);
    dispatch_dm(c->dm, [&](auto dm) {
        constexpr int DM = dm();
        double s[DM][DM];
        thermal_unit_stress<DM>(c->mat_kind, c->h_C, c->mat_params[1], s);
        for (int i = 0; i < DM * DM; ++i) th.s[i] = alpha * s[i / DM][i % DM];
    });
    if (!dispatch_element(c->npe, c->dm, [&](auto npe, auto dm) { thermal_force<npe(), dm()>(c, th); }))
        return no_kernel(c, "thermal-load");
    c->thermals.push_back(std::move(th));
    *id_out = (int32_t)c->thermals.size() - 1;
    return FEMCY_OK;
}
int femcy_thermal_force(femcy_ctx* ctx, int32_t id, double* out) {
    CTX_OR_FAIL(ctx);
    FEMCY_OBJECT_OR_FAIL(th, c->thermals, id, "thermal load");
    FEMCY_REQUIRE(out, TEXT_NULL_OUTPUT);
    std::copy(th.f.begin(), th.f.end(), out);
    return FEMCY_OK;
}
int femcy_thermal_apply(femcy_ctx* ctx, int32_t id, double scale, int rhs_vec, int32_t add) {
    CTX_OR_FAIL(ctx);
    VEC_OR_FAIL(rhs_vec);
    FEMCY_OBJECT_OR_FAIL(th, c->thermals, id, "thermal load");
    double* rhs = c->vec[rhs_vec].data();
    // the product is rounded before it is added (two passes: no fused multiply-add), as on the device
    std::vector<double> f((size_t)c->n);
    for (int64_t i = 0; i < c->n; ++i) f[i] = scale * th.f[i];
    if (add)
        for (int64_t i = 0; i < c->n; ++i) rhs[i] += f[i];
    else
        std::copy(f.begin(), f.end(), rhs);
    return FEMCY_OK;
}
int femcy_thermal_stress(femcy_ctx* ctx, int32_t id, double scale) {
    CTX_OR_FAIL(ctx);
    FEMCY_TRY(check_thermal_stress(c, id));
    const Thermal& th = c->thermals[id];
    c->post_small = false;
    const int64_t ngp = (int64_t)c->ne * c->nGP;
    const int npe = c->npe, nGP = c->nGP;
    dispatch_dm(c->dm, [&](auto dm) {
        constexpr int DM = dm();
        double s[DM][DM];
        for (int i = 0; i < DM * DM; ++i) s[i / DM][i % DM] = th.s[i];
#pragma omp parallel for schedule(static)
        for (int64_t t = 0; t < ngp; ++t) {
            const int64_t e = t / nGP;
            const int g = (int)(t - e * nGP);
            double tg = 0.0;
            for (int a = 0; a < npe; ++a) tg += th.N[(size_t)g * npe + a] * th.dT[c->elems[e * npe + a]];
            thermal_post_point<DM>(c->mat_kind, c->mat_params[1], s, scale * tg, c->sigma.data() + t * DM * DM,
                                   c->mises.data() + t);
        }
    });
    return FEMCY_OK;
}

// ------------------------------------------------------------------------------ implicit dynamics
}  // extern "C"
namespace {
// the two passes of the device's femcy_mass_create (csrc/element_math.hpp: mass_points_element, mass_pair): rho |det J| w at
// the mass rule's points per element, then every block of a row from the row's incident elements in ascending order
template <int NPE, int DM>
void mass_blocks(femcy_ctx* c, int32_t nq, const double* Nq, const double* dNq, const double* wq, double rho,
                 std::vector<double>& m) {
    std::vector<double> vq((size_t)c->ne * nq, 0.0);
#pragma omp parallel for schedule(static)
    for (int32_t e = 0; e < c->ne; ++e) {
        double X[NPE][DM];
        for (int a = 0; a < NPE; ++a)
            for (int i = 0; i < DM; ++i) X[a][i] = c->nodes[(int64_t)c->elems[(int64_t)e * NPE + a] * DM + i];
        mass_points_element<NPE, DM>(X, nq, dNq, wq, rho, vq.data() + (size_t)e * nq, 1);
    }
    m.assign(c->col.size(), 0.0);
#pragma omp parallel for schedule(static)
    for (int32_t a = 0; a < c->nn; ++a)
        for (int32_t k = c->ne_ptr[a]; k < c->ne_ptr[a + 1]; ++k) {
            const int32_t code = c->ne_idx[k];
            const int64_t e = code / NPE;
            const int la = code - (int32_t)e * NPE;
            for (int lb = 0; lb < NPE; ++lb)
                m[c->eslot[((int64_t)e * NPE + la) * NPE + lb]] += mass_pair(nq, NPE, Nq, la, lb, vq.data() + (size_t)e * nq);
        }
}
}  // namespace
extern "C" {

int femcy_mass_create(femcy_ctx* ctx, int32_t nq, const double* Nq, const double* dNq, const double* wq, double rho,
                      int32_t* id_out) {
    CTX_OR_FAIL(ctx);
    FEMCY_TRY(check_mass_rule(c, "femcy_mass_create", nq, Nq, dNq, wq, rho, id_out));
    Mass ms;
    if (!dispatch_element(c->npe, c->dm,
                          [&](auto npe, auto dm) { mass_blocks<npe(), dm()>(c, nq, Nq, dNq, wq, rho, ms.m); }))
        return no_kernel(c, "mass");
    c->masses.push_back(std::move(ms));
    *id_out = (int32_t)c->masses.size() - 1;
    return FEMCY_OK;
}
int femcy_mass_get(femcy_ctx* ctx, int32_t id, double* vals) {
    CTX_OR_FAIL(ctx);
    FEMCY_OBJECT_OR_FAIL(ms, c->masses, id, "mass object");
    FEMCY_REQUIRE(vals, TEXT_NULL_OUTPUT);
    int64_t w = 0;
    std::vector<std::pair<int32_t, int64_t>> order;
    for (int32_t a = 0; a < c->nn; ++a) {       // the block order of femcy_get_K_bsr
        order.clear();
        for (int64_t p = c->rowptr[a]; p < c->rowptr[a + 1]; ++p) order.push_back({c->col[p], p});
        std::sort(order.begin(), order.end());
        for (auto& pr : order) vals[w++] = ms.m[pr.second];
    }
    return FEMCY_OK;
}

int femcy_mass_apply(femcy_ctx* ctx, int32_t id, int x_vec, int y_vec, double scale, int32_t add) {
    CTX_OR_FAIL(ctx);
    FEMCY_TRY(check_mass_apply(c, id, x_vec, y_vec));
    const Mass& ms = c->masses[id];
    const double* x = c->vec[x_vec].data();
    double* y = c->vec[y_vec].data();
    const int dm = c->dm;
#pragma omp parallel for schedule(static)
    for (int32_t a = 0; a < c->nn; ++a) {
        double acc[3] = {0.0, 0.0, 0.0};
        for (int64_t p = c->rowptr[a]; p < c->rowptr[a + 1]; ++p) {
            const double* xv = x + (int64_t)c->col[p] * dm;
            for (int r = 0; r < dm; ++r) acc[r] += ms.m[p] * xv[r];
        }
        for (int r = 0; r < dm; ++r) {
            double& dst = y[(int64_t)a * dm + r];
            dst = add ? dst + scale * acc[r] : scale * acc[r];
        }
    }
    return FEMCY_OK;
}

int femcy_mass_add_to_K(femcy_ctx* ctx, int32_t id, double cc, int32_t overwrite) {
    CTX_OR_FAIL(ctx);
    FEMCY_TRY(check_mass_add_to_K(c, id, cc));
    const Mass& ms = c->masses[id];
    const int dm = c->dm, dd = dm * dm;
    // the product is rounded before it is added (two statements on a volatile: no fused multiply-add), as on the device
#pragma omp parallel for schedule(static)
    for (int64_t p = 0; p < (int64_t)c->col.size(); ++p) {
        volatile double v = cc * ms.m[p];
        double* blk = c->K.data() + p * dd;
        if (overwrite) {
            for (int q = 0; q < dd; ++q) blk[q] = (q % (dm + 1) == 0) ? v : 0.0;
        } else {
            for (int d = 0; d < dm; ++d) blk[d * (dm + 1)] += v;
        }
    }
    return FEMCY_OK;
}

int femcy_mass_kinetic_energy(femcy_ctx* ctx, int32_t id, int v_vec, double* out) {
    CTX_OR_FAIL(ctx);
    VEC_OR_FAIL(v_vec);
    FEMCY_OBJECT_OR_FAIL(ms, c->masses, id, "mass object");
    FEMCY_REQUIRE(out, TEXT_NULL_OUTPUT);
    const double* x = c->vec[v_vec].data();
    const int dm = c->dm;
    const int64_t nchunk = (c->nn + NODE_CHUNK - 1) / NODE_CHUNK;
    std::vector<double> part((size_t)nchunk, 0.0);      // sums of fixed chunks of rows, combined in order
#pragma omp parallel for schedule(static)
    for (int64_t ch = 0; ch < nchunk; ++ch) {
        double pd = 0.0;
        const int32_t a1 = (int32_t)std::min<int64_t>(c->nn, (ch + 1) * NODE_CHUNK);
        for (int32_t a = (int32_t)(ch * NODE_CHUNK); a < a1; ++a) {
            double acc[3] = {0.0, 0.0, 0.0};
            for (int64_t p = c->rowptr[a]; p < c->rowptr[a + 1]; ++p) {
                const double* xv = x + (int64_t)c->col[p] * dm;
                for (int r = 0; r < dm; ++r) acc[r] += ms.m[p] * xv[r];
            }
            for (int r = 0; r < dm; ++r) pd += x[(int64_t)a * dm + r] * acc[r];
        }
        part[ch] = pd;
    }
    double sum = 0.0;
    for (double v : part) sum += v;
    *out = 0.5 * sum;
    return FEMCY_OK;
}

int femcy_newmark_predict(femcy_ctx* ctx, int u_vec, int v_vec, int a_vec, int out_vec, double c0, double c1, double c2) {
    CTX_OR_FAIL(ctx);
    FEMCY_TRY(check_newmark_predict(c, u_vec, v_vec, a_vec, out_vec));
    const double *u = c->vec[u_vec].data(), *v = c->vec[v_vec].data(), *a = c->vec[a_vec].data();
    double* out = c->vec[out_vec].data();
#pragma omp parallel for schedule(static)
    for (int64_t i = 0; i < c->n; ++i) out[i] = c0 * u[i] + c1 * v[i] + c2 * a[i];
    return FEMCY_OK;
}

int femcy_newmark_update(femcy_ctx* ctx, int u_new_vec, int u_vec, int v_vec, int a_vec, double beta, double gamma,
                         double dt) {
    CTX_OR_FAIL(ctx);
    FEMCY_TRY(check_newmark_update(c, u_new_vec, u_vec, v_vec, a_vec, beta, gamma, dt));
    const double *un = c->vec[u_new_vec].data(), *u = c->vec[u_vec].data();
    double *v = c->vec[v_vec].data(), *a = c->vec[a_vec].data();
    const double b0 = 1.0 / (beta * dt * dt), b1 = 1.0 / (beta * dt), b2 = 1.0 / (2.0 * beta) - 1.0;
#pragma omp parallel for schedule(static)
    for (int64_t i = 0; i < c->n; ++i) newmark_update_entry(un[i], u[i], v[i], a[i], b0, b1, b2, dt, gamma);
    return FEMCY_OK;
}

// ------------------------------------------------------------------------------ explicit dynamics
}  // extern "C"
namespace {
// out[0..w) = the sum of node a's incident rows of src (w doubles each, w <= 3) in the order of the device's half-wavefront
// gather (csrc/node_gather.hpp): partial sums of every 32nd incident row, combined by half_wave_tree
void node_sum(const femcy_ctx* c, int32_t a, const double* src, int w, double* out) {
    double p[3][32] = {{0.0}};
    const int32_t k0 = c->ne_ptr[a];
    for (int32_t k = k0; k < c->ne_ptr[a + 1]; ++k)
        for (int i = 0; i < w; ++i) p[i][(k - k0) & 31] += src[(int64_t)c->ne_idx[k] * w + i];
    for (int i = 0; i < w; ++i) out[i] = half_wave_tree(p[i]);
}

// the two passes of the device's femcy_lumped_mass_create (csrc/element_math.hpp: lumped_element, then node_sum)
template <int NPE, int DM>
void lumped_mass(femcy_ctx* c, int32_t nq, const double* Nq, const double* dNq, const double* wq, double rho,
                 std::vector<double>& m, std::vector<double>& me) {
    me.assign((size_t)c->ne * NPE, 0.0);
#pragma omp parallel for schedule(static)
    for (int32_t e = 0; e < c->ne; ++e) {
        double X[NPE][DM], w[NPE];
        for (int a = 0; a < NPE; ++a)
            for (int i = 0; i < DM; ++i) X[a][i] = c->nodes[(int64_t)c->elems[(int64_t)e * NPE + a] * DM + i];
        lumped_element<NPE, DM>(X, nq, Nq, dNq, wq, rho, w);
        for (int a = 0; a < NPE; ++a) me[(size_t)e * NPE + a] = w[a];
    }
    m.assign((size_t)c->nn, 0.0);
#pragma omp parallel for schedule(static)
    for (int32_t a = 0; a < c->nn; ++a) node_sum(c, a, me.data(), 1, &m[a]);
}

// the device's node pass (kernels_explicit.hip: explicit_node_pass) on the host: node sums of fe in the order of its gather,
// then explicit_kick / explicit_drift; what mode and st say is with ExplicitStep in csrc/element_math.hpp
// With motion (t: the time of the state being kicked, t_drift: the time the drift reaches) a held and moved DOF takes
// explicit_moved instead of the kick, as the device's motion policy does.
// With the energy balance running (ex.energy_on) every DOF's addends of the step that led to the state (csrc/element_math.hpp:
// explicit_energy_free / _moved, the device's functions) go to the node's row of ex.ew and are then added to the four sums
// node by node: one order, whatever the number of threads.  The forces of the state stay in ex.efint / ex.ealpha.
// With rigid walls (ex.walls.n) the kick is explicit_kick_wall at x = X + u of the node, u before any of its DOFs drifts.
template <int DM>
void explicit_node(femcy_ctx* c, Explicit& ex, const double* f, const ExplicitStep& st, int mode, double t = 0.0,
                   double t_drift = 0.0) {
    const int dm = DM;
    const bool wall = ex.walls.n != 0;
    const MotionTables& mo = ex.motion;
    const bool moved = ex.moved(), energy = ex.energy_on, start = mode == XN_START, count = !start && st.hh != 0.0;
    const double* mass = c->lumped_masses[ex.lumped].m.data();
    double *u = c->vec[FEMCY_VEC_DOF].data(), *v = c->vec[FEMCY_VEC_VEL].data(), *acc = c->vec[FEMCY_VEC_ACC].data();
#pragma omp parallel for schedule(static)
    for (int32_t a = 0; a < c->nn; ++a) {
        double fint[3], wn[4] = {0.0, 0.0, 0.0, 0.0};
        node_sum(c, a, c->fe.data(), dm, fint);
        double x[DM];
        for (int i = 0; i < dm; ++i) x[i] = c->nodes[(int64_t)a * dm + i] + u[(int64_t)a * dm + i];
        for (int i = 0; i < dm; ++i) {
            const int64_t q = (int64_t)a * dm + i;
            if (const int32_t s = moved ? mo.slot[q] : -1; s >= 0 && ex.minv[q] == 0.0) {
                const double a_prev = acc[q];
                explicit_moved(mo.amp[mo.curve[s]], mo.val[s], t, t_drift, mode == XN_START, st.drift, u[q], v[q], acc[q]);
                if (energy) {
                    if (count) {
                        double w[4];
                        explicit_energy_moved(mo.amp[mo.curve[s]], mo.val[s], ex.en_t, t, mass[a], ex.en_s, st.s, f[q],
                                              ex.efint[q], fint[i], a_prev, acc[q], w);
                        for (int k = 0; k < 4; ++k) wn[k] += w[k];
                    }
                    ex.efint[q] = fint[i];
                    ex.ealpha[q] = 0.0;
                }
                continue;
            }
            // at the start vec[ACC] is not read; vec[VEL] only by the damped kick (v_{-1/2} := v_0)
            double vi = mode != XN_START || st.alpha != 0.0 ? v[q] : 0.0, ai = mode != XN_START ? acc[q] : 0.0;
            if (energy) {
                double w[4], ga;
                explicit_energy_free(ex.minv[q], mass[a], ex.en_s, st.s, f[q], ex.efint[q], fint[i], ex.ealpha[q], st.alpha, vi,
                                     ai, st.hh, !count, w, ga);
                for (int k = 0; k < 4; ++k) wn[k] += w[k];
                ex.efint[q] = fint[i];
                ex.ealpha[q] = ga;
            }
            if (wall)
                explicit_kick_wall<DM>(ex.minv[q], st.s, f[q], fint[i], st.hh, st.alpha, ex.walls, x, i, vi, ai);
            else if (st.alpha != 0.0)
                explicit_kick_damped(ex.minv[q], st.s, f[q], fint[i], st.hh, st.alpha, vi, ai);
            else
                explicit_kick(ex.minv[q], st.s, f[q], fint[i], st.hh, vi, ai);
            acc[q] = ai;
            if (mode == XN_START) continue;
            v[q] = vi;
            if (st.drift) u[q] = explicit_drift(u[q], vi, ai, st.h, st.h2h);
        }
        if (energy && count)
            for (int k = 0; k < 4; ++k) ex.ew[(size_t)a * 4 + k] = wn[k];
    }
    if (!energy) return;
    if (start) std::fill(ex.en, ex.en + 4, 0.0);
    if (count) {
        double step[4] = {0.0, 0.0, 0.0, 0.0};
        for (int32_t a = 0; a < c->nn; ++a)
            for (int k = 0; k < 4; ++k) step[k] += ex.ew[(size_t)a * 4 + k];
        for (int k = 0; k < 4; ++k) ex.en[k] += step[k];
    }
    ex.en_s = st.s;
    ex.en_t = t;
}
void explicit_node_any(femcy_ctx* c, Explicit& ex, const double* f, const ExplicitStep& st, int mode, double t = 0.0,
                       double t_drift = 0.0) {
    if (c->dm == 2)
        explicit_node<2>(c, ex, f, st, mode, t, t_drift);
    else
        explicit_node<3>(c, ex, f, st, mode, t, t_drift);
}

// max_e omega_e^2 at u (csrc/element_math.hpp: explicit_bound_element); a NaN counts as infinity
template <int NPE, int DM>
void element_bound(femcy_ctx* c, const double* u, const double* me_all, double s_C, const HostDamping* hd, double kappa,
                   double& out) {
    double best = 0.0;
#pragma omp parallel for schedule(static) reduction(max : best)
    for (int32_t e = 0; e < c->ne; ++e) {
        double X[NPE][DM], U[NPE][DM], Vh[NPE][DM], me[NPE], g, w2;
        for (int a = 0; a < NPE; ++a) {
            const int32_t nd = c->elems[(int64_t)e * NPE + a];
            for (int i = 0; i < DM; ++i) {
                X[a][i] = c->nodes[(int64_t)nd * DM + i];
                U[a][i] = u[(int64_t)nd * DM + i];
                if (hd) {
                    const double vi = hd->v[(int64_t)nd * DM + i];
                    Vh[a][i] = hd->a ? explicit_vhalf(vi, hd->a[(int64_t)nd * DM + i], hd->hh) : vi;
                }
            }
            me[a] = me_all[(int64_t)e * NPE + a];
        }
        if (hd)
            explicit_bound_element_damped<NPE, DM>(X, U, Vh, hd->d, c->nGP, c->dN.data(), c->w.data(), c->mat_kind, c->h_C,
                                                   c->mat_params[0], c->mat_params[1], me, s_C, g, w2, kappa);
        else
            explicit_bound_element<NPE, DM>(X, U, c->nGP, c->dN.data(), c->w.data(), c->mat_kind, c->h_C, c->mat_params[0],
                                            c->mat_params[1], me, s_C, g, w2, kappa);
        if (w2 != w2) w2 = INFINITY;
        best = std::fmax(best, w2);
    }
    out = best;
}
// what the damped passes of an integrator take (the device's damping_of): start: v_{-1/2} := v_0, vec[ACC] is not read
HostDamping damping_of(const femcy_ctx* c, const Explicit& ex, double h, bool start) {
    return {c->vec[FEMCY_VEC_VEL].data(), start ? nullptr : c->vec[FEMCY_VEC_ACC].data(), 0.5 * h,
            {ex.alpha, ex.b1, ex.b2, ex.Md, c->lumped_masses[ex.lumped].rho}};
}
int element_bound_any(femcy_ctx* c, const Explicit& ex, const double* u, double s_C, double* w2, const HostDamping* hd = nullptr) {
    const double* me = c->lumped_masses[ex.lumped].me.data();
    if (!dispatch_element(c->npe, c->dm,
                          [&](auto npe, auto dm) { element_bound<npe(), dm()>(c, u, me, s_C, hd, ex.wall_kappa(), *w2); }))
        return no_kernel(c, "element-bound");
    return FEMCY_OK;
}

// a workgroup's 256 values -> one, in the order of the device's block_reduce (kernels_explicit.hip): xor tree inside each
// wavefront of 64, then the four wave results in ascending order
double block_reduce_sum(double (&x)[256]) {
    double r = 0.0;
    for (int w = 0; w < 4; ++w) {
        double* y = x + w * 64;
        for (int o = 32; o > 0; o >>= 1)
            for (int l = 0; l < o; ++l) y[l] += y[l + o];
        r = w ? r + y[0] : y[0];
    }
    return r;
}

// the device's two sum reductions over n items (k_explicit_energy / k_mass_total, then k_explicit_final<false>): 256 strided
// partial sums per workgroup, at most 1024 workgroups, then one workgroup; add(acc, i) folds item i into a thread's sum
template <class Add>
double device_order_sum(int64_t n, Add add) {
    const int64_t g = std::max<int64_t>(1, std::min<int64_t>((n + 255) / 256, 1024));
    std::vector<double> part((size_t)g);
#pragma omp parallel for schedule(static)
    for (int64_t b = 0; b < g; ++b) {
        double x[256];
        for (int t = 0; t < 256; ++t) {
            double acc = 0.0;
            for (int64_t a = b * 256 + t; a < n; a += g * 256) acc = add(acc, a);
            x[t] = acc;
        }
        part[(size_t)b] = block_reduce_sum(x);
    }
    double x[256];
    for (int t = 0; t < 256; ++t) {
        double acc = 0.0;
        for (int64_t i = t; i < g; i += 256) acc += part[(size_t)i];
        x[t] = acc;
    }
    return block_reduce_sum(x);
}

// the device's k_mass_scale_factors: fac[e] = k_e from omega_e^2 at u = 0 with the element's current shares
// (csrc/element_math.hpp: explicit_bound_element, mass_scale_factor); -> max omega_e^2, max k_e (each with what is not a
// usable number counted as infinity), the number of k_e != 1.  fac null: the measuring pass, max omega_e^2 alone
template <int NPE, int DM>
void mass_scale_factors(femcy_ctx* c, const double* me_all, double s_C, double w2max, double factor, double tau, int type,
                        double* fac, double (&res)[3]) {
    double best = 0.0, kbest = 0.0;
    int64_t scaled = 0;
#pragma omp parallel for schedule(static) reduction(max : best, kbest) reduction(+ : scaled)
    for (int32_t e = 0; e < c->ne; ++e) {
        double X[NPE][DM], U[NPE][DM], me[NPE], g, w2;
        for (int a = 0; a < NPE; ++a) {
            const int32_t nd = c->elems[(int64_t)e * NPE + a];
            for (int i = 0; i < DM; ++i) {
                X[a][i] = c->nodes[(int64_t)nd * DM + i];
                U[a][i] = 0.0;
            }
            me[a] = me_all[(int64_t)e * NPE + a];
        }
        explicit_bound_element<NPE, DM>(X, U, c->nGP, c->dN.data(), c->w.data(), c->mat_kind, c->h_C, c->mat_params[0],
                                        c->mat_params[1], me, s_C, g, w2);
        best = std::fmax(best, mass_scale_nan_to_inf(w2));
        if (!fac) continue;
        const double k = mass_scale_factor(w2, w2max, factor, tau, type);
        fac[e] = k;
        kbest = std::fmax(kbest, mass_scale_bad_to_inf(k));
        scaled += k != 1.0;
    }
    res[0] = best;
    res[1] = kbest;
    res[2] = (double)scaled;
}

// the device's k_explicit_place: u, v, a (what: MOVE_*) of the moved DOFs at time t
void place_moved(femcy_ctx* c, const Explicit& ex, double t, int what) {
    const MotionTables& mo = ex.motion;
    double *u = c->vec[FEMCY_VEC_DOF].data(), *v = c->vec[FEMCY_VEC_VEL].data(), *a = c->vec[FEMCY_VEC_ACC].data();
    for (size_t k = 0; k < mo.dof.size(); ++k) {
        const int32_t i = mo.dof[k];
        explicit_place(mo.amp[mo.curve[k]], mo.val[k], t, what, u[i], v[i], a[i]);
    }
}

// nsteps steps from a started state, as the device's explicit_steps runs them: the first drift, then per step the element
// pass and the node pass.  A fixed run (clock null) takes dt and the load scale scale0 + k dscale from the caller; an
// automatic one bounds the element frequencies and ticks its clock between the two passes, which then gives both.
int explicit_steps(femcy_ctx* c, Explicit& ex, ExplicitClock* clock, int rhs_vec, int32_t nsteps, double dt,
                   double scale0, double dscale) {
    if (nsteps == 0) return FEMCY_OK;
    double* u = c->vec[FEMCY_VEC_DOF].data();
    const double *v = c->vec[FEMCY_VEC_VEL].data(), *a = c->vec[FEMCY_VEC_ACC].data();
    auto time_of = [&](int32_t k) { return explicit_fixed_time(ex.t_base, ex.n_base, ex.n_done + k, dt); };
    if (const double h = clock ? clock->h_next : dt; h != 0.0) {
        const double h2h = 0.5 * h * h;
#pragma omp parallel for schedule(static)
        for (int64_t i = 0; i < c->n; ++i) u[i] = explicit_drift(u[i], v[i], a[i], h, h2h);
        place_moved(c, ex, clock ? clock->t_next : time_of(1), MOVE_U);      // a moved u is set, not integrated
    }
    for (int32_t k = 1; k <= nsteps; ++k) {
        const bool last = k == nsteps;      // F and sigma of the last state stay behind for post-processing
        const int mode = last ? XN_KICK : XN_KICK_DRIFT;
        // the increment of the drift that led to u: the clock's h_next until it ticks
        const HostDamping hd = damping_of(c, ex, clock ? clock->h_next : dt, false);
        geom(c, u, last ? (GEOM_DSDX | GEOM_F | GEOM_SIGMA | GEOM_FE) : (GEOM_DSDX | GEOM_FE), ex.bulk() ? &hd : nullptr);
        ExplicitStep st;
        if (clock) {
            double w2 = 0.0;
            int rc = element_bound_any(c, ex, u, clock->s_C, &w2, ex.damped() ? &hd : nullptr);
            if (rc) return rc;
            explicit_clock_tick(*clock, w2);
            if (!explicit_step_clock(*clock, mode, st, ex.alpha)) continue;
        } else {
            st = explicit_step_fixed(scale0 + k * dscale, dt, mode, ex.alpha);
        }
        explicit_node_any(c, ex, c->vec[rhs_vec].data(), st, mode, clock ? clock->t : time_of(k),
                      clock ? clock->t_next : time_of(k + 1));
    }
    return FEMCY_OK;
}
}  // namespace
extern "C" {

int femcy_lumped_mass_create(femcy_ctx* ctx, int32_t nq, const double* Nq, const double* dNq, const double* wq, double rho,
                             int32_t* id_out) {
    CTX_OR_FAIL(ctx);
    FEMCY_TRY(check_mass_rule(c, "femcy_lumped_mass_create", nq, Nq, dNq, wq, rho, id_out));
    LumpedMass lm;
    lm.rho = rho;
    if (!dispatch_element(c->npe, c->dm,
                          [&](auto npe, auto dm) { lumped_mass<npe(), dm()>(c, nq, Nq, dNq, wq, rho, lm.m, lm.me); }))
        return no_kernel(c, "lumped-mass");
    c->lumped_masses.push_back(std::move(lm));
    *id_out = (int32_t)c->lumped_masses.size() - 1;
    return FEMCY_OK;
}
int femcy_lumped_mass_get(femcy_ctx* ctx, int32_t id, double* out) {
    CTX_OR_FAIL(ctx);
    FEMCY_OBJECT_OR_FAIL(lm, c->lumped_masses, id, "lumped mass");
    FEMCY_REQUIRE(out, TEXT_NULL_OUTPUT);
    std::copy(lm.m.begin(), lm.m.end(), out);
    return FEMCY_OK;
}

// the device's femcy_lumped_mass_scale: the total mass, the factors (FEMCY_MS_UNIFORM: the maximum first), and only once
// omega_e^2 and every factor are finite and positive the shares, the node sums and the total again
int femcy_lumped_mass_scale(femcy_ctx* ctx, int32_t lumped_id, double s_C, double factor, double dt, int32_t type,
                            double* mass_before, double* mass_after, int64_t* n_scaled, double* factor_max) {
    CTX_OR_FAIL(ctx);
    READY_OR_FAIL();
    FEMCY_TRY(check_lumped_mass_scale(c, lumped_id, s_C, factor, dt, type, mass_before, mass_after, n_scaled, factor_max));
    LumpedMass& lm = c->lumped_masses[lumped_id];
    const double sc = dt != 0.0 ? s_C : 1.0;      // without dt the estimate serves the test for broken elements alone
    std::vector<double> fac((size_t)c->ne);
    double res[3] = {0.0, 0.0, 0.0}, w2max = 0.0;
    auto pass = [&](double* out) {
        return dispatch_element(c->npe, c->dm, [&](auto npe, auto dm) {
            mass_scale_factors<npe(), dm()>(c, lm.me.data(), sc, w2max, factor, dt, type, out, res);
        });
    };
    const double m0 = device_order_sum(c->nn, [&](double acc, int64_t a) { return acc + lm.m[(size_t)a]; });
    if (dt != 0.0 && type == FEMCY_MS_UNIFORM) {
        if (!pass(nullptr)) return no_kernel(c, "mass-scaling");
        w2max = res[0];
    }
    if (std::isfinite(w2max) && !pass(fac.data())) return no_kernel(c, "mass-scaling");
    if (!std::isfinite(w2max) || !std::isfinite(res[0]) || !std::isfinite(res[1])) {
        set_error("femcy_lumped_mass_scale: an element frequency or a factor is not finite and positive (max omega_e^2 = %g, "
                  "max factor = %g): a broken element; the lumped mass is unchanged", res[0], res[1]);
        return FEMCY_ENUMERIC;
    }
    if (lm.scale.empty()) lm.scale.assign((size_t)c->ne, 1.0);
    const int npe = c->npe;
#pragma omp parallel for schedule(static)
    for (int32_t e = 0; e < c->ne; ++e) {
        for (int a = 0; a < npe; ++a) lm.me[(size_t)e * npe + a] *= fac[(size_t)e];
        lm.scale[(size_t)e] *= fac[(size_t)e];
    }
#pragma omp parallel for schedule(static)
    for (int32_t a = 0; a < c->nn; ++a) node_sum(c, a, lm.me.data(), 1, &lm.m[a]);
    *mass_before = m0;
    *mass_after = device_order_sum(c->nn, [&](double acc, int64_t a) { return acc + lm.m[(size_t)a]; });
    *n_scaled = (int64_t)res[2];
    *factor_max = res[1];
    return FEMCY_OK;
}
int femcy_lumped_mass_get_scaling(femcy_ctx* ctx, int32_t lumped_id, double* out) {
    CTX_OR_FAIL(ctx);
    FEMCY_OBJECT_OR_FAIL(lm, c->lumped_masses, lumped_id, "lumped mass");
    FEMCY_REQUIRE(out, TEXT_NULL_OUTPUT);
    if (lm.scale.empty())
        std::fill(out, out + c->ne, 1.0);
    else
        std::copy(lm.scale.begin(), lm.scale.end(), out);
    return FEMCY_OK;
}

int femcy_explicit_create(femcy_ctx* ctx, int32_t lumped_id, int32_t ndofsets, const int32_t* dofset_ids, int32_t* id_out) {
    CTX_OR_FAIL(ctx);
    FEMCY_TRY(check_explicit_create(c, lumped_id, ndofsets, dofset_ids, id_out));
    const LumpedMass& lm = c->lumped_masses[lumped_id];
    Explicit ex;
    ex.lumped = lumped_id;
    ex.held.assign(dofset_ids, dofset_ids + ndofsets);
    ex.minv.resize((size_t)c->n);
    for (int64_t i = 0; i < c->n; ++i) ex.minv[i] = 1.0 / lm.m[i / c->dm];
    for (int32_t k = 0; k < ndofsets; ++k)
        for (int32_t dof : c->dofsets[dofset_ids[k]].dofs) ex.minv[dof] = 0.0;
    c->explicits.push_back(std::move(ex));
    *id_out = (int32_t)c->explicits.size() - 1;
    return FEMCY_OK;
}

int femcy_explicit_start(femcy_ctx* ctx, int32_t id, int rhs_vec, double scale) {
    CTX_OR_FAIL(ctx);
    READY_OR_FAIL();
    FEMCY_TRY(check_explicit_start(c, id, rhs_vec, scale));
    Explicit& ex = c->explicits[id];
    ex.n_done = ex.n_base = 0;                      // the clock of a fixed run: t = 0
    ex.t_base = ex.dt_prev = 0.0;
    place_moved(c, ex, 0.0, MOVE_U | MOVE_V | MOVE_A);
    const HostDamping hd = damping_of(c, ex, 0.0, true);
    geom(c, c->vec[FEMCY_VEC_DOF].data(), GEOM_DSDX | GEOM_F | GEOM_SIGMA | GEOM_FE, ex.bulk() ? &hd : nullptr);
    ex.energy_on = ex.energy_want;                  // the start zeroes the sums and records the forces of state 0
    explicit_node_any(c, ex, c->vec[rhs_vec].data(), explicit_step_fixed(scale, 0.0, XN_START, ex.alpha), XN_START);
    return FEMCY_OK;
}

int femcy_explicit_set_damping(femcy_ctx* ctx, int32_t id, double alpha, double b1, double b2, double M_d) {
    CTX_OR_FAIL(ctx);
    FEMCY_TRY(check_explicit_set_damping(c, id, alpha, b1, b2, M_d));
    Explicit& ex = c->explicits[id];
    ex.alpha = alpha;
    ex.b1 = b1;
    ex.b2 = b2;
    ex.Md = M_d;
    return FEMCY_OK;
}

int femcy_explicit_advance(femcy_ctx* ctx, int32_t id, int rhs_vec, int32_t nsteps, double dt, double scale0, double dscale) {
    CTX_OR_FAIL(ctx);
    READY_OR_FAIL();
    FEMCY_TRY(check_explicit_advance(c, id, rhs_vec, nsteps, dt, scale0, dscale));
    Explicit& ex = c->explicits[id];
    if (nsteps && dt != ex.dt_prev) {               // another increment: the clock counts on from the time it has reached
        ex.t_base = explicit_fixed_time(ex.t_base, ex.n_base, ex.n_done, ex.dt_prev);
        ex.n_base = ex.n_done;
        ex.dt_prev = dt;
    }
    const int rc = explicit_steps(c, ex, nullptr, rhs_vec, nsteps, dt, scale0, dscale);
    if (!rc) ex.n_done += nsteps;
    return rc;
}

int femcy_amplitude_create(femcy_ctx* ctx, int32_t kind, int32_t npts, const double* t, const double* A, int32_t* id_out) {
    CTX_OR_FAIL(ctx);
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

int femcy_explicit_set_motion(femcy_ctx* ctx, int32_t id, int32_t nsets, const int32_t* dofset_ids, const double* values,
                              const int32_t* amplitude_ids) {
    CTX_OR_FAIL(ctx);
    FEMCY_TRY(check_explicit_set_motion(c, id, nsets, dofset_ids, values, amplitude_ids));
    std::vector<std::vector<int32_t>> sets((size_t)nsets);
    for (int32_t k = 0; k < nsets; ++k) sets[k] = c->dofsets[dofset_ids[k]].dofs;
    c->explicits[id].motion = motion_tables(c->n, sets, values, amplitude_ids, c->amplitudes);
    return FEMCY_OK;
}

int femcy_explicit_energy_enable(femcy_ctx* ctx, int32_t id, int32_t on) {
    CTX_OR_FAIL(ctx);
    FEMCY_TRY(check_object(c->explicits, id, "explicit integrator"));
    Explicit& ex = c->explicits[id];
    ex.energy_want = on != 0;
    if (!on) {
        ex.energy_on = false;
        return FEMCY_OK;
    }
    if (ex.efint.empty()) {                         // a running balance keeps what it holds
        ex.efint.assign((size_t)c->n, 0.0);
        ex.ealpha.assign((size_t)c->n, 0.0);
        ex.ew.assign((size_t)c->nn * 4, 0.0);
    }
    return FEMCY_OK;
}

int femcy_explicit_energy_get(femcy_ctx* ctx, int32_t id, double* out) {
    CTX_OR_FAIL(ctx);
    FEMCY_TRY(check_explicit_energy_get(c, id, out));
    std::copy(c->explicits[id].en, c->explicits[id].en + 4, out);
    return FEMCY_OK;
}

int femcy_explicit_set_wall(femcy_ctx* ctx, int32_t id, int32_t nwalls, const double* point, const double* normal,
                            const double* kappa) {
    CTX_OR_FAIL(ctx);
    ExplicitWalls w{};
    FEMCY_TRY(check_explicit_set_wall(c, id, nwalls, point, normal, kappa, w));
    c->explicits[id].walls = w;
    return FEMCY_OK;
}

}  // extern "C"
namespace {
// the device's k_explicit_wall and its four final reductions: the terms of wall_node_terms in the order of device_order_sum,
// the maximum as it is
template <int DM>
void wall_get(const femcy_ctx* c, const Explicit& ex, int k, double* out) {
    const double* m = c->lumped_masses[ex.lumped].m.data();
    const double* u = c->vec[FEMCY_VEC_DOF].data();
    auto term = [&](int64_t a, int j) {
        double x[DM], t[4];
        bool any_free = false;
        for (int i = 0; i < DM; ++i) {
            x[i] = c->nodes[a * DM + i] + u[a * DM + i];
            any_free = any_free || ex.minv[a * DM + i] != 0.0;
        }
        wall_node_terms<DM>(ex.walls, k, x, m[a], any_free, t);
        return t[j];
    };
    for (int j = 0; j < 3; ++j) out[j] = device_order_sum(c->nn, [&](double acc, int64_t a) { return acc + term(a, j); });
    double p = 0.0;
    for (int64_t a = 0; a < c->nn; ++a) p = std::fmax(p, term(a, 3));
    out[3] = p;
}
}  // namespace
extern "C" {

int femcy_explicit_wall_get(femcy_ctx* ctx, int32_t id, int32_t wall, double* out) {
    CTX_OR_FAIL(ctx);
    FEMCY_TRY(check_explicit_wall_get(c, id, wall, out));
    if (c->dm == 2)
        wall_get<2>(c, c->explicits[id], wall, out);
    else
        wall_get<3>(c, c->explicits[id], wall, out);
    return FEMCY_OK;
}

int femcy_explicit_kinetic_energy(femcy_ctx* ctx, int32_t id, int v_vec, double* out) {
    CTX_OR_FAIL(ctx);
    FEMCY_OBJECT_OR_FAIL(ex, c->explicits, id, "explicit integrator");
    VEC_OR_FAIL(v_vec);
    FEMCY_REQUIRE(out, TEXT_NULL_OUTPUT);
    const double* m = c->lumped_masses[ex.lumped].m.data();
    const double* v = c->vec[v_vec].data();
    const int dm = c->dm;
    // the device's two reductions: 256 strided partial sums per workgroup, at most 1024 workgroups, then one workgroup
    const int64_t g = std::max<int64_t>(1, std::min<int64_t>(((int64_t)c->nn + 255) / 256, 1024));
    std::vector<double> part((size_t)g);
#pragma omp parallel for schedule(static)
    for (int64_t b = 0; b < g; ++b) {
        double x[256];
        for (int t = 0; t < 256; ++t) {
            double acc = 0.0;
            for (int64_t a = b * 256 + t; a < c->nn; a += g * 256) {
                double vv = v[a * dm] * v[a * dm];
                for (int i = 1; i < dm; ++i) vv = std::fma(v[a * dm + i], v[a * dm + i], vv);
                acc = std::fma(m[a], vv, acc);
            }
            x[t] = acc;
        }
        part[(size_t)b] = block_reduce_sum(x);
    }
    double x[256];
    for (int t = 0; t < 256; ++t) {
        double acc = 0.0;
        for (int64_t i = t; i < g; i += 256) acc += part[(size_t)i];
        x[t] = acc;
    }
    *out = 0.5 * block_reduce_sum(x);
    return FEMCY_OK;
}

int femcy_explicit_stable_dt(femcy_ctx* ctx, int32_t id, double* dt, double* omega_bound) {
    CTX_OR_FAIL(ctx);
    FEMCY_OBJECT_OR_FAIL(ex, c->explicits, id, "explicit integrator");
    FEMCY_REQUIRE(dt && omega_bound, TEXT_NULL_OUTPUT);
    FEMCY_REQUIRE(c->have_pattern && c->have_K, TEXT_ASSEMBLE_FIRST);
    const int dm = c->dm, dd = dm * dm;
    double best = 0.0;
    for (int32_t a = 0; a < c->nn; ++a) {      // blocks in storage order, entries of a scalar row in ascending column order
        double sum[3] = {0.0, 0.0, 0.0};
        for (int64_t p = c->rowptr[a]; p < c->rowptr[a + 1]; ++p)
            for (int k = 0; k < dd; ++k) sum[k / dm] += std::fabs(c->K[p * dd + k]);
        for (int r = 0; r < dm; ++r) {
            const double mi = ex.minv[(int64_t)a * dm + r];
            if (mi != 0.0) best = std::fmax(best, nan_to_inf_abs(sum[r] * mi));
        }
    }
    *omega_bound = std::sqrt(best);
    *dt = 2.0 / *omega_bound;
    return FEMCY_OK;
}

int femcy_explicit_element_bound(femcy_ctx* ctx, int32_t id, int u_vec, double s_C, double* omega) {
    CTX_OR_FAIL(ctx);
    READY_OR_FAIL();
    FEMCY_TRY(check_explicit_element_bound(c, id, u_vec, s_C, omega));
    double w2 = 0.0;
    const Explicit& ex = c->explicits[id];
    const HostDamping hd = damping_of(c, ex, 0.0, true);      // v_{1/2} := vec[VEL]
    int rc = element_bound_any(c, ex, c->vec[u_vec].data(), s_C, &w2, ex.damped() ? &hd : nullptr);
    if (rc) return rc;
    *omega = std::sqrt(w2);
    return FEMCY_OK;
}

int femcy_explicit_auto_begin(femcy_ctx* ctx, int32_t id, int rhs_vec, double s_C, double scale_factor, double T,
                              int32_t ramp) {
    CTX_OR_FAIL(ctx);
    READY_OR_FAIL();
    FEMCY_TRY(check_explicit_auto_begin(c, id, rhs_vec, s_C, scale_factor, T));
    Explicit& exm = c->explicits[id];
    const double* u = c->vec[FEMCY_VEC_DOF].data();
    double w2 = 0.0;
    place_moved(c, exm, 0.0, MOVE_U | MOVE_V | MOVE_A);
    const HostDamping hd = damping_of(c, exm, 0.0, true);      // v_{-1/2} := v_0, vec[ACC] is not read
    int rc = element_bound_any(c, exm, u, s_C, &w2, exm.damped() ? &hd : nullptr);
    if (rc) return rc;
    exm.clock = ExplicitClock{};
    exm.clock.T = T;
    exm.clock.sf = scale_factor;
    exm.clock.s_C = s_C;
    exm.clock.h_min = INFINITY;
    exm.clock.ramp = ramp ? 1 : 0;
    geom(c, u, GEOM_DSDX | GEOM_F | GEOM_SIGMA | GEOM_FE, exm.bulk() ? &hd : nullptr);
    explicit_clock_tick(exm.clock, w2);                        // t = 0, the first h
    ExplicitStep st;
    explicit_step_clock(exm.clock, XN_START, st, exm.alpha);   // always something to do at the start
    exm.energy_on = exm.energy_want;                           // as femcy_explicit_start
    explicit_node_any(c, exm, c->vec[rhs_vec].data(), st, XN_START);
    exm.auto_begun = true;
    return FEMCY_OK;
}

int femcy_explicit_auto_advance(femcy_ctx* ctx, int32_t id, int rhs_vec, int32_t nsteps) {
    CTX_OR_FAIL(ctx);
    READY_OR_FAIL();
    FEMCY_TRY(check_explicit_auto_advance(c, id, rhs_vec, nsteps));
    return explicit_steps(c, c->explicits[id], &c->explicits[id].clock, rhs_vec, nsteps, 0.0, 0.0, 0.0);
}

int femcy_explicit_auto_state(femcy_ctx* ctx, int32_t id, double* t, double* h_last, double* h_min, int64_t* steps_done) {
    CTX_OR_FAIL(ctx);
    FEMCY_TRY(check_explicit_auto_state(c, id, t, h_last, h_min, steps_done));
    const Explicit& ex = c->explicits[id];
    *t = ex.clock.t;
    *h_last = ex.clock.h_last;
    *h_min = ex.clock.steps ? ex.clock.h_min : 0.0;
    *steps_done = ex.clock.steps;
    return FEMCY_OK;
}

int femcy_spmv(femcy_ctx* ctx, int x_vec, int y_vec) {
    CTX_OR_FAIL(ctx);
    FEMCY_TRY(check_two_vectors(c, x_vec, y_vec, TEXT_SPMV_IN_PLACE));
    spmv(c, c->vec[x_vec].data(), c->vec[y_vec].data(), nullptr);
    return FEMCY_OK;
}

int femcy_direct_plan(femcy_ctx* ctx, femcy_direct_info* info) {
    CTX_OR_FAIL(ctx);
    FEMCY_TRY(check_direct_plan(c, info));
    if (!c->have_band_order) {
        c->band_order = band_order_rcm(c->nn, c->ne, c->npe, c->elems.data());
        c->have_band_order = true;
    }
    *info = femcy_direct_info{};
    const int64_t bw = ((int64_t)c->band_order.half_band_nodes + 1) * c->dm - 1;
    info->n = c->n;
    info->bandwidth = (int32_t)bw;
    info->band_bytes = (int64_t)((double)c->n * (double)(bw + 1) * 8.0);
    return FEMCY_OK;
}

// solve_by_scipy (stiffnessMtrx.py:219-251): direct solve -- reverse Cuthill-McKee, lower band by columns, K = L S L^T,
// residual check + refinement (csrc/band_order.hpp; the device library does the same on tiles, csrc/kernels_direct.hip)
int femcy_direct_solve(femcy_ctx* ctx, int b_vec, int x_vec, femcy_direct_info* info) {
    CTX_OR_FAIL(ctx);
    FEMCY_TRY(check_two_vectors(c, b_vec, x_vec, TEXT_DIRECT_IN_PLACE));
    if (!c->have_band_order) {
        c->band_order = band_order_rcm(c->nn, c->ne, c->npe, c->elems.data());
        c->have_band_order = true;
    }
    const BandOrder& o = c->band_order;
    const int dm = c->dm, dd = dm * dm;
    const int64_t n = c->n, bw = ((int64_t)o.half_band_nodes + 1) * dm - 1, w = bw + 1;
    const double bytes = (double)n * (double)w * 8.0;
    femcy_direct_info local{};
    if (!info) info = &local;
    *info = femcy_direct_info{};
    info->n = n;
    info->band_bytes = (int64_t)bytes;
    info->bandwidth = (int32_t)bw;
    if (bytes > (double)c->direct_max_bytes) {
        set_error("direct solve: the band of this system (%lld DOF, %lld sub-diagonals after reverse Cuthill-McKee) takes "
                  "%.1f GB, more than the limit of %.1f GB (FEMCY_OPT_DIRECT_MAX_BYTES)",
                  (long long)n, (long long)bw, bytes * 1e-9, (double)c->direct_max_bytes * 1e-9);
        return FEMCY_ENOMEM;
    }
    std::vector<double> A, sgn((size_t)n);
    try {
        A.assign((size_t)n * (size_t)w, 0.0);
    } catch (const std::bad_alloc&) {
        set_error("direct solve: out of memory (%.1f GB)", bytes * 1e-9);
        return FEMCY_ENOMEM;
    }
#pragma omp parallel for schedule(static)
    for (int32_t a = 0; a < c->nn; ++a)
        for (int64_t q = c->rowptr[a]; q < c->rowptr[a + 1]; ++q) {
            const int32_t b = c->col[q];
            const int64_t ra = o.rank[a], rb = o.rank[b];
            if (ra < rb) continue;
            for (int r = 0; r < dm; ++r)
                for (int cc = 0; cc < dm; ++cc) {
                    const int64_t i = ra * dm + r, j = rb * dm + cc;
                    if (i >= j) A[(size_t)(j * w + (i - j))] = c->K[q * dd + r * dm + cc];
                }
        }
    int64_t negative = 0;
    const int64_t bad = band_factor_host(n, bw, A.data(), sgn.data(), &negative);
    info->negative_pivots = (int32_t)std::min<int64_t>(negative, INT32_MAX);
    if (bad) {
        info->singular_at = (int32_t)bad;
        set_error("direct solve: pivot %lld (band order) is zero or not a number -- the matrix is singular",
                  (long long)(bad - 1));
        return FEMCY_ENUMERIC;
    }
    const double* bvec = c->vec[b_vec].data();
    double* x = c->vec[x_vec].data();
    std::vector<double> y((size_t)n), res((size_t)n), Kx((size_t)n);
    auto solve_into = [&](const double* rhs, double* out, bool add) {      // out (+)= K^-1 rhs
        for (int64_t i = 0; i < n; ++i) y[(size_t)i] = rhs[(int64_t)o.node_at[i / dm] * dm + i % dm];
        band_solve_host(n, bw, A.data(), sgn.data(), y.data());
        for (int64_t i = 0; i < n; ++i) {
            double& dst = out[(int64_t)o.node_at[i / dm] * dm + i % dm];
            dst = add ? dst + y[(size_t)i] : y[(size_t)i];
        }
    };
    auto residual = [&]() {                                                 // res = b - K x; -> max|res| / max|b|
        spmv(c, x, Kx.data(), nullptr);
        double rm = 0.0, bm = 0.0;
        for (int64_t i = 0; i < n; ++i) {
            res[(size_t)i] = bvec[i] - Kx[(size_t)i];
            rm = std::fmax(rm, std::fabs(res[(size_t)i]));
            bm = std::fmax(bm, std::fabs(bvec[i]));
        }
        if (std::isnan(rm)) return rm;
        return bm > 0.0 ? rm / bm : rm;
    };
    solve_into(bvec, x, false);
    double rel = residual();
    while (info->refinements < DIRECT_MAX_REFINE && rel > DIRECT_REFINE_ABOVE) {
        solve_into(res.data(), x, true);
        ++info->refinements;
        const double rel2 = residual();
        const bool stalled = !(rel2 < 0.5 * rel);
        rel = rel2;
        if (stalled) break;
    }
    info->residual = rel;
    if (!(rel <= DIRECT_ACCEPT)) {
        set_error("direct solve: residual %.3e max|b| after %d refinement steps (%d negative pivots): elimination without "
                  "pivoting lost this matrix", rel, info->refinements, info->negative_pivots);
        return FEMCY_ENUMERIC;
    }
    return FEMCY_OK;
}

// ConjugateGradientSolver_rowMajor.solve (conjugateGradientSolver.py:103-127)
int femcy_pcg(femcy_ctx* ctx, int b_vec, int x_vec, double eps, int32_t maxit, int32_t* iters, double* rmax0,
              double* rmax_out) {
    CTX_OR_FAIL(ctx);
    FEMCY_TRY(check_two_vectors(c, b_vec, x_vec, TEXT_PCG_IN_PLACE));
    if (maxit <= 0) maxit = (int32_t)std::min<int64_t>(c->n, INT32_MAX);
    const double t_start = now_ms();
    const int64_t n = c->n;
    const int dm = c->dm, dd = dm * dm;
    const double* b = c->vec[b_vec].data();
    double *x = c->vec[x_vec].data(), *r = c->r.data(), *d = c->d.data(), *M = c->M.data(), *Ad = c->Ad.data();
    const int64_t nchunk = (n + CHUNK - 1) / CHUNK;
    std::vector<double> ps((size_t)nchunk), pm((size_t)nchunk);
    // M_init (:48-51), re_init + r_d_init (:32-38, 60-65)
#pragma omp parallel for schedule(static)
    for (int32_t a = 0; a < c->nn; ++a)
        for (int q = 0; q < dm; ++q) M[(int64_t)a * dm + q] = 1.0 / c->K[c->rowptr[a] * dd + q * dm + q];
    auto reduce_pair = [&](double& s, double& m) {
        s = 0.0;
        m = 0.0;
        for (int64_t ch = 0; ch < nchunk; ++ch) {
            s += ps[ch];
            m = std::fmax(m, pm[ch]);
        }
    };
#pragma omp parallel for schedule(static)
    for (int64_t ch = 0; ch < nchunk; ++ch) {
        double s = 0.0, m = 0.0;
        const int64_t i1 = std::min(n, (ch + 1) * CHUNK);
        for (int64_t i = ch * CHUNK; i < i1; ++i) {
            x[i] = 0.0;
            r[i] = b[i];
            d[i] = M[i] * b[i];
            s += b[i] * M[i] * b[i];
            m = std::fmax(m, nan_to_inf_abs(b[i]));
        }
        ps[ch] = s;
        pm[ch] = m;
    }
    double rMr, r0;
    reduce_pair(rMr, r0);
    double rmax = r0;
    int done = (r0 == 0.0) ? 1 : ((r0 != r0 || std::isinf(r0)) ? 2 : 0);
    int32_t it = 0;
    while (!done && it < maxit) {
        double dAd = 0.0;
        spmv(c, d, Ad, &dAd);
        const double alpha = rMr / dAd;
#pragma omp parallel for schedule(static)
        for (int64_t ch = 0; ch < nchunk; ++ch) {
            double s = 0.0, m = 0.0;
            const int64_t i1 = std::min(n, (ch + 1) * CHUNK);
            for (int64_t i = ch * CHUNK; i < i1; ++i) {
                x[i] += alpha * d[i];
                const double ri = r[i] - alpha * Ad[i];
                r[i] = ri;
                s += ri * M[i] * ri;
                m = std::fmax(m, nan_to_inf_abs(ri));
            }
            ps[ch] = s;
            pm[ch] = m;
        }
        double rMr_new;
        reduce_pair(rMr_new, rmax);
        ++it;
        if (rmax != rmax || std::isinf(rmax) || rMr_new != rMr_new) {
            done = 2;
        } else if (rmax < eps * r0) {
            done = 1;
        } else {
            const double beta = rMr_new / rMr;
#pragma omp parallel for schedule(static)
            for (int64_t i = 0; i < n; ++i) d[i] = M[i] * r[i] + beta * d[i];
        }
        rMr = rMr_new;
    }
    if (iters) *iters = it;
    if (rmax0) *rmax0 = r0;
    if (rmax_out) *rmax_out = rmax;
    c->timing.pcg_iters += it;
    c->timing.solves_three++;
    if (c->opt_timing) c->timing.pcg_ms += now_ms() - t_start;
    if (done == 2) {
        set_error("PCG breakdown: NaN/Inf residual after %d iterations (r0 = %g)", it, r0);
        return FEMCY_ENUMERIC;
    }
    return FEMCY_OK;
}

// ------------------------------------------------------------------------------ post-processing
int femcy_compute_strain_stress(femcy_ctx* ctx, int u_vec, int large) {
    CTX_OR_FAIL(ctx);
    FEMCY_REQUIRE(c->have_mesh && c->have_element && c->have_material, TEXT_NOT_DEFINED);
    VEC_OR_FAIL(u_vec);
    geom(c, c->vec[u_vec].data(), GEOM_F);   // F only: dsdx, vol and (nlgeom) the stress of the last force evaluation stay
    const int64_t ngp = (int64_t)c->ne * c->nGP;
    const int dd = c->dm * c->dm;
#pragma omp parallel for schedule(static)
    for (int64_t t = 0; t < ngp; ++t) {
        if (c->dm == 3)
            post_point<3>(large ? 1 : 0, c->mat_kind, c->h_C, c->mat_params[0], c->mat_params[1], c->F.data() + t * dd,
                          c->sigma.data() + t * dd, c->strain.data() + t * dd, c->mises.data() + t);
        else
            post_point<2>(large ? 1 : 0, c->mat_kind, c->h_C, c->mat_params[0], c->mat_params[1], c->F.data() + t * dd,
                          c->sigma.data() + t * dd, c->strain.data() + t * dd, c->mises.data() + t);
    }
    c->post_small = !large;                    // what femcy_thermal_stress may correct, once
    return FEMCY_OK;
}

int femcy_elastic_energy(femcy_ctx* ctx, int u_vec, double* total) {
    CTX_OR_FAIL(ctx);
    FEMCY_REQUIRE(c->have_mesh && c->have_element && c->have_material && total, TEXT_NOT_DEFINED);
    VEC_OR_FAIL(u_vec);
    geom(c, c->vec[u_vec].data(), GEOM_F);
    const int64_t ngp = (int64_t)c->ne * c->nGP;
    const int dm = c->dm, dd = dm * dm;
#pragma omp parallel for schedule(static)
    for (int64_t t = 0; t < ngp; ++t) {
        if (dm == 3) {
            double F[3][3];
            for (int i = 0; i < 3; ++i)
                for (int j = 0; j < 3; ++j) F[i][j] = c->F[t * dd + i * 3 + j];
            c->energy[t] = energy_density<3>(c->mat_kind, c->h_C, c->mat_params[0], c->mat_params[1], F);
        } else {
            double F[2][2];
            for (int i = 0; i < 2; ++i)
                for (int j = 0; j < 2; ++j) F[i][j] = c->F[t * dd + i * 2 + j];
            c->energy[t] = energy_density<2>(c->mat_kind, c->h_C, c->mat_params[0], c->mat_params[1], F);
        }
    }
    double s = 0.0;
    for (int64_t t = 0; t < ngp; ++t) s += c->energy[t] * c->vol[t];   // get_elasEng_kernel (:597-606)
    *total = s;
    return FEMCY_OK;
}

int femcy_elastic_energy_small(femcy_ctx* ctx, int u_vec, double* total) {
    CTX_OR_FAIL(ctx);
    FEMCY_TRY(check_elastic_energy_small(c, u_vec, total));
    geom(c, c->vec[u_vec].data(), GEOM_F);
    geom(c, nullptr, GEOM_DSDX);                     // the weights det J w of the UNDEFORMED mesh
    const int64_t ngp = (int64_t)c->ne * c->nGP;
    const int dm = c->dm, dd = dm * dm;
#pragma omp parallel for schedule(static)
    for (int64_t t = 0; t < ngp; ++t) {
        if (dm == 3) {
            double F[3][3];
            for (int i = 0; i < 3; ++i)
                for (int j = 0; j < 3; ++j) F[i][j] = c->F[t * dd + i * 3 + j];
            c->energy[t] = energy_density_small<3>(c->mat_kind, c->h_C, c->mat_params[0], c->mat_params[1], F);
        } else {
            double F[2][2];
            for (int i = 0; i < 2; ++i)
                for (int j = 0; j < 2; ++j) F[i][j] = c->F[t * dd + i * 2 + j];
            c->energy[t] = energy_density_small<2>(c->mat_kind, c->h_C, c->mat_params[0], c->mat_params[1], F);
        }
    }
    double s = 0.0;
    for (int64_t t = 0; t < ngp; ++t) s += c->energy[t] * c->vol[t];
    *total = s;
    return FEMCY_OK;
}

int femcy_extrapolate(femcy_ctx* ctx, int gp_field, int comp, const double* E, double* out) {
    CTX_OR_FAIL(ctx);
    int width = 1;
    FEMCY_TRY(check_extrapolate(c, gp_field, comp, E, out, &width));
    const double* field = nullptr;
    switch (gp_field) {
        case FEMCY_GP_VOL: field = c->vol.data(); break;
        case FEMCY_GP_MISES: field = c->mises.data(); break;
        case FEMCY_GP_ENERGY: field = c->energy.data(); break;
        case FEMCY_GP_F: field = c->F.data(); break;
        case FEMCY_GP_SIGMA: field = c->sigma.data(); break;
        case FEMCY_GP_STRAIN: field = c->strain.data(); break;
        default: return FEMCY_EINVAL;             // not reached: check_extrapolate has refused everything else
    }
    for (int64_t e = 0; e < c->ne; ++e)
        for (int a = 0; a < c->npe; ++a) {
            double acc = 0.0;
            for (int g = 0; g < c->nGP; ++g) acc += E[a * c->nGP + g] * field[(e * c->nGP + g) * width + comp];
            out[e * c->npe + a] = acc;
        }
    return FEMCY_OK;
}

// ---------------------------------------------------------------------------------- inspection
int femcy_get_K_ell(femcy_ctx* ctx, int32_t* ij, double* A) {
    CTX_OR_FAIL(ctx);
    FEMCY_REQUIRE(c->have_pattern && ij && A, TEXT_GET_K);
    const int dm = c->dm, dd = dm * dm, W = c->max_row_blocks * dm;
    for (int32_t a = 0; a < c->nn; ++a) {
        const int L = (int)(c->rowptr[a + 1] - c->rowptr[a]);
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
                    row_ij[1 + j * dm + cc] = c->col[c->rowptr[a] + j] * dm + cc;
                    row_A[j * dm + cc] = c->K[(c->rowptr[a] + j) * dd + r * dm + cc];
                }
        }
    }
    return FEMCY_OK;
}

int femcy_get_K_bsr(femcy_ctx* ctx, int32_t* rowptr, int32_t* colidx, double* out) {
    CTX_OR_FAIL(ctx);
    FEMCY_REQUIRE(c->have_pattern && rowptr && colidx && out, TEXT_GET_K);
    const int dd = c->dm * c->dm;
    int64_t w = 0;
    rowptr[0] = 0;
    std::vector<std::pair<int32_t, int64_t>> order;
    for (int32_t a = 0; a < c->nn; ++a) {
        order.clear();
        for (int64_t p = c->rowptr[a]; p < c->rowptr[a + 1]; ++p) order.push_back({c->col[p], p});
        std::sort(order.begin(), order.end());
        for (auto& pr : order) {
            colidx[w] = pr.first;
            for (int k = 0; k < dd; ++k) out[w * dd + k] = c->K[pr.second * dd + k];
            ++w;
        }
        rowptr[a + 1] = (int32_t)w;
    }
    return FEMCY_OK;
}

int femcy_get_gp_field(femcy_ctx* ctx, int which, double* out) {
    CTX_OR_FAIL(ctx);
    FEMCY_TRY(check_get_gp_field(c, which, out));
    const std::vector<double>* src = nullptr;
    switch (which) {
        case FEMCY_GP_DSDX: src = &c->dsdx; break;
        case FEMCY_GP_VOL: src = &c->vol; break;
        case FEMCY_GP_F: src = &c->F; break;
        case FEMCY_GP_SIGMA: src = &c->sigma; break;
        case FEMCY_GP_STRAIN: src = &c->strain; break;
        case FEMCY_GP_MISES: src = &c->mises; break;
        case FEMCY_GP_ENERGY: src = &c->energy; break;
        default: return FEMCY_EINVAL;             // not reached: check_get_gp_field has refused everything else
    }
    std::memcpy(out, src->data(), src->size() * sizeof(double));
    return FEMCY_OK;
}

int femcy_timing(femcy_ctx* ctx, femcy_timing_t* out) {
    CTX_OR_FAIL(ctx);
    FEMCY_REQUIRE(out, TEXT_NULL_OUTPUT);
    *out = c->timing;
    return FEMCY_OK;
}
int femcy_timing_reset(femcy_ctx* ctx) {
    CTX_OR_FAIL(ctx);
    c->timing = femcy_timing_t{};
    return FEMCY_OK;
}

// ------------------------------------------------------------ not on the host: device probes, multi-rank
int femcy_probe_stream(femcy_ctx*, int64_t, int32_t, int32_t, double*, int64_t*) {
    set_error("femcy_probe_stream measures a GPU: not available in the CPU backend");
    return FEMCY_EINVAL;
}
int femcy_probe_spmv(femcy_ctx*, int32_t, int32_t, double*) {
    set_error("femcy_probe_spmv measures a GPU: not available in the CPU backend");
    return FEMCY_EINVAL;
}
int femcy_probe_exchange(femcy_ctx*, int32_t, int32_t, double*) {
    set_error("femcy_probe_exchange measures a GPU: not available in the CPU backend");
    return FEMCY_EINVAL;
}
int femcy_persist_streamed_bytes(femcy_ctx* ctx, int64_t* bytes) {
    CTX_OR_FAIL(ctx);
    (void)c;
    FEMCY_REQUIRE(bytes, TEXT_NULL_OUTPUT);
    *bytes = 0;
    return FEMCY_OK;
}
#define NO_COMM(name)                                                                             \
    set_error(name ": the CPU backend holds the whole mesh in one process (no communicator)"); \
    return FEMCY_ECOMM
int femcy_comm_unique_id(void*) { NO_COMM("femcy_comm_unique_id"); }
int femcy_comm_local_id(void*) { NO_COMM("femcy_comm_local_id"); }
int femcy_comm_shm_id(void*, int64_t) { NO_COMM("femcy_comm_shm_id"); }
int femcy_probe_mailbox(femcy_ctx*, int32_t, double*) { NO_COMM("femcy_probe_mailbox"); }
int femcy_comm_allgather_host(femcy_ctx*, const void*, int32_t, void*) { NO_COMM("femcy_comm_allgather_host"); }
int femcy_comm_init(femcy_ctx*, int32_t, int32_t, const void*, int32_t, const int32_t*, const int32_t*, int32_t,
                    const uint8_t*) { NO_COMM("femcy_comm_init"); }
int femcy_comm_set_neighbours(femcy_ctx*, int32_t, const int32_t*, const int32_t*, const int32_t*) { NO_COMM("femcy_comm_set_neighbours"); }
int femcy_comm_tune(femcy_ctx*, int32_t, int32_t*, double*) { NO_COMM("femcy_comm_tune"); }
int femcy_iface_sum(femcy_ctx*, int) { NO_COMM("femcy_iface_sum"); }
int femcy_comm_mailbox_export(femcy_ctx*, void*) { NO_COMM("femcy_comm_mailbox_export"); }
int femcy_comm_mailbox_import(femcy_ctx*, int32_t, const void*) { NO_COMM("femcy_comm_mailbox_import"); }
int femcy_comm_persist_agree(femcy_ctx*, int32_t*) { NO_COMM("femcy_comm_persist_agree"); }
int femcy_comm_info(femcy_ctx* ctx, int32_t* rank, int32_t* nranks, int64_t* n_global) {
    CTX_OR_FAIL(ctx);
    if (rank) *rank = 0;
    if (nranks) *nranks = 1;
    if (n_global) *n_global = c->n;
    return FEMCY_OK;
}

}  // extern "C"
