// Explicit dynamics for gfx950 (*Dynamic, explicit): HRZ-lumped mass, the fused node pass of a velocity-Verlet step, the
// kinetic energy and the Gershgorin bound behind the stable increment.  The reference has no dynamics; the element pass of a
// step is k_geom<..., true> of kernels_assembly.hip (launch_geom with GEOM_DSDX | GEOM_FE), which leaves fe[e][a][:].
//
// A step is two launches: that element pass and the node pass (explicit_node_pass), which does what femcy_internal_force's
// node gather and four vector kernels would do in five launches -- the node sums of fe are never stored, and f, minv, a, v, u
// are read and a, v, u written once per step, dm contiguous doubles per node each.  The node pass has two entry points that
// differ only in where the step's numbers (ExplicitStep, element_math.hpp) come from: k_explicit_node takes them from the
// host, k_explicit_node_auto from the device clock of an element-by-element run; k_explicit_drift / _auto likewise.  The
// node sums of the lumped mass are k_node_sum of kernels_assembly.hip (launch_node_sum).  With damping set
// (femcy_explicit_set_damping) the element pass is k_geom<..., true, GeomDampHost / GeomDampClock>, which adds the bulk
// viscosity, the node pass subtracts alpha v_{n+1/2} (explicit_kick_damped) and the bound kernel returns omega_eff.
#include <algorithm>
#include <cmath>
#include <type_traits>
#include "ctx.hpp"
#include "element_dispatch.hpp"
#include "element_math.hpp"
#include "load_row.hpp"
#include "node_gather.hpp"
#include "wave_reduce.hpp"

namespace femcy {

constexpr int XBS = 256;

// ----------------------------------------------------------------------------------- lumped mass
// element pass in the shape of k_mass_points: one thread per element, the mass rule's tables Nq / dNq / wq wave-uniform, node
// rows by load_row; the element's NPE lumped masses (element_math.hpp: lumped_element) go to me[e][0..NPE).  Built once per
// run, so the stores are left strided.
template <int NPE, int DM>
__global__ void __launch_bounds__(XBS) k_lumped_elem(int32_t ne, int32_t nq, const double* __restrict__ nodes,
                                                     const int32_t* __restrict__ elems, const double* __restrict__ Nq,
                                                     const double* __restrict__ dNq, const double* __restrict__ wq,
                                                     double rho, double* __restrict__ me_out) {
    const int32_t e = blockIdx.x * blockDim.x + threadIdx.x;
    if (e >= ne) return;
    double X[NPE][DM], me[NPE];
#pragma unroll
    for (int a = 0; a < NPE; ++a) load_row<DM>(nodes + (int64_t)elems[(int64_t)e * NPE + a] * DM, X[a]);
    lumped_element<NPE, DM>(X, nq, Nq, dNq, wq, rho, me);
#pragma unroll
    for (int a = 0; a < NPE; ++a) me_out[(int64_t)e * NPE + a] = me[a];
}

// minv[a * DM + i] = 1 / m[a]; the constrained DOFs are zeroed afterwards by the DOF sets' own scatter
template <int DM>
__global__ void __launch_bounds__(XBS) k_explicit_minv(int64_t n, const double* __restrict__ m, double* __restrict__ minv) {
    const int64_t i = (int64_t)blockIdx.x * XBS + threadIdx.x;
    if (i < n) minv[i] = 1.0 / m[i / DM];
}

// ------------------------------------------------------------------------------------ node pass
// Launch shape and gather of k_nodal_force (node_gather.hpp): half a wavefront (32 lanes) owns a node and sums its incident
// rows of fe.  The tree leaves the same bits in all 32 lanes, so lane i < DM takes component i: its f, minv, a, v, u are
// requested before the gather and DM neighbouring lanes read and write DM contiguous doubles.  What mode and st say is with
// ExplicitStep in element_math.hpp; the arithmetic is explicit_kick / explicit_drift there, the functions the first drift
// below and the host backend call.
// MOTION (empty, or one NodeMotion: an integrator with femcy_explicit_set_motion): a lane whose DOF is held (minv = 0) and
// moved (slot >= 0) ignores the gathered force and stores explicit_moved of element_math.hpp instead -- a and v of its curve
// at mo.t, the time of the state being kicked, and when drifting u at mo.t_drift by assignment.  Every other lane runs the
// arithmetic below unchanged; without the argument the kernel has the arguments and the code it always had.
struct NodeMotion {
    const int32_t *slot, *curve;      // [n] position in the compact list or -1; [moved] curve of each list entry
    const double* val;                // [moved] the value g
    const Amplitude* amp;             // the curves
    double t, t_drift;                // k_explicit_node_auto fills both from the clock
};
// WALL (empty, or one NodeWall after the motion if there is one: an integrator with femcy_explicit_set_wall): a lane also
// reads X[i] and, in every mode, u[i]; once the gather has reconverged the wavefront -- before any lane leaves -- the DM
// lanes of a node hand x = X + u round inside their quad on the DPP network (quad_perm broadcasts of the quad's lanes
// 0 .. DM-1, which are all `mine` or all not; a lane that is not reads back the 0 it put in and uses nothing of it), and
// every lane evaluates the gap and its own component by wall_accel of element_math.hpp inside explicit_kick_wall.  A moved
// lane takes no wall force, but its u has entered x.  Without the argument a kernel has the arguments and the code it has
// with the motion alone.
struct NodeWall {
    const double* X;                  // [n] the node coordinates
    ExplicitWalls w;
};
template <class T, class... A>
constexpr bool has_opt = (std::is_same_v<T, A> || ...);
template <class T, class A, class... R>
__device__ __forceinline__ const T& opt_arg(const A& a, const R&... r) {
    if constexpr (std::is_same_v<T, A>)
        return a;
    else
        return opt_arg<T>(r...);
}
template <class... OPT>
constexpr bool opt_known = ((std::is_same_v<NodeMotion, OPT> || std::is_same_v<NodeWall, OPT>) && ...) && sizeof...(OPT) <= 2 &&
                           (sizeof...(OPT) < 2 || (has_opt<NodeMotion, OPT...> && has_opt<NodeWall, OPT...>));
// x[j] of the lane's node from the quad's lane j; all 64 lanes active
template <int DM>
__device__ __forceinline__ void quad_gather(double xi, double (&x)[DM]) {
    static_assert(DM <= 3, "a node's components must stand in the first lanes of one quad");
    x[0] = dpp_move<0x00, 0xf>(xi);   // quad_perm [0,0,0,0]
    x[1] = dpp_move<0x55, 0xf>(xi);   // quad_perm [1,1,1,1]
    if constexpr (DM == 3) x[2] = dpp_move<0xAA, 0xf>(xi);   // quad_perm [2,2,2,2]
}
template <int DM, class... MOTION>
__device__ __forceinline__ void explicit_node_pass(int32_t nn, const int32_t* __restrict__ ne_ptr,
                                                   const int32_t* __restrict__ ne_idx, const double* __restrict__ fe,
                                                   const double* __restrict__ f, const double* __restrict__ minv,
                                                   const ExplicitStep& st, int mode, double* __restrict__ u,
                                                   double* __restrict__ v, double* __restrict__ acc_vec,
                                                   const MOTION&... motion) {
    constexpr bool MOVE = has_opt<NodeMotion, MOTION...>, WALL = has_opt<NodeWall, MOTION...>;
    static_assert(opt_known<MOTION...>, "at most one motion and one wall argument");
    const int64_t t = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    const int32_t a = (int32_t)(t >> 5);
    const int sub = (int)(t & 31);
    const bool mine = a < nn && sub < DM;
    const int64_t i = (int64_t)a * DM + sub;
    double fi = 0.0, mi = 0.0, ai = 0.0, vi = 0.0, ui = 0.0;
    [[maybe_unused]] double xi = 0.0;
    [[maybe_unused]] int32_t slot = -1;
    if (mine) {
        if constexpr (MOVE) slot = opt_arg<NodeMotion>(motion...).slot[i];
        fi = f[i];
        mi = minv[i];
        if (mode != XN_START) {
            ai = acc_vec[i];
            vi = v[i];
        } else if (st.alpha != 0.0) {
            vi = v[i];                                  // v_{-1/2} := v_0; vec[ACC] is not read at the start
        }
        if (WALL || st.drift) ui = u[i];
        if constexpr (WALL) xi = opt_arg<NodeWall>(motion...).X[i] + ui;
    }
    double acc[DM];
    node_gather<DM>(a, sub, nn, ne_ptr, ne_idx, fe, acc);
    [[maybe_unused]] double x[DM];
    if constexpr (WALL) quad_gather<DM>(xi, x);
    if (!mine) return;
    if constexpr (MOVE) {
        if (mi == 0.0 && slot >= 0) {
            const NodeMotion& mo = opt_arg<NodeMotion>(motion...);
            explicit_moved(mo.amp[mo.curve[slot]], mo.val[slot], mo.t, mo.t_drift, mode == XN_START, st.drift, ui, vi, ai);
            acc_vec[i] = ai;
            if (mode == XN_START) return;
            v[i] = vi;
            if (st.drift) u[i] = ui;
            return;
        }
    }
    const double fint = sub == 0 ? acc[0] : (sub == 1 ? acc[1] : acc[DM - 1]);
    if constexpr (WALL)
        explicit_kick_wall<DM>(mi, st.s, fi, fint, st.hh, st.alpha, opt_arg<NodeWall>(motion...).w, x, sub, vi, ai);
    else if (st.alpha != 0.0)
        explicit_kick_damped(mi, st.s, fi, fint, st.hh, st.alpha, vi, ai);
    else
        explicit_kick(mi, st.s, fi, fint, st.hh, vi, ai);
    acc_vec[i] = ai;
    if (mode == XN_START) return;
    v[i] = vi;
    if (st.drift) u[i] = explicit_drift(ui, vi, ai, st.h, st.h2h);
}

// a fixed step: the host filled st (explicit_step_fixed)
template <int DM, class... MOTION>
__global__ void __launch_bounds__(XBS) k_explicit_node(int32_t nn, const int32_t* __restrict__ ne_ptr,
                                                       const int32_t* __restrict__ ne_idx,
                                                       const double* __restrict__ fe, const double* __restrict__ f,
                                                       const double* __restrict__ minv, ExplicitStep st, int mode,
                                                       double* __restrict__ u, double* __restrict__ v,
                                                       double* __restrict__ acc_vec, MOTION... motion) {
    explicit_node_pass<DM>(nn, ne_ptr, ne_idx, fe, f, minv, st, mode, u, v, acc_vec, motion...);
}

// a step of an automatic run: st from the device clock, which may say that nothing is written (explicit_step_clock)
// with motion: the state being kicked is at the clock's t, the drift reaches its t_next; a no-op step writes no moved DOF
// either
template <int DM, class... MOTION>
__global__ void __launch_bounds__(XBS) k_explicit_node_auto(int32_t nn, const int32_t* __restrict__ ne_ptr,
                                                            const int32_t* __restrict__ ne_idx,
                                                            const double* __restrict__ fe, const double* __restrict__ f,
                                                            const double* __restrict__ minv,
                                                            const ExplicitClock* __restrict__ clk, int mode,
                                                            double alpha, double* __restrict__ u,
                                                            double* __restrict__ v, double* __restrict__ acc_vec,
                                                            MOTION... motion) {
    ExplicitStep st;
    if (!explicit_step_clock(*clk, mode, st, alpha)) return;
    if constexpr (has_opt<NodeMotion, MOTION...>) {
        NodeMotion mo = opt_arg<NodeMotion>(motion...);
        mo.t = clk->t;
        mo.t_drift = clk->t_next;
        if constexpr (has_opt<NodeWall, MOTION...>)
            explicit_node_pass<DM>(nn, ne_ptr, ne_idx, fe, f, minv, st, mode, u, v, acc_vec, mo, opt_arg<NodeWall>(motion...));
        else
            explicit_node_pass<DM>(nn, ne_ptr, ne_idx, fe, f, minv, st, mode, u, v, acc_vec, mo);
    } else {
        explicit_node_pass<DM>(nn, ne_ptr, ne_idx, fe, f, minv, st, mode, u, v, acc_vec, motion...);
    }
}

// ---------------------------------------------------------------------- node pass with the energy balance
// The node pass above plus the work addends of the step that led to the state being kicked (femcy.h at
// femcy_explicit_energy_enable; the arithmetic is explicit_energy_free / _moved of element_math.hpp): a variant of its own,
// so that the pass above keeps its arguments and its code.  u, v and a go through the same functions in the same order: the
// same bits.  The lanes of a DOF hold what the addends need in registers -- f, minv, v and a of the previous state, the
// gathered force -- and read three more numbers: the node's mass and the two forces of the previous state (NodeEnergy::
// fint, falpha), which they then replace by this state's.
// Sums: a wavefront covers two nodes, so its addends stand in the lanes 0 .. DM-1 and 32 .. 32+DM-1 and every other lane
// holds 0.  Two quad swaps on the DPP network sum each quad, lane 0's and lane 32's results are read as scalars and added:
// a fixed order, no LDS, no barrier, no atomics.  Lane 0 adds the four sums to the wavefront's own slot (EN_SLOT doubles,
// one 64-byte line), which nobody else touches; the grid is the same in every step of a run, and launch_explicit_energy_sum
// adds the slots up.  The slot also carries the load scale and the time of the last kicked state from one kick to the
// next (every lane reads them, lane 0 writes them): a split run needs nothing from the host.  No lane leaves before the
// sums, a >= nn included.  At XN_START the slot is zeroed and only the forces of state 0 are recorded.  hh = 0 in a kick
// (nothing led to the state): nothing is added.
struct NodeEnergy {
    const double* m;                  // [nn] the lumped mass
    double *fint, *falpha;            // [n] the gathered force and the alpha force of the last kicked state
    double* slot;                     // [wavefronts of the grid][EN_SLOT]
};
enum { EN_S = 4, EN_T = 5 };          // where a slot keeps the load scale and the time of the last kicked state
__device__ __forceinline__ double energy_wave_sum(double x) {
    x += dpp_move<0xB1, 0xf>(x);      // quad_perm [1,0,3,2]
    x += dpp_move<0x4E, 0xf>(x);      // quad_perm [2,3,0,1]: lanes 0 and 32 hold their quad's sum
    const double lo = __hiloint2double(__builtin_amdgcn_readlane(__double2hiint(x), 0),
                                       __builtin_amdgcn_readlane(__double2loint(x), 0));
    const double hi = __hiloint2double(__builtin_amdgcn_readlane(__double2hiint(x), 32),
                                       __builtin_amdgcn_readlane(__double2loint(x), 32));
    return lo + hi;
}
template <int DM, class... MOTION>
__device__ __forceinline__ void explicit_node_pass_energy(int32_t nn, const int32_t* __restrict__ ne_ptr,
                                                          const int32_t* __restrict__ ne_idx,
                                                          const double* __restrict__ fe, const double* __restrict__ f,
                                                          const double* __restrict__ minv, const ExplicitStep& st, int mode,
                                                          double* __restrict__ u, double* __restrict__ v,
                                                          double* __restrict__ acc_vec, const NodeEnergy& en,
                                                          const MOTION&... motion) {
    constexpr bool MOVE = has_opt<NodeMotion, MOTION...>, WALL = has_opt<NodeWall, MOTION...>;
    static_assert(opt_known<MOTION...>, "at most one motion and one wall argument");
    static_assert(DM <= 4 && XBS % 64 == 0, "a node's addends must stand in one quad, a wavefront in one workgroup");
    const int64_t t = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    const int32_t a = (int32_t)(t >> 5);
    const int sub = (int)(t & 31);
    const bool mine = a < nn && sub < DM;
    const bool start = mode == XN_START;
    const int64_t i = (int64_t)a * DM + sub;
    double* my_slot = en.slot + (t >> 6) * EN_SLOT;
    double fi = 0.0, mi = 0.0, ai = 0.0, vi = 0.0, ui = 0.0, ma = 0.0, fp = 0.0, gp = 0.0, s_prev = 0.0;
    [[maybe_unused]] double t_prev = 0.0, xi = 0.0;
    [[maybe_unused]] int32_t slot = -1;
    if (!start) {
        s_prev = my_slot[EN_S];
        if constexpr (MOVE) t_prev = my_slot[EN_T];
    }
    if (mine) {
        if constexpr (MOVE) slot = opt_arg<NodeMotion>(motion...).slot[i];
        fi = f[i];
        mi = minv[i];
        ma = en.m[a];
        if (!start) {
            ai = acc_vec[i];
            vi = v[i];
            fp = en.fint[i];
            gp = en.falpha[i];
        } else if (st.alpha != 0.0) {
            vi = v[i];                                  // v_{-1/2} := v_0; vec[ACC] is not read at the start
        }
        if (WALL || st.drift) ui = u[i];
        if constexpr (WALL) xi = opt_arg<NodeWall>(motion...).X[i] + ui;
    }
    double acc[DM];
    node_gather<DM>(a, sub, nn, ne_ptr, ne_idx, fe, acc);
    [[maybe_unused]] double x[DM];
    if constexpr (WALL) quad_gather<DM>(xi, x);
    double w[4] = {0.0, 0.0, 0.0, 0.0};
    [[maybe_unused]] double t_now = 0.0;
    if constexpr (MOVE) t_now = opt_arg<NodeMotion>(motion...).t;
    if (mine) {
        const double fint = sub == 0 ? acc[0] : (sub == 1 ? acc[1] : acc[DM - 1]);
        const bool count = !start && st.hh != 0.0;
        bool moved = false;
        if constexpr (MOVE) moved = mi == 0.0 && slot >= 0;
        if constexpr (MOVE) {
            if (moved) {
                const NodeMotion& mo = opt_arg<NodeMotion>(motion...);
                const Amplitude& am = mo.amp[mo.curve[slot]];
                const double a_prev = ai;
                explicit_moved(am, mo.val[slot], mo.t, mo.t_drift, start, st.drift, ui, vi, ai);
                if (count) explicit_energy_moved(am, mo.val[slot], t_prev, mo.t, ma, s_prev, st.s, fi, fp, fint, a_prev, ai, w);
                en.fint[i] = fint;
                en.falpha[i] = 0.0;
                acc_vec[i] = ai;
                if (!start) {
                    v[i] = vi;
                    if (st.drift) u[i] = ui;
                }
            }
        }
        if (!moved) {
            double ga;
            explicit_energy_free(mi, ma, s_prev, st.s, fi, fp, fint, gp, st.alpha, vi, ai, st.hh, !count, w, ga);
            en.fint[i] = fint;
            en.falpha[i] = ga;
            if constexpr (WALL)
                explicit_kick_wall<DM>(mi, st.s, fi, fint, st.hh, st.alpha, opt_arg<NodeWall>(motion...).w, x, sub, vi, ai);
            else if (st.alpha != 0.0)
                explicit_kick_damped(mi, st.s, fi, fint, st.hh, st.alpha, vi, ai);
            else
                explicit_kick(mi, st.s, fi, fint, st.hh, vi, ai);
            acc_vec[i] = ai;
            if (!start) {
                v[i] = vi;
                if (st.drift) u[i] = explicit_drift(ui, vi, ai, st.h, st.h2h);
            }
        }
    }
    if (start) {
        if ((threadIdx.x & 63) == 0) {
#pragma unroll
            for (int k = 0; k < 4; ++k) my_slot[k] = 0.0;
            my_slot[EN_S] = st.s;
            my_slot[EN_T] = t_now;
        }
        return;
    }
    if (st.hh != 0.0) {
#pragma unroll
        for (int k = 0; k < 4; ++k) w[k] = energy_wave_sum(w[k]);
    }
    if ((threadIdx.x & 63) == 0) {
        if (st.hh != 0.0) {
#pragma unroll
            for (int k = 0; k < 4; ++k) my_slot[k] += w[k];
        }
        my_slot[EN_S] = st.s;
        my_slot[EN_T] = t_now;
    }
}

template <int DM, class... MOTION>
__global__ void __launch_bounds__(XBS) k_explicit_node_energy(int32_t nn, const int32_t* __restrict__ ne_ptr,
                                                              const int32_t* __restrict__ ne_idx,
                                                              const double* __restrict__ fe, const double* __restrict__ f,
                                                              const double* __restrict__ minv, ExplicitStep st, int mode,
                                                              double* __restrict__ u, double* __restrict__ v,
                                                              double* __restrict__ acc_vec, NodeEnergy en, MOTION... motion) {
    explicit_node_pass_energy<DM>(nn, ne_ptr, ne_idx, fe, f, minv, st, mode, u, v, acc_vec, en, motion...);
}

// a step that does nothing (explicit_step_clock false) returns before anything is read: no slot, no force is written
template <int DM, class... MOTION>
__global__ void __launch_bounds__(XBS) k_explicit_node_auto_energy(int32_t nn, const int32_t* __restrict__ ne_ptr,
                                                                   const int32_t* __restrict__ ne_idx,
                                                                   const double* __restrict__ fe,
                                                                   const double* __restrict__ f,
                                                                   const double* __restrict__ minv,
                                                                   const ExplicitClock* __restrict__ clk, int mode,
                                                                   double alpha, double* __restrict__ u,
                                                                   double* __restrict__ v, double* __restrict__ acc_vec,
                                                                   NodeEnergy en, MOTION... motion) {
    ExplicitStep st;
    if (!explicit_step_clock(*clk, mode, st, alpha)) return;
    if constexpr (has_opt<NodeMotion, MOTION...>) {
        NodeMotion mo = opt_arg<NodeMotion>(motion...);
        mo.t = clk->t;
        mo.t_drift = clk->t_next;
        if constexpr (has_opt<NodeWall, MOTION...>)
            explicit_node_pass_energy<DM>(nn, ne_ptr, ne_idx, fe, f, minv, st, mode, u, v, acc_vec, en, mo, opt_arg<NodeWall>(motion...));
        else
            explicit_node_pass_energy<DM>(nn, ne_ptr, ne_idx, fe, f, minv, st, mode, u, v, acc_vec, en, mo);
    } else {
        explicit_node_pass_energy<DM>(nn, ne_ptr, ne_idx, fe, f, minv, st, mode, u, v, acc_vec, en, motion...);
    }
}

// u, v and a (what: MOVE_U | MOVE_V | MOVE_A of element_math.hpp) of the moved DOFs at one time, one thread per entry of the
// compact list: at the start of a run everything at t, before the element pass; after the first drift of a call u alone, at
// the time that drift reached -- t, or with clk the clock's t_next, and nothing when its h_next = 0 (the drift wrote
// nothing either).  Every DOF stands in the list once.
__global__ void __launch_bounds__(XBS) k_explicit_place(int32_t nmoved, const int32_t* __restrict__ dof,
                                                        const double* __restrict__ val, const int32_t* __restrict__ curve,
                                                        const Amplitude* __restrict__ amp,
                                                        const ExplicitClock* __restrict__ clk, double t, int what,
                                                        double* __restrict__ u, double* __restrict__ v,
                                                        double* __restrict__ a) {
    const int32_t k = blockIdx.x * XBS + threadIdx.x;
    if (k >= nmoved) return;
    if (clk) {
        if (clk->h_next == 0.0) return;
        t = clk->t_next;
    }
    const int32_t i = dof[k];
    double ui = 0.0, vi = 0.0, ai = 0.0;
    explicit_place(amp[curve[k]], val[k], t, what, ui, vi, ai);
    if (what & MOVE_U) u[i] = ui;
    if (what & MOVE_V) v[i] = vi;
    if (what & MOVE_A) a[i] = ai;
}

// the first drift of a call: u += h v + (h^2 / 2) a from memory, by the function the node pass applies to its registers
__device__ __forceinline__ void explicit_first_drift(int64_t n, double h, double h2h, const double* __restrict__ v,
                                                     const double* __restrict__ a, double* __restrict__ u) {
    const int64_t i = (int64_t)blockIdx.x * XBS + threadIdx.x;
    if (i < n) u[i] = explicit_drift(u[i], v[i], a[i], h, h2h);
}
__global__ void __launch_bounds__(XBS) k_explicit_drift(int64_t n, double h, double h2h, const double* __restrict__ v,
                                                        const double* __restrict__ a, double* __restrict__ u) {
    explicit_first_drift(n, h, h2h, v, a, u);
}
// by h_next of the device clock; h_next = 0 writes nothing
__global__ void __launch_bounds__(XBS) k_explicit_drift_auto(int64_t n, const ExplicitClock* __restrict__ clk,
                                                             const double* __restrict__ v, const double* __restrict__ a,
                                                             double* __restrict__ u) {
    const double h = clk->h_next;
    if (h != 0.0) explicit_first_drift(n, h, 0.5 * h * h, v, a, u);
}

// ------------------------------------------------------------------------------------ reductions
// a workgroup's 256 values -> one, in a fixed order: xor tree inside each wavefront, then the four wave results in ascending
// order by thread 0 (MAX: the maximum instead of the sum)
template <bool MAX>
__device__ __forceinline__ double block_reduce(double x, double* sm) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
        const double y = __shfl_xor(x, o, 64);
        x = MAX ? fmax(x, y) : x + y;
    }
    if ((threadIdx.x & 63) == 0) sm[threadIdx.x >> 6] = x;
    __syncthreads();
    double r = sm[0];
#pragma unroll
    for (int w = 1; w < XBS / 64; ++w) r = MAX ? fmax(r, sm[w]) : r + sm[w];
    __syncthreads();
    return r;
}

// partial sums of m_a |v_a|^2: thread t of workgroup b takes the nodes b * 256 + t + k * (workgroups * 256), k ascending
template <int DM>
__global__ void __launch_bounds__(XBS) k_explicit_energy(int32_t nn, const double* __restrict__ m,
                                                         const double* __restrict__ v, double* __restrict__ part) {
    __shared__ double sm[XBS / 64];
    double acc = 0.0;
    for (int64_t a = (int64_t)blockIdx.x * XBS + threadIdx.x; a < nn; a += (int64_t)gridDim.x * XBS) {
        double vv = v[a * DM] * v[a * DM];
#pragma unroll
        for (int c = 1; c < DM; ++c) vv = fma(v[a * DM + c], v[a * DM + c], vv);
        acc = fma(m[a], vv, acc);
    }
    const double r = block_reduce<false>(acc, sm);
    if (threadIdx.x == 0) part[blockIdx.x] = r;
}

// np partials -> one, by one workgroup: thread t takes the partials t, t + 256, ... in ascending order, then the same tree
template <bool MAX>
__device__ __forceinline__ double reduce_partials(int np, const double* __restrict__ part, double* sm) {
    double acc = 0.0;
    for (int i = threadIdx.x; i < np; i += XBS) acc = MAX ? fmax(acc, part[i]) : acc + part[i];
    return block_reduce<MAX>(acc, sm);
}

template <bool MAX>
__global__ void __launch_bounds__(XBS) k_explicit_final(int np, const double* __restrict__ part, double* __restrict__ out) {
    __shared__ double sm[XBS / 64];
    const double r = reduce_partials<MAX>(np, part, sm);
    if (threadIdx.x == 0) *out = r;
}

// the read-back of the energy balance: workgroup k = 0 .. 3 sums the k-th double of the nslots slots of the node pass, thread
// t the slots t, t + 256, ... in ascending order, then the same tree
__global__ void __launch_bounds__(XBS) k_explicit_energy_sum(int nslots, const double* __restrict__ slot,
                                                             double* __restrict__ out) {
    __shared__ double sm[XBS / 64];
    double acc = 0.0;
    for (int i = threadIdx.x; i < nslots; i += XBS) acc += slot[(int64_t)i * EN_SLOT + blockIdx.x];
    const double r = block_reduce<false>(acc, sm);
    if (threadIdx.x == 0) out[blockIdx.x] = r;
}

// the read-back of a rigid wall (femcy_explicit_wall_get): partials of the four terms of wall_node_terms (element_math.hpp)
// over the nodes in the pattern of k_explicit_energy -- thread t of workgroup b takes the nodes b * 256 + t + k *
// (workgroups * 256), k ascending -- into part[j * gridDim.x + b]: three sums and one maximum, then k_explicit_final
template <int DM>
__global__ void __launch_bounds__(XBS) k_explicit_wall(int32_t nn, const double* __restrict__ X, const double* __restrict__ u,
                                                       const double* __restrict__ m, const double* __restrict__ minv,
                                                       ExplicitWalls wl, int k, double* __restrict__ part) {
    __shared__ double sm[XBS / 64];
    double acc[4] = {0.0, 0.0, 0.0, 0.0};
    for (int64_t a = (int64_t)blockIdx.x * XBS + threadIdx.x; a < nn; a += (int64_t)gridDim.x * XBS) {
        double x[DM], t[4];
        bool any_free = false;
#pragma unroll
        for (int c = 0; c < DM; ++c) {
            x[c] = X[a * DM + c] + u[a * DM + c];
            any_free = any_free || minv[a * DM + c] != 0.0;
        }
        wall_node_terms<DM>(wl, k, x, m[a], any_free, t);
        acc[0] += t[0];
        acc[1] += t[1];
        acc[2] += t[2];
        acc[3] = fmax(acc[3], t[3]);
    }
#pragma unroll
    for (int j = 0; j < 3; ++j) {
        const double r = block_reduce<false>(acc[j], sm);
        if (threadIdx.x == 0) part[j * gridDim.x + blockIdx.x] = r;
    }
    const double r = block_reduce<true>(acc[3], sm);
    if (threadIdx.x == 0) part[3 * gridDim.x + blockIdx.x] = r;
}

// Gershgorin pass over the SELL storage: one lane per stored row position p = slice * 64 + lane (node_of[p] < 0: padding),
// the node's blocks j = 0 .. rowlen - 1 in storage order, the DM entries of each of its DM scalar rows through kv_index in
// ascending column order; a scalar row counts with sum_j |K_ij| minv_i unless minv_i = 0 (constrained).  A NaN counts as
// infinity, so that a broken matrix gives no increment.  Then the maximum reduction above.
template <int DM>
__global__ void __launch_bounds__(XBS) k_rowabs_bound(int64_t npos, const int32_t* __restrict__ node_of,
                                                      const int32_t* __restrict__ rowlen,
                                                      const int64_t* __restrict__ slice_off,
                                                      const double* __restrict__ K, const double* __restrict__ minv,
                                                      double* __restrict__ part) {
    __shared__ double sm[XBS / 64];
    double best = 0.0;
    for (int64_t p = (int64_t)blockIdx.x * XBS + threadIdx.x; p < npos; p += (int64_t)gridDim.x * XBS) {
        const int32_t a = node_of[p];
        if (a < 0) continue;
        const int lane = (int)(p & 63);
        const int64_t off = slice_off[p >> 6];
        const int32_t L = rowlen[a];
        double sum[DM];
#pragma unroll
        for (int r = 0; r < DM; ++r) sum[r] = 0.0;
        for (int32_t j = 0; j < L; ++j)
#pragma unroll
            for (int k = 0; k < DM * DM; ++k) sum[k / DM] += fabs(K[kv_index<DM>(off + j, k, lane)]);
#pragma unroll
        for (int r = 0; r < DM; ++r) {
            const double mi = minv[(int64_t)a * DM + r];
            const double b = sum[r] * mi;
            if (mi != 0.0) best = fmax(best, b != b ? INFINITY : b);
        }
    }
    const double r = block_reduce<true>(best, sm);
    if (threadIdx.x == 0) part[blockIdx.x] = r;
}

// ---------------------------------------------------------------------- element-by-element increment
// omega_e^2 of element_math.hpp (explicit_bound_element), one thread per element, recomputed from nodes, u, elems and the
// element's own lumped masses me[e][0..NPE): the launch shape of k_lumped_elem.  (Reading the records of an element pass that
// also stores sigma was measured against this: 218.3 against 181.5 us per step on the 1 M C3D4 plate, the fixed step at
// 149.2 -- the extra 72 B per element the element pass then writes cost more than the gathers here;
// profiles/explicit_auto.json.)  The workgroup's maximum goes to
// part[blockIdx.x] (ceil(ne / 256) partials, no grid-stride loop: k_explicit_clock loops over any number of them).  A NaN
// counts as infinity, as in k_rowabs_bound, so that a broken element gives no increment.
// DAMPING (empty, or one BoundDamping: an integrator with damping set): omega_eff,e^2 of explicit_bound_element_damped, with
// v_{n+1/2} gathered and formed as the damped element pass does it -- hh from the host or, with clk, half of the clock's
// h_next, read before k_explicit_clock ticks.  Without it the kernel has the code it always had.  kappa: the sum of the
// penalties of the integrator's rigid walls, added to omega_e^2 before the damping factor; an argument the kernel always
// takes, 0 without walls, when nothing is added and the bits are those of a kernel without it.
struct BoundDamping {
    const double *vel, *accv;
    ExplicitDamping d;
    double hh;
    const ExplicitClock* clk;
};
template <int NPE, int DM, class... DAMPING>
__global__ void __launch_bounds__(XBS) k_explicit_bound(int32_t ne, int32_t nGP, const double* __restrict__ nodes,
                                                        const double* __restrict__ u, const int32_t* __restrict__ elems,
                                                        const double* __restrict__ dN, const double* __restrict__ w,
                                                        int mat_kind, const double* __restrict__ C, double p0, double p1,
                                                        const double* __restrict__ me_in, double s_C, double kappa,
                                                        double* __restrict__ part, DAMPING... damping) {
    constexpr bool DAMP = sizeof...(DAMPING) == 1;
    static_assert(sizeof...(DAMPING) <= 1, "at most one damping argument");
    __shared__ double sm[XBS / 64];
    const int32_t e = blockIdx.x * blockDim.x + threadIdx.x;
    double best = 0.0;
    if (e < ne) {
        double X[NPE][DM], U[NPE][DM], me[NPE], g, w2;
        [[maybe_unused]] double Vh[DAMP ? NPE : 1][DM];
#pragma unroll
        for (int a = 0; a < NPE; ++a) {
            const int32_t nd = elems[(int64_t)e * NPE + a];
            load_row<DM>(nodes + (int64_t)nd * DM, X[a]);
            load_row<DM>(u + (int64_t)nd * DM, U[a]);
            me[a] = me_in[(int64_t)e * NPE + a];
            if constexpr (DAMP) {
                const BoundDamping& dp = (damping, ...);
                load_row<DM>(dp.vel + (int64_t)nd * DM, Vh[a]);
                if (dp.accv) {
                    double A[DM];
                    load_row<DM>(dp.accv + (int64_t)nd * DM, A);
                    const double hh = dp.clk ? 0.5 * dp.clk->h_next : dp.hh;
#pragma unroll
                    for (int i = 0; i < DM; ++i) Vh[a][i] = explicit_vhalf(Vh[a][i], A[i], hh);
                }
            }
        }
        if constexpr (DAMP)
            explicit_bound_element_damped<NPE, DM>(X, U, Vh, (damping, ...).d, nGP, dN, w, mat_kind, C, p0, p1, me, s_C, g, w2,
                                                   kappa);
        else
            explicit_bound_element<NPE, DM>(X, U, nGP, dN, w, mat_kind, C, p0, p1, me, s_C, g, w2, kappa);
        best = w2 != w2 ? INFINITY : w2;
    }
    const double r = block_reduce<true>(best, sm);
    if (threadIdx.x == 0) part[blockIdx.x] = r;
}

// one workgroup: the maximum of the np partials (reduce_partials), and one tick of the clock by thread 0 (element_math.hpp:
// explicit_clock_tick)
__global__ void __launch_bounds__(XBS) k_explicit_clock(int np, const double* __restrict__ part, ExplicitClock* __restrict__ clk) {
    __shared__ double sm[XBS / 64];
    const double r = reduce_partials<true>(np, part, sm);
    if (threadIdx.x == 0) {
        ExplicitClock c = *clk;
        explicit_clock_tick(c, r);
        *clk = c;
    }
}

// ------------------------------------------------------------------------------- fixed mass scaling
// The factors of femcy_lumped_mass_scale, one thread per element in the launch shape of k_explicit_bound: omega_e^2 is
// explicit_bound_element at U = 0 with the element's current shares, the call femcy_explicit_element_bound makes at u = 0, so
// the same bits; k_e is mass_scale_factor (element_math.hpp).  np = gridDim.x partials of each of
//   part[0 .. np)      max omega_e^2, NaN counted as infinity
//   part[np .. 2 np)   max k_e, anything but a finite positive factor counted as infinity
//   part[2 np .. 3 np) the number of elements with k_e != 1 (a sum of 0.0 / 1.0: exact)
// through block_reduce, in a fixed order.  measure: only the first (FEMCY_MS_UNIFORM needs max_e omega_e^2 before any factor
// is known), fac is not written.
template <int NPE, int DM>
__global__ void __launch_bounds__(XBS) k_mass_scale_factors(int32_t ne, int32_t nGP, const double* __restrict__ nodes,
                                                            const int32_t* __restrict__ elems,
                                                            const double* __restrict__ dN, const double* __restrict__ w,
                                                            int mat_kind, const double* __restrict__ C, double p0, double p1,
                                                            const double* __restrict__ me_in, double s_C, double w2max,
                                                            double factor, double tau, int type, bool measure,
                                                            double* __restrict__ fac, double* __restrict__ part) {
    __shared__ double sm[XBS / 64];
    const int32_t e = blockIdx.x * blockDim.x + threadIdx.x;
    double best = 0.0, kbest = 0.0, scaled = 0.0;
    if (e < ne) {
        double X[NPE][DM], U[NPE][DM], me[NPE], g, w2;
#pragma unroll
        for (int a = 0; a < NPE; ++a) {
            load_row<DM>(nodes + (int64_t)elems[(int64_t)e * NPE + a] * DM, X[a]);
#pragma unroll
            for (int i = 0; i < DM; ++i) U[a][i] = 0.0;
            me[a] = me_in[(int64_t)e * NPE + a];
        }
        explicit_bound_element<NPE, DM>(X, U, nGP, dN, w, mat_kind, C, p0, p1, me, s_C, g, w2);
        best = mass_scale_nan_to_inf(w2);
        if (!measure) {
            const double k = mass_scale_factor(w2, w2max, factor, tau, type);
            fac[e] = k;
            kbest = mass_scale_bad_to_inf(k);
            scaled = k != 1.0 ? 1.0 : 0.0;
        }
    }
    const int np = gridDim.x;
    const double r = block_reduce<true>(best, sm);
    if (threadIdx.x == 0) part[blockIdx.x] = r;
    if (measure) return;
    const double rk = block_reduce<true>(kbest, sm);
    const double rs = block_reduce<false>(scaled, sm);
    if (threadIdx.x == 0) {
        part[np + blockIdx.x] = rk;
        part[2 * np + blockIdx.x] = rs;
    }
}

// the apply pass: me[e][a] *= fac[e] over the ne * npe contiguous shares; the thread of a = 0 also carries the element's
// cumulative factor on (first: the first call on this lumped mass, cum is not read)
__global__ void __launch_bounds__(XBS) k_mass_scale_apply(int64_t nshares, int32_t npe, const double* __restrict__ fac,
                                                          bool first, double* __restrict__ me, double* __restrict__ cum) {
    const int64_t i = (int64_t)blockIdx.x * XBS + threadIdx.x;
    if (i >= nshares) return;
    const int64_t e = i / npe;
    const double k = fac[e];
    me[i] *= k;
    if (i == e * npe) cum[e] = first ? k : cum[e] * k;
}

// partial sums of the nodal masses, the pattern of k_explicit_energy: thread t of workgroup b takes the nodes
// b * 256 + t + k * (workgroups * 256), k ascending
__global__ void __launch_bounds__(XBS) k_mass_total(int32_t nn, const double* __restrict__ m, double* __restrict__ part) {
    __shared__ double sm[XBS / 64];
    double acc = 0.0;
    for (int64_t a = (int64_t)blockIdx.x * XBS + threadIdx.x; a < nn; a += (int64_t)gridDim.x * XBS) acc += m[a];
    const double r = block_reduce<false>(acc, sm);
    if (threadIdx.x == 0) part[blockIdx.x] = r;
}

// ------------------------------------------------------------------------------- host launchers
static int reduction_grid(int64_t items) {
    return (int)std::max<int64_t>(1, std::min<int64_t>((items + XBS - 1) / XBS, 1024));   // <= MAX_PARTIALS partials
}

int launch_lumped_mass(Ctx* c, int32_t nq, const double* d_Nq, const double* d_dNq, const double* d_wq, double rho,
                       double* d_me, double* d_m) {
    const int grid = (c->ne + XBS - 1) / XBS;
    size_t tm = timing_begin(c, T_GEOM);
    const bool launched = dispatch_element(c->npe, c->dm, [&](auto npe, auto dm) {
        hipLaunchKernelGGL((k_lumped_elem<npe(), dm()>), dim3(grid), dim3(XBS), 0, c->stream, c->ne, nq, c->d_nodes,
                           c->d_elems, d_Nq, d_dNq, d_wq, rho, d_me);
    });
    if (launched) launch_node_sum(c, d_me, d_m);
    timing_end(c, tm);
    if (!launched) {
        set_error("no lumped-mass kernel instantiated for npe=%d dm=%d", c->npe, c->dm);
        return FEMCY_ENOKERNEL;
    }
    FEMCY_HIP(hipGetLastError());
    return FEMCY_OK;
}

int launch_explicit_minv(Ctx* c, const double* d_m, double* d_minv) {
    const unsigned grid = (unsigned)((c->n + XBS - 1) / XBS);
    dispatch_dm(c->dm, [&](auto dm) {
        hipLaunchKernelGGL((k_explicit_minv<dm()>), dim3(grid), dim3(XBS), 0, c->stream, c->n, d_m, d_minv);
    });
    FEMCY_HIP(hipGetLastError());
    return FEMCY_OK;
}

int explicit_energy_slots(const Ctx* c) { return (int)node_gather_grid(c->nn, XBS) * (XBS / 64); }

// the energy variants of the four node-pass launches below, on the same grid
static void launch_explicit_node_energy(Ctx* c, unsigned grid, const double* d_minv, const double* d_f,
                                        const ExplicitClock* d_clk, double scale, double h, int mode, double alpha,
                                        const ExplicitMotion* mv, const ExplicitEnergy& e, const ExplicitWalls* wl) {
    double *u = c->d_vec[FEMCY_VEC_DOF], *v = c->d_vec[FEMCY_VEC_VEL], *a = c->d_vec[FEMCY_VEC_ACC];
    const NodeEnergy en{e.d_m, e.d_fint, e.d_falpha, e.d_slot};
    dispatch_dm(c->dm, [&](auto dm) {
        if (wl) {
            const NodeWall nw{c->d_nodes.get(), *wl};
            if (mv) {
                const NodeMotion mo{mv->d_slot, mv->d_curve, mv->d_val, mv->d_amp, mv->t, mv->t_drift};
                if (d_clk)
                    hipLaunchKernelGGL((k_explicit_node_auto_energy<dm(), NodeMotion, NodeWall>), dim3(grid), dim3(XBS), 0,
                                       c->stream, c->nn, c->d_ne_ptr, c->d_ne_idx, c->d_fe, d_f, d_minv, d_clk, mode, alpha, u, v,
                                       a, en, mo, nw);
                else
                    hipLaunchKernelGGL((k_explicit_node_energy<dm(), NodeMotion, NodeWall>), dim3(grid), dim3(XBS), 0, c->stream,
                                       c->nn, c->d_ne_ptr, c->d_ne_idx, c->d_fe, d_f, d_minv,
                                       explicit_step_fixed(scale, h, mode, alpha), mode, u, v, a, en, mo, nw);
            } else if (d_clk)
                hipLaunchKernelGGL((k_explicit_node_auto_energy<dm(), NodeWall>), dim3(grid), dim3(XBS), 0, c->stream, c->nn,
                                   c->d_ne_ptr, c->d_ne_idx, c->d_fe, d_f, d_minv, d_clk, mode, alpha, u, v, a, en, nw);
            else
                hipLaunchKernelGGL((k_explicit_node_energy<dm(), NodeWall>), dim3(grid), dim3(XBS), 0, c->stream, c->nn,
                                   c->d_ne_ptr, c->d_ne_idx, c->d_fe, d_f, d_minv, explicit_step_fixed(scale, h, mode, alpha),
                                   mode, u, v, a, en, nw);
        } else if (mv) {
            const NodeMotion mo{mv->d_slot, mv->d_curve, mv->d_val, mv->d_amp, mv->t, mv->t_drift};
            if (d_clk)
                hipLaunchKernelGGL((k_explicit_node_auto_energy<dm(), NodeMotion>), dim3(grid), dim3(XBS), 0, c->stream, c->nn,
                                   c->d_ne_ptr, c->d_ne_idx, c->d_fe, d_f, d_minv, d_clk, mode, alpha, u, v, a, en, mo);
            else
                hipLaunchKernelGGL((k_explicit_node_energy<dm(), NodeMotion>), dim3(grid), dim3(XBS), 0, c->stream, c->nn,
                                   c->d_ne_ptr, c->d_ne_idx, c->d_fe, d_f, d_minv, explicit_step_fixed(scale, h, mode, alpha),
                                   mode, u, v, a, en, mo);
        } else if (d_clk)
            hipLaunchKernelGGL((k_explicit_node_auto_energy<dm()>), dim3(grid), dim3(XBS), 0, c->stream, c->nn, c->d_ne_ptr,
                               c->d_ne_idx, c->d_fe, d_f, d_minv, d_clk, mode, alpha, u, v, a, en);
        else
            hipLaunchKernelGGL((k_explicit_node_energy<dm()>), dim3(grid), dim3(XBS), 0, c->stream, c->nn, c->d_ne_ptr,
                               c->d_ne_idx, c->d_fe, d_f, d_minv, explicit_step_fixed(scale, h, mode, alpha), mode, u, v, a, en);
    });
}

int launch_explicit_energy_sum(Ctx* c, const double* d_slot, double* out) {
    hipLaunchKernelGGL(k_explicit_energy_sum, dim3(4), dim3(XBS), 0, c->stream, explicit_energy_slots(c), d_slot, c->d_part2);
    FEMCY_HIP(hipGetLastError());
    FEMCY_HIP(hipMemcpyAsync(c->h_scalar, c->d_part2, sizeof(double) * 4, hipMemcpyDeviceToHost, c->stream));
    FEMCY_HIP(hipStreamSynchronize(c->stream));
    for (int k = 0; k < 4; ++k) out[k] = c->h_scalar[k];
    return FEMCY_OK;
}

int launch_explicit_node(Ctx* c, const double* d_minv, const double* d_f, const ExplicitClock* d_clk, double scale, double h,
                         int mode, double alpha, const ExplicitMotion* mv, const ExplicitEnergy* en, const ExplicitWalls* wl) {
    const unsigned grid = node_gather_grid(c->nn, XBS);
    double *u = c->d_vec[FEMCY_VEC_DOF], *v = c->d_vec[FEMCY_VEC_VEL], *a = c->d_vec[FEMCY_VEC_ACC];
    size_t tm = timing_begin(c, T_FORCE);
    if (en) {
        launch_explicit_node_energy(c, grid, d_minv, d_f, d_clk, scale, h, mode, alpha, mv, *en, wl);
        timing_end(c, tm);
        FEMCY_HIP(hipGetLastError());
        return FEMCY_OK;
    }
    dispatch_dm(c->dm, [&](auto dm) {
        if (wl) {
            const NodeWall nw{c->d_nodes.get(), *wl};
            if (mv) {
                const NodeMotion mo{mv->d_slot, mv->d_curve, mv->d_val, mv->d_amp, mv->t, mv->t_drift};
                if (d_clk)
                    hipLaunchKernelGGL((k_explicit_node_auto<dm(), NodeMotion, NodeWall>), dim3(grid), dim3(XBS), 0, c->stream,
                                       c->nn, c->d_ne_ptr, c->d_ne_idx, c->d_fe, d_f, d_minv, d_clk, mode, alpha, u, v, a, mo, nw);
                else
                    hipLaunchKernelGGL((k_explicit_node<dm(), NodeMotion, NodeWall>), dim3(grid), dim3(XBS), 0, c->stream, c->nn,
                                       c->d_ne_ptr, c->d_ne_idx, c->d_fe, d_f, d_minv,
                                       explicit_step_fixed(scale, h, mode, alpha), mode, u, v, a, mo, nw);
            } else if (d_clk)
                hipLaunchKernelGGL((k_explicit_node_auto<dm(), NodeWall>), dim3(grid), dim3(XBS), 0, c->stream, c->nn,
                                   c->d_ne_ptr, c->d_ne_idx, c->d_fe, d_f, d_minv, d_clk, mode, alpha, u, v, a, nw);
            else
                hipLaunchKernelGGL((k_explicit_node<dm(), NodeWall>), dim3(grid), dim3(XBS), 0, c->stream, c->nn, c->d_ne_ptr,
                                   c->d_ne_idx, c->d_fe, d_f, d_minv, explicit_step_fixed(scale, h, mode, alpha), mode, u, v, a,
                                   nw);
        } else if (mv) {
            const NodeMotion mo{mv->d_slot, mv->d_curve, mv->d_val, mv->d_amp, mv->t, mv->t_drift};
            if (d_clk)
                hipLaunchKernelGGL((k_explicit_node_auto<dm(), NodeMotion>), dim3(grid), dim3(XBS), 0, c->stream, c->nn,
                                   c->d_ne_ptr, c->d_ne_idx, c->d_fe, d_f, d_minv, d_clk, mode, alpha, u, v, a, mo);
            else
                hipLaunchKernelGGL((k_explicit_node<dm(), NodeMotion>), dim3(grid), dim3(XBS), 0, c->stream, c->nn, c->d_ne_ptr,
                                   c->d_ne_idx, c->d_fe, d_f, d_minv, explicit_step_fixed(scale, h, mode, alpha), mode, u, v, a,
                                   mo);
        } else if (d_clk)
            hipLaunchKernelGGL((k_explicit_node_auto<dm()>), dim3(grid), dim3(XBS), 0, c->stream, c->nn, c->d_ne_ptr,
                               c->d_ne_idx, c->d_fe, d_f, d_minv, d_clk, mode, alpha, u, v, a);
        else
            hipLaunchKernelGGL((k_explicit_node<dm()>), dim3(grid), dim3(XBS), 0, c->stream, c->nn, c->d_ne_ptr, c->d_ne_idx,
                               c->d_fe, d_f, d_minv, explicit_step_fixed(scale, h, mode, alpha), mode, u, v, a);
    });
    timing_end(c, tm);
    FEMCY_HIP(hipGetLastError());
    return FEMCY_OK;
}

int launch_explicit_place(Ctx* c, const ExplicitMotion& mv, const ExplicitClock* d_clk, double t, int what) {
    if (mv.nmoved == 0) return FEMCY_OK;
    const unsigned grid = (unsigned)((mv.nmoved + XBS - 1) / XBS);
    hipLaunchKernelGGL(k_explicit_place, dim3(grid), dim3(XBS), 0, c->stream, mv.nmoved, mv.d_dof, mv.d_val, mv.d_curve,
                       mv.d_amp, d_clk, t, what, c->d_vec[FEMCY_VEC_DOF].get(), c->d_vec[FEMCY_VEC_VEL].get(),
                       c->d_vec[FEMCY_VEC_ACC].get());
    FEMCY_HIP(hipGetLastError());
    return FEMCY_OK;
}

int launch_explicit_drift(Ctx* c, const ExplicitClock* d_clk, double h) {
    const unsigned grid = (unsigned)((c->n + XBS - 1) / XBS);
    double *u = c->d_vec[FEMCY_VEC_DOF], *v = c->d_vec[FEMCY_VEC_VEL], *a = c->d_vec[FEMCY_VEC_ACC];
    size_t tm = timing_begin(c, T_FORCE);
    if (d_clk)
        hipLaunchKernelGGL(k_explicit_drift_auto, dim3(grid), dim3(XBS), 0, c->stream, c->n, d_clk, v, a, u);
    else
        hipLaunchKernelGGL(k_explicit_drift, dim3(grid), dim3(XBS), 0, c->stream, c->n, h, 0.5 * h * h, v, a, u);
    timing_end(c, tm);
    FEMCY_HIP(hipGetLastError());
    return FEMCY_OK;
}

static int fetch_scalar(Ctx* c, const double* d_val, double* out) {
    FEMCY_HIP(hipMemcpyAsync(c->h_scalar, d_val, sizeof(double), hipMemcpyDeviceToHost, c->stream));
    FEMCY_HIP(hipStreamSynchronize(c->stream));
    *out = c->h_scalar[0];
    return FEMCY_OK;
}

int launch_explicit_energy(Ctx* c, const double* d_m, const double* d_v, double* out) {
    const int g = reduction_grid(c->nn);
    dispatch_dm(c->dm, [&](auto dm) {
        hipLaunchKernelGGL((k_explicit_energy<dm()>), dim3(g), dim3(XBS), 0, c->stream, c->nn, d_m, d_v, c->d_part1);
    });
    hipLaunchKernelGGL((k_explicit_final<false>), dim3(1), dim3(XBS), 0, c->stream, g, c->d_part1, c->d_part2);
    FEMCY_HIP(hipGetLastError());
    double s = 0.0;
    int rc = fetch_scalar(c, c->d_part2, &s);
    *out = 0.5 * s;
    return rc;
}

int launch_explicit_wall_get(Ctx* c, const ExplicitWalls& wl, int k, const double* d_m, const double* d_minv, double* out) {
    const int g = reduction_grid(c->nn);        // 4 g <= MAX_PARTIALS partials
    dispatch_dm(c->dm, [&](auto dm) {
        hipLaunchKernelGGL((k_explicit_wall<dm()>), dim3(g), dim3(XBS), 0, c->stream, c->nn, c->d_nodes.get(),
                           c->d_vec[FEMCY_VEC_DOF].get(), d_m, d_minv, wl, k, c->d_part1);
    });
    double* res = c->d_part2;
    for (int j = 0; j < 3; ++j)
        hipLaunchKernelGGL((k_explicit_final<false>), dim3(1), dim3(XBS), 0, c->stream, g, c->d_part1.get() + (size_t)j * g, res + j);
    hipLaunchKernelGGL((k_explicit_final<true>), dim3(1), dim3(XBS), 0, c->stream, g, c->d_part1.get() + 3 * (size_t)g, res + 3);
    FEMCY_HIP(hipGetLastError());
    FEMCY_HIP(hipMemcpyAsync(c->h_scalar, res, sizeof(double) * 4, hipMemcpyDeviceToHost, c->stream));
    FEMCY_HIP(hipStreamSynchronize(c->stream));
    for (int j = 0; j < 4; ++j) out[j] = c->h_scalar[j];
    return FEMCY_OK;
}

int launch_rowabs_bound(Ctx* c, const double* d_minv, double* out) {
    const int64_t npos = (int64_t)c->nslices * SLICE;
    const int g = reduction_grid(npos);
    dispatch_dm(c->dm, [&](auto dm) {
        hipLaunchKernelGGL((k_rowabs_bound<dm()>), dim3(g), dim3(XBS), 0, c->stream, npos, c->d_node_of, c->d_rowlen,
                           c->d_slice_off, c->d_Kvals, d_minv, c->d_part1);
    });
    hipLaunchKernelGGL((k_explicit_final<true>), dim3(1), dim3(XBS), 0, c->stream, g, c->d_part1, c->d_part2);
    FEMCY_HIP(hipGetLastError());
    return fetch_scalar(c, c->d_part2, out);
}

int explicit_bound_partials(const Ctx* c) { return (c->ne + XBS - 1) / XBS; }

int launch_explicit_bound(Ctx* c, const double* d_u, const double* d_me, double s_C, double* d_part, const GeomDamping* gd,
                          double kappa) {
    const int grid = explicit_bound_partials(c);
    size_t tm = timing_begin(c, T_GEOM);
    const bool launched = dispatch_element(c->npe, c->dm, [&](auto npe, auto dm) {
        if (gd)
            hipLaunchKernelGGL((k_explicit_bound<npe(), dm(), BoundDamping>), dim3(grid), dim3(XBS), 0, c->stream, c->ne,
                               c->nGP, c->d_nodes, d_u, c->d_elems, c->d_dN, c->d_w, c->mat_kind, c->d_C, c->mat_params[0],
                               c->mat_params[1], d_me, s_C, kappa, d_part,
                               BoundDamping{gd->d_v, gd->d_a, {gd->alpha, gd->b1, gd->b2, gd->Md, gd->rho0}, 0.5 * gd->h,
                                            gd->d_clk});
        else
            hipLaunchKernelGGL((k_explicit_bound<npe(), dm()>), dim3(grid), dim3(XBS), 0, c->stream, c->ne, c->nGP, c->d_nodes, d_u,
                           c->d_elems, c->d_dN, c->d_w, c->mat_kind, c->d_C, c->mat_params[0], c->mat_params[1], d_me, s_C,
                           kappa, d_part);
    });
    timing_end(c, tm);
    if (!launched) {
        set_error("no element-bound kernel instantiated for npe=%d dm=%d", c->npe, c->dm);
        return FEMCY_ENOKERNEL;
    }
    FEMCY_HIP(hipGetLastError());
    return FEMCY_OK;
}

int launch_explicit_bound_max(Ctx* c, const double* d_part, double* out) {
    hipLaunchKernelGGL((k_explicit_final<true>), dim3(1), dim3(XBS), 0, c->stream, explicit_bound_partials(c), d_part,
                       c->d_part2);
    FEMCY_HIP(hipGetLastError());
    return fetch_scalar(c, c->d_part2, out);
}

int launch_explicit_clock(Ctx* c, const double* d_part, ExplicitClock* d_clk) {
    hipLaunchKernelGGL(k_explicit_clock, dim3(1), dim3(XBS), 0, c->stream, explicit_bound_partials(c), d_part, d_clk);
    FEMCY_HIP(hipGetLastError());
    return FEMCY_OK;
}

int launch_mass_total(Ctx* c, const double* d_m, double* out) {
    const int g = reduction_grid(c->nn);
    hipLaunchKernelGGL(k_mass_total, dim3(g), dim3(XBS), 0, c->stream, c->nn, d_m, c->d_part1);
    hipLaunchKernelGGL((k_explicit_final<false>), dim3(1), dim3(XBS), 0, c->stream, g, c->d_part1, c->d_part2);
    FEMCY_HIP(hipGetLastError());
    return fetch_scalar(c, c->d_part2, out);
}

int launch_mass_scale_factors(Ctx* c, const double* d_me, double s_C, double w2max, double factor, double tau, int type,
                              bool measure, double* d_fac, double* d_part, double* out) {
    const int np = explicit_bound_partials(c);
    size_t tm = timing_begin(c, T_GEOM);
    const bool launched = dispatch_element(c->npe, c->dm, [&](auto npe, auto dm) {
        hipLaunchKernelGGL((k_mass_scale_factors<npe(), dm()>), dim3(np), dim3(XBS), 0, c->stream, c->ne, c->nGP, c->d_nodes,
                           c->d_elems, c->d_dN, c->d_w, c->mat_kind, c->d_C, c->mat_params[0], c->mat_params[1], d_me, s_C,
                           w2max, factor, tau, type, measure, d_fac, d_part);
    });
    timing_end(c, tm);
    if (!launched) {
        set_error("no mass-scaling kernel instantiated for npe=%d dm=%d", c->npe, c->dm);
        return FEMCY_ENOKERNEL;
    }
    double* res = c->d_part2;
    hipLaunchKernelGGL((k_explicit_final<true>), dim3(1), dim3(XBS), 0, c->stream, np, d_part, res);
    if (!measure) {
        hipLaunchKernelGGL((k_explicit_final<true>), dim3(1), dim3(XBS), 0, c->stream, np, d_part + np, res + 1);
        hipLaunchKernelGGL((k_explicit_final<false>), dim3(1), dim3(XBS), 0, c->stream, np, d_part + 2 * (size_t)np, res + 2);
    }
    FEMCY_HIP(hipGetLastError());
    const int nres = measure ? 1 : 3;
    FEMCY_HIP(hipMemcpyAsync(c->h_scalar, res, sizeof(double) * nres, hipMemcpyDeviceToHost, c->stream));
    FEMCY_HIP(hipStreamSynchronize(c->stream));
    for (int k = 0; k < nres; ++k) out[k] = c->h_scalar[k];
    return FEMCY_OK;
}

int launch_mass_scale_apply(Ctx* c, const double* d_fac, bool first, double* d_me, double* d_cum, double* d_m) {
    const int64_t nshares = (int64_t)c->ne * c->npe;
    const unsigned grid = (unsigned)((nshares + XBS - 1) / XBS);
    hipLaunchKernelGGL(k_mass_scale_apply, dim3(grid), dim3(XBS), 0, c->stream, nshares, c->npe, d_fac, first, d_me, d_cum);
    launch_node_sum(c, d_me, d_m);
    FEMCY_HIP(hipGetLastError());
    return FEMCY_OK;
}

}  // namespace femcy
