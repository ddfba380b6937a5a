// The arithmetic of one element / one Gauss point / one facet of the path, defined ONCE for both backends of the C ABI:
// the HIP kernels (kernels_assembly.hip) and the host implementation (csrc_cpu/femcy_cpu.cpp) include this header, so
// the two cannot drift apart.  Everything here is a pure function of its arguments (no memory layout, no threading).
// References (paths relative to the FEMcy checkout) are given at each function.
#pragma once
#include <cmath>
#include <stdint.h>
#include "../../include/femcy.h"

#if defined(__HIPCC__)
#define FEMCY_HD __host__ __device__ __forceinline__
#else
#define FEMCY_HD inline
#endif

namespace femcy {

// ------------------------------------------------------------------------------ small matrices
template <int DM>
FEMCY_HD double det_inv(const double (&J)[DM][DM], double (&inv)[DM][DM]);

template <>
FEMCY_HD double det_inv<2>(const double (&J)[2][2], double (&inv)[2][2]) {
    double det = J[0][0] * J[1][1] - J[0][1] * J[1][0];
    double id = 1.0 / det;
    inv[0][0] = J[1][1] * id;
    inv[0][1] = -J[0][1] * id;
    inv[1][0] = -J[1][0] * id;
    inv[1][1] = J[0][0] * id;
    return det;
}

template <>
FEMCY_HD double det_inv<3>(const double (&J)[3][3], double (&inv)[3][3]) {
    double c00 = J[1][1] * J[2][2] - J[1][2] * J[2][1];
    double c01 = J[1][2] * J[2][0] - J[1][0] * J[2][2];
    double c02 = J[1][0] * J[2][1] - J[1][1] * J[2][0];
    double det = J[0][0] * c00 + J[0][1] * c01 + J[0][2] * c02;
    double id = 1.0 / det;
    inv[0][0] = c00 * id;
    inv[1][0] = c01 * id;
    inv[2][0] = c02 * id;
    inv[0][1] = (J[0][2] * J[2][1] - J[0][1] * J[2][2]) * id;
    inv[1][1] = (J[0][0] * J[2][2] - J[0][2] * J[2][0]) * id;
    inv[2][1] = (J[0][1] * J[2][0] - J[0][0] * J[2][1]) * id;
    inv[0][2] = (J[0][1] * J[1][2] - J[0][2] * J[1][1]) * id;
    inv[1][2] = (J[0][2] * J[1][0] - J[0][0] * J[1][2]) * id;
    inv[2][2] = (J[0][0] * J[1][1] - J[0][1] * J[1][0]) * id;
    return det;
}

FEMCY_HD double det3(const double (&A)[3][3]) {
    return A[0][0] * (A[1][1] * A[2][2] - A[1][2] * A[2][1]) - A[0][1] * (A[1][0] * A[2][2] - A[1][2] * A[2][0]) +
           A[0][2] * (A[1][0] * A[2][1] - A[1][1] * A[2][0]);
}

// sigma = F S F^T / J for a 3x3 F and symmetric S given in Voigt order [xx,yy,zz,xy,zx,yz]
FEMCY_HD void push_forward3(const double (&F)[3][3], const double (&sv)[6], double (&sig)[3][3]) {
    double S[3][3] = {{sv[0], sv[3], sv[4]}, {sv[3], sv[1], sv[5]}, {sv[4], sv[5], sv[2]}};
    double FS[3][3];
#pragma unroll
    for (int i = 0; i < 3; ++i)
#pragma unroll
        for (int j = 0; j < 3; ++j) FS[i][j] = F[i][0] * S[0][j] + F[i][1] * S[1][j] + F[i][2] * S[2][j];
    double J = det3(F);
#pragma unroll
    for (int i = 0; i < 3; ++i)
#pragma unroll
        for (int j = 0; j < 3; ++j) sig[i][j] = (FS[i][0] * F[j][0] + FS[i][1] * F[j][1] + FS[i][2] * F[j][2]) / J;
}

// Green strain of a 3x3 F in Voigt order with engineering shear
FEMCY_HD void green_voigt3(const double (&F)[3][3], double (&ev)[6]) {
    double E[3][3];
#pragma unroll
    for (int i = 0; i < 3; ++i)
#pragma unroll
        for (int j = 0; j < 3; ++j)
            E[i][j] = (F[0][i] * F[0][j] + F[1][i] * F[1][j] + F[2][i] * F[2][j] - (i == j ? 1.0 : 0.0)) / 2.0;
    ev[0] = E[0][0];
    ev[1] = E[1][1];
    ev[2] = E[2][2];
    ev[3] = 2.0 * E[0][1];
    ev[4] = 2.0 * E[2][0];
    ev[5] = 2.0 * E[1][2];
}

// constitutiveOfLargeDeform: linear_isotropic.py:55-76, linear_isotropic_plane_strain.py:66-86,
// linear_isotropic_plane_stress.py:65-96, neo_hookean.py:66-77.  C is the per-Gauss-point ddsdde
// (a constant copy of material.C in the reference).
template <int DM>
FEMCY_HD void cauchy_large(int kind, const double* __restrict__ C, double p0, double p1,
                                             const double (&F)[DM][DM], double (&sig)[DM][DM]);

template <>
FEMCY_HD void cauchy_large<3>(int kind, const double* __restrict__ C, double p0, double p1,
                                                const double (&F)[3][3], double (&sig)[3][3]) {
    if (kind == FEMCY_MAT_NEOHOOKE) {
        double J = det3(F);
#pragma unroll
        for (int i = 0; i < 3; ++i)
#pragma unroll
            for (int j = 0; j < 3; ++j) {
                double B = F[i][0] * F[j][0] + F[i][1] * F[j][1] + F[i][2] * F[j][2];
                double eye = (i == j) ? 1.0 : 0.0;
                sig[i][j] = 2.0 * p0 / J * (B - eye) + 2.0 * p1 * (J - 1.0) * eye;
            }
    } else {
        double ev[6], sv[6];
        green_voigt3(F, ev);
#pragma unroll
        for (int p = 0; p < 6; ++p) {
            double a = 0.0;
#pragma unroll
            for (int q = 0; q < 6; ++q) a += C[p * 6 + q] * ev[q];
            sv[p] = a;
        }
        push_forward3(F, sv, sig);
    }
}

template <>
FEMCY_HD void cauchy_large<2>(int kind, const double* __restrict__ C, double p0, double p1,
                                                const double (&F)[2][2], double (&sig)[2][2]) {
    if (kind == FEMCY_MAT_NEOHOOKE) {
        // plane-strain neo-Hookean (extension: the reference has the 3-D form only, neo_hookean.py:66-77, and its
        // reader rejects it on 2-D elements): F33 = 1, so the in-plane part of the 3-D expression with J = det F
        const double J = F[0][0] * F[1][1] - F[0][1] * F[1][0];
#pragma unroll
        for (int i = 0; i < 2; ++i)
#pragma unroll
            for (int j = 0; j < 2; ++j) {
                const double B = F[i][0] * F[j][0] + F[i][1] * F[j][1];
                const double eye = (i == j) ? 1.0 : 0.0;
                sig[i][j] = 2.0 * p0 / J * (B - eye) + 2.0 * p1 * (J - 1.0) * eye;
            }
    } else if (kind == FEMCY_MAT_PSTRESS) {
        // F embedded in 3-D with F33 = 1 - nu/(1-nu) (F00 + F11 - 2); uses C_6x6, not ddsdde
        const double E = p0, nu = p1;
        double F3[3][3] = {{F[0][0], F[0][1], 0.0}, {F[1][0], F[1][1], 0.0}, {0.0, 0.0, 0.0}};
        F3[2][2] = -nu / (1.0 - nu) * (F[0][0] + F[1][1] - 2.0) + 1.0;
        double ev[6], sv[6], s3[3][3];
        green_voigt3(F3, ev);
        const double G = E / 2.0 / (1.0 + nu);
        const double c00 = E / (1.0 - nu * nu), c01 = c00 * nu;
        sv[0] = c00 * ev[0] + c01 * ev[1];
        sv[1] = c01 * ev[0] + c00 * ev[1];
        sv[2] = 0.0;
        sv[3] = G * ev[3];
        sv[4] = 0.0;
        sv[5] = 0.0;
        push_forward3(F3, sv, s3);
        sig[0][0] = s3[0][0];
        sig[0][1] = s3[0][1];
        sig[1][0] = s3[1][0];
        sig[1][1] = s3[1][1];
    } else {
        double E2[2][2];
#pragma unroll
        for (int i = 0; i < 2; ++i)
#pragma unroll
            for (int j = 0; j < 2; ++j) E2[i][j] = (F[0][i] * F[0][j] + F[1][i] * F[1][j] - (i == j ? 1.0 : 0.0)) / 2.0;
        double ev[3] = {E2[0][0], E2[1][1], E2[0][1] + E2[1][0]}, sv[3];
#pragma unroll
        for (int p = 0; p < 3; ++p) sv[p] = C[p * 3 + 0] * ev[0] + C[p * 3 + 1] * ev[1] + C[p * 3 + 2] * ev[2];
        double S[2][2] = {{sv[0], sv[2]}, {sv[2], sv[1]}}, FS[2][2];
#pragma unroll
        for (int i = 0; i < 2; ++i)
#pragma unroll
            for (int j = 0; j < 2; ++j) FS[i][j] = F[i][0] * S[0][j] + F[i][1] * S[1][j];
        double J = F[0][0] * F[1][1] - F[0][1] * F[1][0];
#pragma unroll
        for (int i = 0; i < 2; ++i)
#pragma unroll
            for (int j = 0; j < 2; ++j) sig[i][j] = (FS[i][0] * F[j][0] + FS[i][1] * F[j][1]) / J;
    }
}

// ---------------------------------------------------------------------- B_a^T C B_b * vol blocks
template <int DM>
FEMCY_HD void kblock_add(const double* __restrict__ ga, const double* __restrict__ gb,
                                           const double* __restrict__ C, double v, double (&acc)[DM * DM]);

template <>
FEMCY_HD void kblock_add<3>(const double* __restrict__ ga, const double* __restrict__ gb,
                                              const double* __restrict__ C, double v, double (&acc)[9]) {
    const double a0 = ga[0], a1 = ga[1], a2 = ga[2], b0 = gb[0], b1 = gb[1], b2 = gb[2];
    double CB[6][3];   // C . B_b, non-zeros of B_b only, ascending Voigt index
#pragma unroll
    for (int p = 0; p < 6; ++p) {
        CB[p][0] = C[p * 6 + 0] * b0 + C[p * 6 + 3] * b1 + C[p * 6 + 4] * b2;
        CB[p][1] = C[p * 6 + 1] * b1 + C[p * 6 + 3] * b0 + C[p * 6 + 5] * b2;
        CB[p][2] = C[p * 6 + 2] * b2 + C[p * 6 + 4] * b0 + C[p * 6 + 5] * b1;
    }
#pragma unroll
    for (int k = 0; k < 3; ++k) {
        acc[0 * 3 + k] += (a0 * CB[0][k] + a1 * CB[3][k] + a2 * CB[4][k]) * v;
        acc[1 * 3 + k] += (a1 * CB[1][k] + a0 * CB[3][k] + a2 * CB[5][k]) * v;
        acc[2 * 3 + k] += (a2 * CB[2][k] + a0 * CB[4][k] + a1 * CB[5][k]) * v;
    }
}

template <>
FEMCY_HD void kblock_add<2>(const double* __restrict__ ga, const double* __restrict__ gb,
                                              const double* __restrict__ C, double v, double (&acc)[4]) {
    const double a0 = ga[0], a1 = ga[1], b0 = gb[0], b1 = gb[1];
    double CB[3][2];
#pragma unroll
    for (int p = 0; p < 3; ++p) {
        CB[p][0] = C[p * 3 + 0] * b0 + C[p * 3 + 2] * b1;
        CB[p][1] = C[p * 3 + 1] * b1 + C[p * 3 + 2] * b0;
    }
#pragma unroll
    for (int k = 0; k < 2; ++k) {
        acc[0 * 2 + k] += (a0 * CB[0][k] + a1 * CB[2][k]) * v;
        acc[1 * 2 + k] += (a1 * CB[1][k] + a0 * CB[2][k]) * v;
    }
}

// consistent tangent block (FEMCY_OPT_TANGENT = 1), updated-Lagrangian form:
//   K_ab[i][k] = vol * ( gradN_a[j] c_ijkl gradN_b[l]  +  delta_ik gradN_a . sigma . gradN_b )
// with the spatial elasticity tensor c = (1/J) push-forward of dS/dE:
//   StVK (S = C:E, isotropic lambda, mu):  c_ijkl = (lambda b_ij b_kl + mu (b_ik b_jl + b_il b_jk)) / J,  b = F F^T
//   neo-Hookean of neo_hookean.py:66-77 (sigma = 2 C1/J (b - I) + 2 D1 (J-1) I):
//                                          c_ijkl = lambda' d_ij d_kl + mu' (d_ik d_jl + d_il d_jk),
//                                          mu' = 2 C1/J - 2 D1 (J-1),  lambda' = 2 D1 (2J-1)
// checked against central differences of femcy_internal_force (tests/test_gpu_tangent.py) and, entry by entry on every
// element family and both branches, against a long-double complex-step derivative (tests/tangent_shapes.py).
template <int DM>
FEMCY_HD void kblock_consistent(const double* __restrict__ ga, const double* __restrict__ gb,
                                                  const double* __restrict__ Fp, const double* __restrict__ Sp,
                                                  bool neo, double lam, double mu, double p0, double p1, double v,
                                                  double (&acc)[DM * DM]) {
    double F[DM][DM];
#pragma unroll
    for (int i = 0; i < DM; ++i)
#pragma unroll
        for (int j = 0; j < DM; ++j) F[i][j] = Fp[i * DM + j];
    double J;
    if constexpr (DM == 3) J = det3(F);
    else J = F[0][0] * F[1][1] - F[0][1] * F[1][0];
    double geo = 0.0;                       // gradN_a . sigma . gradN_b
#pragma unroll
    for (int i = 0; i < DM; ++i)
#pragma unroll
        for (int j = 0; j < DM; ++j) geo += ga[i] * Sp[i * DM + j] * gb[j];
    if (neo) {
        const double mu_s = 2.0 * p0 / J - 2.0 * p1 * (J - 1.0), lam_s = 2.0 * p1 * (2.0 * J - 1.0);
        double ab = 0.0;
#pragma unroll
        for (int i = 0; i < DM; ++i) ab += ga[i] * gb[i];
#pragma unroll
        for (int i = 0; i < DM; ++i)
#pragma unroll
            for (int k = 0; k < DM; ++k)
                acc[i * DM + k] += v * (lam_s * ga[i] * gb[k] + mu_s * gb[i] * ga[k] + (i == k ? mu_s * ab + geo : 0.0));
    } else {
        double b[DM][DM], bga[DM], bgb[DM];
#pragma unroll
        for (int i = 0; i < DM; ++i)
#pragma unroll
            for (int j = 0; j < DM; ++j) {
                double t = 0.0;
#pragma unroll
                for (int m = 0; m < DM; ++m) t += F[i][m] * F[j][m];
                b[i][j] = t;
            }
        double s = 0.0;
#pragma unroll
        for (int i = 0; i < DM; ++i) {
            double ta = 0.0, tb = 0.0;
#pragma unroll
            for (int j = 0; j < DM; ++j) {
                ta += b[i][j] * ga[j];
                tb += b[i][j] * gb[j];
            }
            bga[i] = ta;
            bgb[i] = tb;
        }
#pragma unroll
        for (int i = 0; i < DM; ++i) s += ga[i] * bgb[i];
        const double vj = v / J;
#pragma unroll
        for (int i = 0; i < DM; ++i)
#pragma unroll
            for (int k = 0; k < DM; ++k)
                acc[i * DM + k] += vj * (lam * bga[i] * bgb[k] + mu * (s * b[i][k] + bgb[i] * bga[k])) + (i == k ? v * geo : 0.0);
    }
}

// B_a^T C B_b * v for a C with the cubic sparsity pattern (c11 on the normal diagonal, c12 between normal
// components, c44 on the shear diagonal, zero elsewhere): every material of the reference -- isotropic Hooke
// (c11 = lambda + 2 mu, c12 = lambda, c44 = mu) and the neo-Hookean constant tangent 4 C1 I + 2 D1 1x1 -- has it.
//   K[i][k] = c12 a_i b_k + c44 a_k b_i                     (i != k)
//   K[i][i] = c11 a_i b_i + c44 sum_{j != i} a_j b_j
// 30 multiply-adds instead of the 90 of the dense-pattern evaluation; femcy_set_material detects the pattern with
// exact comparisons and everything else takes kblock_add.
FEMCY_HD void kblock_cubic3(const double* __restrict__ ga, const double* __restrict__ gb, double c11,
                                              double c12, double c44, double v, double (&acc)[9]) {
    const double a0 = ga[0] * v, a1 = ga[1] * v, a2 = ga[2] * v, b0 = gb[0], b1 = gb[1], b2 = gb[2];
    const double p00 = a0 * b0, p11 = a1 * b1, p22 = a2 * b2;
    acc[0] += c11 * p00 + c44 * (p11 + p22);
    acc[4] += c11 * p11 + c44 * (p00 + p22);
    acc[8] += c11 * p22 + c44 * (p00 + p11);
    acc[1] += c12 * (a0 * b1) + c44 * (a1 * b0);
    acc[2] += c12 * (a0 * b2) + c44 * (a2 * b0);
    acc[3] += c12 * (a1 * b0) + c44 * (a0 * b1);
    acc[5] += c12 * (a1 * b2) + c44 * (a2 * b1);
    acc[6] += c12 * (a2 * b0) + c44 * (a0 * b2);
    acc[7] += c12 * (a2 * b1) + c44 * (a1 * b2);
}

// The same block for a material that is the same in every element (c11, c12, c44 are kernel arguments): K_ab is
// linear in the geometric sum S_ab = sum_g |J| w (ga (x) gb), so the row kernels accumulate S over Gauss points AND
// over the incident elements (12 instead of 40 f64 instructions per block and Gauss point) and apply the constants
// once per stored block, when the row is complete: K[i][k] = c12 S[i][k] + c44 S[k][i] (i != k),
// K[i][i] = c11 S[i][i] + c44 (tr S - S[i][i]).
FEMCY_HD void outer3_add(const double* __restrict__ ga, const double* __restrict__ gb, double v, double (&S)[9]) {
    const double a0 = ga[0] * v, a1 = ga[1] * v, a2 = ga[2] * v, b0 = gb[0], b1 = gb[1], b2 = gb[2];
    S[0] += a0 * b0; S[1] += a0 * b1; S[2] += a0 * b2;
    S[3] += a1 * b0; S[4] += a1 * b1; S[5] += a1 * b2;
    S[6] += a2 * b0; S[7] += a2 * b1; S[8] += a2 * b2;
}
FEMCY_HD void cubic_from_outer3(const double (&S)[9], double c11, double c12, double c44, double (&K)[9]) {
    K[0] = c11 * S[0] + c44 * (S[4] + S[8]);
    K[4] = c11 * S[4] + c44 * (S[0] + S[8]);
    K[8] = c11 * S[8] + c44 * (S[0] + S[4]);
    K[1] = c12 * S[1] + c44 * S[3];
    K[3] = c12 * S[3] + c44 * S[1];
    K[2] = c12 * S[2] + c44 * S[6];
    K[6] = c12 * S[6] + c44 * S[2];
    K[5] = c12 * S[5] + c44 * S[7];
    K[7] = c12 * S[7] + c44 * S[5];
}

// ------------------------------------------------------------------------------ post-processing
// compute_strain_stress (stiffnessMtrx.py:436-501), constitutiveOfSmallDeform x4, the three Mises kernels,
// elasticEnergyDensity x4 (material_zoo/*.py), get_elasEng_kernel (:597-606).  One thread per Gauss point.
template <int DM>
FEMCY_HD void cauchy_small(int kind, const double* __restrict__ C, double p0, double p1,
                                             const double (&F)[DM][DM], double (&sig)[DM][DM]);

template <>
FEMCY_HD void cauchy_small<3>(int kind, const double* __restrict__ C, double p0, double p1,
                                                const double (&F)[3][3], double (&sig)[3][3]) {
    if (kind == FEMCY_MAT_NEOHOOKE) {
        cauchy_large<3>(kind, C, p0, p1, F, sig);   // neo_hookean.py:44-60: same expression
        return;
    }
    double E[3][3];
#pragma unroll
    for (int i = 0; i < 3; ++i)
#pragma unroll
        for (int j = 0; j < 3; ++j) E[i][j] = (F[i][j] + F[j][i]) / 2.0 - (i == j ? 1.0 : 0.0);
    const double ev[6] = {E[0][0], E[1][1], E[2][2], 2.0 * E[0][1], 2.0 * E[2][0], 2.0 * E[1][2]};
    double sv[6];
#pragma unroll
    for (int p = 0; p < 6; ++p) {
        double a = 0.0;
#pragma unroll
        for (int q = 0; q < 6; ++q) a += C[p * 6 + q] * ev[q];
        sv[p] = a;
    }
    sig[0][0] = sv[0]; sig[1][1] = sv[1]; sig[2][2] = sv[2];
    sig[0][1] = sig[1][0] = sv[3];
    sig[0][2] = sig[2][0] = sv[4];
    sig[1][2] = sig[2][1] = sv[5];
}

template <>
FEMCY_HD void cauchy_small<2>(int kind, const double* __restrict__ C, double p0, double p1,
                                                const double (&F)[2][2], double (&sig)[2][2]) {
    if (kind == FEMCY_MAT_NEOHOOKE) {
        cauchy_large<2>(kind, C, p0, p1, F, sig);   // as in 3-D: the same expression for small and large deformation
    } else if (kind == FEMCY_MAT_PSTRESS) {
        const double E_ = p0, nu = p1;
        const double F33 = -nu / (1.0 - nu) * (F[0][0] + F[1][1] - 2.0) + 1.0;   // E33 = F33 - 1 multiplies zeros of C_6x6
        (void)F33;
        const double e00 = F[0][0] - 1.0, e11 = F[1][1] - 1.0, g01 = 2.0 * ((F[0][1] + F[1][0]) / 2.0);
        const double G = E_ / 2.0 / (1.0 + nu), c00 = E_ / (1.0 - nu * nu), c01 = c00 * nu;
        sig[0][0] = c00 * e00 + c01 * e11;
        sig[1][1] = c01 * e00 + c00 * e11;
        sig[0][1] = sig[1][0] = G * g01;
    } else {
        const double e00 = F[0][0] - 1.0, e11 = F[1][1] - 1.0;
        const double e01 = (F[0][1] + F[1][0]) / 2.0;
        const double ev[3] = {e00, e11, e01 + e01};
        double v[3];
#pragma unroll
        for (int p = 0; p < 3; ++p) v[p] = C[p * 3 + 0] * ev[0] + C[p * 3 + 1] * ev[1] + C[p * 3 + 2] * ev[2];
        sig[0][0] = v[0];
        sig[1][1] = v[1];
        sig[0][1] = sig[1][0] = v[2];
    }
}

FEMCY_HD double energy_voigt3(const double (&F3)[3][3], const double (&C6)[6][6]) {
    double ev[6];
    green_voigt3(F3, ev);
    double acc = 0.0;
#pragma unroll
    for (int p = 0; p < 6; ++p) {
        double a = 0.0;
#pragma unroll
        for (int q = 0; q < 6; ++q) a += C6[p][q] * ev[q];
        acc += ev[p] * a;
    }
    return acc / 2.0;
}

// energy density of the INFINITESIMAL strain, sigma : eps / 2 with sigma = constitutiveOfSmallDeform(eps) and
// eps = sym(F) - I: the quadratic form u.Ku / 2 per unit reference volume, which is what a linear (small-strain) analysis
// stores and what the Newmark integrator conserves; energy_density below is the reference's energy of the GREEN strain and
// differs from it by the order of the strain.  Linear materials only.
template <int DM>
FEMCY_HD double energy_density_small(int kind, const double* __restrict__ C, double p0, double p1,
                                     const double (&F)[DM][DM]) {
    double sig[DM][DM];
    cauchy_small<DM>(kind, C, p0, p1, F, sig);
    double acc = 0.0;
#pragma unroll
    for (int i = 0; i < DM; ++i)
#pragma unroll
        for (int j = 0; j < DM; ++j) acc += sig[i][j] * ((F[i][j] + F[j][i]) / 2.0 - (i == j ? 1.0 : 0.0));
    return acc / 2.0;
}

template <int DM>
FEMCY_HD double energy_density(int kind, const double* __restrict__ C, double p0, double p1,
                                                 const double (&F)[DM][DM]) {
    double F3[3][3] = {{0, 0, 0}, {0, 0, 0}, {0, 0, 0}}, C6[6][6];
#pragma unroll
    for (int i = 0; i < 6; ++i)
#pragma unroll
        for (int j = 0; j < 6; ++j) C6[i][j] = 0.0;
#pragma unroll
    for (int i = 0; i < DM; ++i)
#pragma unroll
        for (int j = 0; j < DM; ++j) F3[i][j] = F[i][j];
    if (kind == FEMCY_MAT_NEOHOOKE) {
        if (DM == 2) F3[2][2] = 1.0;                 // plane strain
        const double J = det3(F3);
        double trB = 0.0;
#pragma unroll
        for (int i = 0; i < 3; ++i)
#pragma unroll
            for (int j = 0; j < 3; ++j) trB += F3[i][j] * F3[i][j];
        return p0 * (trB - 3.0 - 2.0 * log(J)) + p1 * (J - 1.0) * (J - 1.0);
    }
    if (kind == FEMCY_MAT_LIN3D) {
#pragma unroll
        for (int i = 0; i < 6; ++i)
#pragma unroll
            for (int j = 0; j < 6; ++j) C6[i][j] = C[i * 6 + j];
    } else if (kind == FEMCY_MAT_PSTRESS) {       // linear_isotropic_plane_stress.py:22-31, 98-114
        const double E_ = p0, nu = p1, c00 = E_ / (1.0 - nu * nu);
        F3[2][2] = -nu / (1.0 - nu) * (F[0][0] + F[1][1] - 2.0) + 1.0;
        C6[0][0] = C6[1][1] = c00;
        C6[0][1] = C6[1][0] = c00 * nu;
        C6[3][3] = E_ / 2.0 / (1.0 + nu);
    } else {                                      // plane strain: linear_isotropic_plane_strain.py:31-40, 88-100
        F3[2][2] = 1.0;
        const double c00 = C[0], c01 = C[1];
        C6[0][0] = C6[1][1] = c00;
        C6[0][1] = C6[1][0] = C6[0][2] = C6[2][0] = C6[1][2] = C6[2][1] = c01;
        C6[3][3] = C[8];
    }
    return energy_voigt3(F3, C6);
}

// one Gauss point of compute_strain_stress (stiffnessMtrx.py:436-501): strain (infinitesimal, or Green when `large`),
// Cauchy stress by constitutiveOfSmallDeform when !large (kept as given otherwise: "stress has been computed for
// geometric nonlinear case", :446-447), von Mises stress by material type (:449-501)
template <int DM>
FEMCY_HD void post_point(int large, int kind, const double* __restrict__ C, double p0, double p1,
                         const double* __restrict__ Fin, double* __restrict__ sigma, double* __restrict__ strain,
                         double* __restrict__ mises) {
    double F[DM][DM], sig[DM][DM];
#pragma unroll
    for (int i = 0; i < DM; ++i)
#pragma unroll
        for (int j = 0; j < DM; ++j) F[i][j] = Fin[i * DM + j];
#pragma unroll
    for (int i = 0; i < DM; ++i)
#pragma unroll
        for (int j = 0; j < DM; ++j) {
            double e;
            if (large) {
                e = 0.0;
#pragma unroll
                for (int k = 0; k < DM; ++k) e += F[k][i] * F[k][j];
                e = (e - (i == j ? 1.0 : 0.0)) / 2.0;       // Green strain (:575-589)
            } else {
                e = (F[i][j] + F[j][i]) / 2.0 - (i == j ? 1.0 : 0.0);   // infinitesimal strain (:559-572)
            }
            strain[i * DM + j] = e;
        }
    if (!large) {
        cauchy_small<DM>(kind, C, p0, p1, F, sig);
#pragma unroll
        for (int i = 0; i < DM; ++i)
#pragma unroll
            for (int j = 0; j < DM; ++j) sigma[i * DM + j] = sig[i][j];
    } else {
#pragma unroll
        for (int i = 0; i < DM; ++i)
#pragma unroll
            for (int j = 0; j < DM; ++j) sig[i][j] = sigma[i * DM + j];
    }
    double s3[3][3] = {{0, 0, 0}, {0, 0, 0}, {0, 0, 0}};
#pragma unroll
    for (int i = 0; i < DM; ++i)
#pragma unroll
        for (int j = 0; j < DM; ++j) s3[i][j] = sig[i][j];
    if (kind == FEMCY_MAT_PSTRAIN) s3[2][2] = p1 * (sig[0][0] + sig[1][1]);   // nu (s_xx + s_yy) (:475-489)
    if (DM == 2 && kind == FEMCY_MAT_NEOHOOKE)      // plane-strain neo-Hookean: b33 = 1 leaves the volumetric part
        s3[2][2] = 2.0 * p1 * (F[0][0] * F[1][1] - F[0][1] * F[1][0] - 1.0);
    const double tr = (s3[0][0] + s3[1][1] + s3[2][2]) / 3.0;
    double ss = 0.0;
#pragma unroll
    for (int i = 0; i < 3; ++i)
#pragma unroll
        for (int j = 0; j < 3; ++j) {
            const double dv = s3[i][j] - (i == j ? tr : 0.0);
            ss += dv * dv;
        }
    *mises = sqrt(1.5 * ss);
}

// one loaded facet of neumannBC (stiffnessMtrx.py:369-411, ELE.globalNormal): the loads of the facet's nodes on the
// UNDEFORMED element, contrib[fn][d]; `en` = the owning element's nodes, `t` = facet type (index into the element
// plugin's facet tables), dir_or_null = traction direction (TRVEC) or NULL for the outward normal (pressure)
template <int DM>
FEMCY_HD void neumann_facet(int32_t npe, int32_t nfn, int32_t nip, const double* __restrict__ nodes,
                            const int32_t* __restrict__ en, int32_t t, const int32_t* __restrict__ ft_nodes,
                            const double* __restrict__ ft_N, const double* __restrict__ ft_dN,
                            const double* __restrict__ ft_normal, const double* __restrict__ ft_weight, double traction,
                            const double* __restrict__ dir_or_null, double* __restrict__ contrib) {
    const int32_t* key = ft_nodes + (int64_t)t * nfn;
    // a quadrilateral facet in 3-D (hexahedron face): every facet point weighted by its surface Jacobian (Nanson's
    // formula, da = |det J| |J^-T n_nat| w), exact in area and shape for warped faces.  Every other facet keeps the size
    // of its first sorted local nodes (ELE.globalNormal): edge length, or corner-triangle area
    const bool nanson = DM == 3 && nfn == 4;
    double size = 0.0;
    if (!nanson) {
        const double* p0 = nodes + (int64_t)en[key[0]] * DM;
        const double* p1 = nodes + (int64_t)en[key[1]] * DM;
        if (DM == 2) {
            const double dx = p0[0] - p1[0], dy = p0[1] - p1[1];
            size = sqrt(dx * dx + dy * dy);
        } else {
            const double* p2 = nodes + (int64_t)en[key[2]] * DM;
            const double a0 = p1[0] - p0[0], a1 = p1[1] - p0[1], a2 = p1[2] - p0[2];
            const double b0 = p2[0] - p0[0], b1 = p2[1] - p0[1], b2 = p2[2] - p0[2];
            const double c0 = a1 * b2 - a2 * b1, c1 = a2 * b0 - a0 * b2, c2 = a0 * b1 - a1 * b0;
            size = 0.5 * sqrt(c0 * c0 + c1 * c1 + c2 * c2);
        }
    }
    for (int32_t fn = 0; fn < nfn; ++fn)
        for (int d = 0; d < DM; ++d) contrib[(int64_t)fn * DM + d] = 0.0;
    for (int32_t ip = 0; ip < nip; ++ip) {
        const int64_t tip = (int64_t)t * nip + ip;
        double J[DM][DM], inv[DM][DM];
        for (int i = 0; i < DM; ++i)
            for (int j = 0; j < DM; ++j) J[i][j] = 0.0;
        for (int32_t a = 0; a < npe; ++a) {
            const double* x = nodes + (int64_t)en[a] * DM;
            const double* dn = ft_dN + (tip * npe + a) * DM;
            for (int i = 0; i < DM; ++i)
                for (int j = 0; j < DM; ++j) J[i][j] += x[i] * dn[j];
        }
        const double det = det_inv<DM>(J, inv);
        double flux[DM];
        if (nanson) {
            double nrm = 0.0;
            for (int j = 0; j < DM; ++j) {
                double v = 0.0;
                for (int i = 0; i < DM; ++i) v += ft_normal[tip * DM + i] * inv[i][j];
                flux[j] = v;
                nrm += v * v;
            }
            nrm = sqrt(nrm);
            const double da = fabs(det) * nrm * ft_weight[tip];
            for (int d = 0; d < DM; ++d) flux[d] = traction * (dir_or_null ? dir_or_null[d] : flux[d] / (nrm + 1.e-30)) * da;
        } else if (dir_or_null) {
            for (int d = 0; d < DM; ++d) flux[d] = dir_or_null[d];
        } else {
            double nrm = 0.0;
            for (int j = 0; j < DM; ++j) {
                double v = 0.0;
                for (int i = 0; i < DM; ++i) v += ft_normal[tip * DM + i] * inv[i][j];
                flux[j] = v;
                nrm += v * v;
            }
            nrm = sqrt(nrm) + 1.e-30;
            for (int d = 0; d < DM; ++d) flux[d] /= nrm;
        }
        if (!nanson) {
            const double axw = size * ft_weight[tip];
            for (int d = 0; d < DM; ++d) flux[d] = traction * flux[d] * axw;
        }
        for (int32_t fn = 0; fn < nfn; ++fn) {
            const double shape = ft_N[tip * npe + key[fn]];
            for (int d = 0; d < DM; ++d) contrib[(int64_t)fn * DM + d] += flux[d] * shape;
        }
    }
}

// one element of a body load (*Dload GRAV / BX / BY / BZ): we[a] = sum_g N_a(xi_g) |det J_g| w_g on the UNDEFORMED
// coordinates X (dead load on the reference volume).  The consistent nodal load of a uniform force b per unit volume
// is we[a] * b.  dN[g][a][:] and N[g][a] are the plugin's tables at the Gauss points.
template <int NPE, int DM>
FEMCY_HD void body_weights_element(const double (&X)[NPE][DM], int32_t nGP, const double* __restrict__ dN,
                                   const double* __restrict__ N, const double* __restrict__ w, double (&we)[NPE]) {
#pragma unroll
    for (int a = 0; a < NPE; ++a) we[a] = 0.0;
    for (int32_t g = 0; g < nGP; ++g) {
        const double* __restrict__ dNg = dN + g * NPE * DM;
        const double* __restrict__ Ng = N + g * NPE;
        double J[DM][DM], inv[DM][DM];
#pragma unroll
        for (int i = 0; i < DM; ++i)
#pragma unroll
            for (int j = 0; j < DM; ++j) {
                double acc = 0.0;
#pragma unroll
                for (int a = 0; a < NPE; ++a) acc += X[a][i] * dNg[a * DM + j];
                J[i][j] = acc;
            }
        const double vg = fabs(det_inv<DM>(J, inv)) * w[g];
#pragma unroll
        for (int a = 0; a < NPE; ++a) we[a] += Ng[a] * vg;
    }
}

// ------------------------------------------------------------------------------------ thermal loads
// *Expansion + *Temperature (small strain): the stress of full restraint at alpha * dT = 1, s = C : eps_th with the
// isotropic thermal strain eps_th = k I and C exactly as femcy_set_material received it (no isotropy is assumed: an
// anisotropic C gives shear entries).  3-D: Voigt order [xx,yy,zz,xy,zx,yz], k = 1.  Plane stress: [xx,yy,xy], k = 1.
// Plane strain: eps_zz = 0 is enforced, the in-plane effective thermal strain is (1 + nu) alpha dT, so k = 1 + nu
// (nu = p1, as post_point uses it) and s_xx = s_yy = E / (1 - 2 nu) for the isotropic C.
template <int DM>
FEMCY_HD void thermal_unit_stress(int kind, const double* __restrict__ C, double p1, double (&s)[DM][DM]);

template <>
FEMCY_HD void thermal_unit_stress<3>(int, const double* __restrict__ C, double, double (&s)[3][3]) {
    double v[6];
#pragma unroll
    for (int p = 0; p < 6; ++p) v[p] = C[p * 6 + 0] + C[p * 6 + 1] + C[p * 6 + 2];
    s[0][0] = v[0]; s[1][1] = v[1]; s[2][2] = v[2];
    s[0][1] = s[1][0] = v[3];
    s[0][2] = s[2][0] = v[4];
    s[1][2] = s[2][1] = v[5];
}

template <>
FEMCY_HD void thermal_unit_stress<2>(int kind, const double* __restrict__ C, double p1, double (&s)[2][2]) {
    const double k = kind == FEMCY_MAT_PSTRAIN ? 1.0 + p1 : 1.0;
    double v[3];
#pragma unroll
    for (int p = 0; p < 3; ++p) v[p] = k * (C[p * 3 + 0] + C[p * 3 + 1]);
    s[0][0] = v[0]; s[1][1] = v[1];
    s[0][1] = s[1][0] = v[2];
}

// one element of a thermal load: fe[a*DM + i] = sum_g dT_g |det J_g| w_g sum_j dN_a/dx_j s[i][j] on the UNDEFORMED
// coordinates X, with dT_g = sum_a N_a(xi_g) dT[a] interpolated by the element's own shape functions and s the stress
// of full restraint per unit temperature change (alpha x the unit stress above).  dN[g][a][:] and N[g][a] are the
// plugin's tables at the Gauss points.
template <int NPE, int DM>
FEMCY_HD void thermal_force_element(const double (&X)[NPE][DM], const double (&dT)[NPE], int32_t nGP,
                                    const double* __restrict__ dN, const double* __restrict__ N,
                                    const double* __restrict__ w, const double (&s)[DM][DM], double (&fe)[NPE * DM]) {
#pragma unroll
    for (int q = 0; q < NPE * DM; ++q) fe[q] = 0.0;
    for (int32_t g = 0; g < nGP; ++g) {
        const double* __restrict__ dNg = dN + g * NPE * DM;
        const double* __restrict__ Ng = N + g * NPE;
        double J[DM][DM], inv[DM][DM];
#pragma unroll
        for (int i = 0; i < DM; ++i)
#pragma unroll
            for (int j = 0; j < DM; ++j) {
                double acc = 0.0;
#pragma unroll
                for (int a = 0; a < NPE; ++a) acc += X[a][i] * dNg[a * DM + j];
                J[i][j] = acc;
            }
        double tg = 0.0;
#pragma unroll
        for (int a = 0; a < NPE; ++a) tg += Ng[a] * dT[a];
        const double vg = fabs(det_inv<DM>(J, inv)) * w[g] * tg;
#pragma unroll
        for (int a = 0; a < NPE; ++a) {
            double ga[DM];
#pragma unroll
            for (int j = 0; j < DM; ++j) {
                double acc = 0.0;
#pragma unroll
                for (int k = 0; k < DM; ++k) acc += dNg[a * DM + k] * inv[k][j];
                ga[j] = acc;
            }
#pragma unroll
            for (int i = 0; i < DM; ++i) {
                double d = 0.0;
#pragma unroll
                for (int j = 0; j < DM; ++j) d += ga[j] * s[i][j];
                fe[a * DM + i] += d * vg;
            }
        }
    }
}

// one Gauss point of the stress correction: sigma -= th * s with th = scale * dT_g (s per unit temperature change), then the von Mises stress of
// the corrected tensor by material kind as post_point forms it; plane strain: s_zz = nu (s_xx + s_yy) - E alpha dT_g with
// E alpha dT_g = (1 - 2 nu) th s_xx, so that no further material parameter is needed.  The strain stays the total strain.
template <int DM>
FEMCY_HD void thermal_post_point(int kind, double p1, const double (&s)[DM][DM], double th,
                                 double* __restrict__ sigma, double* __restrict__ mises) {
    double s3[3][3] = {{0, 0, 0}, {0, 0, 0}, {0, 0, 0}};
#pragma unroll
    for (int i = 0; i < DM; ++i)
#pragma unroll
        for (int j = 0; j < DM; ++j) {
            const double v = sigma[i * DM + j] - th * s[i][j];
            sigma[i * DM + j] = v;
            s3[i][j] = v;
        }
    if (kind == FEMCY_MAT_PSTRAIN) s3[2][2] = p1 * (s3[0][0] + s3[1][1]) - (1.0 - 2.0 * p1) * (th * s[0][0]);
    const double tr = (s3[0][0] + s3[1][1] + s3[2][2]) / 3.0;
    double ss = 0.0;
#pragma unroll
    for (int i = 0; i < 3; ++i)
#pragma unroll
        for (int j = 0; j < 3; ++j) {
            const double dv = s3[i][j] - (i == j ? tr : 0.0);
            ss += dv * dv;
        }
    *mises = sqrt(1.5 * ss);
}

// --------------------------------------------------------------------------------- implicit dynamics
// one element of the consistent mass: vq[q * stride] = rho |det J_q| w_q at the nq points of the element's MASS rule, on
// the UNDEFORMED coordinates X.  dNq[q][a][:] are the plugin's natural derivatives at those points (mass_rule(), not the
// Gauss points of the stiffness).
template <int NPE, int DM>
FEMCY_HD void mass_points_element(const double (&X)[NPE][DM], int32_t nq, const double* __restrict__ dNq,
                                  const double* __restrict__ wq, double rho, double* __restrict__ vq, int64_t stride) {
    for (int32_t q = 0; q < nq; ++q) {
        const double* __restrict__ dNg = dNq + q * NPE * DM;
        double J[DM][DM], inv[DM][DM];
#pragma unroll
        for (int i = 0; i < DM; ++i)
#pragma unroll
            for (int j = 0; j < DM; ++j) {
                double acc = 0.0;
#pragma unroll
                for (int a = 0; a < NPE; ++a) acc += X[a][i] * dNg[a * DM + j];
                J[i][j] = acc;
            }
        vq[q * stride] = rho * (fabs(det_inv<DM>(J, inv)) * wq[q]);
    }
}

// the contribution of one element to the mass block (a, b): sum_q (N_a N_b)(xi_q) vq[q].  The product N_a N_b is formed
// first, so that (a, b) and (b, a) receive the same bits.
FEMCY_HD double mass_pair(int32_t nq, int32_t npe, const double* __restrict__ Nq, int la, int lb,
                          const double* __restrict__ vq) {
    double acc = 0.0;
    for (int32_t q = 0; q < nq; ++q) acc += (Nq[q * npe + la] * Nq[q * npe + lb]) * vq[q];
    return acc;
}

// Newmark, one entry: a_new = b0 (u_new - u) - b1 v - b2 a with b0 = 1 / (beta dt^2), b1 = 1 / (beta dt),
// b2 = 1 / (2 beta) - 1; v_new = v + dt ((1 - gamma) a + gamma a_new).  v and a are replaced.
FEMCY_HD void newmark_update_entry(double un, double u, double& v, double& a, double b0, double b1, double b2, double dt,
                                   double gamma) {
    const double an = b0 * (un - u) - b1 * v - b2 * a;
    v = v + dt * ((1.0 - gamma) * a + gamma * an);
    a = an;
}

// --------------------------------------------------------------------------------- explicit dynamics
// one element of the LUMPED mass by HRZ lumping (Hinton, Rock, Zienkiewicz): with vq = rho |det J_q| w_q at the nq points of
// the element's mass rule, on the UNDEFORMED coordinates X,
//   m_e = sum_q vq,   d_a = sum_q N_a(xi_q)^2 vq,   me[a] = d_a m_e / sum_b d_b
// i.e. the diagonal of the consistent element mass scaled to the element's mass: strictly positive for every family (the row
// sums are negative at the corners of C3D10 / CPS6 / CPS8), m_e / NPE on CPS3 / C3D4.
template <int NPE, int DM>
FEMCY_HD void lumped_element(const double (&X)[NPE][DM], int32_t nq, const double* __restrict__ Nq,
                             const double* __restrict__ dNq, const double* __restrict__ wq, double rho, double (&me)[NPE]) {
    double mass = 0.0;
#pragma unroll
    for (int a = 0; a < NPE; ++a) me[a] = 0.0;
    for (int32_t q = 0; q < nq; ++q) {
        double vq;
        mass_points_element<NPE, DM>(X, 1, dNq + q * NPE * DM, wq + q, rho, &vq, 1);
        mass += vq;
#pragma unroll
        for (int a = 0; a < NPE; ++a) me[a] += (Nq[q * NPE + a] * Nq[q * NPE + a]) * vq;
    }
    double diag = 0.0;
#pragma unroll
    for (int a = 0; a < NPE; ++a) diag += me[a];
#pragma unroll
    for (int a = 0; a < NPE; ++a) me[a] = me[a] * mass / diag;
}

// Velocity Verlet (central differences with all state at whole steps), one scalar DOF.  The fused multiply-adds are written
// out, so that the node kernel, the vector kernel of a call's first drift and the host backend round alike: a run split into
// several calls gives the bits of one call.
//   kick:  a_new = minv (s f - f_int),  v_new = v + (h / 2)(a + a_new)      hh = h / 2
//   drift: u_new = u + h v + (h^2 / 2) a                                    h2h = h^2 / 2
FEMCY_HD void explicit_kick(double minv, double s, double f, double fint, double hh, double& v, double& a) {
    const double an = minv * fma(s, f, -fint);
    v = fma(hh, a + an, v);
    a = an;
}
FEMCY_HD double explicit_drift(double u, double v, double a, double h, double h2h) { return fma(h2h, a, fma(h, v, u)); }

// Damping (*Bulk Viscosity, *Damping alpha=; femcy_explicit_set_damping).  Both forces are evaluated at u_{n+1} with the
// LAGGED half-step velocity, the one the drift by h to u_{n+1} used (hh = h / 2):
//   v_{n+1/2} = fma(h / 2, a_n, v_n)
//   a_{n+1}   = minv (s f - f_int(u_{n+1}) - f_bv(u_{n+1}, v_{n+1/2})) - alpha v_{n+1/2},   v_{n+1} = v_n + h/2 (a_n + a_{n+1})
// At the start v_{-1/2} := v_0: the callers pass a = 0 there (vec[ACC] is not read), and fma(hh, 0, v) is v.  A held DOF
// (minv = 0) takes no damping force either, so that it keeps a = 0.
FEMCY_HD double explicit_vhalf(double v, double a, double hh) { return fma(hh, a, v); }
FEMCY_HD void explicit_kick_damped(double minv, double s, double f, double fint, double hh, double alpha, double& v, double& a) {
    const double vh = explicit_vhalf(v, a, hh);
    double an = minv * fma(s, f, -fint);
    if (minv != 0.0) an = fma(-alpha, vh, an);
    v = fma(hh, a + an, v);
    a = an;
}

// Frictionless planar rigid walls (*Rigid Wall; femcy_explicit_set_wall, where the law stands).  Wall k: the unit normal
// nrm[k] into the free half space, d[k] = nrm[k] . point and the penalty kappa[k] in 1/s^2, all formed once on the host
// (api_checks.hpp: check_explicit_set_wall).  The gap of a node at x = X + u (one rounding per component) is the fma chain
//   g = fma(n[DM-1], x[DM-1], ... fma(n[0], x[0], -d)),
// and wall_accel adds the wall's share to the acceleration of component i of a node inside it, walls in ascending order:
//   g < 0:  a = fma(-kappa g, n_i, a)        i.e. a_i += -kappa min(g, 0) n_i; a wall that is not reached adds nothing at all
struct ExplicitWalls {
    int32_t n;
    double nrm[FEMCY_WALL_MAX][3], d[FEMCY_WALL_MAX], kappa[FEMCY_WALL_MAX];
};
template <int DM>
FEMCY_HD double wall_gap(const ExplicitWalls& w, int k, const double (&x)[DM]) {
    double g = fma(w.nrm[k][0], x[0], -w.d[k]);
#pragma unroll
    for (int j = 1; j < DM; ++j) g = fma(w.nrm[k][j], x[j], g);
    return g;
}
template <int DM>
FEMCY_HD double wall_accel(const ExplicitWalls& w, const double (&x)[DM], int i, double a) {
    for (int k = 0; k < w.n; ++k) {
        const double g = wall_gap<DM>(w, k, x);
        const double ni = i == 0 ? w.nrm[k][0] : (i == 1 ? w.nrm[k][1] : w.nrm[k][DM - 1]);
        if (g < 0.0) a = fma(-w.kappa[k] * g, ni, a);
    }
    return a;
}
// the kick of a DOF of an integrator with walls: explicit_kick / explicit_kick_damped (alpha = 0: the former's arithmetic)
// with the wall term after minv (s f - f_int) and before the alpha term, on a free DOF only
template <int DM>
FEMCY_HD void explicit_kick_wall(double minv, double s, double f, double fint, double hh, double alpha, const ExplicitWalls& w,
                                 const double (&x)[DM], int i, double& v, double& a) {
    const double vh = explicit_vhalf(v, a, hh);
    double an = minv * fma(s, f, -fint);
    if (minv != 0.0) {
        an = wall_accel<DM>(w, x, i, an);
        if (alpha != 0.0) an = fma(-alpha, vh, an);
    }
    v = fma(hh, a + an, v);
    a = an;
}
// what femcy_explicit_wall_get sums of one node for wall k: its mass m, whether any of its DOFs is free; t[0] the normal
// force kappa m p, t[1] the potential 1/2 kappa m p^2 (both 0 on a node that is held in every DOF), t[2] 1 if g < 0,
// t[3] the penetration p = max(-g, 0)
template <int DM>
FEMCY_HD void wall_node_terms(const ExplicitWalls& w, int k, const double (&x)[DM], double m, bool any_free, double (&t)[4]) {
    const double g = wall_gap<DM>(w, k, x);
    const double p = fmax(-g, 0.0);
    const double km = any_free ? w.kappa[k] * m : 0.0;
    const double fn = km * p;
    t[0] = fn;
    t[1] = (0.5 * fn) * p;
    t[2] = g < 0.0 ? 1.0 : 0.0;
    t[3] = p;
}

// Bulk viscosity at one Gauss point of the stiffness rule, on the CURRENT configuration.  With G_a = grad_x N_a (formed from
// dNg and inv = J_x^-1 as the element pass forms them) and vh the element's rows of v_{n+1/2}:
//   rate = sum_a vh_a . G_a        (the dm-dimensional divergence; plane stress: in the plane only)
//   gmax = max_a |G_a|^2,  L = gmax^(-1/2)      (C3D4: the smallest altitude; a bar of length L: L)
//   rho  = rho0 / |det F|
//   p    = b1 sqrt(rho M_d) L rate + rho (b2 L)^2 |rate| min(0, rate)
// p enters the force accumulation as sigma + p I and nothing else: the stored stress never contains it.
// NPE > 0: the number of nodes at compile time (device); NPE = 0: npe at run time (host).
struct ExplicitDamping {
    double alpha, b1, b2, Md, rho0;
};
template <int NPE, int DM>
FEMCY_HD void bulk_rate_point(int npe, const double* __restrict__ dNg, const double (&inv)[DM][DM], const double* vh,
                              double& rate, double& gmax) {
    const int n = NPE > 0 ? NPE : npe;
    rate = 0.0;
    gmax = 0.0;
#pragma unroll
    for (int a = 0; a < n; ++a) {
        double gg = 0.0;
#pragma unroll
        for (int j = 0; j < DM; ++j) {
            double acc = 0.0;
#pragma unroll
            for (int k = 0; k < DM; ++k) acc += dNg[a * DM + k] * inv[k][j];
            rate = fma(vh[a * DM + j], acc, rate);
            gg = fma(acc, acc, gg);
        }
        gmax = fmax(gmax, gg);
    }
}
FEMCY_HD double bulk_pressure(const ExplicitDamping& d, double rate, double gmax, double detF) {
    const double L = 1.0 / sqrt(gmax), rho = d.rho0 / fabs(detF), bl = d.b2 * L;
    return d.b1 * sqrt(rho * d.Md) * L * rate + rho * (bl * bl) * fabs(rate) * fmin(0.0, rate);
}
// the quadratic term's share of the critical fraction, L sqrt(rho / M_d) max(0, -rate) (b2^2 is applied by the caller)
FEMCY_HD double bulk_xi_point(const ExplicitDamping& d, double rate, double gmax, double detF) {
    return sqrt(d.rho0 / fabs(detF) / d.Md / gmax) * fmax(0.0, -rate);
}

// The element-by-element estimate of the highest frequency (*Dynamic, explicit, element by element), at the CURRENT
// configuration x = X + u.  With m_a^e the element's own HRZ share of the lumped mass (lumped_element), v_q = |det J_x| w_q at
// the stiffness rule's Gauss points, sigma_q = cauchy_large(F_q) and s_C = max eps:C:eps / eps:eps of the small-strain matrix,
//   g_e       = sum_q v_q sum_a |grad_x N_a|^2 / m_a^e
//   omega_e^2 = sum_q v_q (s_C + |sigma_q|_F) sum_a |grad_x N_a|^2 / m_a^e,      omega = sqrt(max_e omega_e^2).
// At u = 0 with a linear material this is a proof: Cauchy-Schwarz gives |grad u|_F^2 <= (sum_a |grad N_a|^2 / m_a)(x^T M_e x),
// hence lambda_max(M_e^-1 K_e) <= s_C g_e, and lambda_max(M^-1 K) <= max_e lambda_max(M_e^-1 K_e) because M and K are sums
// over the elements; the |sigma|_F term bounds the geometric stiffness the same way.  At finite strain the material part is
// an ESTIMATE: the spatial tangent is not C.  The user's `scale factor` is the margin there.
// One Gauss point: G = grad_x N [NPE][DM], v = |det J_x| w, sig [DM][DM], rme[a] = 1 / m_a^e.
template <int NPE, int DM>
FEMCY_HD void explicit_bound_point(const double* __restrict__ G, double v, const double* __restrict__ sig,
                                   const double (&rme)[NPE], double s_C, double& g, double& w2) {
    double q = 0.0;
#pragma unroll
    for (int a = 0; a < NPE; ++a) {
        double gg = 0.0;
#pragma unroll
        for (int j = 0; j < DM; ++j) gg += G[a * DM + j] * G[a * DM + j];
        q += gg * rme[a];
    }
    double ss = 0.0;
#pragma unroll
    for (int k = 0; k < DM * DM; ++k) ss += sig[k] * sig[k];
    const double qv = q * v;
    g += qv;
    w2 += (s_C + sqrt(ss)) * qv;
}

// the whole element from its coordinates X, displacements U and masses me: gradients, F and sigma as the element pass of the
// internal force forms them (dN[g][a][:], w[g]: the plug-in's tables at the Gauss points)
// DAMP (femcy_explicit_set_damping; vh = the element's rows of v_{n+1/2}, d the coefficients): omega_e^2 is replaced by
//   omega_eff,e^2 = omega_e^2 (sqrt(1 + xi_e^2) + xi_e)^2,
//   xi_e = alpha / (2 omega_e) + b1 + b2^2 max_q [L_q sqrt(rho_q / M_d) max(0, -rate_q)]
// the critical fraction of the lagged damping forces in the element's highest mode (bulk_rate_point, bulk_xi_point).  An
// element with omega_e = 0 and alpha != 0 gives xi_e = inf and omega_eff,e^2 = NaN, which the callers count as an infinite
// frequency: no increment, the safe side.
// kappa (the sum of the penalties of the integrator's rigid walls, 0: none): added to omega_e^2 BEFORE the damping factor.
// On a node in contact wall k adds kappa_k m_a n n^T to the stiffness; in the M-inner product that is kappa_k n n^T on the
// node's block, positive semi-definite with the largest eigenvalue kappa_k (|n| = 1), so by Weyl's inequality
// lambda_max(M^-1 (K + K_w)) <= lambda_max(M^-1 K) + sum_k kappa_k: omega_c^2 <= omega^2 + kappa.  Any element may touch a
// wall, so every element takes the whole sum: the safe side.
template <int NPE, int DM, bool DAMP>
FEMCY_HD void explicit_bound_element_impl(const double (&X)[NPE][DM], const double (&U)[NPE][DM], const double* vh,
                                          const ExplicitDamping* d, int32_t nGP, const double* __restrict__ dN,
                                          const double* __restrict__ w, int kind, const double* __restrict__ C, double p0,
                                          double p1, const double (&me)[NPE], double s_C, double& g, double& w2,
                                          double kappa) {
    double rme[NPE];
    double xq = 0.0;
#pragma unroll
    for (int a = 0; a < NPE; ++a) rme[a] = 1.0 / me[a];
    g = 0.0;
    w2 = 0.0;
    for (int32_t q = 0; q < nGP; ++q) {
        const double* __restrict__ dNg = dN + q * NPE * DM;
        double J[DM][DM], inv[DM][DM], J0[DM][DM], inv0[DM][DM], F[DM][DM], sig[DM][DM], G[NPE * DM], sl[DM * DM];
#pragma unroll
        for (int i = 0; i < DM; ++i)
#pragma unroll
            for (int j = 0; j < DM; ++j) {
                double acc = 0.0, acc0 = 0.0;
#pragma unroll
                for (int a = 0; a < NPE; ++a) {
                    acc += (X[a][i] + U[a][i]) * dNg[a * DM + j];
                    acc0 += X[a][i] * dNg[a * DM + j];
                }
                J[i][j] = acc;
                J0[i][j] = acc0;
                F[i][j] = i == j ? 1.0 : 0.0;
            }
        const double det = det_inv<DM>(J, inv);
        [[maybe_unused]] const double det0 = det_inv<DM>(J0, inv0);
#pragma unroll
        for (int a = 0; a < NPE; ++a) {
#pragma unroll
            for (int j = 0; j < DM; ++j) {
                double acc = 0.0, acc0 = 0.0;
#pragma unroll
                for (int k = 0; k < DM; ++k) {
                    acc += dNg[a * DM + k] * inv[k][j];
                    acc0 += dNg[a * DM + k] * inv0[k][j];
                }
                G[a * DM + j] = acc;
#pragma unroll
                for (int i = 0; i < DM; ++i) F[i][j] += U[a][i] * acc0;
            }
        }
        cauchy_large<DM>(kind, C, p0, p1, F, sig);
#pragma unroll
        for (int i = 0; i < DM; ++i)
#pragma unroll
            for (int j = 0; j < DM; ++j) sl[i * DM + j] = sig[i][j];
        explicit_bound_point<NPE, DM>(G, fabs(det) * w[q], sl, rme, s_C, g, w2);
        if constexpr (DAMP) {
            if (d->b2 != 0.0) {
                double rate, gmax;
                bulk_rate_point<NPE, DM>(NPE, dNg, inv, vh, rate, gmax);
                xq = fmax(xq, bulk_xi_point(*d, rate, gmax, det / det0));
            }
        }
    }
    if (kappa != 0.0) w2 += kappa;
    if constexpr (DAMP) {
        const double om = sqrt(w2);
        const double xi = (d->alpha != 0.0 ? d->alpha / (2.0 * om) : 0.0) + d->b1 + d->b2 * d->b2 * xq;
        const double k = sqrt(1.0 + xi * xi) + xi;
        w2 *= k * k;
    }
}
template <int NPE, int DM>
FEMCY_HD void explicit_bound_element(const double (&X)[NPE][DM], const double (&U)[NPE][DM], int32_t nGP,
                                     const double* __restrict__ dN, const double* __restrict__ w, int kind,
                                     const double* __restrict__ C, double p0, double p1, const double (&me)[NPE], double s_C,
                                     double& g, double& w2, double kappa = 0.0) {
    explicit_bound_element_impl<NPE, DM, false>(X, U, nullptr, nullptr, nGP, dN, w, kind, C, p0, p1, me, s_C, g, w2, kappa);
}
template <int NPE, int DM>
FEMCY_HD void explicit_bound_element_damped(const double (&X)[NPE][DM], const double (&U)[NPE][DM], const double (&vh)[NPE][DM],
                                            const ExplicitDamping& d, int32_t nGP, const double* __restrict__ dN,
                                            const double* __restrict__ w, int kind, const double* __restrict__ C, double p0,
                                            double p1, const double (&me)[NPE], double s_C, double& g, double& w2,
                                            double kappa = 0.0) {
    explicit_bound_element_impl<NPE, DM, true>(X, U, &vh[0][0], &d, nGP, dN, w, kind, C, p0, p1, me, s_C, g, w2, kappa);
}

// Fixed mass scaling (femcy_lumped_mass_scale): the factor k_e of one element from w2 = its undamped omega_e^2 at u = 0 with
// its current shares, w2max = max_e omega_e^2 (read by FEMCY_MS_UNIFORM alone), the caller's factor f and target increment
// tau (0: not given) and the type.  omega_e^2 is linear in 1 / m_a^e, so with dt_e = 2 / omega_e
//   f alone                 k_e = f
//   tau, BELOW_MIN          k_e = max(1, omega_e^2 tau^2 / 4)
//   tau, SET_EQUAL_DT       k_e = omega_e^2 tau^2 / 4
//   tau, UNIFORM            k_e = max_e omega_e^2 tau^2 / 4
//   f and tau               f first: omega_e^2 / f enters the tau rule, k_e is the product
// A NaN w2 comes back as NaN under every rule with tau but FEMCY_MS_BELOW_MIN's fmax; the callers test omega_e^2 themselves.
FEMCY_HD double mass_scale_factor(double w2, double w2max, double f, double tau, int type) {
    const double f1 = f != 0.0 ? f : 1.0;
    if (tau == 0.0) return f1;
    const double r = ((type == FEMCY_MS_UNIFORM ? w2max : w2) / f1) * (tau * tau) * 0.25;
    return f1 * (type == FEMCY_MS_BELOW_MIN ? fmax(1.0, r) : r);
}
// what a reduction over the elements carries of one of them: omega_e^2 with NaN counted as infinity (k_explicit_bound), and
// k_e with anything but a finite positive number counted as infinity, so that one finite maximum vouches for every factor
FEMCY_HD double mass_scale_nan_to_inf(double w2) { return w2 != w2 ? INFINITY : w2; }
FEMCY_HD double mass_scale_bad_to_inf(double k) { return k > 0.0 ? k : INFINITY; }

// the clock of an automatic run, advanced once per step on whichever backend: t is the time of the state the element pass
// has just seen, h_next the increment of the next drift, t_next the time that drift reaches.
struct ExplicitClock {
    double t, t_next, T, sf, s_C, h_prev, h_next, h_last, h_min, omega;
    int32_t steps, ramp;
};
// one tick: the drift by h_next has happened (a real step when h_next > 0), omega2 is the estimate at the new state.
//   h_next = min(sf 2 / omega, T - t), exactly 0 once t >= T or when omega is not finite; the step that takes the remainder
//   sets the clock to T itself.
FEMCY_HD void explicit_clock_tick(ExplicitClock& r, double omega2) {
    const double t = r.t_next, hp = r.h_next;
    if (hp > 0.0) {
        r.steps += 1;
        r.h_last = hp;
        r.h_min = hp < r.h_min ? hp : r.h_min;
    }
    const double omega = sqrt(omega2);
    double h = 0.0, tn = t;
    if (t < r.T && omega == omega && omega <= 1.79769313486231570815e308) {
        const double rem = r.T - t, hs = r.sf * (2.0 / omega);
        if (hs >= rem) {
            h = rem;
            tn = r.T;
        } else {
            h = hs;
            tn = t + hs < r.T ? t + hs : r.T;
        }
    }
    r.t = t;
    r.t_next = tn;
    r.h_prev = hp;
    r.h_next = h;
    r.omega = omega;
}

// What the node pass of a step does: XN_START a_0 = minv (s f - f_int), nothing else is touched; XN_KICK the kick, a and v
// are replaced; XN_KICK_DRIFT the kick, then u drifts to the next state with the new a and v.  Its numbers: the load scale
// s, hh = half the increment of the kick, h and h2h = h^2 / 2 of the drift.
enum { XN_START = 0, XN_KICK = 1, XN_KICK_DRIFT = 2 };
struct ExplicitStep {
    double s, hh, h, h2h;
    bool drift;
    double alpha;   // mass-proportional damping (explicit_kick_damped); 0: the undamped kick, today's arithmetic
};
// a fixed increment h: kick and drift by the same h (h > 0 in a step, 0 with XN_START)
FEMCY_HD ExplicitStep explicit_step_fixed(double s, double h, int mode, double alpha = 0.0) {
    return {s, 0.5 * h, h, 0.5 * h * h, mode == XN_KICK_DRIFT && h != 0.0, alpha};
}
// from the clock of an automatic run: the kick uses h_prev (the increment that led to the state being kicked), the drift
// h_next and is skipped when that is 0; the scale is 1 (STEP) or t / T (RAMP) at the time t of the state being kicked.
// false: h_prev = h_next = 0 in a step, nothing may be written -- the steps of a batch that overshoots T leave u, v, a bit
// for bit alone.
FEMCY_HD bool explicit_step_clock(const ExplicitClock& k, int mode, ExplicitStep& st, double alpha = 0.0) {
    const double hp = k.h_prev, h = k.h_next;
    if (mode != XN_START && hp == 0.0 && h == 0.0) return false;
    st = {k.ramp ? k.t / k.T : 1.0, 0.5 * hp, h, 0.5 * h * h, mode == XN_KICK_DRIFT && h != 0.0, alpha};
    return true;
}

// Prescribed motion (*Boundary, amplitude=; femcy_amplitude_create, femcy_explicit_set_motion).  One curve: npts points
// t[0] < t[1] < ... with the values A[], in step time.  amplitude() returns A(t), A'(t) and A''(t); a moved DOF with the
// value g then has u = g A, v = g A', a = g A'' (explicit_moved).  Between two points, xi = (t - t_k) / (t_{k+1} - t_k):
//   FEMCY_AMP_TABULAR      A = A_k + (A_{k+1} - A_k) xi,  A' the slope of [t_k, t_{k+1}) -- the right-hand one at a point --,
//                          A'' = 0
//   FEMCY_AMP_SMOOTH_STEP  A = A_k + (A_{k+1} - A_k) xi^3 (10 - 15 xi + 6 xi^2), and from the same polynomial
//                          A'  = (A_{k+1} - A_k) / dt_k    30 xi^2 (1 - xi)^2
//                          A'' = (A_{k+1} - A_k) / dt_k^2  60 xi (1 - xi)(1 - 2 xi):      both exactly 0 at every point
// Outside the table both are clamped: (A_0, 0, 0) for t <= t_0 and (A_last, 0, 0), exactly, for t >= t_last.  The fused
// multiply-adds are written out, so that the device kernels and the host backend round alike.
struct Amplitude {
    int32_t kind, npts;
    double t[FEMCY_AMP_MAX_POINTS], A[FEMCY_AMP_MAX_POINTS];
};
FEMCY_HD void amplitude(const Amplitude& am, double t, double& A, double& dA, double& ddA) {
    const int last = am.npts - 1;
    dA = 0.0;
    ddA = 0.0;
    if (!(t > am.t[0])) {
        A = am.A[0];
        return;
    }
    if (t >= am.t[last]) {
        A = am.A[last];
        return;
    }
    int k = 0;
    while (k + 1 < last && t >= am.t[k + 1]) ++k;
    const double dt = am.t[k + 1] - am.t[k], rise = am.A[k + 1] - am.A[k];
    const double xi = (t - am.t[k]) / dt, slope = rise / dt;
    if (am.kind == FEMCY_AMP_TABULAR) {
        A = fma(rise, xi, am.A[k]);
        dA = slope;
        return;
    }
    const double om = 1.0 - xi;
    A = fma(rise, (xi * xi * xi) * fma(fma(6.0, xi, -15.0), xi, 10.0), am.A[k]);
    dA = slope * (30.0 * (xi * xi) * (om * om));
    ddA = (slope / dt) * (60.0 * xi * om * fma(-2.0, xi, 1.0));
}
// u, v and a of a moved DOF with the value g at time t: what k_explicit_place and the host backend store (what: a mask)
enum { MOVE_U = 1, MOVE_V = 2, MOVE_A = 4 };
FEMCY_HD void explicit_place(const Amplitude& am, double g, double t, int what, double& u, double& v, double& a) {
    double A, dA, ddA;
    amplitude(am, t, A, dA, ddA);
    if (what & MOVE_U) u = g * A;
    if (what & MOVE_V) v = g * dA;
    if (what & MOVE_A) a = g * ddA;
}
// what the node pass does to a moved DOF instead of the kick (modes below, at ExplicitStep): a (and, but at the start, v) at
// the time t of the state being kicked, then u at the time t_drift the drift reaches, by assignment
FEMCY_HD void explicit_moved(const Amplitude& am, double g, double t, double t_drift, bool start, bool drift, double& u,
                             double& v, double& a) {
    explicit_place(am, g, t, start ? MOVE_A : MOVE_V | MOVE_A, u, v, a);
    if (!start && drift) explicit_place(am, g, t_drift, MOVE_U, u, v, a);
}
// the clock of a fixed run: state n is at t_base + (n - n_base) dt, one rounding whichever call reaches it
FEMCY_HD double explicit_fixed_time(double t_base, int64_t n_base, int64_t n, double dt) {
    return fma((double)(n - n_base), dt, t_base);
}

// Energy balance (*Energy Output; femcy_explicit_energy_enable / _get, where the definitions stand).  One scalar DOF's
// addends w[FEMCY_EN_*] of the step that led to the state n being kicked, by the trapezoid rule 1/2 du (g_{n-1} + g_n) for
// every force g; what the node pass of either backend calls with the numbers it holds anyway.  The forces of state n - 1
// (fint_prev, ga_prev) and its load scale s_prev come from what the previous kick left behind.
FEMCY_HD double energy_trapezoid(double du, double g_prev, double g) { return 0.5 * du * (g_prev + g); }
// a DOF that is not moved: v and a are those of state n - 1 (at the start v_0 and 0), hh half the increment that led to
// state n.  ga = alpha m v_{n-1/2}, the force explicit_kick_damped subtracts, for the next call; a held DOF (minv = 0)
// has du = 0 and takes no alpha force.  start: only ga.
FEMCY_HD void explicit_energy_free(double minv, double m, double s_prev, double s, double f, double fint_prev, double fint,
                                   double ga_prev, double alpha, double v, double a, double hh, bool start, double (&w)[4],
                                   double& ga) {
    w[0] = w[1] = w[2] = w[3] = 0.0;
    ga = 0.0;
    if (minv == 0.0) return;
    const double vh = explicit_vhalf(v, a, hh);
    if (alpha != 0.0) ga = alpha * m * vh;
    if (start) return;
    const double du = (2.0 * hh) * vh;
    w[FEMCY_EN_LOAD] = energy_trapezoid(du, s_prev * f, s * f);
    w[FEMCY_EN_INTERNAL] = energy_trapezoid(du, fint_prev, fint);
    w[FEMCY_EN_ALPHA] = energy_trapezoid(du, ga_prev, ga);
}
// a moved DOF: du is the curve's own difference between the two states, a_prev and a its accelerations there, and the
// support applies R = m a + fint - s f
FEMCY_HD void explicit_energy_moved(const Amplitude& am, double g, double t_prev, double t, double m, double s_prev, double s,
                                    double f, double fint_prev, double fint, double a_prev, double a, double (&w)[4]) {
    double u0 = 0.0, u1 = 0.0, unused = 0.0;
    explicit_place(am, g, t_prev, MOVE_U, u0, unused, unused);
    explicit_place(am, g, t, MOVE_U, u1, unused, unused);
    const double du = u1 - u0;
    w[FEMCY_EN_LOAD] = energy_trapezoid(du, s_prev * f, s * f);
    w[FEMCY_EN_INTERNAL] = energy_trapezoid(du, fint_prev, fint);
    w[FEMCY_EN_ALPHA] = 0.0;
    w[FEMCY_EN_BOUNDARY] = energy_trapezoid(du, m * a_prev + fint_prev - s_prev * f, m * a + fint - s * f);
}

// sum of 32 partial sums by the xor tree of half a wavefront, as lane 0 of k_nodal_force ends up with it: what the host
// backend runs so that a node sum has the device's summation order
inline double half_wave_tree(double (&p)[32]) {
    for (int o = 16; o > 0; o >>= 1)
        for (int l = 0; l < o; ++l) p[l] += p[l + o];
    return p[0];
}

}  // namespace femcy
