// Stand-alone sanitizer check of the host backend's mass / Newmark / small-strain-energy / body-load / thermal-load calls on
// a 65-node CPS4 mesh (12 x 4 cells): no Python, no GPU.  Build and run from the repository root:
//   g++ -O1 -g -std=c++17 -fopenmp -fsanitize=address,undefined -fno-omit-frame-pointer tools/mass_sanitize.cpp \
//       femcy_amd/csrc_cpu/femcy_cpu.cpp -o /tmp/mass_sanitize && /tmp/mass_sanitize
// It prints one line and returns 0 when every call succeeded; the sanitizers abort on a finding.
#include <cstdio>
#include <vector>
#include <cmath>
#include "../include/femcy.h"
int main() {
    const int nx = 12, ny = 4, nn = (nx + 1) * (ny + 1), ne = nx * ny;
    std::vector<double> nodes(nn * 2);
    for (int j = 0; j <= ny; ++j) for (int i = 0; i <= nx; ++i) { nodes[2 * (j * (nx + 1) + i)] = 0.25 * i + 0.01 * ((i * j) % 3); nodes[2 * (j * (nx + 1) + i) + 1] = 0.5 * j; }
    std::vector<int32_t> el(ne * 4);
    for (int j = 0; j < ny; ++j) for (int i = 0; i < nx; ++i) { int o = j * (nx + 1) + i, e = j * nx + i; el[4*e] = o; el[4*e+1] = o + 1; el[4*e+2] = o + nx + 2; el[4*e+3] = o + nx + 1; }
    const double g = 1.0 / std::sqrt(3.0), gp[4][2] = {{-g,-g},{g,-g},{g,g},{-g,g}}, sg[4][2] = {{-1,-1},{1,-1},{1,1},{-1,1}};
    double N[16], dN[32], w[4] = {1, 1, 1, 1};
    for (int q = 0; q < 4; ++q) for (int a = 0; a < 4; ++a) {
        N[q*4+a] = 0.25 * (1 + sg[a][0] * gp[q][0]) * (1 + sg[a][1] * gp[q][1]);
        dN[(q*4+a)*2] = 0.25 * sg[a][0] * (1 + sg[a][1] * gp[q][1]);
        dN[(q*4+a)*2+1] = 0.25 * sg[a][1] * (1 + sg[a][0] * gp[q][0]);
    }
    femcy_ctx* h = nullptr;
    int rc = femcy_ctx_create(0, &h);
    rc |= femcy_set_mesh(h, nn, 2, nodes.data(), ne, 4, el.data());
    rc |= femcy_set_element(h, 4, dN, w, FEMCY_VOIGT_2D);
    double C[9] = {2.2e5, 6.6e4, 0, 6.6e4, 2.2e5, 0, 0, 0, 7.7e4}, prm[2] = {2e5, 0.3};
    rc |= femcy_set_material(h, FEMCY_MAT_PSTRESS, C, prm, 2);
    rc |= femcy_build_pattern(h);
    int32_t id = -1;
    rc |= femcy_mass_create(h, 4, N, dN, w, 7.85e-3, &id);
    femcy_pattern_info info;
    rc |= femcy_get_pattern_info(h, &info);
    std::vector<double> m(info.nnzb), x(nn * 2, 1.0);
    rc |= femcy_mass_get(h, id, m.data());
    double total = 0; for (double v : m) total += v;
    rc |= femcy_vec_upload(h, FEMCY_VEC_VEL, x.data(), nn * 2);
    rc |= femcy_mass_apply(h, id, FEMCY_VEC_VEL, FEMCY_VEC_RHS, 0.5, 0);
    rc |= femcy_mass_apply(h, id, FEMCY_VEC_VEL, FEMCY_VEC_RHS, 0.5, 1);
    rc |= femcy_assemble_K(h, -1);
    rc |= femcy_mass_add_to_K(h, id, 4.0, 0);
    rc |= femcy_mass_add_to_K(h, id, 1.0, 1);
    double ke = 0;
    rc |= femcy_mass_kinetic_energy(h, id, FEMCY_VEC_VEL, &ke);
    rc |= femcy_newmark_predict(h, FEMCY_VEC_DOF, FEMCY_VEC_VEL, FEMCY_VEC_ACC, FEMCY_VEC_RESIDUAL, 1, 2, 3);
    rc |= femcy_newmark_update(h, FEMCY_VEC_DOF, FEMCY_VEC_DOF_OLD, FEMCY_VEC_VEL, FEMCY_VEC_ACC, 0.25, 0.5, 0.1);
    double es = 0;
    rc |= femcy_elastic_energy_small(h, FEMCY_VEC_VEL, &es);
    int bad = femcy_mass_apply(h, 5, FEMCY_VEC_VEL, FEMCY_VEC_RHS, 1.0, 0);
    // the other two element passes that go through dispatch_element: a body load and a thermal load, created and applied
    int32_t bl = -1, th = -1;
    const double grav[2] = {0.0, -9.81 * 7.85e-3};
    std::vector<double> wts(nn), dT(nn), fth(nn * 2);
    for (int a = 0; a < nn; ++a) dT[a] = 20.0 + 5.0 * nodes[2 * a];
    rc |= femcy_bodyload_create(h, N, 0, nullptr, &bl);
    rc |= femcy_bodyload_weights(h, bl, wts.data());
    rc |= femcy_bodyload_apply(h, bl, grav, FEMCY_VEC_RHS, 0);
    rc |= femcy_thermal_create(h, N, 1.2e-5, dT.data(), &th);
    rc |= femcy_thermal_force(h, th, fth.data());
    rc |= femcy_thermal_apply(h, th, 1.0, FEMCY_VEC_RHS, 1);
    rc |= femcy_compute_strain_stress(h, FEMCY_VEC_DOF, 0);
    rc |= femcy_thermal_stress(h, th, 1.0);
    double area = 0; for (double v : wts) area += v;
    printf("rc=%d nn=%d total mass=%.6g (area 6 x rho = %.6g) ke=%.6g refused=%d body-load weights=%.6g (area 6)\n", rc, nn,
           total, 6 * 7.85e-3, ke, bad, area);
    femcy_ctx_destroy(h);
    return rc;
}
