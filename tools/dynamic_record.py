"""Times of the implicit-dynamics kernels at the bench size, beside the stiffness product on the same context.

    python tools/dynamic_record.py [--out profiles/dynamic_record.json] [--reps 100]

On the 1 M C3D4 bench mesh (the twist plate at k = 12), after a warm-up call each, HIP events of the library's timing class
(FEMCY_OPT_TIMING, one pair per launch), mean over `--reps` launches unless said otherwise:
  mass_create_us     k_mass_points + k_mass_blocks of femcy_mass_create (one event pair around both launches; median of 11)
  mass_spmv_us       k_mass_spmv of femcy_mass_apply(add = 1)
  mass_add_to_K_us   k_mass_add_to_K of femcy_mass_add_to_K
  newmark_predict_us / newmark_update_us
  spmv_us            k_spmv of femcy_spmv on the same context (its T_SPMV event pair)
  step_wall_us       wall clock of one whole step of the hot path between two stream synchronisations: femcy_assemble_K,
                     mass_add_to_K, newmark_predict, mass_apply, Dirichlet rows, the tight PCG, newmark_update (mean of 5)
What to look for: the mass product moves 12 bytes per stored block where k_spmv moves 76, with the same gathers, and should
be the faster of the two.  No gate hangs on these numbers."""
import argparse
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from femcy_amd import backend as be, meshgen                                    # noqa: E402
from femcy_amd.element_zoo import Element_linear_tetrahedral                    # noqa: E402
from femcy_amd.material_zoo import LinearIsotropic                              # noqa: E402


def _mean_us(ctx, call, reps, key="geom", median=False):
    call()                                               # warm-up
    out = []
    for _ in range(reps):
        ctx.timing_reset()
        call()
        t = ctx.timing()
        out.append(1e3 * t[key + "_ms"] / max(t[key + "_launches"], 1))
    return float(np.median(out) if median else np.mean(out))


def record(k, reps):
    m = meshgen.twist_plate_k(k)
    ELE = Element_linear_tetrahedral()
    ctx = be.Context(0)
    ctx.set_mesh(m["nodes"], m["elements"])
    ctx.set_element(ELE)
    ctx.set_material(LinearIsotropic(*m["elastic"]))
    info = ctx.build_pattern()
    rho, beta, gamma, dt = 7.85e-9, 0.25, 0.5, 1.0e-5
    ctx.assemble_K(-1)
    ms = ctx.mass(ELE, rho)
    rng = np.random.default_rng(0)
    for vec in (be.VEC_DOF, be.VEC_DOF_OLD, be.VEC_VEL, be.VEC_ACC):
        ctx.upload(vec, 1e-3 * rng.standard_normal(ctx.n))
    out = {"mesh": "C3D4 k=%d" % k, "elements": int(ctx.ne), "nodes": int(ctx.nn), "stored_blocks": int(info.stored_blocks),
           "reps": reps}
    ctx.set_option(be.OPT_TIMING, 1)
    out["mass_create_us"] = _mean_us(ctx, lambda: ctx.mass(ELE, rho), 11, median=True)
    out["mass_spmv_us"] = _mean_us(ctx, lambda: ctx.mass_apply(ms, be.VEC_DOF, be.VEC_RHS, 1.0, add=True), reps)
    out["mass_add_to_K_us"] = _mean_us(ctx, lambda: ctx.mass_add_to_K(ms, 1.0e-3), reps)
    out["newmark_predict_us"] = _mean_us(ctx, lambda: ctx.newmark_predict(be.VEC_DOF, be.VEC_VEL, be.VEC_ACC, be.VEC_RESIDUAL,
                                                                         4.0, 2.0, 1.0), reps)
    out["newmark_update_us"] = _mean_us(ctx, lambda: ctx.newmark_update(be.VEC_DOF, be.VEC_DOF_OLD, be.VEC_VEL, be.VEC_ACC,
                                                                       beta, gamma, dt), reps)
    out["spmv_us"] = _mean_us(ctx, lambda: ctx.spmv(be.VEC_DOF, be.VEC_TMP0), reps, "spmv")
    ctx.set_option(be.OPT_TIMING, 0)
    foot = ctx.dofset(np.unique(np.concatenate([np.asarray(bc["node_set"]) * 3 + bc["dof"] for bc in m["dirichlet_bc_info"]])))
    a0 = 1.0 / (beta * dt * dt)
    for vec in (be.VEC_DOF, be.VEC_DOF_OLD, be.VEC_ACC):
        ctx.vector(vec).fill(0.0)

    def step():
        ctx.assemble_K(-1)
        ctx.mass_add_to_K(ms, a0)
        ctx.newmark_predict(be.VEC_DOF, be.VEC_VEL, be.VEC_ACC, be.VEC_RESIDUAL, a0, 1.0 / (beta * dt), 1.0 / (2 * beta) - 1.0)
        ctx.vector(be.VEC_RHS).fill(0.0)
        ctx.mass_apply(ms, be.VEC_RESIDUAL, be.VEC_RHS, 1.0, add=True)
        ctx.dofset_dirichlet_linear(foot, 0.0, be.VEC_RHS)
        it = ctx.pcg(be.VEC_RHS, be.VEC_X, eps=1.0e-12, maxit=10 * ctx.n)[0]
        ctx.vector(be.VEC_DOF).copy_from(ctx.vector(be.VEC_X))
        ctx.newmark_update(be.VEC_DOF, be.VEC_DOF_OLD, be.VEC_VEL, be.VEC_ACC, beta, gamma, dt)
        ctx.vector(be.VEC_DOF_OLD).copy_from(ctx.vector(be.VEC_DOF))
        return it

    step()
    ctx.sync()
    t0 = time.perf_counter()
    iters = [step() for _ in range(5)]
    ctx.sync()
    out["step_wall_us"] = 1e6 * (time.perf_counter() - t0) / 5
    out["step_pcg_iterations"] = iters
    ctx.close()
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join("profiles", "dynamic_record.json"))
    ap.add_argument("--k", type=int, default=12)
    ap.add_argument("--reps", type=int, default=100)
    a = ap.parse_args()
    rows = [record(a.k, a.reps)]
    with open(a.out, "w") as f:
        json.dump({"records": rows}, f, indent=1)
    print(json.dumps({"records": rows}))


if __name__ == "__main__":
    main()
