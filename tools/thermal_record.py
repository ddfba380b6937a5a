"""Times of the thermal-load kernels at the bench size, beside k_geom, k_nodal_force and the body load on the same mesh in
the same process.

    python tools/thermal_record.py [--out profiles/thermal_record.json] [--reps 11]

On the 1 M C3D4 bench mesh (the twist plate at k = 12), medians of `--reps` launches, HIP events of the library's timing
class (FEMCY_OPT_TIMING) unless said otherwise:
  geom_us            k_geom<NPE,DM,false> of femcy_assemble_K on the undeformed mesh
  nodal_force_us     k_nodal_force of femcy_internal_force (its T_FORCE event pair)
  thermal_create_us  k_thermal_force + k_nodal_force of femcy_thermal_create (one event pair around both launches)
  body_create_us     k_body_weights + k_node_sum of femcy_bodyload_create (one event pair around both launches)
  thermal_apply_us   k_thermal_apply of one femcy_thermal_apply(add = 1)
  thermal_stress_us  k_thermal_post of one femcy_thermal_stress
  thermal_apply_wall_us / body_apply_wall_us
                     wall clock of `--apply-reps` back-to-back femcy_thermal_apply / femcy_bodyload_apply calls between two
                     stream synchronisations, i.e. launch to launch (femcy_bodyload_apply records no events)
What to look for: apply costs what k_body_apply costs, create stays within a k_geom pass plus a k_nodal_force pass.  No gate
hangs on these numbers: create runs once per solve."""
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


def _median_us(ctx, call, reps, key="geom"):
    """median over `reps` single calls of the time the library's events of class `key` recorded for it"""
    out = []
    for _ in range(reps):
        ctx.timing_reset()
        call()
        t = ctx.timing()
        out.append(1e3 * t[key + "_ms"] / max(t[key + "_launches"], 1))
    return float(np.median(out))


def _wall_us(ctx, call, reps):
    call()
    ctx.sync()
    t0 = time.perf_counter()
    for _ in range(reps):
        call()
    ctx.sync()
    return 1e6 * (time.perf_counter() - t0) / reps


def record(k, reps, apply_reps):
    m = meshgen.twist_plate_k(k)
    ELE = Element_linear_tetrahedral()
    ctx = be.Context(0)
    ctx.set_mesh(m["nodes"], m["elements"])
    ctx.set_element(ELE)
    ctx.set_material(LinearIsotropic(*m["elastic"]))
    ctx.build_pattern()
    nodes = np.asarray(m["nodes"], dtype=np.float64)
    dT = 50.0 + 30.0 * np.sin(nodes[:, 0] / np.abs(nodes[:, 0]).max() * 3.0) + 10.0 * nodes[:, 2] / np.abs(nodes[:, 2]).max()
    ctx.assemble_K(-1)                                   # warm-up
    th, bl = ctx.thermal(ELE, 1.2e-5, dT), ctx.bodyload(ELE)
    ctx.internal_force(be.VEC_DOF, be.VEC_FORCE)
    ctx.compute_strain_stress(be.VEC_DOF, large=False)
    ctx.set_option(be.OPT_TIMING, 1)
    out = {"mesh": "C3D4 k=%d" % k, "elements": int(ctx.ne), "nodes": int(ctx.nn), "reps": reps, "apply_reps": apply_reps}
    out["geom_us"] = _median_us(ctx, lambda: ctx.assemble_K(-1), reps)
    out["nodal_force_us"] = _median_us(ctx, lambda: ctx.internal_force(be.VEC_DOF, be.VEC_FORCE), reps, "force")
    out["thermal_create_us"] = _median_us(ctx, lambda: ctx.thermal(ELE, 1.2e-5, dT), reps)
    out["body_create_us"] = _median_us(ctx, lambda: ctx.bodyload(ELE), reps)
    out["thermal_apply_us"] = _median_us(ctx, lambda: ctx.thermal_apply(th, 0.5, be.VEC_RHS, add=True), reps)

    def stress():
        ctx.set_option(be.OPT_TIMING, 0)                 # the events of the post-processing pass are not wanted
        ctx.compute_strain_stress(be.VEC_DOF, large=False)
        ctx.set_option(be.OPT_TIMING, 1)
        ctx.timing_reset()
        ctx.thermal_stress(th, 0.5)

    out["thermal_stress_us"] = _median_us(ctx, stress, reps)
    ctx.set_option(be.OPT_TIMING, 0)
    b = np.array([0.0, 0.0, -9.81])
    out["thermal_apply_wall_us"] = _wall_us(ctx, lambda: ctx.thermal_apply(th, 0.5, be.VEC_RHS, add=True), apply_reps)
    out["body_apply_wall_us"] = _wall_us(ctx, lambda: ctx.bodyload_apply(bl, b, be.VEC_RHS, add=True), apply_reps)
    f = ctx.thermal_force(th).reshape(-1, 3)
    # the load is self-equilibrated: the resultant is rounding only (congruent cells add theirs coherently)
    out["resultant_over_largest"] = float(np.abs(f.sum(axis=0)).max() / np.abs(f).max())
    ctx.close()
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join("profiles", "thermal_record.json"))
    ap.add_argument("--k", type=int, default=12)
    ap.add_argument("--reps", type=int, default=11)
    ap.add_argument("--apply-reps", type=int, default=200)
    a = ap.parse_args()
    rows = [record(a.k, a.reps, a.apply_reps)]
    with open(a.out, "w") as f:
        json.dump({"records": rows}, f, indent=1)
    print(json.dumps({"records": rows}))


if __name__ == "__main__":
    main()
