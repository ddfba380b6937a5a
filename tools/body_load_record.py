"""Times of the body-load kernels at the bench sizes, beside k_geom on the same mesh in the same process.

    python tools/body_load_record.py [--out profiles/body_load_record.json] [--reps 10]

Per mesh (1 M C3D4: the twist plate at k = 12; 124 k C3D10: k = 6, quadratic):
  geom_us      k_geom<NPE,DM,false> of femcy_assemble_K on the undeformed mesh (HIP events of the library's timing class)
  weights_us   k_body_weights + k_node_sum of femcy_bodyload_create (one event pair around both launches)
  apply_us     one femcy_bodyload_apply(add = 1): wall clock of `--apply-reps` back-to-back calls between two stream
               synchronisations, i.e. launch to launch
No gate hangs on these numbers: create runs once per solve."""
import argparse
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from femcy_amd import backend as be, meshgen                                    # noqa: E402
from femcy_amd.element_zoo import Element_linear_tetrahedral, Element_quadratic_tetrahedral   # noqa: E402
from femcy_amd.material_zoo import LinearIsotropic                              # noqa: E402


def record(name, k, quadratic, reps, apply_reps):
    m = meshgen.twist_plate_k(k, quadratic=quadratic)
    ELE = Element_quadratic_tetrahedral() if quadratic else Element_linear_tetrahedral()
    ctx = be.Context(0)
    ctx.set_mesh(m["nodes"], m["elements"])
    ctx.set_element(ELE)
    ctx.set_material(LinearIsotropic(*m["elastic"]))
    ctx.build_pattern()
    ctx.set_option(be.OPT_TIMING, 1)
    ctx.assemble_K(-1)                                   # warm-up
    bl = ctx.bodyload(ELE)
    ctx.timing_reset()
    for _ in range(reps):
        ctx.assemble_K(-1)
    t = ctx.timing()
    geom_us = 1e3 * t["geom_ms"] / t["geom_launches"]
    ctx.timing_reset()
    ids = [ctx.bodyload(ELE) for _ in range(reps)]
    t = ctx.timing()
    weights_us = 1e3 * t["geom_ms"] / t["geom_launches"]
    ctx.set_option(be.OPT_TIMING, 0)
    b = np.array([0.0, 0.0, -9.81])
    ctx.bodyload_apply(bl, b, be.VEC_RHS)
    ctx.sync()
    t0 = time.perf_counter()
    for _ in range(apply_reps):
        ctx.bodyload_apply(bl, b, be.VEC_RHS, add=True)
    ctx.sync()
    apply_us = 1e6 * (time.perf_counter() - t0) / apply_reps
    weights = ctx.bodyload_weights(ids[-1])
    out = {"mesh": name, "elements": int(ctx.ne), "nodes": int(ctx.nn), "geom_us": geom_us, "weights_us": weights_us,
           "apply_us": apply_us, "reps": reps, "apply_reps": apply_reps, "volume": float(weights.sum())}
    ctx.close()
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join("profiles", "body_load_record.json"))
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--apply-reps", type=int, default=200)
    a = ap.parse_args()
    rows = [record("C3D4 k=12", 12, False, a.reps, a.apply_reps), record("C3D10 k=6", 6, True, a.reps, a.apply_reps)]
    with open(a.out, "w") as f:
        json.dump({"records": rows}, f, indent=1)
    print(json.dumps({"records": rows}))


if __name__ == "__main__":
    main()
