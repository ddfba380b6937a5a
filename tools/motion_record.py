"""Time of one explicit step at the bench size with and without prescribed motion, fixed and element by element.

    python tools/motion_record.py [--out profiles/explicit_motion.json] [--k 12] [--steps 200] [--reps 7]

The set-up and the timing of tools/explicit_damped_record.py (the 1 M C3D4 twist plate at rest, `--steps` steps enqueued
between two stream synchronisations, medians of `--reps` runs after a warm-up run), for an integrator without motion -- the
node pass every deck ran before, with its arguments -- and for the same integrator with its held foot moved along a smooth
step of value 0: the motion instantiation of the node pass and the small launch after a call's first drift run, and the
state stays at rest, so every step does the same work.  Without motion again at the end: the launches must be today's."""
import argparse
import json
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import explicit_record as rec                                                   # noqa: E402
from explicit_damped_record import _stat                                        # noqa: E402
from femcy_amd import backend as be, meshgen                                    # noqa: E402
from femcy_amd.element_zoo import Element_linear_tetrahedral                    # noqa: E402
from femcy_amd.material_zoo import LinearIsotropic                              # noqa: E402


def record(k, steps, reps, rho=7.85e-3):
    m = meshgen.twist_plate_k(k)
    ELE = Element_linear_tetrahedral()
    ctx = be.Context(0)
    ctx.set_mesh(m["nodes"], m["elements"])
    ctx.set_element(ELE)
    ctx.set_material(LinearIsotropic(*m["elastic"]))
    ctx.build_pattern()
    nodes = np.asarray(m["nodes"], dtype=np.float64)
    foot = np.nonzero(nodes[:, 2] < nodes[:, 2].min() + 1e-9)[0]
    held = ctx.dofset((foot[:, None] * 3 + np.arange(3)[None, :]).ravel())
    ex = ctx.explicit(ctx.lumped_mass(ELE, rho), [held])
    ctx.assemble_K(-1)
    dt_stable, omega = ctx.explicit_stable_dt(ex)
    h = 0.1 * dt_stable
    for v in (be.VEC_DOF, be.VEC_VEL, be.VEC_RHS):
        ctx.vector(v).fill(0.0)
    E, nu = m["elastic"]
    s_C = 3 * E * nu / (1 + nu) / (1 - 2 * nu) + E / (1 + nu)
    amp = ctx.amplitude("smooth step", [0.0, 1.0e6 * h], [0.0, 1.0])
    out = {"mesh": "C3D4 k=%d" % k, "elements": int(ctx.ne), "nodes": int(ctx.nn), "moved_dofs": int(foot.size * 3),
           "steps": steps, "reps": reps, "dt": h, "fixed": {}, "auto": {}}
    for name in ("none", "motion", "removed"):
        if name == "motion":
            ctx.explicit_set_motion(ex, [held], [0.0], [amp])
        else:
            ctx.explicit_set_motion(ex)
        ctx.explicit_start(ex, be.VEC_RHS, 1.0)
        out["fixed"][name] = _stat(rec._runs_us(ctx, lambda: ctx.explicit_advance(ex, steps, h, be.VEC_RHS, 1.0, 0.0), steps, reps))
        ctx.explicit_auto_begin(ex, s_C, 0.1, 1.0e9 * dt_stable, False, be.VEC_RHS)
        out["auto"][name] = _stat(rec._runs_us(ctx, lambda: ctx.explicit_auto_advance(ex, steps, be.VEC_RHS), steps, reps))
    out["state_at_rest"] = bool(ctx.vec_absmax(be.VEC_DOF) == 0.0)
    ctx.close()
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join("profiles", "explicit_motion.json"))
    ap.add_argument("--k", type=int, default=12)
    ap.add_argument("--steps", type=int, default=200)
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--commit", default=None)
    a = ap.parse_args()
    doc = {"commit": a.commit or rec._commit(), "records": [record(a.k, a.steps, a.reps)]}
    with open(a.out, "w") as f:
        json.dump(doc, f, indent=1)
    print(json.dumps(doc))


if __name__ == "__main__":
    main()
