"""Time of one explicit step at the bench size, beside the same update composed from the calls the ABI had before.

    python tools/explicit_record.py [--out profiles/explicit_step.json] [--k 12] [--steps 200] [--reps 7]

On the 1 M C3D4 bench mesh (the twist plate at k = 12), medians of `--reps` runs after one warm-up run, each run `--steps`
steps enqueued back to back between two stream synchronisations (wall clock from launch to launch: the library has no entry
point that brackets several calls with one pair of events, and 200 steps of ~0.15 ms make the two synchronisations a
thousandth of the run):
  fused_us_per_step    femcy_explicit_advance(steps): the element pass + k_explicit_node per step
  unfused_us_per_step  femcy_internal_force (element pass, copy of u, k_nodal_force) + six femcy_vec_axpy per step that read
                       and write what the update reads and writes.  The ABI has no element-wise product, so a scalar stands
                       in for the inverse mass: the composition is a traffic and launch count, not the same numbers.
  force_eval_us        femcy_internal_force alone, the same way
  auto_us_per_step     femcy_explicit_auto_advance(steps): the element pass, the element bound + the clock tick and
                       k_explicit_node_auto per step (`*Dynamic, explicit, element by element`), T far away so that every
                       step is a real one; auto_over_fixed_us = that minus fused_us_per_step of the same build
  element_bound_us     femcy_explicit_element_bound alone, the same way (the bound kernel, the maximum and the read-back
                       that synchronises every call)
The increment is a tenth of the estimated stable one and the loads are zero, so the state stays at rest and every step does
the same work.  No gate hangs on these numbers: the correctness tests decide, the record states what the fusion gained."""
import argparse
import json
import os
import subprocess
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from femcy_amd import backend as be, meshgen                                    # noqa: E402
from femcy_amd.element_zoo import Element_linear_tetrahedral                    # noqa: E402
from femcy_amd.material_zoo import LinearIsotropic                              # noqa: E402


def _runs_us(ctx, run, steps, reps):
    """per-step microseconds of `reps` runs of `steps` steps, after one warm-up run"""
    run()
    ctx.sync()
    out = []
    for _ in range(reps):
        ctx.sync()
        t0 = time.perf_counter()
        run()
        ctx.sync()
        out.append(1e6 * (time.perf_counter() - t0) / steps)
    return out


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
    lm = ctx.lumped_mass(ELE, rho)
    ex = ctx.explicit(lm, [held])
    ctx.assemble_K(-1)
    dt_stable, omega = ctx.explicit_stable_dt(ex)
    h = 0.1 * dt_stable
    for v in (be.VEC_DOF, be.VEC_VEL, be.VEC_RHS, be.VEC_TMP1):
        ctx.vector(v).fill(0.0)
    ctx.explicit_start(ex, be.VEC_RHS, 1.0)
    c = float(1.0 / ctx.lumped_mass_get(lm).mean())

    def fused():
        ctx.explicit_advance(ex, steps, h, be.VEC_RHS, 1.0, 0.0)

    def unfused():
        for _ in range(steps):
            ctx.internal_force(be.VEC_DOF, be.VEC_FORCE)
            ctx.vec_axpy(be.VEC_TMP0, be.VEC_FORCE, -1.0, be.VEC_RHS)          # f_int - s f
            ctx.vec_axpy(be.VEC_VEL, be.VEC_VEL, 0.5 * h, be.VEC_ACC)          # v += h / 2 a
            ctx.vec_axpy(be.VEC_ACC, be.VEC_TMP1, -c, be.VEC_TMP0)             # a_new (TMP1 = 0)
            ctx.vec_axpy(be.VEC_VEL, be.VEC_VEL, 0.5 * h, be.VEC_ACC)          # v += h / 2 a_new
            ctx.vec_axpy(be.VEC_DOF, be.VEC_DOF, h, be.VEC_VEL)                # u += h v
            ctx.vec_axpy(be.VEC_DOF, be.VEC_DOF, 0.5 * h * h, be.VEC_ACC)      # u += h^2 / 2 a

    def force():
        for _ in range(steps):
            ctx.internal_force(be.VEC_DOF, be.VEC_FORCE)

    lam, mu = m["elastic"][0] * m["elastic"][1] / (1 + m["elastic"][1]) / (1 - 2 * m["elastic"][1]), m["elastic"][0] / 2 / (1 + m["elastic"][1])
    s_C = 3 * lam + 2 * mu

    def auto():
        ctx.explicit_auto_advance(ex, steps, be.VEC_RHS)

    def element_bound():
        for _ in range(steps):
            ctx.explicit_element_bound(ex, s_C, be.VEC_DOF)

    out = {"mesh": "C3D4 k=%d" % k, "elements": int(ctx.ne), "nodes": int(ctx.nn), "steps": steps, "reps": reps,
           "stable_dt": dt_stable, "omega_bound": omega, "dt": h}
    for name, run in (("fused", fused), ("unfused", unfused), ("force_eval", force), ("auto", auto), ("element_bound", element_bound)):
        if name == "auto":
            ctx.explicit_auto_begin(ex, s_C, 0.1, 1.0e9 * dt_stable, False, be.VEC_RHS)
        us = _runs_us(ctx, run, steps, reps)
        key = name + ("_us" if name in ("force_eval", "element_bound") else "_us_per_step")
        out[key], out[name + "_runs_us"] = float(np.median(us)), [round(x, 3) for x in us]
        if name == "auto":
            t, h_last, h_min, done = ctx.explicit_auto_state(ex)
            out["auto_steps_done"], out["auto_dt"] = done, h_last
            assert done == steps * (reps + 1) and h_last == h_min, (done, h_last, h_min)
    out["unfused_over_fused"] = out["unfused_us_per_step"] / out["fused_us_per_step"]
    out["auto_over_fixed_us"] = out["auto_us_per_step"] - out["fused_us_per_step"]
    out["element_stable_dt"] = 2.0 / ctx.explicit_element_bound(ex, s_C, be.VEC_DOF)
    out["state_at_rest"] = bool(ctx.vec_absmax(be.VEC_DOF) == 0.0)
    ctx.close()
    return out


def _commit():
    try:
        root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
        return subprocess.check_output(["git", "-C", root, "rev-parse", "--short", "HEAD"], stderr=subprocess.DEVNULL).decode().strip()
    except Exception:
        return None


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join("profiles", "explicit_step.json"))
    ap.add_argument("--k", type=int, default=12)
    ap.add_argument("--steps", type=int, default=200)
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--commit", default=None, help="the commit to record where the tree is not a git checkout")
    a = ap.parse_args()
    doc = {"commit": a.commit or _commit(), "records": [record(a.k, a.steps, a.reps)]}
    with open(a.out, "w") as f:
        json.dump(doc, f, indent=1)
    print(json.dumps(doc))


if __name__ == "__main__":
    main()
