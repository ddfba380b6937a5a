"""Time of femcy_lumped_mass_scale at the bench size, once per rule, and of the undamped explicit step beside it.

    python tools/mass_scaling_record.py [--out profiles/mass_scaling.json] [--k 12] [--steps 200] [--reps 7]
                                        [--parent parent.json ...] [--merge record.json]

The set-up and the step timing of tools/explicit_record.py (the 1 M C3D4 twist plate at rest, `--steps` steps enqueued between
two stream synchronisations, medians of `--reps` runs after a warm-up run).  The scaling call is a set-up call that
synchronises, so it is timed with the host clock around the call, each on a fresh lumped mass; the first call of the process
(which loads the code object) is made before the timed ones and reported apart.  The steps are timed on an integrator made
from an unscaled lumped mass and on one made from a scaled one: the kernels are the same, only the numbers in minv and me
differ.  `--parent` merges records of tools/explicit_record.py run on the parent commit in the same session (`--merge` does so
afterwards, without measuring)."""
import argparse
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import explicit_record as rec                                                   # noqa: E402
from explicit_damped_record import _stat                                        # noqa: E402
from femcy_amd import backend as be, meshgen                                    # noqa: E402
from femcy_amd.element_zoo import Element_linear_tetrahedral                    # noqa: E402
from femcy_amd.material_zoo import LinearIsotropic                              # noqa: E402

CALLS = {"factor": dict(factor=4.0), "below min": dict(dt=1.0, type="below min"), "set equal dt": dict(dt=1.0, type="set equal dt"),
         "uniform": dict(dt=1.0, type="uniform")}


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
    E, nu = m["elastic"]
    s_C = 3 * E * nu / (1 + nu) / (1 - 2 * nu) + E / (1 + nu)
    for v in (be.VEC_DOF, be.VEC_VEL, be.VEC_RHS):
        ctx.vector(v).fill(0.0)
    out = {"mesh": "C3D4 k=%d" % k, "elements": int(ctx.ne), "nodes": int(ctx.nn), "steps": steps, "reps": reps, "scale_call": {},
           "fixed": {}, "auto": {}}
    plain = ctx.lumped_mass(ELE, rho)
    ex = ctx.explicit(plain, [held])
    dt_e = 2.0 / ctx.explicit_element_bound(ex, s_C, be.VEC_DOF)               # the smallest element increment of the mesh
    t0 = time.perf_counter()
    ctx.lumped_mass_scale(ctx.lumped_mass(ELE, rho), s_C, None, 1.5 * dt_e, "below min")
    out["first_call_ms"] = 1.0e3 * (time.perf_counter() - t0)                  # with the creation of its lumped mass
    scaled = None
    for name, kw in CALLS.items():
        ms = []
        for _ in range(reps):
            lm = ctx.lumped_mass(ELE, rho)
            ctx.sync()
            t0 = time.perf_counter()
            res = ctx.lumped_mass_scale(lm, s_C, kw.get("factor"), 1.5 * dt_e if "dt" in kw else None, kw.get("type", "below min"))
            ms.append(1.0e3 * (time.perf_counter() - t0))
            scaled = lm if name == "below min" else scaled
        out["scale_call"][name] = {"ms": float(np.median(ms)), "runs_ms": [round(x, 4) for x in ms],
                                   "spread": float((max(ms) - min(ms)) / np.median(ms)), "result": res}
    ctx.assemble_K(-1)
    for label, lm in (("unscaled", plain), ("scaled", scaled)):
        ex = ctx.explicit(lm, [held])
        dt_stable, _ = ctx.explicit_stable_dt(ex)
        h = 0.1 * dt_stable
        ctx.explicit_start(ex, be.VEC_RHS, 1.0)
        out["fixed"][label] = _stat(rec._runs_us(ctx, lambda: ctx.explicit_advance(ex, steps, h, be.VEC_RHS, 1.0, 0.0), steps, reps))
        ctx.explicit_auto_begin(ex, s_C, 0.1, 1.0e9 * dt_stable, False, be.VEC_RHS)
        out["auto"][label] = _stat(rec._runs_us(ctx, lambda: ctx.explicit_auto_advance(ex, steps, be.VEC_RHS), steps, reps))
        out["fixed"][label]["stable_dt"] = dt_stable
    out["state_at_rest"] = bool(ctx.vec_absmax(be.VEC_DOF) == 0.0)
    ctx.close()
    return out


def with_parents(doc, paths):
    """the figures of the parent's tools/explicit_record.py runs beside this commit's unscaled ones"""
    doc["parent"] = []
    for path in paths:
        p = json.load(open(path))
        r = p["records"][0]
        doc["parent"].append({"commit": p.get("commit"), "fixed": _stat(r["fused_runs_us"]), "auto": _stat(r["auto_runs_us"])})
    return doc


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join("profiles", "mass_scaling.json"))
    ap.add_argument("--k", type=int, default=12)
    ap.add_argument("--steps", type=int, default=200)
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--commit", default=None)
    ap.add_argument("--parent", nargs="*", default=[], help="the JSON files tools/explicit_record.py wrote on the parent commit")
    ap.add_argument("--merge", default=None, help="a record of this tool to merge the parent files into, without measuring")
    a = ap.parse_args()
    doc = json.load(open(a.merge)) if a.merge else {"commit": a.commit or rec._commit(), "records": [record(a.k, a.steps, a.reps)]}
    if a.parent:
        with_parents(doc, a.parent)
    with open(a.out, "w") as f:
        json.dump(doc, f, indent=1)
    print(json.dumps(doc))


if __name__ == "__main__":
    main()
