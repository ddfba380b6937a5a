"""Time of one explicit step at the bench size, undamped and damped, fixed and element by element.

    python tools/explicit_damped_record.py [--out profiles/explicit_damped.json] [--k 12] [--steps 200] [--reps 7]
                                           [--parent parent.json]

The set-up and the timing of tools/explicit_record.py (the 1 M C3D4 twist plate at rest, `--steps` steps enqueued between two
stream synchronisations, medians of `--reps` runs after a warm-up run), for four variants of femcy_explicit_advance /
femcy_explicit_auto_advance: undamped, alpha alone (the node pass and the bound change), bulk viscosity alone (the damped
element pass) and both.  The state is at rest, so the damping forces are zero and every step does the same work.  Each figure
comes with its runs and their spread (max - min) / median.  `--parent` merges records of tools/explicit_record.py run on
the parent commit on the same machine in the same session (`--merge` does so afterwards, without measuring), so that the
undamped step can be compared: it may differ from the parent's only by the parent's own run-to-run spread."""
import argparse
import json
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import explicit_record as rec                                                   # noqa: E402
from femcy_amd import backend as be, meshgen                                    # noqa: E402
from femcy_amd.element_zoo import Element_linear_tetrahedral                    # noqa: E402
from femcy_amd.material_zoo import LinearIsotropic                              # noqa: E402

VARIANTS = {"undamped": (0.0, 0.0, 0.0), "alpha": (50.0, 0.0, 0.0), "bulk": (0.0, 0.06, 1.2), "alpha_bulk": (50.0, 0.06, 1.2)}


def _stat(us):
    med = float(np.median(us))
    return {"us_per_step": med, "runs_us": [round(x, 3) for x in us], "spread": float((max(us) - min(us)) / med)}


def record(k, steps, reps, rho=7.85e-3):
    m = meshgen.twist_plate_k(k)
    ELE = Element_linear_tetrahedral()
    material = LinearIsotropic(*m["elastic"])
    ctx = be.Context(0)
    ctx.set_mesh(m["nodes"], m["elements"])
    ctx.set_element(ELE)
    ctx.set_material(material)
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
    lam, mu = E * nu / (1 + nu) / (1 - 2 * nu), E / 2 / (1 + nu)
    s_C, M_d = 3 * lam + 2 * mu, float(np.asarray(material.C)[0][0])
    out = {"mesh": "C3D4 k=%d" % k, "elements": int(ctx.ne), "nodes": int(ctx.nn), "steps": steps, "reps": reps, "dt": h,
           "fixed": {}, "auto": {}}
    for name, (alpha, b1, b2) in VARIANTS.items():
        ctx.explicit_set_damping(ex, alpha, b1, b2, M_d if (b1 or b2) else 0.0)
        ctx.explicit_start(ex, be.VEC_RHS, 1.0)
        out["fixed"][name] = _stat(rec._runs_us(ctx, lambda: ctx.explicit_advance(ex, steps, h, be.VEC_RHS, 1.0, 0.0), steps, reps))
        ctx.explicit_auto_begin(ex, s_C, 0.1, 1.0e9 * dt_stable, False, be.VEC_RHS)
        out["auto"][name] = _stat(rec._runs_us(ctx, lambda: ctx.explicit_auto_advance(ex, steps, be.VEC_RHS), steps, reps))
        assert ctx.explicit_auto_state(ex)[3] == steps * (reps + 1)
    out["state_at_rest"] = bool(ctx.vec_absmax(be.VEC_DOF) == 0.0)
    ctx.close()
    return out


def with_parents(doc, paths):
    """the undamped figures of the parent's tools/explicit_record.py runs beside this commit's; several runs of the parent
    (before and after this commit's, say) show its spread from run to run of the tool, beyond the spread inside one run"""
    doc["parent"] = []
    for path in paths:
        p = json.load(open(path))
        r = p["records"][0]
        doc["parent"].append({"commit": p.get("commit"), "fixed_undamped": _stat(r["fused_runs_us"]),
                              "auto_undamped": _stat(r["auto_runs_us"])})
    for mode in ("fixed", "auto"):
        mine = doc["records"][0][mode]["undamped"]["us_per_step"]
        theirs = [q[mode + "_undamped"]["us_per_step"] for q in doc["parent"]]
        doc["undamped_%s_vs_parent" % mode] = {"this": mine, "parent_min": min(theirs), "parent_max": max(theirs),
                                               "parent_run_to_run": (max(theirs) - min(theirs)) / min(theirs),
                                               "relative_to_parent_mean": mine / float(np.mean(theirs)) - 1.0}
    return doc


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join("profiles", "explicit_damped.json"))
    ap.add_argument("--k", type=int, default=12)
    ap.add_argument("--steps", type=int, default=200)
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--commit", default=None)
    ap.add_argument("--parent", nargs="*", default=[], help="the JSON files tools/explicit_record.py wrote on the parent commit")
    ap.add_argument("--merge", default=None, help="a record of this tool to merge the parent files into, without measuring")
    a = ap.parse_args()
    if a.merge:
        doc = json.load(open(a.merge))
    else:
        doc = {"commit": a.commit or rec._commit(), "records": [record(a.k, a.steps, a.reps)]}
    if a.parent:
        with_parents(doc, a.parent)
    with open(a.out, "w") as f:
        json.dump(doc, f, indent=1)
    print(json.dumps(doc))


if __name__ == "__main__":
    main()
