"""Time of one explicit step at the bench size without a rigid wall and with one that nothing touches, fixed and element by
element.

    python tools/explicit_wall_record.py [--out profiles/explicit_wall.json] [--k 12] [--steps 200] [--reps 7]
                                         [--parent parent.json ...]

The set-up and the timing of tools/explicit_record.py (the 1 M C3D4 twist plate at rest, `--steps` steps enqueued between two
stream synchronisations, medians of `--reps` runs after a warm-up run), for femcy_explicit_advance and
femcy_explicit_auto_advance of an undamped integrator: without femcy_explicit_set_wall ("off": the launches of the
parent), with one wall far below the plate ("on": the wall variant of the node pass, which reads X and u and exchanges x
inside the quads) and after femcy_explicit_set_wall(nwalls = 0) ("off_again").  The state is at rest and no node reaches
the wall, so every step does the same work.  Each figure comes with its runs and their
spread (max - min) / median.  `--parent` merges records of tools/explicit_record.py run on the parent commit on the same
machine in the same session (`--merge` does so afterwards, without measuring): the off-path may differ from the parent's
only by the parent's own run-to-run spread."""
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

VARIANTS = ("off", "on", "off_again")


def _stat(us):
    med = float(np.median(us))
    return {"us_per_step": med, "runs_us": [round(x, 3) for x in us], "spread": float((max(us) - min(us)) / med)}


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
    s_C = 3 * (E * nu / (1 + nu) / (1 - 2 * nu)) + 2 * (E / 2 / (1 + nu))
    out = {"mesh": "C3D4 k=%d" % k, "elements": int(ctx.ne), "nodes": int(ctx.nn), "steps": steps, "reps": reps, "dt": h,
           "fixed": {}, "auto": {}}
    for name in VARIANTS:
        if name == "on":
            ctx.explicit_set_wall(ex, [nodes.min(axis=0) - 10.0 * np.ptp(nodes, axis=0).max()], [[0.0, 0.0, 1.0]], [0.1 * omega * omega])
        else:
            ctx.explicit_set_wall(ex)
        ctx.explicit_start(ex, be.VEC_RHS, 1.0)
        out["fixed"][name] = _stat(rec._runs_us(ctx, lambda: ctx.explicit_advance(ex, steps, h, be.VEC_RHS, 1.0, 0.0), steps, reps))
        if name == "on":
            out["wall_at_rest"] = [float(x) for x in ctx.explicit_wall_get(ex, 0)]
        ctx.explicit_auto_begin(ex, s_C, 0.1, 1.0e9 * dt_stable, False, be.VEC_RHS)
        out["auto"][name] = _stat(rec._runs_us(ctx, lambda: ctx.explicit_auto_advance(ex, steps, be.VEC_RHS), steps, reps))
        assert ctx.explicit_auto_state(ex)[3] == steps * (reps + 1)
    for mode in ("fixed", "auto"):
        out[mode]["on_over_off"] = out[mode]["on"]["us_per_step"] / out[mode]["off"]["us_per_step"] - 1.0
    out["state_at_rest"] = bool(ctx.vec_absmax(be.VEC_DOF) == 0.0)
    ctx.close()
    return out


def with_parents(doc, paths):
    """the figures of the parent's tools/explicit_record.py runs beside this commit's off-path; several runs of the parent
    (before and after this commit's) show its spread from run to run of the tool, beyond the spread inside one run"""
    doc["parent"] = []
    for path in paths:
        p = json.load(open(path))
        r = p["records"][0]
        doc["parent"].append({"commit": p.get("commit"), "fixed": _stat(r["fused_runs_us"]), "auto": _stat(r["auto_runs_us"])})
    for mode in ("fixed", "auto"):
        mine = doc["records"][0][mode]["off"]["us_per_step"]
        theirs = [q[mode]["us_per_step"] for q in doc["parent"]]
        doc["off_%s_vs_parent" % mode] = {"this": mine, "parent_min": min(theirs), "parent_max": max(theirs),
                                          "parent_run_to_run": (max(theirs) - min(theirs)) / min(theirs),
                                          "relative_to_parent_mean": mine / float(np.mean(theirs)) - 1.0}
    return doc


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join("profiles", "explicit_wall.json"))
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
