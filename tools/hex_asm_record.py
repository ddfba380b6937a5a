"""Record: geometry + assembly time of C3D8 on the 995 328-hexahedron twist plate (192 x 24 x 216 cells), AUTO against
every generic mode that accepts the hexahedron, in ONE process, modes alternated launch by launch, one warm-up per mode,
median / min / max of the per-launch times from femcy_timing (HIP events around the two kernels).

    python tools/hex_asm_record.py [--cells 192 24 216] [--reps 20] [--out profiles/hex_asm_record.json]
                                   [--tune-pairs 163 161 ...]

Algorithmic bytes of one assembly: the element records read once (dsdx + det J w), the stored matrix written once, the
pair lists of the hex path.  The fraction of the 8 TB/s HBM peak is information only.

--tune-pairs times the hex path under each FEMCY_TUNE_PAIRS value in a block of its own after two warm-up launches
(a new value rebuilds the pair lists on the host: alternating values would time that rebuild).

Counters, in runs of their own (PMC only, no tracing), then merged into the record:
    rocprofv3 --pmc FETCH_SIZE WRITE_SIZE -d DIR -- python tools/hex_asm_record.py --modes AUTO --reps 2 --out SCRATCH
    python tools/hex_asm_record.py --merge-pmc AUTO:DIR [ROWS:DIR2 ...] --out profiles/hex_asm_record.json"""
import argparse
import glob
import json
import os
import sqlite3
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from femcy_amd import backend as be, meshgen                 # noqa: E402
from femcy_amd.element_zoo import Element_linear_hexahedral   # noqa: E402
from femcy_amd.material_zoo import LinearIsotropic            # noqa: E402

MODES = {"AUTO": be.ASM_AUTO, "PAIRS": be.ASM_PAIRS, "GATHER": be.ASM_GATHER, "GATHER_SYM": be.ASM_GATHER_SYM,
         "GATHER_SYM_ROWSUM": be.ASM_GATHER_SYM_ROWSUM, "ROWS": be.ASM_ROWS, "ATOMIC": be.ASM_ATOMIC}
NAMES = {v: k for k, v in MODES.items() if k != "AUTO"}
HBM_PEAK = 8.0e12
ASM_KERNELS = ("k_assemble_", "k_diag_from_rowsum")


def merge_pmc(specs, path):
    """add the counters of rocprofv3 PMC runs (LABEL:DIR, rocpd .db under DIR) to the record at `path`: per assembly
    kernel the mean per dispatch of every counter collected, and for FETCH_SIZE / WRITE_SIZE (KB as rocprofv3 reports
    them) the traffic against the algorithmic bytes of one assembly."""
    with open(path) as f:
        out = json.load(f)
    algo = out["bytes"]["records_read_once"] + out["bytes"]["K_written_stored"]
    pmc = out.setdefault("pmc", {})
    for spec in specs:
        label, d = spec.split(":", 1)
        ent = pmc.setdefault(label, {})
        for db in sorted(glob.glob(os.path.join(d, "**", "*.db"), recursive=True)):
            rows = sqlite3.connect(db).cursor().execute(
                "select kernel_name, counter_name, count(*), avg(value), avg(duration) from counters_collection "
                "group by kernel_name, counter_name").fetchall()
            for name, ctr, n, val, dur in rows:
                if not any(k in name for k in ASM_KERNELS):
                    continue
                k = ent.setdefault(name.split("(")[0], {"dispatches": 0, "avg_us": 0.0, "counters": {}})
                k["dispatches"], k["avg_us"] = n, dur / 1e3
                k["counters"][ctr] = val
        kb = {c: sum(k["counters"].get(c, 0.0) for k in ent.values() if isinstance(k, dict) and "counters" in k)
              for c in ("FETCH_SIZE", "WRITE_SIZE")}
        if kb["FETCH_SIZE"] or kb["WRITE_SIZE"]:
            ent["traffic"] = {"FETCH_SIZE_bytes": kb["FETCH_SIZE"] * 1024, "WRITE_SIZE_bytes": kb["WRITE_SIZE"] * 1024,
                              "algorithmic_bytes": algo,
                              "fetch_plus_write_over_algorithmic": (kb["FETCH_SIZE"] + kb["WRITE_SIZE"]) * 1024 / algo,
                              "note": "FETCH_SIZE as reported; on gfx950 it reads half the bytes of wide coalesced "
                                      "streaming reads, other access widths are uncalibrated"}
    with open(path, "w") as f:
        json.dump(out, f, indent=1)
    print(json.dumps(pmc, indent=1))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--cells", type=int, nargs=3, default=[192, 24, 216])
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "hex_asm_record.json"))
    ap.add_argument("--modes", nargs="+", default=list(MODES), choices=list(MODES),
                    help="a subset, e.g. AUTO alone under rocprofv3 --pmc")
    ap.add_argument("--tune-pairs", type=int, nargs="*", default=[],
                    help="also time the hex path under these FEMCY_TUNE_PAIRS values, each in a block of its own")
    ap.add_argument("--merge-pmc", nargs="+", metavar="LABEL:DIR",
                    help="merge rocprofv3 PMC runs into the record at --out instead of measuring")
    a = ap.parse_args()
    if a.merge_pmc:
        merge_pmc(a.merge_pmc, a.out)
        return
    modes = {k: MODES[k] for k in a.modes}
    t0 = time.time()
    m = meshgen.twist_plate_hex(*a.cells)
    nodes, el = m["nodes"], m["elements"]
    ctx = be.Context(0)
    ctx.set_mesh(nodes, el)
    ctx.set_element(Element_linear_hexahedral())
    ctx.set_material(LinearIsotropic(*m["elastic"]))
    info = ctx.build_pattern()
    print(f"[hex] {len(el)} C3D8, {len(nodes)} nodes, {ctx.n} DOF, nnzb {info.nnzb}, set-up {time.time() - t0:.1f} s",
          flush=True)
    ctx.set_option(be.OPT_TIMING, 1)
    runs = {}
    for name, mode in modes.items():                      # warm-up: code objects, pair lists, LDS attributes
        ctx.set_option(be.OPT_ASSEMBLY, mode)
        ctx.assemble_K(-1)
        ctx.sync()
        runs[name] = {"used": NAMES[ctx.assembly_used()], "geom_ms": [], "asm_ms": []}
    for _ in range(a.reps):
        for name, mode in modes.items():
            ctx.set_option(be.OPT_ASSEMBLY, mode)
            ctx.timing_reset()
            ctx.assemble_K(-1)
            ctx.sync()
            tm = ctx.timing()
            runs[name]["geom_ms"].append(tm["geom_ms"])
            runs[name]["asm_ms"].append(tm["assemble_ms"])
    knobs = {}
    for tune in a.tune_pairs:
        ctx.set_option(be.OPT_ASSEMBLY, be.ASM_PAIRS)
        ctx.set_option(be.TUNE_PAIRS, tune)
        for _ in range(2):
            ctx.assemble_K(-1)
        ctx.sync()
        s = []
        for _ in range(a.reps):
            ctx.timing_reset()
            ctx.assemble_K(-1)
            ctx.sync()
            s.append(ctx.timing()["assemble_ms"])
        s = np.array(s)
        knobs[str(tune)] = [float(np.median(s)), float(s.min()), float(s.max())]
        print(f"[hex] PAIRS tune {tune:4d}: assembly median {knobs[str(tune)][0]:8.3f} [{s.min():.3f}, {s.max():.3f}] ms",
              flush=True)
    ctx.set_option(be.TUNE_PAIRS, -1)
    ne, nGP = len(el), 8
    rec_bytes = ne * nGP * (8 * 3 + 1) * 8
    k_bytes = info.stored_blocks * 9 * 8
    nb_nnzb = info.nnzb * 9 * 8
    pair_words = int(np.bincount(el.ravel(), minlength=len(nodes)).sum())   # one 4-byte code per (row, element)
    out = {"workload": {"cells": a.cells, "elements": ne, "nodes": len(nodes), "dof": ctx.n, "nnzb": info.nnzb,
                        "stored_blocks": info.stored_blocks},
           "method": f"one process, modes alternated launch by launch, one warm-up each, {a.reps} launches per mode, "
                     "femcy_timing (HIP events around k_geom and the assembly kernels)",
           "bytes": {"records_read_once": rec_bytes, "K_written_stored": k_bytes, "K_written_nnz": nb_nnzb,
                     "pair_lists_at_least": 4 * pair_words},
           "modes": {}}
    if knobs:
        out["pairs_knobs_ms"] = {"method": "one block per FEMCY_TUNE_PAIRS value after two warm-up launches, median / "
                                           "min / max of the block", **knobs}
    for name, r in runs.items():
        g, s = np.array(r["geom_ms"]), np.array(r["asm_ms"])
        tot = g + s
        med = float(np.median(s))
        out["modes"][name] = {"ran": r["used"], "geom_ms": [float(np.median(g)), float(g.min()), float(g.max())],
                              "assemble_ms": [med, float(s.min()), float(s.max())],
                              "total_ms": [float(np.median(tot)), float(tot.min()), float(tot.max())],
                              "assemble_fraction_of_hbm_peak": (rec_bytes + k_bytes) / (med * 1e-3) / HBM_PEAK}
        print(f"[hex] {name:20s} ran {r['used']:18s} geom {np.median(g):8.3f} ms  assembly median {med:8.3f} "
              f"[{s.min():.3f}, {s.max():.3f}] ms", flush=True)
    if all(k in out["modes"] for k in ("AUTO", "ROWS", "GATHER_SYM_ROWSUM")):
        auto = out["modes"]["AUTO"]["assemble_ms"][0]
        best_generic = min(out["modes"][k]["assemble_ms"][0] for k in ("ROWS", "GATHER_SYM_ROWSUM"))
        out["auto_speedup_over_best_of_rows_and_gather_sym_rowsum"] = best_generic / auto
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(out, f, indent=1)
    print(json.dumps({k: v for k, v in out.items() if k != "modes"}))
    ctx.close()


if __name__ == "__main__":
    main()
