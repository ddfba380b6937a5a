"""Record: geometry + assembly time of C3D6 on the 1 990 656-wedge twist plate (192 x 24 x 216 cells, two wedges per
cell, the 1 047 025 nodes of the hexahedron plate), PAIRS against the generic modes ROWS and GATHER_SYM_ROWSUM (and
AUTO), in ONE process, modes alternated launch by launch, one warm-up per mode, median / min / max of the per-launch
times from femcy_timing (HIP events around the kernels).  `auto_choice` names the faster of PAIRS and the best generic
mode: the mode launch_assemble's AUTO rule takes for C3D6.

    python tools/wedge_asm_record.py [--cells 192 24 216] [--reps 20] [--out profiles/wedge_asm_record.json]
                                     [--tune-pairs 163 161 ...]

Algorithmic bytes of one assembly: the element records read once (6 Gauss points x 6 nodes x 3 doubles + 6 volumes =
912 B per wedge) and the stored matrix written once (nnzb x 72 B; stored_blocks x 72 B with the SELL padding).  The
fraction of the 8 TB/s HBM peak is information only.

Counters, in runs of their own (PMC only, no tracing), merged into the record as tools/hex_asm_record.py does:
    rocprofv3 --pmc FETCH_SIZE -d DIR -- python tools/wedge_asm_record.py --modes PAIRS --reps 2 --out SCRATCH
    python tools/wedge_asm_record.py --merge-pmc PAIRS:DIR [PAIRS:DIR2 ...] --out profiles/wedge_asm_record.json"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tools")]

from femcy_amd import backend as be, meshgen                 # noqa: E402
from femcy_amd.element_zoo import Element_linear_wedge        # noqa: E402
from femcy_amd.material_zoo import LinearIsotropic            # noqa: E402
from hex_asm_record import HBM_PEAK, merge_pmc                # noqa: E402

MODES = {"AUTO": be.ASM_AUTO, "PAIRS": be.ASM_PAIRS, "ROWS": be.ASM_ROWS, "GATHER_SYM_ROWSUM": be.ASM_GATHER_SYM_ROWSUM}
NAMES = {be.ASM_GATHER: "GATHER", be.ASM_ATOMIC: "ATOMIC", be.ASM_ROWS: "ROWS", be.ASM_GATHER_SYM: "GATHER_SYM",
         be.ASM_GATHER_SYM_ROWSUM: "GATHER_SYM_ROWSUM", be.ASM_PAIRS: "PAIRS"}
GENERIC = ("ROWS", "GATHER_SYM_ROWSUM")


def _stats(x):
    x = np.asarray(x)
    return [float(np.median(x)), float(x.min()), float(x.max())]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--cells", type=int, nargs=3, default=[192, 24, 216])
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "wedge_asm_record.json"))
    ap.add_argument("--modes", nargs="+", default=list(MODES), choices=list(MODES))
    ap.add_argument("--tune-pairs", type=int, nargs="*", default=[],
                    help="also time PAIRS under these FEMCY_TUNE_PAIRS values, each in a block of its own")
    ap.add_argument("--merge-pmc", nargs="+", metavar="LABEL:DIR",
                    help="merge rocprofv3 PMC runs into the record at --out instead of measuring")
    a = ap.parse_args()
    if a.merge_pmc:
        merge_pmc(a.merge_pmc, a.out)
        return
    modes = {k: MODES[k] for k in a.modes}
    t0 = time.time()
    m = meshgen.twist_plate_wedge(*a.cells)
    nodes, el = m["nodes"], m["elements"]
    ctx = be.Context(0)
    ctx.set_mesh(nodes, el)
    ctx.set_element(Element_linear_wedge())
    ctx.set_material(LinearIsotropic(*m["elastic"]))
    info = ctx.build_pattern()
    print(f"[wedge] {len(el)} C3D6, {len(nodes)} nodes, {ctx.n} DOF, nnzb {info.nnzb}, set-up {time.time() - t0:.1f} s",
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
        knobs[str(tune)] = _stats(s)
        print(f"[wedge] PAIRS tune {tune:4d}: assembly median {knobs[str(tune)][0]:8.3f} ms", flush=True)
    ctx.set_option(be.TUNE_PAIRS, -1)
    ne, nGP = len(el), 6
    rec_bytes = ne * nGP * (6 * 3 + 1) * 8                # 912 B per wedge
    k_bytes = info.nnzb * 9 * 8
    out = {"workload": {"cells": a.cells, "elements": ne, "nodes": len(nodes), "dof": ctx.n, "nnzb": info.nnzb,
                        "stored_blocks": info.stored_blocks, "max_row_blocks": info.max_row_blocks,
                        "max_node_elems": info.max_node_elems},
           "method": f"one process, modes alternated launch by launch, one warm-up each, {a.reps} launches per mode, "
                     "femcy_timing (HIP events around k_geom and the assembly kernels)",
           "bytes": {"records_read_once": rec_bytes, "K_written_once": k_bytes,
                     "K_written_stored": info.stored_blocks * 9 * 8, "K_written_stored_note": "with SELL padding"},
           "modes": {}}
    if knobs:
        out["pairs_knobs_ms"] = {"method": "one block per FEMCY_TUNE_PAIRS value after two warm-up launches, median / "
                                           "min / max of the block", **knobs}
    for name, r in runs.items():
        s = _stats(r["asm_ms"])
        out["modes"][name] = {"ran": r["used"], "geom_ms": _stats(r["geom_ms"]), "assemble_ms": s,
                              "total_ms": _stats(np.add(r["geom_ms"], r["asm_ms"])),
                              "assemble_fraction_of_hbm_peak": (rec_bytes + k_bytes) / (s[0] * 1e-3) / HBM_PEAK}
        print(f"[wedge] {name:20s} ran {r['used']:18s} geom {out['modes'][name]['geom_ms'][0]:8.3f} ms  assembly median "
              f"{s[0]:8.3f} [{s[1]:.3f}, {s[2]:.3f}] ms", flush=True)
    if "PAIRS" in out["modes"] and all(k in out["modes"] for k in GENERIC):
        best = min(GENERIC, key=lambda k: out["modes"][k]["assemble_ms"][0])
        pairs = out["modes"]["PAIRS"]["assemble_ms"][0]
        out["pairs_speedup_over_best_generic"] = out["modes"][best]["assemble_ms"][0] / pairs
        out["auto_choice"] = "PAIRS" if pairs < out["modes"][best]["assemble_ms"][0] else best
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(out, f, indent=1)
    print(json.dumps({k: v for k, v in out.items() if k != "modes"}))
    ctx.close()


if __name__ == "__main__":
    main()
