"""-m gpu: bench.py prints exactly one JSON line with the contract's keys (small mesh, seconds)."""
import json
import os
import subprocess
import sys

import pytest

from helpers import ROOT

pytestmark = pytest.mark.gpu


def test_bench_json_contract():
    out = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--steps", "2", "--warmup", "1", "--iters", "20",
                          "--cells", "16,4,24", "--full"], capture_output=True, text=True, timeout=600, cwd=ROOT)
    assert out.returncode == 0, out.stderr[-2000:]
    lines = [l for l in out.stdout.splitlines() if l.strip()]
    assert len(lines) == 1, out.stdout
    d = json.loads(lines[0])
    for key, typ in (("metric", str), ("value", float), ("unit", str), ("n_gpus", int), ("steps", int), ("warmup", int),
                     ("ms_per_step", float), ("higher_is_better", bool), ("scaling", str), ("dtype", str),
                     ("data", str), ("config", dict), ("roofline", dict), ("cpu_baseline", dict)):
        assert isinstance(d[key], typ), (key, d[key])
    assert d["vs_baseline"] is None and d["n_gpus"] == 1 and d["steps"] == 2 and d["dtype"] == "f64"
    assert d["metric"].startswith("CG iters/sec") and "workload" in d["config"] and "model" not in d["config"]
    r = d["roofline"]
    assert r["bound"] == "hbm" and r["unit"] == "GB/s" and r["peak"] == 8000.0
    assert abs(r["frac"] - r["achieved"] / r["peak"]) < 1e-12 and r["achieved"] > 0 and r["launches_timed"] > 0
    c = d["cpu_baseline"]
    assert c["kind"] == "port" and c["cores"] >= 1 and c["value"] > 0 and c["unit"] == "CG iters/s" and c["sample"]
    # round 4: the host-backend point also as scalar keys (nested objects got lost in the driver's parsed record)
    assert c["host_backend_value"] == c["host_backend"]["value"] > 0 and c["host_backend_threads"] >= 1
    assert d["value"] > 0 and d["cg_iters_per_s"] > 0 and d["assemblies_per_s"] > 0


def test_bench_plain_line_and_dumped_outputs(tmp_path):
    """a run without --full carries the headline only; --dump-outputs writes what the last timed step computed -- K
    after the Dirichlet treatment (sampled block rows), the right-hand side and the PCG iterate -- and it is what the
    oracle computes for the same mesh and state"""
    import numpy as np
    sys.path.insert(0, ROOT)
    import bench
    from femcy_amd import meshgen
    from femcy_amd.user_defined import user_dirichletBC_values
    from oracle import femcy_oracle as orc
    from oracle.elements import elem_def
    out = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--steps", "3", "--warmup", "1", "--iters", "20",
                          "--prewarm", "0", "--cells", "16,4,24", "--dump-outputs", str(tmp_path)],
                         capture_output=True, text=True, timeout=600, cwd=ROOT)
    assert out.returncode == 0, out.stderr[-2000:]
    lines = [l for l in out.stdout.splitlines() if l.strip()]
    assert len(lines) == 1, out.stdout
    d = json.loads(lines[0])
    assert d["steps"] == 3 and d["ms_per_step"] > 0 and d["value"] > 0 and d["dtype"] == "f64" and d["higher_is_better"]
    assert not {"roofline", "cpu_baseline", "hbm_bound", "direct_branch", "strong_scaling"} & set(d)
    files = {f: np.load(tmp_path / f) for f in os.listdir(tmp_path)}
    assert set(files) == {"x.npy", "residual.npy", "pcg.npy", "K_blocks.npy", "K_block_index.npy"}
    assert all(a.dtype == np.float64 for a in files.values()) and sum(a.nbytes for a in files.values()) < 64 << 20

    m = meshgen.twist_plate(16, 4, 24)
    u, cons = bench.s1_state(m["nodes"], m["dirichlet_bc_info"], user_dirichletBC_values)
    topo = orc.Topology(m["nodes"], m["elements"], elem_def("C3D4"))
    mat = orc.Material("lin3d", m["elastic"])
    Ko = orc._zero_rows_cols_unit_diag(orc.assemble_K(topo, u, mat.C), cons).tocsr()
    fo = orc.internal_force(topo, u, mat)[0]
    fo[cons] = 0.0
    assert files["x.npy"].shape == files["residual.npy"].shape == (Ko.shape[0],)
    assert np.abs(files["residual.npy"] - fo).max() <= 1e-11 * np.abs(fo).max()
    idx, blocks = files["K_block_index.npy"].astype(np.int64), files["K_blocks.npy"]
    assert blocks.shape == (idx.shape[0], 3, 3) and idx.shape[0] > 2048
    ref = np.stack([Ko[3 * r:3 * r + 3, 3 * c:3 * c + 3].toarray() for r, c in idx])
    assert np.abs(blocks - ref).max() <= 1e-12 * abs(Ko).max()
    it, r0, rmax = files["pcg.npy"]
    assert it == 20 and r0 > 0
    xo = orc.pcg_reference(Ko, fo, eps=0.0, maxit=20)[0]
    assert np.linalg.norm(files["x.npy"] - xo) <= 1e-8 * np.linalg.norm(xo)


def test_bench_c3d10_workload_and_forced_comm():
    """the configs[4] workload line and the N = 1 run of the RCCL exchange path (both exchange forms, the neighbour
    one with the overlapped schedule) keep the same contract"""
    base = [sys.executable, os.path.join(ROOT, "bench.py"), "--steps", "1", "--warmup", "1", "--iters", "20", "--prewarm", "0",
            "--full", "--no-cpu-baseline"]
    for extra, workload in ((["--workload", "c3d10", "--cells", "8,2,12"], "C3D10"),
                            (["--cells", "16,4,24", "--force-comm", "--exchange", "allreduce"], "C3D4"),
                            (["--cells", "16,4,24", "--force-comm", "--exchange", "neighbour"], "C3D4")):
        out = subprocess.run(base + extra, capture_output=True, text=True, timeout=600, cwd=ROOT)
        assert out.returncode == 0, out.stderr[-2000:]
        lines = [l for l in out.stdout.splitlines() if l.strip()]
        assert len(lines) == 1, out.stdout
        d = json.loads(lines[0])
        assert workload in d["config"]["workload"] and d["value"] > 0 and d["n_gpus"] == 1 and "cpu_baseline" not in d
        assert d["roofline"]["bound"] == "hbm" and d["roofline"]["traffic"] is None       # non-standard --cells
        if "--force-comm" in extra:
            assert d["config"]["interface_exchange"]["exchange"] == extra[-1]
            # round 4: a communicator run reports BOTH PCG paths, the rank count RCCL saw and the mailbox probe
            pm = d["config"]["persistent_pcg_across_ranks"]
            assert d["config"]["interface_exchange"]["communicator_ranks"] == 1
            assert pm["us_per_iteration"]["three_launches_plus_collectives"] > 0
            if pm["enabled"]:
                assert pm["us_per_iteration"]["persistent_across_ranks"] > 0
            assert pm["mailbox_round_trip_us"] is None or 0.0 < pm["mailbox_round_trip_us"] < 1000.0


def test_bench_headline_workload_runs_the_persistent_pcg():
    """the 1 M-element configuration the metric is quoted on: the PCG solves are single launches of k_pcg_persist, and
    the roofline object prices THAT kernel against the ceiling that binds it -- the bytes its layout moves per launch /
    HIP-event time of the launch, over the stream rate probed in the kernel's own launch shape: a fraction <= 1 -- with
    the algorithmic figure of SURVEY.md 8d (which exceeds the HBM peak) under its own name"""
    out = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--steps", "2", "--warmup", "1", "--iters", "100",
                          "--prewarm", "0", "--full", "--no-cpu-baseline", "--hbm-bound", "off"], capture_output=True, text=True,
                         timeout=900, cwd=ROOT)
    assert out.returncode == 0, out.stderr[-2000:]
    lines = [l for l in out.stdout.splitlines() if l.strip()]
    assert len(lines) == 1, out.stdout
    d = json.loads(lines[0])
    r = d["roofline"]
    assert "995328 elements" in d["config"]["workload"] and d["config"]["cg_iters_per_step"] == 100
    assert r["kernel"].startswith("k_pcg_persist") and r["launches_timed"] == 2 and r["bound"] == "infinity-cache"
    spmv_bytes = 8 * 23454045 + 4 * 2606005 + 4 * (182845 + 1) + 16 * 548535          # SURVEY.md 8d at this size
    assert r["algorithmic_bytes_per_launch"] == 100 * (spmv_bytes + 88 * 548535)
    assert abs(r["algorithmic_gbs"] - r["algorithmic_bytes_per_launch"] / (r["avg_launch_us"] * 1e-6) / 1e9) < 1e-6 * r["algorithmic_gbs"]
    # what the kernel moves: the streamed block rows (less than the stored 198 MB, more than a third of it) + 16 n
    assert 60e6 < r["streamed_matrix_bytes_per_iteration"] < 150e6
    assert r["bytes_per_iteration"] == r["streamed_matrix_bytes_per_iteration"] + 16 * 548535
    assert r["bytes_per_launch"] == 100 * r["bytes_per_iteration"]
    assert abs(r["achieved"] - r["bytes_per_launch"] / (r["avg_launch_us"] * 1e-6) / 1e9) < 1e-6 * r["achieved"]
    assert r["peak"] > 1000.0 and abs(r["frac"] - r["achieved"] / r["peak"]) < 1e-12 and 0.05 < r["frac"] <= 1.0
    tmod = r["time_model"]
    assert tmod["exchanges_per_iteration"] == 3 and 0.3 < tmod["exchange_us"] < 20.0
    assert abs(tmod["floor_us_per_iteration"] - (tmod["stream_us"] + 3 * tmod["exchange_us"])) < 1e-9
    assert 0.1 < tmod["frac"] <= 1.0
    # round 4: the same as scalar keys, and SURVEY 8d's fraction of the HBM peak under its own name (> 1 here: the
    # bytes that never reach HBM are counted -- labelled as such)
    assert r["time_model_floor_us_per_iteration"] == tmod["floor_us_per_iteration"] and r["time_model_frac"] == tmod["frac"]
    assert r["time_model_exchanges_per_iteration"] == 3 and r["time_model_stream_us"] == tmod["stream_us"]
    assert r["frac_8d_vs_hbm"] == r["algorithmic_frac_of_hbm_peak"] and "cache-resident" in r["frac_8d_vs_hbm_note"]
    assert 10.0 < r["avg_launch_us"] / 100 < 60.0                                      # us per iteration inside the launch
    assert abs(d["pcg_us_per_iter"] - r["avg_launch_us"] / 100) < 5.0                  # the solve IS that launch (+ Jacobi, copy-back)
    assert "hbm_bound" not in d


def test_direct_branch_record_of_the_bench_line():
    """`direct_branch` of the default N = 1 line: the reference's spsolve branch on a deck-sized system, both solvers
    timed, the same answer"""
    sys.path.insert(0, ROOT)
    import bench
    from femcy_amd import backend as be, meshgen
    from femcy_amd.element_zoo import Element_linear_tetrahedral
    from femcy_amd.material_zoo import LinearIsotropic
    from femcy_amd.user_defined import user_dirichletBC_values
    msh = meshgen.twist_plate(8, 2, 12)
    rec = bench.direct_branch_record(be, "twist plate 8x2x12", msh, Element_linear_tetrahedral(),
                                     LinearIsotropic(*msh["elastic"]), user_dirichletBC_values, reps=2)
    assert rec["dof"] == msh["nodes"].size and 0 < rec["sub_diagonals"] < rec["dof"] and rec["panels"] == (rec["dof"] + 31) // 32
    assert rec["direct_ms"] > 0 and rec["tight_pcg_ms"] > 0 and rec["tight_pcg_iterations"] > 10
    assert rec["negative_pivots"] == 0 and rec["residual"] <= 1e-10 and rec["rel_diff_direct_vs_pcg"] <= 1e-8
    json.dumps(rec)


def test_bench_cpe8_workload_line():
    """`--workload cpe8` (BASELINE configs[1], round 5): the contract's line on a generated plane-strain CPE8 beam; the
    roofline object prices the dominant kernel of the timed region, `hbm_bound[0]` carries the k_spmv<2> product launch
    to launch, the PCG iteration on both paths and the assembly rate"""
    out = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--workload", "cpe8", "--cells", "600,60", "--steps", "2",
                          "--warmup", "1", "--iters", "50", "--prewarm", "0", "--full", "--no-cpu-baseline"], capture_output=True, text=True,
                         timeout=600, cwd=ROOT)
    assert out.returncode == 0, out.stderr[-2000:]
    lines = [l for l in out.stdout.splitlines() if l.strip()]
    assert len(lines) == 1, out.stdout
    d = json.loads(lines[0])
    assert d["metric"].startswith("CG iters/sec") and d["n_gpus"] == 1 and d["dtype"] == "f64" and d["vs_baseline"] is None
    assert "CPE8 600x60" in d["config"]["workload"] and "configs[1]" in d["config"]["workload"] and d["config"]["cg_iters_per_step"] == 50
    assert d["value"] > 0 and d["assemblies_per_s"] > 0 and d["pcg_us_per_iter"] > 0 and d["steps"] == 2
    r = d["roofline"]
    assert r["bound"] in ("hbm", "infinity-cache") and r["unit"] == "GB/s" and r["achieved"] > 0 and r["traffic"] is None
    assert r["kernel"].startswith("k_pcg_persist<2>") or r["kernel"].startswith("k_spmv<2>")
    assert r["spmv_launch_to_launch_us"] > 0 and 0 < r["spmv_frac_of_hbm_peak"] < 1.5
    h = d["hbm_bound"][0]
    assert h["dof"] == 2 * ((2 * 600 + 1) * (2 * 60 + 1) - 600 * 60) and h["elements"] == 36000
    assert h["spmv"]["kernel"].startswith("k_spmv<2>") and h["spmv"]["bound"] == "hbm" and h["spmv"]["peak"] == 8000.0
    assert abs(h["spmv"]["frac"] - h["spmv"]["achieved"] / 8000.0) < 1e-12 and h["spmv"]["launches_timed"] > 0
    p = h["pcg_iteration"]
    assert p["path"] in ("persistent", "three-kernel") and p["us"] > 0 and p["three_launch_us"] > 0
    assert (p["path"] == "persistent") == (p["persistent_streamed_bytes"] is not None)
    assert h["assembly_ms"] > 0 and h["assemblies_per_s"] > 0


def test_hbm_bound_records_of_the_default_line_have_the_2d_configuration():
    """the default N = 1 line carries three HBM-bound configurations since round 5: 8 M C3D4, 124 k C3D10 and the CPE8
    beam of ~1 M DOF (`hbm_bound[2]`); here the record builder on a small beam"""
    sys.path.insert(0, ROOT)
    import bench
    from femcy_amd import backend as be, meshgen
    from femcy_amd.element_zoo import Element_quadratic_quadrilateral
    from femcy_amd.material_zoo import LinearIsotropicPlaneStrain
    from femcy_amd.user_defined import user_dirichletBC_values
    assert bench.CPE8_CELLS == (1280, 128) and "configs[1]" in bench.CPE8_NAME
    msh = meshgen.beam_quad8(360, 60, plane="CPE8")
    rec = bench.hbm_bound_record(be, "beam CPE8 360x60", msh, Element_quadratic_quadrilateral(),
                                 LinearIsotropicPlaneStrain(*msh["elastic"]), user_dirichletBC_values, None, iters=40, spmv_reps=10)
    assert rec["dof"] == msh["nodes"].size and rec["spmv"]["kernel"].startswith("k_spmv<2>")
    assert rec["spmv"]["bytes_per_launch"] > 0 and rec["pcg_iteration"]["bytes"] == rec["spmv"]["bytes_per_launch"] + 88 * rec["dof"]
    assert rec["stored_matrix_mb"] > 0 and rec["pcg_iteration"]["three_launch_us"] > 0
    json.dumps(rec)


def test_committed_pmc_traffic_belongs_to_the_shipped_kernels_and_layout():
    """`roofline.traffic` of the driver's line (verdict of round 5: it came out null because the record was fingerprinted
    by whole source files).  The committed profiles/spmv_traffic.json must be the record of THIS library's PCG kernels
    (machine-code fingerprint) and of the layout `femcy_build_pattern` produces for the headline mesh today -- i.e.
    `bench.py` on the standard workloads will carry a non-null `traffic` with `traffic_over_moved` close to 1."""
    import json
    import bench
    from femcy_amd import backend as be, meshgen
    from femcy_amd.element_zoo import Element_linear_tetrahedral
    from femcy_amd.material_zoo import LinearIsotropic
    doc = json.load(open(os.path.join(ROOT, "profiles", "spmv_traffic.json")))
    assert set(doc["workloads"]) >= {"c3d4", "c3d10", "cpe8"}
    for wl, entry in doc["workloads"].items():                  # every workload: the instantiation its passes ran, as shipped
        assert entry["kernel_sha"] == bench.kernel_object_sha(patterns=(bench.kernel_symbol_fragment(entry["kernel"]),)), wl
    m = meshgen.twist_plate_k(12)
    ctx = be.Context(0)
    try:
        ctx.set_mesh(m["nodes"], m["elements"])
        ctx.set_element(Element_linear_tetrahedral())
        ctx.set_material(LinearIsotropic(*m["elastic"]))
        layout = bench.layout_signature(ctx.build_pattern())
    finally:
        ctx.close()
    assert doc["workloads"]["c3d4"]["layout"] == layout
    traffic, src = bench.pmc_traffic("c3d4", "k_pcg_persist", layout)
    assert traffic is not None and "spmv_traffic.json" in src
    # 1000 iterations per launch: the PMC bytes per iteration within 20 % of what the layout streams (111.8 MB + vectors)
    assert 1.0e8 < traffic / 1000 < 1.4e8
