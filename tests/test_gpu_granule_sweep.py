"""-m gpu: the tagged-granule sweep (csrc/granule.hpp) at the edges of its chunked load.  Wave 0 of every workgroup
loads four granule rows of 64 workgroups per lane together; a lane whose workgroup index is >= G loads a clamped
granule that a select then discards.  The workgroup counts below (FEMCY_TUNE_PERSIST_WGS, multiples of 8) are those
edges: 8 (most lanes hold no granule), 64 (exactly one row), 72 (a partial second row), 200 (a partial fourth row) and
the device's full count.

No case above 256 workgroups: the kernels keep one workgroup per CU (512 registers per lane, nearly all of the LDS), the
co-residency check refuses a larger grid before the launch, and the only over-sized launch of the suite is the
time-out of tests/test_gpu_pcg_persist.py::test_barrier_timeout_falls_back_to_the_three_kernel_loop -- so the loop over
chunks (G > 256) has no passing case on this device.

The mesh is small (87 slices of 64 nodes): at G = 8 its 32 waves hold three slices each, at the full count most waves
hold none -- the sweep is the same either way."""
import threading

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

WGS = [8, 64, 72, 200, 0]                                   # 0 = the device's full count (one workgroup per CU)


@pytest.fixture(scope="module")
def small_plate(gpu_ctx_factory):
    from femcy_amd import backend as be, meshgen
    from femcy_amd.element_zoo import Element_linear_tetrahedral
    from femcy_amd.material_zoo import LinearIsotropic
    m = meshgen.twist_plate(16, 4, 64)                      # 24 576 C3D4, 5 525 nodes = 87 slices, 16 575 DOF
    ctx = gpu_ctx_factory()
    ctx.set_mesh(m["nodes"], m["elements"])
    ctx.set_element(Element_linear_tetrahedral())
    ctx.set_material(LinearIsotropic(*m["elastic"]))
    info = ctx.build_pattern()
    assert 64 < info.nslices <= 96 and ctx.n > 12288        # three slices per wave at G = 8; not the small-system kernel
    ctx.assemble_K(-1)
    cons = np.unique(np.concatenate([np.asarray(b["node_set"]) * 3 + b["dof"] for b in m["dirichlet_bc_info"]]))
    ctx.upload(be.VEC_RESIDUAL, np.sin(np.arange(ctx.n) * 0.11) * 1e3)
    ctx.dirichlet_newton(cons, be.VEC_RESIDUAL)
    # the three-launch loop, once, for every case
    ctx.set_option(be.OPT_PCG_PERSIST, 0)
    t0 = ctx.timing()
    ref = ctx.pcg(be.VEC_RESIDUAL, be.VEC_X, eps=0.0, maxit=30)
    t1 = ctx.timing()
    assert t1["solves_three"] - t0["solves_three"] == 1
    ctx.set_option(be.OPT_PCG_PERSIST, 2)
    return dict(be=be, ctx=ctx, ref=ref, mesh=m)


@pytest.mark.parametrize("wgs", WGS)
def test_sweep_at_the_edges_of_the_chunked_load(small_plate, wgs):
    be, ctx, ref = small_plate["be"], small_plate["ctx"], small_plate["ref"]
    ctx.set_option(107, wgs)                                # FEMCY_TUNE_PERSIST_WGS
    ctx.set_option(be.TUNE_PERSIST_VARIANT, 6)              # tagged granules, d in storage order
    try:
        # the probe checks its own sums: every workgroup saw every other's value in every round
        us = ctx.probe_exchange(500, 1)
        print(f"[granule sweep] G = {wgs or 'all'}: {us:.2f} us per exchange")
        assert us > 0.0
        t0 = ctx.timing()
        got = ctx.pcg(be.VEC_RESIDUAL, be.VEC_X, eps=0.0, maxit=30)
        x1 = ctx.download(be.VEC_X)
        again = ctx.pcg(be.VEC_RESIDUAL, be.VEC_X, eps=0.0, maxit=30)
        x2 = ctx.download(be.VEC_X)
        t1 = ctx.timing()
        assert t1["solves_persist"] - t0["solves_persist"] == 2 and t1["solves_three"] == t0["solves_three"]
        assert t1["barrier_timeouts"] == t0["barrier_timeouts"]
        print(f"[granule sweep] G = {wgs or 'all'}: {got} against {ref}")
        assert got[0] == ref[0] == 30 and abs(got[2] - ref[2]) <= 1e-8 * ref[2]
        # fixed G: fixed order of combination, bit-reproducible iterates
        assert again == got and np.array_equal(x1, x2)
    finally:
        ctx.set_option(be.TUNE_PERSIST_VARIANT, -1)
        ctx.set_option(107, 0)


def test_sweep_across_two_ranks_on_a_reduced_grid(gpu_ctx_factory):
    """two contexts of one process on one GPU, 64 workgroups each (both kernels co-resident; the mesh and the grid of
    tests/test_gpu_multirank.py::test_persistent_pcg_across_ranks_on_one_gpu): the multi-rank kernel sweeps its own
    rank's granules with the same code before the mailbox stage.  (The 87-slice plate above cut in two does not stay on
    the one-launch path across ranks -- its first exchange times out and the solve falls back, with the sweep of this
    file and with the rolled one alike -- so it cannot serve here.)"""
    from femcy_amd import backend as be, meshgen, partition
    from femcy_amd.element_zoo import Element_linear_tetrahedral
    from femcy_amd.material_zoo import LinearIsotropic
    m = meshgen.twist_plate(24, 6, 96)                      # 82 944 C3D4, 16 975 nodes
    nodes, el = m["nodes"], m["elements"]
    mat = LinearIsotropic(*m["elastic"])
    cons_nodes = [(np.asarray(b["node_set"]), b["dof"]) for b in m["dirichlet_bc_info"]]
    b_g = np.sin(np.arange(nodes.size) * 0.11) * 1e3
    ctx = gpu_ctx_factory()                                 # the whole mesh on one context, three launches
    ctx.set_mesh(nodes, el)
    ctx.set_element(Element_linear_tetrahedral())
    ctx.set_material(mat)
    ctx.build_pattern()
    ctx.assemble_K(-1)
    ctx.upload(be.VEC_RESIDUAL, b_g)
    ctx.dirichlet_newton(np.unique(np.concatenate([ns * 3 + d for ns, d in cons_nodes])), be.VEC_RESIDUAL)
    ctx.set_option(be.OPT_PCG_PERSIST, 0)
    ref = ctx.pcg(be.VEC_RESIDUAL, be.VEC_X, eps=0.0, maxit=30)
    nranks = 2
    parts = partition.build_all_parts(nodes, el, nranks, axis=2)
    uid = be.Context.comm_local_id()
    blobs = [None] * nranks
    gate = threading.Barrier(nranks)
    out, err = [None] * nranks, []

    def rank_main(r):
        p = parts[r]
        c = be.Context(0)
        try:
            c.set_option(107, 64)                           # FEMCY_TUNE_PERSIST_WGS: a reduced grid per rank
            c.set_mesh(p.nodes, p.elements)
            c.set_element(Element_linear_tetrahedral())
            c.set_material(mat)
            c.build_pattern()
            c.comm_init(p.rank, p.nranks, uid, p.iface_local_dofs, p.iface_global_slot, p.niface_global, p.owner)
            c.comm_set_neighbours(p)
            blobs[r] = c.comm_mailbox_export()
            gate.wait(timeout=60)
            c.comm_mailbox_import(blobs)
            assert c.comm_persist_agree()
            c.assemble_K(-1)
            c.upload(be.VEC_RESIDUAL, p.scatter_global(b_g))
            cons = np.unique(np.concatenate([p.localize_nodes(ns) * 3 + d for ns, d in cons_nodes]))
            c.dirichlet_newton(cons, be.VEC_RESIDUAL)
            c.set_option(be.OPT_PCG_PERSIST_MULTI, 1)
            t0 = c.timing()
            res = c.pcg(be.VEC_RESIDUAL, be.VEC_X, eps=0.0, maxit=30)
            t1 = c.timing()
            out[r] = (res, t1["solves_persist"] - t0["solves_persist"], t1["solves_three"] - t0["solves_three"],
                      t1["barrier_timeouts"] - t0["barrier_timeouts"])
        except BaseException as e:                          # noqa: BLE001 - reported below
            err.append(e)
            gate.abort()
        finally:
            c.close()

    threads = [threading.Thread(target=rank_main, args=(r,), daemon=True) for r in range(nranks)]
    for t in threads:
        t.start()
    for t in threads:
        t.join(timeout=120)
    assert not any(t.is_alive() for t in threads), "a rank is still running"
    if err:
        raise err[0]
    for res, persist, three, timeouts in out:
        assert (persist, three, timeouts) == (1, 0, 0)
        assert res[0] == ref[0] and abs(res[2] - ref[2]) <= 1e-8 * ref[2]
    assert out[0][0] == out[1][0]                           # the replicas report the same scalars, bit for bit
