"""One context walked through several meshes: every device buffer of the context is (re)allocated, grown, kept with spare
capacity or dropped on the way (csrc/ctx.hpp: DevBuf, dev_alloc, dev_upload), and nothing of an earlier mesh may leak into
a later result.  Each visit -- a PCG solve, a product and a direct solve -- is compared BIT FOR BIT with the same mesh on a
fresh context with the same options: the kernels are deterministic and see the same arguments, so the only thing that can
differ is what the reused context kept (a stale bcolp, a captured graph of old addresses, a buffer that did not grow, a
fill that did not land)."""
import numpy as np
import pytest

from femcy_amd import backend as be
from femcy_amd import meshgen
from femcy_amd.element_zoo import Element_linear_quadrilateral, Element_linear_tetrahedral
from femcy_amd.material_zoo import LinearIsotropic, LinearIsotropicPlaneStress

pytestmark = pytest.mark.gpu
EINVAL = -1

THREE = {be.OPT_PCG_SMALL: 0, be.OPT_PCG_PERSIST: 0}      # the three-launch loop: ensure_pos_vectors, ensure_bcolp
SMALL = {be.OPT_PCG_SMALL: 1, be.OPT_PCG_PERSIST: 1}      # the defaults: the small-system form where it fits
PERSIST = {be.OPT_PCG_SMALL: 0, be.OPT_PCG_PERSIST: 1}    # the persistent form


def quad_mesh():
    """6 x 6 CPS4 on the unit square, the left edge held: 49 nodes, one slice"""
    k = 6
    x, y = np.meshgrid(np.linspace(0.0, 1.0, k + 1), np.linspace(0.0, 1.0, k + 1), indexing="ij")
    nodes = np.stack([x.ravel(), y.ravel()], axis=1)
    i, j = np.meshgrid(np.arange(k), np.arange(k), indexing="ij")
    a = (i * (k + 1) + j).ravel()
    el = np.stack([a, a + (k + 1), a + (k + 1) + 1, a + 1], axis=1).astype(np.int32)
    held = np.flatnonzero(nodes[:, 0] == 0.0)
    cons = np.sort(np.concatenate([held * 2, held * 2 + 1]))
    return dict(nodes=nodes, el=el, ELE=Element_linear_quadrilateral, mat=LinearIsotropicPlaneStress(2.0e5, 0.3), cons=cons)


def tet_mesh():
    """the twist plate of 8 x 2 x 12 cells in C3D4: 351 nodes (more than 64 x 4), six slices, dm = 3"""
    m = meshgen.twist_plate(8, 2, 12)
    cons = np.unique(np.concatenate([np.asarray(bc["node_set"]) * 3 + bc["dof"] for bc in m["dirichlet_bc_info"]]))
    return dict(nodes=m["nodes"], el=m["elements"], ELE=Element_linear_tetrahedral, mat=LinearIsotropic(*m["elastic"]), cons=cons)


MESHES = {"quad": quad_mesh(), "tet": tet_mesh()}


def set_up(ctx, m, opts):
    for k, v in opts.items():
        ctx.set_option(k, v)
    ctx.set_mesh(m["nodes"], m["el"])
    ctx.set_element(m["ELE"]())
    ctx.set_material(m["mat"])
    ctx.build_pattern()


def visit(ctx, name, opts):
    """mesh, pattern, K, a PCG solve, a product, a direct solve -> the bytes of the three results"""
    m = MESHES[name]
    set_up(ctx, m, opts)
    ctx.upload(be.VEC_DOF, np.zeros(ctx.n))
    ctx.assemble_K(be.VEC_DOF)
    ctx.upload(be.VEC_RESIDUAL, np.cos(0.37 * np.arange(ctx.n)) + 0.25)
    ctx.dirichlet_newton(m["cons"], be.VEC_RESIDUAL)
    it, _, _ = ctx.pcg(be.VEC_RESIDUAL, be.VEC_X, eps=1e-8)
    x = ctx.download(be.VEC_X)
    ctx.spmv(be.VEC_X, be.VEC_TMP1)
    y = ctx.download(be.VEC_TMP1)
    ctx.direct_solve(be.VEC_RESIDUAL, be.VEC_TMP0)
    xd = ctx.download(be.VEC_TMP0)
    assert it > 0 and np.isfinite(x).all() and np.abs(x).max() > 0 and np.isfinite(xd).all()
    return x.tobytes(), y.tobytes(), xd.tobytes()


_twins = {}


def twin(name, opts):
    """the same visit on a context of its own, made once per (mesh, options)"""
    key = (name, tuple(sorted(opts.items())))
    if key not in _twins:
        ctx = be.Context(0)
        try:
            _twins[key] = visit(ctx, name, opts)
        finally:
            ctx.close()
    return _twins[key]


def test_one_context_through_three_meshes():
    ctx = be.Context(0)
    try:
        # small, several times larger with dm 2 -> 3 (every buffer regrows), small again (spare capacity, a stale bcolp),
        # then the one-launch forms on both sizes: d_small / d_persist first sized by the larger mesh
        walk = [("quad", THREE), ("tet", THREE), ("quad", THREE), ("tet", SMALL), ("quad", SMALL), ("tet", PERSIST),
                ("quad", PERSIST), ("tet", THREE)]
        for step, (name, opts) in enumerate(walk):
            assert visit(ctx, name, opts) == twin(name, opts), f"step {step}: {name} {opts}"
    finally:
        ctx.close()
    after = be.Context(0)            # what close() released is handed out again
    try:
        assert visit(after, "quad", THREE) == twin("quad", THREE)
    finally:
        after.close()


def _refused(call, text):
    with pytest.raises(be.FemcyError) as err:
        call()
    assert err.value.status == EINVAL and text in str(err.value), str(err.value)


def test_ids_of_the_old_mesh_are_refused():
    ctx = be.Context(0)
    try:
        m = MESHES["quad"]
        set_up(ctx, m, THREE)
        ELE = m["ELE"]()
        ds = ctx.dofset(m["cons"])
        ls = ctx.loadset(ELE, [0], [0])
        bl = ctx.bodyload(ELE)
        th = ctx.thermal(ELE, 1.2e-5, np.linspace(0.0, 30.0, ctx.nn))
        ms = ctx.mass(ELE, 7.85e-9)
        lm = ctx.lumped_mass(ELE, 7.85e-9)
        ex = ctx.explicit(lm, (ds,))
        assert (ds, ls, bl, th, ms, lm, ex) == (0,) * 7
        ctx.dofset_fill(ds, be.VEC_TMP0, 1.0)              # they work on the mesh they were made on
        assert ctx.lumped_mass_get(lm).min() > 0

        assert visit(ctx, "tet", THREE) == twin("tet", THREE)
        _refused(lambda: ctx.dofset_fill(ds, be.VEC_TMP0, 1.0), "unknown dofset 0")
        _refused(lambda: ctx.loadset_neumann(ls, 1.0), "unknown load set 0")
        _refused(lambda: ctx.bodyload_weights(bl), "unknown body load 0")
        _refused(lambda: ctx.thermal_apply(th, 1.0), "unknown thermal load 0")
        _refused(lambda: ctx.mass_apply(ms, be.VEC_X, be.VEC_TMP0), "unknown mass object 0")
        _refused(lambda: ctx.lumped_mass_get(lm), "unknown lumped mass 0")
        _refused(lambda: ctx.explicit_kinetic_energy(ex), "unknown explicit integrator 0")
        assert visit(ctx, "tet", THREE) == twin("tet", THREE)      # the refusals left the context usable
        assert visit(ctx, "quad", THREE) == twin("quad", THREE)
    finally:
        ctx.close()
