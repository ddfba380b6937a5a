"""Block, gather and last-thread edges of the load, boundary and post-processing kernels (csrc/kernels_assembly.hip:
k_neumann_contrib / k_neumann_gather, k_dirichlet_zero, k_post, k_energy, k_energy_small, k_extrapolate, k_thermal_post,
k_dot_partial with the host sum of launch_energy_sum, k_body_weights / k_body_apply, k_thermal_force / k_thermal_apply;
csrc/kernels_pcg.hip: k_scatter / k_scatter_const / k_scatter_add), written against the C ABI (femcy_amd.backend.Context) so
that the host backend (tests/test_post_shapes_cpu.py, backend "cpu") and the device (tests/test_gpu_post_shapes.py, backend
"hip") run the same code.  Every function checks its own result and returns the figure it checked.  The case tables are
static; nothing is skipped at run time.

1. surface() -- the first 126 / 127 / 128 / 129 / 257 facets (workgroups of 128) of the top of a CPS4 strip one cell high (two-
   node edges: nload + 1 loaded nodes, so the gather sees 127 / 128 / 129 / 130 / 258) and of C3D4 / C3D8 / C3D10 plates one
   cell thick (3, 4 and 6 facet nodes), every node moved, the mid-side nodes of C3D10 off their chords; and a fan of 64
   triangles whose 128 spoke facets load the hub, the last loaded node, through 128 contribution slots (along the normal the
   two sides of a spoke cancel, so that run loads one spoke per triangle: 64 slots).  Along the normal and along a fixed
   direction, into a vector of NaN; then as _add on a random vector, bit-equal to base + surface.
2. dirichlet() -- T = k max_row_blocks threads of k_dirichlet_zero on either side of 256 (fans of seven CPS3 triangles, rows
   of 8 and 4 blocks, loose nodes of 1) and of 512 (a C3D8 column, rows of 12 and 8), the last constrained DOF in a longest
   row; K against orc._zero_rows_cols_unit_diag bit for bit, the right-hand side against rhs - K s in long double row by
   row; the Newton and dofset variants.  scatters() -- 255 / 256 / 257 indices in random order, DOF n - 1 last.
3. post() -- ne = floor(256 / g) and + 1 for g = nGP and npe of eight families (and 255 / 256 / 257 for CPS4 and C3D8): F,
   strain, stress, von Mises, small and large, both energy densities, extrapolation, the thermal correction; every
   Gauss-point field is written twice from two displacement fields and the second one is checked.  Materials: plane stress,
   plane strain and the plane-strain neo-Hookean solid in 2-D, linear and neo-Hookean in 3-D; the neo-Hookean kinds take the
   large path only.  The weights det J w of the undeformed mesh after an assembly and after the small-strain energy.  energy
   totals on the same meshes (smooth / the last element only) and, for the energy of the infinitesimal strain,
   which needs no earlier geometry pass, on 1024 x 256 + 1 triangles.
4. bodyload() / thermal() -- the element passes of the loads at 255 / 256 / 257 elements: all elements, the last one only,
   all but the last; a temperature change in the last element only.

Bounds.  The float64 restatement (tests/post_reference.py) against the long-double one on these very cases
(measure_f64_worst, asserted by the CPU twin) gives the constants F64_WORST; a backend is held to 4 x that, since a different
but legitimate order of the same operations differs by as much.  Errors are relative to the largest entry of the reference
field.  Sums: N products summed in any order carry at most (N + 4) eps times the sum of their magnitudes (dyn_shapes.energy).
The Dirichlet right-hand side: one row of rhs - K s has at most W = max_row_blocks dm products, (W + 2) eps (|rhs| + |K| |s|)
(explicit_cases.omega_bound's shape).  The resultant of m loaded nodes errs by at most m times the bound of one entry."""
import functools

import numpy as np

from femcy_amd import backend as be
from femcy_amd.material_zoo import NeoHookean, NeoHookeanPlaneStrain
from oracle import femcy_oracle as orc

import asm_shapes as ash
import dyn_shapes as ds
import loads_cases as lc
import loads_reference as lr
import post_reference as pr
import thermal_cases as tc
import thermal_reference as tr
from dyn_shapes import BLOCK_PLATES, _first

LD = np.longdouble
EPS = 2.0 ** -53
# worst error of the float64 restatement against the long-double one on the cases of this file (measure_f64_worst, as measured)
# (the strains are F - I with entries of 1e-2: two digits go in the difference, and twice that in the energy of the Green strain)
F64_WORST = {"surface": 2.4e-14, "F": 2.8e-16, "strain": 2.1e-14, "stress": 2.3e-14, "mises": 2.0e-14, "green": 2.3e-14,
             "stress_large": 3.5e-14, "mises_large": 2.5e-14, "energy": 9.7e-13, "energy_small": 3.1e-14, "extrapolate": 6.7e-14, "vol": 7.1e-15}


def _rel(got, want):
    return float(np.abs(np.asarray(got, dtype=LD) - want).max() / np.abs(want).max())


def _bits(a, b):
    return np.array_equal(np.ascontiguousarray(a).view(np.uint64), np.ascontiguousarray(b).view(np.uint64))


# ------------------------------------------------------------------------------------------------- 1. surface loads
SURFACE_NLOAD = (126, 127, 128, 129, 257)
SURFACE_PLATES = {"CPS4": ((260, 1), 2), "C3D4": ((12, 11, 1), 3), "C3D8": ((17, 16, 1), 4), "C3D10": ((12, 11, 1), 6)}   # cells, nfn
SURFACE_PERTURB = 0.2
SURFACE_FAN = "fan-64"
SURFACE_CASES = [(family, nload) for family in SURFACE_PLATES for nload in SURFACE_NLOAD] + [("fan", 128)]
SURFACE_WG = 128
TRACTION = -2.5
DIRECTION = np.array([0.6, -0.3, 0.74])
ORACLE_SURFACES = ("CPS4", "C3D4", "C3D10")                           # the families the oracle has


@functools.lru_cache(maxsize=None)
def _surface_plate(family):
    cells, nfn = SURFACE_PLATES[family]
    flat, el, ELE = lr.mesh(family, cells=cells, perturb=0.0)
    top = flat[:, -1] > flat[:, -1].max() - 1e-12
    keys = ELE.facet_tables(nfn)["ft_nodes"]
    le, lf = [], []
    for k, key in enumerate(keys):
        e = np.nonzero(top[el[:, key]].all(axis=1))[0]
        le.append(e)
        lf.append(np.full(len(e), k))
    le, lf = np.concatenate(le), np.concatenate(lf)
    order = np.lexsort((lf, le))                                       # by element, then by facet type
    h = (np.ptp(flat, axis=0) / np.asarray(cells)).min()
    rng = np.random.default_rng(23)
    if family == "C3D10":                                              # moved corners, then mid-sides off their chords
        from femcy_amd import meshgen
        nc = int(el[:, :4].max()) + 1
        corners = flat[:nc] + SURFACE_PERTURB * h * rng.uniform(-1.0, 1.0, (nc, 3))
        nodes, el2 = meshgen.to_quadratic(corners, el[:, :4])
        assert np.array_equal(el2, el)
        nodes = nodes.copy()
        nodes[nc:] += 0.05 * h * rng.uniform(-1.0, 1.0, nodes[nc:].shape)
    else:
        nodes = flat + SURFACE_PERTURB * h * rng.uniform(-1.0, 1.0, flat.shape)
    nodes = np.ascontiguousarray(nodes, dtype=np.float64)
    nodes.setflags(write=False)
    return nodes, np.ascontiguousarray(el, dtype=np.int32), ELE, le[order].astype(np.int32), lf[order].astype(np.int32)


def surface_case(family, nload, along_normal=False):
    """-> nodes, el, ELE, load_elem, load_ft, nfn.  The fan: both spokes of every triangle, 2 k slots of the hub; the normals of
    the two sides of a spoke cancel, so the run along the normal loads the first spoke of every triangle only (k slots)"""
    if family == "fan":
        nodes, el, ELE = ds.shape_mesh(SURFACE_FAN)
        hub = len(nodes) - 1
        keys = ELE.facet_tables(2)["ft_nodes"]
        le, lf = [], []
        for e in np.nonzero((el == hub).any(axis=1))[0]:
            local = int(np.nonzero(el[e] == hub)[0][0])
            for k, key in enumerate(keys):
                if local in key and not (along_normal and le and le[-1] == e):
                    le.append(e)
                    lf.append(k)
        return nodes, el, ELE, np.array(le, np.int32), np.array(lf, np.int32), 2
    nodes, el, ELE, le, lf = _surface_plate(family)
    return nodes, el, ELE, le[:nload], lf[:nload], SURFACE_PLATES[family][1]


def surface_table(family, nload, along_normal=False):
    """the table's own arithmetic -> the loaded nodes"""
    nodes, el, ELE, le, lf, nfn = surface_case(family, nload, along_normal)
    if family == "fan" and along_normal:
        nload //= 2
    keys = ELE.facet_tables(nfn)["ft_nodes"]
    slots = el[le[:, None], keys[lf]]
    loaded = np.unique(slots)
    assert len(le) == nload and keys.shape[1] == nfn
    if family == "fan":
        hub = len(nodes) - 1
        assert nload in (SURFACE_WG, SURFACE_WG // 2) and loaded[-1] == hub and (slots == hub).sum() == nload and len(loaded) == SURFACE_WG // 2 + 1
    else:
        assert len(_surface_plate(family)[3]) >= max(SURFACE_NLOAD)
        assert len(set(zip(le.tolist(), lf.tolist()))) == nload
        if family == "CPS4":
            assert len(loaded) == nload + 1                            # 127 / 128 / 129 nodes for the gather
    return loaded


@functools.lru_cache(maxsize=None)
def reference_surface(family, nload, along_normal):
    """-> {dtype: (rhs, resultant)}"""
    nodes, el, ELE, le, lf, nfn = surface_case(family, nload, along_normal)
    d = None if along_normal else DIRECTION[:nodes.shape[1]]
    out = {dt: pr.neumann(nodes, el, ELE, le, lf, nfn, TRACTION, d, dt) for dt in (LD, np.float64)}
    out[LD][0].setflags(write=False)
    return out


def surface_reference_conditions(family, nload):
    """CPU reference alone: the sum over the nodes is the resultant, along a direction it is traction x area x direction, the
    last facet and the last loaded node carry a load; where the oracle has the family, orc.neumann_rhs agrees"""
    for along_normal in (True, False):
        nodes, el, ELE, le, lf, nfn = surface_case(family, nload, along_normal)
        dm = nodes.shape[1]
        loaded = surface_table(family, nload, along_normal)
        keys = ELE.facet_tables(nfn)["ft_nodes"]
        ref, res = reference_surface(family, nload, along_normal)[LD]
        r = ref.reshape(-1, dm)
        assert np.abs(r.sum(axis=0) - res).max() <= 8 * EPS * np.abs(r).sum()   # the float64 tables: sum_a N_a = 1 to their rounding
        assert np.abs(r[loaded[-1]]).max() > 0 and np.abs(r[el[le[-1], keys[lf[-1]]]]).max() > 0
        assert not np.delete(r, loaded, axis=0).any()
        if not along_normal:
            area = res[0] / (TRACTION * DIRECTION[0])
            assert area > 0 and np.abs(res - TRACTION * area * DIRECTION[:dm].astype(LD)).max() <= 1e-15 * np.abs(res).max()   # a few thousand long-double roundings
        if family in ORACLE_SURFACES:
            from oracle.elements import elem_def
            topo = orc.Topology(nodes, el, elem_def(family))
            facets = [tuple(sorted(el[e, keys[t]].tolist())) for e, t in zip(le, lf)]
            want = orc.neumann_rhs(topo, facets, TRACTION, None if along_normal else DIRECTION[:dm])
            assert _rel(want, ref) <= 1e-13, (family, nload, along_normal)


def surface(family, nload, backend):
    nodes, el, ELE = surface_case(family, nload)[:3]
    dm = nodes.shape[1]
    ctx = lc.make_ctx(nodes, el, ELE, backend)
    base = np.random.default_rng(nload).standard_normal(nodes.size)
    worst = 0.0
    for along_normal in (True, False):
        d = None if along_normal else DIRECTION[:dm]
        le, lf, nfn = surface_case(family, nload, along_normal)[3:]
        loaded = surface_table(family, nload, along_normal)
        ls = ctx.loadset(ELE, le, lf, nfn)
        ref, res = reference_surface(family, nload, along_normal)[LD]
        ctx.vector(be.VEC_RHS).fill(np.nan)
        ctx.loadset_neumann(ls, TRACTION, d, be.VEC_RHS)
        got = ctx.download(be.VEC_RHS)
        assert np.isfinite(got).all() and not np.delete(got.reshape(-1, dm), loaded, axis=0).any()    # exact zeros off the surface
        err = _rel(got, ref)
        eres = float(np.abs(got.astype(LD).reshape(-1, dm).sum(axis=0) - res).max() / np.abs(res).max())
        print(f"surface {family} nload {nload} {'normal' if along_normal else 'direction'} [{backend}]: {err:.3e}, resultant {eres:.3e}")
        assert err <= 4.0 * F64_WORST["surface"], err
        assert eres <= len(loaded) * 4.0 * F64_WORST["surface"] * float(np.abs(ref).max() / np.abs(res).max()), eres
        ctx.upload(be.VEC_RHS, base)
        ctx.loadset_neumann(ls, TRACTION, d, be.VEC_RHS, add=True)
        assert _bits(ctx.download(be.VEC_RHS), base + got)            # one rounded addition per entry; the rest untouched
        worst = max(worst, err)
    ctx.close()
    return worst


# -------------------------------------------------------------------------------------------- 2. boundary conditions
# name -> (mesh, k, T = k max_row_blocks)
DIRICHLET_MESHES = {"fans": 8, "column": 12}                          # max_row_blocks
DIRICHLET_CASES = {"fans-k31": ("fans", 31, 248), "fans-k32": ("fans", 32, 256), "fans-k33": ("fans", 33, 264),
                   "column-k42": ("column", 42, 504), "column-k43": ("column", 43, 516)}
DIRICHLET_SIGMA = 64
DIRICHLET_VALUE = -0.375
COLUMN_CELLS = (1, 1, 20)


@functools.lru_cache(maxsize=None)
def dirichlet_mesh(which):
    """-> nodes, el, ELE, the node of the last constrained DOFs (a longest row), two neighbouring nodes"""
    if which == "fans":                                                # three fans, 44 loose nodes, the fourth fan: 76 nodes
        n3, e3 = ash.fans2d([7, 7, 7])
        n1, e1, ELE = lr.fan(7)
        loose = n3.max(axis=0) + 2.0 + 0.01 * np.arange(44)[:, None] * np.ones(2)
        nodes = np.vstack([n3, loose, n1 + np.array([12.0, 0.0])])
        el = np.vstack([e3, e1 + len(n3) + len(loose)]).astype(np.int32)
        return np.ascontiguousarray(nodes), el, ELE, len(n3) + len(loose), (1, 2)
    nodes, el, ELE = lr.mesh("C3D8", cells=COLUMN_CELLS, perturb=0.0)
    return np.ascontiguousarray(nodes, dtype=np.float64), np.ascontiguousarray(el, np.int32), ELE, len(nodes) - 5, (8, 12)


def dirichlet_dofs(name):
    """-> the constrained DOFs in their order, and what the table promises of them"""
    which, k, T = DIRICHLET_CASES[name]
    nodes, el, ELE, last, (nb0, nb1) = dirichlet_mesh(which)
    dm = nodes.shape[1]
    lay = ash.Layout(nodes, el, DIRICHLET_SIGMA)
    stored = np.nonzero(lay.node_of >= 0)[0]
    lane0, lane63, tail = int(lay.node_of[0]), int(lay.node_of[63]), int(lay.node_of[stored[-1]])
    short = int(np.argmin(lay.rowlen))
    assert lay.max_row == DIRICHLET_MESHES[which] and lay.rowlen[last] == lay.max_row and k * lay.max_row == T
    assert lay.nslices == 2 and stored[-1] % 64 < 63 and lay.pos[tail] // 64 == 1 and lay.pos[last] // 64 == 1
    assert lay.rowlen[short] < lay.max_row and nb1 in el[(el == nb0).any(axis=1)]
    must = [lane0 * dm + i for i in range(dm)] + [a * dm + i for a in (nb0, nb1) for i in range(dm)]
    must += [lane63 * dm, tail * dm + dm - 1, short * dm]
    must = list(dict.fromkeys(must))
    end = [last * dm + i for i in range(dm)]
    assert not set(must) & set(end)
    pool = [d for d in np.random.default_rng(k).permutation(nodes.size).tolist() if d not in must and d not in end]
    dofs = np.array(must + pool[:k - len(must) - dm] + end, dtype=np.int32)
    assert len(dofs) == k == len(set(dofs.tolist())) and dofs[-1] // dm == last
    return dofs


def _dirichlet_ctx(which, backend):
    nodes, el, ELE = dirichlet_mesh(which)[:3]
    ctx = be.Context(0, backend=backend)
    ctx.set_option(be.OPT_NODE_ORDER, 0)                             # the caller's numbering: what the layout restates
    ctx.set_option(be.OPT_SELL_SIGMA, DIRICHLET_SIGMA)
    ctx.set_mesh(nodes, el)
    ctx.set_element(ELE)
    ctx.set_material(tc.material(tr.LIN3D if ELE.dm == 3 else tr.PSTRESS))
    info = ctx.build_pattern()
    assert info.max_row_blocks == DIRICHLET_MESHES[which]
    if backend == "hip":
        assert info.nslices == 2
    return ctx, info


def dirichlet(name, backend):
    which, k, T = DIRICHLET_CASES[name]
    dofs = dirichlet_dofs(name)
    ctx, info = _dirichlet_ctx(which, backend)
    n, W = ctx.n, info.max_row_blocks * ctx.dm
    rng = np.random.default_rng(T)
    rhs, resid = rng.standard_normal(n), rng.standard_normal(n)
    vals = rng.uniform(0.5, 1.5, k) * rng.choice([-1.0, 1.0], k)
    free = np.ones(n, dtype=bool)
    free[dofs] = False

    def fresh():
        ctx.assemble_K(-1)
        return ctx.get_K_bsr().tocsr()

    K0 = fresh()
    Kref = orc._zero_rows_cols_unit_diag(K0, dofs)
    assert np.abs(K0[dofs].toarray()).max() > 0

    def check_K(K):
        K = K.tocsr()
        A = K.toarray()
        off = A.copy()
        off[dofs, dofs] = 0.0
        assert not off[dofs].any() and not off[:, dofs].any() and (A[dofs, dofs] == 1.0).all()
        # the stored entries, explicit zeros included: +0.0 and 1.0 where the reference puts them, every other one keeps its bits
        assert np.array_equal(K.indptr, Kref.indptr) and np.array_equal(K.indices, Kref.indices) and _bits(K.data, Kref.data)

    # the linear variant, prescribed values that differ
    ctx.upload(be.VEC_RHS, rhs)
    ctx.dirichlet_linear(dofs, vals, be.VEC_RHS)
    got = ctx.download(be.VEC_RHS)
    check_K(ctx.get_K_bsr())
    s = np.zeros(n, dtype=LD)
    s[dofs] = vals
    A0 = K0.toarray().astype(LD)
    want = rhs - A0 @ s
    bound = (W + 2) * EPS * (np.abs(rhs) + np.abs(A0) @ np.abs(s))
    assert np.array_equal(got[dofs], vals) and np.abs(A0 @ s)[free].max() > 0
    ratio = float((np.abs(got - want)[free] / bound[free]).max())
    print(f"dirichlet {name} [{backend}]: T = {T}, rhs - K s at {ratio:.3f} of its bound")
    assert ratio <= 1.0, ratio
    # the Newton variant
    assert _bits(fresh().data, K0.data)
    ctx.upload(be.VEC_RESIDUAL, resid)
    ctx.dirichlet_newton(dofs, be.VEC_RESIDUAL)
    r1, K1 = ctx.download(be.VEC_RESIDUAL), ctx.get_K_bsr().tocsr()
    check_K(K1)
    assert not r1[dofs].any() and _bits(r1[free], resid[free])
    # the dofset variants give the bits of the list variants
    dset = ctx.dofset(dofs)
    fresh()
    ctx.upload(be.VEC_RESIDUAL, resid)
    ctx.dofset_dirichlet_newton(dset, be.VEC_RESIDUAL)
    assert _bits(ctx.download(be.VEC_RESIDUAL), r1) and _bits(ctx.get_K_bsr().tocsr().data, K1.data)
    out = []
    for call in (lambda: ctx.dirichlet_linear(dofs, np.full(k, DIRICHLET_VALUE), be.VEC_RHS),
                 lambda: ctx.dofset_dirichlet_linear(dset, DIRICHLET_VALUE, be.VEC_RHS)):
        fresh()
        ctx.upload(be.VEC_RHS, rhs)
        call()
        out.append((ctx.download(be.VEC_RHS), ctx.get_K_bsr().tocsr().data))
    assert _bits(out[0][0], out[1][0]) and _bits(out[0][1], out[1][1]) and (out[0][0][dofs] == DIRICHLET_VALUE).all()
    check_K(ctx.get_K_bsr())
    ctx.close()
    return ratio


SCATTER_K = (255, 256, 257)
SCATTER_N = 513


def scatters(k, backend):
    """femcy_vec_scatter, femcy_dofset_scatter / _fill / _add: exact, DOF n - 1 by the last thread"""
    ctx = ds.vector_ctx(SCATTER_N, backend)
    n = ctx.n
    rng = np.random.default_rng(k)
    idx = np.concatenate([rng.permutation(n - 1)[:k - 1], [n - 1]]).astype(np.int32)
    base, vals = rng.standard_normal(n), rng.standard_normal(k)
    assert len(idx) == k == len(np.unique(idx)) and idx[-1] == n - 1 and n > k
    dset = ctx.dofset(idx)
    put = base.copy()
    put[idx] = vals
    for call, want in ((lambda: ctx.scatter(be.VEC_TMP0, idx, vals), put),
                       (lambda: ctx.dofset_scatter(dset, be.VEC_TMP0, vals), put),
                       (lambda: ctx.dofset_fill(dset, be.VEC_TMP0, 3.5), np.where(np.isin(np.arange(n), idx), 3.5, base)),
                       (lambda: ctx.dofset_add(dset, be.VEC_TMP0, -3.25), np.where(np.isin(np.arange(n), idx), base + -3.25, base))):
        ctx.upload(be.VEC_TMP0, base)
        call()
        assert _bits(ctx.download(be.VEC_TMP0), want), k
    ctx.close()
    return k


# ------------------------------------------------------------------------------------------------ 3. post-processing
# family -> (nGP, npe): the thread counts are ne nGP (k_post, k_energy, k_energy_small, k_thermal_post) and ne npe (k_extrapolate)
POST_SHAPE = {"CPS3": (1, 3), "CPS4": (4, 4), "CPS8": (4, 8), "CPS6": (3, 6), "C3D4": (1, 4), "C3D8": (8, 8), "C3D6": (6, 6),
              "C3D10": (4, 10)}
POST_PLATES = dict(BLOCK_PLATES, CPS6=(16, 9))
POST_GEOM_EDGE = ("CPS4", "C3D8")                                     # k_geom's own edge: 255 / 256 / 257 elements
XBS = 256
POST_NE = {family: tuple(sorted({XBS // g + i for g in POST_SHAPE[family] for i in (0, 1)}
                                | ({255, 256, 257} if family in POST_GEOM_EDGE else set()))) for family in POST_SHAPE}
POST_KINDS = {2: (pr.PSTRESS, pr.PSTRAIN, pr.NEOHOOKE), 3: (pr.LIN3D, pr.NEOHOOKE)}    # 2-D neo-Hookean: plane strain
POST_CASES = [(family, ne, kind) for family in POST_SHAPE for ne in POST_NE[family]
              for kind in POST_KINDS[2 if family.startswith("CP") else 3]]
TKIND = {pr.LIN3D: tr.LIN3D, pr.PSTRAIN: tr.PSTRAIN, pr.PSTRESS: tr.PSTRESS}
ENERGY_VARIANTS = ("smooth", "last")                                 # as dyn_shapes.ENERGY_VARIANTS: everywhere / the last element
POST_SCALE = 0.01
ENERGY_BIG = ("CPS3", (363, 362), 1024 * 256 + 1)


def post_material(kind, dm):
    if kind == pr.NEOHOOKE:
        return NeoHookean(C1=80.0, D1=400.0) if dm == 3 else NeoHookeanPlaneStrain(C1=80.0, D1=400.0)
    return tc.material(TKIND[kind])


@functools.lru_cache(maxsize=None)
def post_mesh(family, ne):
    nodes, el, ELE = lr.mesh(family, cells=POST_PLATES[family], perturb=ds.BLOCK_PERTURB)
    nodes, el = _first(nodes, el, ne)
    nodes = np.ascontiguousarray(nodes, dtype=np.float64)
    nodes.setflags(write=False)
    assert len(el) == ne and len(np.unique(el)) == len(nodes)
    return nodes, el, ELE


def post_disp(nodes, el, which):
    """"first": what a field holds before the checked call; "smooth"; "last": non-zero in the last element's nodes only"""
    u = ash.disp(nodes, POST_SCALE)
    if which == "first":
        return -0.4 * u
    if which == "last":
        keep = np.zeros(nodes.shape, dtype=bool)
        keep[el[-1]] = True
        return np.where(keep.ravel(), u, 0.0)
    return u


@functools.lru_cache(maxsize=None)
def reference_post(family, ne, kind):
    """-> {dtype: {field: array}} from nodes and displacements"""
    nodes, el, ELE = post_mesh(family, ne)
    mat = post_material(kind, ELE.dm)
    E = ELE.extrap_matrix()
    out = {}
    for dt in (LD, np.float64):
        r = {}
        F, r["vol"] = pr.gauss_F(nodes, el, ELE, post_disp(nodes, el, "smooth"), dt)
        r["F"] = F
        if kind != pr.NEOHOOKE:
            r["strain"], r["stress"], r["mises"] = pr.small(F, kind, mat.params, mat.C, dt)
            r["energy_small"] = pr.energy_small(F, kind, mat.params, mat.C, dt)
            r["extrapolate"] = r["mises"] @ E.T.astype(dt)
        r["green"], r["stress_large"], r["mises_large"] = pr.large_stress(F, kind, mat.params, mat.C, dt)
        r["energy"] = pr.energy(F, kind, mat.params, mat.C, dt)
        if kind == pr.NEOHOOKE:
            r["extrapolate"] = r["mises_large"] @ E.T.astype(dt)
        FL, _ = pr.gauss_F(nodes, el, ELE, post_disp(nodes, el, "last"), dt)
        r["energy_last"] = pr.energy(FL, kind, mat.params, mat.C, dt)
        if kind != pr.NEOHOOKE:
            r["energy_small_last"] = pr.energy_small(FL, kind, mat.params, mat.C, dt)
        out[dt] = r
    for x in out[LD].values():
        x.setflags(write=False)
    return out


def post_table(family):
    """the table's own arithmetic: each thread count is the last at or below 256 or the first above it"""
    nodes, el, ELE = post_mesh(family, POST_NE[family][0])
    nGP, npe = POST_SHAPE[family]
    assert (len(ELE.gaussWeights), el.shape[1]) == (nGP, npe) and ELE.extrap_matrix().shape == (npe, nGP)
    for g in (nGP, npe):
        lo = XBS // g
        assert lo in POST_NE[family] and lo + 1 in POST_NE[family] and lo * g <= XBS < (lo + 1) * g
        assert (lo * g == XBS) == (XBS % g == 0)
    return POST_NE[family]


def post_reference_conditions(family, ne, kind):
    """CPU reference alone: the oracle's constitutive functions agree with the restatement; the last Gauss point, the last
    element and the last node slot carry a signal"""
    nodes, el, ELE = post_mesh(family, ne)
    mat = post_material(kind, ELE.dm)
    r = reference_post(family, ne, kind)[LD]
    om = orc.Material({pr.LIN3D: "lin3d", pr.PSTRAIN: "pstrain", pr.PSTRESS: "pstress", pr.NEOHOOKE: "neohooke"}[kind],
                      tuple(float(v) for v in mat.params))
    F = np.asarray(r["F"], dtype=np.float64)
    dm = ELE.dm
    if kind == pr.NEOHOOKE and dm == 2:                                # the 3-D solid at F33 = 1, as tests/test_gpu_neohooke2d.py
        F3 = np.zeros(F.shape[:-2] + (3, 3))
        F3[..., :2, :2], F3[..., 2, 2] = F, 1.0
        F = F3
    s3 = orc.cauchy_large(om, F)
    assert _rel(s3[..., :dm, :dm], r["stress_large"]) <= 1e-12 and _rel(orc.energy_density(om, F), r["energy"]) <= 1e-11
    if kind == pr.NEOHOOKE:                                            # von Mises of the full 3-D stress
        dev = s3 - np.eye(3) * (np.trace(s3, axis1=-2, axis2=-1) / 3.0)[..., None, None]
        assert _rel(np.sqrt(1.5 * (dev * dev).sum(axis=(-1, -2))), r["mises_large"]) <= 1e-12
    if kind != pr.NEOHOOKE:
        assert _rel(orc.cauchy_small(om, F), r["stress"]) <= 1e-12
        assert np.abs(r["stress"][-1, -1]).max() > 0 and r["mises"][-1, -1] > 0 and r["energy_small"][-1, -1] > 0
    assert r["mises_large"][-1, -1] > 0 and r["energy"][-1, -1] > 0 and r["extrapolate"][-1, -1] != 0 and (r["vol"] > 0).all()
    last = r["energy_last"]
    assert (last[-1] > 0).all() and last[-1].sum() >= 1e3 * (last.size + 4) * EPS * last.sum() and np.abs(r["F"][-1, -1] - np.eye(ELE.dm)).max() > 0


def _fields(ctx, *which):
    return [ctx.gauss_field(w).to_numpy() for w in which]


def _check(figures, key, got, want, what):
    err = _rel(got, want)
    figures[key] = max(figures.get(key, 0.0), err)
    assert err <= 4.0 * F64_WORST[key], (what, key, err)


def post(family, ne, kind, backend):
    """every Gauss-point field is written from post_disp "first" and then from "smooth": the second call is checked"""
    nodes, el, ELE = post_mesh(family, ne)
    mat = post_material(kind, ELE.dm)
    dm = ELE.dm
    what = (family, ne, kind, backend)
    r = reference_post(family, ne, kind)[LD]
    ctx = tc.make_ctx(nodes, el, ELE, mat, backend)
    E = ELE.extrap_matrix()
    fig = {}
    fields = ("first", "smooth")
    if kind != pr.NEOHOOKE:
        for which in fields:
            ctx.upload(be.VEC_DOF, post_disp(nodes, el, which))
            ctx.compute_strain_stress(be.VEC_DOF, large=False)
            nod = ctx.extrapolate(be.GP_MISES, E)
            nod11 = ctx.extrapolate(be.GP_SIGMA, E, dm + 1)
        F, strain, sigma0, mises = _fields(ctx, be.GP_F, be.GP_STRAIN, be.GP_SIGMA, be.GP_MISES)
        for key, got in (("F", F), ("strain", strain), ("stress", sigma0), ("mises", mises), ("extrapolate", nod)):
            _check(fig, key, got, r[key], what)
        e11 = float(np.abs(nod11 - r["stress"][..., 1, 1] @ E.T.astype(LD)).max() / np.abs(r["stress"]).max())
        assert e11 <= 4.0 * max(F64_WORST["extrapolate"], F64_WORST["stress"]), (what, e11)
        # the thermal correction of this stress (k_thermal_post), thermal_cases' own bound
        dT = tr.smooth_dT(nodes)
        th = ctx.thermal(ELE, tc.ALPHA, dT)
        ctx.thermal_stress(th, tc.SCALE)
        sig, mis = _fields(ctx, be.GP_SIGMA, be.GP_MISES)
        ref_s, ref_m = tr.corrected_stress(el, ELE, mat.C, TKIND[kind], tc.NU, tc.ALPHA, dT, tc.SCALE, sigma0, LD)
        size = max(np.abs(sigma0).max(), float(np.abs(ref_s - sigma0.astype(LD)).max()))
        fig["thermal"] = max(float(np.abs(sig - ref_s).max() / size), float(np.abs(mis - ref_m).max() / size))
        assert fig["thermal"] <= tc.STRESS_TOL and np.abs(ref_s - sigma0)[-1, -1].max() > 0, (what, fig["thermal"])
    for which in fields:
        ctx.upload(be.VEC_DOF, post_disp(nodes, el, which))
        ctx.internal_force(be.VEC_DOF, be.VEC_FORCE)                  # leaves the large-deformation Cauchy stress
        ctx.compute_strain_stress(be.VEC_DOF, large=True)
        nod = ctx.extrapolate(be.GP_MISES, E)
    F, green, sigma, mises = _fields(ctx, be.GP_F, be.GP_STRAIN, be.GP_SIGMA, be.GP_MISES)
    for key, got in (("F", F), ("green", green), ("stress_large", sigma), ("mises_large", mises)):
        _check(fig, key, got, r[key], what)
    if kind == pr.NEOHOOKE:
        _check(fig, "extrapolate", nod, r["extrapolate"], what)
    ctx.assemble_K(-1)                                                # det J w of the undeformed mesh (k_geom's own tail)
    _check(fig, "vol", ctx.gauss_field(be.GP_VOL).to_numpy(), r["vol"], what)
    # energy densities and totals: the densities against the restatement, the totals against the long-double sum of the
    # backend's own densities and weights
    ngp = ne * len(ELE.gaussWeights)
    for variant in ENERGY_VARIANTS:
        for small in ((False, True) if kind != pr.NEOHOOKE else (False,)):
            ctx.upload(be.VEC_DOF, post_disp(nodes, el, "first"))
            ctx.elastic_energy(be.VEC_DOF, small=small)
            ctx.upload(be.VEC_DOF, post_disp(nodes, el, variant))
            tot = ctx.elastic_energy(be.VEC_DOF, small=small)
            assert tot == ctx.elastic_energy(be.VEC_DOF, small=small)
            dens, vol = _fields(ctx, be.GP_ENERGY, be.GP_VOL)
            if variant == "smooth":
                _check(fig, "energy_small" if small else "energy", dens, r["energy_small" if small else "energy"], what)
            else:
                _check(fig, "energy_small" if small else "energy", dens, r["energy_small_last" if small else "energy_last"], what)
            if small:                                                 # this call takes the weights of the undeformed mesh itself
                _check(fig, "vol", vol, r["vol"], what)
            terms = dens.astype(LD) * vol.astype(LD)
            esum = float(abs(LD(tot) - terms.sum()) / np.abs(terms).sum())
            fig["total"] = max(fig.get("total", 0.0), esum)
            assert terms[-1, -1] != 0 and esum <= (ngp + 4) * EPS, (what, variant, small, esum)
    ctx.close()
    print(f"post {family} ne {ne} kind {kind} [{backend}]: " + ", ".join(f"{k} {v:.2e}" for k, v in fig.items()))
    return fig


@functools.lru_cache(maxsize=None)
def big_case(variant):
    """-> nodes, el, ELE, u, {dtype: (energy density of the infinitesimal strain, det J w)}: vectorised numpy"""
    family, cells, ne = ENERGY_BIG
    nodes, el, ELE = lr.mesh(family, cells=cells, perturb=0.0)
    nodes, el = _first(nodes, el, ne)
    assert len(el) == ne == 1024 * XBS + 1 and len(ELE.gaussWeights) == 1
    x = nodes / np.ptp(nodes, axis=0).max()
    u = 0.01 * np.column_stack([np.sin(1.3 * x[:, 0] + 0.4) * np.cos(0.7 * x[:, 1]), 0.5 * np.cos(2.1 * x[:, 1] - 0.2) * x[:, 0]])
    if variant == "last":
        keep = np.zeros(len(nodes), dtype=bool)
        keep[el[-1]] = True
        u[~keep] = 0.0
    mat = tc.material(tr.PSTRESS)
    ref = {}
    for dt in (LD, np.float64):
        F, vol = pr.gauss_F(nodes, el, ELE, u.ravel(), dt)
        ref[dt] = (pr.energy_small(F, pr.PSTRESS, mat.params, mat.C, dt), vol)
    # bounds by reasoning, since a float64 restatement on grid coordinates that are nearly exact says little about another order
    # of the same sums.  An entry of J = X^T dN is a sum of npe products of size |x| that leaves a cell side h:
    # (npe + 2) eps |x| / h of it; det J doubles that.  An entry of grad u is a sum of npe products |u| / h, each with the error
    # of J^-1 and two roundings, and the density is a quadratic form in dm^2 such entries, so twice their error over the largest
    npe, dm = el.shape[1], nodes.shape[1]
    h = float((np.ptp(nodes, axis=0) / np.asarray(ENERGY_BIG[1][:dm])).min())
    bj = (npe + 2) * EPS * float(np.abs(nodes).max()) / h
    strain = npe * float(np.abs(u).max()) / h * (bj + 2 * EPS)
    bounds = {"vol": 2 * bj, "density": 2 * dm * dm * strain / float(np.abs(F - np.eye(dm)).max())}
    return nodes, el, ELE, u.ravel(), ref, bounds


def energy_big(variant, backend):
    """1024 x 256 + 1 Gauss points: the grid-stride trip behind the cap of 1024 partials, and their host sum; the densities and
    weights of the second of two calls against the vectorised restatement, so a tail that is not written shows"""
    nodes, el, ELE, u, ref, bounds = big_case(variant)
    ne = len(el)
    ctx = lc.make_ctx(nodes, el, ELE, backend, pattern=False)
    # (the energy of the infinitesimal strain: it takes the weights of the undeformed mesh itself, where femcy_elastic_energy
    # reads what the last geometry pass left, and without a pattern there has been none)
    ctx.upload(be.VEC_DOF, -0.4 * u)
    ctx.elastic_energy(be.VEC_DOF, small=True)
    ctx.upload(be.VEC_DOF, u)
    tot = ctx.elastic_energy(be.VEC_DOF, small=True)
    assert tot == ctx.elastic_energy(be.VEC_DOF, small=True)
    dens, vol = _fields(ctx, be.GP_ENERGY, be.GP_VOL)
    ctx.close()
    ed, ev = _rel(dens, ref[LD][0]), _rel(vol, ref[LD][1])
    terms = dens.astype(LD) * vol.astype(LD)
    err = float(abs(LD(tot) - terms.sum()) / np.abs(terms).sum())
    print(f"energy of {ne} triangles, {variant} [{backend}]: total {err:.3e}, density {ed:.3e}, weights {ev:.3e}")
    want = ref[LD][0] * ref[LD][1]
    assert want[-1, -1] > 0 and (variant != "last" or want[-1].sum() >= 1e3 * (ne + 4) * EPS * want.sum())
    assert ed <= bounds["density"] and ev <= bounds["vol"], (ed, ev, bounds)
    assert err <= (ne + 4) * EPS, err
    return err


# ------------------------------------------------------------------------- 4. the load element passes at block edges
BLOCK_FAMILIES = tuple(POST_PLATES)
BLOCK_NE = ds.BLOCK_NE
BLOCK_CASES = [(family, ne) for family in BLOCK_FAMILIES for ne in BLOCK_NE]
SELECTIONS = ("all", "last", "all but last")
DT_VARIANTS = ("smooth", "last")


def bodyload(family, ne, backend):
    nodes, el, ELE = post_mesh(family, ne)
    dm = ELE.dm
    b = lc.B3[:dm]
    ctx = lc.make_ctx(nodes, el, ELE, backend)
    base = np.random.default_rng(ne).standard_normal(nodes.size)
    worst = 0.0
    for sel in SELECTIONS:
        ids = {"all": None, "last": np.array([ne - 1], np.int32), "all but last": np.arange(ne - 1, dtype=np.int32)}[sel]
        bl = ctx.bodyload(ELE, ids)
        m = ctx.bodyload_weights(bl)
        want = lr.nodal_weights(nodes, el, ELE, ids)
        outside = np.setdiff1d(np.arange(len(nodes)), el.ravel() if ids is None else el[ids].ravel())
        assert not m[outside].any() and (sel != "last" or outside.size)    # exactly 0.0 outside the selection
        assert np.abs(want[el[-1]]).min() > 0 or sel == "all but last"
        err = float(np.abs(m - want).max() / np.abs(want).max())
        assert err <= lc.SUM_TOL, (family, ne, sel, err)
        worst = max(worst, err)
        ctx.vector(be.VEC_RHS).fill(np.nan)
        ctx.bodyload_apply(bl, b, be.VEC_RHS)
        f = ctx.download(be.VEC_RHS)
        assert _bits(f, lr.load_vector(m, b))                         # exactly m_a * b_i
        ctx.upload(be.VEC_RHS, base)
        ctx.bodyload_apply(bl, b, be.VEC_RHS, add=True)
        assert _bits(ctx.download(be.VEC_RHS), base + f)
    ctx.close()
    print(f"bodyload {family} ne {ne} [{backend}]: weights {worst:.3e}")
    return worst


def thermal_dT(nodes, el, variant):
    dT = tr.smooth_dT(nodes)
    if variant == "last":
        keep = np.zeros(len(nodes), dtype=bool)
        keep[el[-1]] = True
        dT = np.where(keep, dT + 30.0, 0.0)
    return dT


@functools.lru_cache(maxsize=None)
def reference_thermal(family, ne, variant):
    """-> (long-double f_unit, error of the float64 restatement)"""
    nodes, el, ELE = post_mesh(family, ne)
    kind = tr.LIN3D if ELE.dm == 3 else tr.PSTRESS
    args = (nodes, el, ELE, tc.material(kind).C, kind, tc.NU, tc.ALPHA, thermal_dT(nodes, el, variant))
    ref = tr.thermal_force(*args, LD)
    ref.setflags(write=False)
    return ref, _rel(tr.thermal_force(*args, np.float64), ref)


def thermal(family, ne, variant, backend):
    nodes, el, ELE = post_mesh(family, ne)
    kind = tr.LIN3D if ELE.dm == 3 else tr.PSTRESS
    mat = tc.material(kind)
    dT = thermal_dT(nodes, el, variant)
    ref, _ = reference_thermal(family, ne, variant)
    ctx = tc.make_ctx(nodes, el, ELE, mat, backend)
    th = ctx.thermal(ELE, tc.ALPHA, dT)
    f = ctx.thermal_force(th)
    ef = _rel(f, ref)
    if variant == "last":
        outside = np.setdiff1d(np.arange(len(nodes)), np.unique(el[(np.isin(el, el[-1])).any(axis=1)]))
        assert outside.size and not f.reshape(len(nodes), -1)[outside].any()
    ctx.vector(be.VEC_RHS).fill(np.nan)
    ctx.thermal_apply(th, 1.0, be.VEC_RHS)
    assert _bits(ctx.download(be.VEC_RHS), f)
    for u in (-0.4 * tc.smooth_disp(nodes), tc.smooth_disp(nodes)):
        ctx.upload(be.VEC_DOF, u)
        ctx.compute_strain_stress(be.VEC_DOF, large=False)
    sigma0 = ctx.gauss_field(be.GP_SIGMA).to_numpy()
    ctx.thermal_stress(th, tc.SCALE)
    sig, mis = _fields(ctx, be.GP_SIGMA, be.GP_MISES)
    ctx.close()
    ref_s, ref_m = tr.corrected_stress(el, ELE, mat.C, kind, tc.NU, tc.ALPHA, dT, tc.SCALE, sigma0, LD)
    size = max(np.abs(sigma0).max(), float(np.abs(ref_s - sigma0.astype(LD)).max()))
    es, em = float(np.abs(sig - ref_s).max() / size), float(np.abs(mis - ref_m).max() / size)
    print(f"thermal {family} ne {ne} {variant} [{backend}]: force {ef:.3e}, stress {es:.3e}, mises {em:.3e}")
    assert np.abs(ref.reshape(len(nodes), -1)[el[-1]]).max() > 0 and np.abs(ref_s - sigma0)[-1].max() > 0
    assert ef <= tc.FORCE_TOL and es <= tc.STRESS_TOL and em <= tc.STRESS_TOL, (ef, es, em)
    return ef, es, em


# ------------------------------------------------------------------------------------------------------ the constants
def measure_f64_worst():
    """the constants at the top, as measured: the float64 restatement against the long-double one on the cases of this file"""
    worst = dict.fromkeys(F64_WORST, 0.0)
    for family, nload in SURFACE_CASES:
        for along_normal in (True, False):
            r = reference_surface(family, nload, along_normal)
            worst["surface"] = max(worst["surface"], _rel(r[np.float64][0], r[LD][0]))
    for family, ne, kind in POST_CASES:
        r = reference_post(family, ne, kind)
        for key in r[LD]:
            k = key[:-5] if key.endswith("_last") else key
            worst[k] = max(worst[k], _rel(r[np.float64][key], r[LD][key]))
    return worst
