"""Block, partial and gather edges of the dynamics kernels (csrc/kernels_explicit.hip: k_lumped_elem, k_explicit_bound,
k_explicit_energy, k_rowabs_bound, reduce_partials / k_explicit_final / k_explicit_clock, the node pass; csrc/node_gather.hpp;
csrc/kernels_pcg.hip: k_mass_spmv's partials, k_mass_add_to_K, k_newmark_predict / _update, k_fill / k_sub / k_axpy / k_scale,
k_reduce / k_reduce_final; csrc/kernels_assembly.hip: k_mass_points / k_mass_blocks, k_node_sum), written against the C ABI
(femcy_amd.backend.Context) so that the host backend (tests/test_dyn_shapes_cpu.py, backend "cpu") and the device
(tests/test_gpu_dyn_shapes.py, backend "hip") run the same code.  Every function checks its own result and returns the figure it
checked.  The case tables are static; nothing is skipped at run time.

The scenarios of dynamic_cases / explicit_cases / explicit_auto_cases / explicit_damped_cases are imported, not restated: they
look their meshes up by name, so MESHES below registers the meshes of this file under names of its own and `registered()`
puts the lookup in place for the length of one call.  Their tolerances are their own.

1. planted() -- a maximum planted in one element of 65 884 CPS3 (182 x 181 cells, np = 258 partials of 256 elements) and of
   66 792 C3D4 (23 x 22 x 22 cells, np = 261): one element shrunk about its centroid (PLANT_MESHES has the factor and why it
   is not 2), its row of `el` swapped into partial 0, 63, 64, 255, 256 and the last one (PLANT_AT).  Reference: explicit_auto_cases.reference_bound on the CANDIDATES
   -- the elements that touch a moved node, and element 0 for the congruent rest -- whose margin over everything else is
   asserted on the reference (>= MARGIN).  Plain, damped (omega_eff with a velocity that compresses the planted cell) and
   through two steps of the device clock (k_explicit_clock over np > 256).
2. rowabs() -- the same for k_rowabs_bound through femcy_explicit_stable_dt on a CPS4 plate of 300 nodes (320 stored row
   positions, two workgroups): the cells around one node shrunk towards it, the node chosen through the restated layout
   (asm_shapes.Layout) so that it sits in the first / last lane of workgroup 0, the first lane of workgroup 1 and the last
   stored position.  References: numpy on the backend's own K and lumped mass to the rounding of the row sum (explicit_cases.
   omega_bound's bound), and the long-double Gershgorin row sum from the oracle's K to ROWABS_TOL (below).
3. energy() -- femcy_explicit_kinetic_energy and femcy_mass_kinetic_energy against long-double sums at nn = 255, 256, 257 and
   2049 (ENERGY_MESHES; a prime node count comes from a plate whose trailing elements are dropped), v random and v non-zero in
   the last node only; and the explicit energy alone at nn = 1024 * 256 + 1 (the grid-stride trip behind reduction_grid's cap).
4. block_edge() -- lumped, mass_properties, mass_apply, the element bound and the damped element bound on the first 255 / 256 /
   257 elements of a plate of every family (BLOCK_PLATES).
5. gather_*() -- fans of 32, 33, 64 and 65 triangles whose hub is the last node and alone in the last workgroup of the node
   pass (nn % 8 == 1): one step, the lumped mass and the internal force.
6. vectors() -- the element-wise kernels and the two reductions under FEMCY_OPT_EW_GRID = 1 and 2 against long-double numpy,
   bit-equal to the default cap.  n = nn dm with dm = 2 or 3, so n = 511 and 1025 do not exist: the table takes 510 (n2 = 255),
   512 (n2 = 256), 513 (odd, n2 = 257), 1023 (odd, n2 = 512) and 1026 (n2 = 513, what n = 1025 would give).
7. add_to_K -- dynamic_cases.add_to_K at stored_rows * 64 = 192, 256 and 320.

Bounds.  Where a scenario is imported its bound is its own.  The gather cases follow explicit_cases: the float64 restatement
against the long-double one on these very cases (measure_f64_worst, asserted by tests/test_dyn_shapes_cpu.py), a backend is
held to 4 x that.  Measured: lumped mass 1.67e-16, one step 1.69e-15, internal force 6.24e-16.
ROWABS_TOL: omega = sqrt(minv_i sum_j |K_ij|).  The backend's K and the oracle's are two float64 evaluations of the same sums;
smoke() holds them to 1e-12 of the largest entry, a row sum of magnitudes is at least that entry, so the two row sums agree to
W 1e-12 / W; the square root halves it; the lumped mass adds explicit_cases.LUMPED_TOL / 2.  A partial that is dropped moves
omega by a factor sqrt(MARGIN) at least.
Energy sums: N terms summed in any order carry at most (N - 1) eps times the sum of their magnitudes; the explicit energy has
nn positive terms of a few operations (explicit_cases.one_step's bound (nn + 4) eps), the consistent one the nn dm row sums of
at most W products each, signs mixed: (nn dm + W + 4) eps |v|^T M |v| / 2."""
import collections
import contextlib
import functools

import numpy as np

from femcy_amd import backend as be
from oracle import femcy_oracle as orc
from oracle.elements import elem_def

import asm_shapes as ash
import dynamic_cases as dc
import dynamic_reference as dr
import explicit_auto_cases as eac
import explicit_cases as ec
import explicit_damped_cases as edc
import explicit_damped_reference as edr
import explicit_reference as er
import loads_cases as lc
import loads_reference as lr

LD = np.longdouble
EPS = ec.EPS
RHO = ec.RHO
XBS = 256                                                            # kernels_explicit.hip, kernels_pcg.hip (BS)
# worst error of the float64 restatement against the long-double one on the gather cases (measure_f64_worst, as measured)
F64_WORST_GATHER_LUMPED = 1.7e-16
F64_WORST_GATHER_STEP = 1.7e-15
F64_WORST_GATHER_FORCE = 6.3e-16
ROWABS_TOL = 0.5e-12 + ec.LUMPED_TOL / 2
MARGIN = 1.5

Mesh = collections.namedtuple("Mesh", "family build why")
MESHES = {}


def _first(nodes, el, ne):
    """the first ne elements and the nodes they name, renumbered in their order"""
    el = el[:ne]
    used = np.unique(el)
    new = -np.ones(len(nodes), dtype=np.int64)
    new[used] = np.arange(len(used))
    return np.ascontiguousarray(nodes[used]), np.ascontiguousarray(new[el], dtype=np.int32)


def shape_mesh(name, straight=False):
    m = MESHES[name]
    nodes, el, ELE = m.build(straight)
    return np.ascontiguousarray(nodes, dtype=np.float64), np.ascontiguousarray(el, dtype=np.int32), ELE


@contextlib.contextmanager
def registered():
    """the imported scenarios find the meshes of this file by name; everything is put back afterwards"""
    saved = dc.SHAPES, dc.shape_mesh, ec.shape_mesh
    dc.SHAPES = dict(saved[0], **{name: (m.family, None, 0.25) for name, m in MESHES.items()})
    dc.shape_mesh = lambda name: shape_mesh(name) if name in MESHES else saved[1](name)
    ec.shape_mesh = lambda name, straight=False: shape_mesh(name, straight) if name in MESHES else saved[2](name, straight)
    try:
        yield
    finally:
        dc.SHAPES, dc.shape_mesh, ec.shape_mesh = saved


# ------------------------------------------------------------------------------- 4. per-element block edges
# family -> the plate whose first 255 / 256 / 257 elements make the mesh (no structured mesh of every family hits the three
# counts, so every row drops the trailing elements of a larger plate and the nodes that only they name; every node that is
# left is named by an element).  Perturbed cells, curved sides on CPS8 / C3D10, as in dynamic_cases.SHAPES.
BLOCK_PLATES = {"CPS3": (16, 9), "CPS4": (16, 17), "CPS8": (16, 17), "C3D4": (4, 4, 3), "C3D8": (5, 4, 13), "C3D6": (4, 4, 9),
                "C3D10": (4, 4, 3)}
BLOCK_NE = (255, 256, 257)
BLOCK_PERTURB = 0.25
BLOCK_CHECKS = ("lumped", "mass", "apply", "bound", "damped")


def _block(family, ne):
    def build(straight):
        nodes, el, ELE = lr.mesh(family, cells=BLOCK_PLATES[family], perturb=0.0 if straight else BLOCK_PERTURB)
        nodes, el = _first(nodes, el, ne)
        # moved to the origin: with |x| / h of the 3 x 2 plate at 16 x 17 cells det J loses more digits than on the neighbours'
        # plates, and the float64 bounds of their scenarios were measured there
        return nodes - np.round(nodes.mean(axis=0), 1), el, ELE
    return Mesh(family, build, "the first %d elements of the %s plate %r" % (ne, family, BLOCK_PLATES[family]))


BLOCK_CASES = ["%s-ne%d" % (family, ne) for family in BLOCK_PLATES for ne in BLOCK_NE]
MESHES.update({"%s-ne%d" % (family, ne): _block(family, ne) for family in BLOCK_PLATES for ne in BLOCK_NE})


def block_edge(check, name, backend):
    """one imported scenario on one mesh of 255 / 256 / 257 elements"""
    with registered():
        nodes, el, _ = shape_mesh(name)
        assert len(el) == int(name.rsplit("ne", 1)[1]) and len(np.unique(el)) == len(nodes)
        if check == "lumped":
            return ec.lumped(name, False, backend)
        if check == "mass":
            return dc.mass_properties(name, backend)
        if check == "apply":
            return dc.mass_apply(name, backend)
        if check == "bound":
            return eac.bound(name, "linear", "smooth", None, backend)
        assert check == "damped"
        return edc.omega_eff(name, backend)


# ------------------------------------------------------------------------------------------ 7. mass_add_to_K
def _single(family):
    return lambda straight: lr.single(family)[:3]


def _two_tets(straight):
    nodes, el, ELE, _ = lr.single("C3D4")
    apex = nodes[:3].mean(axis=0) - (nodes[3] - nodes[:3].mean(axis=0))        # node 3 mirrored through the face 0-1-2
    return np.vstack([nodes, apex]), np.array([[0, 1, 2, 3], [0, 2, 1, 4]], np.int32), ELE


# name -> stored_rows * 64: one slice, its longest row has 3, 4 and 5 blocks
ADD_TO_K_CASES = {"k-cps3-192": 192, "k-cps4-256": 256, "k-c3d4-256": 256, "k-fan4-320": 320, "k-tets-320": 320}
MESHES.update({"k-cps3-192": Mesh("CPS3", _single("CPS3"), "one triangle: rows of 3 blocks"),
               "k-cps4-256": Mesh("CPS4", _single("CPS4"), "one quadrilateral: rows of 4 blocks"),
               "k-c3d4-256": Mesh("C3D4", _single("C3D4"), "one tetrahedron: rows of 4 blocks"),
               "k-fan4-320": Mesh("CPS3", lambda straight: lr.fan(4), "four triangles round a hub: its row has 5 blocks"),
               "k-tets-320": Mesh("C3D4", _two_tets, "two tetrahedra on one face: the face's rows have 5 blocks")})


def add_to_K(name, backend):
    with registered():
        nodes, el, ELE = shape_mesh(name)
        ctx = lc.make_ctx(nodes, el, ELE, backend)
        info = ctx.pattern_info()
        ctx.close()
        assert info.max_row_blocks * 64 == ADD_TO_K_CASES[name] and len(nodes) <= 64
        if backend == "hip":                                          # (the host library stores block-CSR)
            assert info.stored_blocks == ADD_TO_K_CASES[name], info.stored_blocks
        dc.add_to_K(name, backend)


# ---------------------------------------------------------------------------------------------- 5. gather trips
# fan of k triangles + a strip beside it, the hub renumbered to be the last node: nn % 8 == 1, so the hub is the only node of
# the last workgroup of the node pass (8 nodes per workgroup) and the other seven half-waves hold no node
GATHER_FANS = {32: (3, 1), 33: (4, 2), 64: (3, 1), 65: (4, 2)}     # k -> cells of the strip
GATHER_CASES = ["fan-%d" % k for k in GATHER_FANS]


def _fan(k):
    def build(straight):
        fn, fe, ELE = lr.fan(k)
        sn, se, _ = lr.mesh("CPS3", cells=GATHER_FANS[k], perturb=0.0)
        nodes = np.vstack([fn, sn * 0.5 + np.array([2.0, -0.5])])
        el = np.vstack([fe, se + len(fn)]).astype(np.int64)
        last = len(nodes) - 1                                          # the hub (node 0) trades places with the last node
        nodes[[0, last]] = nodes[[last, 0]]
        el = np.where(el == 0, -1, el)
        el = np.where(el == last, 0, el)
        el = np.where(el == -1, last, el)
        return nodes, el.astype(np.int32), ELE
    return Mesh("CPS3", build, "a fan of %d triangles, its hub the last of 8 m + 1 nodes" % k)


MESHES.update({"fan-%d" % k: _fan(k) for k in GATHER_FANS})


def gather_edge(name):
    """the table's own arithmetic: the incidence of the hub, its place, nn % 8"""
    nodes, el, _ = shape_mesh(name)
    k = int(name.split("-")[1])
    cnt = np.bincount(el.ravel(), minlength=len(nodes))
    assert len(nodes) % 8 == 1 and cnt[-1] == k == cnt.max() and cnt.min() >= 1 and cnt[:-1].max() <= 6, (len(nodes), cnt)
    return cnt


@functools.lru_cache(maxsize=None)
def reference_gather(name):
    """-> {dtype: (a0, u1, v1, a1, f_int(u0))} of explicit_cases.step_setup's state, composed as one_step composes it"""
    with registered():
        nodes, el, ELE, fixed, f, u0, v0, h, s = ec.step_setup(name)
    out = {}
    for dt in (LD, np.float64):
        mdl = er.Model(nodes, el, ELE, ec.material_of(ELE), dt)
        minv = 1 / np.repeat(er.lumped_mass(nodes, el, ELE, RHO, dt), ELE.dm)
        minv[fixed] = 0
        u0d, v0d, fd, hd = np.asarray(u0, dtype=dt), np.asarray(v0, dtype=dt), np.asarray(f, dtype=dt), dt(h)
        f0 = mdl.f_int(u0d)
        a0 = minv * (dt(s) * fd - f0)
        u1 = u0d + hd * v0d + (hd * hd / 2) * a0
        a1 = minv * (dt(s) * fd - mdl.f_int(u1))
        out[dt] = (a0, u1, v0d + (hd / 2) * (a0 + a1), a1, f0)
    for x in out[LD]:
        x.setflags(write=False)
    return out


def _rel(got, want):
    return float(np.abs(np.asarray(got, dtype=LD) - want).max() / np.abs(want).max())


def gather_step(name, backend):
    """explicit_cases.one_step (against the backend's own composition), then start + one step against the long-double
    composition"""
    gather_edge(name)
    with registered():
        ec.one_step(name, backend)
        nodes, el, ELE, fixed, f, u0, v0, h, s = ec.step_setup(name)
    ref = reference_gather(name)[LD]
    ctx = lc.make_ctx(nodes, el, ELE, backend)
    assert ctx.pattern_info().max_node_elems == int(name.split("-")[1])
    _, ex = ec.make_explicit(ctx, ELE, fixed)
    for vec, arr in ((be.VEC_DOF, u0), (be.VEC_VEL, v0), (be.VEC_RHS, f)):
        ctx.upload(vec, arr)
    ctx.upload(be.VEC_ACC, np.full(nodes.size, np.nan))                # not read at the start
    ctx.explicit_start(ex, be.VEC_RHS, s)
    a0 = ctx.download(be.VEC_ACC)
    ctx.explicit_advance(ex, 1, h, be.VEC_RHS, s, 0.0)
    got = [a0] + [ctx.download(v) for v in (be.VEC_DOF, be.VEC_VEL, be.VEC_ACC)]
    ctx.close()
    err = max(_rel(g, w) for g, w in zip(got, ref[:4]))
    hub = max(float(np.abs(np.asarray(g[-2:], dtype=LD) - w[-2:]).max() / np.abs(w).max()) for g, w in zip(got, ref[:4]))
    print(f"{name} [{backend}]: one step against the long-double composition {err:.3e} (the hub {hub:.3e})")
    assert np.abs(ref[3][-2:]).min() > 0 and err <= 4.0 * F64_WORST_GATHER_STEP, err
    return err


def gather_lumped(name, backend):
    """explicit_cases.lumped (k_node_sum's gather), and its error against this file's own constant"""
    gather_edge(name)
    with registered():
        err = ec.lumped(name, False, backend)
    assert err <= 4.0 * F64_WORST_GATHER_LUMPED, err
    return err


def gather_force(name, backend):
    """femcy_internal_force (k_nodal_force's gather) at the step's u_0 against the long-double node sums; the output vector is
    filled with NaN first"""
    gather_edge(name)
    with registered():
        nodes, el, ELE, fixed, f, u0, v0, h, s = ec.step_setup(name)
    want = reference_gather(name)[LD][4]
    ctx = lc.make_ctx(nodes, el, ELE, backend)
    ctx.upload(be.VEC_DOF, u0)
    ctx.vector(be.VEC_FORCE).fill(np.nan)
    ctx.internal_force(be.VEC_DOF, be.VEC_FORCE)
    got = ctx.download(be.VEC_FORCE)
    ctx.close()
    err = _rel(got, want)
    print(f"{name} [{backend}]: internal force {err:.3e}, the hub's share of the largest entry "
          f"{float(np.abs(want[-2:]).max() / np.abs(want).max()):.2f}")
    assert np.abs(want[-2:]).min() > 0 and err <= 4.0 * F64_WORST_GATHER_FORCE, err
    return err


def measure_f64_worst():
    """the constants at the top, as measured: the float64 restatement against the long-double one on the gather cases"""
    with registered():
        wl = max(ec.reference_lumped(name, False)[1] for name in GATHER_CASES)
    ws = wf = 0.0
    for name in GATHER_CASES:
        ref = reference_gather(name)
        ws = max(ws, max(_rel(x64, x) for x64, x in zip(ref[np.float64][:4], ref[LD][:4])))
        wf = max(wf, _rel(ref[np.float64][4], ref[LD][4]))
    return {"lumped": wl, "step": ws, "force": wf}


# ------------------------------------------------------------------------------- 1. planted maximum, element bound
# family -> (cells, the sides of a cell, the factor its nodes move towards the centroid by, ne, np).  Nodes are shared, so the
# elements next to the shrunken one are squeezed too; how far they stay below it depends on the shape of the cells and only
# weakly on the factor (a factor of 2 on the 3 : 2 plate of loads_reference gives 1.23, in the limit of a point 1.30): square
# cells and 0.3 give 1.54 on CPS3; the six tetrahedra of a cube stop at 1.31, those of a 1 x 1 x 3 cell at 0.1 reach 1.51
PLANT_MESHES = {"CPS3": ((182, 181), (1.0, 1.0), 0.3, 65884, 258), "C3D4": ((23, 22, 22), (1.0, 1.0, 3.0), 0.1, 66792, 261)}
PLANT_H = 1.0 / 64                                                    # the unit of a cell's sides
PLANT_AT = (0, 63, 64, 255, 256, "last")                              # the partial that holds the planted element
PLANT_LANE = 37                                                       # its thread there (the last partial: the last element)
PLANT_CASES = [(family, at) for family in PLANT_MESHES for at in PLANT_AT]
PLANT_SF, PLANT_SPEED = 0.9, 2000.0


def _shrunk(nodes, el, e, factor):
    nodes = nodes.copy()
    c = nodes[el[e]].mean(axis=0)
    nodes[el[e]] = c + factor * (nodes[el[e]] - c)
    cand = np.nonzero(np.isin(el, el[e]).any(axis=1))[0]
    return nodes, np.concatenate([[e], cand[cand != e]])


@functools.lru_cache(maxsize=2)
def _plant_base(family):
    """-> nodes with one interior element shrunk about its centroid, el, ELE, that element, the candidates (the elements that
    name a moved node, and element 0 for the congruent rest); numpy only.  The element is the one of the cell in the middle
    of the mesh whose neighbours stay lowest (float64 is enough to tell them apart)"""
    cells, sides, factor = PLANT_MESHES[family][:3]
    nodes, el, ELE = lr.mesh(family, cells=cells, perturb=0.0)
    nodes = np.array(nodes, dtype=np.float64) * (np.asarray(cells) / np.ptp(nodes, axis=0) * np.asarray(sides) * PLANT_H)[None, :]
    if family == "CPS3":                                               # loads_reference._tris: the lower triangles, then the upper
        cell = (cells[1] // 2) * cells[0] + cells[0] // 2
        middle = (cell, cells[0] * cells[1] + cell)
    else:                                                             # meshgen.plate_grid: six tetrahedra per cell, x fastest
        cell = ((cells[2] // 2) * cells[1] + cells[1] // 2) * cells[0] + cells[0] // 2
        middle = tuple(range(6 * cell, 6 * cell + 6))
    best = None
    for e in middle:
        moved, cand = _shrunk(nodes, el, int(e), factor)
        w2 = eac.Estimate(moved, el[cand], ELE, ec.material_of(ELE), RHO, np.float64).elements(np.zeros(nodes.size))[1]
        if best is None or w2[0] / w2[1:].max() > best[0]:
            best = (w2[0] / w2[1:].max(), int(e))
    e0 = best[1]
    nodes, cand = _shrunk(nodes, el, e0, factor)
    assert 0 not in cand and len(cand) < 128
    nodes.setflags(write=False)
    return nodes, el, ELE, e0, np.concatenate([cand, [0]])


def plant_mesh(family, at):
    """the planted element's row of `el` swapped to its place; -> nodes, el, ELE, its index, the candidates"""
    nodes, el, ELE, e0, cand = _plant_base(family)
    ne = len(el)
    target = ne - 1 if at == "last" else at * XBS + PLANT_LANE
    el = el.copy()
    el[[target, e0]] = el[[e0, target]]
    cand = np.where(cand == e0, target, np.where(cand == target, e0, cand))
    return nodes, el, ELE, target, cand


def _plant_sub(family, at):
    """the candidates as a mesh of their own: -> nodes, el, ELE, the node ids they came from"""
    nodes, el, ELE, target, cand = plant_mesh(family, at)
    used = np.unique(el[cand])
    new = -np.ones(len(nodes), dtype=np.int64)
    new[used] = np.arange(len(used))
    return np.ascontiguousarray(nodes[used]), new[el[cand]].astype(np.int32), ELE, used


MESHES.update({"planted-%s" % family: Mesh(family, (lambda f: lambda straight: _plant_sub(f, 0)[:3])(family),
                                           "the candidates of the planted %s mesh: the planted element first, a regular one last" % family)
               for family in PLANT_MESHES})


def plant_velocity(nodes, el, target):
    """the planted element's nodes move towards its centroid at PLANT_SPEED per unit of distance; every other node rests"""
    v = np.zeros_like(nodes)
    c = nodes[el[target]].mean(axis=0)
    v[el[target]] = -PLANT_SPEED * (nodes[el[target]] - c)
    return v


@functools.lru_cache(maxsize=None)
def reference_planted(family):
    """on the candidates alone: -> (omega plain, omega_eff damped, margin plain, margin damped) in long double; the margins are
    the planted element's omega^2 over the largest of the others"""
    with registered():
        name = "planted-%s" % family
        om, _, arg, _ = eac.reference_bound(name, "linear", "rest", None)
        nodes, el, ELE = shape_mesh(name)
    assert arg == 0
    mat = ec.material_of(ELE)
    est = eac.Estimate(nodes, el, ELE, mat, RHO, LD)
    w2 = est.elements(np.zeros(nodes.size))[1]
    mdl = edr.DampedModel(nodes, el, ELE, mat, LD, RHO, edc.ALPHA, edc.B1, edc.B2, edc.modulus(mat))
    v = plant_velocity(nodes, el, 0).ravel()
    each = []
    for e in range(len(el)):                                           # a few dozen candidates
        one = edr.DampedModel(nodes, el[e:e + 1], ELE, mat, LD, RHO, edc.ALPHA, edc.B1, edc.B2, edc.modulus(mat))
        each.append(one.omega_eff(eac.Estimate(nodes, el[e:e + 1], ELE, mat, RHO, LD), np.zeros(nodes.size), v))
    each = np.array(each)
    om_d = mdl.omega_eff(est, np.zeros(nodes.size), v)
    assert om_d == each.max() == each[0] and om_d > 1.05 * om
    return om, om_d, float(w2[0] / w2[1:].max()), float((each[0] / each[1:].max()) ** 2)


def planted_margin(family):
    """CPU reference alone: the planted element exceeds every other candidate, the regular element included, by MARGIN"""
    _, _, plain, damped = reference_planted(family)
    assert plain >= MARGIN and damped >= MARGIN, (plain, damped)
    ne, np_ = PLANT_MESHES[family][3:]
    nodes, el, _, _, cand = _plant_base(family)
    assert len(el) == ne > 65536 and -(-ne // XBS) == np_ > XBS
    for at in PLANT_AT:
        _, el_at, _, target, cand_at = plant_mesh(family, at)
        assert target // XBS == (np_ - 1 if at == "last" else at) and cand_at[0] == target
        assert np.array_equal(np.sort(el_at, axis=0), np.sort(el, axis=0))          # a renumbering of `el`
    return plain, damped


def planted(family, at, backend):
    """femcy_explicit_element_bound plain and damped, and h_last after two steps of the device clock"""
    nodes, el, ELE, target, cand = plant_mesh(family, at)
    om_ref, omd_ref, _, _ = reference_planted(family)
    mat = ec.material_of(ELE)
    ctx = eac.make_ctx(nodes, el, ELE, mat, backend)
    assert -(-ctx.ne // XBS) == PLANT_MESHES[family][4]
    _, ex = ec.make_explicit(ctx, ELE, [])
    sc = float(eac.s_C(mat))
    om = ctx.explicit_element_bound(ex, sc, be.VEC_DOF)
    assert om == ctx.explicit_element_bound(ex, sc, be.VEC_DOF)
    # the clock: u = v = f = 0, so nothing moves and every increment is sf 2 / omega; T is out of reach
    ctx.explicit_auto_begin(ex, sc, PLANT_SF, 1.0, False, be.VEC_RHS)
    ctx.explicit_auto_advance(ex, 2, be.VEC_RHS)
    t, h_last, h_min, steps = ctx.explicit_auto_state(ex)
    assert not np.abs(ctx.download(be.VEC_DOF)).any()
    ctx.upload(be.VEC_VEL, plant_velocity(nodes, el, target).ravel())
    ctx.explicit_set_damping(ex, edc.ALPHA, edc.B1, edc.B2, edc.modulus(mat))
    omd = ctx.explicit_element_bound(ex, sc, be.VEC_DOF)
    ctx.close()
    err = float(abs(LD(om) - om_ref) / om_ref)
    errd = float(abs(LD(omd) - omd_ref) / omd_ref)
    h_ref = LD(PLANT_SF) * (2 / om_ref)
    eh = float(abs(LD(h_last) - h_ref) / h_ref)
    print(f"{family} planted in partial {at} (element {target}) [{backend}]: omega {err:.3e}, omega_eff {errd:.3e}, h_last {eh:.3e}")
    assert err <= eac.BOUND_TOL, err
    assert errd <= 4.0 * edc.F64_WORST_OMEGA, errd
    assert steps == 2 and h_min == h_last and t == h_last + h_last
    assert eh <= eac.BOUND_TOL + 4 * EPS, eh                          # omega's error, the quotient and the product
    return err, errd, eh


# ----------------------------------------------------------------------------- 2. planted maximum, Gershgorin bound
ROWABS_CELLS = (19, 14)                                               # CPS4: 300 nodes, 5 slices, 320 stored row positions
ROWABS_AT = ("first lane of workgroup 0", "last lane of workgroup 0", "first lane of workgroup 1", "last stored position")
ROWABS_SIGMA = 64
ROWABS_FIRST, ROWABS_FACTOR = 7 * 20 + 10, 0.35


def rowabs_mesh(at):
    """-> nodes, el, ELE, the planted node, its storage position: every node that shares a cell with the planted one moved
    towards it, to ROWABS_FACTOR of its distance"""
    nodes, el, ELE = lr.mesh("CPS4", cells=ROWABS_CELLS, perturb=0.0)
    new = (np.arange(len(nodes)) - ROWABS_FIRST) % len(nodes)         # numbered from the middle of the plate on, cyclically: the
    nodes, el = nodes[np.argsort(new)], new[el].astype(np.int32)      # four positions then hold no neighbour of a corner node
    lay = ash.Layout(nodes, el, ROWABS_SIGMA)
    stored = np.nonzero(lay.node_of >= 0)[0]
    p = {ROWABS_AT[0]: 0, ROWABS_AT[1]: XBS - 1, ROWABS_AT[2]: XBS, ROWABS_AT[3]: int(stored[-1])}[at]
    a = int(lay.node_of[p])
    assert a >= 0 and XBS < lay.nslices * 64 < 2 * XBS and stored[-1] == len(nodes) - 1
    nodes = np.array(nodes, dtype=np.float64)
    ring = np.setdiff1d(np.unique(el[(el == a).any(axis=1)]), [a])
    nodes[ring] = nodes[a] + ROWABS_FACTOR * (nodes[ring] - nodes[a])
    return nodes, el, ELE, a, p


@functools.lru_cache(maxsize=None)
def reference_rowabs(at):
    """-> (omega of the planted node's rows in long double from the oracle's K, its margin over every other row)"""
    nodes, el, ELE, a, _ = rowabs_mesh(at)
    K = orc.assemble_K(orc.Topology(nodes, el, elem_def("CPS4")), np.zeros(nodes.size), orc.Material("pstress", (ec.E_MOD, ec.NU)).C)
    minv = 1 / np.repeat(er.lumped_mass(nodes, el, ELE, RHO, LD), 2)
    rows = np.abs(K.toarray().astype(LD)).sum(axis=1) * minv
    mine = rows[2 * a:2 * a + 2].max()
    rest = np.delete(rows, [2 * a, 2 * a + 1]).max()
    return np.sqrt(mine), float(mine / rest)


def rowabs_margin(at):
    om, margin = reference_rowabs(at)
    assert margin >= MARGIN, margin
    return margin


def rowabs(at, backend):
    """femcy_explicit_stable_dt with the largest row in a chosen lane"""
    nodes, el, ELE, a, p = rowabs_mesh(at)
    ref, _ = reference_rowabs(at)
    ctx = be.Context(0, backend=backend)
    ctx.set_option(be.OPT_NODE_ORDER, 0)                             # the caller's numbering: what the layout restates
    ctx.set_option(be.OPT_SELL_SIGMA, ROWABS_SIGMA)
    ctx.set_mesh(nodes, el)
    ctx.set_element(ELE)
    ctx.set_material(ec.material_of(ELE))
    info = ctx.build_pattern()
    if backend == "hip":
        assert info.nslices * 64 == 320, info.nslices
    lm, ex = ec.make_explicit(ctx, ELE, [])
    ctx.assemble_K(-1)
    K = ctx.get_K_bsr().toarray()
    minv = 1.0 / np.repeat(ctx.lumped_mass_get(lm), 2)
    dt, om = ctx.explicit_stable_dt(ex)
    width = info.max_row_blocks * 2
    ctx.close()
    rows = np.abs(K.astype(LD)).sum(axis=1) * minv
    assert int(np.argmax(rows)) // 2 == a
    own = float(abs(LD(om) - np.sqrt(rows.max())) / np.sqrt(rows.max()))
    err = float(abs(LD(om) - ref) / ref)
    print(f"rowabs, {at} (node {a}, position {p}) [{backend}]: against its own K {own:.3e}, against the oracle's {err:.3e}")
    assert own <= (width + 2) * EPS, own                              # explicit_cases.omega_bound's bound
    assert err <= ROWABS_TOL and dt == 2.0 / om, err
    return err


# ------------------------------------------------------------------------------------------------ 3. energy sums
# name -> (family, cells, elements kept (None: all), nn).  257 is prime and 2049 = 3 x 683 fits no C3D8 column: those plates
# drop their trailing elements, and with them the nodes that only those name
ENERGY_MESHES = {"CPS4-255": ("CPS4", (2, 84), None, 255), "CPS4-256": ("CPS4", (1, 127), None, 256),
                 "CPS4-257": ("CPS4", (2, 85), 169, 257), "CPS4-2049": ("CPS4", (2, 682), None, 2049),
                 "C3D8-255": ("C3D8", (2, 4, 16), None, 255), "C3D8-256": ("C3D8", (1, 1, 63), None, 256),
                 "C3D8-257": ("C3D8", (4, 3, 12), 141, 257), "C3D8-2049": ("C3D8", (2, 2, 227), 906, 2049)}
ENERGY_BIG = ("CPS3", (544, 480), None, 1024 * 256 + 1)
ENERGY_VARIANTS = ("random", "last")


def energy_mesh(name):
    family, cells, keep, nn = ENERGY_BIG if name == "big" else ENERGY_MESHES[name]
    nodes, el, ELE = lr.mesh(family, cells=cells, perturb=0.0 if name == "big" else 0.25)
    if keep is not None:
        nodes, el = _first(nodes, el, keep)
    assert len(nodes) == nn and len(np.unique(el)) == nn, (name, len(nodes), len(np.unique(el)))
    return np.ascontiguousarray(nodes, dtype=np.float64), np.ascontiguousarray(el, dtype=np.int32), ELE


def energy_velocity(nn, dm, variant):
    v = np.random.default_rng(17).uniform(-1.0, 1.0, (nn, dm))
    if variant == "last":
        v[:-1] = 0.0
    return v


def consistent_energy(nodes, el, ELE, v):
    """-> (v^T M v / 2, |v|^T M |v| / 2) in long double, element by element (dynamic_reference.element_mass)"""
    tables = dr.mass_tables(ELE, LD)
    X, V = np.asarray(nodes, dtype=LD), np.asarray(v, dtype=LD)
    total, mag = LD(0), LD(0)
    for conn in el:
        me = dr.element_mass(X[conn], tables, LD(RHO))
        total += (V[conn] * (me @ V[conn])).sum() / 2
        mag += (np.abs(V[conn]) * (me @ np.abs(V[conn]))).sum() / 2
    return total, mag


def energy(name, variant, backend):
    """both kinetic energies on one mesh; the lumped masses are the backend's own (what is checked is the sum)"""
    nodes, el, ELE = energy_mesh(name)
    dm = ELE.dm
    v = energy_velocity(len(nodes), dm, variant)
    ctx = lc.make_ctx(nodes, el, ELE, backend)
    lm, ex = ec.make_explicit(ctx, ELE, [])
    m = ctx.lumped_mass_get(lm)
    ctx.upload(be.VEC_VEL, v.ravel())
    ke = ctx.explicit_kinetic_energy(ex, be.VEC_VEL)
    again = ctx.explicit_kinetic_energy(ex, be.VEC_VEL)
    want = er.kinetic(m, v, dm, LD)
    e1 = float(abs(LD(ke) - want) / want)
    assert ke == again and want > 0 and (m > 0).all()
    e2 = 0.0
    if name != "big":
        ms = ctx.mass(ELE, RHO)
        width = ctx.pattern_info().max_row_blocks
        kc = ctx.mass_kinetic_energy(ms, be.VEC_VEL)
        assert kc == ctx.mass_kinetic_energy(ms, be.VEC_VEL)
        wantc, mag = consistent_energy(nodes, el, ELE, v)
        e2 = float(abs(LD(kc) - wantc) / mag)
        assert wantc > 0 and e2 <= (len(nodes) * dm + width + 4) * EPS, e2
    ctx.close()
    print(f"{name} {variant} [{backend}]: {len(nodes)} nodes, lumped kinetic energy {e1:.3e}, consistent {e2:.3e}")
    assert e1 <= (len(nodes) + 4) * EPS, e1
    return e1, e2


# ------------------------------------------------------------------------------- 6. element-wise kernels, small caps
# n -> (family of the one element that carries the mesh, nn): the other nodes are loose
VECTOR_N = {510: ("CPS3", 255), 512: ("CPS3", 256), 513: ("C3D4", 171), 1023: ("C3D4", 341), 1026: ("C3D4", 342)}
VECTOR_CAPS = (1, 2)
DEFAULT_CAP = 512


def vector_ctx(n, backend):
    family, nn = VECTOR_N[n]
    nodes, el, ELE, _ = lr.single(family)
    far = nodes.max(axis=0) + 1.0 + 0.01 * np.arange(nn - len(nodes))[:, None]
    ctx = lc.make_ctx(np.vstack([nodes, far]), el, ELE, backend)
    assert ctx.n == n
    return ctx


def _vector_run(ctx, n):
    """every kernel once on fixed data -> {name: result}; the Newmark calls at odd n are followed by femcy_vec_norm on every
    vector they touched"""
    rng = np.random.default_rng(n)
    u, v, a, un = (rng.standard_normal(n) for _ in range(4))
    out = {"in": (u, v, a, un)}
    norms = {}

    def norm_of(tag, vecs):
        for vec in vecs:
            norms[(tag, vec)] = (ctx.vec_norm(vec), ctx.download(vec))

    for vec, arr in ((be.VEC_DOF_OLD, u), (be.VEC_VEL, v), (be.VEC_ACC, a), (be.VEC_DOF, un)):
        ctx.upload(vec, arr)
    ctx.vector(be.VEC_RESIDUAL).fill(np.nan)
    ctx.newmark_predict(be.VEC_DOF_OLD, be.VEC_VEL, be.VEC_ACC, be.VEC_RESIDUAL, 3.5, -0.25, 1.75)
    norm_of("predict", (be.VEC_DOF_OLD, be.VEC_VEL, be.VEC_ACC, be.VEC_RESIDUAL))
    out["predict"] = ctx.download(be.VEC_RESIDUAL)
    ctx.newmark_update(be.VEC_DOF, be.VEC_DOF_OLD, be.VEC_VEL, be.VEC_ACC, 0.3025, 0.6, 0.125)
    norm_of("update", (be.VEC_DOF, be.VEC_DOF_OLD, be.VEC_VEL, be.VEC_ACC))
    out["update"] = (ctx.download(be.VEC_ACC), ctx.download(be.VEC_VEL), ctx.download(be.VEC_DOF), ctx.download(be.VEC_DOF_OLD))
    ctx.upload(be.VEC_TMP0, u)
    ctx.upload(be.VEC_RHS, v)
    ctx.vector(be.VEC_TMP1).fill(np.nan)
    ctx.vec_sub(be.VEC_TMP1, be.VEC_TMP0, be.VEC_RHS)
    out["sub"] = ctx.download(be.VEC_TMP1)
    ctx.vector(be.VEC_DU).fill(np.nan)
    ctx.vec_axpy(be.VEC_DU, be.VEC_TMP0, -0.3, be.VEC_RHS)
    out["axpy"] = ctx.download(be.VEC_DU)
    ctx.vec_scale(be.VEC_DU, 0.7)
    out["scale"] = ctx.download(be.VEC_DU)
    ctx.vector(be.VEC_DU).fill(3.5)
    out["fill"] = ctx.download(be.VEC_DU)
    out["norm"] = ctx.vec_norm(be.VEC_TMP0)
    out["absmax"] = ctx.vec_absmax(be.VEC_TMP0)
    w = u.copy()
    w[-1] = 7.0 * np.abs(u).max()                                      # the maximum in the last entry
    ctx.upload(be.VEC_TMP0, w)
    out["absmax_last"] = (ctx.vec_absmax(be.VEC_TMP0), float(np.abs(w[-1])))
    w[:-1] = 0.0
    ctx.upload(be.VEC_TMP0, w)
    out["norm_last"] = (ctx.vec_norm(be.VEC_TMP0), w)                # a sum that is the last entry alone
    w = u.copy()
    w[-1] = np.nan
    ctx.upload(be.VEC_TMP0, w)
    out["absmax_nan"] = ctx.vec_absmax(be.VEC_TMP0)
    out["norms"] = norms
    return out


def _rms(x):
    x = np.asarray(x, dtype=LD)
    return np.sqrt((x * x).sum() / x.size)


def vectors(n, backend):
    """caps 1 and 2 against long-double numpy, and bit-equal to the default cap"""
    ctx = vector_ctx(n, backend)
    runs = {}
    for cap in VECTOR_CAPS + (DEFAULT_CAP,):
        ctx.set_option(be.OPT_EW_GRID, cap)
        runs[cap] = _vector_run(ctx, n)
    ctx.close()
    worst = 0.0
    for cap, r in runs.items():
        what = (n, cap)
        u, v, a, un = (x.astype(LD) for x in r["in"])
        # dynamic_cases.newmark_kernels' bounds: three products and two sums; the update's few operations
        size = np.abs(3.5 * u) + np.abs(0.25 * v) + np.abs(1.75 * a)
        assert (np.abs(r["predict"] - (3.5 * u - 0.25 * v + 1.75 * a)) <= 4 * EPS * size).all(), what
        beta, gamma, dt = LD(0.3025), LD(0.6), LD(0.125)
        b0, b1, b2 = 1 / (beta * dt * dt), 1 / (beta * dt), 1 / (2 * beta) - 1
        an = b0 * (un - u) - b1 * v - b2 * a
        vn = v + dt * ((1 - gamma) * a + gamma * an)
        sa = b0 * (np.abs(un) + np.abs(u)) + b1 * np.abs(v) + abs(b2) * np.abs(a)
        got_a, got_v, got_un, got_u = r["update"]
        assert (np.abs(got_a - an) <= 8 * EPS * sa).all(), what
        assert (np.abs(got_v - vn) <= 8 * EPS * (np.abs(v) + dt * (np.abs(a) + sa))).all(), what
        assert np.array_equal(got_un, r["in"][3]) and np.array_equal(got_u, r["in"][0]), what
        assert np.array_equal(r["sub"], r["in"][0] - r["in"][1]), what                       # one rounding
        ax = u - LD(0.3) * v
        assert (np.abs(r["axpy"] - ax) <= 4 * EPS * (np.abs(u) + np.abs(0.3 * v))).all(), what
        assert np.array_equal(r["scale"], r["axpy"] * 0.7), what                             # one rounding
        assert (r["fill"] == 3.5).all() and r["fill"].shape == (n,), what
        # the bounds of tests/test_gpu_parity.py: the norm to 1e-13, the maximum exactly
        en = float(abs(LD(r["norm"]) - _rms(u)) / _rms(u))
        worst = max(worst, en)
        assert en < 1e-13, (what, en)
        assert r["absmax"] == np.abs(r["in"][0]).max(), what
        assert r["absmax_last"][0] == r["absmax_last"][1], what
        assert r["absmax_nan"] == np.inf, what
        got, w = r["norm_last"]
        assert abs(LD(got) - _rms(w)) < 1e-13 * _rms(w), what
        for (tag, vec), (got, x) in r["norms"].items():             # the pad entry behind an odd n is still zero
            assert np.isfinite(x).all() and abs(LD(got) - _rms(x)) <= 1e-13 * _rms(x), (what, tag, vec, got)
    for cap in VECTOR_CAPS:
        for key in ("predict", "sub", "axpy", "scale", "fill"):
            assert np.array_equal(runs[cap][key].view(np.uint64), runs[DEFAULT_CAP][key].view(np.uint64)), (n, cap, key)
        for x, y in zip(runs[cap]["update"], runs[DEFAULT_CAP]["update"]):
            assert np.array_equal(x.view(np.uint64), y.view(np.uint64)), (n, cap, "update")
    print(f"n = {n} [{backend}]: caps {VECTOR_CAPS} and {DEFAULT_CAP}, worst norm error {worst:.3e}")
    return worst
