"""The multi-rank device path at the shapes slab cuts never produce (csrc/kernels_pcg.hip: k_iface_pack_all, k_iface_unpack,
k_p2p_pack, k_p2p_sum, the owner branches of k_pcg_init / k_update_xr / k_update_d / k_reduce, k_sum_partials2, the gathered
k_pcg_init_final, split_prepare / launch_spmv_part; csrc/kernels_assembly.hip: the owner branch of k_dirichlet_zero;
csrc/femcy_api.cpp: femcy_comm_set_neighbours' tables, apply_load's interface sum, the collective femcy_apply_dirichlet_linear),
written against the C ABI through the in-process transport (femcy_comm_local_id: one host thread per rank on one GPU, sums in
rank order, a rendezvous that gives up after 60 s).  The host backend has no communicator, so tests/test_rank_shapes_cpu.py
asserts the tables, the reference conditions and the constants, and tests/test_gpu_rank_shapes.py runs the checks.  Every
check returns the figure it checked.  The case tables are static; nothing is skipped at run time.

Cases (CASES; the claims beside each are asserted by case_table()):
1. block edges, two ranks -- a CPS4 plate two cells wide whose cut holds 127 / 128 / 129 nodes: 254 / 256 / 258 slots (n = nn dm,
   so 255 and 257 do not exist for dm = 2); C3D4 plates cut in z at planes of 5 x 17, 2 x 43 and 9 x 19 nodes: 255 / 258 / 513.
2. local and global counts on different sides of 256 -- three and four slabs of a CPS4 plate whose cuts hold 64 nodes: 128
   local slots on the end ranks, 256 on the middle ones, 256 / 384 global; the end ranks leave hole slots.
3. multiplicity -- a 2 x 2 checkerboard of a CPS4 plate (centre node shared by 4), the 2 x 2 x 2 octants of a C3D4 plate (centre by
   8, edge lines by 4, faces by 2), fans of 3 / 5 / 8 CPS3 triangles with one triangle per rank: the hub on every rank, every node
   of every rank on the interface (the interior half of the split product empty), the last rank owns nothing.
4. degenerate ranks -- two disjoint CPS4 plates, ranks 0 and 1 on the first, rank 2 alone on the second (no interface, no
   neighbour); a 1-rank communicator without interface.
5. odd local n -- two z-slabs of a C3D4 plate with 27 nodes, 81 DOFs each (the octants likewise): n2 = 41 and owner[2 i + 1]
   reads the pad; the last local node is owned and non-zero in every vector.
6. first and last local DOF on the interface: the fans.

Checks: iface_sums() a, b; product() c; reductions() d; dirichlet() e; pcg() f; loads() g, each under OPT_EXCHANGE 0 and 1,
the solves under OPT_OVERLAP 0 and 1 as well.  One device run per case (device_run) feeds them all; every comparison happens on
the main thread, so a failed assertion leaves no rank at a rendezvous.

Bounds.  Checks a, b, the ownership diagonal of e, every maximum and every "same bits on all ranks" are exact.  For the rest
the float64 restatement (tests/rank_reference.py) against its long-double twin on these very cases (measure_f64_worst, asserted
by the CPU file) gives the constants F64_WORST_RANK_*; the device is held to 4 x that, the margin of the earlier shape suites
for a different but equally valid summation order.  Each twin assembles its sub-matrices from the coordinates in its own dtype
(rr.assemble), so the float64 one carries the rounding of an assembly as a backend's matrix does; those constants are kept per
element family.  The product and the linear elimination are compared with the long-double product of the oracle's global
matrix, which the CPU file holds to the same 4 x against the long-double twin; the iterates with the long-double twin.  Errors
are relative to the largest entry of the reference; max|r| after k iterations is measured against r0, since on the fans the
recurrence has converged by then and max|r| itself is rounding."""
import functools
import threading

import numpy as np

from femcy_amd import backend as be, meshgen, partition
from oracle import femcy_oracle as orc
from oracle.elements import elem_def

import loads_reference as lr
import post_reference as pr
import rank_reference as rr
import thermal_cases as tc
import thermal_reference as tr
from helpers import oracle_material

LD = np.longdouble
PERTURB = 0.0                                                          # straight cells (distorted elements are asm_shapes.py's subject)
CELL = 0.25
MAX_RANKS = 8
BS = 256                                                               # workgroup of the pack / unpack / sum kernels

# worst error of the float64 restatement against the long-double one on the cases of this file (measure_f64_worst, as measured).
# What goes through the matrix is kept per element family: the twins assemble in their own dtype, and the four-point CPS4
# assembly rounds an order of magnitude more than the one-point C3D4 and CPS3 ones
F64_WORST_RANK_SPMV = {"CPS4": 9.3e-15, "C3D4": 2.2e-15, "CPS3": 3.1e-16}
F64_WORST_RANK_SPMV_SMOOTH = {"CPS4": 1.3e-13, "C3D4": 5.4e-14, "CPS3": 1.1e-15}    # K times a smooth field nearly cancels
F64_WORST_RANK_DIRICHLET = {"CPS4": 8.7e-15, "C3D4": 1.8e-16, "CPS3": 3.2e-16}
F64_WORST_RANK_PCG_X = {"CPS4": 5.9e-15, "C3D4": 8.4e-16, "CPS3": 4.1e-16}
F64_WORST_RANK_PCG_RMAX = {"CPS4": 2.5e-15, "C3D4": 5.5e-16, "CPS3": 1.6e-16}
F64_WORST_RANK_NORM = 1.5e-16
F64_WORST_RANK_NEUMANN = 1.3e-16
F64_WORST_RANK_BODY = 1.2e-15
F64_WORST_RANK_ENERGY = 4.3e-15
F64_WORST = {"spmv": F64_WORST_RANK_SPMV, "spmv_smooth": F64_WORST_RANK_SPMV_SMOOTH, "norm": F64_WORST_RANK_NORM,
             "dirichlet": F64_WORST_RANK_DIRICHLET, "pcg_x": F64_WORST_RANK_PCG_X, "pcg_rmax": F64_WORST_RANK_PCG_RMAX,
             "neumann": F64_WORST_RANK_NEUMANN, "body": F64_WORST_RANK_BODY, "energy": F64_WORST_RANK_ENERGY}
FAMILIES = ("CPS4", "C3D4", "CPS3")


def worst_of(key, family):
    """the constant of `key` for a case of `family`"""
    v = F64_WORST[key]
    return v[family] if isinstance(v, dict) else v


# name -> (mesh, split, ranks, claims): niface_local and nb_ptr[-1] per rank, niface_global, the largest sharing multiplicity
CASES = {
    "edge2d-127": (("CPS4", (2, 126)), "x", 2, dict(local=[254, 254], glob=254, nb=[254, 254], mult=2)),
    "edge2d-128": (("CPS4", (2, 127)), "x", 2, dict(local=[256, 256], glob=256, nb=[256, 256], mult=2)),
    "edge2d-129": (("CPS4", (2, 128)), "x", 2, dict(local=[258, 258], glob=258, nb=[258, 258], mult=2)),
    "edge3d-85": (("C3D4", (4, 16, 2)), "z", 2, dict(local=[255, 255], glob=255, nb=[255, 255], mult=2)),
    "edge3d-86": (("C3D4", (1, 42, 2)), "z", 2, dict(local=[258, 258], glob=258, nb=[258, 258], mult=2)),
    "edge3d-171": (("C3D4", (8, 18, 2)), "z", 2, dict(local=[513, 513], glob=513, nb=[513, 513], mult=2)),
    "slabs-3": (("CPS4", (6, 63)), "x", 3, dict(local=[128, 256, 128], glob=256, nb=[128, 256, 128], mult=2, holes=True)),
    "slabs-4": (("CPS4", (8, 63)), "x", 4, dict(local=[128, 256, 256, 128], glob=384, nb=[128, 256, 256, 128], mult=2, holes=True)),
    "checker": (("CPS4", (12, 10)), "xy", 4, dict(local=[24] * 4, glob=46, nb=[28] * 4, mult=4, holes=True)),
    "octants": (("C3D4", (4, 4, 4)), "xyz", 8, dict(local=[57] * 8, glob=183, nb=[111] * 8, mult=8, holes=True, odd=True)),
    "fan-3": (("fan", 3), "element", 3, dict(local=[6] * 3, glob=8, nb=[8] * 3, mult=3, holes=True, owns_nothing=True)),
    "fan-5": (("fan", 5), "element", 5, dict(local=[6] * 5, glob=12, nb=[12] * 5, mult=5, holes=True, owns_nothing=True)),
    "fan-8": (("fan", 8), "element", 8, dict(local=[6] * 8, glob=18, nb=[18] * 8, mult=8, holes=True, owns_nothing=True)),
    "islands": (("islands", ((8, 6), (5, 4))), "islands", 3, dict(local=[14, 14, 0], glob=14, nb=[14, 14, 0], mult=2, holes=True,
                                                                  empty=True)),
    "single": (("CPS4", (9, 7)), "x", 1, dict(local=[0], glob=0, nb=[0], mult=1, empty=True)),
    "odd3d": (("C3D4", (2, 2, 4)), "z", 2, dict(local=[27, 27], glob=27, nb=[27, 27], mult=2, odd=True)),
}
FANS = ("fan-3", "fan-5", "fan-8")
LOAD_CASES = ("checker", "octants")
MULTIPLICITY_CASES = ("checker", "octants") + FANS
PCG_ITERS = (1, 3, 9)
MODES = ((0, 0), (0, 1), (1, 0), (1, 1))                              # (OPT_EXCHANGE, OPT_OVERLAP)
SOLVE_EPS = 1e-10
SOLVE_BOUND = 1e-9                                                     # 10 x the stopping rule: recurrence residual against the true one
TRACTION = -2.5
DIRECTION = np.array([0.6, -0.3, 0.74])
BODY = np.array([0.7, -1.3, 2.1])
DISP_SCALE = 0.002


class Case:
    pass


def _plate(family, cells, perturb):
    """lr.mesh with cells of equal sides (CELL): the long thin plates of the block-edge cases keep well-shaped elements"""
    if family == "CPS4":
        nodes, el = lr.grid2d(*cells, size=(CELL * cells[0], CELL * cells[1]), perturb=perturb, seed=3)
        return nodes, el, lr.Element_linear_quadrilateral()
    assert family == "C3D4"
    box = tuple(CELL * k for k in cells)
    return meshgen.plate_hex(*cells, perturb=perturb, seed=3, box=box)[0], meshgen.plate_grid(*cells, box=box)[1], lr.Element_linear_tetrahedral()


def _cells_of(flat, el, cells):
    """integer cell coordinates of every element of a structured plate (from the unperturbed nodes)"""
    cen = flat[el].mean(axis=1)
    lo, ext = flat.min(axis=0), np.ptp(flat, axis=0)
    return np.minimum((np.asarray(cells) * (cen - lo) / ext).astype(np.int64), np.asarray(cells) - 1)


@functools.lru_cache(maxsize=None)
def case(name):
    (family, arg), split, nranks, claims = CASES[name]
    c = Case()
    if family == "fan":
        nodes, el, ELE = lr.fan(arg)
        rank_of = np.arange(arg, dtype=np.int32)
        family = "CPS3"
    elif family == "islands":
        (na, ea, ELE), (nb, eb, _) = (_plate("CPS4", cl, PERTURB) for cl in arg)
        flat = _plate("CPS4", arg[0], 0.0)[0]
        left = _cells_of(flat, ea, arg[0])[:, 0] * 2 // arg[0][0]
        nodes = np.vstack([na, nb + np.array([5.0, 0.0])])
        el = np.vstack([ea, eb + len(na)])
        rank_of = np.concatenate([left, np.full(len(eb), 2)]).astype(np.int32)
        family = "CPS4"
    else:
        nodes, el, ELE = _plate(family, arg, PERTURB)
        ijk = _cells_of(_plate(family, arg, 0.0)[0], el, arg)
        if split in ("x", "z"):
            ax = 0 if split == "x" else 2
            rank_of = ijk[:, ax] * nranks // arg[ax]
        else:                                                          # the sign about the centre on each axis
            rank_of = sum((2 * ijk[:, a] >= arg[a]).astype(np.int64) << a for a in range(len(split)))
        rank_of = rank_of.astype(np.int32)
    c.name, c.family, c.ELE, c.nranks, c.claims = name, family, ELE, nranks, claims
    c.nodes = np.ascontiguousarray(nodes, dtype=np.float64)
    c.el = np.ascontiguousarray(el, dtype=np.int32)
    c.nodes.setflags(write=False)
    c.rank_of = rank_of
    c.dm = c.nodes.shape[1]
    c.nn, c.n = len(c.nodes), c.nodes.size
    c.mat = tc.material(tr.LIN3D if c.dm == 3 else tr.PSTRESS)
    c.kind = pr.LIN3D if c.dm == 3 else pr.PSTRESS
    c.parts = [partition.build_part(c.nodes, c.el, nranks, r, rank_of=rank_of) for r in range(nranks)]
    c.touched = partition._sharing(c.el, rank_of, c.nn, nranks)
    c.mult = c.touched.sum(axis=1)
    c.gd = [rr.gdofs(p) for p in c.parts]
    c.hub = int(np.argmax(c.mult)) if nranks > 1 else c.nn // 2       # the most-shared node (1 rank: any node)
    _constraints(c)
    _vectors(c)
    return c


def _constraints(c):
    """e / f: the most-shared node, the first shared node of every pair of neighbours (all components) and the last one (its
    first component), every fifth interior node.  The linear elimination: the last node(s) of the lowest multiplicity on the
    highest rank that holds one -- interior, so one rank alone lists them, except on the fans, which have no interior."""
    dm = c.dm
    dofs = set(c.hub * dm + i for i in range(dm))
    for r in range(c.nranks):
        for q in range(r + 1, c.nranks):
            shared = np.nonzero(c.touched[:, r] & c.touched[:, q])[0]
            if shared.size:
                dofs.update(int(shared[0]) * dm + i for i in range(dm))
                dofs.add(int(shared[-1]) * dm)
    for a in np.nonzero(c.mult == 1)[0][::5]:
        dofs.update(int(a) * dm + i for i in range(dm))
    c.cons = np.array(sorted(dofs), dtype=np.int64)
    low = np.nonzero(c.mult == c.mult.min())[0]
    holder = max(r for r in range(c.nranks) if c.touched[low, r].any())
    mine = low[c.touched[low, holder]]
    c.lin_nodes = mine[-3:] if c.mult.min() == 1 else mine[-1:]
    c.lin_dofs = (c.lin_nodes[:, None] * dm + np.arange(dm)[None, :]).ravel()
    c.lin_vals = 0.01 * (1.0 + np.arange(c.lin_dofs.size)) * np.where(np.arange(c.lin_dofs.size) % 2, -1.0, 1.0)


def _vectors(c):
    """consistent global vectors: non-zero in every entry (the last local node of every rank carries a signal)"""
    rng = np.random.default_rng(len(c.name) + c.n)
    x = c.nodes / np.ptp(c.nodes, axis=0).max()
    phase = x @ np.array([1.3, 0.7, 0.45])[:c.dm]
    smooth = np.stack([1.5 + np.sin(phase + 0.4), 1.25 + np.cos(2.1 * phase - 0.2), 1.75 + np.sin(0.6 * phase + 1.0)][:c.dm], axis=1)
    V = {"smooth": smooth.ravel(), "u": DISP_SCALE * np.ptp(c.nodes, axis=0).max() * smooth.ravel()}
    for key in ("random", "b", "rhs", "base"):
        V[key] = rng.standard_normal(c.n) + 0.0
    V["b"][c.cons] = 0.0                                               # what femcy_apply_dirichlet_newton leaves
    hub_dof = c.hub * c.dm
    V["single"] = np.zeros(c.n)
    V["single"][hub_dof] = -3.5
    V["big"] = rng.uniform(-1.0, 1.0, c.n)
    V["big"][hub_dof] = -(2.0 * np.abs(np.delete(V["big"], hub_dof)).max() + 1.0)
    for v in V.values():
        v.setflags(write=False)
    c.V = V


def local_vectors(c, r):
    """a, b: per-rank vectors that differ from rank to rank.  Integers below 2^20 from (rank, global DOF, component) -- eight of
    them sum below 2^23, exactly; standard-normal numbers without negative zeros"""
    gd = c.gd[r]
    ints = ((r + 1) * 104729 + (gd // c.dm) * 7919 + (gd % c.dm) * 611953) % (1 << 20)
    rnd = np.random.default_rng(1000 * c.n + r).standard_normal(gd.size) + 0.0
    return ints.astype(np.float64), rnd


def case_table(name):
    """the table's own claims, and the partition invariants of tests/test_distributed_cpu.py -> the claims"""
    c = case(name)
    cl = c.claims
    P = c.parts
    assert c.nranks <= MAX_RANKS and sorted(np.concatenate([p.elem_ids for p in P]).tolist()) == list(range(len(c.el)))
    assert [p.iface_local_dofs.size for p in P] == cl["local"] and all(p.niface_global == cl["glob"] for p in P)
    assert [int(p.nb_ptr[-1]) for p in P] == cl["nb"] and int(c.mult.max()) == cl["mult"]
    assert any(p.iface_local_dofs.size < p.niface_global for p in P) == bool(cl.get("holes"))
    assert any(p.iface_local_dofs.size == 0 and p.nb_ranks.size == 0 for p in P) == bool(cl.get("empty"))
    assert any(not p.owner.any() for p in P) == bool(cl.get("owns_nothing"))
    assert any(p.n_local % 2 for p in P) == bool(cl.get("odd"))
    owners = np.zeros(c.n, dtype=int)
    slot_to_gdof = {}
    for p, gd in zip(P, c.gd):
        assert np.array_equal(c.nodes[p.l2g], p.nodes) and np.array_equal(p.l2g[p.elements], c.el[p.elem_ids])
        owners[gd] += p.owner
        for ld, sl in zip(p.iface_local_dofs, p.iface_global_slot):
            assert slot_to_gdof.setdefault(int(sl), int(gd[ld])) == int(gd[ld])
        assert list(p.nb_ranks) == sorted(p.nb_ranks) and p.rank not in p.nb_ranks and p.nb_ptr[0] == 0
        union = set()
        for k, q in enumerate(p.nb_ranks):
            mine = gd[p.nb_dofs[p.nb_ptr[k]:p.nb_ptr[k + 1]]]
            ko = list(P[q].nb_ranks).index(p.rank)
            theirs = c.gd[q][P[q].nb_dofs[P[q].nb_ptr[ko]:P[q].nb_ptr[ko + 1]]]
            assert mine.size and np.all(np.diff(mine) > 0) and np.array_equal(mine, theirs)
            union.update(p.nb_dofs[p.nb_ptr[k]:p.nb_ptr[k + 1]].tolist())
        assert union == set(p.iface_local_dofs.tolist())
        if p.owner.any():                                              # the last local node: owned wherever the rank owns anything at its end
            assert p.owner[-1] or name in FANS
    assert (owners == 1).all() and len(slot_to_gdof) == cl["glob"] and len(set(slot_to_gdof.values())) == cl["glob"]
    # the edges the case names
    if name.startswith("edge"):
        assert cl["glob"] in (BS - 2, BS - 1, BS, BS + 2, 2 * BS + 1) and cl["glob"] == c.dm * int(name.split("-")[1])
    if name.startswith("slabs"):
        assert cl["local"][0] == BS // 2 and cl["local"][1] == BS and cl["glob"] in (BS, BS + BS // 2)
    if name in FANS:                                                   # 6. first and last local DOF on the interface; all slices interface slices
        for p in P:
            assert p.iface_local_dofs[0] == 0 and p.iface_local_dofs[-1] == p.n_local - 1 == p.iface_local_dofs.size - 1
        assert not P[-1].owner.any() and c.mult[c.hub] == c.nranks
    if name == "octants":
        assert sorted(set(c.mult.tolist())) == [1, 2, 4, 8] and (c.mult == 8).sum() == 1
    if name == "checker":
        assert sorted(set(c.mult.tolist())) == [1, 2, 4] and (c.mult == 4).sum() == 1
    if cl.get("odd"):
        odd = [p for p in P if p.n_local % 2]
        assert all(p.owner[-1] and all(abs(c.V[k][gd[-1]]) > 0 for k in ("smooth", "random", "u", "base")) for p, gd in zip(P, c.gd) if p in odd)
    # d: the largest entry is at least twice every other and sits where all sharing ranks but one do not own it
    big, hd = c.V["big"], c.hub * c.dm
    assert abs(big[hd]) >= 2.0 * np.abs(np.delete(big, hd)).max()
    if c.nranks > 1:
        assert sum(1 for p, gd in zip(P, c.gd) if hd in gd and not p.owner[list(gd).index(hd)]) == c.mult[c.hub] - 1 >= 1
    # e: the constrained set holds the most-shared node and a node of every cut; the linear set is held as the docstring says
    for r in range(c.nranks):
        for q in range(r + 1, c.nranks):
            shared = c.touched[:, r] & c.touched[:, q]
            assert not shared.any() or shared[c.cons // c.dm].any()
    holders = [r for r in range(c.nranks) if c.touched[c.lin_nodes, r].any()]
    assert len(holders) == (1 if name not in FANS else 2) and (c.nranks == 1 or len(holders) < c.nranks)
    return cl


# ------------------------------------------------------------------------------------------------------- references
@functools.lru_cache(maxsize=None)
def local_K(name, deformed):
    """the oracle's sub-assembled matrix of every rank, and the global one"""
    c = case(name)
    ed = elem_def(c.family)
    C = oracle_material(c.mat).C
    u = c.V["u"] if deformed else np.zeros(c.n)
    Ks = [orc.assemble_K(orc.Topology(p.nodes, p.elements, ed), p.scatter_global(u), C) for p in c.parts]
    return Ks, orc.assemble_K(orc.Topology(c.nodes, c.el, ed), u, C)


@functools.lru_cache(maxsize=None)
def twin_K(name, deformed, dtype):
    """the sub-assembled matrix of every rank from its coordinates (rr.assemble), every step in `dtype`"""
    c = case(name)
    C = oracle_material(c.mat).C
    u = c.V["u"] if deformed else np.zeros(c.n)
    return [rr.assemble(p.nodes, p.elements, c.ELE, C, p.scatter_global(u), dtype) for p in c.parts]


def _scatter(c, v):
    return [np.asarray(v)[gd] for gd in c.gd]


def _rel(got, want):
    size = np.abs(want).max()
    return float(np.abs(np.asarray(got, dtype=LD) - want).max() / (size if size > 0 else 1.0))


@functools.lru_cache(maxsize=None)
def reference_product(name, deformed, which):
    """-> (the long-double product with the oracle's global K, {dtype: the partitioned product per rank, assembled and
    multiplied in the dtype})"""
    c = case(name)
    K = local_K(name, deformed)[1]
    twins = {dt: rr.product(c.parts, twin_K(name, deformed, dt), _scatter(c, c.V[which]), dt) for dt in (LD, np.float64)}
    return rr.csr_matvec(K, c.V[which], LD), twins


@functools.lru_cache(maxsize=None)
def constrained_K(name):
    c = case(name)
    Ks, K = local_K(name, False)
    out = []
    for p, gd, Kr in zip(c.parts, c.gd, Ks):
        out.append(rr.constrain(Kr, np.nonzero(np.isin(gd, c.cons))[0], p.owner))
    return out, orc._zero_rows_cols_unit_diag(K, c.cons)


def lin_lists(c):
    dofs = [np.nonzero(np.isin(gd, c.lin_dofs))[0].astype(np.int32) for gd in c.gd]
    vals = [c.lin_vals[np.searchsorted(c.lin_dofs, gd[d])] for gd, d in zip(c.gd, dofs)]
    return dofs, vals


@functools.lru_cache(maxsize=None)
def reference_linear(name):
    """-> (long-double rhs - K s with the oracle's global K, prescribed values put in; {dtype: the partitioned restatement})"""
    c = case(name)
    K = local_K(name, False)[1]
    s = np.zeros(c.n, dtype=LD)
    s[c.lin_dofs] = c.lin_vals
    want = c.V["rhs"].astype(LD) - rr.csr_matvec(K, s, LD)
    want[c.lin_dofs] = c.lin_vals
    dofs, vals = lin_lists(c)
    return want, {dt: rr.dirichlet_linear(c.parts, twin_K(name, False, dt), _scatter(c, c.V["rhs"]), dofs, vals, dt) for dt in (LD, np.float64)}


@functools.lru_cache(maxsize=None)
def reference_pcg(name, k):
    c = case(name)
    b = _scatter(c, c.V["b"])
    out = {}
    for dt in (LD, np.float64):
        Kc = [rr.constrain_csr(K, np.nonzero(np.isin(gd, c.cons))[0], p.owner) for p, gd, K in zip(c.parts, c.gd, twin_K(name, False, dt))]
        out[dt] = rr.pcg(c.parts, Kc, b, k, dt)
    return out


def _top_facets(c, nodes, el):
    nfn = c.dm
    keys = c.ELE.facet_tables(nfn)["ft_nodes"]
    top = nodes[:, -1] > c.nodes[:, -1].max() - 1e-12
    le, lf = [], []
    for k, key in enumerate(keys):
        e = np.nonzero(top[el[:, key]].all(axis=1))[0]
        le.append(e)
        lf.append(np.full(len(e), k))
    le, lf = np.concatenate(le), np.concatenate(lf)
    order = np.lexsort((lf, le))
    return le[order].astype(np.int32), lf[order].astype(np.int32), nfn


@functools.lru_cache(maxsize=None)
def reference_loads(name):
    """-> {"neumann" / "body" / "energy": (long double of the global mesh, float64 partitioned restatement)}"""
    c = case(name)
    d = DIRECTION[:c.dm]
    le, lf, nfn = _top_facets(c, c.nodes, c.el)
    assert len(le) and (c.mult[np.unique(c.el[le])] > 1).any()          # the loaded surface crosses a cut
    out = {}
    loc = [pr.neumann(p.nodes, p.elements, c.ELE, *_top_facets(c, p.nodes, p.elements), TRACTION, d, np.float64)[0] for p in c.parts]
    out["neumann"] = (pr.neumann(c.nodes, c.el, c.ELE, le, lf, nfn, TRACTION, d, LD)[0], rr.iface_sum(c.parts, loc, np.float64))
    b = BODY[:c.dm]
    loc = [(rr.body_weights(p.nodes, p.elements, c.ELE, np.float64)[:, None] * b[None, :]).ravel() for p in c.parts]
    out["body"] = ((rr.body_weights(c.nodes, c.el, c.ELE, LD)[:, None] * b.astype(LD)[None, :]).ravel(), rr.iface_sum(c.parts, loc, np.float64))
    e64 = np.float64(0)
    for p in c.parts:
        e64 = e64 + rr.energy_total(p.nodes, p.elements, c.ELE, c.kind, c.mat, p.scatter_global(c.V["u"]), np.float64)
    out["energy"] = (rr.energy_total(c.nodes, c.el, c.ELE, c.kind, c.mat, c.V["u"], LD), e64)
    return out


def reference_conditions(name):
    """CPU reference alone: the partitioned restatements agree with the global ones; replicas of the restatement are equal;
    every shared DOF counts once.  -> the float64 errors of this case, by constant"""
    c = case(name)
    fig = dict.fromkeys(F64_WORST, 0.0)
    held = rr.sharing(c.parts, c.n)
    assert np.array_equal(held.sum(axis=1), np.repeat(c.mult, c.dm))
    # a: the exact sum over the sharing ranks
    ints = [local_vectors(c, r)[0] for r in range(c.nranks)]
    total = np.zeros(c.n)
    for gd, v in zip(c.gd, ints):
        total[gd] += v
    assert total.max() < 2 ** 23
    for p, gd, v, w in zip(c.parts, c.gd, ints, rr.iface_sum(c.parts, ints, np.float64)):
        on = np.zeros(p.n_local, dtype=bool)
        on[p.iface_local_dofs] = True
        assert np.array_equal(w[on], total[gd][on]) and np.array_equal(w[~on], v[~on])
    # c
    for deformed in (False, True):
        for which in ("smooth", "random"):
            want, twins = reference_product(name, deformed, which)
            key = "spmv_smooth" if which == "smooth" else "spmv"
            for gd, y, yl in zip(c.gd, twins[np.float64], twins[LD]):
                fig[key] = max(fig[key], float(np.abs(y - yl).max() / np.abs(want).max()))
                # the issue's reference, a float64 assembly itself, is held to what a backend is
                assert float(np.abs(yl - want[gd]).max() / np.abs(want).max()) <= 4.0 * worst_of(key, c.family), (name, deformed, which)
    # d
    for which in ("random", "single", "big"):
        v = c.V[which]
        want = np.sqrt((v.astype(LD) ** 2).sum() / LD(c.n))
        fig["norm"] = max(fig["norm"], float(abs(rr.norm(c.parts, _scatter(c, v), c.n, np.float64) - want) / want))
        assert rr.absmax(c.parts, _scatter(c, v)) == np.abs(v).max()
    # e
    want, twins = reference_linear(name)
    assert np.abs(rr.csr_matvec(local_K(name, False)[1], want - c.V["rhs"].astype(LD), LD)).max() > 0
    for gd, y, yl in zip(c.gd, twins[np.float64], twins[LD]):
        fig["dirichlet"] = max(fig["dirichlet"], float(np.abs(y - yl).max() / np.abs(want).max()))
        assert float(np.abs(yl - want[gd]).max() / np.abs(want).max()) <= 4.0 * worst_of("dirichlet", c.family), name
    Kc, Kg = constrained_K(name)
    import scipy.sparse as sp
    acc = sp.csr_matrix((c.n, c.n))
    for gd, Kr in zip(c.gd, Kc):
        Kr = Kr.tocoo()
        acc = acc + sp.coo_matrix((Kr.data, (gd[Kr.row], gd[Kr.col])), shape=(c.n, c.n)).tocsr()
    assert abs(acc - Kg).max() <= 1e-12 * abs(Kg).max() and np.array_equal(acc.diagonal()[c.cons], np.ones(c.cons.size))
    # f
    for k in PCG_ITERS:
        ref = reference_pcg(name, k)
        (xl, r0l, rml), (xd, r0d, rmd) = ref[LD], ref[np.float64]
        assert r0l == r0d == np.abs(c.V["b"]).max() > 0
        size = max(float(np.abs(x).max()) for x in xl)
        fig["pcg_x"] = max([fig["pcg_x"]] + [float(np.abs(a - b).max()) / size for a, b in zip(xd, xl)])
        fig["pcg_rmax"] = max(fig["pcg_rmax"], abs(rmd - rml) / r0l)
        glob = {}
        for gd, x in zip(c.gd, xd):                                    # replicas of the restatement are the same numbers
            for g, v in zip(gd, x):
                assert glob.setdefault(int(g), v) == v
    # g
    if name in LOAD_CASES:
        refs = reference_loads(name)
        for key in ("neumann", "body"):
            want, got = refs[key]
            assert np.abs(want).max() > 0
            for gd, y in zip(c.gd, got):
                fig[key] = max(fig[key], float(np.abs(y - want[gd]).max() / np.abs(want).max()))
        want, got = refs["energy"]
        fig["energy"] = float(abs(got - want) / want)
    return fig


def measure_f64_worst():
    """-> {(key, family or None): the worst figure}, in the shape of the constants"""
    worst = {}
    for name in CASES:
        for key, v in reference_conditions(name).items():
            k = (key, case(name).family if isinstance(F64_WORST[key], dict) else None)
            worst[k] = max(worst.get(k, 0.0), v)
    return worst


# ----------------------------------------------------------------------------------------------------------- runner
def run_ranks(parts, ELE, mat, fn, timeout=150.0):
    """fn(ctx, part) on one thread and one context per rank, joined by the in-process transport; the contexts are closed in a
    finally; -> the ranks' results.  A rank still running after `timeout` fails the call; the first error is raised here."""
    nranks = len(parts)
    uid = be.Context.comm_local_id()
    out, err = [None] * nranks, []

    def work(r):
        ctx = None
        try:
            p = parts[r]
            ctx = be.Context(0)
            ctx.set_mesh(p.nodes, p.elements)
            ctx.set_element(ELE)
            ctx.set_material(mat)
            ctx.build_pattern()
            ctx.comm_init(p.rank, p.nranks, uid, p.iface_local_dofs, p.iface_global_slot, p.niface_global, p.owner)
            ctx.comm_set_neighbours(p)
            out[r] = fn(ctx, p)
        except BaseException as e:                                     # noqa: BLE001 - reported below
            err.append((r, e))
        finally:
            if ctx is not None:
                ctx.close()

    threads = [threading.Thread(target=work, args=(r,), daemon=True) for r in range(nranks)]
    for t in threads:
        t.start()
    for t in threads:
        t.join(timeout=timeout)
    assert not any(t.is_alive() for t in threads), "a rank is still running"
    if err:
        raise err[0][1]
    return out


def _program(c, ctx, p):
    """everything one rank computes for the checks below, as plain arrays"""
    r, V, dm = p.rank, c.V, c.dm
    gd = c.gd[r]
    sc = p.scatter_global
    cons = np.nonzero(np.isin(gd, c.cons))[0].astype(np.int32)
    ldofs, lvals = (x[r] for x in lin_lists(c))
    o = {"n_global": ctx.comm_info()[2]}
    t0 = ctx.timing()
    nsolves = 0
    for ex in (0, 1):
        ctx.set_option(be.OPT_EXCHANGE, ex)
        for key, v in zip(("int", "rnd"), local_vectors(c, r)):        # a, b
            ctx.upload(be.VEC_TMP0, v)
            ctx.iface_sum(be.VEC_TMP0)
            o[key, ex] = ctx.download(be.VEC_TMP0)
        for deformed in (False, True):                                 # c
            if deformed:
                ctx.upload(be.VEC_DOF, sc(V["u"]))
            ctx.assemble_K(be.VEC_DOF if deformed else -1)
            for which in ("smooth", "random"):
                ctx.upload(be.VEC_TMP0, sc(V[which]))
                ctx.spmv(be.VEC_TMP0, be.VEC_TMP1)
                o["y", deformed, which, ex] = ctx.download(be.VEC_TMP1)
        for which in ("random", "single", "big"):                      # d
            ctx.upload(be.VEC_TMP0, sc(V[which]))
            o["norm", which, ex] = ctx.vec_norm(be.VEC_TMP0)
            o["absmax", which, ex] = ctx.vec_absmax(be.VEC_TMP0)
        ctx.assemble_K(-1)                                             # e, the Newton variant
        ctx.upload(be.VEC_RESIDUAL, sc(V["random"]))
        ctx.dirichlet_newton(cons, be.VEC_RESIDUAL)
        o["newton_K", ex] = ctx.get_K_bsr().tocsr()
        o["newton_r", ex] = ctx.download(be.VEC_RESIDUAL)
        ctx.upload(be.VEC_RESIDUAL, sc(V["b"]))                        # f, on that matrix
        for ov in (0, 1):
            ctx.set_option(be.OPT_OVERLAP, ov)
            for k in PCG_ITERS:
                o["pcg", k, ex, ov] = (ctx.pcg(be.VEC_RESIDUAL, be.VEC_X, eps=0.0, maxit=k), ctx.download(be.VEC_X))
                nsolves += 1
        if ex == 0:
            o["solve"] = (ctx.pcg(be.VEC_RESIDUAL, be.VEC_X, eps=SOLVE_EPS), ctx.download(be.VEC_X))
            nsolves += 1
        ctx.assemble_K(-1)                                             # e, the linear variant: collective, k == 0 on most ranks
        ctx.upload(be.VEC_RHS, sc(V["rhs"]))
        ctx.dirichlet_linear(ldofs, lvals, be.VEC_RHS)
        o["linear_K", ex] = ctx.get_K_bsr().tocsr()
        o["linear_rhs", ex] = ctx.download(be.VEC_RHS)
        if c.name in LOAD_CASES:                                       # g
            le, lf, nfn = _top_facets(c, p.nodes, p.elements)
            ls = ctx.loadset(c.ELE, le, lf, nfn)
            bl = ctx.bodyload(c.ELE, None)
            for key, call in (("neumann", lambda add: ctx.loadset_neumann(ls, TRACTION, DIRECTION[:dm], be.VEC_RHS, add=add)),
                              ("body", lambda add: ctx.bodyload_apply(bl, BODY[:dm], be.VEC_RHS, add=add))):
                ctx.vector(be.VEC_RHS).fill(np.nan)
                call(False)
                o[key, ex] = ctx.download(be.VEC_RHS)
                ctx.upload(be.VEC_RHS, sc(V["base"]))
                call(True)
                o[key + "_add", ex] = ctx.download(be.VEC_RHS)
            refused = []
            for call in (lambda: ctx.loadset_neumann(ls, TRACTION, DIRECTION[:dm], be.VEC_TMP1, add=True),
                         lambda: ctx.bodyload_apply(bl, BODY[:dm], be.VEC_TMP1, add=True)):
                try:
                    call()
                    refused.append(None)
                except be.FemcyError as e:
                    refused.append(str(e))
            o["refused", ex] = refused
            ctx.assemble_K(-1)                                         # the weights det J w of the undeformed mesh
            ctx.upload(be.VEC_DOF, sc(V["u"]))
            o["energy", ex] = ctx.elastic_energy(be.VEC_DOF)
    t1 = ctx.timing()
    o["solves"] = (nsolves, t1["solves_three"] - t0["solves_three"], t1["solves_persist"] - t0["solves_persist"],
                   t1["solves_small"] - t0["solves_small"])
    return o


_RUNS = {}


def device_run(name, backend):
    """one run per case, shared by its checks (a failure is kept and raised again, not repeated)"""
    assert backend == "hip", "the host backend has no communicator"
    if name not in _RUNS:
        c = case(name)
        try:
            _RUNS[name] = run_ranks(c.parts, c.ELE, c.mat, lambda ctx, p: _program(c, ctx, p))
        except BaseException as e:                                     # noqa: BLE001
            _RUNS[name] = e
    if isinstance(_RUNS[name], BaseException):
        raise _RUNS[name]
    return _RUNS[name]


def _bits(a, b):
    return np.array_equal(np.ascontiguousarray(a, dtype=np.float64).view(np.uint64), np.ascontiguousarray(b, dtype=np.float64).view(np.uint64))


def _replicas_equal(c, vecs):
    glob = np.full(c.n, np.nan)
    seen = np.zeros(c.n, dtype=bool)
    for gd, v in zip(c.gd, vecs):
        old = seen[gd]
        if not _bits(glob[gd][old], v[old]):
            return False
        glob[gd] = v
        seen[gd] = True
    return bool(seen.all())


# ----------------------------------------------------------------------------------------------------------- checks
def iface_sums(name, backend):
    """a, b -> the number of interface entries compared"""
    c = case(name)
    outs = device_run(name, backend)
    ints = [local_vectors(c, r)[0] for r in range(c.nranks)]
    rnds = [local_vectors(c, r)[1] for r in range(c.nranks)]
    total = np.zeros(c.n)
    for gd, v in zip(c.gd, ints):
        total[gd] += v
    want_rnd = rr.iface_sum(c.parts, rnds, np.float64)
    count = 0
    for ex in (0, 1):
        for p, gd, o, vi, vr, wr in zip(c.parts, c.gd, outs, ints, rnds, want_rnd):
            on = np.zeros(p.n_local, dtype=bool)
            on[p.iface_local_dofs] = True
            got = o["int", ex]
            assert np.array_equal(got[on], total[gd][on]), (name, ex, p.rank)          # slots a rank does not hold added nothing
            assert np.array_equal(got[~on], vi[~on]), (name, ex, p.rank)
            assert _bits(o["rnd", ex], wr), (name, ex, p.rank, int((o["rnd", ex] != wr).sum()))
            assert _bits(wr[~on], vr[~on])
            count += int(on.sum())
        assert _replicas_equal(c, [o["rnd", ex] for o in outs]) or c.nranks == 1
    return count


def product(name, backend):
    c = case(name)
    outs = device_run(name, backend)
    worst = {"smooth": 0.0, "random": 0.0}
    for deformed in (False, True):
        for which in ("smooth", "random"):
            want = reference_product(name, deformed, which)[0]
            for ex in (0, 1):
                ys = [o["y", deformed, which, ex] for o in outs]
                assert _replicas_equal(c, ys), (name, deformed, which, ex)
                for gd, y in zip(c.gd, ys):
                    worst[which] = max(worst[which], float(np.abs(y - want[gd]).max() / np.abs(want).max()))
    print(f"product {name} [{backend}]: smooth {worst['smooth']:.3e}, random {worst['random']:.3e}")
    assert worst["random"] <= 4.0 * worst_of("spmv", c.family) and worst["smooth"] <= 4.0 * worst_of("spmv_smooth", c.family), worst
    return worst


def reductions(name, backend):
    c = case(name)
    outs = device_run(name, backend)
    assert all(o["n_global"] == c.n for o in outs)
    worst = 0.0
    for which in ("random", "single", "big"):
        v = c.V[which]
        want = np.sqrt((v.astype(LD) ** 2).sum() / LD(c.n))
        for ex in (0, 1):
            norms = {o["norm", which, ex] for o in outs}
            maxes = {o["absmax", which, ex] for o in outs}
            assert len(norms) == 1 and maxes == {float(np.abs(v).max())}, (name, which, ex, norms, maxes)
            worst = max(worst, float(abs(norms.pop() - want) / want))
    print(f"reductions {name} [{backend}]: {worst:.3e}")
    assert worst <= 4.0 * F64_WORST_RANK_NORM, worst
    return worst


def _check_constrained(c, outs, key, dofs_global):
    """the sum over ranks of the scattered local matrices: unit diagonal, zero rows and columns; each diagonal = owner[dof]"""
    import scipy.sparse as sp
    acc = sp.csr_matrix((c.n, c.n))
    for p, gd, o in zip(c.parts, c.gd, outs):
        K = o[key].tocoo()
        acc = acc + sp.coo_matrix((K.data, (gd[K.row], gd[K.col])), shape=(c.n, c.n)).tocsr()
        loc = np.nonzero(np.isin(gd, dofs_global))[0]
        assert np.array_equal(o[key].diagonal()[loc], p.owner[loc].astype(np.float64)), (c.name, key, p.rank)
    A = acc.toarray()
    assert np.array_equal(A[dofs_global, dofs_global], np.ones(len(dofs_global)))
    A[dofs_global, dofs_global] = 0.0
    assert not A[dofs_global].any() and not A[:, dofs_global].any(), (c.name, key)
    return acc


def dirichlet(name, backend):
    c = case(name)
    outs = device_run(name, backend)
    want = reference_linear(name)[0]
    free = np.ones(c.n, dtype=bool)
    free[c.cons] = False
    worst = 0.0
    for ex in (0, 1):
        _check_constrained(c, outs, ("newton_K", ex), c.cons)
        for gd, o in zip(c.gd, outs):
            r1 = o["newton_r", ex]
            assert not r1[~free[gd]].any() and _bits(r1[free[gd]], c.V["random"][gd][free[gd]])
        _check_constrained(c, outs, ("linear_K", ex), c.lin_dofs)
        rhs = [o["linear_rhs", ex] for o in outs]
        assert _replicas_equal(c, rhs), (name, ex)
        for gd, y in zip(c.gd, rhs):
            assert np.array_equal(y[np.isin(gd, c.lin_dofs)], want[gd][np.isin(gd, c.lin_dofs)].astype(np.float64))
            worst = max(worst, float(np.abs(y - want[gd]).max() / np.abs(want).max()))
    print(f"dirichlet {name} [{backend}]: {worst:.3e}")
    assert worst <= 4.0 * worst_of("dirichlet", c.family), worst
    return worst


def _pcg_figures(c, ref, results):
    """results: per rank ((iters, r0, rmax), x) -> (error of x, error of max|r| against r0)"""
    xl, r0l, rml = ref
    size = max(float(np.abs(x).max()) for x in xl)
    ex = max(float(np.abs(x - w).max()) / size for (_, x), w in zip(results, xl))
    er = max(float(abs(LD(res[2]) - rml) / r0l) for res, _ in results)
    return ex, er


def pcg(name, backend):
    c = case(name)
    outs = device_run(name, backend)
    nsolves, three, persist, small = outs[0]["solves"]
    assert all(o["solves"] == (nsolves, nsolves, 0, 0) for o in outs), outs[0]["solves"]     # the three-launch collective loop
    wx = wr = 0.0
    for k in PCG_ITERS:
        ref = reference_pcg(name, k)[LD]
        for ex, ov in MODES:
            res = [o["pcg", k, ex, ov] for o in outs]
            assert len({r[0] for r in res}) == 1 and res[0][0][0] == k, (name, k, ex, ov, [r[0] for r in res])
            assert res[0][0][1] == ref[1]                              # r0 = max|b|: exact
            assert _replicas_equal(c, [x for _, x in res]), (name, k, ex, ov)
            a, b = _pcg_figures(c, ref, res)
            wx, wr = max(wx, a), max(wr, b)
    if c.nranks == 1:                                                  # the same bound for a plain single-context solve
        ctx = be.Context(0, backend=backend)
        try:
            for opt in (be.OPT_PCG_SMALL, be.OPT_PCG_PERSIST, be.OPT_PCG_STORAGE_ORDER):
                ctx.set_option(opt, 0)
            ctx.set_mesh(c.nodes, c.el)
            ctx.set_element(c.ELE)
            ctx.set_material(c.mat)
            ctx.build_pattern()
            ctx.assemble_K(-1)
            ctx.upload(be.VEC_RESIDUAL, c.V["b"])
            ctx.dirichlet_newton(c.cons.astype(np.int32), be.VEC_RESIDUAL)
            for k in PCG_ITERS:
                res = [(ctx.pcg(be.VEC_RESIDUAL, be.VEC_X, eps=0.0, maxit=k), ctx.download(be.VEC_X))]
                a, b = _pcg_figures(c, reference_pcg(name, k)[LD], res)
                wx, wr = max(wx, a), max(wr, b)
        finally:
            ctx.close()
    # the converged solve against the oracle's constrained global system
    sol = partition.gather_owned(c.parts, [o["solve"][1] for o in outs], c.n)
    assert _replicas_equal(c, [o["solve"][1] for o in outs]) and len({o["solve"][0] for o in outs}) == 1
    Kg = constrained_K(name)[1]
    resid = float(np.abs(rr.csr_matvec(Kg, sol, LD) - c.V["b"]).max() / np.abs(c.V["b"]).max())
    print(f"pcg {name} [{backend}]: x {wx:.3e}, max|r| / r0 {wr:.3e}, converged residual {resid:.3e} after {outs[0]['solve'][0][0]}")
    assert wx <= 4.0 * worst_of("pcg_x", c.family) and wr <= 4.0 * worst_of("pcg_rmax", c.family), (wx, wr)
    assert resid <= SOLVE_BOUND, resid
    return wx, wr, resid


def loads(name, backend):
    c = case(name)
    outs = device_run(name, backend)
    refs = reference_loads(name)
    fig = {}
    for ex in (0, 1):
        for key, bound in (("neumann", F64_WORST_RANK_NEUMANN), ("body", F64_WORST_RANK_BODY)):
            want = refs[key][0]
            got = [o[key, ex] for o in outs]
            assert _replicas_equal(c, got)
            for gd, o, y in zip(c.gd, outs, got):
                assert np.isfinite(y).all()
                fig[key] = max(fig.get(key, 0.0), float(np.abs(y - want[gd]).max() / np.abs(want).max()))
                assert _bits(o[key + "_add", ex], c.V["base"][gd] + y), (name, key, ex)     # one rounded addition per entry
            assert fig[key] <= 4.0 * bound, (key, fig[key])
        for o in outs:
            assert all(msg and "TMP1" in msg for msg in o["refused", ex]), o["refused", ex]
        energies = {o["energy", ex] for o in outs}
        assert len(energies) == 1
        want = refs["energy"][0]
        fig["energy"] = max(fig.get("energy", 0.0), float(abs(energies.pop() - want) / want))
    print(f"loads {name} [{backend}]: " + ", ".join(f"{k} {v:.2e}" for k, v in fig.items()))
    assert fig["energy"] <= 4.0 * F64_WORST_RANK_ENERGY, fig["energy"]
    return fig
