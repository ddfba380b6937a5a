"""Range edges of the SpMV split and of the three-launch PCG (csrc/pattern.cpp: spmv_split; csrc/kernels_pcg.hip: k_spmv,
k_pcg_init, k_update_xr, k_update_d), written against the C ABI (femcy_amd.backend.Context) so that the host backend
(tests/test_pcg_shapes_cpu.py, one child process with FEMCY_BACKEND=cpu) and the device (tests/test_gpu_pcg_shapes.py)
run the same code.  Every function checks its own result against a plain reference in np.longdouble; no check compares
one run of a kernel with another.

ROWS holds one small generated mesh per edge.  A row is pinned to (n, nslices, stored_blocks) and carries the property it
exists for as a predicate over the split, which is RESTATED here in numpy (layout(), split_of()) from the row lengths of
the exported matrix -- the ABI does not export the slice ranges: windows of 4096 nodes in the caller's numbering
(FEMCY_OPT_NODE_ORDER = 0), rows sorted by decreasing length inside a window (stable), slices of 64, slice length = the
longest row; range k starts at the first slice whose offset reaches stored * k / 8.  The restatement is pinned against the
library through nslices and stored_blocks (device) and against the table (both backends): a change of spmv_split, SLICE,
VU or the sort window that moves a row off its edge fails the row's own predicate instead of leaving an ordinary mesh.

Loose nodes: nodes no element names (a row of length 1, the diagonal block; every DOF constrained).  They sort to the end
of their window, give slices of length 1 -- WPS = 4 then has three waves with an empty chunk, j1 < j0 -- and, being cheap,
let one range hold many slices on a small mesh.  L = 2 does not exist: a node an element names has at least npe >= 3
blocks in its row, any other exactly 1.

Fit rows: a row carries a check only where the float64 oracle itself meets it, so check_fit() (host backend) asserts for
every row that the oracle's own stop at eps = 1e-10 stays within half of max(2, 2 %) when the unknowns are reversed or K
moves by one rounding, and that its own max|r| is within a quarter of the bound of max|b - K x|.  That is why the CPE8
beam has length 20 and the sliver strip cells of 0.5 x 5: at length 40 and with unit squares the oracle's count scatters
by twice its bound.

Measured constants (x86-64 long double, scipy 1.x CSR product and oracle.pcg_reference in float64 against the references
below, worst over all rows, right-hand sides and vectors, on the host backend's matrices; the tests allow 4 x):
    C_PROD   worst |K x - y_ref|_i / (eps (|K| |x|)_i)                       7.61       7.31
    T_ALPHA  worst |x_1 - ref|_i / |ref|_i after one iteration                6.55e-16   6.34e-16
    T_X[2]   worst max|x_2 - ref| / max|ref| after two iterations             1.40e-14   7.08e-15
    T_X[7]   the same after seven                                             2.85e-14   1.46e-14
(last column: the worst value the device tests print, pytest -s, over every row, WPS, cache policy, task list, storage
order, graph mode and element-wise grid; there the worst |rmax - max|b - K x|| is 0.46 of its bound, the oracle's 0.17.)
tests/test_pcg_shapes_cpu.py measures the float64 column again and fails if it has moved."""
import collections

import numpy as np
import scipy.sparse as sp

from femcy_amd import backend as be
from femcy_amd import meshgen
from femcy_amd.element_zoo import Element_linear_triangular, Element_quadratic_quadrilateral
from femcy_amd.material_zoo import LinearIsotropic, LinearIsotropicPlaneStrain, LinearIsotropicPlaneStress
from oracle import femcy_oracle as orc

import direct_shapes as ds
import loads_reference as lr

LD = np.longdouble
EPS = 2.0 ** -53
SLICE, NX, BS, VU, PU, PU2, SIGMA = 64, 8, 256, 4, 4, 2, 4096     # ctx.hpp, kernels_pcg.hip, Ctx::sell_sigma
C_PROD = 7.62
T_ALPHA = 6.56e-16
T_X = {2: 1.41e-14, 7: 2.85e-14}
MAXITS = (1, 2, 7)
EPS_STOP = 1.0e-10
WPS = (1, 2, 4)
# (FEMCY_TUNE_SPMV_WG_PER_XCD, FEMCY_TUNE_SPMV_ROT): the default, then 1 / 2 / 3 workgroups per XCD with plain, rotated and
# balanced task lists
KNOBS = ((0, -1), (1, 0), (2, 7), (3, 19), (1, 63), (2, 64), (3, 64), (3, 0), (1, 64))
TUNE_SPMV_NT, TUNE_VEC_NT = 102, 103


# ------------------------------------------------------------------------------------------------- the split, restated
def layout(rowlen, sigma=SIGMA):
    """-> (node_of [nslices * 64], -1 = padding; slice_len [nslices]) of build_pattern with the caller's numbering (sigma:
    the sort window, FEMCY_OPT_SELL_SIGMA, a multiple of 64)"""
    nn = len(rowlen)
    ns = -(-nn // SLICE)
    node_of = -np.ones(ns * SLICE, dtype=np.int64)
    for a0 in range(0, nn, sigma):
        idx = np.arange(a0, min(nn, a0 + sigma))
        node_of[a0:a0 + len(idx)] = idx[np.argsort(-rowlen[idx], kind="stable")]
    L = np.where(node_of >= 0, rowlen[np.maximum(node_of, 0)], 0).reshape(ns, SLICE).max(axis=1)
    return node_of, L


Split = collections.namedtuple("Split", "L start lens stored spb tasks per bpx rounds n2 er elens")


def split_of(L, dm, nn, wps=1, cap=0, storage=True):
    """spmv_split's cut and pcg_solve's element ranges: start[9] in slices, lens[8], tasks[8] of spb slices, bpx workgroups
    per XCD, rounds[8] of the in-kernel loop, er[9] / elens[8] in double2 units (storage or node order)"""
    ns = len(L)
    off = np.concatenate([[0], np.cumsum(L)])
    stored = int(off[-1])
    start, s = [0], 0
    for k in range(1, NX):
        while s < ns and off[s] < stored * k // NX:
            s += 1
        start.append(s)
    start = np.array(start + [ns])
    lens = np.diff(start)
    spb = 4 // wps
    tasks = -(-lens // spb)
    per = max(1, int(tasks.max()))
    bpx = min(per, cap if cap > 0 else 256)
    n2 = ns * SLICE * dm // 2 if storage else (nn * dm + 1) // 2
    er = np.minimum(n2, (start * SLICE * dm + 1) // 2)
    er[0], er[NX] = 0, n2
    return Split(np.asarray(L), start, lens, stored, spb, tasks, per, bpx, -(-tasks // bpx), n2, er, np.diff(er))


def ew_grid(sp_, ew_cap=512):
    """workgroups of k_pcg_init / k_update_xr / k_update_d"""
    return NX * max(1, min(-(-max(1, int(sp_.elens.max())) // BS), max(1, ew_cap // NX)))


def batches(sp_, ew_cap):
    """trips of `while (base < n2)` a range of the vector kernels needs"""
    stride = ew_grid(sp_, ew_cap) // NX * BS
    return -(-sp_.elens // (VU * stride))


# ------------------------------------------------------------------------------------------------------------ meshes
def _with_loose(nodes, el, loose):
    """`loose` unreferenced nodes behind the mesh; the mesh's last node then trades places with the last loose one, so
    that the last DOF of the system is a coupled one"""
    if not loose:
        return nodes, el, np.zeros(0, np.int64)
    nm = len(nodes)
    extra = nodes.max(axis=0) + 1.0 + np.arange(loose)[:, None] * np.ones(nodes.shape[1])
    nodes = np.vstack([nodes, extra])
    last = len(nodes) - 1
    nodes[[nm - 1, last]] = nodes[[last, nm - 1]]
    el = el.copy()
    el[el == nm - 1] = last
    ids = np.arange(nm - 1, last)
    return nodes, el.astype(np.int32), ids


def sliver(strip, lone):
    """`lone` CPS3 triangles that share no node (rows of 3 blocks), then a strip of 2 x strip triangles (rows of 3 .. 5)"""
    nodes, quads = lr.grid2d(strip, 1, size=(strip / 2.0, 5.0))       # (a strip of unit squares is too slender: check_fit)
    pts = [np.array([[2.0 * t + 0.5, 6.0], [2.0 * t + 1.5, 6.0], [2.0 * t + 0.8, 6.9]]) for t in range(lone)]
    tris = [np.array([[0, 1, 2]], np.int32) + 3 * t for t in range(lone)]
    return np.vstack(pts + [nodes]), np.vstack(tris + [lr._tris(quads) + 3 * lone]).astype(np.int32)


def build(row):
    """-> (nodes, elements, plug-in, material, constrained DOFs)"""
    if row.kind == "strip":
        # (persist_shapes.py) nx x ny square cells of CPS3 pairs, BOTH LONG EDGES held: a 2-D system of 100 .. 256 slices
        # whose residual does not grow in the first iterations.  Held at one short edge, a smooth load lifts max|r| to
        # 100 r0 (alpha ~ nodes / held nodes), and the float64 oracle's own max|r| is then two roundings of that away from
        # max|b - K x|: check_fit
        nodes, quads = lr.grid2d(row.args[0], row.args[1], size=(0.05 * row.args[0], 0.05 * row.args[1]), perturb=0.25, seed=3)
        el, ELE, mat = lr._tris(quads), Element_linear_triangular(), LinearIsotropicPlaneStress(2.0e5, 0.3)
    elif row.kind in ("beam", "held-beam"):
        m = meshgen.beam_quad8(*row.args)
        nodes, el, ELE, mat = m["nodes"], m["elements"], Element_quadratic_quadrilateral(), LinearIsotropicPlaneStrain(2.0e5, 0.3)
    elif row.kind == "sliver":
        nodes, el = sliver(*row.args)
        ELE, mat = Element_linear_triangular(), LinearIsotropicPlaneStrain(2.0e5, 0.3)
    else:
        nodes, el, ELE = lr.mesh(row.kind, row.args)
        mat = LinearIsotropic(2.0e5, 0.3) if ELE.dm == 3 else LinearIsotropicPlaneStress(2.0e5, 0.3)
    dm = nodes.shape[1]
    if row.kind in ("strip", "held-beam"):
        held = np.nonzero((nodes[:, 1] == nodes[:, 1].min()) | (nodes[:, 1] == nodes[:, 1].max()))[0]
        held = held[held != len(nodes) - 1]      # (b = e_(n-1) on a constrained DOF alone is solved in one iteration: 0 / 0 next)
        cons = np.concatenate([held * 2, held * 2 + 1])
    elif row.kind == "sliver":   # the strip's left edge; every lone triangle: its first node held, its second in y
        first = 3 * np.arange(row.args[1])
        left = np.nonzero(nodes[:, 0] == 0.0)[0]
        cons = np.concatenate([left * 2, left * 2 + 1, first * 2, first * 2 + 1, (first + 1) * 2 + 1])
    else:
        cons = ds.clamped_dofs(nodes, el, ELE)
    nodes, el, ids = _with_loose(nodes, el, row.loose)
    nm = len(nodes) - row.loose
    cons = np.where(cons // dm == nm - 1, (len(nodes) - 1) * dm + cons % dm, cons) if row.loose else cons
    cons = np.concatenate([cons, (ids[:, None] * dm + np.arange(dm)[None, :]).ravel()])
    return nodes, el, ELE, mat, np.unique(cons).astype(np.int32)


Row = collections.namedtuple("Row", "name kind args loose n nslices stored edge why")


def _r(name, kind, args, loose, n, nslices, stored, edge, why):
    return Row(name, kind, args, loose, n, nslices, stored, edge, why)


def _trailing_empty(elens):
    k = 0
    while k < NX and elens[NX - 1 - k] == 0:
        k += 1
    return k


# S(w): the split with w waves per slice in storage order; N: in node order (both with the default 256 workgroups per XCD)
ROWS = [
    _r("one-slice-c3d4", "C3D4", (1, 1, 2), 0, 36, 1, 576,
       lambda S, N: S(1).lens.tolist() == [1, 0, 0, 0, 0, 0, 0, 0] and N.n2 == 18 and _trailing_empty(N.elens) == 7
       and (S(1).er[1:] == S(1).n2).all() and S(1).n2 == 96,
       "1 slice of 12 nodes: ranges 1..7 empty, n even, every `er` start but the first clamped to n2; storage order: "
       "npos * dm / 2 = 96 is the start of ranges 1..7"),
    _r("one-slice-cps3", "CPS3", (9, 5), 0, 120, 1, 448,
       lambda S, N: S(1).lens.tolist() == [0, 1, 0, 0, 0, 0, 0, 0] and S(1).stored // NX == 0,
       "7 stored block rows: the first target is 0, range 0 is EMPTY and range 1 holds the slice; dm = 2, 60 nodes"),
    _r("two-slices-c3d4", "C3D4", (3, 3, 5), 0, 288, 2, 1536,
       lambda S, N: S(1).lens.tolist() == [1, 0, 0, 0, 0, 1, 0, 0] and _trailing_empty(N.elens) == 2 and N.elens[5] == 48,
       "2 slices: first-but-one, middle and last ranges empty; node order: two trailing ranges empty behind a clamped start"),
    _r("four-slices-c3d10", "C3D10", (2, 2, 4), 0, 675, 4, 7616,
       lambda S, N: S(1).lens.tolist() == [1, 0, 0, 0, 1, 1, 0, 1] and N.n2 == 338 and N.elens[7] == 50,
       "rows of 14 .. 65 blocks: the first slice holds 3 / 8 of the work; n = 675 odd, the last double2 is half padding"),
    _r("seven-slices-c3d10", "C3D10", (3, 3, 4), 0, 1323, 7, 12032,
       lambda S, N: S(1).lens.tolist() == [1, 0, 1, 1, 0, 2, 1, 1] and S(2).tasks[5] == 1 and S(4).tasks[5] == 2,
       "uneven rows move the cuts: ranges 1 and 4 empty, range 5 has 2 slices (0 mod SPB for WPS = 2, two tasks for WPS = 4)"),
    _r("eight-slices-c3d8", "C3D8", (7, 7, 7), 0, 1536, 8, 11136,
       lambda S, N: S(1).lens.tolist() == [1, 1, 1, 1, 0, 2, 1, 1] and N.n2 * 2 == 1536,
       "8 slices and still an empty range; 512 nodes: no padding lane, n even"),
    _r("nine-slices-c3d6", "C3D6", (8, 7, 7), 0, 1728, 9, 9792,
       lambda S, N: S(1).lens.tolist() == [1, 1, 1, 1, 1, 1, 2, 1],
       "9 slices: no range empty, one of 2"),
    _r("nine-slices-cpe8", "beam", (40, 4, 20.0, 4.0), 0, 1138, 9, 8192,
       lambda S, N: S(1).lens.tolist() == [1, 1, 1, 1, 1, 2, 1, 1] and N.n2 % SLICE == 57,        # dm = 2: n2 nodes
       "the CPE8 beam's 40 x 4 cells at half its length: 569 nodes (57 in the last slice), dm = 2"),
    _r("seventeen-slices-c3d4", "C3D4", (5, 5, 29), 0, 3240, 17, 13376,
       lambda S, N: S(1).lens.tolist() == [2, 2, 2, 1, 3, 2, 2, 3] and S(2).tasks[4] == 2 and N.elens[7] == 276,
       "17 slices: ranges of 1, 2 and 3 (3 = 1 mod SPB for WPS = 2)"),
    _r("slivers-cps3", "sliver", (40, 30), 70, 484, 4, 896,
       lambda S, N: S(4).L.tolist() == [5, 5, 3, 1] and S(4).lens.tolist() == [1, 0, 0, 1, 0, 0, 1, 1],
       "slices of length 5, 5, 3 and 1 (the strip, lone triangles, loose nodes): waves with an empty chunk for WPS = 4 "
       "(L = 5: j0 = 6 > j1 = 5; L = 3; L = 1) and for WPS = 2 (L = 1)"),
    _r("task-tails-c3d4", "C3D4", (10, 10, 24), 0, 9075, 48, 40832,
       lambda S, N: S(1).lens.tolist() == [6, 5, 5, 6, 5, 6, 7, 8] and S(1).tasks.tolist() == [2, 2, 2, 2, 2, 2, 2, 2]
       and S(2).tasks.tolist() == [3, 3, 3, 3, 3, 3, 4, 4] and S(1, 1).rounds.max() == 2,
       "48 slices: range lengths 5 (1 mod 4, 1 mod 2), 8 (0 mod 4) and 6 (0 mod 2): the last task of a range full and partial "
       "for every WPS; one workgroup per XCD walks two rounds"),
    _r("rounds-c3d4", "C3D4", (5, 5, 29), 512, 4776, 25, 13888,
       lambda S, N: S(4).tasks.max() >= 9 and S(4).tasks.min() <= 2 and S(4, 3).rounds.max() >= 3 and S(4, 3).rounds.min() == 1
       and S(4, 3).tasks.max() % 3 != 0 and S(4, 2).rounds.max() > S(4, 2).rounds.min() and S(4, 1).rounds.max() >= 9
       and (S(4, 3).rounds.max() * S(4, 3).bpx > S(4, 3).tasks).all() and (S(4, 3).rounds.max() > S(4, 3).rounds).sum() == 7,
       "the 17 slices above and 8 of loose nodes, all in the last range: >= 9 tasks there against 1 or 2 elsewhere at WPS = 4; "
       "1, 2 and 3 workgroups per XCD give rounds that differ from range to range, a partial last round, and a balanced "
       "table (mode 64) whose last rounds are padding for seven ranges"),
    _r("batches-c3d4", "C3D4", (13, 13, 27), 700, 18564, 97, 75840,
       lambda S, N: sorted(set(batches(S(1), 8).tolist())) == [1, 2, 3] and sorted(set(batches(S(1), 16).tolist())) == [1, 2]
       and batches(S(1), 512).max() == 1 and S(1).elens.max() > VU * BS,
       "6 188 nodes, 700 of them loose: FEMCY_OPT_EW_GRID = 8 gives ranges of one, two and (the last) three batches of 1024 "
       "double2; 16 gives one or two; the default 512 one"),
    _r("partials-c3d4", "C3D4", (13, 13, 27), 15600, 63264, 330, 91200,
       lambda S, N: NX * S(4, 512).bpx == 1376 > PU * BS and ew_grid(S(1), 4096) == ew_grid(N, 4096) == 520 > PU2 * BS
       and S(4).lens[7] == 172 and batches(S(1), 4096).max() == 1,
       "the same plate with 15 600 loose nodes, the smallest count that reaches both: range 7 holds 1 / 8 of the stored work, "
       "172 slices of (all but one) length 1 -- 171 would do, 64 * 256 double2 are 170.7 slices of 96.  WPS = 4 with "
       "FEMCY_TUNE_SPMV_WG_PER_XCD = 512 gives 8 * 172 = 1376 SpMV workgroups, FEMCY_OPT_EW_GRID = 4096 gives 8 * 65 = 520: "
       "k_update_xr reads partials beyond PU * BS = 1024 and k_update_d pairs beyond PU2 * BS = 512 in their tail loops"),
]


def row_id(row):
    return row.name


# ----------------------------------------------------------------------------------------------------- references
def mul_ld(K, x, absolute=False):
    """row-wise product in long double (every row of K holds its diagonal: no empty row)"""
    data = K.data.astype(LD)
    xv = np.asarray(x).astype(LD)[K.indices]
    p = np.abs(data) * np.abs(xv) if absolute else data * xv
    return np.add.reduceat(p, K.indptr[:-1])


def pcg_ld(K, b, maxit):
    """oracle.pcg_reference's recurrence (eps = 0) in long double -> the iterates x_1 .. x_maxit"""
    M = LD(1) / K.diagonal().astype(LD)
    b = b.astype(LD)
    x, r, d = np.zeros(len(b), LD), b.copy(), M * b
    out = []
    for _ in range(maxit):
        Ad = mul_ld(K, d)
        rMr = np.dot(r * M, r)
        alpha = rMr / np.dot(d, Ad)
        x = x + alpha * d
        r = r - alpha * Ad
        d = M * r + (np.dot(r * M, r) / rMr) * d
        out.append(x)
    return out


class Case:
    """one row on one backend: the context with K assembled and constrained, the exported K, the restated split, the
    vectors and the long-double references (computed once)"""

    mesh = staticmethod(build)                                     # (a further table may bring its own meshes)

    def __init__(self, row, backend):
        self.row, self.backend = row, backend
        nodes, el, ELE, mat, cons = self.mesh(row)
        self.dm = nodes.shape[1]
        self.sigma = getattr(row, "sigma", SIGMA)                  # (a further table may narrow the sort window)
        ctx = self.ctx = be.Context(0, backend=backend)
        ctx.set_option(be.OPT_NODE_ORDER, 0)                       # the caller's numbering: what layout() restates
        if self.sigma != SIGMA:
            ctx.set_option(be.OPT_SELL_SIGMA, self.sigma)
        ctx.set_mesh(nodes, el)
        ctx.set_element(ELE)
        ctx.set_material(mat)
        ctx.build_pattern()
        ctx.assemble_K(-1)
        ctx.dirichlet_newton(cons, be.VEC_RESIDUAL)
        self.K = ctx.get_K_bsr().tocsr()
        self.K.sort_indices()
        self.n, self.nn, self.cons = ctx.n, len(nodes), cons
        self.rowlen = np.diff(ctx.get_K_bsr().indptr)
        self.node_of, self.L = layout(self.rowlen, self.sigma)
        self.absK = None
        rng = np.random.default_rng(7)
        x0 = rng.standard_normal(self.n)
        x1 = rng.standard_normal(self.n)
        x1[-self.dm:] = 1.0e12                                     # a wrong gather of the last node cannot hide
        self.xs = {"normal": x0, "huge-last": x1}
        self.yref = {k: (mul_ld(self.K, v), mul_ld(self.K, v, True)) for k, v in self.xs.items()}
        self.bs = self._rhs(nodes)
        self.xref = {k: pcg_ld(self.K, b, max(MAXITS)) for k, b in self.bs.items()}

    def S(self, wps=1, cap=0):
        return split_of(self.L, self.dm, self.nn, wps, cap, True)

    @property
    def N(self):
        return split_of(self.L, self.dm, self.nn, 1, 0, False)

    def _rhs(self, nodes):
        """a smooth b; b = e_(n-1); b = 1 at the first DOF of every non-empty range (storage order: the first position of
        the range's first slice; node order: the first double2 of the element range -- the first free DOF from there on)"""
        smooth = np.sin(nodes @ np.arange(1, self.dm + 1) * 0.37)[:, None] * np.arange(1, self.dm + 1)[None, :] * 1.0e3
        last = np.zeros(self.n)
        last[-1] = 1.0e3
        starts = np.zeros(self.n)
        S, N = self.S(), self.N
        free = np.ones(self.n, dtype=bool)
        free[self.cons] = False
        pos_dofs = (self.node_of[self.node_of >= 0][:, None] * self.dm + np.arange(self.dm)[None, :]).ravel()
        for k in range(NX):                                        # (a constrained DOF alone would be solved in one iteration)
            if S.lens[k] > 0:
                behind = pos_dofs[np.searchsorted(np.nonzero(self.node_of >= 0)[0], S.start[k] * SLICE) * self.dm:]
                starts[(behind[free[behind]] if free[behind].any() else behind)[0]] = 1.0e3
            if N.elens[k] > 0:
                starts[2 * N.er[k] + (np.nonzero(free[2 * N.er[k]:])[0][0] if free[2 * N.er[k]:].any() else 0)] = 1.0e3
        return {"smooth": smooth.ravel(), "last": last, "starts": starts}

    def close(self):
        self.ctx.close()


_CASES = collections.OrderedDict()
TABLES = {}                # name -> (row, Case class): the rows of further tables built on this machinery (persist_shapes.py)


def case(name, backend):
    """the Case of a row, built once while the tests walk the table row by row: two stay alive, an older one is closed"""
    key = (name, backend)
    if key not in _CASES:
        while len(_CASES) >= 2:
            _CASES.popitem(last=False)[1].close()
        row, cls = TABLES.get(name) or (next(r for r in ROWS if r.name == name), Case)
        _CASES[key] = cls(row, backend)
    _CASES.move_to_end(key)
    return _CASES[key]


def _reset(ctx):
    for opt, val in ((be.OPT_SPMV_VARIANT, 0), (be.TUNE_SPMV_WG_PER_XCD, 0), (be.TUNE_SPMV_ROT, -1), (TUNE_SPMV_NT, -1),
                     (TUNE_VEC_NT, -1), (be.OPT_EW_GRID, 512), (be.OPT_PCG_SMALL, 1), (be.OPT_PCG_PERSIST, 1),
                     (be.OPT_PCG_STORAGE_ORDER, 1), (be.OPT_PCG_GRAPH, 1), (be.OPT_PCG_POLL, 32)):
        ctx.set_option(opt, val)


def sweeps(c, full=True):
    """(wps, nt, cap, rot) settings: all of them on the device, one on the host (whose library takes the knobs as no-ops)"""
    if c.backend != "hip":
        return [(0, -1, 0, -1)]
    if not full:
        return [(w, 0, cap, rot) for w in WPS for cap, rot in ((0, -1), (3, 64))]
    return [(w, nt, cap, rot) for w in WPS for nt in (0, 1) for cap, rot in KNOBS]


def _set(ctx, wps, nt, cap, rot):
    ctx.set_option(be.OPT_SPMV_VARIANT, wps)
    ctx.set_option(TUNE_SPMV_NT, nt)
    ctx.set_option(TUNE_VEC_NT, nt)
    ctx.set_option(be.TUNE_SPMV_WG_PER_XCD, cap)
    ctx.set_option(be.TUNE_SPMV_ROT, rot)


# ----------------------------------------------------------------------------------------------------------- checks
def check_edge(name, backend):
    """the counts of the table, the restatement against the library, and the property the row exists for"""
    c = case(name, backend)
    row, info = c.row, c.ctx.pattern_info()
    assert (info.n, info.nslices) == (row.n, row.nslices), (info.n, info.nslices, row)
    S = c.S()
    assert len(c.L) == row.nslices and S.stored * SLICE == row.stored, (len(c.L), S.stored * SLICE, row)
    if backend == "hip":                                           # (the host library stores block-CSR: stored = nnzb)
        assert info.stored_blocks == row.stored, (info.stored_blocks, row)
    assert row.edge(c.S, c.N), (row.why, S, c.N)
    for w in WPS:                                                  # the split's own invariants
        Sw = c.S(w)
        assert Sw.start[0] == 0 and Sw.start[NX] == row.nslices and (Sw.lens >= 0).all()
        assert Sw.er[0] == 0 and (np.diff(Sw.er) >= 0).all() and Sw.er[NX] == row.nslices * SLICE * c.dm // 2
        assert (c.N.er <= c.N.n2).all() and c.N.n2 == (row.n + 1) // 2
    return S


def check_product(name, backend):
    """femcy_spmv (node order) row by row: |y - y_ref|_i <= 4 C_PROD eps (|K| |x|)_i for every WPS, cache policy, number of
    workgroups per XCD and task-list mode.  -> the worst ratio to eps (|K| |x|)_i"""
    c = case(name, backend)
    ctx, worst = c.ctx, 0.0
    try:
        for wps, nt, cap, rot in sweeps(c):
            _set(ctx, wps, nt, cap, rot)
            for key, x in c.xs.items():
                ctx.upload(be.VEC_TMP0, x)
                ctx.vector(be.VEC_TMP1).fill(np.nan)               # a row nobody writes stays visible
                ctx.spmv(be.VEC_TMP0, be.VEC_TMP1)
                y = ctx.download(be.VEC_TMP1)
                assert y.shape == (c.n,) and np.isfinite(y).all(), (key, wps, nt, cap, rot)
                yref, scale = c.yref[key]
                ratio = np.abs(y.astype(LD) - yref) / (EPS * scale)
                bad = int(np.argmax(ratio))
                worst = max(worst, float(ratio[bad]))
                assert ratio[bad] <= 4.0 * C_PROD, (key, wps, nt, cap, rot, "row", bad, "node", bad // c.dm, float(ratio[bad]))
    finally:
        _reset(ctx)
    print(f"{name} [{backend}]: product, worst |y - y_ref|_i / (eps (|K| |x|)_i) = {worst:.3f} (allowed {4 * C_PROD:.2f})")
    return worst


def _solve(c, b, maxit, eps=0.0):
    ctx = c.ctx
    ctx.upload(be.VEC_RESIDUAL, b)
    ctx.vector(be.VEC_X).fill(np.nan)
    before = ctx.timing()
    it, r0, rmax = ctx.pcg(be.VEC_RESIDUAL, be.VEC_X, eps=eps, maxit=maxit)
    after = ctx.timing()
    x = ctx.download(be.VEC_X)
    assert x.shape == (c.n,) and np.isfinite(x).all()              # padding lanes of a storage-order solve stay out
    moved = {k: after[k] - before[k] for k in ("solves_three", "solves_small", "solves_persist", "barrier_timeouts")}
    return it, r0, rmax, x, moved


def _check_iterate(c, key, m, out, what, worst, t_alpha=None, t_x=None):
    """one solve of m iterations with eps = 0 against the long-double recurrence (t_alpha, t_x: the measured constants of
    another table; this one's by default)."""
    t_alpha, t_x = t_alpha or T_ALPHA, t_x or T_X
    it, r0, rmax, x, _ = out
    b, ref = c.bs[key], c.xref[key][m - 1]
    assert it == m, (what, it)
    assert r0 == np.abs(b).max(), (what, r0)
    if m == 1:                                                     # x_1 = alpha M b: entry by entry
        nz = ref != 0
        assert not x[~nz].any(), what
        dev = float((np.abs(x[nz].astype(LD) - ref[nz]) / np.abs(ref[nz])).max())
        tol = 4.0 * t_alpha
    else:
        dev = float(np.abs(x.astype(LD) - ref).max() / np.abs(ref).max())
        tol = 4.0 * t_x[m]
    worst[m] = max(worst.get(m, 0.0), dev)
    assert dev <= tol, (what, dev, tol)
    res = float(np.abs(b.astype(LD) - mul_ld(c.K, x)).max())
    worst["rmax"] = max(worst.get("rmax", 0.0), abs(rmax - res) / r0 / tol)
    assert abs(rmax - res) <= tol * r0, (what, rmax, res, tol * r0)


def check_recurrence(name, backend):
    """the three-launch loop, forced: both storage orders, graph replay on and off, maxit 1, 2, 7 with eps = 0, three
    right-hand sides; then x_1 (the storage-order product's d.Ad and the first update) under every WPS, cache policy and
    task list, and under FEMCY_OPT_EW_GRID 8 and 16.  -> worst deviations {1: , 2: , 7: }"""
    c = case(name, backend)
    ctx, worst = c.ctx, {}
    try:
        ctx.set_option(be.OPT_PCG_SMALL, 0)
        ctx.set_option(be.OPT_PCG_PERSIST, 0)
        ctx.set_option(be.OPT_PCG_POLL, 1)                         # a burst of one iteration: replay whenever maxit >= 1
        for order in (1, 0):
            ctx.set_option(be.OPT_PCG_STORAGE_ORDER, order)
            for graph in (2, 0):
                ctx.set_option(be.OPT_PCG_GRAPH, graph)
                grids = [(512, 0, 0), (8, 0, 0), (16, 0, 0)] if graph == 0 or c.n > 4096 else [(512, 0, 0)]
                if NX * c.S(4, 512).bpx > PU * BS:                 # many partials: (element-wise grid, WPS, workgroups per XCD)
                    grids.append((4096, 4, 512))
                for ew, wps, cap in grids:
                    ctx.set_option(be.OPT_EW_GRID, ew)
                    ctx.set_option(be.OPT_SPMV_VARIANT, wps)
                    ctx.set_option(be.TUNE_SPMV_WG_PER_XCD, cap)
                    for key in c.bs:
                        for m in MAXITS:
                            out = _solve(c, c.bs[key], m)
                            assert out[4] == {"solves_three": 1, "solves_small": 0, "solves_persist": 0, "barrier_timeouts": 0}, out[4]
                            _check_iterate(c, key, m, out, (name, "order", order, "graph", graph, "ew", ew, key, m), worst)
                _set(ctx, 0, -1, 0, -1)
                ctx.set_option(be.OPT_EW_GRID, 512)
            ctx.set_option(be.OPT_PCG_GRAPH, 0)
            for wps, nt, cap, rot in sweeps(c):
                _set(ctx, wps, nt, cap, rot)
                for key in ("smooth", "starts"):
                    for m in (1, 2):
                        _check_iterate(c, key, m, _solve(c, c.bs[key], m), (name, "order", order, wps, nt, cap, rot, key, m), worst)
            _set(ctx, 0, -1, 0, -1)
    finally:
        _reset(ctx)
    print(f"{name} [{backend}]: three launches, worst deviation from the long-double recurrence {worst} "
          f"(allowed 1: {4 * T_ALPHA:.1e}, 2: {4 * T_X[2]:.1e}, 7: {4 * T_X[7]:.1e}; rmax as a share of its bound)")
    return worst


def check_convergence(name, backend):
    """eps = 1e-10 to the stop, three launches in both orders: the iteration count of the oracle within max(2, 2 %) and a
    residual that solves the system."""
    c = case(name, backend)
    ctx, eps = c.ctx, EPS_STOP
    b = c.bs["smooth"]
    _, ito, r0o, _ = orc.pcg_reference(c.K, b, eps=eps, maxit=20 * c.n)
    try:
        ctx.set_option(be.OPT_PCG_SMALL, 0)
        ctx.set_option(be.OPT_PCG_PERSIST, 0)
        for order in (1, 0):
            ctx.set_option(be.OPT_PCG_STORAGE_ORDER, order)
            it, r0, rmax, x, moved = _solve(c, b, 20 * c.n, eps)
            assert moved["solves_three"] == 1 and moved["solves_small"] == 0 and moved["solves_persist"] == 0, moved
            assert r0 == r0o and rmax < eps * r0
            assert abs(it - ito) <= max(2, ito // 50), (order, it, ito)
            res = float(np.abs(mul_ld(c.K, x) - b.astype(LD)).max())
            print(f"{name} [{backend}]: order {order}, {it} iterations (oracle {ito}), max|K x - b| / r0 = {res / r0:.2e}")
            assert res < 2 * eps * r0 + 1e-9 * r0, (order, res, r0)
    finally:
        _reset(ctx)


def check_path(name, backend, path):
    """the same iterates through k_pcg_small (path "small") or the persistent kernel ("persist": FEMCY_OPT_PCG_PERSIST = 2,
    any system whose slices fit).  -> (True when the path took the mesh, worst deviations); a path that declines must have
    handed the solve to the three-launch loop without a barrier time-out.  The host library has the one loop."""
    c = case(name, backend)
    ctx, worst, took = c.ctx, {}, set()
    try:
        ctx.set_option(be.OPT_PCG_SMALL, 1 if path == "small" else 0)
        ctx.set_option(be.OPT_PCG_PERSIST, 2 if path == "persist" else 0)
        for key in c.bs:
            for m in MAXITS:
                out = _solve(c, c.bs[key], m)
                moved = out[4]
                assert moved["barrier_timeouts"] == 0 and sum(moved.values()) == 1, moved
                other = "solves_persist" if path == "small" else "solves_small"
                assert moved[other] == 0, moved
                took.add(moved["solves_" + path] == 1 if backend == "hip" else True)
                _check_iterate(c, key, m, out, (name, path, key, m), worst)
    finally:
        _reset(ctx)
    assert len(took) == 1, "a path must take or decline a mesh for every solve alike"
    accepted = took.pop()
    if backend == "hip" and path == "small" and c.n <= 4096:      # 39 KB of LDS, <= 64 workgroups: no device declines that
        assert accepted, "k_pcg_small declined a system of %d DOF" % c.n
    print(f"{name} [{backend}]: path {path} {'took' if accepted else 'DECLINED'} the mesh, worst deviation {worst}")
    return accepted, worst


# ------------------------------------------------------------------------------ the reference's own error, per row
def _one_rounding(K, seed):
    """K with every entry moved by up to one rounding, symmetric"""
    rng = np.random.default_rng(seed)
    U = sp.triu(K, 1).tocsr()
    U.data = U.data * (1.0 + EPS * rng.uniform(-1.0, 1.0, U.nnz))
    Kq = (U + U.T + sp.diags(K.diagonal() * (1.0 + EPS * rng.uniform(-1.0, 1.0, K.shape[0])))).tocsr()
    Kq.sort_indices()
    return Kq


def check_fit(name, backend):
    """the two conditions of the header: what the float64 oracle cannot reproduce of itself, no kernel can be held to.
    -> (the oracle's iteration counts, its worst residual gap as a share of the bound)"""
    c = case(name, backend)
    b, maxit = c.bs["smooth"], 20 * c.n
    rev = np.arange(c.n)[::-1]
    Kr = c.K[rev][:, rev].tocsr()
    Kr.sort_indices()
    its = [orc.pcg_reference(c.K, b, eps=EPS_STOP, maxit=maxit)[1], orc.pcg_reference(Kr, b[rev], eps=EPS_STOP, maxit=maxit)[1]]
    its += [orc.pcg_reference(_one_rounding(c.K, seed), b, eps=EPS_STOP, maxit=maxit)[1] for seed in (1, 2, 3)]
    assert 2 * max(abs(it - its[0]) for it in its) <= max(2, its[0] // 50), (name, its)
    share = 0.0
    for key, b in c.bs.items():
        r0 = np.abs(b).max()
        for m in MAXITS:
            x, _, _, rmax = orc.pcg_reference(c.K, b, eps=0.0, maxit=m)
            res = float(np.abs(b.astype(LD) - mul_ld(c.K, x)).max())
            share = max(share, abs(rmax - res) / (4.0 * (T_ALPHA if m == 1 else T_X[m]) * r0))
            assert 4.0 * share <= 1.0, (name, key, m, rmax, res, share)
    print(f"{name} [{backend}]: the oracle stops at {its}; its own max|r| is within {share:.3f} of the bound of max|b - K x|")
    return its, share


# -------------------------------------------------------------------------------------- the constants, measured
def measure_constants(backend="cpu", rows=None):
    """float64 (scipy's CSR product, oracle.pcg_reference) against the long-double references over the table (or `rows`)"""
    c_prod, t = 0.0, {m: 0.0 for m in MAXITS}
    for row in rows or ROWS:
        c = case(row.name, backend)
        for key, x in c.xs.items():
            yref, scale = c.yref[key]
            c_prod = max(c_prod, float((np.abs((c.K @ x).astype(LD) - yref) / (EPS * scale)).max()))
        for key, b in c.bs.items():
            for m in MAXITS:
                x = orc.pcg_reference(c.K, b, eps=0.0, maxit=m)[0]
                ref = c.xref[key][m - 1]
                if m == 1:
                    nz = ref != 0
                    t[m] = max(t[m], float((np.abs(x[nz].astype(LD) - ref[nz]) / np.abs(ref[nz])).max()))
                else:
                    t[m] = max(t[m], float(np.abs(x.astype(LD) - ref).max() / np.abs(ref).max()))
    return c_prod, t
