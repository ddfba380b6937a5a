"""Band shapes of the direct solve (femcy_direct_solve), written against the C ABI (femcy_amd.backend.Context) so that
the host backend (tests/test_direct_shapes_cpu.py, backend "cpu") and the device (tests/test_gpu_direct_shapes.py,
backend "hip") run the same code.  Every function checks its own result.

A band is (n, bw) -> T = ceil(bw / 32) tiles below the diagonal tile, P = ceil(n / 32) column panels; panel p updates
Tp = min(T, P - 1 - p) tiles and the backward sweep of panel p reaches Tq = min(T, p) panels back.  ROWS holds one small
mesh for every edge of those counts.  Two kinds of system:

  * manufactured(): positive definite, b = K x_true with |K| |x| / |b| ~ 1 -- a correct factor leaves a rounding-level
    residual, five orders under the refinement threshold (band_order.hpp: 1e-10), so `refinements == 0` is a condition:
    a factor that is off in a few entries is a good preconditioner and the refinement would repair it unseen;
  * inertia(): the indefinite K of a configuration with inverted elements -- by Sylvester's law the number of negative
    pivots of K = L S L^T is the number of negative eigenvalues of K, whatever the elimination order."""
import collections
import ctypes as C

import numpy as np
import scipy.sparse.linalg as spl

from femcy_amd import backend as be

import loads_cases as lc
import loads_reference as lr

NB = 32                                   # panel width = tile edge of the device's band storage
MFMA_MIN_TILES = 8                        # kernels_direct.hip: auto takes the matrix-core update from Tp = 8 on
VARIANTS = (-1, 0, 1, 2, 3)               # FEMCY_TUNE_DIRECT_UPDATE: auto, VALU, matrix cores 1 x 1 / 2 x 2, two streams

Row = collections.namedtuple("Row", "kind arg cells n bw T P")

# (n, bw) as band_order.hpp's reverse Cuthill-McKee gives them (measured on the host backend, which shares that file
# with the device): if a generator of loads_reference.py changes, this table has to be derived again
ROWS = [
    Row("single", "CPS8", None, 16, 15, 1, 1),           # one panel, no update, Tq = 0
    Row("single", "C3D10", None, 30, 29, 1, 1),          # one panel, dm = 3, 2 pad rows
    Row("fan", 15, None, 32, 25, 1, 1),                  # one panel, no pad rows
    Row("fan", 16, None, 34, 27, 1, 2),                  # 30 pad rows
    Row("mesh", "C3D4", (2, 2, 10), 297, 32, 1, 10),     # bw = 32 exactly
    Row("mesh", "CPS3", (30, 14), 930, 33, 2, 30),       # bw = 33
    Row("mesh", "C3D10", (1, 1, 1), 81, 59, 2, 3),       # T = P - 1
    Row("fan", 40, None, 82, 75, 3, 3),                  # T > P - 1: every panel clipped
    Row("fan", 70, None, 142, 135, 5, 5),                # the same, T odd
    Row("mesh", "CPS4", (40, 15), 1312, 65, 3, 41),      # no pad rows, many panels
    Row("mesh", "C3D6", (4, 4, 6), 525, 140, 5, 17),     # T odd
    Row("mesh", "C3D8", (4, 4, 8), 675, 185, 6, 22),     # T even
    Row("mesh", "C3D4", (7, 7, 10), 2112, 197, 7, 66),   # one below the matrix-core switch, no pad rows
    Row("mesh", "C3D4", (8, 8, 12), 3159, 248, 8, 99),   # at the switch
    Row("mesh", "C3D8", (5, 5, 8), 972, 275, 9, 31),     # one above
    Row("mesh", "C3D10", (3, 3, 6), 1911, 470, 15, 60),
    Row("mesh", "C3D10", (4, 4, 6), 3159, 728, 23, 99),  # widest
]


def row_id(row):
    tail = "x".join(str(c) for c in row.cells) if row.cells else ""
    return "%s-%s%s-n%d-bw%d" % (row.kind, row.arg, "-" + tail if tail else "", row.n, row.bw)


def build(row):
    """-> (nodes, elements, plug-in)"""
    if row.kind == "single":
        return lr.single(row.arg)[:3]
    if row.kind == "fan":
        return lr.fan(row.arg)
    return lr.mesh(row.arg, row.cells)


def clamped_dofs(nodes, el, ELE):
    """every DOF of the nodes on the face x = min x (nodes 0..2 where that holds fewer than 6 DOF): no rigid mode is
    left.  Quadratic tetrahedra: the face of the corner nodes, and the mid-side nodes between two clamped corners --
    loads_reference.mesh moves the mid-side nodes off the plane, so that `x == min x` would hold a single one of them"""
    dm = nodes.shape[1]
    held = np.zeros(len(nodes), dtype=bool)
    if el.shape[1] == 10:
        corners = np.unique(el[:, :4])
        held[corners[nodes[corners, 0] == nodes[corners, 0].min()]] = True
    else:
        held[nodes[:, 0] == nodes[:, 0].min()] = True
    if el.shape[1] == 10:
        for m, (a, b) in enumerate(TET10_EDGES):
            both = held[el[:, a]] & held[el[:, b]]
            held[el[both, 4 + m]] = True
    pick = np.nonzero(held)[0]
    if pick.size * dm < 6:
        pick = np.arange(3)
    return (pick[:, None] * dm + np.arange(dm)[None, :]).ravel().astype(np.int32)


# corner pairs of the mid-side nodes 4..9 of a quadratic tetrahedron, found from the coordinates of a straight-sided one
def _tet10_edges():
    nodes, el, _, _ = lr.single("C3D10")
    out = []
    for m in range(4, 10):
        pairs = [(a, b) for a in range(4) for b in range(a + 1, 4)
                 if np.allclose(nodes[el[0, m]], 0.5 * (nodes[el[0, a]] + nodes[el[0, b]]))]
        assert len(pairs) == 1
        out.append(pairs[0])
    return out


TET10_EDGES = _tet10_edges()


def check_plan(ctx, row, backend):
    """guards the inputs, not the kernels: the mesh still gives the band of the table"""
    plan = ctx.direct_plan()
    assert (plan["n"], plan["bandwidth"]) == (row.n, row.bw), (plan, row)
    assert row.T == -(-row.bw // NB) and row.P == -(-row.n // NB)
    if backend == "hip":
        assert plan["panels"] == row.P, (plan, row)


def _direct_solve(ctx, b_vec, x_vec):
    """Context.direct_solve, except that a refused solve hands its info back as well, under "status" / "message": the
    pivots are counted before the residual decides, and a wrong count is the better failure to read"""
    info = be.DirectInfo()
    rc = ctx.lib.femcy_direct_solve(ctx._h, int(b_vec), int(x_vec), C.byref(info))
    out = {k: getattr(info, k) for k, _ in be.DirectInfo._fields_ if k != "reserved"}
    out["status"], out["message"] = rc, ctx.lib.femcy_last_error().decode() if rc else ""
    return out


def _solve_variants(ctx, b, variants):
    """-> {variant: (info, x)}; the knob is back at -1 afterwards"""
    out = {}
    try:
        for var in variants:
            ctx.set_option(be.TUNE_DIRECT_UPDATE, var)
            ctx.upload(be.VEC_RESIDUAL, b)
            ctx.vector(be.VEC_X).fill(0.0)
            info = _direct_solve(ctx, be.VEC_RESIDUAL, be.VEC_X)
            assert np.array_equal(ctx.download(be.VEC_RESIDUAL), b)          # the right-hand side is left alone
            out[var] = (info, ctx.download(be.VEC_X))
    finally:
        ctx.set_option(be.TUNE_DIRECT_UPDATE, -1)
    return out


def variants_of(backend):
    return VARIANTS if backend == "hip" else (-1,)      # (the host backend has one elimination: the knob is a no-op there)


def manufactured(row, backend, host_err=None):
    """b = K x_true on the clamped mesh of `row`, every update variant: no refinement, no negative pivot, a residual at
    the sparse LU's level and an error at the level of the LU's and the host backend's (host_err: |x - x_true|_max of
    the host backend on the same mesh and x_true; None on the host backend itself).  -> the measured figures"""
    nodes, el, ELE = build(row)
    ctx = lc.make_ctx(nodes, el, ELE, backend)
    try:
        check_plan(ctx, row, backend)
        cons = clamped_dofs(nodes, el, ELE)
        ctx.assemble_K(-1)
        ctx.dirichlet_newton(cons, be.VEC_RESIDUAL)
        K = ctx.get_K_bsr().tocsr()
        x_true = np.random.default_rng(20).uniform(-1.0, 1.0, ctx.n)
        x_true[cons] = 0.0
        b = K @ x_true
        assert not b[cons].any()
        bmax = np.abs(b).max()
        x_lu = spl.spsolve(K.tocsc(), b)
        res_lu = np.abs(K @ x_lu - b).max() / bmax
        err_lu = np.abs(x_lu - x_true).max()
        assert err_lu <= 1e-9, err_lu                                        # input condition: the system is well posed
        sol = _solve_variants(ctx, b, variants_of(backend))
    finally:
        ctx.close()
    res_bound = max(100.0 * res_lu, row.n * 2.0 ** -53)
    # the device is held to the LU's and the host backend's error; the host backend, the yardstick of that bound, to what
    # the input condition asks of the LU (the two differ by the luck of the rounding: 1.6e-11 against 1.1e-12 at n = 3159)
    err_bound = 1e-9 if host_err is None else 10.0 * max(err_lu, host_err)
    xs = {v: x for v, (_, x) in sol.items()}
    worst = {"res": 0.0, "err": 0.0, "vdiff": 0.0, "res_lu": res_lu, "err_lu": err_lu}
    for var, (info, x) in sol.items():
        res = max(info["residual"], np.abs(K @ x - b).max() / bmax)
        err = np.abs(x - x_true).max()
        print(f"{row_id(row)} [{backend}, update {var}]: T {row.T}, P {row.P}, residual {res:.2e} (sparse LU {res_lu:.2e}, "
              f"bound {res_bound:.2e}), |x - x_true| {err:.2e} (sparse LU {err_lu:.2e}, host {host_err}, bound "
              f"{err_bound:.2e}), refinements {info['refinements']}")
        assert info["status"] == 0, (var, info)
        assert info["n"] == row.n and info["bandwidth"] == row.bw
        assert info["refinements"] == 0, (var, info)      # the LU stays 1e5 under the threshold: a factor that needs one is wrong
        assert info["negative_pivots"] == 0 and info["singular_at"] == 0, (var, info)
        assert res <= res_bound, (var, res, res_bound)
        assert err <= err_bound, (var, err, err_bound)
        worst["res"], worst["err"] = max(worst["res"], res), max(worst["err"], err)
    if backend == "hip":
        diff = {v: np.linalg.norm(xs[v] - xs[0]) / np.linalg.norm(xs[0]) for v in xs}
        worst["vdiff"] = max(diff.values())
        print(f"{row_id(row)}: variants against the VALU product {diff}")
        assert np.array_equal(xs[3], xs[1])               # the two-stream schedule: the same kernels on the same data
        for v in xs:
            assert diff[v] <= 1e-12, (v, diff)
        if row.T < MFMA_MIN_TILES:
            assert np.array_equal(xs[-1], xs[0])          # auto takes the VALU product on every panel
        else:                                             # auto = variant 1 on the panels with Tp >= 8 only: not bits
            assert np.linalg.norm(xs[-1] - xs[1]) <= 1e-12 * np.linalg.norm(xs[1])
    return worst


# ------------------------------------------------------------------------------------------------- inertia
INERTIA_MESHES = {"C3D4": ("C3D4", (3, 3, 10)), "C3D8": ("C3D8", (5, 5, 8)), "CPS4": ("CPS4", (40, 15))}
# (share of the nodes pushed, by how many mean edges): tests/test_gpu_direct.py's recipe for inverted elements, seed 11
CONFIGS = [(12, 0.8), (6, 0.8), (3, 1.0)]


def inertia_ids():
    return [(m, k) for m in INERTIA_MESHES for k in range(len(CONFIGS))]


def inertia(mesh, k, backend, host=None):
    """the displaced configuration CONFIGS[k] of INERTIA_MESHES[mesh]: negative pivots = negative eigenvalues, exactly,
    for every update variant.  host: (residual, |x - x_lu| / |x_lu|) of the host backend on the same configuration
    (None on the host backend itself, which has to solve it with a residual <= 1e-10).  -> the measured figures"""
    etype, cells = INERTIA_MESHES[mesh]
    share, amp = CONFIGS[k]
    nodes, el, ELE = lr.mesh(etype, cells)
    dm = ELE.dm
    ctx = lc.make_ctx(nodes, el, ELE, backend)
    try:
        rng = np.random.default_rng(11)
        h = np.linalg.norm(nodes[el[:, 0]] - nodes[el[:, 1]], axis=1).mean()
        u = np.zeros_like(nodes)
        pick = rng.choice(len(nodes), len(nodes) // share, replace=False)
        u[pick] = rng.standard_normal((pick.size, dm)) * amp * h
        ctx.upload(be.VEC_DOF, u.ravel())
        ctx.assemble_K(be.VEC_DOF)
        vol = ctx.gauss_field(be.GP_VOL).to_numpy()
        assert (vol < 0).any() and (vol > 0).any()
        b = rng.standard_normal(ctx.n)
        ctx.upload(be.VEC_RESIDUAL, b)
        ctx.dirichlet_newton(clamped_dofs(nodes, el, ELE), be.VEC_RESIDUAL)
        b = ctx.download(be.VEC_RESIDUAL)
        K = ctx.get_K_bsr().tocsr()
        ev = np.linalg.eigvalsh(K.toarray())
        gap = np.abs(ev).min() / np.abs(ev).max()
        assert gap >= 1e-10, gap                          # input condition: the count is no rounding matter
        negative = int((ev < 0).sum())
        assert negative > 0
        x_lu = spl.spsolve(K.tocsc(), b)
        res_lu = np.abs(K @ x_lu - b).max() / np.abs(b).max()
        sol = _solve_variants(ctx, b, variants_of(backend))
    finally:
        ctx.close()
    res_bound = 1e-10 if host is None else max(1e-11, 10.0 * host[0], 10.0 * res_lu)
    worst = {"res": 0.0, "err": 0.0, "negative": negative, "gap": gap, "refinements": 0}
    for var, (info, x) in sol.items():
        res = max(info["residual"], np.abs(K @ x - b).max() / np.abs(b).max())
        err = np.linalg.norm(x - x_lu) / np.linalg.norm(x_lu)
        print(f"{mesh} {CONFIGS[k]} [{backend}, update {var}]: n {info['n']}, bandwidth {info['bandwidth']}, "
              f"{info['negative_pivots']} negative pivots / {negative} negative eigenvalues (min |ev| / max |ev| {gap:.1e}), "
              f"residual {res:.2e} (sparse LU {res_lu:.2e}, host {host}), |x - x_lu| / |x_lu| {err:.2e}, "
              f"refinements {info['refinements']}")
        assert info["negative_pivots"] == negative, (var, info, negative)
        assert info["status"] == 0 and info["singular_at"] == 0, (var, info)
        assert res <= res_bound, (var, res, res_bound)
        if host is not None:
            assert err <= 10.0 * host[1], (var, err, host)
        worst["res"], worst["err"] = max(worst["res"], res), max(worst["err"], err)
        worst["refinements"] = max(worst["refinements"], info["refinements"])
    return worst


def host_figures(path):
    """what the device tests compare with, from the host backend: one .npz with |x - x_true|_max per row and
    (residual, |x - x_lu| / |x_lu|) per displaced configuration"""
    out = {}
    for row in ROWS:
        out["row/" + row_id(row)] = manufactured(row, "cpu")["err"]
    for mesh, k in inertia_ids():
        w = inertia(mesh, k, "cpu")
        out["inertia/%s/%d" % (mesh, k)] = np.array([w["res"], w["err"]])
    np.savez(path, **out)
