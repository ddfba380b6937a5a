"""Family, material and slice edges of the consistent tangent (FEMCY_OPT_TANGENT = 1: k_assemble_gather_consistent and
k_diag_from_rowsum in csrc/kernels_assembly.hip, kblock_consistent in csrc/element_math.hpp, the one-pass element sweep
k_geom<..., STRESS> with GEOM_DSDX | GEOM_F | GEOM_SIGMA | GEOM_FE, and the state the option leaves behind), written against
the C ABI (femcy_amd.backend.Context) like tests/asm_shapes.py, whose meshes, Layout, disp, ratio and rows it imports: the
host backend (tests/test_tangent_shapes_cpu.py, one child process with FEMCY_BACKEND=cpu) and the device
(tests/test_gpu_tangent_shapes.py) run the same functions.

The reference.  K_ref is the derivative of the element internal force f^e = sum_g grad N . sigma(F) vol (J = x^T dN, grad N
by the adjugate, vol = det J w, F from the reference configuration: element_pass(), the chain of asm_shapes.reference, to
which it is held bit for bit on the host) by complex-step differentiation in np.clongdouble: one imaginary perturbation of
local DOF k in every element at once is column k of every element tangent.  sigma is orc.cauchy_large; the plane-strain
neo-Hookean solid, which the oracle has in 3-D only, is its 3-D law on F embedded with F33 = 1, in-plane part
(tests/test_gpu_neohooke2d.py).  It shares no formula with kblock_consistent.  Next to every value stands the MAGNITUDE SUM
of the closed form element_math.hpp documents, vol (ga_j c_ijkl gb_l + delta_ik ga . sigma . gb): every term by its
magnitude, |b| = |F| |F|^T, J + 1 for |J - 1|, 2 J + 1 for |2 J - 1|, sigma by the magnitude sum of its own terms, plus what
the roundings of vol and grad N move the sum by (Avol, Adsdx of asm_shapes), and Arow (the off-diagonal magnitudes of the
row) on the diagonal blocks where the diagonal is taken from the row sum.  Then
    |K_ij - K_ref_ij| <= 4 C_TAN 2^-53 A_ij        for every stored scalar entry; A_ij = 0: exactly 0.
Before every assembly that is checked the reference matrix (OPT_TANGENT = 0) is assembled at the other displacement.
dsdx, vol, F, sigma and the nodal force follow asm_shapes' scheme, with constants measured on these rows and scales (the
fans are thinner at scale 0.05 than at asm_shapes' 0.002, and C_FORCE carries another cancellation); the neo-Hookean
sigma = 2 C1 / J (b - I) + 2 D1 (J - 1) I has its own magnitude sum, to first order in the rounding of F like asm_shapes'
Asig: (|F| AF^T + AF |F|^T) / 2 + I for |b - I|, the magnitude sum of det AF, plus 1, for |J - 1|.  The elastic energy (the
state checks) is held to 2^-53 (4 C_ENERGY sum Apsi Avol + n sum |psi vol|): the density's magnitude sum (the Green strain
from |F|; I1 + 3 + 2 |ln J| and (J + 1)^2), and the worst case of any summation order of the n Gauss-point terms.

TABLE holds the rows of asm_shapes the tangent is assembled on, each with the edges of k_assemble_gather_consistent it is
there for as a predicate over the restated Layout (the last workgroup of 256 lanes holds stored_rows % 4 slice rows;
padding positions, tpos = -1; mirrored stores into another slice and another sort window; blocks of 0, 1, 2 and >= 16
contributors; slices of loose rows only, whose row sum is empty; 1, 3, 4, 6 and 8 Gauss points -- CPS8 integrates with 2 x 2
points here, no family has 9).  SWEEP holds every family at 1, 63 .. 257 elements for the one-pass sweep: a family's rows are
the first elements of one plate and share its element references.  STATE names the rows of check_state.

Measured constants (x86-64 long double; the float64 run of the closed form, or of the restatement, against the long-double
complex step / restatement, worst over TABLE at both scales, STATE at its scales and SWEEP at 0.05; the tests allow 4 x).
Last column: the worst value the device tests print (pytest -s).
    TAN_STVK    worst |K - K_ref|_ij / (eps A_ij), Saint Venant-Kirchhoff branch (F's own        10.24     7.27
                rounding, eps AF, is not among the magnitude terms: that is what it carries)
    TAN_NEO     the same, neo-Hookean branch                                                     0.310     0.252
    CLOSED      the closed form in LONG DOUBLE against the complex step, both branches: an       0.119     -
                error in the magnitude terms or in the closed form would show here as >> 1;
                what is left is the float64 rounding of c11 against lambda + 2 mu in the
                material's table (the force reads c11, the tangent lambda and mu)
    DSDX        worst |dsdx - ref| / (eps A_dsdx)   (valence-cps3 at 0.05: det J cancels)       238.6     18.5
    VOL         worst |vol - ref| / (eps A_vol)                                                  1.49      0.680
    F           worst |F - F_ref| / (eps A_F)                                                    1.44      1.37
    SIG_STVK    worst |sigma - ref| / (eps A_sigma), S = C : E                                   0.628     0.578
    SIG_NEO     the same, neo-Hookean                                                            1.14      1.06
    FORCE_STVK  worst |f - f_ref|_i / (eps A_f_i)                                                4898      2358
    FORCE_NEO   the same, neo-Hookean                                                            4505      2329
    ENERGY      worst |E - E_ref| / (eps sum Apsi Avol)                                          0.0735    0.0048
    asm_shapes' C_ASM / C_CUBIC hold the OPT_TANGENT = 0 matrix on these rows and scales (0.951 measured against 1.40;
    device 0.276); the product check (pcg_shapes.C_PROD): on the device at most 0.024 of its bound
tests/test_tangent_shapes_cpu.py measures every one of them again and fails if one has moved, holds element_pass to
asm_shapes.reference bit for bit, and applies the mutations of mutations() to the long-double closed form: each moves a
stored entry by more than 100 x the bound allowed there (the least visible: 9.5e7 x, c3d10-fans)."""
import collections

import numpy as np

from femcy_amd import backend as be
from femcy_amd.material_zoo import LinearIsotropic, LinearIsotropicPlaneStrain, NeoHookean, NeoHookeanPlaneStrain
from oracle import femcy_oracle as orc

import asm_shapes as ash
import loads_reference as lr

LD, EPS, SLICE = ash.LD, ash.EPS, ash.SLICE
SCALES = (0.0, 0.05)
STATE_SCALES = (0.05, 0.03)                                        # u1, u2 of check_state
NEO = 3                                                           # FEMCY_MAT_NEOHOOKE
KINDS = {0: "lin3d", 1: "pstrain", NEO: "neohooke"}
MATS = ("stvk", "neo")
# (measured: the docstring; device column: tests/test_gpu_tangent_shapes.py -s)
C = {"TAN_STVK": 10.24, "TAN_NEO": 0.310, "CLOSED": 0.119, "DSDX": 238.6, "VOL": 1.49, "F": 1.44, "SIG_STVK": 0.628, "SIG_NEO": 1.14,
     "FORCE_STVK": 4898.0, "FORCE_NEO": 4505.0, "ENERGY": 0.0735}


def materials(dm):
    if dm == 3:
        return {"stvk": LinearIsotropic(2.0e5, 0.3), "neo": NeoHookean(3.85e4, 8.3e4)}
    return {"stvk": LinearIsotropicPlaneStrain(2.0e5, 0.3), "neo": NeoHookeanPlaneStrain(3.85e4, 8.3e4)}


# ------------------------------------------------------------------------------------------------------- the reference
def _embed(F):
    """plane strain: F with F33 = 1"""
    F3 = np.zeros(F.shape[:-2] + (3, 3), dtype=F.dtype)
    F3[..., :2, :2] = F
    F3[..., 2, 2] = 1.0
    return F3


def cauchy(mat, F):
    om = orc.Material(KINDS[mat.kind], tuple(float(v) for v in mat.params))
    if mat.kind == NEO and F.shape[-1] == 2:
        return orc.cauchy_large(om, _embed(F))[..., :2, :2]
    return orc.cauchy_large(om, F)


def energy_density(mat, F):
    om = orc.Material(KINDS[mat.kind], tuple(float(v) for v in mat.params))
    return orc.energy_density(om, _embed(F) if mat.kind == NEO and F.shape[-1] == 2 else F)


def element_pass(X, U, dN, w, dsdX, mat):
    """asm_shapes.reference's chain for element coordinates X and displacements U [ne, npe, dm] (U may be complex)
    -> dsdx, vol, F, sigma, f^e"""
    dm = X.shape[-1]
    det, adj = ash._det_inv(np.einsum("eai,gaj->egij", X + U, dN))
    dsdx = np.einsum("gak,egkj->egaj", dN, adj) / det[..., None, None]
    vol = det * w
    F = np.einsum("eai,egaj->egij", U, dsdX) + np.eye(dm, dtype=X.dtype)
    sig = cauchy(mat, F)
    return dsdx, vol, F, sig, np.einsum("egaj,egji,eg->eai", dsdx, sig, vol)


def complex_step(X, U, dN, w, dsdX, mat, h=1.0e-30):
    """-> d f^e[a, i] / d u^e[b, k] as [ne, npe, npe, dm, dm] (e, a, b, i, k)"""
    ne, npe, dm = X.shape
    Ke = np.empty((ne, npe, npe, dm, dm), X.dtype)
    for b in range(npe):
        for k in range(dm):
            Up = U.astype(np.clongdouble if X.dtype == LD else np.complex128)
            Up[:, b, k] += 1j * h
            Ke[:, :, b, :, k] = element_pass(X, Up, dN, w, dsdX, mat)[4].imag / h
    return Ke


def kernel_form(ga, gb, vol, b, sig, J, mat, mag=False, swap=False, geometric=True):
    """the closed form at kblock_consistent, per Gauss point: vol (ga_j c_ijkl gb_l + delta_ik ga . sigma . gb) as
    [e, g, a, b, i, k].  mag: the arguments are magnitudes, every term is added, J - 1 -> J + 1, 2 J - 1 -> 2 J + 1"""
    dm = ga.shape[-1]
    eye = np.eye(dm, dtype=vol.dtype)
    s = 1.0 if mag else -1.0
    geo = np.einsum("egai,egij,egbj->egab", ga, sig, gb)
    if not geometric:
        geo = 0 * geo
    if mat.kind == NEO:
        C1, D1 = (float(v) for v in mat.params)
        mu_s, lam_s = 2.0 * C1 / J + s * 2.0 * D1 * (J + s), 2.0 * D1 * (2.0 * J + s)
        if swap:
            mu_s, lam_s = lam_s, mu_s
        ab = np.einsum("egai,egbi->egab", ga, gb)
        out = (np.einsum("eg,egai,egbk->egabik", lam_s, ga, gb) + np.einsum("eg,egbi,egak->egabik", mu_s, gb, ga)
               + np.einsum("egab,ik->egabik", mu_s[..., None, None] * ab + geo, eye))
        return out * vol[..., None, None, None, None]
    C = np.asarray(mat.C, np.float64)
    lam, mu = (C[-1, -1], C[0, 1]) if swap else (C[0, 1], C[-1, -1])          # launch_assemble: C01, C(shear, shear)
    bga, bgb = np.einsum("egij,egaj->egai", b, ga), np.einsum("egij,egbj->egbi", b, gb)
    sab = np.einsum("egai,egbi->egab", ga, bgb)
    out = (lam * np.einsum("egai,egbk->egabik", bga, bgb)
           + mu * (np.einsum("egab,egik->egabik", sab, b) + np.einsum("egbi,egak->egabik", bgb, bga))) / J[..., None, None, None, None]
    return (out + np.einsum("egab,ik->egabik", geo, eye)) * vol[..., None, None, None, None]


def _green_mag(F3):
    """Voigt magnitudes of E = (F^T F - I) / 2 (engineering shear), every term added"""
    a = np.abs(F3)
    Em = (np.einsum("egki,egkj->egij", a, a) + np.eye(3, dtype=F3.dtype)) / 2
    return np.stack([Em[..., 0, 0], Em[..., 1, 1], Em[..., 2, 2], 2 * Em[..., 0, 1], 2 * Em[..., 2, 0], 2 * Em[..., 1, 2]], -1)


def energy_mag(mat, F):
    F3 = F if F.shape[-1] == 3 else _embed(F)
    J = np.abs(ash._det_inv(F)[0])
    if mat.kind == NEO:
        C1, D1 = (float(v) for v in mat.params)
        return C1 * ((np.abs(F3) ** 2).sum(axis=(-1, -2)) + 3.0 + 2.0 * np.abs(np.log(J))) + D1 * (J + 1.0) ** 2
    om = orc.Material(KINDS[mat.kind], tuple(float(v) for v in mat.params))
    C6 = np.abs(om.C if mat.kind == 0 else om.C_6x6)
    ev = _green_mag(F3)
    return np.einsum("egi,ij,egj->eg", ev, C6, ev) / 2


Elem = collections.namedtuple("Elem", "dsdx Adsdx vol Avol F AF sig Asig fe afe Ke Kg Ae psi Apsi base")
Ref = collections.namedtuple("Ref", "K Kc A Arow dsdx Adsdx vol Avol F AF sig Asig f Af E AE Esum elem slot")


def element_reference(lay, nodes, el, ELE, mats, mat, u, dt=LD, base=None):
    """everything per element in dtype dt; Ke (the complex step) in long double only.  base: asm_shapes.reference of the
    linear material at this displacement, whose dsdx, vol, F and magnitude sums hold for every material"""
    m = mats[mat]
    if base is None:
        base = ash.reference(lay, nodes, el, ELE, mats["stvk"], u, dt, force=True)
    dsdx, vol, F = base.dsdx, base.vol, base.F
    aF = np.abs(F)
    J = ash._det_inv(F)[0]
    assert (J > 0).all() and (vol / ELE.tables()["w"].astype(dt) > 0).all(), "det F, det J > 0 at every Gauss point"
    dm = lay.dm
    if m.kind == NEO:
        C1, D1 = (float(v) for v in m.params)
        sig = cauchy(m, F)
        # every term by its magnitude, to first order in the rounding of F (eps AF, AF >= |F|: asm_shapes' Asig)
        Jm = ash._det_inv(base.AF, mag=True)[0]
        Asig = (2.0 * C1 / J)[..., None, None] * ((np.einsum("egik,egjk->egij", aF, base.AF) + np.einsum("egik,egjk->egij", base.AF, aF)) / 2
                                                  + np.eye(dm, dtype=dt)) + (2.0 * D1 * (Jm + 1.0))[..., None, None] * np.eye(dm, dtype=dt)
        fe = np.einsum("egaj,egji,eg->eai", dsdx, sig, vol)
    else:
        sig, Asig, fe = base.sig, base.Asig, base.fe
    afe = np.einsum("egaj,egji,eg->eai", np.abs(dsdx), np.abs(sig), np.abs(vol))
    b = np.einsum("egik,egjk->egij", F, F)
    Kg = kernel_form(dsdx, dsdx, vol, b, sig, J, m)
    ag, ab = np.abs(dsdx), np.einsum("egik,egjk->egij", aF, aF)
    Ae = (kernel_form(ag, ag, base.Avol, ab, Asig, J, m, mag=True) + kernel_form(base.Adsdx, ag, np.abs(vol), ab, Asig, J, m, mag=True)
          + kernel_form(ag, base.Adsdx, np.abs(vol), ab, Asig, J, m, mag=True)).sum(axis=1)
    Ke = None
    if dt is LD:
        t = ELE.tables()
        dN, w = t["dN"].astype(dt), t["w"].astype(dt)
        X, U = nodes.astype(dt)[el], u.reshape(nodes.shape).astype(dt)[el]
        d0, a0 = ash._det_inv(np.einsum("eai,gaj->egij", X, dN))
        dsdX = np.einsum("gak,egkj->egaj", dN, a0) / d0[..., None, None]
        Ke = complex_step(X, U, dN, w, dsdX, m)
    return Elem(dsdx, base.Adsdx, vol, base.Avol, F, base.AF, sig, Asig, fe, afe, Ke, Kg, Ae, energy_density(m, F), energy_mag(m, F), base)


def assemble_reference(lay, el, E):
    """the element reference E (of at least lay.ne elements, the first lay.ne are taken) summed into lay's pattern"""
    ne, dt = lay.ne, E.vol.dtype
    red = ash.reducer(lay, el, dt)
    cut = lambda v: None if v is None else v[:ne]
    E = Elem(*(cut(v) for v in E[:-1]), E.base)
    Kc, A = red(E.Kg.sum(axis=1)), red(E.Ae)
    K = red(E.Ke) if E.Ke is not None else None
    f, Af = np.zeros((lay.nn, lay.dm), dt), np.zeros((lay.nn, lay.dm), dt)
    np.add.at(f, el.ravel(), E.fe.reshape(-1, lay.dm))
    np.add.at(Af, el.ravel(), E.afe.reshape(-1, lay.dm))
    return Ref(K, Kc, A, ash.row_sums(lay, A), E.dsdx, E.Adsdx, E.vol, E.Avol, E.F, E.AF, E.sig, E.Asig, f, Af,
               (E.psi * E.vol).sum(), (E.Apsi * E.Avol).sum(), np.abs(E.psi * E.vol).sum(), E, red.slot)


# ------------------------------------------------------------------------------------------------------------ the tables
def stored_rows(y):
    return y.stored // SLICE


def _padding(y):
    """a storage position that holds no block (tpos == -1)"""
    return y.stored > len(y.brow)


T = collections.namedtuple("T", "name edge why")
# (y: the restated Layout, g: Gauss points per element)
TABLE = [
    T("c3d10-graded-loose", lambda y, g: g == 4 and stored_rows(y) % 4 == 0 and _padding(y) and ash._cross(y, SLICE)
      and y.sigma < y.nn and ash._cross(y, y.sigma) and 0 in y.contributors,
      "C3D10 (4 Gauss points): full last workgroup, padding positions, mirrored stores into another slice and another sort "
      "window, loose rows (an empty row sum) inside slices of coupled ones"),
    T("c3d10-tail-63", lambda y, g: stored_rows(y) % 4 == 1 and ash._loose_slice(y) and y.L[-1] == 1,
      "a last workgroup of one slice row; slices made only of loose rows"),
    T("c3d10-fans", lambda y, g: {0, 1, 2} <= set(y.contributors.tolist()) and y.contributors.max() >= 16,
      "blocks with 0, 1, 2 and 16 contributors"),
    T("c3d4-graded", lambda y, g: g == 1 and stored_rows(y) % 4 == 2 and ash._cross(y, SLICE) and {1, 2, 3} <= set(y.contributors.tolist()),
      "C3D4 (1 Gauss point): a last workgroup of two slice rows, mirrored stores across slices"),
    T("c3d4-fans", lambda y, g: y.contributors.max() >= 43 and 0 in y.cnt, "blocks with 20 .. 43 contributors, rows with none"),
    T("c3d8-graded", lambda y, g: g == 8 and y.dm == 3, "C3D8: 8 Gauss points"),
    T("c3d6-graded", lambda y, g: g == 6 and y.dm == 3, "C3D6: 6 Gauss points"),
    T("cps3-fan-65", lambda y, g: g == 1 and y.dm == 2 and y.nslices == 1 and y.contributors.max() == 35,
      "2-D, 1 Gauss point: one slice, a block of 35 contributors"),
    T("cps4-graded", lambda y, g: g == 4 and y.dm == 2 and stored_rows(y) % 4 == 3,
      "CPS4 (4 Gauss points): a last workgroup of three slice rows"),
    T("cps6-graded", lambda y, g: g == 3 and stored_rows(y) % 4 == 3 and ash._cross(y, 64), "CPS6 (3 Gauss points), windows of 64"),
    T("cps8-graded", lambda y, g: g == 4 and y.npe == 8 and stored_rows(y) % 4 == 2, "CPS8 (4 Gauss points, 8 nodes)"),
    T("valence-cps3", lambda y, g: {0, 1, 2} <= set(y.contributors.tolist()) and y.contributors.max() >= 16 and y.dm == 2,
      "2-D blocks with 0, 1, 2 and 65 contributors"),
    T("valence-c3d4", lambda y, g: {0, 1, 2} <= set(y.contributors.tolist()) and y.contributors.max() >= 16 and y.dm == 3,
      "3-D blocks with 0, 1, 2 and 65 contributors"),
]
NES = (1, 63, 64, 65, 255, 256, 257)
FIRST = dict(ash.FIRST, C3D6=(5, 4, 7), CPS3=(12, 11), CPS4=(13, 20), CPS6=(12, 11), CPS8=(13, 20))     # plates of >= 257 elements


def chunk(wg):
    """k_geom's staging of a record of wg = npe dm doubles per element (kernels_assembly.hip: STAGE, CHK): whole up to 16,
    else in chunks of the first of 16, 15, 12, 9, 8 that divides it"""
    return wg if wg <= 16 else next(c for c in (16, 15, 12, 9, 8) if wg % c == 0)


# (nn, ne, nslices, stored_blocks, max_row_blocks) of the sweep rows this file adds
PINS = {
    "geom-c3d6-1": (240, 1, 4, 576, 6), "geom-c3d6-63": (240, 63, 4, 2112, 21), "geom-c3d6-64": (240, 64, 4, 2112, 21),
    "geom-c3d6-65": (240, 65, 4, 2112, 21), "geom-c3d6-255": (240, 255, 4, 4160, 21), "geom-c3d6-256": (240, 256, 4, 4160, 21),
    "geom-c3d6-257": (240, 257, 4, 4160, 21),
    "geom-cps3-1": (156, 1, 3, 320, 3), "geom-cps3-63": (156, 63, 3, 704, 7), "geom-cps3-64": (156, 64, 3, 704, 7),
    "geom-cps3-65": (156, 65, 3, 704, 7), "geom-cps3-255": (156, 255, 3, 1216, 7), "geom-cps3-256": (156, 256, 3, 1216, 7),
    "geom-cps3-257": (156, 257, 3, 1216, 7),
    "geom-cps4-1": (294, 1, 5, 512, 4), "geom-cps4-63": (294, 63, 5, 1152, 9), "geom-cps4-64": (294, 64, 5, 1152, 9),
    "geom-cps4-65": (294, 65, 5, 1152, 9), "geom-cps4-255": (294, 255, 5, 2688, 9), "geom-cps4-256": (294, 256, 5, 2688, 9),
    "geom-cps4-257": (294, 257, 5, 2688, 9),
    "geom-cps6-1": (575, 1, 9, 896, 6), "geom-cps6-63": (575, 63, 9, 2816, 16), "geom-cps6-64": (575, 64, 9, 2816, 16),
    "geom-cps6-65": (575, 65, 9, 2816, 16), "geom-cps6-255": (575, 255, 9, 6464, 19), "geom-cps6-256": (575, 256, 9, 6464, 19),
    "geom-cps6-257": (575, 257, 9, 6464, 19),
    "geom-cps8-1": (847, 1, 14, 1344, 8), "geom-cps8-63": (847, 63, 14, 4160, 21), "geom-cps8-64": (847, 64, 14, 4160, 21),
    "geom-cps8-65": (847, 65, 14, 4160, 21), "geom-cps8-255": (847, 255, 14, 12608, 21), "geom-cps8-256": (847, 256, 14, 13056, 21),
    "geom-cps8-257": (847, 257, 14, 13056, 21),
}


def _sweep_row(et, ne):
    name = "geom-%s-%d" % (et.lower(), ne)
    got = [r for r in ash.ROWS if r.name == name]
    if got:
        return got[0]
    return ash.Row(name, ("first", (et, FIRST[et], ne)), (0, 0), 4096, (ash.G,), ash.AUTO, (), (), PINS[name],
                   (lambda ne: lambda y: y.ne == ne and (ne > 1 or 1 in y.cnt))(ne),
                   "k_geom, one pass: %d elements (the last workgroup of 256 threads full, short by one, one over)" % ne)


SWEEP = [_sweep_row(et, ne) for et in ("C3D4", "C3D10", "C3D8", "C3D6", "CPS3", "CPS4", "CPS6", "CPS8") for ne in NES]
STATE = ("c3d4-graded", "cps8-graded")
ROWS = {t.name: next(r for r in ash.ROWS if r.name == t.name) for t in TABLE}
ROWS.update({r.name: r for r in SWEEP})


# ------------------------------------------------------------------------------------------------------------- a case
_FAMILY = {}                                                       # (etype, mat, scale, dtype) -> Elem of the first 257 elements


class Case:
    """one row on one backend: mesh, restated layout, references on demand, contexts on demand"""

    def __init__(self, row, backend):
        self.row, self.backend = row, backend
        self.nodes, self.el, self.ELE = ash.build(row)
        self.lay = ash.Layout(self.nodes, self.el, row.sigma)
        self.ngp = len(self.ELE.tables()["w"])
        self.mats = materials(self.lay.dm)
        self.us = {s: ash.disp(self.nodes, s) for s in SCALES + STATE_SCALES}
        self._refs, self._base, self._ctx = {}, {}, None
        self.x = np.random.default_rng(5).standard_normal(self.lay.nn * self.lay.dm) + 0.25

    def context(self, mat="stvk"):
        """a fresh context with the pattern built"""
        ctx = be.Context(0, backend=self.backend)
        ctx.set_option(be.OPT_NODE_ORDER, 0)                       # the caller's numbering: what Layout restates
        ctx.set_option(be.OPT_SELL_SIGMA, self.row.sigma)
        ctx.set_mesh(self.nodes, self.el)
        ctx.set_element(self.ELE)
        ctx.set_material(self.mats[mat])
        self.info = ctx.build_pattern()
        return ctx

    @property
    def ctx(self):
        if self._ctx is None:
            self._ctx = self.context()
        return self._ctx

    def base(self, scale, dt=LD):
        if (scale, dt) not in self._base:
            self._base[scale, dt] = ash.reference(self.lay, self.nodes, self.el, self.ELE, self.mats["stvk"], self.us[scale], dt,
                                                  force=True)
        return self._base[scale, dt]

    def linear(self, mat, scale):
        """asm_shapes.reference of the OPT_TANGENT = 0 matrix with this material's constant C"""
        if mat == "stvk":
            return self.base(scale)
        if ("lin", mat, scale) not in self._base:
            self._base["lin", mat, scale] = ash.reference(self.lay, self.nodes, self.el, self.ELE, self.mats[mat], self.us[scale],
                                                          LD, force=False)
        return self._base["lin", mat, scale]

    def elem(self, mat, scale, dt=LD):
        if self.row.mesh[0] != "first":
            return element_reference(self.lay, self.nodes, self.el, self.ELE, self.mats, mat, self.us[scale], dt, self.base(scale, dt))
        et, cells, _ = self.row.mesh[1]                            # the rows of a family share its first 257 elements
        key = (et, mat, scale, dt)
        if key not in _FAMILY:
            nodes, el, ELE = ash.build(self.row._replace(mesh=("first", (et, cells, max(NES)))))
            assert np.array_equal(nodes, self.nodes)
            bkey = (et, None, scale, dt)
            if bkey not in _FAMILY:
                _FAMILY[bkey] = ash.reference(ash.Layout(nodes, el, self.row.sigma), nodes, el, ELE, self.mats["stvk"],
                                              self.us[scale], dt, force=True)
            _FAMILY[key] = element_reference(ash.Layout(nodes, el, self.row.sigma), nodes, el, ELE, self.mats, mat,
                                             self.us[scale], dt, _FAMILY[bkey])
        return _FAMILY[key]

    def ref(self, mat, scale, dt=LD):
        key = (mat, scale, dt)
        if key not in self._refs:
            self._refs[key] = assemble_reference(self.lay, self.el, self.elem(mat, scale, dt))
        return self._refs[key]

    def K(self, ctx=None):
        Kb = (ctx or self.ctx).get_K_bsr()
        assert np.array_equal(Kb.indices, self.lay.bcol) and np.array_equal(np.diff(Kb.indptr), self.lay.rowlen)
        return Kb.data.copy()

    def close(self):
        if self._ctx is not None:
            self._ctx.close()


_CASES = collections.OrderedDict()


def case(name, backend):
    key = (name, backend)
    if key not in _CASES:
        while len(_CASES) >= 1:
            _CASES.popitem(last=False)[1].close()
        _CASES[key] = Case(ROWS[name], backend)
    return _CASES[key]


WORST = collections.defaultdict(float)                             # constant -> worst ratio of this process's checks


def _note(worst):
    for k, v in worst.items():
        WORST[k] = max(WORST[k], v)
    return worst


def _held(got, ref, scale, const, what):
    r, k = ash.ratio(got, ref, scale)
    assert r <= 4.0 * const, (what, "entry", k, "ratio", r, "allowed", 4.0 * const)
    return r


# -------------------------------------------------------------------------------------------------------------- checks
def check_table(name):
    """no library: the pins and the edge of the row"""
    row = ROWS[name]
    nodes, el, ELE = ash.build(row)
    y = ash.Layout(nodes, el, row.sigma)
    assert (y.nn, y.ne, y.nslices, y.stored, y.max_row) == row.pins, ((y.nn, y.ne, y.nslices, y.stored, y.max_row), name)
    assert row.edge(y), (name, row.why)
    g = len(ELE.tables()["w"])
    for t in TABLE:
        if t.name == name:
            assert t.edge(y, g), (name, t.why)
    if row.mesh[0] == "first":
        assert len(lr.mesh(row.mesh[1][0], row.mesh[1][1])[1]) >= max(NES)
    return y, g


def check_edge(name, backend):
    """the restatement against the library, and the edges the row exists for"""
    c = case(name, backend)
    y, g = check_table(name)
    info = c.ctx.pattern_info()
    assert (info.n, info.nnzb, info.max_row_blocks) == (y.nn * y.dm, len(y.brow), y.max_row)
    if backend == "hip":
        assert (info.nslices, info.stored_blocks) == (y.nslices, y.stored)
    assert c.ngp == c.ctx.nGP == g


def _mirror(y):
    return np.searchsorted(y.brow * y.nn + y.bcol, y.bcol * y.nn + y.brow)


def _tangent(c, ctx, mat, scale, worst, what):
    """K of the context against the tangent reference; -> (K, the magnitudes its bound uses)"""
    ref = c.ref(mat, scale)
    used = ctx.assembly_used()
    assert used == (ash.SR if c.backend == "hip" else ash.A), (what, ash.NAMES.get(used, used))
    K = c.K(ctx)
    Aerr = ref.Arow if used == ash.SR else ref.A
    r, k = ash.ratio(K, ref.K, Aerr)
    y = c.lay
    worst["TAN_" + mat.upper()] = max(worst.get("TAN_" + mat.upper(), 0.0), r)
    assert r <= 4.0 * C["TAN_" + mat.upper()], (what, "block (%d, %d) entry %d" % (y.brow[k // y.dm ** 2], y.bcol[k // y.dm ** 2],
                                                                                    k % y.dm ** 2), r, 4.0 * C["TAN_" + mat.upper()])
    if c.backend == "hip":                                        # the mirrored stores: K_ba is K_ab^T bit for bit (a diagonal
        off = y.brow != y.bcol                                    # block is a row sum, symmetric within its bound above)
        assert np.array_equal(K[_mirror(y)][off], np.swapaxes(K, 1, 2)[off]), what
    return K, Aerr


def _linear_bound(c, used, base):
    """constant and magnitudes of the OPT_TANGENT = 0 matrix in the mode that ran (asm_shapes.check_assembly)"""
    const = ash.C_CUBIC if used in (ash.R2, ash.R4) else ash.C_ASM
    return const, (base.Arow if used in ash.ROWSUM_MODES else base.A)


def check_tangent(name, backend):
    """both materials, both displacements: assembly_used(), the entry-wise bound, exact symmetry, one product, a second
    assembly bit-equal to the first, and at u = 0 the linear material's tangent against the OPT_TANGENT = 0 matrix"""
    c = case(name, backend)
    ctx, worst = c.ctx, {"product": 0.0}
    try:
        for mat in MATS:
            ctx.set_material(c.mats[mat])
            for scale in SCALES:
                what = (name, mat, scale)
                other = SCALES[1] if scale == SCALES[0] else SCALES[0]

                def assemble():
                    ctx.set_option(be.OPT_TANGENT, 0)               # K then holds another state's values of another matrix
                    ctx.upload(be.VEC_DOF, c.us[other])
                    ctx.assemble_K(be.VEC_DOF)
                    ctx.set_option(be.OPT_TANGENT, 1)
                    ctx.upload(be.VEC_DOF, c.us[scale])
                    ctx.assemble_K(be.VEC_DOF)
                assemble()
                K1, Aerr = _tangent(c, ctx, mat, scale, worst, what)
                worst["product"] = max(worst["product"], ash._product(c, c.ref(mat, scale), Aerr, C["TAN_" + mat.upper()], what))
                assemble()
                K2 = c.K()
                assert np.array_equal(K1, K2), (what, "the second assembly differs in", int((K1 != K2).sum()), "entries")
                if scale == 0.0 and mat == "stvk":
                    ctx.set_option(be.OPT_TANGENT, 0)
                    ctx.assemble_K(be.VEC_DOF)
                    const, A0 = _linear_bound(c, ctx.assembly_used(), c.base(scale))
                    bad = np.abs(K1.astype(LD) - c.K()) > 4.0 * EPS * (C["TAN_" + mat.upper()] * Aerr + const * A0)
                    assert not bad.any(), (what, "differs from the reference's matrix in", int(bad.sum()), "entries")
    finally:
        ctx.set_option(be.OPT_TANGENT, 0)
        ctx.set_material(c.mats["stvk"])
    print(f"{name} [{backend}]: tangent, worst ratios to eps A {({k: round(v, 3) for k, v in worst.items()})} "
          f"(allowed {4 * C['TAN_STVK']:.2f} / {4 * C['TAN_NEO']:.2f}; product as a share of its bound)")
    return _note(worst)


def _fields(c, ctx, mat, ref, worst, what, stress=True):
    """the Gauss-point fields of the context against the reference"""
    rows = [("DSDX", be.GP_DSDX, ref.dsdx, ref.Adsdx), ("VOL", be.GP_VOL, ref.vol, ref.Avol)]
    if stress:
        rows += [("F", be.GP_F, ref.F, ref.AF), ("SIG_" + mat.upper(), be.GP_SIGMA, ref.sig, ref.Asig)]
    out = {}
    for cn, which, rf, sc in rows:
        out[which] = ctx.gauss_field(which).to_numpy()
        worst[cn] = max(worst.get(cn, 0.0), _held(out[which], rf, sc, C[cn], what + (cn,)))
    return out


def _force(c, ctx, mat, ref, worst, what):
    f = ctx.download(be.VEC_FORCE).reshape(-1, c.lay.dm)
    cn = "FORCE_" + mat.upper()
    worst[cn] = max(worst.get(cn, 0.0), _held(f, ref.f, ref.Af, C[cn], what + (cn,)))
    return f


def check_sweep(name, backend):
    """one residual_and_K with the tangent on at scale 0.05 -- k_geom<STRESS> with DSDX | F | SIGMA | FE in ONE launch --
    against the reference: dsdx, vol, F, sigma of every element and Gauss point, the nodal force, K; then the lazy split
    (the tangent off) on a fresh context, bit-equal in dsdx, vol, the force and, once the getters materialise them, F
    and sigma"""
    c = case(name, backend)
    scale, worst = SCALES[1], {}
    assert c.row.edge(c.lay) and c.lay.ne in NES 
    for mat in MATS:
        what, ref = (name, mat), c.ref(mat, scale)
        got = {}
        for tangent in (1, 0):
            ctx = c.context(mat)
            try:
                ctx.set_option(be.OPT_TANGENT, tangent)
                ctx.upload(be.VEC_DOF, c.us[scale])
                ctx.vector(be.VEC_FORCE).fill(np.nan)
                ctx.residual_and_K(be.VEC_DOF, be.VEC_FORCE)
                if tangent:
                    fields = _fields(c, ctx, mat, ref, worst, what)
                    got = dict(fields, f=_force(c, ctx, mat, ref, worst, what))
                    _tangent(c, ctx, mat, scale, worst, what)
                else:
                    for which in (be.GP_DSDX, be.GP_VOL, be.GP_F, be.GP_SIGMA):       # (F, sigma: materialised here)
                        assert np.array_equal(ctx.gauss_field(which).to_numpy(), got[which]), (what, "lazy split, field", which)
                    assert np.array_equal(ctx.download(be.VEC_FORCE).reshape(-1, c.lay.dm), got["f"]), (what, "lazy split, force")
            finally:
                ctx.close()
    print(f"{name} [{backend}]: one-pass sweep, worst ratios {({k: round(v, 3) for k, v in worst.items()})}")
    return _note(worst)


def _energy(c, ctx, mat, ref, u, worst, what):
    ctx.upload(be.VEC_DOF, u)
    E = ctx.elastic_energy(be.VEC_DOF)
    n = ref.vol.size
    err = abs(LD(E) - ref.E)
    worst["ENERGY"] = max(worst.get("ENERGY", 0.0), float(err / (EPS * ref.AE)))
    assert err <= EPS * (4.0 * C["ENERGY"] * ref.AE + n * ref.Esum), (what, "energy", E, float(ref.E))
    return E


def _read(c, ctx, mat, scale_f, scale_K, scale_gp, tangent, worst, what):
    """everything femcy.h defines after a step: the force (of scale_f), K (of scale_K; tangent: which matrix), F and sigma
    and the geometry (scale_gp for F / sigma, scale_K for dsdx / vol), the energy at the state of the geometry"""
    out = {}
    if scale_f is not None:
        out["f"] = _force(c, ctx, mat, c.ref(mat, scale_f), worst, what)
    if scale_K is not None:
        if tangent:
            out["K"] = _tangent(c, ctx, mat, scale_K, worst, what)[0]
        else:
            lin = c.linear(mat, scale_K)
            const, A0 = _linear_bound(c, ctx.assembly_used(), lin)
            out["K"] = c.K(ctx)
            worst["ASM"] = max(worst.get("ASM", 0.0), _held(out["K"], lin.K, A0, const, what + ("K",)))
    geo = c.ref(mat, scale_K if scale_K is not None else scale_f)
    out.update(_fields(c, ctx, mat, geo, worst, what, stress=False))
    gp = c.ref(mat, scale_gp)
    for cn, which, rf, sc in (("F", be.GP_F, gp.F, gp.AF), ("SIG_" + mat.upper(), be.GP_SIGMA, gp.sig, gp.Asig)):
        out[which] = ctx.gauss_field(which).to_numpy()
        worst[cn] = max(worst.get(cn, 0.0), _held(out[which], rf, sc, C[cn], what + (cn,)))
    out["E"] = _energy(c, ctx, mat, geo, c.us[scale_K if scale_K is not None else scale_f], worst, what)
    return out


def _same(a, b, what):
    for k in a:
        assert np.array_equal(a[k], b[k]), (what, "differs from a fresh context in", k)


def _thermal_after_tangent(c, what):
    """femcy_thermal_stress corrects the stress of femcy_compute_strain_stress(large = 0), once; an assembly with the tangent
    on has put the Cauchy stress of its own state into FEMCY_GP_SIGMA since: the correction is refused and sigma stays"""
    ctx = c.context("stvk")
    try:
        th = ctx.thermal(c.ELE, 1.0e-5, np.linspace(10.0, 30.0, c.lay.nn))
        ctx.upload(be.VEC_DOF, c.us[STATE_SCALES[0]])
        ctx.compute_strain_stress(be.VEC_DOF, large=False)
        ctx.set_option(be.OPT_TANGENT, 1)
        ctx.assemble_K(be.VEC_DOF)
        sig = ctx.gauss_field(be.GP_SIGMA).to_numpy()
        try:
            ctx.thermal_stress(th, 1.0)
        except be.FemcyError as e:
            assert "femcy_compute_strain_stress(large = 0)" in str(e), str(e)
        else:
            raise AssertionError((what, "femcy_thermal_stress corrected the stress an assembly with the tangent on left"))
        assert np.array_equal(ctx.gauss_field(be.GP_SIGMA).to_numpy(), sig), what
    finally:
        ctx.close()


def check_state(name, backend):
    """what the option leaves behind (include/femcy.h at FEMCY_OPT_TANGENT): internal_force with the tangent off at u1 (F,
    sigma pending), the tangent on and assemble_K at u2 (F, sigma of u2 now), the tangent off and internal_force +
    assemble_K at u1 -- everything read back after each step against the reference and bit for bit against a fresh
    context that made only the last step.  Once with the reads after step 1 (which materialise F and sigma), once without"""
    c = case(name, backend)
    s1, s2 = STATE_SCALES
    worst = {}
    for mat in MATS:
        for read_first in (True, False):
            what = (name, mat, "reads after step 1" if read_first else "F, sigma pending at step 2")
            ctx = c.context(mat)
            try:
                ctx.upload(be.VEC_DOF, c.us[s1])
                ctx.vector(be.VEC_FORCE).fill(np.nan)
                ctx.internal_force(be.VEC_DOF, be.VEC_FORCE)
                if read_first:
                    first = _read(c, ctx, mat, s1, None, s1, False, worst, what + (1,))
                f1 = ctx.download(be.VEC_FORCE)
                ctx.set_option(be.OPT_TANGENT, 1)
                ctx.upload(be.VEC_DOF, c.us[s2])
                ctx.assemble_K(be.VEC_DOF)
                assert np.array_equal(ctx.download(be.VEC_FORCE), f1), (what, "assemble_K moved vec[FORCE]")
                second = _read(c, ctx, mat, None, s2, s2, True, worst, what + (2,))
                ctx.set_option(be.OPT_TANGENT, 0)
                ctx.upload(be.VEC_DOF, c.us[s1])
                ctx.vector(be.VEC_FORCE).fill(np.nan)
                ctx.internal_force(be.VEC_DOF, be.VEC_FORCE)
                ctx.assemble_K(be.VEC_DOF)
                third = _read(c, ctx, mat, s1, s1, s1, False, worst, what + (3,))
                if read_first:
                    _same({k: first[k] for k in ("f", be.GP_F, be.GP_SIGMA, be.GP_DSDX, be.GP_VOL, "E")}, third, what + ("step 1 again",))
            finally:
                ctx.close()
            if mat == "stvk" and read_first:
                _thermal_after_tangent(c, what)
            fresh = c.context(mat)
            try:
                fresh.set_option(be.OPT_TANGENT, 1)
                fresh.upload(be.VEC_DOF, c.us[s2])
                fresh.assemble_K(be.VEC_DOF)
                _same(second, _read(c, fresh, mat, None, s2, s2, True, worst, what + ("fresh", 2)), what + (2,))
            finally:
                fresh.close()
            fresh = c.context(mat)
            try:
                fresh.upload(be.VEC_DOF, c.us[s1])
                fresh.internal_force(be.VEC_DOF, be.VEC_FORCE)
                fresh.assemble_K(be.VEC_DOF)
                _same(third, _read(c, fresh, mat, s1, s1, s1, False, worst, what + ("fresh", 3)), what + (3,))
            finally:
                fresh.close()
    print(f"{name} [{backend}]: state, worst ratios {({k: round(v, 3) for k, v in worst.items()})}")
    return _note(worst)


# ------------------------------------------------------------------------- the constants and the reference's own conditions
def measure(name, scales=SCALES):
    """float64 against long double on this row -> {constant: worst ratio}; APPLY_ASM: what asm_shapes.C_ASM must bound"""
    c = Case(ROWS[name], None)
    out = collections.defaultdict(float)

    def up(k, v):
        out[k] = max(out[k], v[0] if isinstance(v, tuple) else v)
    for mat in MATS:
        for scale in scales:
            ld, f64 = c.ref(mat, scale), c.ref(mat, scale, np.float64)
            up("TAN_" + mat.upper(), ash.ratio(f64.Kc, ld.K, ld.A))
            up("CLOSED", ash.ratio(ld.Kc, ld.K, ld.A))
            up("ENERGY", float(abs(LD(f64.E) - ld.E) / (EPS * ld.AE)) if ld.AE else 0.0)
            up("SIG_" + mat.upper(), ash.ratio(f64.sig, ld.sig, ld.Asig))
            up("FORCE_" + mat.upper(), ash.ratio(f64.f, ld.f, ld.Af))
            if mat == "stvk":
                up("DSDX", ash.ratio(f64.dsdx, ld.dsdx, ld.Adsdx))
                up("VOL", ash.ratio(f64.vol, ld.vol, ld.Avol))
                up("F", ash.ratio(f64.F, ld.F, ld.AF))
                b64, bld = c.base(scale, np.float64), c.base(scale)
                up("APPLY_ASM", ash.ratio(b64.K, bld.K, bld.A))
    return dict(out)


def check_restatement(name):
    """element_pass, which the complex step differentiates, IS asm_shapes.reference's chain: bit for bit in long double"""
    c = Case(ROWS[name], None)
    t = c.ELE.tables()
    dN, w = t["dN"].astype(LD), t["w"].astype(LD)
    X = c.nodes.astype(LD)[c.el]
    d0, a0 = ash._det_inv(np.einsum("eai,gaj->egij", X, dN))
    dsdX = np.einsum("gak,egkj->egaj", dN, a0) / d0[..., None, None]
    base = c.base(SCALES[1])
    got = element_pass(X, c.us[SCALES[1]].reshape(c.nodes.shape).astype(LD)[c.el], dN, w, dsdX, c.mats["stvk"])
    for g, r, nm in zip(got, (base.dsdx, base.vol, base.F, base.sig, base.fe), ("dsdx", "vol", "F", "sigma", "fe")):
        assert np.array_equal(g, r), (name, nm)


MUTATIONS = ("gauss point left out", "contribution twice", "no geometric term", "sigma of the other displacement",
             "F of the other displacement", "lambda', mu' swapped", "mirror untransposed")


def mutations(name, mat):
    """each mutation applied to the long-double closed form at the non-zero scale
    -> {mutation: the largest move of a stored entry in units of the bound allowed at that entry}.  The first two are
    applied at EVERY Gauss point / every off-diagonal contribution in turn and the least visible one is reported"""
    c = Case(ROWS[name], None)
    y, m = c.lay, c.mats[mat]
    ref, zero = c.ref(mat, SCALES[1]), c.ref(mat, SCALES[0])
    E, Z = ref.elem, zero.elem
    bound = 4.0 * C["TAN_" + mat.upper()] * EPS * ref.Arow                      # what the device is allowed at every stored entry

    def units(delta, at):
        with np.errstate(divide="ignore", invalid="ignore"):
            return np.where(delta == 0, 0.0, np.abs(delta) / at)

    out = {}
    at = bound[ref.slot]                                          # [e, a, b, i, k]
    out[MUTATIONS[0]] = float(units(E.Kg, at[:, None]).max(axis=(2, 3, 4, 5)).min())
    off = ~np.eye(y.npe, dtype=bool)
    out[MUTATIONS[1]] = float(units(E.Kg.sum(axis=1), at).max(axis=(3, 4))[:, off].min())
    red = ash.reducer(y, c.el, LD)
    J = ash._det_inv(E.F)[0]
    b = np.einsum("egik,egjk->egij", E.F, E.F)
    bZ, JZ = np.einsum("egik,egjk->egij", Z.F, Z.F), ash._det_inv(Z.F)[0]
    for nm, Kg in ((MUTATIONS[2], kernel_form(E.dsdx, E.dsdx, E.vol, b, E.sig, J, m, geometric=False)),
                   (MUTATIONS[3], kernel_form(E.dsdx, E.dsdx, E.vol, b, Z.sig, J, m)),
                   (MUTATIONS[4], kernel_form(E.dsdx, E.dsdx, E.vol, bZ, E.sig, JZ, m)),
                   (MUTATIONS[5], kernel_form(E.dsdx, E.dsdx, E.vol, b, E.sig, J, m, swap=True))):
        out[nm] = float(units(red(Kg.sum(axis=1)) - ref.Kc, bound).max())
    up = y.brow < y.bcol
    out[MUTATIONS[6]] = float(units(ref.Kc[up] - np.swapaxes(ref.Kc[up], 1, 2), bound[_mirror(y)[up]]).max())
    return out
