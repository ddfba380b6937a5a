"""`System_of_equations`: the host driver of the MI355X solve path, call-compatible with the
reference class (/root/reference/stiffnessMtrx.py:19-822).

Same constructor, same public attributes (`dof`, `rhs`, `nodal_force`, `residual_nodal_force`,
`du`, `dof_old`, `F`, `cauchy_stress`, `dsdx`, `vol`, `ELE`, `body`, `dm`, ...) and the same
control flow for the increment / modified-Newton / line-search drivers (`solve`, `advance_inc`),
but every kernel is a call into libfemcy_hip.so and every field is a handle to HBM-resident data
(`.to_numpy()` downloads it).  Body forces (`*Dload` GRAV / BX / BY / BZ) and point loads (`*Cload`), which the
reference does not have, are added to `rhs` after its `*Dsload` loop, and so is the load of a thermal strain
(`*Expansion` + `*Temperature`, small strain only), whose stress `compute_strain_stress` then subtracts.  Nothing numerical runs on the CPU except
the consistent Neumann loads (a per-facet loop in the reference too, stiffnessMtrx.py:369-411) and the user
Dirichlet hook.

Deliberate deviations, all outside the arithmetic of the path:
  * `solve_dof`: the reference switches to scipy's direct `spsolve` below 1e5 DOF
    (stiffnessMtrx.py:272-276).  Here that branch is a direct solve too, on the device: reverse Cuthill-McKee +
    band Cholesky (`femcy_direct_solve`, csrc/kernels_direct.hip) -- no iteration, no tolerance.  A mesh split over
    several ranks (`part`) keeps the device PCG with a tight tolerance instead (`direct_eps`, default 1e-12 on
    max|r|/max|r0|; `direct="pcg"` selects it on one rank as well); at >= 1e5 DOF the reference's own CG settings
    (eps = 1e-3) apply.
  * windows / PNG output are not produced (`show_newton_steps`, `save2path` are accepted and ignored);
    `femcy_amd.vtk_out.write_vtk` writes the mesh, displacements and Mises stress for ParaView instead.
  * the reference raises UnboundLocalError when the very first residual is < 1e-9
    (`newton_loop` unbound, :767-822); here that case returns (True, 0).
"""
import copy
import time
from types import SimpleNamespace
from typing import Tuple

import numpy as np

from . import backend as be
from . import tiGadgets as tg
from . import user_defined as ud
from .body import Body
from .conjugateGradientSolver import ConjugateGradientSolver_rowMajor as CG
from .fields import HostField


def deck_view(inp) -> SimpleNamespace:
    """what the step drivers read of a deck, with the keywords a deck may lack at their defaults: the reader's `InpInfo` carries
    all of them, `partition.LocalDeck` and the bare namespaces of the tests only those of a static step."""
    def opt(name, default=None):
        return getattr(inp, name, default)
    return SimpleNamespace(
        neumann_bc_info=inp.neumann_bc_info, dirichlet_bc_info=inp.dirichlet_bc_info, time_incs=inp.time_incs,
        geometric_nonlinear=inp.geometric_nonlinear, procedure=opt("procedure", "static"), amplitude=opt("amplitude", "RAMP"),
        density=opt("density"), body_force_info=opt("body_force_info") or [], cload_info=opt("cload_info") or [],
        expansion=opt("expansion"), temperature_info=opt("temperature_info"),
        initial_velocity_info=opt("initial_velocity_info") or [], dynamic=opt("dynamic"),
        dynamic_auto=bool(opt("dynamic_auto", False)), bulk_viscosity=opt("bulk_viscosity"),
        damping_alpha=float(opt("damping_alpha", 0.0) or 0.0), mass_scaling=opt("mass_scaling"),
        amplitudes=opt("amplitudes") or {}, energy_output=bool(opt("energy_output", False)),
        rigid_walls=opt("rigid_walls") or [])


class LoadSchedule:
    """the loads of one step and how they grow with time, built once per `solve*` call: working copies of the deck's `*Dsload`,
    `*Dload`, `*Cload` and `*Boundary` entries, the thermal load object, and the `boundary_conditions` dict that
    `impose_boundary_condition` takes, at any fraction of the deck's values.  `dirichlet`: whether the `*Boundary` entries are in
    that dict (`solve`) or treated by the caller (the dynamic procedures: after the inertia term, or through the held DOFs)."""

    def __init__(self, system, deck, dirichlet: bool):
        self.deck, self.max_time = deck, deck.time_incs["max_time"]
        self.dirichletBCs = copy.deepcopy(deck.dirichlet_bc_info)
        for bc in self.dirichletBCs:
            bc["node_set"] = HostField(np.array([*bc["node_set"]]), dtype=np.int32)
        self.bcs = {"neumannBCs": copy.deepcopy(deck.neumann_bc_info), "dirichletBCs": self.dirichletBCs if dirichlet else []}
        if deck.body_force_info or deck.cload_info:      # decks without *Dload / *Cload make the calls they always made
            self.bcs["bodyForces"] = copy.deepcopy(deck.body_force_info)
            self.bcs["cloads"] = copy.deepcopy(deck.cload_info)
        if deck.temperature_info is not None and deck.expansion is not None:
            if system.geometric_nonlinear or deck.geometric_nonlinear:
                raise ValueError("a thermal load (*Expansion + *Temperature) with nlgeom has not been supported: the "
                                 "thermal strain is a small-strain one")
            final, initial = (np.asarray(deck.temperature_info[k], dtype=np.float64) for k in ("final", "initial"))
            self.bcs["thermal"] = {"id": system.ctx.thermal(system.ELE, deck.expansion, final - initial), "scale": 0.0}
        self.any_load = bool(self.bcs["neumannBCs"] or deck.body_force_info or deck.cload_info or "thermal" in self.bcs)

    def amplitude(self, t: float) -> float:
        """the fraction of the loads that acts at time t: 1 throughout a STEP, t / T on a ramp"""
        return 1.0 if self.deck.amplitude == "STEP" else t / self.max_time

    def at(self, ratio: float) -> dict:
        """the `boundary_conditions` dict with every load -- and every Dirichlet value in it -- at `ratio` x the deck's; the
        temperature ramps over the step like every other load"""
        deck, bcs = self.deck, self.bcs
        for nb, nb0 in zip(bcs["neumannBCs"], deck.neumann_bc_info):
            nb["traction"] = nb0["traction"] * ratio
        for bf, bf0 in zip(bcs.get("bodyForces", ()), deck.body_force_info):
            bf["force"] = np.asarray(bf0["force"], dtype=np.float64) * ratio
        for cl, cl0 in zip(bcs.get("cloads", ()), deck.cload_info):
            cl["val"] = cl0["val"] * ratio
        if "thermal" in bcs:
            bcs["thermal"]["scale"] = ratio
        for bc, bc0 in zip(bcs["dirichletBCs"], deck.dirichlet_bc_info):
            bc["val"] = bc0["val"] * ratio
        return bcs


class System_of_equations:
    """K(dof) . du = rhs / residual on one MI355X."""

    def __init__(self, body: Body, material, geometric_nonlinear: bool, device: int = 0, verbose: bool = True,
                 direct_eps: float = 1.0e-12, cg_eps: float = 1.0e-3, ctx: "be.Context" = None,
                 part=None, comm_uid: bytes = None, tangent: str = "reference", exchange: str = "allreduce",
                 gather_blobs=None, direct: str = "auto", cg_branch_from: float = 1.0e5):
        """part / comm_uid: this process (or thread) holds one element partition of the mesh
        (`femcy_amd.partition.Part`, `body` built from its local nodes / elements) and joins the communicator
        `comm_uid` (RCCL unique id, or an in-process group id); every rank then runs the same `solve`."""
        self.dm = body.dm
        self.geometric_nonlinear = geometric_nonlinear
        self.body = body
        self.elements, self.nodes = body.elements, body.nodes
        self.ELE = body.ELE
        self.material = material
        self.C = material.C
        self.verbose = verbose
        self.direct_eps, self.cg_eps = direct_eps, cg_eps
        # `solve_dof` (reference :272-276) sends systems of at least 1e5 DOF to its CG (eps = 1e-3, maxit = n); the constant
        # is a parameter here so that the CG leg can be driven on any deck (tests: cg_branch_from = 0)
        self.cg_branch_from = cg_branch_from
        if direct not in ("auto", "auto-timed", "cholesky", "pcg"):
            raise ValueError("direct must be 'auto' (default: chosen by the band of the system), 'auto-timed' (chosen by "
                             "timing both on the running system), 'cholesky' (band factorisation on the device) or 'pcg' "
                             "(tight PCG)")
        self.direct = direct
        # direct = "auto": both stand-ins for the reference's spsolve return the solution to ~1e-12, so which one runs is
        # a question of time only.  The band factorisation costs n * bandwidth^2 flops behind a chain of dependent
        # launches (~20 us per panel of 32 unknowns + the tile updates), the tight PCG iterations * (matrix bytes /
        # memory bandwidth); on 2-D decks and 3-D ones up to ~4e4 DOF the factorisation wins by 1.5 ... 20 x, on 3-D
        # meshes towards 1e5 DOF (bands of 2 000 ... 2 900 sub-diagonals) the PCG is up to 2 x faster
        # (profiles/r05_direct_limit.txt).  "auto" decides from the band alone (femcy_direct_plan: a property of the mesh,
        # the same answer on every run and every machine -- round 6; round 5 timed both solvers on the running system,
        # which made the 1e-9 ... 1e-12 difference between them, and with it borderline Newton counts, depend on the
        # load of the host).  "auto-timed" keeps that exploration for whoever wants the faster solver and accepts that.
        self._auto = {"first": None, "ms": {}, "samples": {}, "tried": set(), "pcg_ok": True, "pick": None}
        self.direct_log = []              # the solver that served each solve of the direct branch, in order

        # ---- device state: mesh, element tables, material, sparsity pattern
        self.ctx = ctx if ctx is not None else be.Context(device)
        t0 = time.time()
        self.ctx.set_mesh(body.np_nodes, body.np_elements)
        self.ctx.set_element(self.ELE)
        self.ctx.set_material(material)
        self.pattern = self.ctx.build_pattern()
        # "reference": K = B^T C B on the current configuration with the constant C, as the reference assembles it
        # (modified Newton).  "consistent": material tangent at F + geometric stiffness (extension, outside parity).
        if tangent not in ("reference", "consistent"):
            raise ValueError("tangent must be 'reference' or 'consistent'")
        self.tangent = tangent
        self.ctx.set_option(be.OPT_TANGENT, 1 if tangent == "consistent" and geometric_nonlinear else 0)
        self.part = part
        if part is not None:
            self.ctx.comm_init(part.rank, part.nranks, comm_uid, part.iface_local_dofs, part.iface_global_slot,
                               part.niface_global, part.owner)
            self.verbose = verbose and part.rank == 0
            # interface exchange per CG iteration: "allreduce" (packed global interface vector), "neighbour"
            # (send/recv with the ranks sharing nodes) or "auto" (femcy_comm_tune measures both at start-up)
            self.ctx.comm_set_neighbours(part)
            if exchange == "auto":
                self.exchange = self.ctx.comm_tune(20)
            else:
                self.ctx.set_option(be.OPT_EXCHANGE, 1 if exchange == "neighbour" else 0)
                self.exchange = {"exchange": exchange}
            # persistent PCG across ranks (femcy.h): `gather_blobs(blob) -> [blob of rank 0, 1, ...]` is the host
            # program's all-gather (torch.distributed in distributed.py); the path is used only if every rank agrees
            # -- systems large enough for the one-launch kernel -- and a rank where the set-up fails votes "no"
            self.persistent_across_ranks = False
            if gather_blobs is not None:
                try:                                 # a rank whose export fails still joins the all-gather (with None)
                    blob = self.ctx.comm_mailbox_export()
                except be.FemcyError as e:
                    self._say(f"mailbox export failed ({e})")
                    blob = None
                try:
                    blobs = gather_blobs(blob)
                    if any(b is None for b in blobs):
                        raise be.FemcyError("a rank has no mailbox")
                    self.ctx.comm_mailbox_import(blobs)
                except be.FemcyError as e:
                    self._say(f"mailbox set-up failed ({e}): three launches + collectives per CG iteration")
                    self.ctx.set_option(be.OPT_PCG_PERSIST_MULTI, 0)
                self.persistent_across_ranks = self.ctx.comm_persist_agree()
        self._say("\033[32;1m pattern: {} DOF, {} blocks of {}x{}, ELL width {} ({:.3f} s) \033[0m".format(
            self.pattern.n, self.pattern.nnzb, self.dm, self.dm, self.pattern.ell_width, time.time() - t0))

        # ---- the reference's fields, as handles to HBM
        v = self.ctx.vector
        self.rhs, self.dof = v(be.VEC_RHS), v(be.VEC_DOF)
        self.nodal_force, self.residual_nodal_force = v(be.VEC_FORCE), v(be.VEC_RESIDUAL)
        self.du, self.dof_old = v(be.VEC_DU), v(be.VEC_DOF_OLD)
        g = self.ctx.gauss_field
        self.F, self.cauchy_stress = g(be.GP_F), g(be.GP_SIGMA)
        self.dsdx, self.vol = g(be.GP_DSDX), g(be.GP_VOL)
        self.strain, self.mises_stress, self.elsEngDens = g(be.GP_STRAIN), g(be.GP_MISES), g(be.GP_ENERGY)
        self.visualize_field = self.mises_stress
        self.nodal_vals = HostField(np.zeros((self.ctx.ne, self.ctx.npe)))
        self.elsEng = 0.0
        self.sparseMtrx_rowMajor = self          # what the reference hands to the CG class
        self.sparseIJ = None

        self.time0 = 0.
        self.time1 = 0.
        self.dt = 0.
        self.compiled = False
        self._dofsets = {}
        self._loadsets = {}
        self._bodyloads = {}
        self._linear_energy = False   # set by solve_dynamic: get_elasEng then reports u.Ku / 2 (femcy_elastic_energy_small)
        self._thermal = None      # {"id", "scale"} of the thermal load that was applied last (compute_strain_stress)
        self.cg_log = []          # one entry per CG solve: iterations, max|r0|, max|r|, increment end time
        self.stats = {"assemblies": 0, "force_evals": 0, "linear_solves": 0, "cg_iterations": 0, "direct_solves": 0,
                      "direct_rejected": 0}

    @property
    def n_system(self) -> int:
        return self.dof.shape[0] if self.part is None else self.ctx.n_global

    def _say(self, msg):
        if self.verbose:
            print(msg)

    # ----------------------------------------------------------------------------- kernels
    def get_dsdx_and_vol(self):
        """geometry is fused into the assembly / internal-force launches (same dof, same result);
        kept as a method because the reference's drivers call it."""

    def assemble_stiffnessMtrx(self):
        self.ctx.assemble_K(be.VEC_DOF)
        self.stats["assemblies"] += 1

    def _first_assembly_took(self, t0: float):
        if not self.compiled:
            self.compiled = True
            self.ctx.sync()
            self._say("\033[35;1m first assembly took {:.4f} s\033[0m".format(time.time() - t0))

    assemble_sparseMtrx = assemble_stiffnessMtrx
    assemble_stiffnessMtrx_faster = assemble_stiffnessMtrx

    def assemble_nodal_force_GN(self):
        """F (reference configuration) -> sigma(F) -> current-configuration grad N, vol -> nodal gather."""
        self.ctx.internal_force(be.VEC_DOF, be.VEC_FORCE)
        self.stats["force_evals"] += 1

    def get_deformation_gradient(self):
        self.ctx.internal_force(be.VEC_DOF, be.VEC_TMP0)      # F and sigma are by-products of the element pass

    # ------------------------------------------------------------------------ linear solve
    def _linear_system(self):
        if not hasattr(self, "PCG"):
            b = self.rhs if not self.geometric_nonlinear else self.residual_nodal_force
            self.PCG = CG(spm=self.sparseMtrx_rowMajor, sparseIJ=self.sparseIJ, b=b, eps=self.cg_eps)
        return self.PCG

    def _take_solution(self):
        self.stats["linear_solves"] += 1
        self.du.copy_from(self.PCG.x)
        if not self.geometric_nonlinear:
            self.dof.copy_from(self.PCG.x)
        else:
            tg.c_equals_a_minus_b(self.dof, self.dof, self.PCG.x)      # Newton: dof -= x
        return self.du

    def solve_by_CG(self, eps=None, maxit=None):
        self._linear_system()
        self.PCG.eps = self.cg_eps if eps is None else eps
        self.PCG.re_init()
        it, r0, rmax = self.ctx.pcg(self.PCG.b.id, self.PCG.x.id, eps=self.PCG.eps,
                                    maxit=self.PCG.maxit if maxit is None else maxit)
        self.PCG.iterations, self.PCG.r0, self.PCG.rmax = it, r0, rmax
        self.PCG.converged = r0 == 0.0 or rmax < self.PCG.eps * r0
        self.stats["cg_iterations"] += it
        self.cg_log.append({"iters": it, "r0": r0, "rmax": rmax, "time1": self.time1, "converged": self.PCG.converged})
        return self._take_solution()

    def _tight_pcg(self):
        """the PCG where a direct solve is meant: eps = direct_eps.  CG in floating point can need more than n iterations on
        an ill-conditioned K (nu -> 0.5), so the cap is 10 n here instead of the reference CG's n.  Whether an unconverged
        iterate is an error is the caller's business (`PCG.converged`)."""
        return self.solve_by_CG(eps=self.direct_eps, maxit=int(min(10 * self.n_system, 2 ** 31 - 1)))

    # sub-diagonals above which the FIRST solve of direct = "auto" goes to the tight PCG.  Cube-like C3D4 meshes, medians of
    # five (profiles/r05_direct_mfma_update.txt): 512 sub-diagonals 3.7 ms against 14.6 (PCG), 1 328: 20.3 against 45.3,
    # 2 192: 51.0 against 59.1, 2 888: 86.4 against 69.0 -- the crossover lies near 2 500
    AUTO_WIDE_BAND = 2560
    AUTO_TRY_OTHER_MS = 5.0      # a first solve slower than this makes the second solve time the other method

    def _auto_method(self) -> str:
        """'cholesky' or 'pcg' for the next solve of the reference's direct branch.  direct = "auto": by the band
        (femcy_direct_plan), once, for the whole run.  direct = "auto-timed": the first solve by the band; if it took more
        than AUTO_TRY_OTHER_MS the next three solves alternate other / first / other, so that each method is timed twice
        (the first call of either carries one-off costs: band allocation, hipGraph capture), and the faster one (minimum
        of its samples) serves the rest of the run.  A PCG that broke down or did not converge leaves the race either way."""
        a = self._auto
        if a["pick"] is not None:
            return a["pick"]
        if a["first"] is None:
            try:
                plan = self.ctx.direct_plan()
                wide = plan["bandwidth"] > self.AUTO_WIDE_BAND
                a["plan"] = plan
            except (be.FemcyError, AttributeError):
                wide = False
            a["first"] = "pcg" if wide else "cholesky"
            if self.direct == "auto":                            # deterministic: the band decides, for the whole run
                a["pick"] = a["first"]
            return a["first"]
        first = a["first"]
        other = "pcg" if first == "cholesky" else "cholesky"
        if not a["pcg_ok"]:
            a["pick"] = "cholesky"
        elif first in a["ms"] and a["ms"][first] <= self.AUTO_TRY_OTHER_MS:
            a["pick"] = first                                    # a millisecond-sized solve: nothing to gain by exploring
        else:
            cnt = a["samples"]
            if cnt.get(other, 0) < cnt.get(first, 0) and cnt.get(other, 0) < 2:
                return other
            if cnt.get(first, 0) < 2:
                return first
            a["pick"] = min(a["ms"], key=a["ms"].get) if a["ms"] else first
        return a["pick"]

    def solve_by_scipy(self):
        """the reference's direct branch (`spsolve`, :219-251; the name is kept): band Cholesky on the device, or the
        tight PCG where that is faster (direct = "auto" / "auto-timed")."""
        if self.part is None and self.direct in ("auto", "auto-timed"):
            method = self._auto_method()
            a = self._auto
            timed = self.direct == "auto-timed"
            if timed:
                self.ctx.sync()
            t0 = time.perf_counter()
            if method == "pcg":
                a["tried"].add("pcg")
                # an exploratory solve: K may be the indefinite matrix of a diverging Newton iterate, on which CG breaks
                # down (NaN: FEMCY_ENUMERIC) or wanders -- the factorisation (L S L^T takes negative pivots, as the
                # reference's LU does) then serves this solve and every later one
                try:
                    du = self._tight_pcg()
                    failed, applied = not self.PCG.converged, True
                except be.FemcyError as e:
                    if e.status != be.FEMCY_ENUMERIC:
                        raise
                    failed, applied = True, False                # the breakdown left before _take_solution: dof untouched
                if not failed:
                    if timed:
                        a["ms"]["pcg"] = min(a["ms"].get("pcg", 1e30), (time.perf_counter() - t0) * 1e3)
                    a["samples"]["pcg"] = a["samples"].get("pcg", 0) + 1
                    self.direct_log.append("pcg")
                    return du
                a["pcg_ok"], a["pick"] = False, "cholesky"
                if applied:
                    self.stats["linear_solves"] -= 1
                    if self.geometric_nonlinear:
                        tg.a_equals_b_plus_c_mul_d(self.dof, self.dof, 1.0, self.PCG.x)       # undo dof -= x
                t0 = time.perf_counter()
            a["tried"].add("cholesky")
            du = self._solve_direct()
            if self.direct_info is not None and timed:
                a["ms"]["cholesky"] = min(a["ms"].get("cholesky", 1e30), (time.perf_counter() - t0) * 1e3)
            # (a rejected factorisation -- ENUMERIC, served by the tight PCG inside _solve_direct -- still counts as a sample:
            # the exploration must end)
            a["samples"]["cholesky"] = a["samples"].get("cholesky", 0) + 1
            return du
        return self._solve_direct()

    def _solve_direct(self):
        self.direct_info = None
        if self.part is None and self.direct in ("cholesky", "auto", "auto-timed"):
            self._linear_system()
            try:
                self.direct_info = self.ctx.direct_solve(self.PCG.b.id, self.PCG.x.id)
            except be.FemcyError as e:
                if e.status == be.FEMCY_ENOMEM:
                    print(f"femcy_amd: {e}; this system is solved by the tight PCG instead", flush=True)
                    self.direct = "pcg"
                elif e.status == be.FEMCY_ENUMERIC:
                    # K singular, or so indefinite that elimination without pivoting lost it (a Newton iterate on its
                    # way out: the increment is usually cut back a few solves later).  The reference's LU with
                    # pivoting still returns something there and the driver's path depends on it, so THIS solve gets
                    # the tight PCG; if that fails as well the breakdown goes to the caller
                    self.stats["direct_rejected"] += 1
                else:
                    raise
            else:
                self.PCG.iterations, self.PCG.converged = 0, True
                self.stats["direct_solves"] += 1
                self.direct_log.append("cholesky")
                return self._take_solution()
        du = self._tight_pcg()                         # a mesh split over ranks (or direct="pcg")
        if not self.PCG.converged:
            # a direct solver would have returned the solution (or failed loudly); an unconverged iterate must not be
            # used as if it were one: report it like a numerical breakdown, so that a Newton step is cut back
            # (advance_inc) and a linear deck fails instead of printing a wrong answer
            raise be.FemcyError("tight PCG in place of the direct solve: stopped at max|r| = {:.3e} > {:.1e} * {:.3e} "
                                "after {} iterations".format(self.PCG.rmax, self.direct_eps, self.PCG.r0,
                                                             self.PCG.iterations), status=be.FEMCY_ENUMERIC)
        self.direct_log.append("pcg")
        return du

    def solve_dof(self):
        if self.n_system < self.cg_branch_from:        # DOFs of the whole system (all ranks take the same branch)
            return self.solve_by_scipy()
        return self.solve_by_CG()

    # ----------------------------------------------------------------- boundary conditions
    @staticmethod
    def _node_ids(nodeSet):
        return np.asarray(nodeSet.to_numpy() if hasattr(nodeSet, "to_numpy") else nodeSet, dtype=np.int64)

    def _dofset(self, nodeSet, dm_specified: int) -> int:
        """device-resident DOF list of a (node set, component) pair; the reference likewise turns every node
        set into a ti.field once per solve (:656-659).  Cached by content."""
        ids = self._node_ids(nodeSet)
        key = (dm_specified, ids.size, int(ids[0]) if ids.size else -1, int(ids[-1]) if ids.size else -1, int(ids.sum()))
        for cached_ids, ds in self._dofsets.get(key, ()):        # keyed by content: solve() re-wraps the node sets on
            if np.array_equal(cached_ids, ids):                  # every call, the device lists must not pile up
                return ds
        ds = self.ctx.dofset(ids * self.dm + dm_specified)
        self._dofsets.setdefault(key, []).append((ids.copy(), ds))
        return ds

    def dirichletBC_linearEquations(self, nodeSet, dm_specified: int, sval: float):
        self.ctx.dofset_dirichlet_linear(self._dofset(nodeSet, dm_specified), sval, be.VEC_RHS)

    def dirichletBC_forNewtonMethod_kernel(self, nodeSet, dm_specified: int, sval: float):
        self.ctx.dofset_dirichlet_newton(self._dofset(nodeSet, dm_specified), be.VEC_RESIDUAL)

    def dirichletBC_forNewtonMethod(self, dirichletBCs):
        for bc in dirichletBCs:
            self.dirichletBC_dof(bc["node_set"], bc["dof"], bc["val"], bc["user"], self.time1)
            self.dirichletBC_forNewtonMethod_kernel(nodeSet=bc["node_set"], dm_specified=bc["dof"], sval=bc["val"])

    def dirichletBC_dof(self, nodeSet, dm_specified: int, sval: float, user: bool, time: float):
        if not user:
            self.dirichletBC_val(nodeSet, dm_specified, sval)
        else:
            ud.user_dirichletBC(self.dof, nodeSet, self.dm, dm_specified, self.nodes, time)

    def dirichletBC_val(self, nodeSet, dm_specified: int, sval: float):
        self.ctx.dofset_fill(self._dofset(nodeSet, dm_specified), be.VEC_DOF, sval)

    def _loadset(self, load_facets) -> list:
        """device load sets of one *Dsload surface, built once per face set: owning element of each facet
        (body.boundary, reference :386) and the facet's type = position of its sorted local node tuple in the
        element plugin's facet tables (reference :388-392).  One set per facet arity of the element, fewest nodes
        first, empty where the surface has no facet of that arity: a wedge surface can hold triangles and
        quadrilaterals, and a load set has one arity.  The number of sets depends on the element alone, so every rank
        of a partitioned run makes the same collective calls in neumannBC, whichever facets it holds."""
        key = frozenset(tuple(f) for f in load_facets)           # by content: repeated solve() calls reuse the device set
        if key not in self._loadsets:
            boundary = self.body.get_boundary()
            arities = self.ELE.facet_arities()
            facets = [tuple(f) for f in load_facets]
            sets = []
            for nfn in arities:
                fk = [f for f in facets if len(f) == nfn]
                if not fk:       # no loaded facet of this arity (on this rank of a partitioned run)
                    sets.append(self.ctx.loadset(self.ELE, np.zeros(0, np.int32), np.zeros(0, np.int32),
                                                 nfn if len(arities) > 1 else None))
                    continue
                elem = np.fromiter((boundary[f] for f in fk), dtype=np.int64, count=len(fk))
                fnodes = np.asarray(fk, dtype=np.int64).reshape(len(fk), -1)
                conn = self.body.np_elements[elem]                                            # [nf, npe]
                local = np.sort((conn[:, None, :] == fnodes[:, :, None]).argmax(axis=2), axis=1)   # sorted local ids
                keys = self.ELE.facet_tables(nfn if len(arities) > 1 else None)["keys"]
                type_of = {k: i for i, k in enumerate(keys)}
                ft = np.fromiter((type_of[tuple(r)] for r in local.tolist()), dtype=np.int32, count=len(fk))
                sets.append(self.ctx.loadset(self.ELE, elem, ft, nfn if len(arities) > 1 else None))
            self._loadsets[key] = (sets, load_facets)
        return self._loadsets[key][0]

    def neumannBC(self, load_facets, load_val: float, load_dir=np.array([])):
        """consistent nodal loads of a surface traction (dead load on the undeformed geometry), evaluated on the
        device.  rhs is refreshed on every call, as in the reference (:384): the first load set (fewest facet nodes)
        overwrites it, a second arity's set is added to it (an empty set adds nothing, but it still takes part in the
        interface sum of a partitioned run)."""
        for i, ls in enumerate(self._loadset(load_facets)):
            self.ctx.loadset_neumann(ls, load_val, load_dir, be.VEC_RHS, add=i > 0)

    def _bodyload(self, ele_set) -> int:
        """device body load (nodal weights) of one element set, None = the whole mesh; built once per set, by content."""
        ids = None if ele_set is None else np.ascontiguousarray(ele_set, dtype=np.int32).ravel()
        key = None if ids is None else ids.tobytes()
        if key not in self._bodyloads:
            self._bodyloads[key] = self.ctx.bodyload(self.ELE, ids)
        return self._bodyloads[key]

    def bodyForce(self, ele_set, force):
        """rhs += consistent nodal loads of a uniform force per unit volume on `ele_set` (*Dload GRAV / BX / BY / BZ):
        a dead load on the undeformed volume, evaluated on the device."""
        self.ctx.bodyload_apply(self._bodyload(ele_set), force, be.VEC_RHS, add=True)

    def cload(self, nodeSet, dm_specified: int, val: float):
        """rhs[node, dm_specified] += val for every node of the set (*Cload)."""
        self.ctx.dofset_add(self._dofset(nodeSet, dm_specified), be.VEC_RHS, val)

    def thermalLoad(self, thermal: dict):
        """rhs += scale x the consistent nodal load of the thermal strain alpha dT I (*Expansion + *Temperature), built
        once on the undeformed geometry by `solve` (ctx.thermal)."""
        self.ctx.thermal_apply(thermal["id"], thermal["scale"], be.VEC_RHS, add=True)
        self._thermal = thermal

    def impose_boundary_condition(self, boundary_conditions: dict):
        for nb in boundary_conditions["neumannBCs"]:
            self.neumannBC(nb["face_set"], load_val=nb["traction"], load_dir=nb.get("direction", np.array([])))
        body_forces = boundary_conditions.get("bodyForces", ())
        cloads = boundary_conditions.get("cloads", ())
        thermal = boundary_conditions.get("thermal")
        if (body_forces or cloads or thermal) and not boundary_conditions["neumannBCs"]:
            self.rhs.fill(0.0)              # no *Dsload refreshed rhs: the added loads start from zero
        for bf in body_forces:
            self.bodyForce(bf["ele_set"], bf["force"])
        for cl in cloads:
            self.cload(cl["node_set"], cl["dof"], cl["val"])
        if thermal:
            self.thermalLoad(thermal)
        for bc in boundary_conditions["dirichletBCs"]:
            if not self.geometric_nonlinear:
                self.dirichletBC_linearEquations(bc["node_set"], bc["dof"], bc["val"])
            else:   # Newton: prescribed values go into dof now, K / residual are treated later
                self.dirichletBC_dof(bc["node_set"], bc["dof"], bc["val"], bc["user"], self.time1)

    # ------------------------------------------------------- shared by the transient drivers
    def _transient_gate(self, deck, step: str, mass: str, motion: bool = False):
        """what neither dynamic procedure takes; `step` and `mass` are the words in which the two name themselves.  `motion`
        (the explicit procedure): a `*Boundary` entry that names an `*Amplitude` is prescribed motion and passes; a non-zero
        value without one is a jump, not a motion, and is refused everywhere."""
        if self.part is not None:
            raise ValueError("a {} on more than one rank has not been supported: the {} is single-rank".format(step, mass))
        if deck.density is None:
            raise ValueError("*Dynamic needs a *Density in the *Material block")
        if any(bc["val"] != 0.0 and not (motion and "amplitude" in bc) for bc in deck.dirichlet_bc_info):
            raise ValueError("a non-zero *Boundary value in a *Dynamic step (prescribed motion) has not been supported")
        for bc in deck.dirichlet_bc_info:
            if "amplitude" in bc and not motion:
                raise ValueError("*Boundary, amplitude={} has not been supported in a {}: prescribed motion is built for "
                                 "*Dynamic, explicit alone".format(bc["amplitude"], step))
            if "amplitude" in bc and bc["amplitude"] not in deck.amplitudes:
                raise ValueError("*Boundary, amplitude={}: the deck has no *Amplitude of that name".format(bc["amplitude"]))

    def _set_motion(self, deck, loads, ex, held):
        """prescribed motion of an explicit step: the `*Boundary` entries that name an `*Amplitude` move as value x A(t), the
        other held entries stay at rest.  One device curve per name that is used; `self.motion` lists the moved entries, in
        the deck's order (empty: no call is made and the integrator is launched as it always was)."""
        ctx = self.ctx
        self.motion = [{"node_set": self._node_ids(bc["node_set"]), "dof": bc["dof"], "val": bc["val"],
                        "amplitude": bc["amplitude"]} for bc in loads.dirichletBCs if "amplitude" in bc]
        if not self.motion:
            return
        curves, sets = {}, [ds for ds, bc in zip(held, loads.dirichletBCs) if "amplitude" in bc]
        for m in self.motion:
            if m["amplitude"] not in curves:
                a = deck.amplitudes[m["amplitude"]]
                curves[m["amplitude"]] = ctx.amplitude(a["definition"], a["t"], a["A"])
        ctx.explicit_set_motion(ex, sets, [m["val"] for m in self.motion], [curves[m["amplitude"]] for m in self.motion])

    def _reaction(self, scale: float) -> list:
        """per moved `*Boundary` entry, the force the body exerts on the boundary that moves it: the sum over the entry's DOFs
        of scale x f - f_int at the current state, so that a bar pulled along +z answers with a negative number -- the
        residual f_int - scale x f of those DOFs with the sign turned.  An internal-force evaluation and two vector calls;
        the bulk-viscosity forces are not part of f_int and are not in it."""
        ctx = self.ctx
        ctx.internal_force(be.VEC_DOF, be.VEC_FORCE)
        ctx.vec_axpy(be.VEC_RESIDUAL, be.VEC_FORCE, -scale, be.VEC_RHS)
        r = ctx.download(be.VEC_RESIDUAL)
        return [-float(r[m["node_set"] * self.dm + m["dof"]].sum()) for m in self.motion]

    def _external_force(self, loads: LoadSchedule, ratio: float):
        """rhs = `ratio` x the loads of a dynamic step, which reads rhs whatever the deck holds: zeroed here if it holds no load"""
        if not loads.any_load:
            self.rhs.fill(0.0)
        self.impose_boundary_condition(loads.at(ratio))

    def _initial_state(self, deck, held):
        """t = 0 of a dynamic step: u_0 = 0, v_0 from `*Initial Conditions, type=VELOCITY`, 0 on the `*Boundary` entries `held`"""
        ctx = self.ctx
        self.velocity, self.acceleration = ctx.vector(be.VEC_VEL), ctx.vector(be.VEC_ACC)
        self.dof.fill(0.0)
        self.dof_old.fill(0.0)
        self.velocity.fill(0.0)
        for iv in deck.initial_velocity_info:
            ctx.dofset_fill(self._dofset(iv["node_set"], iv["dof"]), be.VEC_VEL, iv["val"])
        for bc in held:
            ctx.dofset_fill(self._dofset(bc["node_set"], bc["dof"]), be.VEC_VEL, 0.0)
        self.time0 = self.time1 = 0.0

    def _energies(self, kinetic: float) -> dict:
        out = {"kinetic": kinetic, "strain_energy": self.get_elasEng()}
        bal = getattr(self, "_energy_balance", None)
        if bal is not None:                                           # *Energy Output in an explicit step
            w = self.ctx.explicit_energy(bal["ex"])                   # the work sums since t = 0, one synchronising read-back
            if bal["strain0"] is None:
                bal["strain0"] = out["strain_energy"]
            load, internal, alpha, boundary = (float(x) for x in w)
            external = load + boundary
            # derived on the host: the material is hyperelastic, so what the internal forces did beyond the stored strain
            # energy is the share of the bulk viscosity
            bulk = internal - (out["strain_energy"] - bal["strain0"])
            out.update(external_work=external, boundary_work=boundary, internal_work=internal,
                       viscous_dissipation=alpha + bulk, energy_total=kinetic + internal + alpha - external)
        walls = getattr(self, "walls", None)
        if walls:                                                     # *Rigid Wall: one synchronising read-back per wall
            got = [self.ctx.explicit_wall_get(self.explicit, k) for k in range(len(walls))]
            out["wall"] = [{"force": float(g[0]), "energy": float(g[1]), "nodes": int(g[2]), "penetration": float(g[3])}
                           for g in got]
            if bal is not None:                                       # the walls are conservative: their potential counts
                out["contact_energy"] = float(sum(g[1] for g in got))
                out["energy_total"] += out["contact_energy"]
        return out

    def _set_walls(self, deck, ex, omega_ref: float):
        """`*Rigid Wall` (`deck.rigid_walls`) -> `femcy_explicit_set_wall`, before the start.  A wall without `penalty=` takes
        kappa = 0.1 omega_ref^2 with omega_ref the first frequency estimate of the run.  `self.walls` keeps {"point", "normal",
        "penalty"} per wall as set, `self.wall_kappa` the sum of the penalties (0.0 without walls)."""
        self.walls = [{"point": np.asarray(w["point"], dtype=np.float64), "normal": np.asarray(w["normal"], dtype=np.float64),
                       "penalty": float(w["penalty"]) if w["penalty"] is not None else 0.1 * (omega_ref * omega_ref)}
                      for w in deck.rigid_walls]
        self.wall_kappa = float(sum(w["penalty"] for w in self.walls))
        if self.walls:
            self.ctx.explicit_set_wall(ex, [w["point"] for w in self.walls], [w["normal"] for w in self.walls],
                                       [w["penalty"] for w in self.walls])

    def _record(self, kinc: int, dt: float, kinetic: float, **more):
        """the entry of `increments` after a step, or a batch of steps, that ended at `time1`"""
        self.increments.append({"kinc": kinc, "time1": self.time1, "dt": dt, **more, "converged": True, "newton_loop": 0,
                                **self._energies(kinetic)})

    def _displacements_are_finite(self, after: str):
        if not np.isfinite(self.ctx.vec_absmax(be.VEC_DOF)):
            raise be.FemcyError("explicit step: the displacements are not finite after {} (an unstable increment)".format(after),
                                status=be.FEMCY_ENUMERIC)

    # --------------------------------------------------------------------- time stepping
    def solve(self, inp, show_newton_steps: bool = False, save2path: str = None):
        """multiple time increments with automatic cut-back (reference :647-711).  A `*Dynamic` step goes to
        `solve_dynamic`; a deck without it makes the calls it always made."""
        self._linear_energy = False      # get_elasEng: the reference's energy, unless solve_dynamic says otherwise
        self._energy_balance = None      # set by solve_explicit for a deck with *Energy Output
        deck = deck_view(inp)
        if deck.procedure == "dynamic":
            return self.solve_dynamic(inp)
        if deck.procedure == "explicit":
            return self.solve_explicit(inp)
        max_inc, min_inc, max_time = deck.time_incs["max_inc"], deck.time_incs["min_inc"], deck.time_incs["max_time"]
        self.dt = deck.time_incs["ini_inc"]
        loads = LoadSchedule(self, deck, dirichlet=True)       # rhs: a deck with no load never refreshes it, as in the reference
        self.increments = []
        kinc = -1
        while self.time1 < max_time:
            kinc += 1
            self.time1 = min(self.time0 + self.dt, max_time)
            self._say("\033[40;33;1m >>>>> kinc = {}, time0 = {}, dt = {} \033[0m".format(kinc, self.time0, self.dt))
            converged, newton_loop = self.advance_inc(inp, loads.at(loads.amplitude(self.time1)), show_newton_steps, save2path)
            self.increments.append({"kinc": kinc, "time1": self.time1, "dt": self.dt, "converged": converged,
                                    "newton_loop": newton_loop})
            if not converged:
                self.time1 = self.time0
                self.dt /= 4.
                self.dof.copy_from(self.dof_old)
                kinc -= 1
                if self.dt < min_inc:
                    print("\033[31;1m allowable minimum dt is reached, "
                          "Newton's method not converges, solution is not found. \033[0m")
                    break
                continue
            if newton_loop <= 8:
                self.dt = min(self.dt * 1.5, max_inc)
            self.dof_old.copy_from(self.dof)
            self.time0 = self.time1

    # ------------------------------------------------------------------- implicit dynamics
    def solve_dynamic(self, inp):
        """linear transient dynamics (`*Dynamic, direct`): undamped Newmark with the consistent mass, fixed increments.
        u_0 = 0, v_0 from `*Initial Conditions, type=VELOCITY`, a_0 from M a_0 = f(0+); per step, with a0 = 1/(beta dt^2),
            (K + a0 M) u_{n+1} = f(t_{n+1}) + M (a0 u_n + v_n / (beta dt) + (1/(2 beta) - 1) a_n),
        then a_{n+1}, v_{n+1} by `femcy_newmark_update`.  K is the matrix of the undeformed mesh, rebuilt with the mass
        every step (the last step is clipped to T); the Dirichlet rows take the value 0; every solve uses the tight
        settings of the direct branch (band factorisation, or PCG with eps = direct_eps), whatever the size.  Each entry
        of `increments` carries the kinetic and the strain energy (`get_elasEng`: u.Ku / 2 here) after the step,
        `initial_energy` those of t = 0."""
        from .material_zoo.mater_base import FEMCY_MAT_NEOHOOKE
        if self.geometric_nonlinear or inp.geometric_nonlinear:
            raise ValueError("a *Dynamic step with nlgeom=YES has not been supported: the integrator is linear "
                             "(small strain)")
        if getattr(self.material, "kind", None) == FEMCY_MAT_NEOHOOKE:
            raise ValueError("a *Dynamic step with a neo-Hookean material has not been supported: the integrator is linear "
                             "(small strain)")
        deck = deck_view(inp)
        self._transient_gate(deck, "*Dynamic step", "mass matrix")
        beta, gamma = deck.dynamic["beta"], deck.dynamic["gamma"]
        dt, max_time = deck.time_incs["ini_inc"], deck.time_incs["max_time"]
        ctx = self.ctx
        loads = LoadSchedule(self, deck, dirichlet=False)             # Dirichlet rows are treated after the inertia term

        def dirichlet_rows():
            for bc in loads.dirichletBCs:
                self.dirichletBC_linearEquations(bc["node_set"], bc["dof"], 0.0)

        def linear_solve():
            if self.n_system < self.cg_branch_from:
                return self.solve_by_scipy()
            du = self._tight_pcg()
            if not self.PCG.converged:
                raise be.FemcyError("dynamic step: the PCG stopped at max|r| = {:.3e} > {:.1e} * {:.3e}".format(
                    self.PCG.rmax, self.direct_eps, self.PCG.r0), status=be.FEMCY_ENUMERIC)
            return du

        self._linear_energy = True
        self.mass = ctx.mass(self.ELE, deck.density)
        # ---- t = 0: u_0 = 0, v_0 from the deck (0 where the body is held), M a_0 = f(0+) - K u_0
        self._initial_state(deck, loads.dirichletBCs)
        self._external_force(loads, loads.amplitude(0.0))
        ctx.mass_add_to_K(self.mass, 1.0, overwrite=True)
        dirichlet_rows()
        linear_solve()
        self.acceleration.copy_from(self.dof)
        self.dof.fill(0.0)
        self.initial_energy = self._energies(ctx.mass_kinetic_energy(self.mass, be.VEC_VEL))
        self.increments = []
        kinc = 0
        while self.time0 < max_time * (1.0 - 1.0e-12):
            self.time1 = min((kinc + 1) * dt, max_time)               # the last step is clipped to T
            if max_time - self.time1 < 1.0e-12 * max_time:
                self.time1 = max_time
            self.dt = h = self.time1 - self.time0
            self._say("\033[40;33;1m >>>>> kinc = {}, time0 = {}, dt = {} \033[0m".format(kinc, self.time0, h))
            t0 = time.time()
            a0 = 1.0 / (beta * h * h)
            ctx.assemble_K(-1)                                        # K of the undeformed mesh (small strain)
            self.stats["assemblies"] += 1
            self._first_assembly_took(t0)
            ctx.mass_add_to_K(self.mass, a0)
            ctx.newmark_predict(be.VEC_DOF, be.VEC_VEL, be.VEC_ACC, be.VEC_RESIDUAL, a0, 1.0 / (beta * h),
                                1.0 / (2.0 * beta) - 1.0)
            self._external_force(loads, loads.amplitude(self.time1))
            ctx.mass_apply(self.mass, be.VEC_RESIDUAL, be.VEC_RHS, 1.0, add=True)
            dirichlet_rows()
            linear_solve()                                            # dof = u_{n+1}; dof_old still holds u_n
            ctx.newmark_update(be.VEC_DOF, be.VEC_DOF_OLD, be.VEC_VEL, be.VEC_ACC, beta, gamma, h)
            self.dof_old.copy_from(self.dof)
            self._record(kinc, h, ctx.mass_kinetic_energy(self.mass, be.VEC_VEL))
            self.time0 = self.time1
            kinc += 1

    # ------------------------------------------------------------------- explicit dynamics
    def solve_explicit(self, inp):
        """transient dynamics at large deformation (`*Dynamic, explicit`): central differences with the HRZ-lumped mass, as
        velocity Verlet (`femcy_explicit_*`); no matrix is solved.  The internal force is the large-deformation one for
        every material, whatever the `*Step` line says about nlgeom.  u_0 = 0, v_0 from `*Initial Conditions,
        type=VELOCITY`; tractions, body forces and `*Cload` are dead loads, evaluated once at scale 1 and scaled by the
        amplitude (STEP: 1, RAMP: t / T); constrained DOFs have no inverse mass and stay at rest.
        The increment is the deck's under `direct user control`, else `scale factor` x the stable increment estimated ONCE,
        on the undeformed mesh with its matrix (`femcy_explicit_stable_dt`); either is then adjusted DOWN so that T is a
        whole number of steps, and the run ends at T exactly.  Steps run in batches of `output_every` (default 64) per
        `femcy_explicit_advance`, the last one clipped; after each batch `increments` gains {"kinc" (steps done), "time1",
        "dt", "kinetic", "strain_energy"} (`get_elasEng`, the reference's large-strain energy), `initial_energy` holds those
        of t = 0.  A displacement that is not finite -- an unstable increment -- raises FemcyError(FEMCY_ENUMERIC).
        With `element by element` (`inp.dynamic_auto`) no matrix is assembled: the increment is `scale factor` x 2 / omega of
        the element-by-element estimate at the CURRENT configuration, re-estimated on the device in every step
        (`femcy_explicit_auto_*`), and the last step takes what is left of T.  Batches of `output_every` steps run until the
        clock read back after a batch says t == T (the steps of the last batch past T are no-ops); the records carry "kinc"
        (real steps so far), "time1" (the device clock), "dt" (the last increment) and "dt_min"; `stable_dt` is the first
        estimate, `dt` the last increment.  An increment that collapses to 0 before T raises the same error.
        `*Bulk Viscosity` and `*Damping, alpha=` (`inp.bulk_viscosity`, `inp.damping_alpha`) go to the integrator once
        (`femcy_explicit_set_damping`, M_d from `dilatational_modulus`); the fixed increment estimated from the matrix is
        then 2 / omega x (sqrt(1 + xi^2) - xi) with xi = b1 + alpha / (2 omega), which `stable_dt` reports -- the quadratic
        bulk term cannot be known in advance and is left to `scale factor`; `direct user control` is taken as given.
        `*Fixed Mass Scaling` (`inp.mass_scaling`) scales the element masses once, between the lumped mass and the integrator
        (`femcy_lumped_mass_scale` with `material_stiffness()`); `mass_scaling` keeps {"mass0", "mass1", "scaled_elements",
        "max_factor"} (None without the keyword).  Both increment estimates and the kinetic energy then see the scaled
        masses.  The loads do not: body forces stay those of the deck's density, and so does rho_0 of the bulk viscosity.
        Prescribed motion: a `*Boundary, amplitude=NAME` entry moves its DOFs as value x A(t) with A the deck's `*Amplitude`
        NAME in step time (`femcy_amplitude_create`, `femcy_explicit_set_motion`, right after the integrator is made); held
        entries without an amplitude stay at rest, and a non-zero value without one is refused.  The integrator itself places
        the moved DOFs at t = 0.  `self.motion` lists the moved entries, and only when there are any every record gains
        "reaction": per moved entry the force the body exerts on its boundary, the sum over the entry's DOFs of s f - f_int at
        the record's state, which opposes a pull (`_reaction`; the bulk-viscosity forces are not in it).
        `*Energy Output` (`inp.energy_output`): the integrator keeps an energy balance on the device
        (`femcy_explicit_energy_enable`, with the definitions), and every record and `initial_energy` gain "external_work"
        (loads + moved boundary), "boundary_work", "internal_work", "viscous_dissipation" -- the alpha work plus internal_work
        - (strain_energy - strain_energy at t = 0), the bulk-viscosity share, DERIVED on the host because the material is
        hyperelastic -- and "energy_total" = kinetic + internal_work + alpha work - external_work, which a stable run
        keeps near its initial value.  Without the keyword the records, the launches and the bits are unchanged.
        `*Rigid Wall` (`inp.rigid_walls`, an extension keyword): frictionless planar rigid walls with a mass-proportional
        penalty (`femcy_explicit_set_wall`, with the law), set before the start.  A wall without `penalty=` takes kappa =
        0.1 omega_ref^2, omega_ref being the first estimate the run has: `omega_bound` of the matrix on the fixed path, the
        element bound at u_0 taken before the walls are set on the element-by-element path, 2 / dt under `direct user
        control`.  With kappa the sum of the penalties the fixed path uses omega_c = sqrt(omega_bound^2 + kappa) wherever it
        used omega_bound (`omega_contact`; the lagged-damping factor too), the element-by-element estimate adds kappa itself.
        Every record and `initial_energy` gain "wall": per wall {"force", "energy", "nodes", "penetration"}
        (`femcy_explicit_wall_get`); with `*Energy Output` also "contact_energy", the sum of the walls' potentials, which
        "energy_total" then includes.  Without the keyword the records, the launches and the bits are unchanged."""
        deck = deck_view(inp)
        self._transient_gate(deck, "*Dynamic, explicit step", "lumped mass", motion=True)
        if deck.temperature_info is not None:
            raise ValueError("*Temperature in a *Dynamic, explicit step has not been supported: thermal loads are small "
                             "strain, an explicit step is not")
        self.geometric_nonlinear = True                               # post-processing: Green strain, the stress of f_int
        loads = LoadSchedule(self, deck, dirichlet=False)             # the held DOFs belong to the integrator
        ctx, max_time = self.ctx, loads.max_time
        self._external_force(loads, 1.0)                              # rhs = f at scale 1, once
        held = [self._dofset(bc["node_set"], bc["dof"]) for bc in loads.dirichletBCs]
        self.lumped_mass = ctx.lumped_mass(self.ELE, deck.density)
        self.mass_scaling = None
        if deck.mass_scaling is not None:                             # before the integrator: its inverse mass is derived once
            ms = deck.mass_scaling
            self.mass_scaling = ctx.lumped_mass_scale(self.lumped_mass, self.material_stiffness(), ms["factor"], ms["dt"],
                                                      ms["type"])
            self._say("fixed mass scaling: {scaled_elements} elements scaled, largest factor {max_factor}, total mass "
                      "{mass0} -> {mass1}".format(**self.mass_scaling))
        self.explicit = ex = ctx.explicit(self.lumped_mass, held)
        self._set_motion(deck, loads, ex, held)
        bulk, alpha = deck.bulk_viscosity, deck.damping_alpha
        b1, b2 = bulk if bulk is not None else (0.0, 0.0)
        if bulk is not None or alpha != 0.0:
            ctx.explicit_set_damping(ex, alpha, b1, b2, self.dilatational_modulus() if bulk is not None else 0.0)
        self._energy_balance = None
        if deck.energy_output:                                        # before the start, which zeroes the work sums
            ctx.explicit_energy_enable(ex, True)
            self._energy_balance = {"ex": ex, "strain0": None}
        self.walls, self.wall_kappa = [], 0.0
        if deck.dynamic_auto:
            return self._solve_explicit_auto(deck, loads, ex)
        if deck.dynamic["direct_user_control"]:
            dt = deck.time_incs["ini_inc"]
            self._set_walls(deck, ex, 2.0 / dt)
        else:
            ctx.assemble_K(-1)                                        # the matrix of the undeformed mesh, for the estimate only
            self.stats["assemblies"] += 1
            self.stable_dt, self.omega_bound = ctx.explicit_stable_dt(ex)
            self._set_walls(deck, ex, self.omega_bound)
            omega = self.omega_bound
            if self.walls:                                            # omega_c^2 <= omega^2 + kappa (femcy_explicit_set_wall)
                self.omega_contact = omega = float(np.sqrt(self.omega_bound * self.omega_bound + self.wall_kappa))
                self.stable_dt = 2.0 / omega
            if bulk is not None or alpha != 0.0:
                # lagged damping of critical fraction xi: h <= (2 / omega)(sqrt(1 + xi^2) - xi); the quadratic bulk term is
                # not known in advance and left to `scale factor`
                xi = b1 + alpha / (2.0 * omega)
                self.stable_dt *= np.sqrt(1.0 + xi * xi) - xi
            dt = deck.dynamic["scale_factor"] * self.stable_dt
        if not (np.isfinite(dt) and dt > 0.0):
            raise be.FemcyError("explicit step: no usable increment (dt = {})".format(dt), status=be.FEMCY_ENUMERIC)
        nsteps = max(1, int(np.ceil(max_time / dt * (1.0 - 1.0e-12))))
        self.dt = h = max_time / nsteps                               # <= dt: T is a whole number of steps
        scale0 = loads.amplitude(0.0)                                 # step k scales rhs by scale0 + k dscale: 1 and 0 in a
        dscale = loads.amplitude(h) - scale0                          # STEP, 0 and h / T on a ramp
        self._initial_state(deck, loads.dirichletBCs)
        ctx.explicit_start(ex, be.VEC_RHS, scale0)
        self.initial_energy = self._energies(ctx.explicit_kinetic_energy(ex, be.VEC_VEL))
        self.increments = []
        done, batch = 0, deck.dynamic["output_every"]
        while done < nsteps:
            k = min(batch, nsteps - done)                             # the last batch is clipped
            self._say("\033[40;33;1m >>>>> steps {} .. {} of {}, dt = {} \033[0m".format(done + 1, done + k, nsteps, h))
            ctx.explicit_advance(ex, k, h, be.VEC_RHS, scale0 + done * dscale, dscale)
            self.stats["force_evals"] += k
            done += k
            self.time0, self.time1 = self.time1, max_time if done == nsteps else done * h
            self._displacements_are_finite("{} steps of dt = {}".format(done, h))
            more = {"reaction": self._reaction(scale0 + done * dscale)} if self.motion else {}
            self._record(done, h, ctx.explicit_kinetic_energy(ex, be.VEC_VEL), **more)
        self.dof_old.copy_from(self.dof)

    def material_stiffness(self):
        """s_C = max eps:C:eps / eps:eps over symmetric strains of the material's small-strain matrix C (Voigt, engineering
        shear): the largest eigenvalue of D C D with D = diag(1 on the normal, sqrt 2 on the shear components).  Isotropic:
        3 lambda + 2 mu in 3-D, 2 lambda + 2 mu in plane strain, E / (1 - nu) in plane stress; neo-Hookean: the same with
        mu = 2 C1 and lambda = 2 D1 of its constant tangent."""
        C = np.asarray(self.material.C, dtype=np.float64)
        d = np.where(np.arange(len(C)) < self.dm, 1.0, np.sqrt(2.0))
        return float(np.linalg.eigvalsh(d[:, None] * C * d[None, :]).max())

    def dilatational_modulus(self):
        """M_d = rho c_d^2 of the bulk viscosity: C[0][0] of the small-strain matrix -- lambda + 2 mu in 3-D and plane
        strain, E / (1 - nu^2) in plane stress; neo-Hookean: 2 D1 + 4 C1, lambda + 2 mu with the constants as
        `material_stiffness` reads them."""
        return float(np.asarray(self.material.C, dtype=np.float64)[0][0])

    def _solve_explicit_auto(self, deck, loads, ex):
        """the `element by element` branch of solve_explicit, from the integrator on"""
        ctx, max_time = self.ctx, loads.max_time
        ramp = loads.amplitude(0.0) < 1.0                             # the device ramps the load itself, by its own clock
        s_C, sf, batch = self.material_stiffness(), deck.dynamic["scale_factor"], deck.dynamic["output_every"]
        self._initial_state(deck, loads.dirichletBCs)
        self.omega_bound = ctx.explicit_element_bound(ex, s_C, be.VEC_DOF)
        if deck.rigid_walls:                                          # the reference frequency is taken before the walls are
            self._set_walls(deck, ex, self.omega_bound)               # set; the estimate with them is the run's first
            self.omega_bound = ctx.explicit_element_bound(ex, s_C, be.VEC_DOF)
        self.stable_dt = 2.0 / self.omega_bound if self.omega_bound > 0.0 else np.inf
        if not np.isfinite(self.omega_bound):
            raise be.FemcyError("explicit step: no usable increment (omega = {})".format(self.omega_bound),
                                status=be.FEMCY_ENUMERIC)
        ctx.explicit_auto_begin(ex, s_C, sf, max_time, ramp, be.VEC_RHS)
        self.stats["force_evals"] += 1
        self.initial_energy = self._energies(ctx.explicit_kinetic_energy(ex, be.VEC_VEL))
        self.increments = []
        done, t = 0, 0.0
        while t < max_time:
            self._say("\033[40;33;1m >>>>> steps {} .., t = {} of {} \033[0m".format(done + 1, t, max_time))
            ctx.explicit_auto_advance(ex, batch, be.VEC_RHS)
            self.stats["force_evals"] += batch
            t, h_last, h_min, steps = ctx.explicit_auto_state(ex)
            self.time0, self.time1, self.dt = self.time1, t, h_last
            self._displacements_are_finite("{} steps, the last of dt = {}".format(steps, h_last))
            if steps == done and t < max_time:
                raise be.FemcyError("explicit step: the increment collapsed to 0 at t = {} of {} after {} steps (an unstable "
                                    "increment)".format(t, max_time, steps), status=be.FEMCY_ENUMERIC)
            done = steps
            more = {"reaction": self._reaction(loads.amplitude(t))} if self.motion else {}
            self._record(done, h_last, ctx.explicit_kinetic_energy(ex, be.VEC_VEL), dt_min=h_min, **more)
        self.dof_old.copy_from(self.dof)

    def _residual(self, dirichletBCs):
        """nodal force + K at the current dof, residual = f_int - rhs, Newton Dirichlet treatment,
        RMS norm (the block the reference repeats at :756-759, :779-783 and in inside_relaxation)."""
        self.ctx.residual_and_K(be.VEC_DOF, be.VEC_FORCE)     # assemble_nodal_force_GN + assemble_stiffnessMtrx,
        self.stats["force_evals"] += 1                        # one element pass (same dof for both)
        self.stats["assemblies"] += 1
        tg.c_equals_a_minus_b(self.residual_nodal_force, self.nodal_force, self.rhs)
        self.dirichletBC_forNewtonMethod(dirichletBCs)
        return tg.field_norm(self.residual_nodal_force)

    def advance_inc(self, inp, boundary_conditions: dict, show_newton_steps: bool = False, save2path: str = None,
                    window=None) -> Tuple[bool, int]:
        """one time increment: linear solve, or modified Newton with the reference's "boost" and
        "damp" line searches (reference :714-822)."""
        t0 = time.time()
        self.get_dsdx_and_vol()
        self.assemble_stiffnessMtrx()
        self._first_assembly_took(t0)
        self.impose_boundary_condition(boundary_conditions)

        if not inp.geometric_nonlinear:
            self.solve_dof()
            return True, 0

        dirichletBCs = boundary_conditions["dirichletBCs"]
        pre_residual = self._residual(dirichletBCs)
        if not hasattr(self, "ini_residual"):
            self.ini_residual = pre_residual          # latched once for the whole run
        self._say("\033[40;33;1m initial residual_nodal_force = {} \033[0m".format(self.ini_residual))
        if self.ini_residual < 1.e-9:
            return True, 0

        newton_loop = -1
        while pre_residual / (self.ini_residual + 1.e-30) >= 0.01:
            newton_loop += 1
            if newton_loop >= 24:
                return False, newton_loop
            try:
                du = self.solve_dof()                 # dof -= K^-1 residual
            except be.FemcyError as e:
                if e.status != be.FEMCY_ENUMERIC:
                    raise
                # the reference's solvers would hand back Inf/NaN here and trip the NaN test below on the
                # next residual; the device PCG reports the breakdown instead -> same outcome: cut the step
                self._say("linear solve broke down (NaN/Inf), automatically recompute with smaller time step")
                return False, newton_loop
            residual = self._residual(dirichletBCs)
            if np.isnan(residual):
                self._say("NaN occurs, automatically recompute with smaller time step")
                return False, newton_loop
            self._say("\033[40;33;1m newton_loop = {}, residual_nodal_force = {} \033[0m".format(newton_loop, residual))

            # boost: keep going along du while the residual declines (but not by 10x)
            relax_loop, relaxation = -1, 1.
            while 0.1 * pre_residual < residual < pre_residual:
                new_residual = residual
                relax_loop += 1
                if relax_loop >= 10:
                    break
                tg.a_equals_b_plus_c_mul_d(self.dof, self.dof, -relaxation, du)
                residual = self._residual(dirichletBCs)
                if residual > new_residual:
                    tg.a_equals_b_plus_c_mul_d(self.dof, self.dof, +relaxation, du)
                    residual = self._residual(dirichletBCs)
                    relaxation *= 0.5

            # damp: the residual grew -> take back half of the step (at most twice)
            relax_loop, relaxation = -1, 0.5
            while residual > pre_residual:
                relax_loop += 1
                if relax_loop >= 2:
                    break
                tg.a_equals_b_plus_c_mul_d(self.dof, self.dof, (1. - relaxation), du)
                tg.field_multiply(du, relaxation)
                residual = self._residual(dirichletBCs)

            pre_residual = residual
        return True, newton_loop

    # -------------------------------------------------------------------- post-processing
    def compute_strain_stress(self):
        """F, strain (infinitesimal / Green), Cauchy stress (small deformation: constitutiveOfSmallDeform;
        nlgeom: the stress of the last force evaluation) and von Mises stress per Gauss point, on the device
        (reference :436-501).  Results: .F, .strain, .cauchy_stress, .mises_stress (`.to_numpy()`)."""
        self.ctx.compute_strain_stress(be.VEC_DOF, large=self.geometric_nonlinear)
        if self._thermal is not None:        # sigma = C : eps(u) - sigma_th at the temperature of the last increment
            self.ctx.thermal_stress(self._thermal["id"], self._thermal["scale"])

    def get_elasEng(self):
        """total elastic energy = sum over Gauss points of elasticEnergyDensity(F) * vol (reference :592-606).  In and
        after a `*Dynamic` step it is the energy of the infinitesimal strain on the undeformed mesh, u.Ku / 2: the
        analysis is linear there, and that is the energy its integrator exchanges with the kinetic one (the reference's
        density is that of the Green strain, which is off by the order of the strain)."""
        if self._linear_energy:
            self.elsEng = self.ctx.elastic_energy(be.VEC_DOF, small=True)
        else:
            self.elsEng = self.ctx.elastic_energy(be.VEC_DOF)
        return self.elsEng
