"""ctypes binding of the C ABI of include/femcy.h.

Two libraries implement it:
  libfemcy_hip.so  the product: hand-written HIP kernels for gfx950 (csrc/).  The default, and the only thing a run on
                   a GPU box ever uses.
  libfemcy_cpu.so  the same ABI on the host (csrc_cpu/, C++ / OpenMP; the arithmetic of an element is the code the HIP
                   kernels run, csrc/element_math.hpp).  Loaded ONLY when FEMCY_BACKEND=cpu is set (or
                   Context(backend="cpu")): there is no silent fallback -- if the HIP library is missing, or no MI355X
                   is visible, construction of a `Context` raises `FemcyError`.  (The CPU restatement of the reference
                   in `oracle/` is something else again: test infrastructure only.)

`import torch` happens before the HIP library is loaded so that libfemcy_hip.so binds to the HIP
runtime (and, for multi-GPU runs, the RCCL) that PyTorch already mapped into the process: the
wheel bundles its own libamdhip64.so/librccl.so with the same SONAMEs as /opt/rocm's, and two
HIP runtimes in one process do not mix.
"""
from __future__ import annotations

import ctypes as C
import os
from typing import Optional, Sequence

import numpy as np

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.environ.get("FEMCY_HIP_LIB") or os.path.join(_HERE, "libfemcy_hip.so")   # override: kernel A/B runs
CPU_LIB_PATH = os.environ.get("FEMCY_CPU_LIB") or os.path.join(_HERE, "libfemcy_cpu.so")


def default_backend() -> str:
    """"hip" unless FEMCY_BACKEND=cpu was set explicitly"""
    kind = os.environ.get("FEMCY_BACKEND", "hip").lower()
    if kind not in ("hip", "cpu"):
        raise FemcyError(f"FEMCY_BACKEND={kind!r}: expected 'hip' or 'cpu'")
    return kind

# enum femcy_vec
VEC_DOF, VEC_RHS, VEC_RESIDUAL, VEC_FORCE, VEC_DU, VEC_DOF_OLD, VEC_X, VEC_TMP0, VEC_TMP1 = range(9)
VEC_VEL, VEC_ACC = 9, 10     # implicit dynamics: nodal velocities and accelerations
# enum femcy_gpfield
GP_DSDX, GP_VOL, GP_F, GP_SIGMA, GP_STRAIN, GP_MISES, GP_ENERGY = range(7)
# enum femcy_option
OPT_ASSEMBLY, OPT_PCG_POLL, OPT_TIMING, OPT_SPMV_VARIANT, OPT_EW_GRID, OPT_PCG_GRAPH, OPT_SELL_SIGMA = range(7)
OPT_TANGENT = 7          # 0 = the reference's matrix (default), 1 = consistent tangent (extension)
OPT_EXCHANGE = 8         # multi-rank: 0 = packed all-reduce (default), 1 = neighbour send/recv
OPT_PCG_STORAGE_ORDER = 13   # 1 (default) = the single-rank three-launch PCG keeps its vectors in storage order
OPT_DIRECT_MAX_BYTES = 17   # femcy_direct_solve: largest band it may allocate (bytes, default 48 GiB)
OPT_NODE_ORDER = 14      # 0 = caller's numbering, 1 (default) = measured choice among coordinate orders, 2 + k = forced (before build_pattern)
OPT_PCG_PERSIST = 11     # 1 (default) = persistent one-launch PCG (single rank, <= ~7e5 DOF, matrix <= Infinity Cache); 2 = any matrix size
OPT_PCG_PERSIST_MULTI = 12   # 1 (default) = the persistent kernel across ranks once the mailboxes are exchanged and agreed
OPT_PCG_SMALL = 10       # 1 (default) = one persistent launch per solve for systems that fit LDS
TUNE_SMALL_REG_ROWS = 108    # small-system PCG: block rows per wave kept in registers (-1 default: a wave's share of the longest row; femcy.h)
TUNE_PERSIST_VARIANT = 109   # persistent PCG variant bits (-1 default; femcy.h)
TUNE_SKIP_OCCUPANCY_CHECK = 111
TUNE_BARRIER_SPIN_LIMIT = 112
TUNE_PERSIST_L2_ROWS = 113
TUNE_SPMV_WG_PER_XCD = 101  # SpMV workgroups per XCD: 0 auto (512 beyond 512 tasks per XCD, else 256)
TUNE_SPMV_ROT = 119         # SpMV task lists: -1 auto (by the spread of the row lengths), 0 plain, 1..63 rotated rounds, 64 balanced
TUNE_PAIRS = 117            # PAIRS assembly knobs (femcy.h)
TUNE_DIRECT_UPDATE = 115    # femcy_direct_solve tile update: -1 auto, 0 VALU, 1 / 2 matrix cores
TUNE_PERSIST_MAX_MB = 114   # persistent PCG: streamed-matrix limit in MiB (0 = none, the default since round 5; 240 = rounds 2-4)
OPT_OVERLAP = 9          # multi-rank, neighbour exchange: 1 (default) = exchange overlapped with the interior product
ASM_GATHER, ASM_ATOMIC, ASM_ROWS, ASM_AUTO, ASM_GATHER_SYM, ASM_GATHER_SYM_ROWSUM, ASM_ROWS2, ASM_ROWS4, ASM_PAIRS = 0, 1, 2, 3, 4, 5, 6, 8, 9
ASM_ROWS3 = 7               # retired: the HIP library refuses it (the name stays so that callers of the old list still import)

EXPORTS = [
    "femcy_ctx_create", "femcy_ctx_destroy", "femcy_last_error", "femcy_version", "femcy_set_option", "femcy_sync",
    "femcy_set_mesh", "femcy_set_element", "femcy_set_material", "femcy_build_pattern", "femcy_get_pattern_info",
    "femcy_get_assembly_used",
    "femcy_vec_upload", "femcy_vec_download", "femcy_vec_fill", "femcy_vec_copy", "femcy_vec_scatter",
    "femcy_vec_sub", "femcy_vec_axpy", "femcy_vec_scale", "femcy_vec_norm", "femcy_vec_absmax",
    "femcy_assemble_K", "femcy_internal_force", "femcy_residual_and_K", "femcy_apply_dirichlet_linear", "femcy_apply_dirichlet_newton",
    "femcy_dofset_create", "femcy_dofset_dirichlet_newton", "femcy_dofset_dirichlet_linear", "femcy_dofset_fill",
    "femcy_dofset_scatter", "femcy_dofset_add", "femcy_bodyload_create", "femcy_bodyload_weights", "femcy_bodyload_apply",
    "femcy_thermal_create", "femcy_thermal_force", "femcy_thermal_apply", "femcy_thermal_stress",
    "femcy_mass_create", "femcy_mass_get", "femcy_mass_apply", "femcy_mass_add_to_K", "femcy_mass_kinetic_energy",
    "femcy_newmark_predict", "femcy_newmark_update",
    "femcy_lumped_mass_create", "femcy_lumped_mass_get", "femcy_explicit_create", "femcy_explicit_start",
    "femcy_explicit_advance", "femcy_explicit_kinetic_energy", "femcy_explicit_stable_dt",
    "femcy_explicit_element_bound", "femcy_explicit_auto_begin", "femcy_explicit_auto_advance", "femcy_explicit_auto_state",
    "femcy_explicit_set_damping", "femcy_lumped_mass_scale", "femcy_lumped_mass_get_scaling",
    "femcy_amplitude_create", "femcy_explicit_set_motion", "femcy_explicit_energy_enable", "femcy_explicit_energy_get",
    "femcy_explicit_set_wall", "femcy_explicit_wall_get",
    "femcy_loadset_create", "femcy_loadset_neumann", "femcy_loadset_neumann_add", "femcy_spmv", "femcy_pcg", "femcy_compute_strain_stress", "femcy_elastic_energy", "femcy_elastic_energy_small", "femcy_extrapolate",
    "femcy_get_K_ell", "femcy_get_K_bsr", "femcy_get_gp_field", "femcy_timing",
    "femcy_timing_reset", "femcy_comm_unique_id", "femcy_comm_local_id", "femcy_comm_init", "femcy_comm_info", "femcy_comm_set_neighbours",
    "femcy_comm_tune", "femcy_iface_sum",
    "femcy_probe_stream", "femcy_probe_exchange", "femcy_persist_streamed_bytes",
    "femcy_comm_mailbox_export", "femcy_comm_mailbox_import", "femcy_comm_persist_agree",
    "femcy_comm_shm_id", "femcy_comm_allgather_host", "femcy_get_node_order", "femcy_probe_mailbox", "femcy_probe_spmv",
    "femcy_direct_solve", "femcy_direct_plan",
]


class FemcyError(RuntimeError):
    """a non-zero femcy_status; `.status` carries the code (include/femcy.h)."""

    def __init__(self, msg, status=None):
        super().__init__(msg)
        self.status = status


FEMCY_ENUMERIC = -4
FEMCY_ENOMEM = -6
# femcy_lumped_mass_scale: the rule that turns a target increment into factors (*Fixed Mass Scaling, type=)
MS_BELOW_MIN, MS_SET_EQUAL_DT, MS_UNIFORM = 0, 1, 2
MS_TYPES = {"below min": MS_BELOW_MIN, "set equal dt": MS_SET_EQUAL_DT, "uniform": MS_UNIFORM}
# femcy_amplitude_create: the kind of a curve (*Amplitude, definition=)
AMP_TABULAR, AMP_SMOOTH_STEP = 0, 1
AMP_KINDS = {"tabular": AMP_TABULAR, "smooth step": AMP_SMOOTH_STEP}
AMP_MAX_POINTS = 16
# femcy_explicit_set_wall: the most walls an integrator takes
WALL_MAX = 4
# femcy_explicit_energy_get: the four work sums of the energy balance (*Energy Output)
EN_LOAD, EN_INTERNAL, EN_ALPHA, EN_BOUNDARY = 0, 1, 2, 3


class DirectInfo(C.Structure):
    _fields_ = [("n", C.c_int64), ("band_bytes", C.c_int64), ("bandwidth", C.c_int32), ("panels", C.c_int32),
                ("singular_at", C.c_int32), ("negative_pivots", C.c_int32), ("refinements", C.c_int32),
                ("reserved", C.c_int32), ("residual", C.c_double)]


class PatternInfo(C.Structure):
    _fields_ = [("n", C.c_int64), ("nnzb", C.c_int64), ("nnz", C.c_int64), ("max_row_blocks", C.c_int32),
                ("ell_width", C.c_int32), ("stored_blocks", C.c_int64), ("nslices", C.c_int32),
                ("max_node_elems", C.c_int32)]


class Timing(C.Structure):
    _fields_ = [("geom_ms", C.c_double), ("geom_launches", C.c_int64),
                ("assemble_ms", C.c_double), ("assemble_launches", C.c_int64),
                ("force_ms", C.c_double), ("force_launches", C.c_int64),
                ("spmv_ms", C.c_double), ("spmv_launches", C.c_int64),
                ("pcg_ms", C.c_double), ("pcg_iters", C.c_int64),
                ("persist_ms", C.c_double), ("persist_launches", C.c_int64), ("persist_iters", C.c_int64),
                ("solves_three", C.c_int64), ("solves_small", C.c_int64), ("solves_persist", C.c_int64),
                ("barrier_timeouts", C.c_int64)]

    def as_dict(self):
        return {k: getattr(self, k) for k, _ in self._fields_}


_libs = {}


def load_library(require_gpu_runtime: bool = True, kind: Optional[str] = None):
    """dlopen the library of the backend (default: FEMCY_BACKEND, i.e. "hip").  Raises FemcyError when the in-tree
    library has not been built."""
    kind = kind or default_backend()
    if kind in _libs:
        return _libs[kind]
    if kind == "cpu":
        if not os.path.exists(CPU_LIB_PATH):
            raise FemcyError(f"{CPU_LIB_PATH} not found: build it with `bash femcy_amd/csrc_cpu/build.sh`")
        lib = C.CDLL(CPU_LIB_PATH)
        return _bind(lib, kind)
    if not os.path.exists(LIB_PATH):
        raise FemcyError(f"{LIB_PATH} not found: build it with `python -c 'import __graft_entry__ as g; g.build()'` "
                         "(there is no silent CPU fallback; FEMCY_BACKEND=cpu selects the host backend explicitly)")
    if require_gpu_runtime:
        import torch  # noqa: F401  (maps PyTorch's HIP runtime first; see module docstring)
    lib = C.CDLL(LIB_PATH, mode=C.RTLD_GLOBAL)
    return _bind(lib, kind)


def _bind(lib, kind):
    p, i32, i64, f64 = C.c_void_p, C.c_int32, C.c_int64, C.c_double
    cint = C.c_int
    sig = {
        "femcy_ctx_create": [cint, C.POINTER(p)], "femcy_ctx_destroy": [p], "femcy_version": [],
        "femcy_set_option": [p, cint, i64], "femcy_sync": [p],
        "femcy_set_mesh": [p, i32, i32, p, i32, i32, p], "femcy_set_element": [p, i32, p, p, i32],
        "femcy_set_material": [p, i32, p, p, i32], "femcy_build_pattern": [p],
        "femcy_get_pattern_info": [p, C.POINTER(PatternInfo)], "femcy_get_assembly_used": [p, C.POINTER(i32)],
        "femcy_vec_upload": [p, cint, p, i64], "femcy_vec_download": [p, cint, p, i64],
        "femcy_vec_fill": [p, cint, f64], "femcy_vec_copy": [p, cint, cint],
        "femcy_vec_scatter": [p, cint, p, p, i32], "femcy_vec_sub": [p, cint, cint, cint],
        "femcy_vec_axpy": [p, cint, cint, f64, cint], "femcy_vec_scale": [p, cint, f64],
        "femcy_vec_norm": [p, cint, C.POINTER(f64)], "femcy_vec_absmax": [p, cint, C.POINTER(f64)],
        "femcy_assemble_K": [p, cint], "femcy_internal_force": [p, cint, cint], "femcy_residual_and_K": [p, cint, cint],
        "femcy_apply_dirichlet_linear": [p, p, p, i32, cint], "femcy_apply_dirichlet_newton": [p, p, i32, cint],
        "femcy_dofset_create": [p, p, i32, C.POINTER(i32)], "femcy_dofset_dirichlet_newton": [p, i32, cint],
        "femcy_dofset_dirichlet_linear": [p, i32, f64, cint], "femcy_dofset_fill": [p, i32, cint, f64],
        "femcy_dofset_scatter": [p, i32, cint, p], "femcy_dofset_add": [p, i32, cint, f64],
        "femcy_bodyload_create": [p, p, i32, p, C.POINTER(i32)], "femcy_bodyload_weights": [p, i32, p],
        "femcy_bodyload_apply": [p, i32, p, cint, i32],
        "femcy_thermal_create": [p, p, f64, p, C.POINTER(i32)], "femcy_thermal_force": [p, i32, p],
        "femcy_thermal_apply": [p, i32, f64, cint, i32], "femcy_thermal_stress": [p, i32, f64],
        "femcy_mass_create": [p, i32, p, p, p, f64, C.POINTER(i32)], "femcy_mass_get": [p, i32, p],
        "femcy_mass_apply": [p, i32, cint, cint, f64, i32], "femcy_mass_add_to_K": [p, i32, f64, i32],
        "femcy_mass_kinetic_energy": [p, i32, cint, C.POINTER(f64)],
        "femcy_newmark_predict": [p, cint, cint, cint, cint, f64, f64, f64],
        "femcy_newmark_update": [p, cint, cint, cint, cint, f64, f64, f64],
        "femcy_lumped_mass_create": [p, i32, p, p, p, f64, C.POINTER(i32)], "femcy_lumped_mass_get": [p, i32, p],
        "femcy_explicit_create": [p, i32, i32, p, C.POINTER(i32)], "femcy_explicit_start": [p, i32, cint, f64],
        "femcy_explicit_advance": [p, i32, cint, i32, f64, f64, f64],
        "femcy_explicit_kinetic_energy": [p, i32, cint, C.POINTER(f64)],
        "femcy_explicit_stable_dt": [p, i32, C.POINTER(f64), C.POINTER(f64)],
        "femcy_explicit_element_bound": [p, i32, cint, f64, C.POINTER(f64)],
        "femcy_explicit_auto_begin": [p, i32, cint, f64, f64, f64, i32],
        "femcy_explicit_auto_advance": [p, i32, cint, i32],
        "femcy_explicit_set_damping": [p, i32, f64, f64, f64, f64],
        "femcy_lumped_mass_scale": [p, i32, f64, f64, f64, i32, C.POINTER(f64), C.POINTER(f64), C.POINTER(i64), C.POINTER(f64)],
        "femcy_lumped_mass_get_scaling": [p, i32, p],
        "femcy_amplitude_create": [p, i32, i32, p, p, C.POINTER(i32)],
        "femcy_explicit_set_motion": [p, i32, i32, p, p, p],
        "femcy_explicit_energy_enable": [p, i32, i32], "femcy_explicit_energy_get": [p, i32, p],
        "femcy_explicit_set_wall": [p, i32, i32, p, p, p], "femcy_explicit_wall_get": [p, i32, i32, p],
        "femcy_explicit_auto_state": [p, i32, C.POINTER(f64), C.POINTER(f64), C.POINTER(f64), C.POINTER(C.c_int64)],
        "femcy_loadset_create": [p, i32, i32, i32, p, p, p, p, p, i32, p, p, C.POINTER(i32)],
        "femcy_loadset_neumann": [p, i32, f64, p, cint],
        "femcy_loadset_neumann_add": [p, i32, f64, p, cint],
        "femcy_spmv": [p, cint, cint],
        "femcy_pcg": [p, cint, cint, f64, i32, C.POINTER(i32), C.POINTER(f64), C.POINTER(f64)],
        "femcy_compute_strain_stress": [p, cint, cint], "femcy_elastic_energy": [p, cint, C.POINTER(f64)],
        "femcy_elastic_energy_small": [p, cint, C.POINTER(f64)],
        "femcy_extrapolate": [p, cint, cint, p, p],
        "femcy_get_K_ell": [p, p, p], "femcy_get_K_bsr": [p, p, p, p], "femcy_get_gp_field": [p, cint, p],
        "femcy_timing": [p, C.POINTER(Timing)], "femcy_timing_reset": [p],
        "femcy_comm_unique_id": [p], "femcy_comm_local_id": [p], "femcy_comm_info": [p, p, p, p],
        "femcy_comm_set_neighbours": [p, i32, p, p, p], "femcy_comm_tune": [p, i32, C.POINTER(i32), p], "femcy_comm_init": [p, i32, i32, p, i32, p, p, i32, p],
        "femcy_iface_sum": [p, cint],
        "femcy_probe_stream": [p, i64, i32, i32, C.POINTER(f64), C.POINTER(i64)],
        "femcy_probe_exchange": [p, i32, i32, C.POINTER(f64)],
        "femcy_persist_streamed_bytes": [p, C.POINTER(i64)],
        "femcy_comm_mailbox_export": [p, p], "femcy_comm_mailbox_import": [p, i32, p],
        "femcy_comm_shm_id": [p, i64], "femcy_comm_allgather_host": [p, p, i32, p],
        "femcy_get_node_order": [p, C.POINTER(i32), p], "femcy_probe_mailbox": [p, i32, C.POINTER(f64)],
        "femcy_probe_spmv": [p, i32, i32, C.POINTER(f64)],
        "femcy_comm_persist_agree": [p, C.POINTER(i32)],
        "femcy_direct_solve": [p, cint, cint, C.POINTER(DirectInfo)],
        "femcy_direct_plan": [p, C.POINTER(DirectInfo)],
    }
    for name, args in sig.items():
        fn = getattr(lib, name)
        fn.argtypes = args
        fn.restype = cint
    lib.femcy_last_error.argtypes = []
    lib.femcy_last_error.restype = C.c_char_p
    _libs[kind] = lib
    return lib


def _ptr(a: Optional[np.ndarray]):
    return None if a is None else a.ctypes.data_as(C.c_void_p)


def _f64(a):
    return np.ascontiguousarray(a, dtype=np.float64)


def _i32(a):
    return np.ascontiguousarray(a, dtype=np.int32)


class DeviceVector:
    """handle to one of the context's HBM-resident solver vectors; quacks like the ti.field the
    reference exposes (`to_numpy`, `from_numpy`, `fill`, `copy_from`, `shape`)."""

    def __init__(self, ctx: "Context", vec_id: int):
        self.ctx, self.id = ctx, vec_id

    @property
    def shape(self):
        return (self.ctx.n,)

    def to_numpy(self) -> np.ndarray:
        return self.ctx.download(self.id)

    def from_numpy(self, arr):
        self.ctx.upload(self.id, arr)

    def fill(self, value: float):
        self.ctx._call("femcy_vec_fill", self.id, float(value))

    def copy_from(self, other: "DeviceVector"):
        self.ctx._call("femcy_vec_copy", self.id, other.id)

    def __len__(self):
        return self.ctx.n


class GaussField:
    """handle to a device Gauss-point field (dsdx, vol, F, cauchy stress)."""

    def __init__(self, ctx: "Context", which: int, tail_shape):
        self.ctx, self.which, self._tail = ctx, which, tuple(tail_shape)

    @property
    def shape(self):
        return (self.ctx.ne, self.ctx.nGP)

    def to_numpy(self) -> np.ndarray:
        out = np.empty((self.ctx.ne, self.ctx.nGP) + self._tail, dtype=np.float64)
        self.ctx._call("femcy_get_gp_field", self.which, _ptr(out))
        return out


class Context:
    """one HIP device + stream + all device state of one System_of_equations (backend "cpu": the host)."""

    def __init__(self, device: int = 0, backend: Optional[str] = None):
        self.backend = backend or default_backend()
        self.lib = load_library(kind=self.backend)
        h = C.c_void_p()
        rc = self.lib.femcy_ctx_create(int(device), C.byref(h))
        if rc != 0:
            raise FemcyError(f"femcy_ctx_create({device}) -> {rc}: {self.lib.femcy_last_error().decode()}")
        self._h = h
        self.device = device
        self.n = self.nn = self.dm = self.ne = self.npe = self.nGP = 0

    # ------------------------------------------------------------------------------- plumbing
    def _call(self, name, *args):
        rc = getattr(self.lib, name)(self._h, *args)
        if rc != 0:
            raise FemcyError(f"{name} -> {rc}: {self.lib.femcy_last_error().decode()}", status=rc)

    def close(self):
        if getattr(self, "_h", None):
            self.lib.femcy_ctx_destroy(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def set_option(self, opt: int, value: int):
        self._call("femcy_set_option", int(opt), int(value))

    def sync(self):
        self._call("femcy_sync")

    # --------------------------------------------------------------------- problem definition
    def set_mesh(self, nodes: np.ndarray, elements: np.ndarray):
        nodes, elements = _f64(nodes), _i32(elements)
        self.nn, self.dm = nodes.shape
        self.ne, self.npe = elements.shape
        self.n = self.nn * self.dm
        self._call("femcy_set_mesh", self.nn, self.dm, _ptr(nodes), self.ne, self.npe, _ptr(elements))

    def set_element(self, ELE):
        """ELE: an element_zoo plugin (anything with .tables())."""
        t = ELE.tables()
        if t["npe"] != self.npe or t["dm"] != self.dm:
            raise FemcyError(f"element plugin (npe={t['npe']}, dm={t['dm']}) does not match mesh "
                             f"(npe={self.npe}, dm={self.dm})")
        self.nGP = int(t["nGP"])
        self._call("femcy_set_element", self.nGP, _ptr(_f64(t["dN"])), _ptr(_f64(t["w"])), int(t["voigt_kind"]))

    def set_material(self, material):
        params = _f64(material.params)
        self._call("femcy_set_material", int(material.kind), _ptr(_f64(material.C)), _ptr(params), int(params.size))

    def build_pattern(self) -> PatternInfo:
        self._call("femcy_build_pattern")
        return self.pattern_info()

    def node_order(self):
        """(order taken by build_pattern: 0 = the caller's numbering, 1 + k = coordinate order k; mean cache lines per
        wavefront gather of every evaluated candidate, the caller's numbering first)"""
        used, lines = C.c_int32(), (C.c_double * 7)()
        self._call("femcy_get_node_order", C.byref(used), C.cast(lines, C.c_void_p))
        return int(used.value), [float(v) for v in lines]

    def pattern_info(self) -> PatternInfo:
        info = PatternInfo()
        self._call("femcy_get_pattern_info", C.byref(info))
        return info

    # --------------------------------------------------------------------------------- vectors
    def vector(self, vec_id: int) -> DeviceVector:
        return DeviceVector(self, vec_id)

    def upload(self, vec_id: int, arr):
        a = _f64(arr).ravel()
        self._call("femcy_vec_upload", int(vec_id), _ptr(a), a.size)

    def download(self, vec_id: int) -> np.ndarray:
        out = np.empty(self.n, dtype=np.float64)
        self._call("femcy_vec_download", int(vec_id), _ptr(out), out.size)
        return out

    def scatter(self, vec_id: int, idx, vals):
        idx, vals = _i32(idx).ravel(), _f64(vals).ravel()
        self._call("femcy_vec_scatter", int(vec_id), _ptr(idx), _ptr(vals), idx.size)

    def vec_sub(self, c: int, a: int, b: int):
        self._call("femcy_vec_sub", c, a, b)

    def vec_axpy(self, a: int, b: int, c: float, d: int):
        self._call("femcy_vec_axpy", a, b, float(c), d)

    def vec_scale(self, v: int, s: float):
        self._call("femcy_vec_scale", v, float(s))

    def vec_norm(self, v: int) -> float:
        out = C.c_double()
        self._call("femcy_vec_norm", v, C.byref(out))
        return out.value

    def vec_absmax(self, v: int) -> float:
        out = C.c_double()
        self._call("femcy_vec_absmax", v, C.byref(out))
        return out.value

    # -------------------------------------------------------------------------------- hot path
    def assemble_K(self, u_vec: int = VEC_DOF):
        self._call("femcy_assemble_K", int(u_vec))

    def assembly_used(self) -> int:
        """the femcy_assembly mode (ASM_*) the last assemble_K / residual_and_K ran, AUTO resolved."""
        out = C.c_int32()
        self._call("femcy_get_assembly_used", C.byref(out))
        return out.value

    def internal_force(self, u_vec: int = VEC_DOF, f_vec: int = VEC_FORCE):
        self._call("femcy_internal_force", int(u_vec), int(f_vec))

    def residual_and_K(self, u_vec: int = VEC_DOF, f_vec: int = VEC_FORCE):
        """internal force + matrix of one Newton residual evaluation from ONE element pass."""
        self._call("femcy_residual_and_K", int(u_vec), int(f_vec))

    def dirichlet_linear(self, dofs, vals, rhs_vec: int = VEC_RHS):
        dofs, vals = _i32(dofs).ravel(), _f64(vals).ravel()
        self._call("femcy_apply_dirichlet_linear", _ptr(dofs), _ptr(vals), dofs.size, int(rhs_vec))

    def dirichlet_newton(self, dofs, residual_vec: int = VEC_RESIDUAL):
        dofs = _i32(dofs).ravel()
        self._call("femcy_apply_dirichlet_newton", _ptr(dofs), dofs.size, int(residual_vec))

    # device-resident DOF lists of *Boundary blocks (no per-call upload / sync)
    def dofset(self, dofs) -> int:
        dofs = _i32(dofs).ravel()
        out = C.c_int32()
        self._call("femcy_dofset_create", _ptr(dofs), dofs.size, C.byref(out))
        return out.value

    # device-resident *Dsload surfaces
    def loadset(self, ELE, load_elem, load_ft, nfn=None) -> int:
        """load_elem[k]: element owning loaded facet k; load_ft[k]: its facet type (index into ELE.facet_tables(nfn):
        the facets of nfn nodes, or all of them where the element has one facet arity)."""
        t = ELE.facet_tables(nfn)
        load_elem, load_ft = _i32(load_elem).ravel(), _i32(load_ft).ravel()
        out = C.c_int32()
        self._call("femcy_loadset_create", t["nft"], t["nfn"], t["nip"], _ptr(t["ft_nodes"]), _ptr(t["N"]),
                   _ptr(t["dN"]), _ptr(t["normal"]), _ptr(t["weight"]), load_elem.size, _ptr(load_elem), _ptr(load_ft),
                   C.byref(out))
        return out.value

    def loadset_neumann(self, ls: int, traction: float, direction=None, rhs_vec: int = VEC_RHS, add: bool = False):
        """rhs = the set's consistent nodal loads (add: rhs += them, femcy_loadset_neumann_add)."""
        d = None if direction is None or len(direction) == 0 else _f64(direction).ravel()
        if d is not None and d.size < self.dm:
            raise FemcyError(f"load direction needs {self.dm} components")
        self._call("femcy_loadset_neumann_add" if add else "femcy_loadset_neumann", int(ls), float(traction),
                   None if d is None else _ptr(d), int(rhs_vec))

    def dofset_dirichlet_newton(self, ds: int, residual_vec: int = VEC_RESIDUAL):
        self._call("femcy_dofset_dirichlet_newton", int(ds), int(residual_vec))

    def dofset_dirichlet_linear(self, ds: int, value: float, rhs_vec: int = VEC_RHS):
        self._call("femcy_dofset_dirichlet_linear", int(ds), float(value), int(rhs_vec))

    def dofset_fill(self, ds: int, vec_id: int, value: float):
        self._call("femcy_dofset_fill", int(ds), int(vec_id), float(value))

    def dofset_scatter(self, ds: int, vec_id: int, vals):
        self._call("femcy_dofset_scatter", int(ds), int(vec_id), _ptr(_f64(vals).ravel()))

    def dofset_add(self, ds: int, vec_id: int, value: float):
        """vec[dofs of the set] += value (*Cload)."""
        self._call("femcy_dofset_add", int(ds), int(vec_id), float(value))

    # device-resident body loads (*Dload GRAV / BX / BY / BZ)
    def bodyload(self, ELE, elems=None) -> int:
        """nodal weights m_a = sum N_a |det J| w over `elems` (None: every element) on the undeformed geometry."""
        N = _f64(ELE.tables()["N"])
        if N.shape != (self.nGP, self.npe):
            raise FemcyError(f"shape-function table must be {self.nGP} x {self.npe}, got {N.shape}")
        sel = None if elems is None else _i32(elems).ravel()
        out = C.c_int32()
        self._call("femcy_bodyload_create", _ptr(N), 0 if sel is None else sel.size,
                   None if sel is None else (_ptr(sel) if sel.size else _ptr(np.zeros(1, np.int32))), C.byref(out))
        return out.value

    def bodyload_weights(self, bl: int) -> np.ndarray:
        out = np.empty(self.nn, dtype=np.float64)
        self._call("femcy_bodyload_weights", int(bl), _ptr(out))
        return out

    def bodyload_apply(self, bl: int, b, rhs_vec: int = VEC_RHS, add: bool = False):
        """rhs = m_a * b (add: rhs += it); b = force per unit volume, dm components."""
        b = _f64(b).ravel()
        if b.size < self.dm:
            raise FemcyError(f"body force needs {self.dm} components")
        self._call("femcy_bodyload_apply", int(bl), _ptr(b), int(rhs_vec), 1 if add else 0)

    # device-resident thermal loads (*Expansion + *Temperature)
    def thermal(self, ELE, alpha: float, dT) -> int:
        """consistent nodal load of the thermal strain alpha * dT I at scale 1, dT = nodal temperature changes [nn], on
        the undeformed geometry with the material of this moment (linear materials only)."""
        N = _f64(ELE.tables()["N"])
        if N.shape != (self.nGP, self.npe):
            raise FemcyError(f"shape-function table must be {self.nGP} x {self.npe}, got {N.shape}")
        dT = _f64(dT).ravel()
        if dT.size != self.nn:
            raise FemcyError(f"temperature field needs {self.nn} nodal values, got {dT.size}")
        out = C.c_int32()
        self._call("femcy_thermal_create", _ptr(N), float(alpha), _ptr(dT), C.byref(out))
        return out.value

    def thermal_force(self, th: int) -> np.ndarray:
        out = np.empty(self.n, dtype=np.float64)
        self._call("femcy_thermal_force", int(th), _ptr(out))
        return out

    def thermal_apply(self, th: int, scale: float, rhs_vec: int = VEC_RHS, add: bool = False):
        """rhs = scale * f_unit (add: rhs += it)."""
        self._call("femcy_thermal_apply", int(th), float(scale), int(rhs_vec), 1 if add else 0)

    def thermal_stress(self, th: int, scale: float):
        """after compute_strain_stress(large=False): sigma -= scale * sigma_th, von Mises again."""
        self._call("femcy_thermal_stress", int(th), float(scale))

    # device-resident consistent mass and the Newmark vector passes (*Dynamic)
    def mass(self, ELE, rho: float) -> int:
        """consistent mass M (x) I of the undeformed mesh at density rho, one scalar per stored block of K, integrated
        with the plug-in's mass_rule()."""
        t = ELE.mass_tables()
        if t["Nq"].shape != (t["nq"], self.npe) or t["dNq"].shape != (t["nq"], self.npe, self.dm):
            raise FemcyError(f"mass-rule tables do not match the mesh (npe={self.npe}, dm={self.dm})")
        out = C.c_int32()
        self._call("femcy_mass_create", int(t["nq"]), _ptr(t["Nq"]), _ptr(t["dNq"]), _ptr(t["wq"]), float(rho),
                   C.byref(out))
        return out.value

    def mass_get(self, ms: int):
        """scipy.sparse.csr_matrix [nn, nn] of the scalars m_ab (ascending columns, the block order of get_K_bsr)."""
        import scipy.sparse as sp
        info = self.pattern_info()
        rowptr = np.empty(self.nn + 1, dtype=np.int32)
        col = np.empty(info.nnzb, dtype=np.int32)
        kv = np.empty((info.nnzb, self.dm, self.dm), dtype=np.float64)
        self._call("femcy_get_K_bsr", _ptr(rowptr), _ptr(col), _ptr(kv))
        vals = np.empty(info.nnzb, dtype=np.float64)
        self._call("femcy_mass_get", int(ms), _ptr(vals))
        return sp.csr_matrix((vals, col, rowptr), shape=(self.nn, self.nn))

    def mass_apply(self, ms: int, x_vec: int, y_vec: int, scale: float = 1.0, add: bool = False):
        """y = [y +] scale * (M (x) I) x"""
        self._call("femcy_mass_apply", int(ms), int(x_vec), int(y_vec), float(scale), 1 if add else 0)

    def mass_add_to_K(self, ms: int, c: float, overwrite: bool = False):
        """K += c * M (x) I on the block diagonals (overwrite: K := c * M (x) I)"""
        self._call("femcy_mass_add_to_K", int(ms), float(c), 1 if overwrite else 0)

    def mass_kinetic_energy(self, ms: int, v_vec: int = VEC_VEL) -> float:
        out = C.c_double()
        self._call("femcy_mass_kinetic_energy", int(ms), int(v_vec), C.byref(out))
        return out.value

    def newmark_predict(self, u_vec: int, v_vec: int, a_vec: int, out_vec: int, c0: float, c1: float, c2: float):
        """out = c0 u + c1 v + c2 a"""
        self._call("femcy_newmark_predict", int(u_vec), int(v_vec), int(a_vec), int(out_vec), float(c0), float(c1), float(c2))

    def newmark_update(self, u_new_vec: int, u_vec: int, v_vec: int, a_vec: int, beta: float, gamma: float, dt: float):
        """a, v of t + dt in place of a, v, from the displacements u_new (t + dt) and u (t)"""
        self._call("femcy_newmark_update", int(u_new_vec), int(u_vec), int(v_vec), int(a_vec), float(beta), float(gamma),
                   float(dt))

    # lumped mass and the explicit integrator (*Dynamic, explicit)
    def lumped_mass(self, ELE, rho: float) -> int:
        """HRZ-lumped nodal masses of the undeformed mesh at density rho, integrated with the plug-in's mass_rule()."""
        t = ELE.mass_tables()
        if t["Nq"].shape != (t["nq"], self.npe) or t["dNq"].shape != (t["nq"], self.npe, self.dm):
            raise FemcyError(f"mass-rule tables do not match the mesh (npe={self.npe}, dm={self.dm})")
        out = C.c_int32()
        self._call("femcy_lumped_mass_create", int(t["nq"]), _ptr(t["Nq"]), _ptr(t["dNq"]), _ptr(t["wq"]), float(rho),
                   C.byref(out))
        return out.value

    def lumped_mass_get(self, lm: int) -> np.ndarray:
        out = np.empty(self.nn, dtype=np.float64)
        self._call("femcy_lumped_mass_get", int(lm), _ptr(out))
        return out

    def lumped_mass_scale(self, lm: int, s_C: float = 0.0, factor=None, dt=None, type="below min") -> dict:
        """fixed mass scaling of the lumped mass lm, before an integrator is made from it: every element's shares times
        `factor`, and / or times what brings its estimated increment 2 / omega_e to `dt` under `type` ("below min": only the
        elements below dt, "set equal dt": every element, "uniform": one factor for all; or an MS_* constant).  s_C: the
        material stiffness of explicit_element_bound, read with dt.  -> {"mass0", "mass1", "scaled_elements", "max_factor"}"""
        m0, m1, fmax, k = C.c_double(), C.c_double(), C.c_double(), C.c_int64()
        kind = MS_TYPES.get(type.lower(), -1) if isinstance(type, str) else int(type)
        self._call("femcy_lumped_mass_scale", int(lm), float(s_C), float(factor or 0.0), float(dt or 0.0), kind,
                   C.byref(m0), C.byref(m1), C.byref(k), C.byref(fmax))
        return {"mass0": m0.value, "mass1": m1.value, "scaled_elements": int(k.value), "max_factor": fmax.value}

    def lumped_mass_scaling(self, lm: int) -> np.ndarray:
        """[ne] the cumulative mass-scaling factor of every element; 1.0 before any lumped_mass_scale"""
        out = np.empty(self.ne, dtype=np.float64)
        self._call("femcy_lumped_mass_get_scaling", int(lm), _ptr(out))
        return out

    def explicit(self, lm: int, dofsets=()) -> int:
        """an explicit integrator on the lumped mass lm; the DOFs of the given DOF sets are held (inverse mass 0)."""
        ids = np.ascontiguousarray(list(dofsets), dtype=np.int32)
        out = C.c_int32()
        self._call("femcy_explicit_create", int(lm), int(ids.size), _ptr(ids) if ids.size else None, C.byref(out))
        return out.value

    def explicit_start(self, ex: int, rhs_vec: int = VEC_RHS, scale: float = 1.0):
        """ACC = a_0 = minv (scale f - f_int(DOF))"""
        self._call("femcy_explicit_start", int(ex), int(rhs_vec), float(scale))

    def explicit_advance(self, ex: int, nsteps: int, dt: float, rhs_vec: int = VEC_RHS, scale0: float = 1.0,
                         dscale: float = 0.0):
        """nsteps velocity-Verlet steps on DOF, VEL, ACC; the k-th new state is loaded with (scale0 + k dscale) f"""
        self._call("femcy_explicit_advance", int(ex), int(rhs_vec), int(nsteps), float(dt), float(scale0), float(dscale))

    def explicit_kinetic_energy(self, ex: int, v_vec: int = VEC_VEL) -> float:
        out = C.c_double()
        self._call("femcy_explicit_kinetic_energy", int(ex), int(v_vec), C.byref(out))
        return out.value

    def explicit_stable_dt(self, ex: int):
        """-> (dt, omega_bound): Gershgorin's bound on M_L^-1 K of the last assemble_K, and 2 / that bound"""
        dt, om = C.c_double(), C.c_double()
        self._call("femcy_explicit_stable_dt", int(ex), C.byref(dt), C.byref(om))
        return dt.value, om.value

    def explicit_element_bound(self, ex: int, s_C: float, u_vec: int = VEC_DOF) -> float:
        """omega of the element-by-element estimate at vec[u_vec] (no matrix): the stable increment is 2 / omega"""
        om = C.c_double()
        self._call("femcy_explicit_element_bound", int(ex), int(u_vec), float(s_C), C.byref(om))
        return om.value

    def explicit_auto_begin(self, ex: int, s_C: float, scale_factor: float, T: float, ramp: bool = False,
                            rhs_vec: int = VEC_RHS):
        """t = 0 on the device, vec[ACC] = a_0 and the first increment of an element-by-element run up to T"""
        self._call("femcy_explicit_auto_begin", int(ex), int(rhs_vec), float(s_C), float(scale_factor), float(T), int(bool(ramp)))

    def explicit_auto_advance(self, ex: int, nsteps: int, rhs_vec: int = VEC_RHS):
        """nsteps steps with the increment re-estimated on the device in each; steps past T are no-ops; only enqueues"""
        self._call("femcy_explicit_auto_advance", int(ex), int(rhs_vec), int(nsteps))

    def explicit_set_damping(self, ex: int, alpha: float = 0.0, b1: float = 0.0, b2: float = 0.0, M_d: float = 0.0):
        """mass-proportional damping alpha and bulk viscosity (b1, b2, dilatational modulus M_d) of an integrator, from the
        next stepping call on; all zero restores the undamped launches and bits"""
        self._call("femcy_explicit_set_damping", int(ex), float(alpha), float(b1), float(b2), float(M_d))

    def amplitude(self, definition: str, t, A) -> int:
        """a curve A(t) in step time from 2 .. 16 points, t strictly increasing: "tabular" (piecewise linear) or
        "smooth step" (quintic between the points, A' = A'' = 0 at each); clamped outside the table"""
        kind = AMP_KINDS[str(definition).strip().lower()]
        t, A = np.ascontiguousarray(t, dtype=np.float64), np.ascontiguousarray(A, dtype=np.float64)
        if t.ndim != 1 or t.shape != A.shape:
            raise ValueError("amplitude: t and A must be one-dimensional and of the same length")
        out = C.c_int32()
        self._call("femcy_amplitude_create", kind, int(t.size), _ptr(t), _ptr(A), C.byref(out))
        return out.value

    def explicit_set_motion(self, ex: int, dofsets=(), values=(), amplitudes=()):
        """prescribed motion of an integrator, from its next explicit_start / explicit_auto_begin: the DOFs of held set
        dofsets[k] follow u = values[k] A_k(t), v = values[k] A_k', a = values[k] A_k'' with A_k = amplitudes[k]; a later set
        wins where two overlap.  No sets: the motion is removed and the integrator is launched as without it."""
        ids = np.ascontiguousarray(list(dofsets), dtype=np.int32)
        vals = np.ascontiguousarray(list(values), dtype=np.float64)
        amps = np.ascontiguousarray(list(amplitudes), dtype=np.int32)
        if not ids.size == vals.size == amps.size:
            raise ValueError("explicit_set_motion: one value and one amplitude per DOF set")
        some = ids.size > 0
        self._call("femcy_explicit_set_motion", int(ex), int(ids.size), _ptr(ids) if some else None,
                   _ptr(vals) if some else None, _ptr(amps) if some else None)

    def explicit_energy_enable(self, ex: int, on: bool = True):
        """the energy balance of an integrator: on from its next explicit_start / explicit_auto_begin, which zero the four
        work sums; the node pass of every step then adds to them on the device, with no launch added and the same u, v, a.
        off: the launches of an integrator that never had it"""
        self._call("femcy_explicit_energy_enable", int(ex), int(bool(on)))

    def explicit_energy(self, ex: int) -> np.ndarray:
        """-> [EN_LOAD, EN_INTERNAL, EN_ALPHA, EN_BOUNDARY]: the synchronising read-back of the work sums since the start"""
        out = np.zeros(4, dtype=np.float64)
        self._call("femcy_explicit_energy_get", int(ex), _ptr(out))
        return out

    def explicit_set_wall(self, ex: int, points=(), normals=(), kappas=()):
        """frictionless planar rigid walls of an integrator (*Rigid Wall), from its next explicit_start /
        explicit_auto_begin: wall k passes through points[k] with the normal normals[k] into the free half space (normalised
        by the library) and the penalty kappas[k] in 1/s^2; a node with the gap g < 0 takes the acceleration -kappa g n on
        its free DOFs.  At most WALL_MAX walls; none: the launches of an integrator that never had one"""
        pts = np.ascontiguousarray(points, dtype=np.float64).reshape(-1)
        nrm = np.ascontiguousarray(normals, dtype=np.float64).reshape(-1)
        kap = np.ascontiguousarray(kappas, dtype=np.float64).reshape(-1)
        if pts.size != kap.size * self.dm or nrm.size != kap.size * self.dm:
            raise ValueError("explicit_set_wall: one point and one normal of dm entries and one kappa per wall")
        some = kap.size > 0
        self._call("femcy_explicit_set_wall", int(ex), int(kap.size), _ptr(pts) if some else None,
                   _ptr(nrm) if some else None, _ptr(kap) if some else None)

    def explicit_wall_get(self, ex: int, wall: int = 0) -> np.ndarray:
        """-> [normal force, potential E_w, nodes with g < 0, largest penetration] of one wall at vec[DOF]: a synchronising
        read-back, reduced in a fixed order"""
        out = np.zeros(4, dtype=np.float64)
        self._call("femcy_explicit_wall_get", int(ex), int(wall), _ptr(out))
        return out

    def explicit_auto_state(self, ex: int):
        """-> (t, h_last, h_min, steps_done): the synchronising read-back of the device clock"""
        t, hl, hm, k = C.c_double(), C.c_double(), C.c_double(), C.c_int64()
        self._call("femcy_explicit_auto_state", int(ex), C.byref(t), C.byref(hl), C.byref(hm), C.byref(k))
        return t.value, hl.value, hm.value, int(k.value)

    def spmv(self, x_vec: int, y_vec: int):
        self._call("femcy_spmv", int(x_vec), int(y_vec))

    def pcg(self, b_vec: int, x_vec: int = VEC_X, eps: float = 1.0e-3, maxit: int = 0):
        it, r0, rm = C.c_int32(), C.c_double(), C.c_double()
        self._call("femcy_pcg", int(b_vec), int(x_vec), float(eps), int(maxit), C.byref(it), C.byref(r0), C.byref(rm))
        return it.value, r0.value, rm.value

    def direct_solve(self, b_vec: int, x_vec: int = VEC_X) -> dict:
        """vec[x] = K^-1 vec[b] by a band factorisation K = L S L^T (solve_by_scipy, stiffnessMtrx.py:219-251).
        -> what was factored and how good the solution is.  FemcyError with status FEMCY_ENUMERIC when K is singular or
        the residual stays large, FEMCY_ENOMEM when the band is too large."""
        info = DirectInfo()
        self._call("femcy_direct_solve", int(b_vec), int(x_vec), C.byref(info))
        return {k: getattr(info, k) for k, _ in DirectInfo._fields_ if k != "reserved"}

    def direct_plan(self) -> dict:
        """the band `direct_solve` would factor for the current pattern (n, bandwidth, panels, band_bytes), without
        factoring anything"""
        info = DirectInfo()
        self._call("femcy_direct_plan", C.byref(info))
        return {k: getattr(info, k) for k in ("n", "band_bytes", "bandwidth", "panels")}

    # -------------------------------------------------------------------------- post-processing
    def compute_strain_stress(self, u_vec: int = VEC_DOF, large: bool = False):
        self._call("femcy_compute_strain_stress", int(u_vec), int(bool(large)))

    def elastic_energy(self, u_vec: int = VEC_DOF, small: bool = False) -> float:
        """small: the energy of the infinitesimal strain on the undeformed mesh (u.Ku / 2 of a linear analysis) instead of
        the reference's energy of the Green strain"""
        out = C.c_double()
        self._call("femcy_elastic_energy_small" if small else "femcy_elastic_energy", int(u_vec), C.byref(out))
        return out.value

    def extrapolate(self, gp_field: int, E: np.ndarray, comp: int = 0) -> np.ndarray:
        """Gauss-point field (component `comp`) -> patch-wise nodal values [ne, npe]; E is npe x nGP."""
        E = _f64(E)
        if E.shape != (self.npe, self.nGP):
            raise FemcyError(f"extrapolation matrix must be {self.npe} x {self.nGP}, got {E.shape}")
        out = np.empty((self.ne, self.npe), dtype=np.float64)
        self._call("femcy_extrapolate", int(gp_field), int(comp), _ptr(E), _ptr(out))
        return out

    # ------------------------------------------------------------------------------ inspection
    def get_K_ell(self):
        info = self.pattern_info()
        W = info.ell_width
        ij = np.empty((self.n, W + 1), dtype=np.int32)
        A = np.empty((self.n, W), dtype=np.float64)
        self._call("femcy_get_K_ell", _ptr(ij), _ptr(A))
        return ij, A

    def get_K_bsr(self):
        """scipy.sparse.bsr_matrix of the device matrix (ascending block columns)."""
        import scipy.sparse as sp
        info = self.pattern_info()
        rowptr = np.empty(self.nn + 1, dtype=np.int32)
        col = np.empty(info.nnzb, dtype=np.int32)
        vals = np.empty((info.nnzb, self.dm, self.dm), dtype=np.float64)
        self._call("femcy_get_K_bsr", _ptr(rowptr), _ptr(col), _ptr(vals))
        return sp.bsr_matrix((vals, col, rowptr), shape=(self.n, self.n))

    def gauss_field(self, which: int) -> GaussField:
        mat = (self.dm, self.dm)
        tail = {GP_DSDX: (self.npe, self.dm), GP_VOL: (), GP_F: mat, GP_SIGMA: mat, GP_STRAIN: mat, GP_MISES: (),
                GP_ENERGY: ()}[which]
        return GaussField(self, which, tail)

    def probe_stream(self, nbytes: int, reps: int = 20, mode: int = 0):
        """(GB/s, bytes per pass) of a read-only sweep in the persistent PCG's launch shape (femcy.h)"""
        us, moved = C.c_double(), C.c_int64()
        self._call("femcy_probe_stream", int(nbytes), int(reps), int(mode), C.byref(us), C.byref(moved))
        return moved.value / (us.value * 1e-6) / 1e9, moved.value

    def probe_exchange(self, rounds: int = 2000, form: int = 0) -> float:
        """microseconds per grid-wide exchange of one value per workgroup (femcy.h)"""
        us = C.c_double()
        self._call("femcy_probe_exchange", int(rounds), int(form), C.byref(us))
        return us.value

    def probe_spmv(self, reps: int = 100, storage_order: bool = True) -> float:
        """microseconds from launch to launch of `reps` back-to-back products (one HIP event pair around the batch)"""
        us = C.c_double()
        self._call("femcy_probe_spmv", int(reps), 1 if storage_order else 0, C.byref(us))
        return float(us.value)

    def probe_mailbox(self, rounds: int = 2000) -> float:
        """collective: microseconds per cross-rank mailbox reduction between the ranks' kernels"""
        us = C.c_double()
        self._call("femcy_probe_mailbox", int(rounds), C.byref(us))
        return float(us.value)

    def persist_streamed_bytes(self) -> int:
        out = C.c_int64()
        self._call("femcy_persist_streamed_bytes", C.byref(out))
        return out.value

    def timing(self) -> dict:
        t = Timing()
        self._call("femcy_timing", C.byref(t))
        return t.as_dict()

    def timing_reset(self):
        self._call("femcy_timing_reset")

    # ------------------------------------------------------------------------------- multi-GPU
    @staticmethod
    def comm_unique_id() -> bytes:
        lib = load_library()
        buf = C.create_string_buffer(128)
        rc = lib.femcy_comm_unique_id(buf)
        if rc != 0:
            raise FemcyError(f"femcy_comm_unique_id -> {rc}: {lib.femcy_last_error().decode()}")
        return buf.raw

    @staticmethod
    def comm_local_id() -> bytes:
        """id of an in-process group: contexts driven by one thread each in this process (single-GPU verification
        of the multi-rank path)."""
        lib = load_library()
        buf = C.create_string_buffer(128)
        rc = lib.femcy_comm_local_id(buf)
        if rc != 0:
            raise FemcyError(f"femcy_comm_local_id -> {rc}: {lib.femcy_last_error().decode()}")
        return buf.raw

    @staticmethod
    def comm_shm_id(max_values: int = 1 << 20) -> bytes:
        """id of a shared-memory group: the ranks are processes of one host (any devices, also all on one GPU);
        max_values = the longest vector of one collective, in doubles."""
        lib = load_library()
        buf = C.create_string_buffer(128)
        rc = lib.femcy_comm_shm_id(buf, int(max_values))
        if rc != 0:
            raise FemcyError(f"femcy_comm_shm_id -> {rc}: {lib.femcy_last_error().decode()}")
        return buf.raw

    def comm_allgather_host(self, payload: bytes) -> list:
        """collective: every rank's `payload` (same length on all ranks) in rank order, through the context's own
        transport"""
        n = len(payload)
        nranks = C.c_int32()
        self._call("femcy_comm_info", None, C.byref(nranks), None)
        send = C.create_string_buffer(payload, n)
        recv = C.create_string_buffer(n * nranks.value)
        self._call("femcy_comm_allgather_host", send, n, recv)
        return [recv.raw[i * n:(i + 1) * n] for i in range(nranks.value)]

    def comm_mailbox_connect(self) -> bool:
        """export -> all-gather over the context's transport -> import -> agree: True when every rank keeps the
        one-launch PCG"""
        self.comm_mailbox_import(self.comm_allgather_host(self.comm_mailbox_export()))
        return self.comm_persist_agree()

    def comm_init(self, rank: int, nranks: int, uid: bytes, iface_local_dofs, iface_global_slot, niface_global: int,
                  owner):
        d, s = _i32(iface_local_dofs).ravel(), _i32(iface_global_slot).ravel()
        ow = np.ascontiguousarray(owner, dtype=np.uint8).ravel()
        if ow.size != self.n:
            raise FemcyError("owner mask must have one entry per local DOF")
        idbuf = C.create_string_buffer(uid, 128)
        self._call("femcy_comm_init", int(rank), int(nranks), idbuf, d.size, _ptr(d), _ptr(s), int(niface_global),
                   _ptr(ow))
        ng = C.c_int64()
        self._call("femcy_comm_info", None, None, C.byref(ng))
        self.n_global = int(ng.value)

    def comm_info(self):
        """(rank, ranks of the communicator, DOF count of the whole system); (0, 1, n) without a communicator"""
        r, k, ng = C.c_int32(), C.c_int32(), C.c_int64()
        self._call("femcy_comm_info", C.byref(r), C.byref(k), C.byref(ng))
        return int(r.value), int(k.value), int(ng.value)

    def comm_set_neighbours(self, part):
        """part: a `femcy_amd.partition.Part` (nb_ranks / nb_ptr / nb_dofs)."""
        r, q, d = _i32(part.nb_ranks).ravel(), _i32(part.nb_ptr).ravel(), _i32(part.nb_dofs).ravel()
        self._call("femcy_comm_set_neighbours", r.size, _ptr(r), _ptr(q), _ptr(d))

    def comm_tune(self, iters: int = 20) -> dict:
        """collective: measure both interface exchanges, keep the faster one on every rank."""
        chosen, us = C.c_int32(), (C.c_double * 2)()
        self._call("femcy_comm_tune", int(iters), C.byref(chosen), C.cast(us, C.c_void_p))
        return {"exchange": "neighbour" if chosen.value == 1 else "allreduce", "allreduce_us": us[0], "neighbour_us": us[1]}

    # persistent PCG across ranks: the peers' kernels write into each other's mailboxes (femcy.h)
    def comm_mailbox_export(self) -> bytes:
        buf = C.create_string_buffer(256)
        self._call("femcy_comm_mailbox_export", buf)
        return buf.raw

    def comm_mailbox_import(self, blobs) -> None:
        """blobs: the 256-byte exports of ALL ranks, in rank order"""
        joined = b"".join(blobs)
        assert len(joined) == 256 * len(blobs)
        buf = C.create_string_buffer(joined, len(joined))
        self._call("femcy_comm_mailbox_import", len(blobs), buf)

    def comm_persist_agree(self) -> bool:
        """collective: True when every rank can keep the one-launch PCG (femcy_comm_persist_agree)"""
        out = C.c_int32()
        self._call("femcy_comm_persist_agree", C.byref(out))
        return bool(out.value)

    def iface_sum(self, vec_id: int):
        self._call("femcy_iface_sum", int(vec_id))
