#!/usr/bin/env python
"""bench.py -- BASELINE.json's headline metric on MI355X:
    "CG iters/sec + element-stiffness assemblies/sec, 1M C3D4 elems, 1/2/4/8 GPU".

One *step* = one pass of the hot path over the synthetic twist plate at state S1 (prescribed twist
of t = 0.05 on the z=0 face), exactly what one residual evaluation + linear solve of
the reference's Newton loop does on the device:
    femcy_assemble_K            get_dsdx_and_vol + assemble_stiffnessMtrx   (995 328 C3D4 per GPU)
    femcy_apply_dirichlet_newton  0/1 treatment of K, residual rows zeroed
    femcy_pcg(eps=0, maxit=ITERS) ITERS Jacobi-PCG iterations, reference recurrence + stopping test
All inputs are resident in HBM when the timed region starts.  N GPUs: the plate is cut into N z-slabs
of 995 328 elements each (weak scaling; N=1 is BASELINE's 1M mesh k=12, N=8 is its 8M mesh k=24) with
the interface exchange + two scalar reductions per CG iteration over RCCL; every rank generates only its
own slab (femcy_amd.partition.plate_slab_part), never the global mesh.

`python bench.py --gpus N` with N > 1 and no launcher environment starts its own N ranks (it re-executes itself
under `python -m torch.distributed.run --nnodes=1 --nproc-per-node N --master-addr 127.0.0.1`); launched BY
torch.distributed.run (WORLD_SIZE set) it is one rank of the job.  Rank 0 prints the one JSON line either way.

`--workload c3d10` runs the same step on BASELINE configs[4] (C3D10 plate 48x6x72: 124 416 quadratic tets on
the same 182 845 nodes) -- single GPU only; the default `c3d4` is the configuration the metric is quoted on.

`value` = CG iterations of all steps / wall time of the whole timed region (assembly included), times
global_elements/elements-per-GPU (= N) so that it is a whole-job aggregate; `cg_iters_per_s` (PCG only) and
`assemblies_per_s` (elements/s, geometry + assembly kernels) come from HIP events on the ctx stream.

A plain run (no --full) does only what the headline needs: set-up, pre-warm, W warm-up steps, K timed steps, the
outputs of the last timed step if --dump-outputs is given, one JSON line.  Besides the contract's keys that line holds
the figures the HIP events of the timed steps themselves give (cg_iters_per_s, assemblies_per_s, pcg_us_per_iter, ...).

--full adds everything that takes runs of its own:
  roofline     the dominant kernel of the timed region against the ceiling that binds it.  On the headline workload
               that kernel is k_pcg_persist, whose matrix stream comes from the Infinity Cache: `achieved` = the bytes
               its layout makes it move per launch / launch time, `peak` = what a read-only sweep of the same footprint
               reaches in the kernel's own launch shape on this GPU (femcy_probe_stream), `frac` <= 1; a time model
               (stream + 3 grid-wide exchanges, both probed) says how much of an iteration is accounted for; the
               ALGORITHMIC bytes / s of SURVEY.md 8d (which exceed the HBM peak because 47 % of the matrix and all
               vectors never leave the chip) are kept in separately named fields.
  hbm_bound    (N = 1, default workload) the same invocation then runs the two HBM-bound configurations --
               BASELINE configs[3]'s 7 962 624-element plate on this one GPU and configs[4]'s C3D10 plate -- and
               reports SpMV and PCG-iteration rates against 8 TB/s and against the copy probe of this GPU.
  direct_branch (N = 1, default workload) the reference's OTHER solver branch -- `solve_dof` below 1e5 DOF, scipy spsolve
               there, femcy_direct_solve here (band factorisation on the device) -- on three deck-sized systems: ms per
               solve beside the tight PCG (eps 1e-12) that served the branch before round 4.
  cpu_baseline the as-written C/OpenMP port of the reference on the host, in a child process pinned one thread per
               physical core (OMP_PLACES=cores, OMP_PROC_BIND=spread; arrays first-touched by the threads that use them).
  N > 1        the strong-scaling record, both multi-rank PCG paths timed, the mailbox round trip.

Order of a --full run (so that an external GPU-utilisation sampler sees one contiguous busy stretch at the end):
mesh -> CPU baseline leg (rank 0, N = 1) -> device set-up -> pre-warm (`--prewarm` seconds of untimed steps) ->
W warm-up steps -> K timed steps -> ceiling probes -> HBM-bound records -> one JSON line.

--dump-outputs DIR writes what the last timed step handed its caller as float64 .npy files (see dump_outputs); the
inputs depend on the arguments only, so two builds can be compared output for output.

  python bench.py [--gpus N] [--steps K] [--warmup W] [--iters ITERS] [--workload c3d4|c3d10|cpe8] [--full]
                  [--no-cpu-baseline] [--dump-outputs DIR]
"""
import argparse
import hashlib
import json
import os
import signal
import socket
import subprocess
import sys
import threading
import time

import numpy as np

ROOT = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, ROOT)

HBM_PEAK_GBS = 8000.0           # MI355X HBM3E spec (MI355X_MICROARCH.md, HBM section); the D2D probe below reports what
                                # a plain device copy reaches on the box the bench runs on
ELEMS_PER_GPU = {"c3d4": 995328, "c3d10": 124416, "cpe8": 163840}
CPE8_CELLS = (1280, 128)        # 163 840 CPE8 elements, 494 337 nodes, 988 674 DOF (~1 M DOF: the size of the 3-D headline system)
CPE8_NAME = ("beam CPE8 1280x128 serendipity quadrilaterals, plane strain, nlgeom (BASELINE configs[1] stand-in, "
             "163 840 elements, 988 674 DOF)")
TRAFFIC_KERNELS = ("k_pcg_persist", "k_spmv")     # kernels whose machine code the committed PMC traffic belongs to


def log(*a):
    print(*a, file=sys.stderr, flush=True)


def kernel_object_sha(lib_path=None, patterns=TRAFFIC_KERNELS):
    """fingerprint of the MACHINE CODE of the dominant kernels (every instantiation of the persistent PCG and of the
    product) inside libfemcy_hip.so: profiles/spmv_traffic.json is valid for the kernels it was measured on.  Round 5
    hashed whole source files (ctx.hpp and pattern.cpp among them), and an edit for an unrelated assembly option voided the
    record of the driver's line; the code object changes when, and only when, a kernel does.  (What the host decides --
    the matrix layout -- is pinned separately, by the pattern sizes stored with each workload.)
    Parses the clang offload bundles of the shared object (one per translation unit) and the gfx950 ELF inside each."""
    import struct
    if lib_path is None:
        lib_path = os.path.join(ROOT, "femcy_amd", "libfemcy_hip.so")
    data = open(lib_path, "rb").read()
    magic = b"__CLANG_OFFLOAD_BUNDLE__"
    found = {}
    pos = data.find(magic)
    while pos >= 0:
        n = struct.unpack_from("<Q", data, pos + len(magic))[0]
        q = pos + len(magic) + 8
        for _ in range(n):
            off, size, tlen = struct.unpack_from("<QQQ", data, q)
            triple = data[q + 24:q + 24 + tlen]
            q += 24 + tlen
            if b"gfx950" not in triple or size < 64:
                continue
            elf = data[pos + off:pos + off + size]
            if elf[:4] != b"\x7fELF":
                continue
            shoff, = struct.unpack_from("<Q", elf, 0x28)
            shentsize, shnum = struct.unpack_from("<HH", elf, 0x3A)
            secs = [struct.unpack_from("<IIQQQQIIQQ", elf, shoff + i * shentsize) for i in range(shnum)]
            for sh in secs:
                if sh[1] != 2:                                   # SHT_SYMTAB
                    continue
                strtab = secs[sh[6]]
                for k in range(sh[5] // 24):
                    name_off, info, _, shndx, value, ssize = struct.unpack_from("<IBBHQQ", elf, sh[4] + 24 * k)
                    if (info & 0xF) != 2 or ssize == 0 or shndx == 0 or shndx >= shnum:      # STT_FUNC, defined
                        continue
                    end = elf.index(b"\0", strtab[4] + name_off)
                    name = elf[strtab[4] + name_off:end].decode()
                    if not any(pt in name for pt in patterns):
                        continue
                    sec = secs[shndx]
                    code = elf[value - sec[3] + sec[4]:value - sec[3] + sec[4] + ssize]
                    found[name] = hashlib.sha256(code).hexdigest()
        pos = data.find(magic, pos + 1)
    if not found:
        raise RuntimeError(f"no {patterns} kernels found in the gfx950 code objects of {lib_path}")
    h = hashlib.sha256()
    for name in sorted(found):
        h.update(name.encode() + b"=" + found[name].encode() + b";")
    return h.hexdigest()[:16]


def kernel_symbol_fragment(demangled):
    """'void femcy::(anonymous namespace)::k_pcg_persist<3, 3, 4, 6, false>(...)' -> '13k_pcg_persistILi3ELi3ELi4ELi6ELb0EE':
    the piece of the Itanium-mangled symbol that names ONE instantiation (integer and bool template arguments)"""
    import re
    m = re.search(r"(k_\w+)<([^>]*)>", demangled)
    if not m:
        m2 = re.search(r"(k_\w+)", demangled)
        return f"{len(m2.group(1))}{m2.group(1)}" if m2 else None
    args = ""
    for a in (x.strip() for x in m.group(2).split(",")):
        if a in ("true", "false"):
            args += "Lb%dE" % (a == "true")
        elif re.fullmatch(r"-?\d+", a):
            args += "Li%sE" % a.replace("-", "n")
        else:
            return None
    return f"{len(m.group(1))}{m.group(1)}I{args}E"


def pmc_traffic(workload, kernel, layout=None):
    """HBM-side bytes per launch of the dominant kernel from the committed rocprofv3 PMC passes (FETCH_SIZE x2 +
    WRITE_SIZE, separate passes, MI355X_MICROARCH.md HBM section) -- refused (None + reason) when the machine code of
    the kernel INSTANTIATION the passes were taken on changed since (`kernel_sha` of the workload; records without one:
    the fingerprint over all PCG / SpMV kernels), when the matrix layout of the workload (pattern sizes) is not the one
    the passes saw, or when the passes were taken on a different kernel."""
    tpath = os.path.join(ROOT, "profiles", "spmv_traffic.json")
    if not os.path.exists(tpath):
        return None, "no profiles/spmv_traffic.json"
    try:
        doc = json.load(open(tpath))
        entry = doc.get("workloads", {}).get(workload)
        if entry is None:
            return None, f"no PMC pass recorded for workload {workload}"
        if kernel not in entry.get("kernel", ""):
            return None, f"PMC passes of workload {workload} were taken on {entry.get('kernel', '?')[:60]}, not on {kernel}"
        frag = kernel_symbol_fragment(entry.get("kernel", "")) if entry.get("kernel_sha") else None
        if frag:
            sha = kernel_object_sha(patterns=(frag,))
            if entry["kernel_sha"] != sha:
                return None, f"stale: PMC passes were taken on {frag} with code {entry['kernel_sha']}, the library holds {sha}"
        else:
            sha = kernel_object_sha()
            if doc.get("kernel_object_sha") != sha:
                return None, (f"stale: PMC passes were taken on kernel code {doc.get('kernel_object_sha')}, "
                              f"the library holds {sha}")
        if layout is not None and entry.get("layout") is not None and entry["layout"] != layout:
            return None, f"stale: PMC passes saw the layout {entry['layout']}, this run has {layout}"
        return entry["hbm_bytes_per_launch"], f"profiles/spmv_traffic.json @ {doc.get('git_head', '?')}"
    except Exception as e:                                      # noqa: BLE001
        return None, f"unreadable profiles/spmv_traffic.json: {e!r}"


def layout_signature(info):
    """what the host decides about the matrix the kernels stream (femcy_get_pattern_info)"""
    return {k: int(getattr(info, k)) for k in ("n", "nnzb", "stored_blocks", "nslices") if hasattr(info, k)}


DUMP_VEC_ENTRIES = 2_000_000        # --dump-outputs: entries per vector over all ranks (16 MB of float64)
DUMP_K_BLOCK_ROWS = 2048            # block rows of K over all ranks (a few MB of blocks)


def dump_outputs(ctx, be, out_dir, pcg_result, rank, nranks):
    """--dump-outputs: what the last timed step handed its caller, float64 .npy files in `out_dir`:
        x            the PCG solution (VEC_X)
        residual     the right-hand side it solved for (VEC_RESIDUAL, Dirichlet rows zeroed)
        pcg          (iterations, r0, rmax) as femcy_pcg returned them
        K_blocks     the dm x dm blocks of the assembled K after the Dirichlet treatment, for a seeded sample of block
        K_block_index  rows (all of them on small meshes), ascending block columns; their (block row, block column)
    Vectors longer than their share of DUMP_VEC_ENTRIES are sampled at seeded positions that depend on the length only,
    so that the files stay below 64 MB for every size and rank count.  N > 1: each rank writes its slab as
    `<name>.rank<r>.npy`."""
    os.makedirs(out_dir, exist_ok=True)
    suffix = f".rank{rank}" if nranks > 1 else ""

    def save(name, arr):
        np.save(os.path.join(out_dir, f"{name}{suffix}.npy"), np.ascontiguousarray(arr, dtype=np.float64))

    def sample(count, cap):
        if count <= cap:
            return np.arange(count)
        return np.sort(np.random.default_rng(0).choice(count, cap, replace=False))

    idx = sample(ctx.n, DUMP_VEC_ENTRIES // nranks)
    save("x", ctx.download(be.VEC_X)[idx])
    save("residual", ctx.download(be.VEC_RESIDUAL)[idx])
    save("pcg", np.array(pcg_result, dtype=np.float64))
    K = ctx.get_K_bsr()
    rows = sample(K.indptr.size - 1, max(1, DUMP_K_BLOCK_ROWS // nranks))
    pos = np.concatenate([np.arange(K.indptr[r], K.indptr[r + 1]) for r in rows])
    save("K_blocks", K.data[pos])
    save("K_block_index", np.stack([np.repeat(rows, np.diff(K.indptr)[rows]), K.indices[pos]], axis=1))


def hbm_copy_probe(torch):
    """device-to-device copy of 1 GiB (read + write = 2 GiB of traffic), best of 5: the bandwidth a plain copy reaches
    on this box, printed next to the 8 TB/s spec the roofline fraction is quoted against"""
    try:
        nbytes = 1 << 30
        a = torch.empty(nbytes, dtype=torch.uint8, device="cuda")
        b = torch.empty_like(a)
        a.zero_()
        b.copy_(a)
        torch.cuda.synchronize()
        best = 0.0
        for _ in range(5):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            b.copy_(a)
            e1.record()
            torch.cuda.synchronize()
            best = max(best, 2 * nbytes / (e0.elapsed_time(e1) * 1e-3) / 1e9)
        del a, b
        return best
    except Exception as e:                                      # noqa: BLE001
        log(f"[bench] HBM copy probe failed: {e!r}")
        return None


class Watchdog:
    """hard time-out around a phase that can hang on a broken node (RCCL communicator set-up, the exchange tuning):
    the rank exits with code 3, torch.distributed.run then tears the job down, the self-launcher returns non-zero"""

    def __init__(self, seconds, what):
        self.seconds, self.what, self.timer = seconds, what, None

    def __enter__(self):
        def fire():
            log(f"[bench] rank {os.environ.get('RANK', '0')}: '{self.what}' did not finish within {self.seconds} s -- giving up")
            os._exit(3)
        if self.seconds > 0:
            self.timer = threading.Timer(self.seconds, fire)
            self.timer.daemon = True
            self.timer.start()
        return self

    def __exit__(self, *exc):
        if self.timer:
            self.timer.cancel()
        return False


def self_launch(n, argv, timeout):
    """`python bench.py --gpus N` typed without a launcher: start N ranks of this script under torch.distributed.run
    (one rank per GPU, rendezvous on 127.0.0.1 at a free port), pass rank 0's JSON line through, return the job's
    exit code (non-zero if any rank failed or the job exceeded `timeout` seconds)."""
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    port = s.getsockname()[1]
    s.close()
    cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", f"--nproc-per-node={n}",
           "--master-addr", "127.0.0.1", "--master-port", str(port), os.path.abspath(__file__)] + argv
    log(f"[bench] --gpus {n} without a launcher environment: starting {n} ranks: {' '.join(cmd[1:9])} ...")
    env = dict(os.environ)
    env.setdefault("HSA_ENABLE_IPC_MODE_LEGACY", "0")           # dmabuf IPC (RCCL across processes on this driver)
    env["FEMCY_BENCH_SELF_LAUNCHED"] = "1"
    proc = subprocess.Popen(cmd, stdout=subprocess.PIPE, text=True, env=env, start_new_session=True)
    try:
        out, _ = proc.communicate(timeout=timeout)
    except subprocess.TimeoutExpired:
        log(f"[bench] the {n}-rank job did not finish within {timeout} s: killing it")
        try:
            os.killpg(proc.pid, signal.SIGKILL)                 # exactly the process group started above
        except ProcessLookupError:
            pass
        proc.wait()
        return 4
    lines = [l for l in out.splitlines() if l.strip().startswith("{")]
    if proc.returncode == 0 and len(lines) != 1:
        log(f"[bench] expected one JSON line from rank 0, got {len(lines)}")
        return 5
    for l in lines:
        sys.stdout.write(l + "\n")
    sys.stdout.flush()
    return proc.returncode


def s1_state(nodes, bcs, user_dirichletBC_values, t1=0.05, load_ratio=None):
    """state S1: the prescribed values of the first increment (end time t1: user blocks are evaluated at
    t1, plain blocks hold val * load_ratio, stiffnessMtrx.py:679-690) written into dof, zero elsewhere, and the sorted
    list of constrained DOFs"""
    dm = nodes.shape[1]
    u = np.zeros(nodes.size)
    cons = []
    for bc in bcs:
        ids = np.asarray(bc["node_set"], dtype=np.int64)
        cons.append(ids * dm + bc["dof"])
        if bc["user"] and ids.size:
            user_dirichletBC_values(u, ids, dm, bc["dof"], nodes, t1)
        elif ids.size and bc["val"] != 0.0:
            u[ids * dm + bc["dof"]] = bc["val"] * (t1 if load_ratio is None else load_ratio)
    return u, np.unique(np.concatenate(cons)).astype(np.int32)


def algorithmic_bytes(info, nn, n):
    """SURVEY.md 8d, padding never counted: one SpMV = 8 nnz + 4 nnz/dm^2 + 4 (nn + 1) + 16 n; one PCG iteration = the
    SpMV + 88 n (the fused vector updates of the reference recurrence)"""
    spmv = 8 * info.nnz + 4 * info.nnzb + 4 * (nn + 1) + 16 * n
    return spmv, spmv + 88 * n


def read_stream_probe(ctx, be, footprint):
    """GB/s of a read-only sweep of `footprint` bytes (capped at 1 GiB) with eight workgroups per CU and 16-byte loads,
    best of the default / non-temporal policy (femcy_probe_stream modes 2, 3): what a read-mostly kernel such as the
    SpMV can reach on THIS GPU from HBM -- the demonstrated ceiling next to the 8 TB/s of the spec"""
    if not hasattr(ctx, "probe_stream"):
        return None
    try:
        nbytes = int(max(1 << 20, min(int(footprint), 1 << 30)))
        return max(ctx.probe_stream(nbytes, 8, mode)[0] for mode in (2, 3) for _ in range(2))
    except be.FemcyError as e:
        log(f"[bench] read-stream probe failed: {e}")
        return None


def hbm_bound_record(be, name, mesh, element, material, user_values, probe, iters=100, spmv_reps=40):
    """one HBM-bound configuration on this GPU: SpMV (dispatch-attached HIP events on every launch) and the PCG
    iteration (whole solves of `iters` iterations, every 16th SpMV sampled) with their algorithmic-byte rates"""
    t0 = time.time()
    ctx = be.Context(int(os.environ.get("LOCAL_RANK", "0")))
    try:
        nodes, el = mesh["nodes"], mesh["elements"]
        ctx.set_mesh(nodes, el)
        ctx.set_element(element)
        ctx.set_material(material)
        info = ctx.build_pattern()
        ti = mesh.get("time_incs", {})
        u, cons = s1_state(nodes, mesh["dirichlet_bc_info"], user_values, t1=ti.get("ini_inc", 0.05),
                           load_ratio=ti.get("ini_inc", 0.05) / ti.get("max_time", 1.0))
        block_bytes = ctx.dm * ctx.dm * 8 + 4
        ctx.upload(be.VEC_DOF, u)
        ctx.vector(be.VEC_RHS).fill(0.0)
        ctx.internal_force(be.VEC_DOF, be.VEC_FORCE)
        ctx.vec_sub(be.VEC_RESIDUAL, be.VEC_FORCE, be.VEC_RHS)
        cs = ctx.dofset(cons)
        ctx.assemble_K(be.VEC_DOF)
        ctx.dofset_dirichlet_newton(cs, be.VEC_RESIDUAL)
        ctx.pcg(be.VEC_RESIDUAL, be.VEC_X, eps=0.0, maxit=iters)          # warm: clocks, caches, lazy allocations
        spmv_b, iter_b = algorithmic_bytes(info, ctx.nn, ctx.n)
        # (a) the product through the public entry point femcy_spmv (vectors in the caller's node order)
        # (round 5: timed as whole calls between two synchronisations -- what a caller of the public entry point sees,
        # launch overhead included -- instead of HIP events around the kernel alone)
        for _ in range(3):
            ctx.spmv(be.VEC_RESIDUAL, be.VEC_TMP0)
        ctx.sync()
        t_api = time.perf_counter()
        for _ in range(spmv_reps):
            ctx.spmv(be.VEC_RESIDUAL, be.VEC_TMP0)
        ctx.sync()
        api_us = (time.perf_counter() - t_api) / spmv_reps * 1e6
        api_n = spmv_reps
        # (b) the product as the three-launch PCG runs it (round 4: vectors in storage order) -- dispatch-attached events
        # on every 4th launch inside whole solves.  (Round 5: a system that fits the persistent kernel's vector layout
        # takes ONE launch per solve whatever the size of its matrix -- the C3D10 plate -- so the product kernel is
        # timed with that path switched off, and the iteration is reported for BOTH paths below.)
        ctx.set_option(be.OPT_PCG_PERSIST, 0)
        ctx.set_option(be.OPT_TIMING, 4)
        ctx.timing_reset()
        its = 0
        for _ in range(3):
            ctx.assemble_K(be.VEC_DOF)
            ctx.dofset_dirichlet_newton(cs, be.VEC_RESIDUAL)
            its += ctx.pcg(be.VEC_RESIDUAL, be.VEC_X, eps=0.0, maxit=iters)[0]
        tm = ctx.timing()
        ctx.set_option(be.OPT_TIMING, 0)
        sampled_us = tm["spmv_ms"] * 1e3 / max(tm["spmv_launches"], 1) if tm["spmv_launches"] else api_us
        # (c) the same kernel, 200 launches back to back between ONE pair of HIP events (femcy_probe_spmv): launch-to-launch
        # time = kernel + the ~1.5 us boundary.  Dispatch-attached events on single launches inside a solve read ~5 us
        # high (the profiled packet drains the pipeline; 71.1 against 65.8 us in rocprofv3's kernel trace of the same
        # run, profiles/r04_kernel_stats_bench_c3d10.txt), so THIS is the figure reported as `spmv`
        spmv_us, spmv_n = sampled_us, int(tm["spmv_launches"]) or api_n
        how = "dispatch-attached HIP events on every 4th product launch inside the PCG solves"
        if hasattr(ctx, "probe_spmv"):
            try:
                spmv_us, spmv_n = min(ctx.probe_spmv(200, True) for _ in range(3)), 200
                how = "200 launches back to back between one pair of HIP events, best of 3 (kernel + launch boundary)"
            except be.FemcyError as e:
                log(f"[bench] femcy_probe_spmv failed: {e}")
        # the sampled dispatches cost a pipeline drain each (~5 us on every 4th iteration): the iteration time comes from
        # a second set of solves with sparse sampling
        ctx.set_option(be.OPT_TIMING, 64)
        ctx.timing_reset()
        its = 0
        for _ in range(3):
            its += ctx.pcg(be.VEC_RESIDUAL, be.VEC_X, eps=0.0, maxit=iters)[0]
        tm2 = ctx.timing()
        ctx.set_option(be.OPT_TIMING, 0)
        three_us = iter_us = tm2["pcg_ms"] * 1e3 / max(its, 1)
        asm_ms = (tm["geom_ms"] + tm["assemble_ms"]) / max(tm["assemble_launches"], 1)
        # the library's default path for this system: one persistent launch per solve where the vector layout fits
        ctx.set_option(be.OPT_PCG_PERSIST, 1)
        path, streamed = "three-kernel", None
        ctx.pcg(be.VEC_RESIDUAL, be.VEC_X, eps=0.0, maxit=iters)
        ctx.set_option(be.OPT_TIMING, 64)
        ctx.timing_reset()
        its = 0
        for _ in range(3):
            its += ctx.pcg(be.VEC_RESIDUAL, be.VEC_X, eps=0.0, maxit=iters)[0]
        tm3 = ctx.timing()
        ctx.set_option(be.OPT_TIMING, 0)
        if tm3["solves_persist"] > 0 and tm3["solves_three"] == 0:
            path = "persistent"
            iter_us = tm3["pcg_ms"] * 1e3 / max(its, 1)
            streamed = int(ctx.persist_streamed_bytes()) if hasattr(ctx, "persist_streamed_bytes") else None
        spmv_gbs = spmv_b / (spmv_us * 1e-6) / 1e9
        iter_gbs = iter_b / (iter_us * 1e-6) / 1e9
        rprobe = read_stream_probe(ctx, be, info.stored_blocks * block_bytes)
        rec = {"workload": name, "elements": int(ctx.ne), "dof": int(ctx.n), "stored_matrix_mb": info.stored_blocks * block_bytes / 1e6,
               "pcg_path": path,
               "spmv": {"kernel": f"k_spmv<{ctx.dm}> inside the PCG solves (vectors in storage order)", "bound": "hbm",
                        "avg_launch_us": spmv_us, "launches_timed": spmv_n, "bytes_per_launch": int(spmv_b), "achieved": spmv_gbs,
                        "timed_as": how, "sampled_inside_pcg_us": sampled_us,
                        "through_femcy_spmv_us": api_us, "through_femcy_spmv_frac": spmv_b / (api_us * 1e-6) / 1e9 / HBM_PEAK_GBS,
                        "peak": HBM_PEAK_GBS, "unit": "GB/s", "frac": spmv_gbs / HBM_PEAK_GBS,
                        "frac_of_copy_probe": (spmv_gbs / probe) if probe else None,
                        "read_stream_probe_gbs": rprobe, "frac_of_read_stream_probe": (spmv_gbs / rprobe) if rprobe else None},
               "pcg_iteration": {"us": iter_us, "iterations_timed": int(its), "bytes": int(iter_b), "achieved": iter_gbs,
                                 "peak": HBM_PEAK_GBS, "unit": "GB/s", "frac": iter_gbs / HBM_PEAK_GBS,
                                 "frac_of_copy_probe": (iter_gbs / probe) if probe else None,
                                 "path": path, "three_launch_us": three_us,
                                 "three_launch_frac": iter_b / (three_us * 1e-6) / 1e9 / HBM_PEAK_GBS,
                                 # persistent: the bytes its layout streams per iteration (the register / LDS-resident
                                 # block rows and the vectors never move); `frac` above prices SURVEY 8d's bytes
                                 "persistent_streamed_bytes": streamed,
                                 "persistent_streamed_gbs": ((streamed + 16 * ctx.n) / (iter_us * 1e-6) / 1e9) if streamed else None},
               "assembly_ms": asm_ms, "assemblies_per_s": ctx.ne / (asm_ms * 1e-3) if asm_ms > 0 else 0.0,
               "wall_s": time.time() - t0}
        return rec
    finally:
        ctx.close()


def direct_branch_record(be, label, mesh, element, material, user_values, reps=5):
    """one system of the size the reference's decks have, solved the way `solve_dof` solves it below 1e5 DOF: the
    direct solve (factorisation redone on every call, as in a Newton iteration) and the tight PCG, ms per solve"""
    ctx = be.Context(int(os.environ.get("LOCAL_RANK", "0")))
    try:
        nodes, el = mesh["nodes"], mesh["elements"]
        ctx.set_mesh(nodes, el)
        ctx.set_element(element)
        ctx.set_material(material)
        ctx.build_pattern()
        u, cons = s1_state(nodes, mesh["dirichlet_bc_info"], user_values)
        ctx.upload(be.VEC_DOF, u)
        ctx.vector(be.VEC_RHS).fill(0.0)
        ctx.internal_force(be.VEC_DOF, be.VEC_FORCE)
        ctx.vec_sub(be.VEC_RESIDUAL, be.VEC_FORCE, be.VEC_RHS)
        ctx.assemble_K(be.VEC_DOF)
        ctx.dofset_dirichlet_newton(ctx.dofset(cons), be.VEC_RESIDUAL)

        def timed(fn):
            out = fn()                                               # warm-up (allocations, the band order)
            ts = []
            for _ in range(reps):
                ctx.sync()
                t0 = time.perf_counter()
                out = fn()
                ctx.sync()
                ts.append((time.perf_counter() - t0) * 1e3)
            return float(np.median(ts)), out
        t_direct, info = timed(lambda: ctx.direct_solve(be.VEC_RESIDUAL, be.VEC_X))
        xd = ctx.download(be.VEC_X)
        t_pcg, res = timed(lambda: ctx.pcg(be.VEC_RESIDUAL, be.VEC_TMP0, eps=1e-12, maxit=10 * ctx.n))
        xp = ctx.download(be.VEC_TMP0)
        return {"system": label, "dof": int(ctx.n), "sub_diagonals": int(info["bandwidth"]), "panels": int(info["panels"]),
                "band_mb": info["band_bytes"] / 1e6, "direct_ms": t_direct, "residual": info["residual"],
                "refinements": int(info["refinements"]), "negative_pivots": int(info["negative_pivots"]),
                "tight_pcg_ms": t_pcg, "tight_pcg_iterations": int(res[0]),
                "rel_diff_direct_vs_pcg": float(np.linalg.norm(xd - xp) / max(np.linalg.norm(xd), 1e-300))}
    finally:
        ctx.close()


class RankEnv:
    """what a rank needs to set a problem up: arguments, rank numbers, torch.distributed (or None), the modules"""

    def __init__(self, **kw):
        self.__dict__.update(kw)

    def barrier(self):
        if self.use_dist:
            self.dist.barrier()

    def dev(self):
        return "cuda" if self.on_gpu else "cpu"

    def agreed_elapsed(self, t0):
        """seconds since t0, maximum over the ranks"""
        dt = time.perf_counter() - t0
        if self.use_dist:
            box = self.torch.tensor([dt], dtype=self.torch.float64, device=self.dev())
            self.dist.all_reduce(box, op=self.dist.ReduceOp.MAX)
            dt = float(box.item())
        return dt

    def agree_min(self, flag):
        if self.use_dist:
            box = self.torch.tensor([int(flag)], dtype=self.torch.int32, device=self.dev())
            self.dist.all_reduce(box, op=self.dist.ReduceOp.MIN)
            return int(box.item())
        return int(flag)

    def agree_max(self, flag):
        if self.use_dist:
            box = self.torch.tensor([int(flag)], dtype=self.torch.int32, device=self.dev())
            self.dist.all_reduce(box, op=self.dist.ReduceOp.MAX)
            return int(box.item())
        return int(flag)


def rank_problem(env, cells, quadratic, use_comm, element, material_cls):
    """this rank's share of the twist plate on `cells` at state S1, ready to step: context, communicator, the interface
    exchange chosen by measurement, the persistent PCG across ranks agreed and cross-checked, BOTH multi-rank PCG paths
    timed (so that one record of a multi-GPU run holds the whole decomposition even when a path falls back)."""
    args, N, rank, be, dist, torch = env.args, env.N, env.rank, env.be, env.dist, env.torch
    nx, ny, nz = cells
    elastic = (2.0e11, 0.3)
    if use_comm:
        if nz % N == 0:
            part = env.partition.plate_slab_part(nx, ny, nz, N, rank)      # this rank's cell layers only
        else:                                                              # odd debug grids: cut the global mesh
            g = env.meshgen.twist_plate(nx, ny, nz)
            part = env.partition.build_part(g["nodes"], g["elements"], N, rank)
        nodes, el = part.nodes, part.elements
        bcs, _ = env.meshgen.twist_plate_bcs(nodes)
        ne_global, n_global = 6 * nx * ny * nz, 3 * (nx + 1) * (ny + 1) * (nz + 1)
    else:
        part = None
        # FEMCY_BENCH_RENUM=1 numbers the mid-side nodes of the C3D10 plate next to the corners they connect instead of
        # behind all corners (measured in this bench: PCG iteration -4 %, row-centric assembly +50 %; default off)
        mesh = env.meshgen.twist_plate(nx, ny, nz, quadratic=quadratic,
                                       renumber=quadratic and os.environ.get("FEMCY_BENCH_RENUM", "0") == "1")
        nodes, el, bcs, elastic = mesh["nodes"], mesh["elements"], mesh["dirichlet_bc_info"], mesh["elastic"]
        ne_global, n_global = el.shape[0], nodes.size
    u, cons = s1_state(nodes, bcs, env.user_values)

    # FEMCY_BENCH_ALL_ON_GPU0=1 (with FEMCY_BENCH_TRANSPORT=shm, FEMCY_BENCH_DIST_BACKEND=gloo, FEMCY_BENCH_DEVICE=cpu): the N
    # ranks of this very program as N processes on ONE GPU -- RCCL refuses that, the shared-memory transport does not --
    # each with 1/N of the CUs' worth of persistent workgroups so that the ranks' kernels are co-resident.  Rates mean
    # nothing then; what it exercises is every host step of a multi-GPU run plus the cross-process mailbox path
    # (tools/r04_gpu2.sh).
    one_gpu = os.environ.get("FEMCY_BENCH_ALL_ON_GPU0") == "1"
    ctx = be.Context(0 if one_gpu else env.local_rank)
    if one_gpu and N > 1:
        ctx.set_option(107, max(8, (256 // N) // 8 * 8))        # FEMCY_TUNE_PERSIST_WGS
    for var, opt in (("FEMCY_BENCH_SIGMA", be.OPT_SELL_SIGMA),            # tuning knob: SELL sorting window
                     ("FEMCY_BENCH_PERSIST", be.OPT_PCG_PERSIST),         # 0 = the three-kernel PCG loop (comparison records)
                     ("FEMCY_BENCH_VARIANT", be.TUNE_PERSIST_VARIANT),    # persistent PCG variant bits (comparison records)
                     ("FEMCY_BENCH_NODE_ORDER", getattr(be, "OPT_NODE_ORDER", None)),
                     ("FEMCY_BENCH_STORAGE_ORDER", getattr(be, "OPT_PCG_STORAGE_ORDER", None))):
        if os.environ.get(var) and opt is not None:
            ctx.set_option(opt, int(os.environ[var]))
    ctx.set_mesh(nodes, el)
    ctx.set_element(element)
    ctx.set_material(material_cls(*elastic))
    info = ctx.build_pattern()
    exchange = pmulti = None
    if use_comm:
        if os.environ.get("FEMCY_BENCH_TRANSPORT") == "shm":     # processes of one host, no RCCL (see above)
            uid = [be.Context.comm_shm_id(1 << 20) if rank == 0 else None]
        else:
            uid = [be.Context.comm_unique_id() if rank == 0 else None]
        if env.use_dist:
            dist.broadcast_object_list(uid, src=0)
        with Watchdog(args.comm_timeout, "femcy_comm_init (RCCL communicator)"):
            ctx.comm_init(rank, N, uid[0], part.iface_local_dofs, part.iface_global_slot, part.niface_global, part.owner)
        # interface exchange: measure the packed all-reduce against send/recv with the slab neighbours and keep the
        # faster one (all ranks decide alike from the maximum over the ranks); --exchange pins it
        exchange = {"exchange": "allreduce", "allreduce_us": None, "neighbour_us": None}
        if hasattr(ctx, "comm_set_neighbours"):
            ctx.comm_set_neighbours(part)
            if args.exchange == "auto":
                try:
                    with Watchdog(args.comm_timeout, "femcy_comm_tune"):
                        exchange = ctx.comm_tune(20)
                    failed = 0
                except be.FemcyError as e:                  # the send/recv form is the newer one: never let it take the
                    log(f"[bench] rank {rank}: comm_tune failed ({e}); using the all-reduce exchange")     # run down
                    failed = 1
                failed = env.agree_max(failed)              # every rank must run the same exchange
                if failed:
                    ctx.set_option(be.OPT_EXCHANGE, 0)
                    exchange = {"exchange": "allreduce", "allreduce_us": None, "neighbour_us": None, "tune": "failed"}
            else:
                ctx.set_option(be.OPT_EXCHANGE, 1 if args.exchange == "neighbour" else 0)
                exchange["exchange"] = args.exchange
        # the one-launch PCG on every rank, the ranks' kernels exchanging through mailboxes in each other's HBM
        # (femcy.h "Persistent PCG across ranks"): blobs all-gathered here, the path agreed collectively; a rank on
        # which a step fails still takes part in the agreement (with a "no")
        pmulti = {"enabled": False, "mailbox_round_trip_us": None}
        if hasattr(ctx, "comm_mailbox_export") and os.environ.get("FEMCY_BENCH_PERSIST_MULTI", "1") != "0":
            try:                                                 # export may fail on ONE rank: it still joins the
                blob = ctx.comm_mailbox_export()                 # all-gather below (with None), or the others hang in it
            except Exception as e:                               # noqa: BLE001
                log(f"[bench] rank {rank}: mailbox export failed ({e})")
                blob = None
            imported = 0
            try:
                with Watchdog(args.comm_timeout, "mailbox exchange"):
                    blobs = [None] * N
                    if env.use_dist:
                        dist.all_gather_object(blobs, blob)
                    else:
                        blobs = [blob]
                    if any(b is None for b in blobs):
                        raise RuntimeError(f"no mailbox on rank(s) {[i for i, b in enumerate(blobs) if b is None]}")
                    ctx.comm_mailbox_import(blobs)
                    imported = 1
            except Exception as e:                               # noqa: BLE001
                log(f"[bench] rank {rank}: mailbox set-up failed ({e}); this rank votes for the RCCL loop")
                ctx.set_option(be.OPT_PCG_PERSIST_MULTI, 0)
            with Watchdog(args.comm_timeout, "femcy_comm_persist_agree"):
                pmulti["enabled"] = bool(ctx.comm_persist_agree())
            pmulti["agreed"] = pmulti["enabled"]
            # the mailbox round trip between the ranks' kernels (xGMI latency + skew), measured by the solver's own
            # cross-rank reduction in a one-wave kernel per rank; collective, so only if EVERY rank imported (--full)
            if args.full and env.agree_min(imported) and hasattr(ctx, "probe_mailbox"):
                try:
                    with Watchdog(args.comm_timeout, "mailbox probe"):
                        env.barrier()
                        ok, us = 1, ctx.probe_mailbox(2000)
                except be.FemcyError as e:
                    log(f"[bench] rank {rank}: mailbox probe failed ({e})")
                    ok, us = 0, None
                if env.agree_min(ok):
                    pmulti["mailbox_round_trip_us"] = us
        try:
            _, nranks_seen, _ = ctx.comm_info() if hasattr(ctx, "comm_info") else (None, N, None)
        except Exception:                                        # noqa: BLE001
            nranks_seen = None
        exchange["communicator_ranks"] = nranks_seen

    ctx.upload(be.VEC_DOF, u)
    ctx.vector(be.VEC_RHS).fill(0.0)
    ctx.internal_force(be.VEC_DOF, be.VEC_FORCE)           # multi-rank: already summed over the interface
    ctx.vec_sub(be.VEC_RESIDUAL, be.VEC_FORCE, be.VEC_RHS)           # Newton residual = f_int - rhs
    cons_set = ctx.dofset(cons)            # device-resident *Boundary DOF list (what System_of_equations uses)

    def step(iters=None):
        ctx.assemble_K(be.VEC_DOF)
        ctx.dofset_dirichlet_newton(cons_set, be.VEC_RESIDUAL)
        return ctx.pcg(be.VEC_RESIDUAL, be.VEC_X, eps=0.0, maxit=iters or args.iters)

    # --exchange auto, second half: femcy_comm_tune compared the bare exchanges (and cross-checked their sums); what
    # counts is the whole iteration -- the send/recv form splits the product and adds launches, the all-reduce form
    # moves the whole interface vector through every rank -- so one untimed step is run with each, the maximum over the
    # ranks is taken, and every rank keeps the faster form.
    def timed_step_all_ranks(iters=None):
        env.barrier()
        ctx.sync()
        t0 = time.perf_counter()
        step(iters)
        ctx.sync()
        return env.agreed_elapsed(t0)

    if use_comm and args.exchange == "auto" and exchange.get("tune") != "failed" \
            and exchange.get("neighbour_us") is not None and exchange["neighbour_us"] >= 0:
        trial = {}
        if pmulti and pmulti["enabled"]:
            ctx.set_option(be.OPT_PCG_PERSIST_MULTI, 0)          # the trial is about the loop that uses the exchange
        with Watchdog(2 * args.comm_timeout, "exchange trial steps"):
            for name, code in (("allreduce", 0), ("neighbour", 1)):
                ctx.set_option(be.OPT_EXCHANGE, code)
                step(100)                                        # connections, split lists, clocks
                trial[name] = min(timed_step_all_ranks(100), timed_step_all_ranks(100))
        pick = "neighbour" if trial["neighbour"] < trial["allreduce"] else "allreduce"
        ctx.set_option(be.OPT_EXCHANGE, 1 if pick == "neighbour" else 0)
        exchange["exchange"] = pick
        exchange["step_ms_100_iterations"] = {k: v * 1e3 for k, v in trial.items()}
        if pmulti and pmulti["enabled"]:
            ctx.set_option(be.OPT_PCG_PERSIST_MULTI, 1)

    # persistent PCG across ranks, second half: one short solve with it and one with the three-launch + collective loop
    # must give the same numbers (the scalars are global: every rank sees the same ones); otherwise every rank keeps
    # the loop.  A solve that times out anywhere falls back everywhere by itself.
    if use_comm and pmulti and pmulti["enabled"]:
        with Watchdog(2 * args.comm_timeout, "persistent multi-rank PCG cross-check"):
            ctx.assemble_K(be.VEC_DOF)
            ctx.dofset_dirichlet_newton(cons_set, be.VEC_RESIDUAL)
            ctx.set_option(be.OPT_PCG_PERSIST_MULTI, 0)
            ref3 = ctx.pcg(be.VEC_RESIDUAL, be.VEC_X, eps=0.0, maxit=25)
            ctx.set_option(be.OPT_PCG_PERSIST_MULTI, 1)
            t_before = ctx.timing()
            got = ctx.pcg(be.VEC_RESIDUAL, be.VEC_X, eps=0.0, maxit=25)
            t_after = ctx.timing()
        took = t_after["solves_persist"] > t_before["solves_persist"]
        same = got[0] == ref3[0] and abs(got[2] - ref3[2]) <= 1e-8 * abs(ref3[2])
        verdict = env.agree_min(1 if (took and same) else 0)
        pmulti.update(took_persistent_path=bool(took), matches_three_launch_loop=bool(same), enabled=bool(verdict))
        if not verdict:
            ctx.set_option(be.OPT_PCG_PERSIST_MULTI, 0)
            log(f"[bench] rank {rank}: persistent multi-rank PCG not used (took {took}, same {same}): RCCL loop")

    # both multi-rank PCG paths, timed back to back (solves of 100 iterations, best of three, maximum over the ranks):
    # whatever the run ends up using, the record holds the price of the other one too (--full)
    if args.full and use_comm and pmulti is not None:
        paths = {}
        with Watchdog(4 * args.comm_timeout, "timing of the multi-rank PCG paths"):
            ctx.assemble_K(be.VEC_DOF)
            ctx.dofset_dirichlet_newton(cons_set, be.VEC_RESIDUAL)
            for name, flag in (("persistent_across_ranks", 1), ("three_launches_plus_collectives", 0)):
                if flag and not pmulti["enabled"]:
                    paths[name] = None
                    continue
                ctx.set_option(be.OPT_PCG_PERSIST_MULTI, flag)
                best = None
                for rep in range(4):
                    env.barrier()
                    ctx.sync()
                    t1 = time.perf_counter()
                    it = ctx.pcg(be.VEC_RESIDUAL, be.VEC_X, eps=0.0, maxit=100)[0]
                    ctx.sync()
                    dt = env.agreed_elapsed(t1) / max(it, 1) * 1e6
                    if rep:                                      # the first solve of a path warms it up
                        best = dt if best is None else min(best, dt)
                paths[name] = best
            ctx.set_option(be.OPT_PCG_PERSIST_MULTI, 1 if pmulti["enabled"] else 0)
        pmulti["us_per_iteration"] = paths
    return {"ctx": ctx, "info": info, "exchange": exchange, "pmulti": pmulti, "ne_global": ne_global, "n_global": n_global,
            "step": step, "cons_set": cons_set, "cells": cells}


def strong_scaling_record(env, element, material_cls, iters=300):
    """BASELINE's metric reads "1M C3D4 elems, 1/2/4/8 GPU": the SAME 995 328-element plate cut into N z-slabs (strong
    scaling), measured after the weak-scaling headline of a multi-GPU run: CG iterations / s of whole solves of
    `iters` iterations with the path the ranks agreed on, both paths' microseconds per iteration, the mailbox probe"""
    t0 = time.time()
    cells = env.meshgen.scaling_cells(1)
    if os.environ.get("FEMCY_BENCH_STRONG_CELLS"):               # debug / CPU tests: a small plate instead
        cells = tuple(int(v) for v in os.environ["FEMCY_BENCH_STRONG_CELLS"].split(","))
    prob = rank_problem(env, cells, False, True, element, material_cls)
    ctx, be = prob["ctx"], env.be
    try:
        prob["step"](iters)
        best = None
        for _ in range(3):
            env.barrier()
            ctx.sync()
            t1 = time.perf_counter()
            it = prob["step"](iters)[0]
            ctx.sync()
            dt = env.agreed_elapsed(t1)
            best = dt if best is None else min(best, dt)
        tm = ctx.timing()
        return {"workload": f"twist plate C3D4 {cells[0]}x{cells[1]}x{cells[2]} cells, {prob['ne_global']} elements cut into "
                            f"{env.N} z-slabs (BASELINE's 1 M mesh on {env.N} GPUs)",
                "scaling": "strong", "n_gpus": env.N, "elements_per_gpu": int(ctx.ne), "dof_per_gpu": int(ctx.n),
                "cg_iters_per_step": iters, "value": it / best, "unit": "CG iters/s (assembly + Dirichlet + solve)",
                "ms_per_step": best * 1e3, "interface_exchange": prob["exchange"],
                "persistent_pcg_across_ranks": prob["pmulti"],
                "solves_persist": int(tm["solves_persist"]), "solves_three": int(tm["solves_three"]),
                "barrier_timeouts": int(tm["barrier_timeouts"]), "wall_s": time.time() - t0}
    finally:
        ctx.close()



def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--gpus", type=int, default=1)
    ap.add_argument("--steps", type=int, default=40)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--iters", type=int, default=1000,
                    help="PCG iterations per step (the reference's own solve of this system -- eps = 1e-3 -- takes 891)")
    ap.add_argument("--scaling", choices=("weak", "strong"), default="weak",
                    help="weak (default, the contract's line): 995 328 elements per GPU; strong: BASELINE's 1 M-element "
                         "plate cut into N z-slabs.  A weak --full run on N > 1 GPUs appends a short strong-scaling "
                         "record (`strong_scaling`) unless --no-strong")
    ap.add_argument("--no-strong", action="store_true", help="N > 1, --scaling weak: skip the appended strong-scaling record")
    ap.add_argument("--workload", choices=("c3d4", "c3d10", "cpe8"), default="c3d4",
                    help="c3d4 = BASELINE configs[2]/[3] (the metric's configuration); c3d10 = configs[4], single GPU; "
                         "cpe8 = configs[1] (2-D: generated plane-strain beam, ~1 M DOF), single GPU")
    ap.add_argument("--sample", type=int, default=16, help="time every k-th SpMV launch with HIP events (1 = all)")
    ap.add_argument("--prewarm", type=float, default=4.0, help="seconds of untimed steps before the warm-up steps")
    ap.add_argument("--no-cpu-baseline", action="store_true", help="--full without the CPU baseline leg")
    ap.add_argument("--cpu-baseline", choices=("tuned", "both"), default="tuned",
                    help="tuned = one pinned thread per physical core (default); both = also the unpinned all-threads run")
    ap.add_argument("--hbm-bound", choices=("auto", "off"), default="auto",
                    help="auto: an N = 1 --full run of the default workload also measures the HBM-bound configurations "
                         "(8 M C3D4 on this GPU, 124 k C3D10) and reports them under `hbm_bound`")
    ap.add_argument("--force-comm", action="store_true", help="N=1: still run the RCCL exchange path (1-rank communicator)")
    ap.add_argument("--force-dist", action="store_true", help="N=1: still create the torch.distributed (nccl) group and use its barrier / broadcast / all-reduce (exercises the N>1 host code on one GPU)")
    ap.add_argument("--exchange", choices=("auto", "allreduce", "neighbour"), default="auto",
                    help="N>1: interface exchange per CG iteration.  auto (default) = measure both forms at start-up "
                         "(femcy_comm_tune: cross-checks their sums, takes the maximum time over the ranks) and keep "
                         "the faster, falling back to the all-reduce if the measurement fails; allreduce = the packed "
                         "global interface vector; neighbour = send/recv with the slab neighbours (overlapped with "
                         "the product of the interior rows)")
    ap.add_argument("--cells", type=str, default=None, help="override nx,ny,nz (debug / small runs)")
    ap.add_argument("--launch-timeout", type=float, default=3600.0, help="self-launched N > 1 job: kill after this many seconds")
    ap.add_argument("--comm-timeout", type=float, default=300.0, help="seconds allowed for communicator set-up / tuning")
    ap.add_argument("--full", action="store_true",
                    help="also measure what takes runs of its own: roofline with its ceiling probes, cpu_baseline, "
                         "direct_branch, hbm_bound; N > 1: strong_scaling, both multi-rank PCG paths, the mailbox probe")
    ap.add_argument("--dump-outputs", metavar="DIR", default=None,
                    help="write the outputs of the last timed step to DIR/<name>.npy (float64)")
    ap.add_argument("--cpu-leg", type=str, default=None, help=argparse.SUPPRESS)   # internal: the pinned child process
    args = ap.parse_args()
    if args.steps < 1 or args.warmup < 0:
        ap.error("--steps must be >= 1 and --warmup >= 0")

    if args.cpu_leg:                                            # child of cpu_baseline_subprocess(): host work only
        return cpu_leg_main(args.cpu_leg)

    world_env = os.environ.get("WORLD_SIZE")
    N = args.gpus
    if world_env is None and N > 1:                             # typed as documented, without a launcher: start the ranks
        sys.exit(self_launch(N, sys.argv[1:], args.launch_timeout))

    # the contract is ONE JSON line on rank 0's stdout: libraries (RCCL prints a version banner on init) must not
    # be able to add to it, so fd 1 is pointed at stderr for the whole run and the JSON goes to the saved fd
    real_stdout = os.fdopen(os.dup(1), "w")
    sys.stdout.flush()
    os.dup2(2, 1)

    import torch
    import torch.distributed as dist
    from femcy_amd import backend as be, meshgen, partition
    from femcy_amd.element_zoo import Element_linear_tetrahedral, Element_quadratic_tetrahedral
    from femcy_amd.material_zoo import LinearIsotropic
    from femcy_amd.user_defined import user_dirichletBC_values

    world = int(world_env or "1")
    rank = int(os.environ.get("RANK", "0"))
    local_rank = int(os.environ.get("LOCAL_RANK", "0"))
    if world != N:
        raise SystemExit(f"WORLD_SIZE={world} does not match --gpus {N}")
    if args.workload == "cpe8":
        if N > 1 or args.force_comm or args.force_dist:
            raise SystemExit("--workload cpe8 is BASELINE configs[1], a single-GPU configuration")
        result = cpe8_line(args, be, meshgen, torch, user_dirichletBC_values)
        real_stdout.write(json.dumps(result) + "\n")
        real_stdout.flush()
        return 0
    quadratic = args.workload == "c3d10"
    if quadratic and (N > 1 or args.force_comm):
        raise SystemExit("--workload c3d10 is BASELINE configs[4], a single-GPU configuration")
    # test hooks (tests/test_bench_multirank_cpu.py runs the N>1 host logic on CPU with gloo and a mock Context):
    dist_backend = os.environ.get("FEMCY_BENCH_DIST_BACKEND", "nccl")
    on_gpu = os.environ.get("FEMCY_BENCH_DEVICE", "cuda") == "cuda"
    if os.environ.get("FEMCY_BENCH_MOCK"):                      # "module:Class" standing in for backend.Context (CPU tests)
        import importlib
        mod, cls = os.environ["FEMCY_BENCH_MOCK"].split(":")
        be.Context = getattr(importlib.import_module(mod), cls)
    if on_gpu:
        torch.cuda.set_device(local_rank)
    use_dist = N > 1 or args.force_dist
    if use_dist:
        os.environ.setdefault("MASTER_ADDR", "127.0.0.1")
        os.environ.setdefault("MASTER_PORT", "29533")
        with Watchdog(args.comm_timeout, "torch.distributed process group"):
            if on_gpu:
                dist.init_process_group(dist_backend, rank=rank, world_size=world,
                                        device_id=torch.device("cuda", local_rank))
            else:
                dist.init_process_group(dist_backend, rank=rank, world_size=world)

    # ------------------------------------------------------------------ problem (deterministic, O(local) per rank)
    t0 = time.time()
    strong = args.scaling == "strong"
    if args.cells:
        nx, ny, nz = tuple(int(v) for v in args.cells.split(","))
    else:
        nx, ny, nz = (48, 6, 72) if quadratic else (meshgen.scaling_cells(1) if strong else meshgen.scaling_cells(N))
    use_comm = N > 1 or args.force_comm
    env = RankEnv(args=args, N=N, rank=rank, local_rank=local_rank, use_dist=use_dist, on_gpu=on_gpu, dist=dist, torch=torch,
                  be=be, meshgen=meshgen, partition=partition, user_values=user_dirichletBC_values)

    # ------------------------------------------------------------------ CPU baseline leg (rank 0, N = 1 only), FIRST:
    # it is host work (20-40 s); running it before the device leg keeps the GPU-busy part of the command contiguous
    cpu = None
    want_cpu = args.full and rank == 0 and N == 1 and not args.no_cpu_baseline
    if want_cpu:
        try:
            cpu = cpu_baseline_subprocess(nx, ny, nz, "C3D10" if quadratic else "C3D4", args.cpu_baseline == "both")
        except Exception as e:   # the checker must never take the GPU number down with it
            log(f"[bench] cpu_baseline failed: {e!r}")

    prob = rank_problem(env, (nx, ny, nz), quadratic, use_comm,
                        Element_quadratic_tetrahedral() if quadratic else Element_linear_tetrahedral(), LinearIsotropic)
    ctx, info, exchange, pmulti = prob["ctx"], prob["info"], prob["exchange"], prob["pmulti"]
    ne_global, n_global, step, cons_set = prob["ne_global"], prob["n_global"], prob["step"], prob["cons_set"]
    barrier, agreed_elapsed = env.barrier, env.agreed_elapsed
    n, ne = ctx.n, ctx.ne
    if rank == 0:
        log(f"[bench] {args.workload} cells {nx}x{ny}x{nz}: {ne_global} elements / {n_global} DOF global, {ne} elements "
            f"/ {n} DOF per rank, nnzb {info.nnzb}, setup {time.time()-t0:.1f}s")

    # untimed pre-warm on top of the W warmup steps: a fresh box needs ~1 s of load before the GPU sits at its
    # sustained clocks (first bench of a cold box measured 4-6 % low with 2 warmup steps = 46 ms of work), and an
    # external utilisation sampler needs seconds, not the 0.5 s of the timed region, to see the device busy.  A step
    # holds collectives, so the ranks must agree on the number of pre-warm steps: the stop test uses the MAX of the
    # elapsed time over the ranks.
    t_warm = time.perf_counter()
    while args.warmup > 0:
        step()
        ctx.sync()
        if agreed_elapsed(t_warm) >= args.prewarm:
            break
    ctx.set_option(be.OPT_TIMING, args.sample)    # HIP events on the ctx stream; every k-th SpMV launch is sampled
    for _ in range(args.warmup):
        step()
    ctx.timing_reset()

    def device_sync():
        if on_gpu:
            torch.cuda.synchronize()
        else:
            ctx.sync()

    barrier()
    device_sync()
    t_start = time.perf_counter()
    total_iters = 0
    for _ in range(args.steps):
        it, r0, rmax = step()
        total_iters += it
    device_sync()
    barrier()
    elapsed = time.perf_counter() - t_start
    if use_dist:
        t = torch.tensor([elapsed], dtype=torch.float64, device="cuda" if on_gpu else "cpu")
        dist.all_reduce(t, op=dist.ReduceOp.MAX)
        elapsed = float(t.item())
    tm = ctx.timing()
    ctx.set_option(be.OPT_TIMING, 0)
    if args.dump_outputs:
        dump_outputs(ctx, be, args.dump_outputs, (it, r0, rmax), rank, N)
    spmv_bytes, iter_bytes = algorithmic_bytes(info, ctx.nn, n)
    spmv_us = tm["spmv_ms"] * 1e3 / max(tm["spmv_launches"], 1)
    cg_only = total_iters / (tm["pcg_ms"] * 1e-3) if tm["pcg_ms"] > 0 else 0.0

    # ------------------------------------------------------------------ roofline of the dominant kernel (--full)
    roof = probe = None
    if args.full:
        probe = hbm_copy_probe(torch) if (on_gpu and rank == 0) else None
        persist = tm["persist_launches"] > 0 and tm["spmv_launches"] == 0
        iter_gbs = iter_bytes * total_iters / (tm["pcg_ms"] * 1e-3) / 1e9 if tm["pcg_ms"] > 0 else 0.0
        if persist:
            roof = persist_roofline(ctx, be, tm, args, n, iter_bytes, probe, rank)
            kernel = "k_pcg_persist"
        else:
            kernel = "k_spmv"
            achieved = spmv_bytes / (spmv_us * 1e-6) / 1e9 if spmv_us > 0 else 0.0
            roof = {"kernel": f"k_spmv<{ctx.dm}> (compute_Ad)", "bound": "hbm", "achieved": achieved, "peak": HBM_PEAK_GBS,
                    "unit": "GB/s", "frac": achieved / HBM_PEAK_GBS, "peak_source": "spec (MI355X HBM3E)",
                    "frac_of_copy_probe": (achieved / probe) if probe else None,
                    "bytes_per_launch": int(spmv_bytes), "avg_launch_us": spmv_us, "launches_timed": int(tm["spmv_launches"])}
        if not persist and on_gpu and rank == 0 and not use_comm and hasattr(ctx, "probe_spmv"):
            # the product launch to launch (200 back-to-back launches, one HIP event pair): see hbm_bound_record
            try:
                b2b = min(ctx.probe_spmv(200, os.environ.get("FEMCY_BENCH_STORAGE_ORDER", "1") != "0") for _ in range(3))
                roof["launch_to_launch_us"] = b2b
                roof["launch_to_launch_gbs"] = spmv_bytes / (b2b * 1e-6) / 1e9
                roof["launch_to_launch_frac"] = roof["launch_to_launch_gbs"] / HBM_PEAK_GBS
            except be.FemcyError as e:
                log(f"[bench] femcy_probe_spmv failed: {e}")
        if not persist and on_gpu and rank == 0:
            rprobe = read_stream_probe(ctx, be, info.stored_blocks * 76)
            roof["read_stream_probe_gbs"] = rprobe
            roof["frac_of_read_stream_probe"] = (roof["achieved"] / rprobe) if rprobe else None
        traffic, traffic_src = pmc_traffic(args.workload, kernel, layout_signature(info)) if not args.cells else (None, "non-standard --cells")
        roof["traffic"], roof["traffic_source"] = traffic, traffic_src
        roof["copy_probe_gbs"] = probe
        roof["pcg_iteration_gbs"] = iter_gbs
        roof["pcg_iteration_frac_of_hbm_peak"] = iter_gbs / HBM_PEAK_GBS
        if traffic is not None and roof.get("avg_launch_us", 0) > 0:
            # the rate of the bytes that actually moved between the L2s and the fabric (HBM + Infinity Cache): PMC counters
            roof["traffic_gbs"] = traffic / (roof["avg_launch_us"] * 1e-6) / 1e9
            roof["traffic_over_moved"] = traffic / roof["bytes_per_launch"] if roof.get("bytes_per_launch") else None

    asm_ms = (tm["geom_ms"] + tm["assemble_ms"]) / max(tm["assemble_launches"], 1)
    per_gpu = ELEMS_PER_GPU[args.workload]
    scale = ne_global / per_gpu                                       # weak: N; strong (one 1 M mesh for all N): 1
    kflop_per_elem = 57.0 if quadratic else 2.9                       # as-written dense contraction
    etype = "C3D10" if quadratic else "C3D4"
    which = ("BASELINE configs[4]" if quadratic else
             ("BASELINE configs[2], cut into N slabs" if strong else "BASELINE configs[2] at N=1, configs[3] at N=8"))

    result = {
        "metric": "CG iters/sec + element-stiffness assemblies/sec, 1M C3D4 elems, 1/2/4/8 GPU",
        "value": total_iters / elapsed * scale,
        "unit": f"CG iters/s x (global elements / {per_gpu})",
        "n_gpus": N, "steps": args.steps, "warmup": args.warmup,
        "ms_per_step": elapsed / args.steps * 1e3,
        "higher_is_better": True, "scaling": "strong" if strong else "weak", "vs_baseline": None,
        "dtype": "f64", "data": "synthetic",
        "config": {"workload": f"twist plate {etype} {nx}x{ny}x{nz} cells, {ne_global} elements, {n_global} DOF "
                               f"({which}), state S1 (t=0.05), "
                               f"step = assemble K + Dirichlet + {args.iters} PCG iterations",
                   "elements_per_gpu": int(ne), "cg_iters_per_step": args.iters, "layout": layout_signature(info),
                   "parallelism": (f"element z-slabs x{N}, slab-local mesh generation" +
                                   (" (strong scaling: the 1 M mesh cut into N)" if strong else "")) if N > 1 else "single GPU",
                   "launcher": "self-launched torch.distributed.run" if os.environ.get("FEMCY_BENCH_SELF_LAUNCHED") else
                               ("torch.distributed.run" if world_env is not None else "single process"),
                   "interface_exchange": exchange, "persistent_pcg_across_ranks": pmulti,
                   "transport": (None if not use_comm else
                                 ("shared-memory TEST transport (N processes on one GPU, host-staged collectives with two "
                                  "stream synchronisations each): exercises the host steps, its timings say nothing about RCCL"
                                  if os.environ.get("FEMCY_BENCH_TRANSPORT") == "shm" else "RCCL"))},
        # the step of rounds 1-3 held 500 PCG iterations (--iters 500 --steps 10): since round 4 the one assembly per step
        # is amortised over 1000, so `value` is NOT comparable with BENCH_r03 and earlier; `cg_iters_per_s` (PCG time
        # only) and `assemblies_per_s` are
        "notes": f"step = 1 assembly + Dirichlet + {args.iters} PCG iterations (500 until round 3); compare rounds through "
                 f"cg_iters_per_s / pcg_us_per_iter / assembly_ms, which do not depend on the step definition",
        "cg_iters_per_s": cg_only * scale,
        "assemblies_per_s": ne_global / (asm_ms * 1e-3) if asm_ms > 0 else 0.0,
        "assembly_ms": asm_ms,
        "pcg_us_per_iter": tm["pcg_ms"] * 1e3 / max(total_iters, 1),
        # algorithmic flop rates: SpMV 2*nnz per launch; assembly 2.9 (C3D4) / 57 (C3D10) kflop per element
        "spmv_tflops": (2 * info.nnz / (spmv_us * 1e-6) / 1e12 if spmv_us > 0 else
                        (2 * info.nnz * total_iters / (tm["pcg_ms"] * 1e-3) / 1e12 if tm["pcg_ms"] > 0 else 0.0)),
        "assembly_tflops": kflop_per_elem * 1e3 * ne_global / (asm_ms * 1e-3) / 1e12 if asm_ms > 0 else 0.0,
    }
    if args.full:
        result["roofline"] = roof
    if want_cpu:
        result["cpu_baseline"] = cpu
        if isinstance(cpu, dict) and isinstance(cpu.get("host_backend"), dict):     # scalars survive flattening parsers
            for k, v in cpu["host_backend"].items():
                if isinstance(v, (int, float)):
                    cpu[f"host_backend_{k}"] = v
    ctx.close()

    # ------------------------------------------------------------------ strong scaling beside the weak-scaling line:
    # BASELINE's metric names ONE mesh ("1M C3D4 elems") on 1 / 2 / 4 / 8 GPUs (--full)
    if args.full and use_comm and not strong and not args.no_strong and not quadratic and \
            (not args.cells or os.environ.get("FEMCY_BENCH_STRONG_CELLS")):
        try:
            rec = strong_scaling_record(env, Element_linear_tetrahedral(), LinearIsotropic)
        except Exception as e:                                   # noqa: BLE001  (never lose the headline line)
            log(f"[bench] rank {rank}: strong-scaling record failed: {e!r}")
            rec = {"error": repr(e)}
        # a failure on ANY rank voids the record (the others may have timed a fallback path)
        if env.agree_max(1 if "error" in rec else 0) and "error" not in rec:
            rec = {"error": "failed on another rank"}
        result["strong_scaling"] = rec

    # ------------------------------------------------- the reference's direct branch (deck-sized systems), --full
    if args.full and rank == 0 and N == 1 and on_gpu and args.hbm_bound == "auto" and not args.cells and not quadratic \
            and not args.force_comm and not args.force_dist:
        recs = []
        for label, gen, ele in (
                ("twist plate C3D4 8x2x12 cells (the size of the reference's twist_plate_C3D4 deck)",
                 lambda: meshgen.twist_plate(8, 2, 12), Element_linear_tetrahedral()),
                ("twist plate C3D10 8x2x12 cells (the size of twist_plate_C3D10)",
                 lambda: meshgen.twist_plate(8, 2, 12, quadratic=True), Element_quadratic_tetrahedral()),
                ("twist plate C3D4 24x6x36 cells (19 k DOF)",
                 lambda: meshgen.twist_plate(24, 6, 36), Element_linear_tetrahedral())):
            try:
                msh = gen()
                recs.append(direct_branch_record(be, label, msh, ele, LinearIsotropic(*msh["elastic"]),
                                                 user_dirichletBC_values))
            except Exception as e:                               # noqa: BLE001  (never lose the headline line)
                log(f"[bench] direct_branch record '{label[:40]}' failed: {e!r}")
                recs.append({"system": label, "error": repr(e)})
        result["direct_branch"] = recs

    # ------------------------------------------------------------------ the HBM-bound configurations, --full
    if args.full and rank == 0 and N == 1 and on_gpu and args.hbm_bound == "auto" and not args.cells and not quadratic \
            and not args.force_comm and not args.force_dist:
        recs = []
        for name, gen, ele in (
                ("twist plate C3D4 192x24x288 cells (BASELINE configs[3]'s 7 962 624 elements on ONE GPU)",
                 lambda: meshgen.twist_plate(192, 24, 288), Element_linear_tetrahedral()),
                ("twist plate C3D10 48x6x72 cells (BASELINE configs[4], 124 416 elements)",
                 lambda: meshgen.twist_plate(48, 6, 72, quadratic=True), Element_quadratic_tetrahedral()),
                # round 5: the 2-D configuration (BASELINE configs[1]; no CPE8 beam deck is shipped, SURVEY.md 8d: the
                # 40 x 4 beam of tests/beam_deflection meshed with serendipity quadrilaterals, plane strain, nlgeom)
                (CPE8_NAME, lambda: meshgen.beam_quad8(*CPE8_CELLS, plane="CPE8"), None),
                # round 6: BASELINE configs[4] OUT of cache (SURVEY 8d "C3D10 ... then raise k"): 2.99 GB of stored matrix
                ("twist plate C3D10 96x12x144 cells (BASELINE configs[4] at k = 12: 995 328 elements, 4 183 275 DOF)",
                 lambda: meshgen.twist_plate_k(12, quadratic=True), Element_quadratic_tetrahedral())):
            try:
                msh = gen()
                if ele is None:
                    from femcy_amd.element_zoo import Element_quadratic_quadrilateral
                    from femcy_amd.material_zoo import LinearIsotropicPlaneStrain
                    ele, mat = Element_quadratic_quadrilateral(), LinearIsotropicPlaneStrain(*msh["elastic"])
                else:
                    mat = LinearIsotropic(*msh["elastic"])
                recs.append(hbm_bound_record(be, name, msh, ele, mat, user_dirichletBC_values, probe))
                del msh
            except Exception as e:                               # noqa: BLE001  (never lose the headline line)
                log(f"[bench] hbm_bound record '{name[:40]}' failed: {e!r}")
                recs.append({"workload": name, "error": repr(e)})
        result["hbm_bound"] = recs

    if rank == 0:
        real_stdout.write(json.dumps(result) + "\n")
        real_stdout.flush()
    if use_dist:
        dist.destroy_process_group()


def cpe8_line(args, be, meshgen, torch, user_values):
    """`--workload cpe8`: the contract's line on the 2-D configuration.  One step = femcy_assemble_K (k_geom<8,2> +
    the CPE8 assembly) + Newton Dirichlet treatment + femcy_pcg(eps = 0, maxit = iters) on the generated plane-strain
    beam at state S1 (prescribed values of the first increment), inputs resident in HBM.  The dominant kernel is
    k_spmv<2> (2 x 2 blocks, 36 bytes per stored block): with --full its roofline comes from `hbm_bound_record` of the
    same mesh (launch to launch between one HIP event pair), PMC traffic from profiles/spmv_traffic.json when recorded."""
    from femcy_amd.element_zoo import Element_quadratic_quadrilateral
    from femcy_amd.material_zoo import LinearIsotropicPlaneStrain
    nx, ny = (int(v) for v in args.cells.split(",")[:2]) if args.cells else CPE8_CELLS
    mesh = meshgen.beam_quad8(nx, ny, plane="CPE8")
    ele, mat = Element_quadratic_quadrilateral(), LinearIsotropicPlaneStrain(*mesh["elastic"])
    nodes, el = mesh["nodes"], mesh["elements"]
    ti = mesh["time_incs"]
    ctx = be.Context(0)
    try:
        ctx.set_mesh(nodes, el)
        ctx.set_element(ele)
        ctx.set_material(mat)
        info = ctx.build_pattern()
        u, cons = s1_state(nodes, mesh["dirichlet_bc_info"], user_values, t1=ti["ini_inc"], load_ratio=ti["ini_inc"] / ti["max_time"])
        ctx.upload(be.VEC_DOF, u)
        ctx.vector(be.VEC_RHS).fill(0.0)
        ctx.internal_force(be.VEC_DOF, be.VEC_FORCE)
        ctx.vec_sub(be.VEC_RESIDUAL, be.VEC_FORCE, be.VEC_RHS)
        cs = ctx.dofset(cons)

        def step():
            ctx.assemble_K(be.VEC_DOF)
            ctx.dofset_dirichlet_newton(cs, be.VEC_RESIDUAL)
            return ctx.pcg(be.VEC_RESIDUAL, be.VEC_X, eps=0.0, maxit=args.iters)

        t_warm = time.perf_counter()
        while args.warmup > 0:
            step()
            ctx.sync()
            if time.perf_counter() - t_warm >= args.prewarm:
                break
        ctx.set_option(be.OPT_TIMING, args.sample)
        for _ in range(args.warmup):
            step()
        ctx.timing_reset()
        on_gpu = os.environ.get("FEMCY_BENCH_DEVICE", "cuda") == "cuda"      # (test hook: the host backend on CPU)
        if on_gpu:
            torch.cuda.synchronize()
        ctx.sync()
        t0 = time.perf_counter()
        total = 0
        for _ in range(args.steps):
            last = step()
            total += last[0]
        ctx.sync()
        if on_gpu:
            torch.cuda.synchronize()
        elapsed = time.perf_counter() - t0
        tm = ctx.timing()
        ctx.set_option(be.OPT_TIMING, 0)
        if args.dump_outputs:
            dump_outputs(ctx, be, args.dump_outputs, last, 0, 1)
        spmv_b, iter_b = algorithmic_bytes(info, ctx.nn, ctx.n)
        ne, n, dm = int(ctx.ne), int(ctx.n), int(ctx.dm)
        nnz = int(info.nnz)
        probe = hbm_copy_probe(torch) if (args.full and on_gpu) else None
        # the dominant kernel of the timed region: since round 5 a 2-D system of up to 8 192 slices takes the persistent
        # kernel (k_pcg_persist<2, 8, 2>: eight slices per wave); otherwise the product of the three-launch loop
        persist = tm["persist_launches"] > 0 and tm["spmv_launches"] == 0
        roof = persist_roofline(ctx, be, tm, args, n, iter_b, probe, 0) if (args.full and persist) else None
    finally:
        ctx.close()
    name = CPE8_NAME if not args.cells else f"beam CPE8 {nx}x{ny} serendipity quadrilaterals, plane strain, nlgeom"
    asm_ms = (tm["geom_ms"] + tm["assemble_ms"]) / max(tm["assemble_launches"], 1)
    # as-written flops of one CPE8 stiffness (B^T C B at 4 Gauss points, B 3 x 16: 2 * (3*3*16 + 16*3*16) * 4)
    kflop = 2 * (3 * 3 * 16 + 16 * 3 * 16) * 4 / 1e3
    line = {
        "metric": "CG iters/sec + element-stiffness assemblies/sec, 1M C3D4 elems, 1/2/4/8 GPU",
        "value": total / elapsed * (ne / ELEMS_PER_GPU["cpe8"]),
        "unit": f"CG iters/s x (global elements / {ELEMS_PER_GPU['cpe8']})",
        "n_gpus": 1, "steps": args.steps, "warmup": args.warmup, "ms_per_step": elapsed / args.steps * 1e3,
        "higher_is_better": True, "scaling": "weak", "vs_baseline": None, "dtype": "f64", "data": "synthetic",
        "config": {"workload": f"{name} (BASELINE configs[1]: the 2-D configuration, not the one the metric is quoted on), "
                               f"state S1 (first increment, load ratio {ti['ini_inc'] / ti['max_time']}), "
                               f"step = assemble K + Dirichlet + {args.iters} PCG iterations",
                   "elements_per_gpu": ne, "dof": n, "cg_iters_per_step": args.iters, "layout": layout_signature(info),
                   "parallelism": "single GPU", "launcher": "single process"},
        "cg_iters_per_s": total / (tm["pcg_ms"] * 1e-3) if tm["pcg_ms"] > 0 else 0.0,
        "assemblies_per_s": ne / (asm_ms * 1e-3) if asm_ms > 0 else 0.0,
        "assembly_ms": asm_ms,
        "pcg_us_per_iter": tm["pcg_ms"] * 1e3 / max(total, 1),
        "assembly_tflops": kflop * 1e3 * ne / (asm_ms * 1e-3) / 1e12 if asm_ms > 0 else 0.0,
    }
    if not args.full:
        return line
    rec = hbm_bound_record(be, name, mesh, ele, mat, user_values, probe)
    kernel = "k_pcg_persist" if persist else "k_spmv"
    if roof is None:
        roof = dict(rec["spmv"])
    traffic, traffic_src = pmc_traffic("cpe8", kernel, layout_signature(info)) if not args.cells else (None, "non-standard --cells")
    roof.update(traffic=traffic, traffic_source=traffic_src, copy_probe_gbs=probe,
                pcg_iteration_gbs=rec["pcg_iteration"]["achieved"], pcg_iteration_frac_of_hbm_peak=rec["pcg_iteration"]["frac"],
                pcg_iteration_us=rec["pcg_iteration"]["us"], pcg_path=rec["pcg_path"],
                spmv_launch_to_launch_us=rec["spmv"]["avg_launch_us"], spmv_frac_of_hbm_peak=rec["spmv"]["frac"])
    if traffic is not None and roof.get("avg_launch_us", 0) > 0:
        roof["traffic_gbs"] = traffic / (roof["avg_launch_us"] * 1e-6) / 1e9
        roof["traffic_over_moved"] = traffic / roof["bytes_per_launch"] if roof.get("bytes_per_launch") else None
    line.update(spmv_tflops=2 * nnz / (rec["spmv"]["avg_launch_us"] * 1e-6) / 1e12 if rec["spmv"].get("avg_launch_us") else 0.0,
                roofline=roof, hbm_bound=[rec])
    return line


def persist_roofline(ctx, be, tm, args, n, iter_bytes, probe, rank):
    """k_pcg_persist against the ceiling that binds it.  The kernel keeps the vectors and the register / LDS-resident
    block rows on chip for the whole solve; per iteration its layout makes it move
        the streamed block rows (femcy_persist_streamed_bytes: stored - resident, values + block columns)
      + 8 n bytes of d published + 8 n bytes of d read at least once by the gathers
    from / to the Infinity Cache (the matrix of this configuration lives there).  `peak` is what a read-only sweep of a
    buffer of the streamed size reaches in the kernel's own launch shape on this GPU, `achieved / peak` <= 1 is the
    roofline fraction.  The time model adds the price of the three grid-wide exchanges of an iteration, probed with the
    kernel's own exchange code: floor = streamed / peak + 3 x exchange."""
    launches = int(tm["persist_launches"])
    launch_us = tm["persist_ms"] * 1e3 / launches
    iters_per_launch = tm["persist_iters"] / launches
    streamed = ctx.persist_streamed_bytes() if hasattr(ctx, "persist_streamed_bytes") else 0
    moved_iter = streamed + 16 * n
    moved_launch = moved_iter * iters_per_launch
    achieved = moved_launch / (launch_us * 1e-6) / 1e9
    alg_launch = iter_bytes * iters_per_launch
    alg_gbs = alg_launch / (launch_us * 1e-6) / 1e9
    peak = exch = None
    variant = int(os.environ.get("FEMCY_BENCH_VARIANT", "-1"))
    if hasattr(ctx, "probe_stream") and streamed > 0:
        try:
            peak = max(ctx.probe_stream(max(streamed, 1 << 20), 30, 0)[0] for _ in range(3))
            # the exchange form the kernel uses: tagged granules (form 1) for the library's default variant (6) and every
            # variant with bit 1; per-XCD counters + data (form 0) otherwise
            eff = variant if variant >= 0 else 6
            form = int(os.environ.get("FEMCY_BENCH_EXCHANGE_FORM", "1" if (eff & 2) else "0"))
            exch = min(ctx.probe_exchange(2000, form) for _ in range(3))
        except be.FemcyError as e:
            log(f"[bench] ceiling probes failed: {e}")
    us_iter = launch_us / iters_per_launch
    roof = {"kernel": f"k_pcg_persist<{ctx.dm}> (one launch = {args.iters} PCG iterations: compute_Ad + the vector updates "
                      f"+ 3 grid-wide exchanges per iteration)",
            # the streamed part of the 1 M C3D4 matrix (112 MB) lives in the 256 MiB Infinity Cache; the C3D10 plate's
            # (287 MB) comes from HBM every iteration
            "bound": "infinity-cache" if streamed <= (240 << 20) else "hbm", "unit": "GB/s",
            "achieved": achieved, "peak": peak, "frac": (achieved / peak) if peak else None,
            "peak_source": "femcy_probe_stream: read-only sweep of the streamed footprint in the kernel's launch shape "
                           "(256 workgroups x 4 waves, 16-byte loads), this GPU, this run",
            "bytes_per_launch": int(moved_launch), "bytes_per_iteration": int(moved_iter),
            "streamed_matrix_bytes_per_iteration": int(streamed),
            "avg_launch_us": launch_us, "launches_timed": launches, "us_per_iteration": us_iter,
            # SURVEY.md 8d's storage-independent figure (what BASELINE's metric prices): above the HBM peak because the
            # bytes the kernel keeps on chip are counted
            "algorithmic_bytes_per_launch": int(alg_launch), "algorithmic_gbs": alg_gbs,
            "algorithmic_frac_of_hbm_peak": alg_gbs / HBM_PEAK_GBS, "hbm_peak": HBM_PEAK_GBS,
            # SURVEY 8d's fraction under the name the round-3 verdict asked for: > 1 because the matrix part the kernel
            # keeps in registers / LDS and all vectors never move, and the rest streams from the Infinity Cache -- NOT
            # an HBM-bandwidth claim (the HBM-bound fractions are in `hbm_bound`)
            "frac_8d_vs_hbm": alg_gbs / HBM_PEAK_GBS, "frac_8d_vs_hbm_note": "cache-resident: bytes that never reach HBM are counted"}
    if peak and exch:
        stream_us = streamed / (peak * 1e9) * 1e6
        floor = stream_us + 3 * exch
        roof["time_model"] = {"stream_us": stream_us, "exchange_us": exch, "exchanges_per_iteration": 3,
                              "floor_us_per_iteration": floor, "measured_us_per_iteration": us_iter,
                              "frac": floor / us_iter,
                              "exchange_form": "tagged granules" if form == 1 else "per-XCD counters + data",
                              "not_in_the_floor": "gathers of d, resident-row multiplies, wave / workgroup reductions, vector updates"}
        # the same as scalar keys (nested objects did not survive into the driver's parsed record in round 3)
        roof.update(time_model_stream_us=stream_us, time_model_exchange_us=exch, time_model_exchanges_per_iteration=3,
                    time_model_floor_us_per_iteration=floor, time_model_frac=floor / us_iter)
    return roof


# ---------------------------------------------------------------------------------------------- CPU baseline
def physical_cores():
    """(cpu ids, one per physical core) among the CPUs this process may run on"""
    allowed = sorted(os.sched_getaffinity(0)) if hasattr(os, "sched_getaffinity") else list(range(os.cpu_count() or 1))
    seen, pick = set(), []
    for cpu in allowed:
        try:
            base = f"/sys/devices/system/cpu/cpu{cpu}/topology/"
            key = (open(base + "physical_package_id").read().strip(), open(base + "core_id").read().strip())
        except OSError:
            key = ("?", str(cpu))
        if key not in seen:
            seen.add(key)
            pick.append(cpu)
    return pick


def cpu_baseline_subprocess(nx, ny, nz, etype, both):
    """runs cpu_leg_main in child processes whose OpenMP runtime is configured BEFORE it starts: one thread per
    physical core, bound (OMP_PLACES=cores, OMP_PROC_BIND=spread); the ELL arrays and CG vectors are first touched
    inside the same static parallel loops that later use them (oracle/femcy_oracle.c), so pages sit on the NUMA node of
    their thread.  `both`: also the round-2 configuration (all hardware threads, unbound) for comparison."""
    cores = physical_cores()
    # a container with a CPU quota (cgroup cpu.max) is throttled as soon as more threads than that run: the 128 pinned
    # threads of the first version of this leg got 260 CG iterations / s on a 16-CPU quota, 16 threads get 1.3 k
    nthreads = len(cores)
    try:
        q = open("/sys/fs/cgroup/cpu.max").read().split()
        if q[0] != "max":
            nthreads = max(1, min(nthreads, int(float(q[0]) / float(q[1]) + 0.5)))
    except (OSError, ValueError, IndexError):
        pass

    def run(env_extra, label):
        env = dict(os.environ)
        env.update(env_extra)
        out = subprocess.run([sys.executable, os.path.abspath(__file__), "--cpu-leg", f"{nx},{ny},{nz},{etype}"],
                             capture_output=True, text=True, env=env, timeout=1200)
        if out.returncode != 0:
            raise RuntimeError(f"cpu leg ({label}) failed: {out.stderr[-800:]}")
        rec = json.loads([l for l in out.stdout.splitlines() if l.startswith("{")][-1])
        rec["omp"] = {k: env_extra.get(k) for k in ("OMP_NUM_THREADS", "OMP_PLACES", "OMP_PROC_BIND")}
        return rec

    tuned = run({"OMP_NUM_THREADS": str(nthreads), "OMP_PLACES": "cores", "OMP_PROC_BIND": "spread"}, "pinned")
    tuned["physical_cores"] = len(cores)
    if both:
        try:
            un = run({"OMP_NUM_THREADS": str(os.cpu_count() or 1)}, "unpinned")
            tuned["unpinned_all_threads"] = {k: un[k] for k in ("value", "cores", "gbs", "assemblies_per_s", "sample")}
        except Exception as e:                                   # noqa: BLE001
            tuned["unpinned_all_threads"] = {"error": repr(e)}
    return tuned


def cpu_leg_main(spec):
    """oracle/femcy_oracle.c (the reference's algorithm as written: ELL n x W, per-entry linear search +
    atomic adds, thread-per-row SpMV, 8 vector passes + 4 reductions per CG iteration) with OpenMP, on a bounded sample
    of the same workload: 1 assembly + ~10 s of CG iterations.  Prints one JSON object."""
    nx, ny, nz, etype = spec.split(",")
    nx, ny, nz = int(nx), int(ny), int(nz)
    from femcy_amd import meshgen
    from femcy_amd.user_defined import user_dirichletBC_values
    mesh = meshgen.twist_plate(nx, ny, nz, quadratic=(etype == "C3D10"))
    u, cons = s1_state(mesh["nodes"], mesh["dirichlet_bc_info"], user_dirichletBC_values)
    rec = cpu_baseline(mesh["nodes"], mesh["elements"], mesh["elastic"], u, cons, etype)
    try:
        rec["host_backend"] = cpu_backend_point(mesh, u, cons, etype)
    except Exception as e:                                       # noqa: BLE001
        rec["host_backend"] = {"error": repr(e)}
    sys.stdout.write(json.dumps(rec) + "\n")
    sys.stdout.flush()
    return 0


def cpu_backend_point(mesh, u, cons, etype):
    """second, optimised CPU point: libfemcy_cpu.so, the host implementation of the same C ABI (block-CSR, fused PCG
    passes, owner-computes assembly; femcy_amd/csrc_cpu/) on the same mesh and state, ~5 s of CG in solves of 100"""
    from femcy_amd import backend as be
    from femcy_amd.element_zoo import Element_linear_tetrahedral, Element_quadratic_tetrahedral
    from femcy_amd.material_zoo import LinearIsotropic
    ctx = be.Context(0, backend="cpu")
    ctx.set_mesh(mesh["nodes"], mesh["elements"])
    ctx.set_element(Element_quadratic_tetrahedral() if etype == "C3D10" else Element_linear_tetrahedral())
    ctx.set_material(LinearIsotropic(*mesh["elastic"]))
    info = ctx.build_pattern()
    ctx.upload(be.VEC_DOF, u)
    ctx.vector(be.VEC_RHS).fill(0.0)
    ctx.internal_force(be.VEC_DOF, be.VEC_FORCE)
    ctx.vec_sub(be.VEC_RESIDUAL, be.VEC_FORCE, be.VEC_RHS)
    ctx.assemble_K(be.VEC_DOF)
    t = time.perf_counter()
    ctx.assemble_K(be.VEC_DOF)
    t_asm = time.perf_counter() - t
    ctx.dirichlet_newton(cons, be.VEC_RESIDUAL)
    ctx.pcg(be.VEC_RESIDUAL, be.VEC_X, eps=0.0, maxit=3)
    it, dt = 0, 0.0
    t_end = time.perf_counter() + 5.0
    while time.perf_counter() < t_end:
        t = time.perf_counter()
        k, _, _ = ctx.pcg(be.VEC_RESIDUAL, be.VEC_X, eps=0.0, maxit=100)
        dt += time.perf_counter() - t
        it += k
    spmv_b, iter_b = algorithmic_bytes(info, ctx.nn, ctx.n)
    rec = {"value": it / dt, "unit": "CG iters/s", "gbs_algorithmic": iter_b * it / dt / 1e9,
           "assemblies_per_s": ctx.ne / t_asm, "threads": int(os.environ.get("OMP_NUM_THREADS", os.cpu_count() or 1)),
           "what": "femcy_amd/libfemcy_cpu.so (host implementation of include/femcy.h), same mesh and state"}
    ctx.close()
    return rec


def cpu_baseline(nodes, el, elastic, u, cons, etype):
    from oracle.c_oracle import COracle
    from oracle.elements import elem_def
    from oracle.femcy_oracle import Material
    ed = elem_def(etype)
    t0 = time.time()
    co = COracle(nodes, el, ed.dN_table(), ed.gauss_weights, Material("lin3d", elastic).C)
    setup = time.time() - t0
    co.get_dsdx_and_vol(u)
    co.assemble()                                    # warm (page faults of the ELL array: first touch, in parallel)
    t = time.perf_counter()
    co.get_dsdx_and_vol(u)
    co.assemble()
    t_asm = time.perf_counter() - t
    co.zero_rows_cols_unit_diag(cons)
    f = co.internal_force(u, 0, *elastic)
    f[cons] = 0.0
    # CG in solves of 100 iterations from x0 = 0 (a single long solve would run past convergence into denormal
    # residuals, which cost the host cores up to 100x per operation and are not what the GPU step does either).
    # First a short scan over the thread count -- more threads than memory channels / the container's CPU quota can
    # feed only adds synchronisation -- then ~10 s at the best count.
    co.cg(f, eps=0.0, maxit=3)
    chunk = 100

    def sample(seconds):
        n_it, t_sum = 0, 0.0
        t_end = time.perf_counter() + seconds
        while time.perf_counter() < t_end:
            t = time.perf_counter()
            _, k, _, _ = co.cg(f, eps=0.0, maxit=chunk)
            t_sum += time.perf_counter() - t
            n_it += k
        return n_it, t_sum

    scan, tmax = {}, co.threads()
    try:
        import ctypes
        gomp = ctypes.CDLL("libgomp.so.1")
        nt = tmax
        while nt >= max(1, tmax // 16):
            gomp.omp_set_num_threads(int(nt))
            k, tt = sample(1.5)
            scan[int(nt)] = k / tt
            nt //= 2
        best = max(scan, key=scan.get)
        gomp.omp_set_num_threads(int(best))
    except Exception as e:                                       # noqa: BLE001
        scan = {"error": repr(e)}
        best = tmax
    it, dt = sample(10.0)
    quota = None
    try:
        q = open("/sys/fs/cgroup/cpu.max").read().split()
        quota = None if q[0] == "max" else float(q[0]) / float(q[1])
    except (OSError, ValueError, IndexError):
        pass
    # as-written bytes of one CG iteration: the ELL arrays (8 + 4 bytes per slot, padding included: the port reads
    # them) + 17 vector passes of 8 n bytes (SpMV + 136 n)
    bytes_it = co.n * co.W * 12 + 4 * co.n + 16 * co.n + 136 * co.n
    # second, implementation-independent anchor: single-thread scipy CSR A @ x
    Kcsr = co.to_csr()
    xs = np.random.default_rng(0).standard_normal(co.n)
    Kcsr @ xs
    t = time.perf_counter()
    for _ in range(5):
        Kcsr @ xs
    t_scipy = (time.perf_counter() - t) / 5
    cpu_model = "unknown"
    try:
        for line in open("/proc/cpuinfo"):
            if line.startswith("model name"):
                cpu_model = line.split(":", 1)[1].strip()
                break
    except OSError:
        pass
    numa = len([d for d in os.listdir("/sys/devices/system/node") if d.startswith("node")]) \
        if os.path.isdir("/sys/devices/system/node") else None
    return {"value": it / dt, "unit": "CG iters/s", "cores": int(best), "kind": "port",
            "gbs": bytes_it * it / dt / 1e9,
            "threads_scan_iters_per_s": scan, "container_cpu_quota": quota, "numa_nodes": numa,
            "assemblies_per_s": co.ne / t_asm, "assembly_ms": t_asm * 1e3,
            "cpu_model": cpu_model, "host_threads_available": os.cpu_count(),
            "scipy_csr_spmv_per_s_1thread": 1.0 / t_scipy,
            "sample": f"same {co.ne}-element {etype} mesh and state: 1 as-written assembly ({t_asm:.2f} s) + {it} CG "
                      f"iterations ({dt:.1f} s) of oracle/femcy_oracle.c, OpenMP x{int(best)} threads (best of the scan); setup "
                      f"{setup:.0f} s untimed"}


if __name__ == "__main__":
    main()
