"""Bucket and chunk edges of the one-launch small-system PCG (csrc/kernels_pcg.hip: pcg_small_solve's choice among the 14
instantiations k_pcg_small<DM, K, RR>, and every wave's chunk of a slice against RR), on the machinery of tests/pcg_shapes.py
(Case, layout, mul_ld, pcg_ld, _solve, _check_iterate, check_fit): every check is against the long-double recurrence, never
one run of a kernel against another.  tests/test_small_shapes_cpu.py runs the table on the host backend (references,
conditions, constants), tests/test_gpu_small_shapes.py on the device.

The ABI does not export the instantiation that ran, so the selection is RESTATED here (select()) from PatternInfo's n,
nslices and max_row_blocks, the knob FEMCY_TUNE_SMALL_REG_ROWS and the slice lengths of pcg_shapes.layout:
    declined   n > 48 * 256, more slices than half the CUs (128), or more LDS than the device allows
    K          kneed = ceil(n / 256): 8 up to 8, 24 up to 24, else 48 (entries of r and M per thread)
    RR         share = ceil(max_row_blocks / 4), or the knob when it is >= 0: 0 for share 0 and always for K = 48, 8 up to 8,
               above that 16 (K = 8) or 12 (K = 24) (block rows per wave kept in registers)
    lds        (npad + 4 dm 64 + 8) * 8 bytes with npad = n rounded up to even; above 48 KiB the launch sets the attribute
    chunk      wave w of slice s multiplies block columns j0 = w * ceil(L / 4) .. j1 = min(L, j0 + chunk): the first RR from
               registers (`has` = j0 + jj < j1), the rest streamed in a loop unrolled by 2
Every row is pinned to (dm, n, nslices, max_row_blocks, K, RR, lds) and carries its edge as a predicate over the restatement.
On the device a taken row must move solves_small alone, a declined one solves_three alone, neither barrier_timeouts
(FEMCY_OPT_PCG_PERSIST = 0 throughout, so that a declined system has one place to go).

Meshes (build()): a base -- a strip of CPS3 cells held along both long edges, a clamped C3D4 plate, or pcg_shapes' slivers --
then a STOPPER (a closed fan of 3 triangles with 5 free DOF, or a lone tetrahedron with 6), then at most one FAN
(asm_shapes.fans2d / fans3d) whose hub row has the length the row is about, then loose nodes, which move n in steps of dm
(pcg_shapes._with_loose: the last system DOF stays a coupled one).  Every fan is held at ring nodes only (statically
determinate), so the hub row keeps its blocks.  With the caller's numbering and the default sort window the hub sorts to the
front: slice 0 has the hub's length L while the other slices are ordinary ones, so L differs from workgroup to workgroup under
one global RR.  (No row needed a narrower window; Row.sigma is there for one that does.)
Fit (pcg_shapes.check_fit, every row, host): the 2-D strips are 3 cells across (7 for the two rows at n = 2048 | 2050).  At 15
across, and for 12 288 DOF at 47 across, the float64 oracle's own stop at eps = 1e-10 scatters by 3 .. 19 iterations of
200 .. 680 under a reversal of the unknowns or one rounding of K, more than half of max(2, 2 %); at 47 across its max|r| after
seven iterations is 1e5 r0 and misses max|b - K x| by more than the bound.

Right-hand sides: pcg_shapes' smooth one and e_(n-1), and "edge": 1e3 on both (three) DOFs of the hub of the row's fan, or, in
a row without one, on the first free DOF of the first slice of every distinct length and of the last slice.
The stop: a further right-hand side, "stopper", loads the free DOFs of the stopper and every constrained DOF (unit rows of
K: one eigenvalue of M K), so that the recurrence ends by itself within 7 iterations; eps is chosen from the long-double
recurrence (stop_of()) so that iteration m in 5 .. 7 is the first under eps r0 with a factor of two to spare on both sides.
Its iterates beyond the stop are 0 / 0, so it stays out of the fixed-count checks.  The other three right-hand sides are
used for the stop as well wherever the reference offers such an eps (it seldom does: max|r| does not fall by four in seven
iterations of a plate).

Sensitivity (host): for every chunk row the long-double recurrence is run with the smallest stored off-diagonal block of
the hub's row that the constraints have not zeroed taken out of K; x_1 or x_2 of one of the right-hand sides must move by
more than the device is allowed, or the row could not see a block row that a wave skips.

Measured constants (x86-64 long double; oracle.pcg_reference in float64 against pcg_ld over these rows and their three
right-hand sides on the host backend's matrices; the tests allow 4 x; tests/test_small_shapes_cpu.py measures them again):
    T_ALPHA  worst |x_1 - ref|_i / |ref|_i after one iteration                7.83e-16   5.24e-16
    T_X[2]   worst max|x_2 - ref| / max|ref| after two iterations             3.69e-15   3.13e-15
    T_X[7]   the same after seven (and at the stop, m <= 7)                   5.59e-15   3.65e-15
(last column: the worst value the device tests print, pytest -s, over every row: k24-top-c3d4, hub64-rr16-cps3 twice; the
worst |rmax - max|b - K x|| is 0.10 of its bound, the worst x at a stop 0.006 of its.)  x_1 exceeds pcg_shapes' T_ALPHA = 6.56e-16,
so T_ALPHA is this table's own figure; x_2 and x_7 stay within pcg_shapes' T_X (1.41e-14, 2.85e-14), which are used as they are."""
import collections

import numpy as np

from femcy_amd import backend as be
from oracle import femcy_oracle as orc

import asm_shapes as am
import pcg_shapes as ps

LD = ps.LD
SLICE, BS, WAVES = 64, 256, 4                                      # ctx.hpp, kernels_pcg.hip
KMAX, MAX_WG, MAX_LDS, ATTR_LDS = 48, 128, 160 * 1024, 48 * 1024   # pcg_small_solve; half of 256 CUs; LDS of a gfx950 workgroup
INSTANCES = tuple((dm, K, RR) for dm in (2, 3) for K, RR in ((8, 0), (24, 0), (48, 0), (8, 8), (8, 16), (24, 8), (24, 12)))
MEASURED = (7.83e-16, 3.69e-15, 5.59e-15)                          # float64 against long double over this table (header)
T_ALPHA = MEASURED[0]                                              # above pcg_shapes' 6.56e-16: this table's own
T_X = dict(ps.T_X)                                                 # the rows stay within pcg_shapes' 1.41e-14 / 2.85e-14
MAXITS = ps.MAXITS
STOP_M = (5, 6, 7)
THREE_MAX_N = 2050                                                 # the stop through three launches: rows up to here


# --------------------------------------------------------------------------------------------- the selection, restated
def select(dm, n, nslices, mrb, knob=-1):
    """pcg_small_solve -> (K, RR, dynamic LDS bytes), or None where it declines"""
    npad = (n + 1) & ~1
    lds = (npad + WAVES * dm * 64 + 2 * (BS // 64)) * 8
    if n > KMAX * BS or nslices > MAX_WG or lds + 256 > MAX_LDS:
        return None
    kneed = -(-n // BS)
    share = -(-mrb // WAVES) if knob < 0 else knob
    K = 8 if kneed <= 8 else (24 if kneed <= 24 else 48)
    RR = 0 if share == 0 or K == 48 else (8 if share <= 8 else (16 if K == 8 else 12))
    return K, RR, lds


Chunk = collections.namedtuple("Chunk", "j0 j1 rows reg missing streamed")


def chunks(L, RR):
    """the four waves' shares of a slice of length L: block columns j0 .. j1, `rows` of them (0: an empty chunk), `reg` in
    registers, `missing` register rows without a block (`has` false), `streamed` trips of the loop behind them"""
    c = -(-L // WAVES)
    out = []
    for w in range(WAVES):
        j0 = w * c
        j1 = min(L, j0 + c)
        rows = max(0, j1 - j0)
        out.append(Chunk(j0, j1, rows, min(rows, RR), max(0, RR - rows), max(0, rows - RR)))
    return out


class Restated:
    def __init__(self, row, dm, n, nn, L, node_of):
        self.row, self.dm, self.n, self.nn, self.L, self.node_of = row, dm, n, nn, np.asarray(L), node_of
        self.nslices, self.mrb = len(L), int(np.max(L))
        self.npad, self.kneed = (n + 1) & ~1, -(-n // BS)
        self.share = -(-self.mrb // WAVES) if row.knob < 0 else row.knob
        self.sel = select(dm, n, self.nslices, self.mrb, row.knob)
        self.K, self.RR, self.lds = self.sel or (None, None, None)

    def ch(self, s=0):
        return chunks(int(self.L[s]), self.RR)

    def ordinary(self):
        """slices other than slice 0 that are no loose nodes: the hub's slice is not the only kind"""
        return int((self.L[1:] >= 4).sum())

    def padding(self):
        return int((self.node_of < 0).sum())


# ------------------------------------------------------------------------------------------------------------ meshes
def _fan_cons(dm, base, k):
    """the DOFs that hold one fan of k elements whose first node is `base`: ring nodes only, six (three) DOF"""
    if dm == 2:                                                    # hub, ring 0 .. k-1
        a, b = base + 1, base + 1 + max(1, k // 2)
        if k == 1:                                                 # a lone triangle
            a, b = base, base + 1
        return [a * 2, a * 2 + 1, b * 2 + 1]
    if k == 1:                                                     # a lone tetrahedron
        a, b, c = base, base + 1, base + 2
    else:                                                          # axis 0, axis 1, ring 0 .. k-1
        a, b, c = base + 2, base + 2 + k // 2, base + 2 + max(1, k // 4)
    return [a * 3, a * 3 + 1, a * 3 + 2, b * 3 + 1, b * 3 + 2, c * 3 + 2]


def build(row):
    """-> (nodes, elements, plug-in, material, constrained DOFs); row.base = (pcg_shapes kind, args), row.fan = k or 0"""
    kind, args = row.base
    nodes, el, ELE, mat, cons = ps.build(ps.Row(row.name, kind, args, 0, 0, 0, 0, None, ""))
    dm = nodes.shape[1]
    ks = [3 if dm == 2 else 1] + ([row.fan] if row.fan else [])
    fn, fe = am.fans2d(ks) if dm == 2 else am.fans3d(ks, False)
    nb = len(nodes)
    hubs, at = [], 0
    cons = list(cons)
    for k in ks:
        hubs.append(nb + at)
        cons += _fan_cons(dm, nb + at, k)
        at += (k + 1 if k > 1 else 3) if dm == 2 else (k + 2 if k > 1 else 4)
    assert at == len(fn)
    nodes = np.vstack([nodes, fn + nodes.max(axis=0) + 2.0])
    el = np.vstack([el, fe + nb]).astype(np.int32)
    cons = np.asarray(cons, dtype=np.int64)
    nodes, el, ids = ps._with_loose(nodes, el, row.loose)
    nm = len(nodes) - row.loose
    cons = np.where(cons // dm == nm - 1, (len(nodes) - 1) * dm + cons % dm, cons) if row.loose else cons
    cons = np.concatenate([cons, (ids[:, None] * dm + np.arange(dm)[None, :]).ravel()])
    return nodes, el, ELE, mat, np.unique(cons).astype(np.int32)


def components(row, dm, nb):
    """-> (node numbers of the stopper, the fan's hub or None); nb = nodes of the base"""
    ns = 4
    last = nb + ns + ((row.fan + (1 if dm == 2 else 2)) if row.fan else 0) - 1     # the mesh's last node: traded with a loose one
    stopper = [nb + i for i in range(ns)]
    if row.loose:
        stopper = [a if a != last else last + row.loose for a in stopper]
    return stopper, (nb + ns if row.fan else None)


# --------------------------------------------------------------------------------------------------------- the table
Row = collections.namedtuple("Row", "name base fan loose knob sigma pin group edge why")


def _r(name, base, fan, loose, knob, pin, group, edge, why):
    return Row(name, base, fan, loose, knob, ps.SIGMA, pin, group, edge, why)


S8, S24, SL, S24B, S48 = ("strip", (119, 3)), ("strip", (375, 3)), ("strip", (695, 3)), ("strip", (759, 3)), ("strip", (1527, 3))
S8B = ("strip", (123, 7))
P8, P24, PL, P8B, P24B, P48 = ("C3D4", (5, 5, 15)), ("C3D4", (5, 5, 29)), ("C3D4", (7, 7, 26)), ("C3D4", (5, 5, 17)), \
    ("C3D4", (7, 7, 30)), ("C3D4", (9, 9, 39))


def _hub(T, L, RR):
    return int(T.L[0]) == L == T.mrb and T.RR == RR and T.ordinary() >= 2


def _bucket(K, odd=None, kneed=None):
    return lambda T: T.K == K and (odd is None or T.n % 2 == odd) and (kneed is None or T.kneed == kneed)


# pin = (dm, n, nslices, max_row_blocks, K, RR, lds bytes); K = RR = lds = None: declined
ROWS = [
    # ---- 1. K buckets
    _r("k8-top-cps3", S8B, 0, 28, -1, (2, 2048, 16, 7, 8, 8, 20544), "bucket", _bucket(8, 0, 8),
       "n = 2048 = 8 * 256: the last thread's last entry is the last DOF, K = 8"),
    _r("k24-bottom-cps3", S8B, 0, 29, -1, (2, 2050, 17, 7, 24, 8, 20560), "bucket", _bucket(24, 0, 9),
       "n = 2050: kneed = 9, the first system of K = 24; 1025 nodes, a last slice of one node and 63 padding lanes"),
    _r("k24-top-cps3", S24B, 0, 28, -1, (2, 6144, 48, 7, 24, 8, 53312), "bucket", lambda T: T.K == 24 and T.kneed == 24 and T.lds > ATTR_LDS,
       "n = 6144 = 24 * 256, K = 24 at its ceiling (above 48 KiB of LDS)"),
    _r("k48-bottom-cps3", S24B, 0, 29, -1, (2, 6146, 49, 7, 48, 0, 53328), "bucket", lambda T: T.K == 48 and T.kneed == 25 and T.RR == 0 and T.share > 0,
       "n = 6146: kneed = 25, the first system of K = 48, which keeps no block row in registers whatever the share"),
    _r("k48-top-cps3", S48, 0, 28, -1, (2, 12288, 96, 7, 48, 0, 102464), "bucket", lambda T: T.K == 48 and T.kneed == 48 and T.nslices == 96,
       "n = 12288 = 48 * 256: the largest system the kernel takes, 96 workgroups"),
    _r("above-k48-cps3", S48, 0, 29, -1, (2, 12290, 97, 7, None, None, None), "bucket", lambda T: T.sel is None and T.nslices <= MAX_WG,
       "n = 12290: declined by its size alone (97 slices would fit)"),
    _r("k8-top-c3d4", P8B, 0, 30, -1, (3, 2046, 11, 15, 8, 8, 22576), "bucket", _bucket(8, 0, 8),
       "n = 2046, the last multiple of 3 up to 2048: threads 254 and 255 clamp their last entry to n - 1"),
    _r("k24-bottom-c3d4", P8B, 0, 31, -1, (3, 2049, 11, 15, 24, 8, 22608), "bucket", _bucket(24, 1, 9),
       "n = 2049 odd: npad = n + 1, kneed = 9, of 24 entries per thread 15 and more are clamped"),
    _r("k24-top-c3d4", P24B, 0, 60, -1, (3, 6144, 32, 15, 24, 8, 55360), "bucket", lambda T: T.K == 24 and T.kneed == 24 and T.padding() == 0,
       "n = 6144 at dm = 3: 2048 nodes, no padding lane, no clamped entry"),
    _r("k48-bottom-c3d4", P24B, 0, 61, -1, (3, 6147, 33, 15, 48, 0, 55392), "bucket", lambda T: T.K == 48 and T.n % 2 == 1 and T.kneed == 25,
       "n = 6147 odd: the first system of K = 48; a last slice of one node"),
    _r("k48-top-c3d4", P48, 0, 92, -1, (3, 12288, 64, 15, 48, 0, 104512), "bucket", lambda T: T.K == 48 and T.kneed == 48 and T.nslices == 64,
       "n = 12288 at dm = 3: 64 workgroups, 102 KiB of LDS, the most the kernel ever asks for"),
    _r("above-k48-c3d4", P48, 0, 93, -1, (3, 12291, 65, 15, None, None, None), "bucket", lambda T: T.sel is None,
       "n = 12291: declined"),
    # ---- 2. the share boundary (and chunk == RR, every wave short)
    _r("hub32-k8-cps3", S8, 31, 6, -1, (2, 1044, 9, 32, 8, 8, 12512), "share",
       lambda T: _hub(T, 32, 8) and T.share == 8 and all(c.rows == 8 and c.streamed == 0 for c in T.ch()),
       "a hub row of 32 blocks: share 8, the last of RR = 8; every wave's chunk is exactly RR, no streamed trip"),
    _r("hub33-k8-cps3", S8, 32, 6, -1, (2, 1046, 9, 33, 8, 16, 12528), "share",
       lambda T: _hub(T, 33, 16) and T.share == 9 and all(0 < c.rows < 16 for c in T.ch()),
       "33 blocks: share 9, RR = 16; chunks of 9, 9, 9 and 6: every wave is short of RR"),
    _r("hub32-k24-cps3", S24, 31, 6, -1, (2, 3092, 25, 32, 24, 8, 28896), "share", lambda T: _hub(T, 32, 8) and T.K == 24,
       "the same hub of 32 in the K = 24 bucket"),
    _r("hub33-k24-cps3", S24, 32, 6, -1, (2, 3094, 25, 33, 24, 12, 28912), "share",
       lambda T: _hub(T, 33, 12) and T.K == 24 and all(0 < c.rows < 12 for c in T.ch()),
       "33 blocks in the K = 24 bucket: RR = 12, every wave short"),
    _r("hub32-k8-c3d4", P8, 30, 6, -1, (3, 1854, 10, 32, 8, 8, 21040), "share", lambda T: _hub(T, 32, 8) and T.K == 8,
       "a fan of 30 tetrahedra: axis rows of 32 blocks, 3 x 3 blocks (the odd ninth entry of a block comes by its own load)"),
    _r("hub33-k8-c3d4", P8, 31, 6, -1, (3, 1857, 10, 33, 8, 16, 21072), "share", lambda T: _hub(T, 33, 16) and T.n % 2 == 1,
       "31 tetrahedra: 33 blocks, RR = 16; n odd in the K = 8 bucket"),
    _r("hub32-k24-c3d4", P24, 30, 6, -1, (3, 3366, 18, 32, 24, 8, 33136), "share", lambda T: _hub(T, 32, 8) and T.K == 24, "(24, 8) at dm = 3"),
    _r("hub33-k24-c3d4", P24, 31, 6, -1, (3, 3369, 18, 33, 24, 12, 33168), "share", lambda T: _hub(T, 33, 12) and T.K == 24, "(24, 12) at dm = 3"),
    _r("knob0-k8-cps3", S8, 32, 6, 0, (2, 1046, 9, 33, 8, 0, 12528), "share", lambda T: T.share == 0 and (T.K, T.RR) == (8, 0) and T.ch()[0].streamed == 9,
       "knob 0: (8, 0), every block row streamed: trips of 9, 9, 9 and 6"),
    _r("knob0-k24-cps3", S24, 32, 6, 0, (2, 3094, 25, 33, 24, 0, 28912), "share", lambda T: (T.K, T.RR) == (24, 0), "knob 0: (24, 0)"),
    _r("knob0-k8-c3d4", P8, 31, 6, 0, (3, 1857, 10, 33, 8, 0, 21072), "share", lambda T: (T.K, T.RR) == (8, 0), "knob 0: (8, 0) at dm = 3"),
    _r("knob0-k24-c3d4", P24, 31, 6, 0, (3, 3369, 18, 33, 24, 0, 33168), "share", lambda T: (T.K, T.RR) == (24, 0), "knob 0: (24, 0) at dm = 3"),
    # ---- 3. the LDS attribute
    _r("lds-below-cps3", SL, 0, 24, -1, (2, 5624, 44, 7, 24, 8, 49152), "lds", lambda T: T.K == 24 and T.lds == ATTR_LDS,
       "exactly 48 KiB of dynamic LDS: the last launch without the attribute"),
    _r("lds-above-cps3", SL, 0, 25, -1, (2, 5626, 44, 7, 24, 8, 49168), "lds", lambda T: T.K == 24 and T.lds == ATTR_LDS + 16,
       "16 bytes more: the first K = 24 launch that sets hipFuncAttributeMaxDynamicSharedMemorySize"),
    _r("lds-below-c3d4", PL, 0, 57, -1, (3, 5367, 28, 15, 24, 8, 49152), "lds", lambda T: T.K == 24 and T.lds == ATTR_LDS and T.n % 2 == 1,
       "n = 5367 odd: npad = 5368 lands on 48 KiB exactly"),
    _r("lds-above-c3d4", PL, 0, 58, -1, (3, 5370, 28, 15, 24, 8, 49168), "lds", lambda T: T.K == 24 and T.lds == ATTR_LDS + 16, "one node more: above"),
    # ---- 4. chunk against RR
    _r("empty-chunks-cps3", ("sliver", (40, 30)), 0, 66, -1, (2, 484, 4, 5, 8, 8, 8032), "chunk",
       lambda T: T.L.tolist() == [5, 5, 3, 1] and T.RR == 8 and [c.rows for c in T.ch(0)] == [2, 2, 1, 0] and T.ch(0)[3].j0 > 5
       and [c.rows for c in T.ch(2)] == [1, 1, 1, 0] and [c.rows for c in T.ch(3)] == [1, 0, 0, 0] and T.ch(3)[2].j0 > 1,
       "slices of L = 5, 5, 3 and 1: waves with an empty chunk, j0 == L and j0 > L; every register row but one or two without a block"),
    _r("hub29-rr8-cps3", S8, 28, 6, -1, (2, 1038, 9, 29, 8, 8, 12464), "chunk",
       lambda T: _hub(T, 29, 8) and [c.missing for c in T.ch()] == [0, 0, 0, 3] and T.padding() > 0,
       "L = 29: chunks of 8, 8, 8 and 5, `has` false for three register rows of the last wave; the last slice has padding lanes "
       "behind nn (node_of = -1)"),
    _r("hub33-rr8-cps3", S8, 32, 6, 8, (2, 1046, 9, 33, 8, 8, 12528), "chunk",
       lambda T: _hub(T, 33, 8) and [c.streamed for c in T.ch()] == [1, 1, 1, 0] and T.ch()[3].missing == 2,
       "L = 33 under knob 8: one streamed trip (the odd trip of the loop unrolled by 2) behind full registers, the last wave short"),
    _r("hub36-rr8-cps3", S8, 35, 6, 8, (2, 1052, 9, 36, 8, 8, 12576), "chunk",
       lambda T: _hub(T, 36, 8) and [c.streamed for c in T.ch()] == [1, 1, 1, 1],
       "L = 36 under knob 8: every wave streams exactly one block row"),
    _r("hub40-rr8-cps3", S8, 39, 6, 8, (2, 1060, 9, 40, 8, 8, 12640), "chunk",
       lambda T: _hub(T, 40, 8) and [c.streamed for c in T.ch()] == [2, 2, 2, 2],
       "L = 40 under knob 8: two streamed trips, the even parity of the unrolled loop (L = 36 gives ceil(36 / 4) - 8 = 1 as 33 does)"),
    _r("hub48-rr12-cps3", S24, 47, 6, -1, (2, 3124, 25, 48, 24, 12, 29152), "chunk",
       lambda T: _hub(T, 48, 12) and all(c.rows == 12 and c.streamed == 0 for c in T.ch()), "L = 48: chunk == RR = 12"),
    _r("hub64-rr16-cps3", S8, 63, 6, -1, (2, 1108, 9, 64, 8, 16, 13024), "chunk",
       lambda T: _hub(T, 64, 16) and all(c.rows == 16 and c.streamed == 0 for c in T.ch()), "L = 64: chunk == RR = 16"),
    _r("hub65-rr16-cps3", S8, 64, 6, -1, (2, 1110, 9, 65, 8, 16, 13040), "chunk",
       lambda T: _hub(T, 65, 16) and [c.streamed for c in T.ch()] == [1, 1, 1, 0] and T.ch()[3].missing == 2,
       "L = 65: one streamed trip behind 16 register rows, the last wave short by two"),
    _r("hub29-rr8-c3d4", P8, 27, 6, -1, (3, 1845, 10, 29, 8, 8, 20976), "chunk", lambda T: _hub(T, 29, 8) and T.ch()[3].missing == 3,
       "L = 29 at dm = 3"),
    _r("hub36-rr8-c3d4", P8, 34, 6, 8, (3, 1866, 10, 36, 8, 8, 21136), "chunk", lambda T: _hub(T, 36, 8) and [c.streamed for c in T.ch()] == [1] * 4,
       "L = 36 under knob 8 at dm = 3: the streamed loop's own ninth-entry load, one trip"),
    _r("hub48-rr12-c3d4", P24, 46, 6, -1, (3, 3414, 18, 48, 24, 12, 33520), "chunk", lambda T: _hub(T, 48, 12) and T.ch()[0].streamed == 0,
       "L = 48 at dm = 3: chunk == RR = 12"),
    _r("hub65-rr16-c3d4", P8, 63, 6, -1, (3, 1953, 11, 65, 8, 16, 21840), "chunk", lambda T: _hub(T, 65, 16) and T.ch()[0].streamed == 1 and T.n % 2 == 1,
       "L = 65 at dm = 3, n odd"),
]
BY_NAME = {r.name: r for r in ROWS}


def row_id(row):
    return row.name


# --------------------------------------------------------------------------------------------------------------- cases
def residuals_ld(K, b, xs):
    """max|b - K x_k| of the iterates, in long double"""
    return [float(np.abs(b.astype(LD) - ps.mul_ld(K, x)).max()) for x in xs]


def stop_of(r0, rmax):
    """(m, eps) with m in 5 .. 7 the first iterate under eps r0, a factor of two clear on both sides: min_(k<m) rmax_k >=
    2 eps r0 and rmax_m <= eps r0 / 2; None where the recurrence offers none.  eps sits four decades under the upper end
    where the interval is that wide (a recurrence that ends by itself), else in its geometric middle."""
    for m in STOP_M:
        lo, hi = 2.0 * rmax[m - 1] / r0, min(rmax[:m - 1]) / (2.0 * r0)
        if lo <= hi:
            eps = 1.0e-4 * hi if lo <= 1.0e-4 * hi else float(np.sqrt(lo * hi))
            assert min(rmax[:m - 1]) >= 2.0 * eps * r0 and rmax[m - 1] <= eps * r0 / 2.0
            return m, eps
    return None


class SCase(ps.Case):
    """pcg_shapes.Case on this table's meshes, with the restatement, the "edge" right-hand side in the place of "starts", and
    the stop of every right-hand side that offers one"""
    mesh = staticmethod(build)

    def __init__(self, row, backend):
        super().__init__(row, backend)
        self.T = Restated(row, self.dm, self.n, self.nn, self.L, self.node_of)
        b = np.zeros(self.n)
        free = self.free()
        stopper, _ = components(row, self.dm, self.nb)
        dofs = np.array([a * self.dm + r for a in stopper for r in range(self.dm)])
        dofs = dofs[free[dofs]]
        b[dofs] = 1.0e3 * np.cos(1.0 + 2.0 * np.arange(len(dofs)))
        b[self.cons] = 250.0
        self.stop_b = {"stopper": b, **self.bs}
        self.stops = {}
        for key, v in self.stop_b.items():
            xs = self.xref[key] if key in self.xref else ps.pcg_ld(self.K, v, max(STOP_M))
            got = stop_of(float(np.abs(v).max()), residuals_ld(self.K, v, xs))
            if got:
                self.stops[key] = (got[0], got[1], xs[got[0] - 1])

    def free(self):
        free = np.ones(self.n, dtype=bool)
        free[self.cons] = False
        return free

    @property
    def nb(self):
        kind, args = self.row.base
        if kind == "strip":
            return (args[0] + 1) * (args[1] + 1)
        if kind == "sliver":
            return 3 * args[1] + 2 * (args[0] + 1)
        return (args[0] + 1) * (args[1] + 1) * (args[2] + 1)

    def edge_nodes(self):
        """the hub of the row's fan; without one, the first node of the first slice of every length and of the last slice"""
        hub = components(self.row, self.dm, self.nb)[1]
        if hub is not None:
            return [hub]
        first = [int(np.nonzero(self.L == v)[0][0]) for v in sorted(set(self.L.tolist()), reverse=True)] + [len(self.L) - 1]
        return [int(self.node_of[s * SLICE]) for s in dict.fromkeys(first)]

    def _rhs(self, nodes):
        bs = super()._rhs(nodes)
        del bs["starts"]
        free, edge = self.free(), np.zeros(self.n)
        for a in self.edge_nodes():
            dofs = a * self.dm + np.arange(self.dm)
            if self.row.fan:
                edge[dofs] = 1.0e3
            else:
                behind = np.nonzero(free[dofs[0]:])[0]
                edge[dofs[0] + (behind[0] if len(behind) else 0)] = 1.0e3
        bs["edge"] = edge
        return bs


for _row in ROWS:                                                  # (pcg_shapes.case finds a row by its name alone, across the tables)
    assert _row.name not in ps.TABLES and all(_row.name != r.name for r in ps.ROWS), "row name taken by another table: " + _row.name
    ps.TABLES[_row.name] = (_row, SCase)


def case(name, backend):
    return ps.case(name, backend)


def _apply(c):
    c.ctx.set_option(be.OPT_PCG_SMALL, 1)
    c.ctx.set_option(be.OPT_PCG_PERSIST, 0)
    c.ctx.set_option(be.TUNE_SMALL_REG_ROWS, c.row.knob)


def _reset(c):
    c.ctx.set_option(be.TUNE_SMALL_REG_ROWS, -1)
    ps._reset(c.ctx)


def _counted(c, out, what, three=False):
    if c.backend == "hip":
        small = c.T.sel is not None and not three
        want = {"solves_three": 0 if small else 1, "solves_small": 1 if small else 0, "solves_persist": 0, "barrier_timeouts": 0}
        assert out[4] == want, (what, out[4], want)
    return out


# -------------------------------------------------------------------------------------------------------------- checks
def check_table(name, backend):
    """the pins against the library's PatternInfo and against the restatement; the row's predicate"""
    c = case(name, backend)
    row, info, T = c.row, c.ctx.pattern_info(), c.T
    dm, n, nslices, mrb, K, RR, lds = row.pin
    assert (c.dm, info.n, info.nslices) == (dm, n, nslices), (c.dm, info.n, info.nslices, row.pin)
    assert (T.n, T.nslices, T.mrb) == (n, nslices, mrb), (T.n, T.nslices, T.mrb, row.pin)
    if backend == "hip":                                           # (the host library keeps block-CSR and no slices)
        assert info.max_row_blocks == mrb, (info.max_row_blocks, mrb)
    assert (T.K, T.RR, T.lds) == (K, RR, lds), (T.sel, row.pin)
    assert row.edge(T), (row.name, row.why, T.sel, T.L[:4], T.ch() if T.sel else None)
    assert c.free()[n - 1], "the last DOF of the system must be a coupled one"
    if T.sel:
        assert T.lds + 256 <= MAX_LDS and (dm, K, RR) in INSTANCES
        for s in range(nslices):                                    # the chunks of every slice tile it
            ch = chunks(int(T.L[s]), RR)
            assert sum(x.rows for x in ch) == T.L[s] and all(x.reg + x.streamed == x.rows and x.reg + x.missing == RR for x in ch)
    print(f"{name} [{backend}]: n {n}, {nslices} slices, longest row {mrb}, knob {row.knob} -> (K, RR) = ({K}, {RR}), LDS {lds} B")
    return T


def check_iterates(name, backend):
    """x after 1, 2 and 7 iterations (eps = 0) of the three right-hand sides against the long-double recurrence, r0 and max|r|
    as pcg_shapes._check_iterate has them, x downloaded into NaN (pcg_shapes._solve).  -> worst deviations"""
    c = case(name, backend)
    worst = {}
    try:
        _apply(c)
        for key in c.bs:
            for m in MAXITS:
                out = _counted(c, ps._solve(c, c.bs[key], m), (name, key, m))
                ps._check_iterate(c, key, m, out, (name, c.T.sel, key, m), worst, T_ALPHA, T_X)
    finally:
        _reset(c)
    shares = {m: round(worst[m] / (4.0 * (T_ALPHA if m == 1 else T_X[m])), 3) for m in MAXITS}
    print(f"{name} [{backend}]: (K, RR) = ({c.T.K}, {c.T.RR}), LDS {c.T.lds} B, worst deviation {worst}, shares of the bounds "
          f"{shares}, rmax {worst['rmax']:.3f}")
    return worst


def check_stop(name, backend, poll=None):
    """every right-hand side with a stop: the device reports iters == m exactly, x is x_m within the bound of seven iterations
    (m <= 7) and max|r| < eps r0.  poll: the same through the three-launch loop with that FEMCY_OPT_PCG_POLL -- the x
    returned is the iterate of the reported count, however many iterations a burst ran past it.  -> worst share of the bound"""
    c = case(name, backend)
    assert c.stops, "no right-hand side of %s offers a stop in 5 .. 7 iterations" % name
    worst = 0.0
    try:
        _apply(c)
        if poll is not None:
            c.ctx.set_option(be.OPT_PCG_SMALL, 0)
            c.ctx.set_option(be.OPT_PCG_POLL, poll)
        for key, (m, eps, xm) in c.stops.items():
            b = c.stop_b[key]
            it, r0, rmax, x, _ = _counted(c, ps._solve(c, b, 50, eps), (name, key, "stop"), three=poll is not None)
            assert it == m, (name, key, "stopped after", it, "not", m, "eps", eps)
            assert r0 == np.abs(b).max() and rmax < eps * r0, (name, key, r0, rmax, eps * r0)
            dev = float(np.abs(x.astype(LD) - xm).max() / np.abs(xm).max())
            worst = max(worst, dev / (4.0 * T_X[7]))
            assert dev <= 4.0 * T_X[7], (name, key, m, dev)
    finally:
        _reset(c)
    print(f"{name} [{backend}] poll {poll}: stops {[(k, v[0], float('%.2e' % v[1])) for k, v in c.stops.items()]}, worst share "
          f"of the bound {worst:.3f}")
    return worst


def check_sensitivity(name, backend="cpu"):
    """a condition on the row: with one block of the hub's row missing from K the long-double x_1 or x_2 moves by more than
    the device is allowed.  -> the largest movement as a multiple of the bound"""
    c = case(name, backend)
    a = c.edge_nodes()[0]
    dm, K = c.dm, c.K
    rows = a * dm + np.arange(dm)
    blocks = {}
    for r in rows:
        for p in range(K.indptr[r], K.indptr[r + 1]):
            col = int(K.indices[p]) // dm
            blocks[col] = max(blocks.get(col, 0.0), abs(K.data[p]))
    cands = [(v, col) for col, v in blocks.items() if col != a and v > 0.0]
    assert cands, (name, "the hub's row has no off-diagonal block left")
    drop = min(cands)[1]
    Kd = K.copy()
    for r in rows:
        sl = slice(Kd.indptr[r], Kd.indptr[r + 1])
        Kd.data[sl] = np.where(Kd.indices[sl] // dm == drop, 0.0, Kd.data[sl])
    seen = 0.0
    for key, b in c.bs.items():
        xs = ps.pcg_ld(Kd, b, 2)
        ref = c.xref[key]
        nz = ref[0] != 0
        seen = max(seen, float((np.abs(xs[0][nz] - ref[0][nz]) / np.abs(ref[0][nz])).max()) / (4.0 * T_ALPHA),
                   float(np.abs(xs[1] - ref[1]).max() / np.abs(ref[1]).max()) / (4.0 * T_X[2]))
    print(f"{name}: without block ({a}, {drop}) of the hub's row x_1 / x_2 move by {seen:.3g} x the bound")
    assert seen > 1.0, (name, a, drop, seen)
    return seen


def measure_constants(backend="cpu", rows=None):
    _, t = ps.measure_constants(backend, rows or ROWS)
    return t


def stop_on_the_oracle(name, backend="cpu"):
    """the float64 oracle at the chosen eps: the same count and x_m within the unmultiplied constant"""
    c = case(name, backend)
    for key, (m, eps, xm) in c.stops.items():
        x, it, _, rmax = orc.pcg_reference(c.K, c.stop_b[key], eps=eps, maxit=50)
        assert it == m, (name, key, it, m)
        assert float(np.abs(x.astype(LD) - xm).max() / np.abs(xm).max()) <= T_X[7], (name, key)
    return sorted(c.stops)
