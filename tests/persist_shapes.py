"""Slices-per-wave and residency edges of the persistent one-launch PCG (csrc/kernels_pcg_persist.hip: persist_shape,
pcg_persist_solve's hand-out of slices to waves, k_pcg_persist), on the machinery of tests/pcg_shapes.py (Case, mul_ld, pcg_ld,
_solve, _check_iterate, check_fit): every check is against the long-double recurrence, never one kernel against another.

ROWS holds one small mesh per edge, with the grid G (FEMCY_TUNE_PERSIST_WGS = 8, 16 or 24) at which it runs, so that every
instantiation of the launch ladder is reached below 45 000 DOF and 260 slices.  A row is pinned to (n, nslices, stored_blocks)
and to its (per_wave, SPW, RJ), and carries its edge as a predicate over the RESTATEMENT of what the ABI does not export:
    shape_of      persist_shape: waves per XCD nwx = G / 8 * 4, per_wave = ceil(longest range / nwx), the ladder
                  3 x 3 blocks SPW 3 (RJ = option 105), 4 (3), 5 / 6 (1), 7 (0), declined above; 2 x 2 blocks SPW 3 / 4 (5),
                  6 (3), 8 (2), declined above 8; lds_rows = min(option 104, SPW * max_row_blocks)
    assign_of     inside each of the 8 ranges the slices go by decreasing length (stable) to the wave with the least block rows
                  so far that still has a free slot; tagged-granule variants (bit 1 of the variant) start wave 0 of every
                  workgroup with CH = 4 rows
    residency_of  per wave and slot t: jl = min(RJ, L) rows in registers, LDS rows handed out from the last slot backwards
                  until lds_rows are spent, the rest streamed; npf = min(CH, streamed rows of slot 0) prefetched, 0 for wave 0
                  of a tagged-granule variant, under option 106 = 16 and for <3, 7, 0>
The restatement is pinned to the library by the counts, by taken | declined at the per_wave ceilings (solves_persist /
solves_three) and by femcy_persist_streamed_bytes, which equals the restated streamed rows x (DD * 8 + 4) * 64 where every
wave's LDS fills and is below it elsewhere.  (The library answers 0 bytes below one slice per workgroup: empty-waves-c3d4 and
empty-ranges-c3d4 are pinned by their counts and by solves_persist alone.)

Shape -> rows (every one under option 105 = 0 and on, option 106 = 16, and the variants the build carries):
    <3,3,{0,4,5}>  spw3-c3d4, long-c3d10, loose-rj4-c3d4, empty-waves-c3d4, empty-ranges-c3d4      (variants 6, 14, 0)
    <3,4,{0,3}>    spw4-c3d4, loose-rj3-c3d4 (G = 24)                                             (variants 6, 14, 0)
    <3,5,{0,1}>    spw5-c3d4      <3,6,{0,1}>  spw6-c3d4      <3,7,0>  spw7-c3d4, spw7-c3d8       (variant 6; 14 and 0 refused)
    <2,3,{0,5}>    spw3-cps3, slivers-rj5-cps3     <2,4,{0,5}>  spw4-cps3 (G = 16)                 (variants 6, 14, 0)
    <2,6,{0,3}>    spw6-cps3 (per_wave 6), spw6-cpe8 (per_wave 5), slivers-rj3-cps3                (variants 6, 14, 0)
    <2,8,{0,2}>    spw8-pw7-cps3 (per_wave 7), spw8-pw8-cps3 (per_wave 8)                          (variants 6, 14, 0)
    declined       declined-c3d4 (per_wave 8), declined-cps3 (per_wave 9): three launches, no barrier time-out

Measured constants (x86-64 long double; oracle.pcg_reference in float64 against pcg_ld over these rows and the four right-hand
sides on the host backend's matrices; the tests allow 4 x; tests/test_persist_shapes_cpu.py measures them again):
    T_ALPHA  worst |x_1 - ref|_i / |ref|_i after one iteration                6.12e-16   5.64e-16
    T_X[2]   worst max|x_2 - ref| / max|ref| after two iterations             6.98e-15   9.30e-15
    T_X[7]   the same after seven                                             9.14e-15   1.18e-14
(last column: the worst value the device tests print, pytest -s, over every row and configuration; the worst
|rmax - max|b - K x|| is 0.55 of its bound.)  Worst share of the 4 x bound per shape on the device (x_1 / x_2 / x_7 / rmax):
    <3,3,*> 0.22 0.03 0.04 0.31 (long-c3d10, empty-ranges-c3d4)   <3,4,*> 0.20 0.01 0.01 0.06   <3,5,*> 0.15 0.01 0.01 0.05
    <3,6,*> 0.18 0.01 0.01 0.06   <3,7,0> 0.20 0.02 0.02 0.05   <2,3,*> 0.16 0.07 0.14 0.50   <2,4,*> 0.13 0.08 0.08 0.45
    <2,6,*> 0.23 0.33 0.32 0.55 (spw6-cps3)   <2,8,*> 0.18 0.24 0.23 0.45   three launches (declined) 0.19 0.25 0.24 0.40

That the table bites, measured with three arithmetic-only mutations of k_pcg_persist (scratch builds, never committed), each
against this table (247 tests), the persist path of pcg_shapes' table (14) and test_persistent_pcg_residency_variants_agree (5):
    the last row of a short LDS batch not multiplied (u < nb - 1)       170 fail here (every taken row)   old table 10   variants 5
    register row RJ - 1 of slot SPW - 1 left out of the sum            88 fail here (every row that fills slot SPW - 1 with
                                                                        RJ > 0)                           old table 0    variants 0
    the last row of a partial prefetched batch not added (npf 1 .. 3)   51 fail here (the rows with npf in 1 .. 3: spw3 / spw4 /
                                                                        spw6-cps3, loose-rj4, empty-*, slivers)   old table 9   variants 5

The 2-D rows are strips of square CPS3 cells (and the CPE8 beam) HELD ALONG BOTH LONG EDGES (pcg_shapes.build: "strip",
"held-beam").  A plate of this many nodes held at one short edge does not fit the checks: a smooth load lifts max|r| to
100 r0 in the first iterations, the float64 oracle's own max|r| is then two roundings of that away from max|b - K x|
(pcg_shapes.check_fit), and float64 PCG stops with max|b - K x| = 1.7e-9 .. 7.7e-9 r0 against the bound of 1.2e-9 r0.
UNFIT names the rows pcg_shapes.check_fit leaves out of the stopping check, 4 of 21: the C3D10 plate (the oracle's x_1
residual) and the three largest strips, where the oracle's own iteration count at eps = 1e-10 scatters by 8 .. 10 of 300
under a reversal of the unknowns or one rounding of K -- more than half of max(2, 2 %)."""
import collections

import numpy as np

from femcy_amd import backend as be
from oracle import femcy_oracle as orc

import pcg_shapes as ps

LD = ps.LD
PNX, CH, SLICE = 8, 4, 64                                          # kernels_pcg_persist.hip
MAX_LDS = 160 * 1024                                               # LDS a workgroup may allocate on gfx950
T_ALPHA = 6.12e-16
T_X = {2: 6.98e-15, 7: 9.14e-15}
MAXITS = ps.MAXITS
EPS_STOP = ps.EPS_STOP
OPT_LDS, OPT_RJ, OPT_DBG, OPT_WGS = 104, 105, 106, 107             # include/femcy.h: FEMCY_TUNE_PERSIST_*
GRIDS = (8, 16, 24)
MAX_SLICES, MAX_DOF = 260, 45000
# rows pcg_shapes.check_fit leaves out of the stopping check (header)
UNFIT = ("long-c3d10", "spw8-pw7-cps3", "spw8-pw8-cps3", "declined-cps3")

Shape = collections.namedtuple("Shape", "SPW RJ lds_rows per_wave nwx")
Res = collections.namedtuple("Res", "sl L jl je lds streamed npf fills")


# ------------------------------------------------------------------------------------------------- the launch, restated
def ranges_of(L):
    return ps.split_of(L, 2, 0).start


def shape_of(L, dm, G, rj_opt=4, lds_opt=-1, max_row_blocks=None, max_lds=MAX_LDS):
    """persist_shape -> Shape, or None when the ladder declines the pattern"""
    nwx = G // PNX * 4
    per_wave = -(-int(np.diff(ranges_of(L)).max()) // nwx)
    on = rj_opt != 0
    if dm == 3:
        if per_wave > 7:
            return None
        spw = max(per_wave, 3)
        rj = rj_opt if spw == 3 else (0 if not on else (3 if spw == 4 else (0 if spw == 7 else 1)))
    else:
        if per_wave > 8:
            return None
        spw = 8 if per_wave > 6 else (6 if per_wave > 4 else (4 if per_wave > 3 else 3))
        rj = 0 if not on else (2 if spw == 8 else (3 if spw == 6 else 5))
    rows = (max_lds - 2048) // (4 * 64 * (dm * dm * 8 + 4)) if lds_opt < 0 else lds_opt
    mrb = int(L.max()) if max_row_blocks is None else max_row_blocks
    return Shape(spw, rj, max(0, min(rows, spw * mrb)), per_wave, nwx)


def assign_of(L, G, spw, a2a):
    """-> [8][nwx][SPW] slices of every wave, -1 = none"""
    nwx = G // PNX * 4
    start = ranges_of(L)
    out = -np.ones((PNX, nwx, spw), dtype=np.int64)
    for k in range(PNX):
        order = np.arange(start[k], start[k + 1])
        order = order[np.argsort(-L[order], kind="stable")]
        load = [CH if (a2a and w % 4 == 0) else 0 for w in range(nwx)]
        cnt = [0] * nwx
        for s in order:
            best = -1
            for w in range(nwx):
                if cnt[w] < spw and (best < 0 or load[w] < load[best]):
                    best = w
            out[k, best, cnt[best]] = s
            cnt[best] += 1
            load[best] += int(L[s])
    return out


def residency_of(L, assign, sh, dm, a2a=True, noprefetch=False):
    """-> per [range][wave][slot]: slice, its length, jl, je, LDS rows, streamed rows; per wave: npf, LDS full"""
    Lw = np.where(assign >= 0, L[np.maximum(assign, 0)], 0)
    jl = np.minimum(sh.RJ, Lw)
    je = jl.copy()
    for k in range(assign.shape[0]):
        for w in range(assign.shape[1]):
            qn = 0
            for t in range(sh.SPW - 1, -1, -1):
                nl = max(0, min(Lw[k, w, t] - jl[k, w, t], sh.lds_rows - qn))
                je[k, w, t] = jl[k, w, t] + nl
                qn += nl
    lds, streamed = je - jl, Lw - je
    npf = np.minimum(CH, streamed[:, :, 0])
    if noprefetch or (dm == 3 and sh.SPW >= 7):
        npf[:] = 0
    if a2a:
        npf[:, 0::4] = 0
    return Res(assign, Lw, jl, je, lds, streamed, npf, lds.sum(axis=2) == sh.lds_rows)


Config = collections.namedtuple("Config", "variant rj lds dbg l2")


class Restated:
    """the restatement of one row; sh() / res() take a Config (default: the row's base configuration)"""

    def __init__(self, row, L, dm):
        self.row, self.L, self.dm = row, np.asarray(L), dm
        self.lens = np.diff(ranges_of(self.L))

    def sh(self, cfg=None, G=None):
        cfg = cfg or base(self.row)
        return shape_of(self.L, self.dm, G or self.row.G, cfg.rj, cfg.lds)

    def res(self, cfg=None, G=None):
        cfg = cfg or base(self.row)
        sh = self.sh(cfg, G)
        a2a = ((6 if cfg.variant < 0 else cfg.variant) & 2) != 0
        return residency_of(self.L, assign_of(self.L, G or self.row.G, sh.SPW, a2a), sh, self.dm, a2a, cfg.dbg == 16)

    def streamed_rows(self, cfg=None):
        return int(self.res(cfg).streamed.sum())

    def occupied(self, cfg=None):
        """slots in use per wave [8][nwx]"""
        return (self.res(cfg).sl >= 0).sum(axis=2)


# ------------------------------------------------------------------------------------------------------------ the table
Row = collections.namedtuple("Row", "name kind args loose G n nslices stored shape lds edge why")


def _r(name, kind, args, loose, G, n, nslices, stored, shape, lds, edge, why):
    return Row(name, kind, args, loose, G, n, nslices, stored, shape, lds, edge, why)


def _real(T):
    return T.L.min() >= 5


def _short_next_to_full(T):
    occ, spw = T.occupied(), T.sh().SPW
    return any(0 < occ[k].min() < spw and occ[k].max() == spw for k in range(PNX)) or \
        any(0 < o < spw for o in occ.ravel()) and (occ == spw).any()


# shape = (per_wave, SPW, RJ) at the row's G under the defaults, None = declined; lds = the option 104 values the row runs
# (the first is the base configuration's: a middle value chosen from the restatement)
ROWS = [
    _r("spw3-c3d4", "C3D4", (9, 9, 51), 0, 8, 15600, 82, 69760, (3, 3, 4), (5, 0, 1, 8),
       lambda T: _real(T) and (T.res().npf == 4).any() and (T.res().npf[:, 0] == 0).all()
       and ((T.res().lds > 0) & (T.res().streamed > 0)).any(),
       "three slices of 7 .. 15 rows per wave: the LDS budget of 5 ends inside a slice, slot 0 streams a prefetched batch of 4; "
       "wave 0 of every workgroup prefetches nothing"),
    _r("spw4-c3d4", "C3D4", (10, 10, 55), 0, 8, 20328, 106, 91520, (4, 4, 3), (8, 0, 1, 4),
       lambda T: _real(T) and T.lens.max() == 16 and T.lens.min() == 12 and _short_next_to_full(T),
       "ranges of 12 .. 16 slices on 4 waves: full waves (4 slots) next to waves of 3"),
    _r("spw5-c3d4", "C3D4", (11, 11, 63), 0, 8, 27648, 144, 125824, (5, 5, 1), (6, 0, 1, 8),
       lambda T: _real(T) and T.lens.max() == 20 and _short_next_to_full(T),
       "five slices per wave, one register row each; ranges of 16 .. 20: slot 4 free on some waves"),
    _r("spw6-c3d4", "C3D4", (12, 12, 59), 0, 8, 30420, 159, 139328, (6, 6, 1), (7, 0, 1, 8),
       lambda T: _real(T) and T.lens.max() == 22,
       "six slices per wave (no C3D4 plate of the issue's list lands here: 12 x 12 x 59 cells do)"),
    _r("spw7-c3d4", "C3D4", (13, 13, 63), 0, 8, 37632, 196, 173184, (7, 7, 0), (8, 0, 1, 3),
       lambda T: _real(T) and T.lens.max() == 28 and (T.res().npf == 0).all() and (T.res().jl == 0).all(),
       "seven slices per wave at the ceiling: no register row, no prefetch buffer; a range of exactly 28 fills every slot"),
    _r("spw7-c3d8", "C3D8", (15, 15, 47), 0, 8, 36864, 192, 301248, (7, 7, 0), (8, 0, 1, 5),
       lambda T: T.L.max() == 27 and T.L.min() == 12 and (T.res().streamed >= 2 * CH + 1).any(),
       "hexahedra, rows of 12 .. 27 blocks in <3,7,0>: three and more streamed batches per slice"),
    _r("declined-c3d4", "C3D4", (13, 13, 71), 0, 8, 42336, 221, 195136, None, (-1,),
       lambda T: T.lens.max() == 30 and T.sh() is None and T.sh(G=16).SPW == 4 and T.sh(G=24).SPW == 3,
       "a range of 30 slices: per_wave 8, just above the ceiling of 3 x 3 blocks -- three launches"),
    _r("long-c3d10", "C3D10", (5, 5, 12), 0, 8, 9075, 48, 77440, (3, 3, 4), (6, 0, 1, 8),
       lambda T: T.L.max() == 65 and T.row.n % 2 == 1 and ((T.res().npf == 4) & (T.res().streamed[:, :, 0] >= 3 * CH)).any()
       and (T.occupied() < 3).any(),
       "rows of 10 .. 65 blocks: several streamed batches behind the prefetched one; n = 9075 odd (npad rounding); ranges of "
       "3 .. 10 slices: waves with 1 and 2 slices"),
    _r("loose-rj4-c3d4", "C3D4", (5, 5, 29), 512, 8, 4776, 25, 13888, (3, 3, 4), (3, 0, 1, 8),
       lambda T: (T.L == 1).sum() == 8 and ((T.res().L == 1) & (T.res().jl == 1)).any() and _short_next_to_full(T)
       and ((T.res().sl >= 0) & (T.res().streamed == 0) & (T.res().lds == 0)).any(),
       "8 slices of loose nodes (L = 1 < RJ = 4 and 5: zero register rows, min(RJ, L)) in the last range, whose waves are full "
       "while the others hold 2 or 3 slices of 7 .. 15 rows"),
    _r("loose-rj3-c3d4", "C3D4", (10, 10, 55), 1500, 24, 24828, 130, 93504, (4, 4, 3), (4, 0, 1, 8),
       lambda T: T.sh().nwx == 12 and T.lens.max() == 38 and ((T.res().L == 1) & (T.res().jl == 1)).any()
       and (T.occupied() == 1).any() and (T.occupied() == 4).any(),
       "G = 24: 12 waves per XCD (no power of two, three workgroups per XCD); 23 slices of loose nodes give the last range 38 "
       "slices (SPW 4, RJ 3 > L = 1: full waves) while the other ranges leave waves with a single slice"),
    _r("empty-waves-c3d4", "C3D4", (5, 5, 29), 0, 24, 3240, 17, 13376, (1, 3, 4), (2, 0, 1, 8),
       lambda T: T.lens.max() == 3 and any((T.occupied()[k, 4 * g:4 * g + 4] == 0).all() for k in range(PNX) for g in range(3))
       and any(0 < (T.occupied()[k, 4 * g:4 * g + 4] > 0).sum() < 4 for k in range(PNX) for g in range(3)),
       "17 slices on 96 waves: whole workgroups without a slice, and workgroups where some waves own one and the others none"),
    _r("empty-ranges-c3d4", "C3D4", (3, 3, 5), 0, 8, 288, 2, 1536, (1, 3, 4), (4, 0, 1, 8),
       lambda T: T.lens.tolist() == [1, 0, 0, 0, 0, 1, 0, 0],
       "2 slices: six of the 8 ranges (workgroups at G = 8) are empty"),
    _r("spw3-cps3", "strip", (703, 15), 0, 16, 22528, 176, 76032, (3, 3, 5), (3, 0, 1, 6),
       lambda T: _real(T) and T.sh().nwx == 8 and T.lens.max() == 24
       and ((T.res().L == 5) & (T.res().lds == 0) & (T.res().streamed == 0)).any()
       and T.streamed_rows(base(T.row)._replace(lds=6)) == 0 and (T.res().lds == 1).any(),
       "2 x 2 blocks at G = 16, rows of 5 and 7: a slice with L == RJ == 5 (nothing in LDS, nothing streamed); 6 LDS rows hold "
       "everything (npf = 0 everywhere, a prefetch of nothing), 3 end in the middle of a slice (LDS batches of 1 and 2)"),
    _r("spw4-cps3", "strip", (895, 15), 0, 16, 28672, 224, 96768, (4, 4, 5), (4, 0, 1, 8),
       lambda T: _real(T) and T.sh().nwx == 8 and T.lens.max() == 31 and T.lens.min() == 27 and _short_next_to_full(T)
       and (T.res().fills).all(),
       "G = 16: 27 .. 31 slices on 8 waves, full waves next to waves of three slices; the LDS budget of 4 ends at a slice "
       "boundary (two slices of 2 rows beyond RJ)"),
    _r("spw6-cps3", "strip", (703, 15), 0, 8, 22528, 176, 76032, (6, 6, 3), (9, 0, 1, 17),
       lambda T: _real(T) and T.lens.max() == 24 and T.occupied().max() == 6
       and (T.res().lds == 4).any() and (T.res().lds == 1).any(),
       "per_wave 6: ranges of 21 .. 24 slices, those of 24 fill every slot of their waves; rows of 5 and 7 at RJ = 3 (LDS "
       "batches of 2 and 4 rows, one of 1 where the budget of 9 ends)"),
    _r("spw6-cpe8", "held-beam", (160, 16, 20.0, 4.0), 0, 8, 16066, 126, 123200, (5, 6, 3), (9, 0, 1, 17),
       lambda T: T.L.max() == 21 and T.L.min() == 8 and T.lens.max() == 19 and (T.res().lds == 5).any()
       and T.occupied().max() == 5 and T.occupied().min() == 3,
       "per_wave 5 lands on SPW 6: the CPE8 beam, rows of 8 .. 21, LDS batches of 5 rows (4 + 1) and streamed tails; slot 5 is free on every wave, "
       "slots 3 and 4 on some"),
    _r("spw8-pw7-cps3", "strip", (831, 15), 0, 8, 26624, 208, 89856, (7, 8, 2), (10, 0, 1, 17),
       lambda T: _real(T) and T.lens.max() == 28 and T.occupied().max() == 7 and (T.res().lds == 5).any(),
       "per_wave 7 lands on SPW 8: slot 7 of every wave is free (assign = -1); LDS batches of 5 rows"),
    _r("spw8-pw8-cps3", "strip", (943, 15), 0, 8, 30208, 236, 102144, (8, 8, 2), (10, 0, 1, 17),
       lambda T: _real(T) and T.lens.max() == 32 and T.lens.min() == 28 and T.occupied().max() == 8 and T.occupied().min() == 7,
       "per_wave 8, the ceiling of 2 x 2 blocks: a range of 32 slices fills all 8 slots of its 4 waves, the others leave slot 7 "
       "free"),
    _r("declined-cps3", "strip", (991, 15), 0, 8, 31744, 248, 107264, None, (-1,),
       lambda T: T.lens.max() == 35 and T.sh() is None and T.sh(G=16).SPW == 6,
       "a range of 35 slices: per_wave 9, just above the ceiling of 2 x 2 blocks -- three launches"),
    _r("slivers-rj5-cps3", "sliver", (40, 400), 1000, 8, 4564, 36, 5248, (3, 3, 5), (1, 0, 2, 6),
       lambda T: sorted(set(T.L.tolist())) == [1, 3, 5] and ((T.res().L == 3) & (T.res().jl == 3)).any()
       and ((T.res().L == 1) & (T.res().jl == 1)).any() and (T.res().streamed.sum() == 0),
       "lone triangles (L = 3), loose nodes (L = 1) and the strip (L = 5 == RJ): every slice lives wholly in registers, the `has` "
       "zero rows and min(RJ, L) run for L = 1 and 3; the last slice of the strip is partly padding"),
    _r("slivers-rj3-cps3", "sliver", (40, 600), 2400, 8, 8564, 67, 8576, (5, 6, 3), (1, 0, 2, 6),
       lambda T: {1, 3, 5} <= set(T.L.tolist()) and ((T.res().L == 1) & (T.res().jl == 1)).any()
       and ((T.res().L == 3) & (T.res().lds == 0) & (T.res().streamed == 0)).any() and (T.res().lds == 1).any(),
       "the same at SPW 6, RJ = 3: L = 1 < RJ, L = 3 == RJ, L = 5 with two rows beyond -- one in LDS, one streamed at a budget "
       "of 1"),
]
BY_NAME = {r.name: r for r in ROWS}


def row_id(row):
    return row.name


def base(row):
    return Config(-1, 4, row.lds[0], 0, 1)


def carried(row, variant):
    """does the shipped build carry the row's shape in this variant?  (5 .. 7 slices of 3 x 3 blocks: the default only)"""
    return variant in (-1, 6) or not (row.kind.startswith("C3D") and row.shape[1] >= 5)


L2_ROWS = ("spw3-c3d4", "spw3-cps3")                               # option 113 and option 104 = -1: once per block size


def configs(row):
    """the configurations a row runs on the device (declined rows: the default alone)"""
    b = base(row)
    if row.shape is None:
        return [b]
    out = [b] + [b._replace(lds=v) for v in row.lds[1:]]
    out += [b._replace(variant=14), b._replace(variant=0), b._replace(rj=0), b._replace(dbg=16)]
    if carried(row, 14):                                           # the shape without register rows in the other variants
        out += [b._replace(rj=0, variant=14), b._replace(rj=0, variant=0)]
    if row.shape[1] == 3 and row.kind.startswith("C3D"):
        out.append(b._replace(rj=5))
        out.append(b._replace(rj=5, variant=14))
        out.append(b._replace(rj=5, variant=0))
    if row.name in L2_ROWS:
        out += [b._replace(l2=0), b._replace(l2=3), b._replace(lds=-1)]
    return out


def config_id(cfg):
    return "v%d-rj%d-lds%d-dbg%d-l2%d" % cfg


# --------------------------------------------------------------------------------------------------------------- cases
class PCase(ps.Case):
    """pcg_shapes.Case and a fourth right-hand side placed from the restatement (base configuration): 1e3 at the first free
    DOF of a wave's last occupied slot, of a slot 0 whose first streamed batch is prefetched, and of the first slice that
    lives wholly in registers"""

    def __init__(self, row, backend):
        super().__init__(row, backend)
        self.T = Restated(row, self.L, self.dm)
        G = row.G if row.shape is not None else 16                 # (a declined row: placed as the next grid would run it)
        res = self.T.res(G=G)
        self.marks = self._marks(res)
        b = np.zeros(self.n)
        for s in self.marks.values():
            b[self.first_free(s)] = 1.0e3
        self.bs["placed"] = b
        self.xref["placed"] = ps.pcg_ld(self.K, b, max(MAXITS))

    @staticmethod
    def _marks(res):
        occ = (res.sl >= 0).sum(axis=2)
        k, w = np.unravel_index(np.argmax(occ), occ.shape)
        marks = {"last-slot": int(res.sl[k, w, occ[k, w] - 1])}
        pf = np.argwhere(res.npf > 0)
        if len(pf):
            marks["prefetched"] = int(res.sl[pf[0][0], pf[0][1], 0])
        reg = np.argwhere((res.sl >= 0) & (res.L == res.jl))
        if len(reg):
            marks["registers"] = int(res.sl[tuple(reg[0])])
        return marks

    def first_free(self, s):
        nodes = self.node_of[s * SLICE:(s + 1) * SLICE]
        dofs = (nodes[nodes >= 0][:, None] * self.dm + np.arange(self.dm)[None, :]).ravel()
        free = np.ones(self.n, dtype=bool)
        free[self.cons] = False
        return int(dofs[free[dofs]][0]) if free[dofs].any() else int(dofs[0])


for _row in ROWS:
    ps.TABLES[_row.name] = (_row, PCase)


def case(name, backend):
    return ps.case(name, backend)


def _reset(ctx, backend):
    if backend == "hip":
        for opt, val in ((be.TUNE_PERSIST_VARIANT, -1), (OPT_RJ, 4), (OPT_LDS, -1), (OPT_DBG, 0), (OPT_WGS, 0),
                         (be.TUNE_PERSIST_L2_ROWS, 1)):
            ctx.set_option(opt, val)
    ps._reset(ctx)


def _apply(c, cfg, G=None):
    ctx = c.ctx
    ctx.set_option(be.OPT_PCG_SMALL, 0)
    ctx.set_option(be.OPT_PCG_PERSIST, 2)
    if c.backend == "hip":
        ctx.set_option(OPT_WGS, G or c.row.G)
        ctx.set_option(be.TUNE_PERSIST_VARIANT, cfg.variant)
        ctx.set_option(OPT_RJ, cfg.rj)
        ctx.set_option(OPT_LDS, cfg.lds)
        ctx.set_option(OPT_DBG, cfg.dbg)
        ctx.set_option(be.TUNE_PERSIST_L2_ROWS, cfg.l2)


def _want(c):
    """the counters one solve moves"""
    if c.backend != "hip":
        return None
    took = c.row.shape is not None
    return {"solves_three": 0 if took else 1, "solves_small": 0, "solves_persist": 1 if took else 0, "barrier_timeouts": 0}


def _counted(c, out, what):
    want = _want(c)
    if want is not None:
        assert out[4] == want, (what, out[4])
    return out


# -------------------------------------------------------------------------------------------------------------- checks
def check_table(name, backend):
    """the pinned counts, the row's own limits, its shape and its edge -- from the restatement; on the device the library's
    stored_blocks and femcy_persist_streamed_bytes for every configuration"""
    c = case(name, backend)
    row, info, T = c.row, c.ctx.pattern_info(), c.T
    assert (info.n, info.nslices) == (row.n, row.nslices), (info.n, info.nslices, row.name)
    assert len(c.L) == row.nslices and int(c.L.sum()) * SLICE == row.stored, (len(c.L), int(c.L.sum()) * SLICE)
    assert row.nslices <= MAX_SLICES and row.n <= MAX_DOF and row.G in GRIDS
    sh = T.sh()
    assert (None if sh is None else (sh.per_wave, sh.SPW, sh.RJ)) == row.shape, (sh, row.shape)
    assert row.edge(T), (row.name, row.why)
    for cfg in configs(row):
        sh = T.sh(cfg)
        if sh is None:
            continue
        res = T.res(cfg)
        assert sorted(res.sl[res.sl >= 0].tolist()) == list(range(row.nslices))         # every slice once
        assert (res.lds.sum(axis=2) <= sh.lds_rows).all() and (res.streamed >= 0).all()
        assert sh.lds_rows <= sh.SPW * int(c.L.max())
        assert 4 * sh.lds_rows * SLICE * (c.dm * c.dm * 8 + 4) + 16 <= MAX_LDS, (cfg, sh)
    if backend == "hip":
        assert info.stored_blocks == row.stored and info.max_row_blocks == int(c.L.max()), (info.stored_blocks, info.max_row_blocks)
        try:
            for cfg in configs(row):
                _apply(c, cfg)
                got = c.ctx.persist_streamed_bytes()
                if row.shape is None or row.nslices < row.G:       # (the library answers 0 below one slice per workgroup)
                    assert got == 0, (cfg, got)
                    continue
                sh, res = T.sh(cfg), T.res(cfg)
                if cfg.lds < 0:
                    # the device's own LDS limit decides the rows: only the bound holds
                    assert got <= int((c.L.sum() - res.jl.sum())) * (c.dm * c.dm * 8 + 4) * SLICE, (cfg, got)
                    continue
                mine = int(res.streamed.sum()) * (c.dm * c.dm * 8 + 4) * SLICE
                if res.fills.all() or res.streamed.sum() == 0:
                    assert got == mine, (cfg, got, mine)
                else:
                    assert got <= mine, (cfg, got, mine)
        finally:
            _reset(c.ctx, backend)
    return T


def check_config(name, cfg, backend):
    """one configuration: the iterates at maxit 1, 2, 7 (eps = 0) of the four right-hand sides against the long-double
    recurrence, the counters, VEC_X prefilled with NaN (ps._solve).  A variant the build does not carry for the shape must be
    refused in the library's own words and leave the next default solve untouched.  -> worst deviations"""
    c = case(name, backend)
    ctx, worst = c.ctx, {}
    try:
        _apply(c, cfg)
        if backend == "hip" and not carried(c.row, cfg.variant):
            ctx.upload(be.VEC_RESIDUAL, c.bs["smooth"])
            try:
                ctx.pcg(be.VEC_RESIDUAL, be.VEC_X, eps=0.0, maxit=2)
                raise AssertionError("variant %d of %s was not refused" % (cfg.variant, name))
            except be.FemcyError as e:
                assert "default variant" in str(e) and "only" in str(e), str(e)
            ctx.set_option(be.TUNE_PERSIST_VARIANT, -1)
            for m in MAXITS:
                out = _counted(c, ps._solve(c, c.bs["smooth"], m), (name, cfg, m))
                ps._check_iterate(c, "smooth", m, out, (name, cfg, "after the refusal", m), worst, T_ALPHA, T_X)
        else:
            for key in c.bs:
                for m in MAXITS:
                    out = _counted(c, ps._solve(c, c.bs[key], m), (name, cfg, key, m))
                    ps._check_iterate(c, key, m, out, (name, config_id(cfg), key, m), worst, T_ALPHA, T_X)
    finally:
        _reset(ctx, backend)
    shares = {m: worst[m] / (4.0 * (T_ALPHA if m == 1 else T_X[m])) for m in MAXITS if m in worst}
    print(f"{name} [{backend}] {config_id(cfg)}: worst deviation {worst}, shares of the bounds {shares}")
    return worst


def check_once(name, backend, fit=True):
    """once per shape (base configuration): the stop at eps = 1e-10 -- max|r| below eps r0 and the long-double max|b - K x|
    on every row, the oracle's iteration count where check_fit holds (fit) --, b = 0, a NaN in a wave's last occupied slot, a
    repeated solve, and the same solve after a different-sized one at another grid"""
    c = case(name, backend)
    ctx = c.ctx
    b = c.bs["smooth"]
    try:
        _apply(c, base(c.row))
        _, ito, r0o, _ = orc.pcg_reference(c.K, b, eps=EPS_STOP, maxit=20 * c.n)
        it, r0, rmax, x, _ = _counted(c, ps._solve(c, b, 20 * c.n, EPS_STOP), (name, "stop"))
        assert r0 == r0o and rmax < EPS_STOP * r0 and 0 < it < 20 * c.n, (r0, r0o, rmax, it)
        if fit:                                                    # (elsewhere the oracle's own count scatters: UNFIT)
            assert abs(it - ito) <= max(2, ito // 50), (it, ito)
        res = float(np.abs(ps.mul_ld(c.K, x) - b.astype(LD)).max())
        print(f"{name} [{backend}]: {it} iterations (oracle {ito}), max|K x - b| / r0 = {res / r0:.2e}")
        assert res < 2 * EPS_STOP * r0 + 1e-9 * r0, (res, r0)
        it, r0, rmax, x, _ = _counted(c, ps._solve(c, np.zeros(c.n), 7), (name, "b = 0"))
        assert it == 0 and r0 == 0.0 and not x.any(), (it, r0)
        bad = b.copy()
        bad[c.first_free(c.marks["last-slot"])] = np.nan
        ctx.upload(be.VEC_RESIDUAL, bad)
        try:
            ctx.pcg(be.VEC_RESIDUAL, be.VEC_X, eps=0.0, maxit=7)
            raise AssertionError("a NaN in b went unnoticed")
        except be.FemcyError as e:
            assert e.status == be.FEMCY_ENUMERIC, e
        first = _counted(c, ps._solve(c, b, 7), (name, "first"))
        again = _counted(c, ps._solve(c, b, 7), (name, "again"))
        assert first[:3] == again[:3] and np.array_equal(first[3], again[3]), "a repeated solve differs"
        if backend == "hip":
            other = next(G for G in GRIDS if G != c.row.G)
            ctx.set_option(OPT_WGS, other)
            out = ps._solve(c, c.bs["last"], 3)                     # another grid, another length: taken or declined, no time-out
            assert out[4]["barrier_timeouts"] == 0 and out[4]["solves_small"] == 0, out[4]
            ps._check_iterate(c, "last", 2, ps._solve(c, c.bs["last"], 2), (name, "G", other), {}, T_ALPHA, T_X)
            ctx.set_option(OPT_WGS, c.row.G)
            back = _counted(c, ps._solve(c, b, 7), (name, "back"))
            assert first[:3] == back[:3] and np.array_equal(first[3], back[3]), "a solve at another grid left something behind"
    finally:
        _reset(ctx, backend)


def seen(T):
    """what the row's configurations reach, as lists (tests/test_persist_shapes_cpu.py takes the union over the table)"""
    row, dm = T.row, T.dm
    out = collections.defaultdict(set)
    out["G"].add(row.G)
    if row.n % 2:
        out["odd_n"].add(row.name)
    if (row.n // dm) % SLICE:
        out["padding_last"].add(row.name)
    if row.shape is None:
        out["declined"].add(dm)
        return {k: sorted(v) for k, v in out.items()}
    out["per_wave%d" % dm].add(row.shape[0])
    if (T.lens == 0).any():
        out["empty_range"].add(row.name)
    for cfg in configs(row):
        sh, res = T.sh(cfg), T.res(cfg)
        if carried(row, cfg.variant):
            out["shapes"].add((dm, sh.SPW, sh.RJ, 6 if cfg.variant < 0 else cfg.variant))
        on = res.sl >= 0
        occ = on.sum(axis=2)
        out["npf"] |= set(res.npf.ravel().tolist())
        out["lds_batch"] |= set(res.lds[on & (res.lds > 0)].tolist())
        out["streamed"] |= set(res.streamed[on].tolist())
        out["rj_above_L"] |= {sh.RJ} if (on & (res.L < sh.RJ)).any() else set()
        out["rj_equals_L"] |= {sh.RJ} if (on & (res.L == sh.RJ) & (sh.RJ > 0)).any() else set()
        if ((occ > 0) & (occ < sh.SPW)).any() and (occ == sh.SPW).any():
            out["free_slots"].add(row.name)
        wg = occ.reshape(PNX, -1, 4)
        if (((wg == 0).any(axis=2)) & ((wg > 0).any(axis=2))).any():
            out["empty_wave"].add(row.name)
        if (wg == 0).all(axis=2).any():
            out["empty_workgroup"].add(row.name)
        if sh.lds_rows == 0:
            out["budget"].add("none")
            continue
        if res.streamed.sum() == 0:
            out["budget"].add("nothing-streamed")
        partial = on & (res.lds > 0) & (res.streamed > 0)
        if partial.any():
            out["budget"].add("inside")
        full = res.fills & ~partial.any(axis=2) & (res.streamed.sum(axis=2) > 0)
        if full.any():
            out["budget"].add("boundary")
        if (res.fills & (res.lds[:, :, 0] == 0) & (res.streamed[:, :, 0] > 0) & (occ > 1)).any():
            out["budget"].add("before-slot-0")
    return {k: sorted(v) for k, v in out.items()}


def measure_constants(backend="cpu", rows=None):
    _, t = ps.measure_constants(backend, rows or ROWS)
    return t
