"""The solver menu of the HIP backend, device-free:
what a solver variant is, which pairs of graphs fit it, the LDS, the register
slots and the occupancy it needs, and the partition of a job list into
launches.  `HIPBackend` inherits `SolverMenu`; a `SolverMenu` by itself
answers the same questions without a device, a compiler or a code generator.

Module-level imports: numpy and `._devicegraph`, nothing else -- not
`hip.runtime`, `hip.jit`, `codegen` or torch; `hip.hostlib` inside the native
branches only.
"""
from collections import namedtuple
from typing import NamedTuple
import numpy as np
from ._devicegraph import (HIST_BINS, class_bytes, term_bytes,
                           graph_features, quotient_images)

Variant = namedtuple('Variant', 'W S R')
#: owner-computes solver (csrc/device/mgk_oc.h): S nonzero slots and R rows
#: per lane, for pairs of graphs whose largest degree is at most D
#: L: None, or the static row-batch layout (seg_layout<L...> in mgk_oc.h):
#: batch k of a lane owns exactly L[k] slots, S = sum(L), R = len(L)
OCVariant = namedtuple('OCVariant', 'W S R D L', defaults=(None,))


#: measured efficiency of M workgroups on one pair of the streamed solver
#: against M times one workgroup (MI355X, protein-like graphs of 150-600
#: atoms, float; profiles/sessions.md r5_session18 and DESIGN.md section 4c:
#: three grid-wide barriers per iteration, B staged by every part)
STREAM_PART_EFFICIENCY = ((1, 1.0), (2, 0.74), (4, 0.58), (8, 0.53),
                          (16, 0.50), (32, 0.49), (64, 0.46), (128, 0.35),
                          (256, 0.26))


def stream_parts(costs, count, resident, queued):
    """Workgroups per pair (M) of a streamed launch: the M with the smallest
    estimated time for the launch's pairs -- `costs`, largest first, in
    arbitrary units.  One workgroup per pair (`queued` workgroups, the
    hardware hands the next pair to the first free compute unit) takes
    max(largest pair, sum / resident); M workgroups per pair form
    resident // M groups that walk the pairs round-robin, a group's time is
    the sum of its pairs over M x efficiency(M).  136 pairs of 16 graphs:
    M = 1 105.8 ms (the largest pair on one workgroup, 120 compute units
    idle), 2 / 4 / 8 / 16: 84.8 / 73.7 / 65.8 / 65.7 ms; 528 pairs: 140.9 ms
    at M = 1 against 191-198 at 2 ... 16."""
    if costs is None or len(costs) == 0:
        return max(1, min(resident // max(count, 1), STREAM_MAX_PARTS))
    c = np.asarray(costs, dtype=np.float64)
    best, best_t = 1, max(c[0], c.sum() / max(1, min(resident, queued)))
    table = dict(STREAM_PART_EFFICIENCY)
    ms, es = zip(*STREAM_PART_EFFICIENCY)
    # (powers of two, and what gives every pair a group of its own)
    own = min(resident // max(len(c), 1), STREAM_MAX_PARTS)
    for M in sorted(set(ms[1:]) | ({own} if own > 1 else set())):
        if M > min(resident, STREAM_MAX_PARTS):
            break
        eff = table.get(M) or float(np.interp(np.log2(M), np.log2(ms), es))
        groups = max(1, resident // M)
        pad = -len(c) % groups
        load = np.concatenate((c, np.zeros(pad))).reshape(-1, groups).sum(0)
        t = load.max() / (M * eff)
        if t < 0.95 * best_t:        # (a larger M must earn its barriers)
            best, best_t = M, t
    return best


def OCStatic(*L, D=4):
    """One-wave owner-computes variant with the static layout L."""
    return OCVariant(1, int(sum(L)), len(L), D, tuple(int(x) for x in L))


#: register-resident solver menu, cheapest first.  A pair fits a variant if
#: its stage-1 walk needs <= S slots per lane and N = n1*n2 <= 64*W*R.
VARIANTS = [
    Variant(1, 8, 2), Variant(1, 12, 3), Variant(1, 16, 4), Variant(1, 20, 5),
    Variant(1, 24, 6), Variant(1, 28, 7), Variant(1, 32, 9), Variant(1, 48, 9),
    Variant(1, 64, 16),
    Variant(4, 16, 4), Variant(4, 32, 8), Variant(4, 64, 16),
    Variant(16, 16, 2), Variant(16, 32, 4), Variant(16, 64, 8),
    Variant(16, 128, 16),
]
#: owner-computes menu, cheapest first: molecular graphs (every degree <= 4)
#: take the D = 4 kernels, graphs with degrees up to 8 (the Newman-Watts-
#: Strogatz graphs of configuration 2: 4..7) the D = 8 kernels with 1, 4, 8
#: or 16 waves per pair.  S <= 64: larger slot arrays are not promoted to
#: registers by the compiler (they would live in scratch memory).
#: Static layouts first: a pair whose per-batch degree products fit one takes
#: it (no flush tests, row sums in registers); the dynamic variants behind
#: them take what is left.  The layouts are the profiles of molecular graphs
#: (degrees <= 4: the first batch holds the 16-term rows of two four-valent
#: atoms, then 4 = 2 x 2 / 4 x 1, then hydrogens): on the QM7-like set 66
#: distinct profiles, all under one of these.
#: The twin-leaf quotient images have lost most of their
#: leaves: the first rows of a quotient pair have 16, 12 or 9 terms (largest
#: degrees 4 x 4, 4 x 3, 3 x 3) and no second batch opens with more than 3 on
#: all but 3 % of the QM7-like pairs.  OC_QUOTIENT_LAYOUTS are cut to that; they
#: are offered to the plans on quotient images only (C = 1, graph-level values)
#: -- every other path keeps the menu its occupancy targets were swept with.
OC_QUOTIENT_LAYOUTS = ((12, 3), (16, 3), (12, 3, 1), (16, 3, 1))
OC_STATIC_VARIANTS = [
    OCStatic(12, 3), OCStatic(16), OCStatic(16, 3), OCStatic(16, 4),
    OCStatic(12, 3, 1), OCStatic(16, 3, 1), OCStatic(16, 4, 1), OCStatic(16, 4, 4),
    OCStatic(16, 4, 4, 1), OCStatic(16, 4, 4, 1, 1), OCStatic(16, 4, 4, 3, 1),
    OCStatic(16, 4, 4, 3, 1, 1), OCStatic(16, 4, 4, 4, 1, 1, 1),
    OCStatic(16, 4, 4, 4, 3, 1, 1, 1), OCStatic(16, 4, 4, 4, 4, 1, 1, 1, 1),
]
#: on-the-fly variants (mgk_oc.h FLY: S = 0, D = 0): no register slots, the
#: edge microkernel is evaluated per term in every iteration; any degree.
#: For the pairs no slot variant fits (dense from_ase-like graphs): values
#: (graph-level and nodal) and graph-level value + gradient.
OC_FLY_VARIANTS = [
    OCVariant(4, 0, 1, 0), OCVariant(4, 0, 2, 0), OCVariant(4, 0, 3, 0),
    OCVariant(8, 0, 2, 0), OCVariant(16, 0, 2, 0), OCVariant(16, 0, 4, 0),
]
OC_VARIANTS = OC_STATIC_VARIANTS + [
    OCVariant(1, 12, 2, 4), OCVariant(1, 16, 3, 4), OCVariant(1, 20, 3, 4),
    OCVariant(1, 20, 4, 4), OCVariant(1, 24, 4, 4), OCVariant(1, 28, 5, 4),
    OCVariant(1, 28, 6, 4), OCVariant(1, 32, 7, 4), OCVariant(1, 36, 9, 4),
    OCVariant(1, 32, 3, 8), OCVariant(1, 48, 5, 8), OCVariant(1, 64, 9, 8),
    OCVariant(4, 32, 3, 8), OCVariant(4, 40, 2, 8), OCVariant(4, 48, 4, 8),
    OCVariant(4, 64, 5, 8),
    OCVariant(8, 40, 2, 8), OCVariant(8, 48, 3, 8), OCVariant(8, 64, 4, 8),
    OCVariant(16, 32, 2, 8), OCVariant(16, 40, 2, 8), OCVariant(16, 48, 3, 8),
    OCVariant(16, 64, 3, 8),
] + OC_FLY_VARIANTS
#: pairs with a node of more than this many neighbours are what the
#: on-the-fly variants are for (the slot variants stop at degree 8)
FLY_MIN_DEGREE = 8
#: sentinel: the global-memory general solver (any pair size)
GENERAL = Variant(0, 0, 0)
#: sentinel: the kernel that fills the global microkernel tables
TABLES = Variant(-1, 0, 0)
GENERAL_THREADS = 1024
#: sentinel: the dense-tile solver on the matrix cores (csrc/device/mgk_mfma.h):
#: float value solves of DENSE pairs of graphs of at most 32 nodes under an
#: edge microkernel that ignores the labels (`Constant`: one separable term).
#: 82 M pairs/s against 4.2 M of the on-the-fly dense product on the dense
#: molecular set (scripts/mfma_experiment.py).  GD_MFMA=0: off.
MFMA = Variant(-3, 0, 0)
MFMA_MAX_NODES = 32
#: sentinel: the streamed solver for large pairs (csrc/device/mgk_stream.h):
#: value solves of pairs beyond every register- and LDS-resident variant; one
#: graph of the pair staged in LDS, the other streamed row by row, CG vectors
#: in a global scratch.
STREAM = Variant(-2, 0, 0)
STREAM_THREADS = 1024
#: rows of p staged per pass and row group (mgk_stream.h A_ROWS)
STREAM_ROWS = {4: 8, 8: 8}       # by the size of a real
#: neighbours per lane segment of the LDS-resident graph (mgk_stream.h SEG_CAP)
STREAM_CAP = 16
#: workgroups that may share one pair of the streamed solver
STREAM_MAX_PARTS = 256
#: dynamic LDS a pair of the streamed solver may ask for (mgk_stream.h LDS_BUDGET)
STREAM_LDS_BUDGET = 159 * 1024
LDS_LIMIT = 160 * 1024
_LARGE_PAIR_SOLVERS = [MFMA, STREAM, GENERAL]
#: independent pairs (waves) per workgroup of the one-wave variants (mgk_solver.h
#: WPB; four pairs per 256-thread workgroup were 4-5 % slower: a workgroup's
#: LDS and wave slots are only released when its slowest pair is done)
WPB1 = 1
#: microkernel value tables (label classes) are used when they fit this much
#: LDS per workgroup: (n_node_classes^2 + n_edge_classes^2) reals
TABLE_LDS_LIMIT = 8 * 1024
#: class pairs (node + edge) up to which the global tables are used
GLOBAL_TABLE_LIMIT = 1 << 16


class ClassPairs:
    """The jobs of a call by pair of graph classes: `pk[t]` the key of job t,
    `upk` the sorted keys in use (position = index into the per-class-pair
    results), `count[key]` the jobs per key."""

    def __init__(self, pk, upk, count, nc):
        self.pk, self.upk, self.count, self.nc = pk, upk, count, nc
        self._sel = None

    @property
    def sel(self):
        """index of every job's class pair in the per-class-pair results"""
        if self._sel is None:
            pos = np.zeros(self.nc * self.nc, dtype=np.int32)
            pos[self.upk] = np.arange(len(self.upk), dtype=np.int32)
            self._sel = pos[self.pk]
        return self._sel

    @property
    def members(self):
        return self.count[self.upk].astype(np.int64)


class Partition(tuple):
    """Result of `HIPBackend._partition`: (jobs, used, order_all, launches)
    as a tuple, plus `.jobs_sorted` -- the job records in launch order when
    the native ordering wrote them (else None) -- and `.merge_map`, the
    launch merging that was applied ({variant index: variant index})."""
    jobs_sorted = None
    merge_map = {}


class CallShape(NamedTuple):
    """What a call is, as far as classification and code generation look:
    made by `HIPBackend._call_shape` ("The host plan of a call")."""
    C: int                    # right-hand sides: 2 = value + analytic gradient
    nodal: bool = False
    ngrad: bool = False       # finite-difference Jacobian in the launch
    maximin: int = 0          # epilogue: 0 none, 1 maximin, 2 M3
    quot: bool = False        # twin-leaf quotient images
    tab_bytes: int = 0        # LDS tables of the two-stage solvers
    gtab: bool = False        # global tables of the owner-computes solvers
    oc_only: bool = False     # solver menu: owner-computes only
    mfma: bool = False        # solver menu: the dense-tile MFMA solver
    tab = property(lambda self: self.tab_bytes > 0)


class NotOwnerComputes(Exception):
    """Some pair of the call does not fit an owner-computes solver variant
    (raised when a feature only those solvers have was asked for)."""


class SolverMenu:
    """The solver menu of one arithmetic.

    Parameters
    ----------
    real: numpy float32 or float64
    variants: list of Variant / OCVariant, or None
        The menu in order of preference (None: the default menu,
        ``OC_VARIANTS + VARIANTS`` and the large-pair solvers).
    occupancy: dict (W, S) -> waves per SIMD, or None
        Overrides the measured occupancy targets.
    native: bool
        Classification and ordering in C++ (libgdhost.so) or in numpy.
    min_launch: int
        Owner-computes launches of fewer waves are merged (0: never).
    jobs_per_unit: int
        Graph pairs per wave or workgroup; sets the launch grid.
    """

    def __init__(self, real=np.float32, variants=None, occupancy=None,
                 native=True, min_launch=8192, jobs_per_unit=1):
        self.real = np.dtype(real).type
        self.variants = list(
            OC_VARIANTS + VARIANTS + _LARGE_PAIR_SOLVERS
            if variants is None else variants)
        self.occupancy = occupancy
        self.native = bool(native)
        self.min_launch = int(min_launch)
        self.jobs_per_unit = int(jobs_per_unit)

    @property
    def f64(self):
        """double arithmetic (else float)"""
        return np.dtype(self.real) == np.float64

    @property
    def rsize(self):
        """bytes of a real"""
        return np.dtype(self.real).itemsize

    #: occupancy targets of the fp32 value solver, W = 1 (hipcc 7.2, gfx950):
    #: S -> waves per SIMD.  Spill-free or nearly so, except S = 24 where 16
    #: VGPRs spilled around (never inside) the CG loop buy 4 instead of 3
    #: waves: +7 % on the whole Gram matrix for 2 KB of scratch traffic per
    #: pair.  S = 16 at 6 waves and S = 28 at 4 are another +3 % but write
    #: 5-10 KB of scratch per pair to HBM (profiles/README.md) -- not taken.
    _WAVES_F32_VALUE = {8: 6, 12: 6, 16: 5, 20: 4, 24: 4, 28: 3, 32: 2}
    #: same for the value + gradient solver (C = 2) and the fp64 value solver:
    #: the fastest of a per-variant sweep (scripts/occupancy_sweep2.sh)
    _WAVES_F32_GRADIENT = {8: 5, 12: 4, 16: 3, 20: 2, 24: 2, 28: 2, 32: 1}
    _WAVES_F64_VALUE = {8: 5, 12: 4, 16: 3, 20: 3, 24: 2, 28: 2, 32: 2}
    _WAVES_F64_GRADIENT = {8: 3, 12: 3, 16: 2, 20: 2, 24: 1, 28: 1, 32: 1}
    _WAVES_F32_VALUE_W4 = {(4, 32): 3, (4, 64): 2}
    _WAVES_F64_VALUE_W4 = {(4, 32): 2}

    def waves_per_eu(self, v, C):
        """Occupancy target handed to the register allocator
        (amdgpu_waves_per_eu).  The fp32 value solver needs about
        5.3 S + 4 R + 6 VGPRs to stay spill-free (measured: S=12 -> 81,
        S=16 -> 106, S=24 -> 150, S=32 -> 211); the targets are the highest
        occupancies with at most a handful of spilled registers, which were
        also the fastest or within 2 % of it in a per-variant sweep
        (scripts/occupancy_sweep.sh) and keep scratch traffic out of HBM."""
        floor = -(-64 * v.W * (WPB1 if v.W == 1 else 1) // 256)  # block must fit
        if self.occupancy is not None and (v.W, v.S) in self.occupancy:
            return max(self.occupancy[(v.W, v.S)], floor)
        if isinstance(v, OCVariant):
            return max(self._oc_waves(v, C), -(-64 * v.W // 256))
        if v.W == 1:
            table = {(1, False): self._WAVES_F32_VALUE,
                     (2, False): self._WAVES_F32_GRADIENT,
                     (1, True): self._WAVES_F64_VALUE,
                     (2, True): self._WAVES_F64_GRADIENT}.get(
                         (C, self.f64), {})
            if v.S in table:
                return max(table[v.S], floor)
        # four-wave variants of the fp32 value solver, measured on the
        # 8..48-node random graphs of configuration 2
        if C == 1:
            w4 = self._WAVES_F64_VALUE_W4 if self.f64 \
                else self._WAVES_F32_VALUE_W4
            if (v.W, v.S) in w4:
                return max(w4[(v.W, v.S)], floor)
        need = 5.3 * v.S + 4 * v.R + 6
        if C == 2:
            need = 1.6 * need
        if self.f64:                   # every real takes two VGPRs
            need = 1.8 * need
        for n in (8, 6, 5, 4, 3, 2):
            if need <= (512 // n) // 8 * 8 + 4:
                return max(n, floor)
        return max(1, floor)

    #: occupancy targets of the owner-computes variants, the fastest of a
    #: per-variant sweep on MI355X (scripts/oc_sweep.py: QM7-like set for
    #: D = 4, configuration 2 for D = 8): (double?, C) -> {(W, S, R, D): waves}
    #: (float (28, 5) at 5 waves is 2 % faster than at 4 but writes 2 KB of
    #: scratch per pair to HBM, profiles/r02_f32_pmc.csv: not taken)
    _OC_WAVES = {
        (False, 1): {('L', 16): 6, ('L', 16, 4): 6, ('L', 16, 4, 1): 5, ('L', 16, 4, 4): 5,
                     # (the layouts of quotient images, OC_QUOTIENT_LAYOUTS:
                     # the targets of (16,4) and (16,4,1), not yet swept)
                     ('L', 12, 3): 6, ('L', 16, 3): 6, ('L', 12, 3, 1): 5, ('L', 16, 3, 1): 5,
                     ('L', 16, 4, 4, 1): 3, ('L', 16, 4, 4, 1, 1): 3,
                     ('L', 16, 4, 4, 3, 1): 4, ('L', 16, 4, 4, 3, 1, 1): 4,
                     ('L', 16, 4, 4, 4, 1, 1, 1): 3,
                     ('L', 16, 4, 4, 4, 3, 1, 1, 1): 3,
                     ('L', 16, 4, 4, 4, 4, 1, 1, 1, 1): 3,
                     (1, 12, 2, 4): 6, (1, 16, 3, 4): 6, (1, 20, 3, 4): 6,
                     (1, 20, 4, 4): 4, (1, 24, 4, 4): 5, (1, 28, 5, 4): 4,
                     (1, 28, 6, 4): 4, (1, 32, 7, 4): 4, (1, 36, 9, 4): 2,
                     (1, 32, 3, 8): 2, (1, 48, 5, 8): 2, (1, 64, 9, 8): 2,
                     (4, 32, 3, 8): 4, (4, 40, 2, 8): 4, (4, 48, 4, 8): 2,
                     (4, 64, 5, 8): 3, (8, 40, 2, 8): 4, (8, 48, 3, 8): 4,
                     (8, 64, 4, 8): 4, (16, 32, 2, 8): 4, (16, 40, 2, 8): 4,
                     (16, 48, 3, 8): 4, (16, 64, 3, 8): 4},
        (True, 1): {('L', 16): 4, ('L', 16, 4): 4, ('L', 16, 4, 1): 3, ('L', 16, 4, 4): 3,
                    # (OC_QUOTIENT_LAYOUTS: the targets of (16,4) and (16,4,1),
                    # not yet swept; (12,3) is spill-free at four waves with
                    # 122 registers, the three-batch ones at three)
                    ('L', 12, 3): 4, ('L', 16, 3): 4, ('L', 12, 3, 1): 3, ('L', 16, 3, 1): 3,
                    # (round 5: the five-batch layouts at three waves -- with
                    # the row sums zeroed late and p updated in place
                    # (mgk_oc.h) their iteration is spill-free at 168
                    # registers: (16,4,4,1,1) 0.864 -> 0.726 ms, (16,4,4,3,1)
                    # 0.115 -> 0.105; the six-batch layout reloads 12 values
                    # per iteration at three -- 0.557 -> 0.849 -- unless its
                    # diagonals leave the registers, below)
                    ('L', 16, 4, 4, 1): 3, ('L', 16, 4, 4, 1, 1): 3,
                    # ((16,4,4,3,1,1): three waves with the Jacobi diagonals in
                    # LDS, mgk_oc.h DLDS -- nothing reloaded in the iteration)
                    ('L', 16, 4, 4, 3, 1): 3, ('L', 16, 4, 4, 3, 1, 1): 3,
                    ('L', 16, 4, 4, 4, 1, 1, 1): 2,
                    ('L', 16, 4, 4, 4, 3, 1, 1, 1): 2,
                    ('L', 16, 4, 4, 4, 4, 1, 1, 1, 1): 2,
                    (1, 12, 2, 4): 4, (1, 16, 3, 4): 4, (1, 20, 3, 4): 4,
                    (1, 20, 4, 4): 3, (1, 24, 4, 4): 3, (1, 28, 5, 4): 3,
                    (1, 28, 6, 4): 3, (1, 32, 7, 4): 2, (1, 36, 9, 4): 2,
                    (1, 64, 9, 8): 1, (4, 32, 3, 8): 3, (4, 40, 2, 8): 3,
                    (4, 64, 5, 8): 2, (8, 40, 2, 8): 2, (8, 64, 4, 8): 2},
        (False, 2): {('L', 16): 4, ('L', 16, 4): 4, ('L', 16, 4, 1): 4, ('L', 16, 4, 4): 2,
                     ('L', 16, 4, 4, 1): 2, ('L', 16, 4, 4, 1, 1): 3,
                     ('L', 16, 4, 4, 3, 1): 3, ('L', 16, 4, 4, 3, 1, 1): 3,
                     ('L', 16, 4, 4, 4, 1, 1, 1): 2,
                     ('L', 16, 4, 4, 4, 3, 1, 1, 1): 2,
                     ('L', 16, 4, 4, 4, 4, 1, 1, 1, 1): 2,
                     (1, 12, 2, 4): 4, (1, 16, 3, 4): 4, (1, 20, 3, 4): 3,
                     (1, 20, 4, 4): 2, (1, 24, 4, 4): 3, (1, 28, 5, 4): 3,
                     (1, 28, 6, 4): 2, (1, 32, 7, 4): 2, (1, 36, 9, 4): 2},
        # (static layouts: the sequential solves of mgk_oc.h SEQ, round 4 --
        # profiles/sessions.md r4_session2 / r4_session4: three waves only
        # where the loop stays free of scratch reloads, the three-batch kernel)
        # (round 5: the four-batch sequential solver at three waves -- with
        # the row sums zeroed late and p updated in place nothing is reloaded
        # inside its iteration at 168 registers: 2.89 -> 2.65 ms; (16,4,4)
        # loses at three, 0.175 -> 0.188, the five-batch kernel reloads three
        # values per iteration there, 2.0 -> 2.86 ms)
        (True, 2): {('L', 16): 2, ('L', 16, 4): 2, ('L', 16, 4, 1): 3, ('L', 16, 4, 4): 2,
                    ('L', 16, 4, 4, 1): 3, ('L', 16, 4, 4, 1, 1): 2,
                    ('L', 16, 4, 4, 3, 1): 2, ('L', 16, 4, 4, 3, 1, 1): 2,
                    ('L', 16, 4, 4, 4, 1, 1, 1): 2,
                    ('L', 16, 4, 4, 4, 3, 1, 1, 1): 2,
                    ('L', 16, 4, 4, 4, 4, 1, 1, 1, 1): 1,
                    (1, 12, 2, 4): 3, (1, 16, 3, 4): 3, (1, 20, 3, 4): 3,
                    (1, 20, 4, 4): 2, (1, 24, 4, 4): 2, (1, 28, 5, 4): 2,
                    (1, 28, 6, 4): 2, (1, 32, 7, 4): 2, (1, 36, 9, 4): 2},
    }

    #: static layouts that lose to the dynamic variants behind them in the
    #: menu (measured, scripts/oc_sweep.py): (double?, C) -> {layout, ...}.
    #: Round 3 had the double value + gradient solves here: the STACKED
    #: two-right-hand-side solver moves 16 bytes per gathered element and
    #: keeps both systems' vectors in registers, and its static form was no
    #: faster than the dynamic one (14.3 / 18.4 / 22.7 ns per pair for the
    #: three- / four- / five-batch pairs against 14.5 / 17.2 / 21.7).  The
    #: static double kernels now solve the two systems one after the other
    #: (mgk_oc.h SEQ) and are back in the menu.
    _STATIC_OFF = {}

    def _static_enabled(self, v, C, quot=True):
        """Is the static layout of `v` on the menu of a plan with C right-hand
        sides, on quotient images (`quot`) or full ones?"""
        if v.L in OC_QUOTIENT_LAYOUTS and not quot:
            return False
        return v.L not in self._STATIC_OFF.get((self.f64, C), ())

    @staticmethod
    def grid_of(L, D):
        """(GU, GV) of the grid walk that mgk_oc.h gives the first batch of the
        static layout L of a D-kernel (oc_solver::grid_rows), or None: the
        running walk.  A pair fits the grid if the larger of its graphs'
        largest degrees is <= GU and the smaller <= GV.  (A grid that is not
        square exists in the graph-level value kernels of quotient images
        only, the plans OC_QUOTIENT_LAYOUTS are offered to; there the kernel
        takes either graph in the first role, and the host sizes p for
        both.)"""
        if not L or D < 2:
            return None
        if L[0] in (D * D, D * (D - 1)):
            return D, L[0] // D
        if L[0] == (D - 1) * (D - 1):
            return D - 1, D - 1
        return None

    @classmethod
    def swaps_roles(cls, v, maxdeg_j):
        """Does the kernel of variant `v` give the second graph of a job the
        first role (mgk_oc.h ORIENT)?  In a grid that is not square, when that
        graph -- of largest degree `maxdeg_j`, an array -- has a node of more
        than GV neighbours."""
        g = cls.grid_of(v.L, v.D) if isinstance(v, OCVariant) else None
        maxdeg_j = np.asarray(maxdeg_j)
        if g is None or g[0] == g[1]:
            return np.zeros(maxdeg_j.shape, dtype=bool)
        return maxdeg_j > g[1]

    @classmethod
    def _grid_takes(cls, v2, v):
        """May the pairs of the static layout `v` ride in the static layout
        `v2` -- does every pair that fits v's first batch fit v2's grid?"""
        g2 = cls.grid_of(v2.L, v2.D)
        if g2 is None or g2 == (v2.D, v2.D):
            return True
        g = cls.grid_of(v.L, v.D)
        return g is not None and g[0] <= g2[0] and g[1] <= g2[1]

    _FLY_WAVES = 3     # (occupancy 3-6 waves per SIMD: 4.95-4.86 M pairs/s, round 3)

    def _oc_waves(self, v, C, ngrad=False):
        """Occupancy target of an owner-computes variant: per lane S values +
        S gather indices, 6 registers per row (x, r, p, diagonal, its inverse,
        the publish address), the gathers in flight and ~24 others; a double
        takes two registers."""
        f64 = self.f64
        if v.S == 0:
            # on-the-fly kernels: no slot arrays, but the unrolled term loops
            # keep ~140 registers busy (spill-free at three waves per SIMD)
            return max(self._FLY_WAVES, -(-64 * v.W // 256))
        # (static layouts under ('L',) + layout: a four-batch layout is a
        # 4-tuple like the (W, S, R, D) of a dynamic variant)
        hit = self._OC_WAVES.get((f64, C), {}).get(
            ('L',) + v.L if v.L else tuple(v)[:4])
        if hit and not ngrad:
            return hit
        w = 2 if f64 else 1
        need = (w * C + 1) * 0 + v.S * (w + 1) + v.R * (5 * w * C + 1) \
            + 8 * w * C + 24 + (6 * w * v.R if ngrad else 0)
        for n in (8, 6, 5, 4, 3, 2):
            if need <= (512 // n) // 8 * 8:
                return n
        return 1

    # -- job partitioning ---------------------------------------------------------
    @staticmethod
    def _dense_bytes(dgraphs, n):
        """LDS bytes of the two dense edge arrays of a pair (mgk_oc.h DENSE)
        for graphs of at most n nodes -- the largest graph among the pairs of
        the LAUNCH, not of the call: a call that mixes small dense graphs with
        large ones keeps the dense product for the small ones --: n x n
        records, and the record's dword planes in rows of 32 words; 0 if n
        exceeds 32 nodes (the kernel's row stride) or the records are not
        whole words."""
        esize = np.dtype(dgraphs[0].edge_t).itemsize if len(dgraphs) else 0
        if not 0 < n <= 32 or esize == 0 or esize % 4:
            return 0
        return -(-(n * n * esize) // 16) * 16 + esize * (n + 3) * 32 + 256

    @staticmethod
    def stream_virtual_rows(adjacency_count):
        """Lanes the streamed solver deals a graph's nodes onto when it is
        the LDS-resident one (mgk_stream.h, "virtual rows"): a node is cut
        into segments of at most CAP neighbours, CAP = 16 doubled until the
        segments fit the STREAM_THREADS lanes of a workgroup; every node has
        a first segment."""
        d = np.asarray(adjacency_count, dtype=np.int64)
        cap = STREAM_CAP
        while True:
            nv = len(d) + sum(int((d > l * cap).sum())
                              for l in range(1, int(d.max(initial=0)) // cap + 1))
            if nv <= STREAM_THREADS or cap > (1 << 20):
                return nv
            cap *= 2

    def stream_lds_bytes(self, image1, image2, n1, n2, nv1, nv2):
        """Dynamic LDS of a pair in the streamed solver (mgk_stream.h): the
        image of B -- the smaller image among the graphs of at most
        STREAM_THREADS nodes, ties: graph 2 -- in 16-byte units (if it fits
        STREAM_LDS_BUDGET beside the staged rows at their largest; otherwise
        B is read from L2 and takes no LDS), and behind it, for each of the
        G = STREAM_THREADS // ceil64(nV) row groups of a workgroup step (nV:
        B's virtual rows), STREAM_ROWS rows of p and one partial sum per
        lane.  A huge number if neither graph qualifies."""
        image1, image2 = np.asarray(image1), np.asarray(image2)
        n1, n2 = np.asarray(n1), np.asarray(n2)
        w1, w2 = -(-image1 // 16), -(-image2 // 16)
        ok1, ok2 = n1 <= STREAM_THREADS, n2 <= STREAM_THREADS
        first = ok1 & (~ok2 | (w1 < w2))
        nB = np.maximum(np.where(first, n1, n2), 1)
        nV = np.maximum(np.where(first, nv1, nv2), 1)
        LB = (-(-nV // 64) * 64).clip(max=STREAM_THREADS)
        G = STREAM_THREADS // LB
        rs = self.rsize
        stage = (STREAM_ROWS[rs] * G * nB + G * LB) * rs
        image = np.where(first, w1, w2) * 16
        # (an image that does not fit beside the staged rows at their largest
        # stays in L2: the pair's body is instantiated for that case too)
        fits = image + (STREAM_ROWS[rs] + 1) * STREAM_THREADS * rs \
            <= STREAM_LDS_BUDGET
        out = np.where(fits, image, 0) + -(-stage // 16) * 16
        return np.where(ok1 | ok2, out, np.iinfo(np.int64).max // 4)

    def lds_slot_bytes(self, v, C, nodal=False):
        """LDS bytes of the slot values a variant keeps in LDS instead of
        registers (mgk_oc.h SL, `lds_slot_count`: the 16-wave double
        graph-level value solvers, 10 slots per lane; nodal outputs -- and
        with them the nodal-gradient and maximin launches -- keep every slot
        in registers)."""
        if (isinstance(v, OCVariant) and not v.L and C == 1 and v.W == 16
                and not nodal
                and v.S in (40, 64) and self.f64):
            return 10 * 64 * v.W * 8
        return 0

    def _waves_without_lds_diagonals(self, v, C, nodal):
        """Occupancy target of a kernel: `waves_per_eu`, but the six-batch
        double value layout runs three waves only WITH its Jacobi diagonals in
        LDS (mgk_oc.h DLDS) -- its nodal flavours and the builds without them
        stay at two (twelve values reloaded per iteration at three)."""
        w = self.waves_per_eu(v, C)
        if (isinstance(v, OCVariant) and v.L == (16, 4, 4, 3, 1, 1) and C == 1
                and self.f64
                and not self.diagonals_in_lds(v, C, nodal)
                and not (self.occupancy and (v.W, v.S) in self.occupancy)):
            w = min(w, 2)
        return w

    def diagonals_in_lds(self, v, C, nodal=False):
        """mgk_oc.h DLDS: the double one-wave static value solver of six row
        batches keeps the Jacobi diagonal and its inverse in lane-private LDS
        cells (2 R reals per lane in the [Y] region)."""
        return bool(isinstance(v, OCVariant) and v.L and v.W == 1
                    and v.R == 6 and C == 1 and not nodal and self.f64)

    # The LDS layout of a workgroup, once per solver family: (static bytes,
    # dynamic bytes) for a vector cap and an image size, ints or arrays.
    # `lds_bytes` (does a pair fit?) reads them at the image bytes as they
    # are, `_partition` (a launch's dynamic_lds) at its image cap, which is
    # rounded up to 16 bytes: the two figures differ by that rounding, as they
    # always have.  csrc/gdhost.cpp gdh_classify_oc restates `_pcap` and
    # `_oc_lds` in C++ (tests/test_host_model.py,
    # test_native_job_layout_equals_the_numpy_restatement).
    @staticmethod
    def _pcap(NP):
        """Cells of p per right-hand side (mgk_oc.h u_capacity): the rows with
        the odd stride + the dump cell, in fours."""
        return -(-(np.asarray(NP) + 1) // 4) * 4

    @staticmethod
    def _ucap(ntask):
        """Entries of U per pair slot (mgk_solver.h u_capacity): the stage-1
        tasks in whole waves + a wave of zero pad."""
        return -(-np.asarray(ntask) // 64) * 64 + 64

    def _oc_lds(self, v, C, nodal, pcap, gbytes):
        """Owner-computes solvers (mgk_oc.h).  Dynamic: [p: pcap * C reals]
        [Y: NR_y * C reals][row map: NR u32][G1][G2: gbytes each][SL: the
        LDS-resident slot values].  Static: lds_t -- red, tab_off, tab_cls,
        mm_cell."""
        rs = self.rsize
        NR = 64 * v.W * v.R
        # static layouts keep the row sums in registers: no Y region,
        # except the value + gradient solvers, which keep x there
        NR_y = 0 if ((v.L and C != 2) or v.S == 0) else NR
        if self.diagonals_in_lds(v, C, nodal):
            NR_y = 2 * NR
        dynamic = (pcap + NR_y) * C * rs + 4 * NR + 2 * np.asarray(gbytes) \
            + self.lds_slot_bytes(v, C, nodal)
        return 4 * v.W * rs + 4 * (128 if v.D > 6 else 64) + 256 + 16, dynamic

    def _two_stage_lds(self, v, C, ucap, gbytes, tab_bytes):
        """Two-stage solvers (mgk_solver.h).  Dynamic, per pair slot: [U: ucap
        * C reals][G1][G2: gbytes each], and behind the slots the microkernel
        tables.  Static: lds_t -- p (R rows per lane) and red per slot."""
        rs = self.rsize
        wpb = WPB1 if v.W == 1 else 1
        dynamic = (ucap * C * rs + 2 * np.asarray(gbytes)) * wpb + tab_bytes
        return (v.R * 64 * v.W * C * wpb + wpb * 2 * v.W) * rs, dynamic

    def lds_bytes(self, v, C, ntask=0, gbytes=0, tab_bytes=0, nodal=False):
        """LDS bytes of one workgroup: static p + scratch, dynamic U, the two
        staged graph images per pair slot and the microkernel tables."""
        if isinstance(v, OCVariant):
            static, dynamic = self._oc_lds(v, C, nodal, self._pcap(ntask),
                                           gbytes)
        else:
            static, dynamic = self._two_stage_lds(v, C, self._ucap(ntask),
                                                  gbytes, tab_bytes)
        return static + dynamic

    @staticmethod
    def slots_needed(nnz1, n2, jj, deg_sorted, W):
        """Register slots per lane that the stage-1 walk of mgk_solver.h takes
        for each job: tasks (a, i2) are dealt i2-major in batches of T = 64 W,
        and wave w of batch k walks max(1, deg2(i2 of its first task)) slots.
        Returns the maximum over the W waves."""
        T = 64 * W
        ldu = nnz1 + 1                     # padded task stride (mgk_solver.h)
        ntask = ldu * n2
        worst = np.zeros(len(nnz1), dtype=np.int64)
        nb = int(-(-ntask.max() // T)) if len(ntask) else 0
        for w in range(W):
            total = np.zeros(len(nnz1), dtype=np.int64)
            for k in range(nb):
                first = k * T + 64 * w
                live = first < ntask
                if not live.any():
                    break
                i2 = np.where(live, first // ldu, 0)
                d = np.maximum(deg_sorted[jj, i2], 1)
                total += np.where(live, d, 0)
            worst = np.maximum(worst, total)
        return worst

    @staticmethod
    def _oc_rectangles(hist1, hist2, D):
        """The sorted row order of the owner-computes walk (mgk_oc.h): rows
        by descending degree product, rectangle (d1, d2) holding hist1[d1] *
        hist2[d2] rows.  Returns (the rectangles in that order, their degree
        products + a closing 0, the cumulative row counts (n_jobs, ncp))."""
        order = sorted(((a, b) for a in range(D + 1) for b in range(D + 1)),
                       key=lambda t: -t[0] * t[1])    # stable: row-major ties
        prods = np.array([a * b for a, b in order] + [0], dtype=np.int64)
        sizes = hist1[:, [a for a, _ in order]] * hist2[:, [b for _, b in order]]
        return order, prods, np.cumsum(sizes, axis=1)

    @staticmethod
    def oc_trips(hist1, hist2, D, nb):
        """Per-batch trip counts of the one-wave owner-computes walk: entry
        [t, k] is the degree product of the first row of batch k (rows
        64 k ...) of job t in the sorted row order, 0 for batches without
        rows.  A static layout L fits job t iff trips[t, k] <= L[k] for all
        k < len(L) and the job has no rows beyond 64 len(L)."""
        order, prods, cum = SolverMenu._oc_rectangles(hist1, hist2, D)
        n = len(cum)
        if n == 0:
            return np.zeros((0, nb), dtype=np.int64)
        first = 64 * np.arange(nb, dtype=np.int64)
        # rectangle of row `first`: number of cumulative sizes <= first
        c = (cum[:, None, :] <= first[None, :, None]).sum(axis=2)
        live = first[None, :] < cum[:, -1:]
        return np.where(live, prods[np.minimum(c, len(order))], 0)

    @staticmethod
    def oc_slots_needed(hist1, hist2, W, D):
        """Slots per lane of the owner-computes walk (mgk_oc.h): rows are
        sorted by descending degree product -- rectangle (d1, d2) holds
        hist1[d1] * hist2[d2] rows -- and dealt in batches of T = 64 W, the
        64-row chunks of a batch to the waves in snake order; a wave walks, per
        batch, the product of the first row of its chunk.  `hist*`: (n_jobs,
        D + 1) degree histograms of the two graphs.  Returns the maximum over
        the waves."""
        order, prods, cum = SolverMenu._oc_rectangles(hist1, hist2, D)
        ncp = len(order)
        n = len(cum)
        if n == 0:
            return np.zeros(0, dtype=np.int64)
        N = cum[:, -1]
        T = 64 * W
        nb = int(-(-N.max() // T))
        # rectangle of the first row of every (wave, batch): one sorted search
        # over all jobs at once (row r of `cum` shifted by r * stride)
        stride = int(max(N.max(), nb * T)) + 1
        shift = np.arange(n, dtype=np.int64) * stride
        flat = (cum + shift[:, None]).ravel()
        worst = np.zeros(n, dtype=np.int64)
        kk = np.arange(nb, dtype=np.int64)
        for w in range(W):
            # (snake order of the chunks over the waves: mgk_oc.h, row_pos)
            first = kk * T + 64 * np.where(kk % 2 == 1, W - 1 - w, w)
            c = np.searchsorted(flat, (first[None, :] + shift[:, None]).ravel(),
                                side='right').reshape(n, nb) \
                - (np.arange(n, dtype=np.int64) * ncp)[:, None]
            live = first[None, :] < N[:, None]
            trip = np.where(live, prods[np.minimum(c, ncp)], 0)
            worst = np.maximum(worst, trip.sum(axis=1))
        return worst

    def classify(self, ji, jj, dgraphs, C, tab_bytes=0, gtab=False,
                 oc_only=False, nodal=False, mfma=False):
        """Assign every job the cheapest solver variant it fits.  Returns
        (variant index, cost, stage-1 tasks, image bytes, padded rows, image
        bytes incl. class ids) per job.

        Everything the assignment looks at -- node and nonzero counts, image
        sizes, the slot walks -- is a function of the two graphs' degree
        histograms (nodes are stored by descending degree) and image sizes,
        and a set of graphs has few distinct ones (about 150 among the 1000
        QM7-like molecules): large job lists are classified once per pair of
        graph classes and looked up."""
        sel, out = self._classify_classes(ji, jj, dgraphs, CallShape(
            C, nodal=nodal, tab_bytes=tab_bytes, gtab=gtab, oc_only=oc_only,
            mfma=mfma))
        out = out[:6]      # (the seventh, the larger node count, is _partition's)
        return out if sel is None else tuple(a[sel.sel] for a in out)

    def _classify_classes(self, ji, jj, dgraphs, shape, jobs=None):
        """(sel, per-class-pair results): job t has the results of class pair
        sel.sel[t] (`ClassPairs`: class-pair key per job, jobs per key); sel is
        None for short job lists (results are per job).  `jobs`: the job list
        as the (u32, u32) record array ji, jj were taken from (native path)."""
        n_jobs = len(jobs) if jobs is not None else len(ji)
        if n_jobs < 4096:
            if ji is None:
                ji, jj = jobs['i'], jobs['j']
            ji = np.asarray(ji, dtype=np.int64)
            jj = np.asarray(jj, dtype=np.int64)
            return None, self._classify_pairs(ji, jj, dgraphs, shape)
        # graphs of one degree histogram and image size are classified alike
        f = graph_features(dgraphs)
        if int(f['max_degree'].max()) < HIST_BINS - 1:
            # (the 16-bin histograms of the headers are exact)
            key = np.column_stack((f['hist'], f['image_bytes']))
        else:
            width = int(f['max_degree'].max()) + 1
            key = np.zeros((len(dgraphs), width + 1), dtype=np.int64)
            for k, g in enumerate(dgraphs):
                key[k, :width] = np.bincount(g.adjacency_count,
                                             minlength=width)
                key[k, width] = g.image_bytes
        if self.native:
            # (distinct rows through a hash table, gdh_number_records:
            # np.unique(axis=0) sorts the rows as byte strings, 0.7 ms)
            from ...hip import hostlib
            rows = np.ascontiguousarray(key)
            rows = rows.view(np.dtype((np.void, rows.shape[1]
                                       * rows.itemsize))).reshape(-1)
            cid, rep = hostlib.number_records(rows, [(0, rows.dtype.itemsize)])
        else:
            _, rep, cid = np.unique(key, axis=0, return_index=True,
                                    return_inverse=True)
        cid, nc = cid.reshape(-1).astype(np.int32), len(rep)
        if self.native and jobs is not None:
            from ...hip import hostlib
            pk, count = hostlib.pair_keys(jobs, cid, nc)
        else:
            if ji is None:
                ji, jj = jobs['i'], jobs['j']
            ji = np.asarray(ji, dtype=np.int64)
            jj = np.asarray(jj, dtype=np.int64)
            pk = cid[ji] * np.int32(nc) + cid[jj]
            count = np.bincount(pk, minlength=nc * nc)
        upk = np.flatnonzero(count)
        out = self._classify_pairs(rep[upk // nc], rep[upk % nc], dgraphs,
                                   shape)
        return ClassPairs(pk, upk, count, nc), out

    #: row batches the trip tables cover (static layouts have at most this many)
    TRIP_BATCHES = 12

    def _degree_hists(self, dgraphs, maxdeg, D, hists):
        """(distinct degree histograms H, id of every graph's) for the graphs
        of largest degree <= D (others: a zero row)."""
        if D not in hists:
            h = np.zeros((len(dgraphs), D + 1), dtype=np.int64)
            for g_, dg_ in enumerate(dgraphs):
                if maxdeg[g_] <= D:
                    h[g_] = np.bincount(dg_.adjacency_count, minlength=D + 1)
            H, hid = np.unique(h, axis=0, return_inverse=True)
            hists[D] = (H, hid.reshape(-1))
        return hists[D]

    def _trip_table(self, ji, jj, dgraphs, maxdeg, pair_maxdeg, D, hists):
        """(trips per distinct histogram pair in use, row of every job in
        that table or -1 if a graph of the job exceeds degree D)."""
        H, hid = self._degree_hists(dgraphs, maxdeg, D, hists)
        row = np.full(len(ji), -1, dtype=np.int64)
        idx = np.flatnonzero(pair_maxdeg <= D)
        h1, h2, row[idx] = self._hist_pairs(H, hid, ji, jj, idx)
        return self.oc_trips(h1, h2, D, self.TRIP_BATCHES), row

    @staticmethod
    def _hist_pairs(H, hid, ji, jj, idx):
        """The pairs of distinct degree histograms among the jobs `idx`, in
        the order of their keys: (histograms of the first graphs, of the
        second, position of every job of `idx` among the pairs).  The slot
        walk and the trip counts depend on the two histograms only, and a set
        of graphs has few distinct ones: they are evaluated once per pair."""
        nH = len(H)
        pk = hid[ji[idx]] * nH + hid[jj[idx]]
        pos = np.full(nH * nH, -1, dtype=np.int64)
        pos[pk] = 0
        upk = np.flatnonzero(pos == 0)
        pos[upk] = np.arange(len(upk))
        return H[upk // nH], H[upk % nH], pos[pk]

    def _classify_pairs(self, ji, jj, dgraphs, shape):
        C, nodal, tab_bytes, gtab = shape.C, shape.nodal, shape.tab_bytes, \
            shape.gtab
        oc_only, mfma = shape.oc_only, shape.mfma
        f = graph_features(dgraphs)
        n_node, n_nz = f['n_node'], f['n_nz']
        deg_sorted = None      # (the two-stage variants' walk: made on demand)
        n1, n2 = n_node[ji], n_node[jj]
        nnz1 = n_nz[ji]
        N = n1 * n2
        NP = n1 * (n2 | 1)                 # row space with the odd LDS stride
        # ... of a kernel that may take either graph in the first role
        # (mgk_oc.h ORIENT: grids that are not square): n1 (n2 | 1) is not
        # symmetric -- 8 x 9 is 72, 9 x 8 is 81 -- so the larger of both orders
        NP_either = np.maximum(NP, n2 * (n1 | 1))

        def rows_of(v):
            g = self.grid_of(v.L, v.D) if isinstance(v, OCVariant) else None
            return NP_either if g is not None and g[0] != g[1] else NP
        cost = n_nz[ji] * n_nz[jj] + 4 * N
        choice = np.full(len(ji), -1, dtype=np.int64)
        slots = {}
        # U entries per pair: one per stage-1 task; the region also stages the
        # CSR row pointers of both graphs during setup
        ntask = np.maximum((nnz1 + 1) * n2, n1 + n2 + 2)
        image = f['image_bytes']
        if tab_bytes:      # the label-class section is staged with the image
            image = image + class_bytes(n_node, n_nz)
        gbytes = np.maximum(image[ji], image[jj])
        # the owner-computes solvers with global tables stage the class ids
        image_oc = image + class_bytes(n_node, n_nz) if gtab else image
        # ... and, in double, the half-term records of quotient images (the
        # one-pass set-up reads them, mgk_oc.h RECS; sized for every variant)
        if gtab and self.f64 and quotient_images(dgraphs):
            image_oc = image_oc + term_bytes(n_nz)
        gbytes_oc = np.maximum(image_oc[ji], image_oc[jj])
        maxdeg = f['max_degree']
        pair_maxdeg = np.maximum(maxdeg[ji], maxdeg[jj])
        oc_slots, hists, trips = {}, {}, {}
        # (the on-the-fly kernels have every flavour of the slot kernels but
        # the static layouts)
        fly_off = False
        # `rem`: the jobs without a variant yet -- every test below runs on
        # that shrinking subset only (most jobs leave in the first variants)
        rem = np.arange(len(ji))
        # the owner-computes menu natively (gdh_classify_oc restates the
        # tests of the loop below), when it precedes every other variant
        is_oc = [isinstance(v, OCVariant) for v in self.variants]
        n_oc = sum(is_oc)
        # the layouts cut for quotient images: plain values on such images
        quot = bool(C == 1 and not nodal and quotient_images(dgraphs))

        def grid_fits(v, idx):
            """Grid rule: the pairs `idx` whose largest degrees fit the grid
            of the first batch of v's layout (mgk_oc.h GRID; implied by the
            cap of the first batch unless the grid is narrower than D)."""
            g = self.grid_of(v.L, v.D)
            if g is None:
                return np.ones(len(idx), dtype=bool)
            a, b = maxdeg[ji[idx]], maxdeg[jj[idx]]
            return (np.maximum(a, b) <= g[0]) & (np.minimum(a, b) <= g[1])
        menu = [(k, v) for k, v in enumerate(self.variants[:n_oc])
                if isinstance(v, OCVariant)
                and (not v.L or self._static_enabled(v, C, quot))
                and (v.S > 0 or not fly_off)]
        native_oc = (self.native and not tab_bytes and n_oc > 0
                     and all(is_oc[:n_oc]) and len(ji) > 0
                     and len(dgraphs) < 2**31)
        if native_oc:
            from ...hip import hostlib
            hist = f['hist']
            ch, _ = hostlib.classify_oc(
                ji, jj, n_node, n_nz, image_oc, maxdeg, hist,
                [(v.W, v.S, v.R, v.D, v.L) for _, v in menu], C,
                self.rsize, LDS_LIMIT, FLY_MIN_DEGREE,
                [self.lds_slot_bytes(v, C, nodal) for _, v in menu])
            idx = np.array([k for k, _ in menu], dtype=np.int64)
            hit = ch >= 0
            choice[hit] = idx[ch[hit]]
            rem = rem[~hit]
        for k, v in enumerate(self.variants):
            if not len(rem):
                break
            if v in (GENERAL, STREAM, MFMA) or (
                    oc_only and not isinstance(v, OCVariant)):
                continue
            if isinstance(v, OCVariant):
                if tab_bytes or native_oc:  # (table kernels: two-stage only)
                    continue
                if v.L and not self._static_enabled(v, C, quot):
                    continue
                if v.S == 0:
                    # on-the-fly: the pairs whose degrees no slot variant
                    # takes (sparse pairs that merely overflow
                    # the slots are faster in the two-stage solver: 152 against
                    # 229 us for the 118 largest pairs of configuration 2)
                    if fly_off:
                        continue
                    fits = (N[rem] <= 64 * v.W * v.R) & (NP[rem] < 0x3FFF) \
                        & (pair_maxdeg[rem] > FLY_MIN_DEGREE)
                    fits &= self.lds_bytes(v, C, NP[rem], gbytes_oc[rem],
                                           nodal=nodal) <= LDS_LIMIT
                    choice[rem[fits]] = k
                    rem = rem[~fits]
                    continue
                NPv = rows_of(v)
                fits = ((pair_maxdeg[rem] <= v.D) & (N[rem] <= 64 * v.W * v.R)
                        & (NPv[rem] < 0xFFFF))
                if not fits.any():
                    continue
                fits &= self.lds_bytes(v, C, NPv[rem], gbytes_oc[rem],
                                       nodal=nodal) <= LDS_LIMIT
                if v.L:
                    # static layout: the trip count of every batch under its
                    # segment (looked up per pair of distinct histograms)
                    if v.D not in trips:
                        trips[v.D] = self._trip_table(
                            ji, jj, dgraphs, maxdeg, pair_maxdeg, v.D, hists)
                    tr, row = trips[v.D]
                    idx = rem[fits]
                    ok = row[idx] >= 0
                    L = np.zeros(tr.shape[1], dtype=np.int64)
                    L[:v.R] = v.L
                    ok[ok] = (tr[row[idx[ok]]] <= L[None, :]).all(axis=1)
                    ok &= grid_fits(v, idx)
                    choice[idx[ok]] = k
                    fits[fits] = ok
                    rem = rem[~fits]
                    continue
                if (v.W, v.D) not in oc_slots:
                    # (once per pair of distinct histograms: _hist_pairs)
                    H, hid = self._degree_hists(dgraphs, maxdeg, v.D, hists)
                    idx = rem[pair_maxdeg[rem] <= v.D]
                    h1, h2, pos = self._hist_pairs(H, hid, ji, jj, idx)
                    sl = np.full(len(ji), np.iinfo(np.int64).max,
                                 dtype=np.int64)
                    sl[idx] = self.oc_slots_needed(h1, h2, v.W, v.D)[pos]
                    oc_slots[(v.W, v.D)] = sl
                fits &= oc_slots[(v.W, v.D)][rem] <= v.S
                choice[rem[fits]] = k
                rem = rem[~fits]
                continue
            fits = (NP[rem] <= 64 * v.W * v.R) & (NP[rem] <= 0xFFFF)
            if not fits.any():
                continue
            fits &= self.lds_bytes(v, C, ntask[rem], gbytes[rem], tab_bytes) \
                <= LDS_LIMIT
            if v.W not in slots:
                if deg_sorted is None:
                    deg_sorted = np.zeros((len(dgraphs), int(n_node.max())),
                                          dtype=np.int64)
                    for k_, g in enumerate(dgraphs):
                        deg_sorted[k_, :g.n_node] = g.adjacency_count
                sl = np.full(len(ji), np.iinfo(np.int64).max, dtype=np.int64)
                sl[rem] = self.slots_needed(nnz1[rem], n2[rem], jj[rem],
                                            deg_sorted, v.W)
                slots[v.W] = sl
            fits &= slots[v.W][rem] <= v.S
            choice[rem[fits]] = k
            rem = rem[~fits]
        if mfma and MFMA in self.variants and C == 1 and not oc_only:
            # dense pairs of small graphs under a label-blind edge kernel: the
            # dense-tile solver on the matrix cores (mgk_mfma.h) -- by the
            # rule of the dense product of the on-the-fly variants (mgk_oc.h
            # DENSE): adjacency matrices more than ~60 % full
            dense = (n1 <= MFMA_MAX_NODES) & (n2 <= MFMA_MAX_NODES) & \
                (23 * n_nz[ji] * n_nz[jj] > 9 * N * N)
            choice[dense] = self.variants.index(MFMA)
            gbytes = np.where(dense, np.maximum(f['image_bytes'][ji],
                                                f['image_bytes'][jj]), gbytes)
        if np.any(choice < 0) and oc_only:
            raise NotOwnerComputes
        if np.any(choice < 0):
            if GENERAL not in self.variants:
                bad = int(np.argmax(choice < 0))
                raise NotImplementedError(
                    f'graph pair ({ji[bad]}, {jj[bad]}) with '
                    f'{n1[bad]}x{n2[bad]} nodes and {nnz1[bad]}x'
                    f'{n_nz[jj[bad]]} adjacency nonzeros exceeds the largest '
                    'register-resident solver variant and the general '
                    'solver is disabled')
            left = choice < 0
            choice[left] = self.variants.index(GENERAL)
            if STREAM in self.variants:
                # large pairs (values, and values + analytic gradient as two
                # sequential solves): the streamed solver, if the
                # image of the smaller graph (of at most STREAM_THREADS nodes:
                # one lane per node of it) fits the LDS beside the staged
                # rows of p -- the rule of mgk_stream.h
                raw = f['image_bytes']
                # (virtual rows of the graphs these pairs touch: a pass over
                # their degree lists, only when there are such pairs)
                nv = np.zeros(len(dgraphs), dtype=np.int64)
                for g_ in np.unique(np.concatenate((ji[left], jj[left]))):
                    nv[g_] = self.stream_virtual_rows(
                        dgraphs[g_].adjacency_count) \
                        if n_node[g_] <= STREAM_THREADS else 0
                sb = self.stream_lds_bytes(raw[ji], raw[jj], n1, n2,
                                           nv[ji], nv[jj])
                fits = left & (sb + 1024 <= LDS_LIMIT)
                choice[fits] = self.variants.index(STREAM)
                # (for these pairs `gbytes` is the dynamic LDS of the pair)
                gbytes = np.where(fits, sb, gbytes)
        # (the launches size p from this: a pair keeps the larger figure if
        # its launch is merged into a square grid later)
        for k in set(choice.tolist()):
            if k >= 0 and rows_of(self.variants[k]) is NP_either:
                NP = np.where(choice == k, NP_either, NP)
        return choice, cost, ntask, gbytes, NP, gbytes_oc, np.maximum(n1, n2)

    def _partition(self, dgraphs, jobs, shape, merge_map=None):
        """Host half of a layout: solver variant per job, launch order (by
        variant, then descending cost) and launch geometry.  No device."""
        C, nodal, tab_bytes, gtab = shape.C, shape.nodal, shape.tab_bytes, \
            shape.gtab
        jobs = np.ascontiguousarray(jobs)
        jobs_sorted = None             # (set by the native ordering)
        sel, (choice, cost, ntask, gbytes, NP, gbytes_oc, nmax) = \
            self._classify_classes(None, None, dgraphs, shape, jobs=jobs)
        # Launch order: by variant, then descending cost, then job index.
        # `choice` ... `gbytes_oc` are per class pair (or per job when sel is
        # None); the jobs are ordered by the rank of their class pair with one
        # stable sort of small integers, and every per-launch maximum is taken
        # over class pairs.
        # Launches of a few thousand waves cannot fill 256 CUs for long (a pair
        # takes ~20 us from staging to result: every launch has a tail of that
        # length): their jobs ride in the next larger owner-computes variant in
        # use (same waves per pair and degree bound, S and R at least as large)
        # -- fewer, fuller launches, which matters most for the shards of a
        # multi-GPU run (scripts/minlaunch_experiment.sh: 8192 against 2048
        # waves: -1 % on the full matrix, -2...8 % on 1/2...1/8 of it).
        applied = {}                   # launch merging of this job list
        if merge_map is not None:
            # decided elsewhere, on a larger job list this one is a shard of
            # (_sharded.ShardPlan.merge_map)
            for k, k2 in merge_map.items():
                choice = np.where(choice == k, k2, choice)
            applied = dict(merge_map)
        elif self.min_launch > 0:
            members_ = np.ones(len(choice), dtype=np.int64) if sel is None \
                else sel.members
            used_ = sorted(set(choice.tolist()))
            for a_, k in enumerate(used_):
                v = self.variants[k]
                if not isinstance(v, OCVariant):
                    continue
                here = choice == k
                if int(members_[here].sum()) * v.W >= self.min_launch:
                    continue
                for k2 in used_[a_ + 1:]:
                    v2 = self.variants[k2]
                    if not (isinstance(v2, OCVariant) and v2.W == v.W
                            and v2.D == v.D and v2.S >= v.S and v2.R >= v.R):
                        continue
                    # a static layout takes the jobs of another static layout
                    # it dominates batch by batch, first-batch grid included: a
                    # 12-first launch may ride in a 16-first layout, never the
                    # reverse (never those of a dynamic variant); a dynamic
                    # variant takes any total <= S
                    if v2.L and not (v.L and all(
                            a <= b for a, b in zip(v.L, v2.L))
                            and self._grid_takes(v2, v)):
                        continue
                    choice = np.where(here, k2, choice)
                    # (chains collapse: what rode in k now rides in k2)
                    for k0, k1 in list(applied.items()):
                        if k1 == k:
                            applied[k0] = k2
                    applied[k] = k2
                    break
        choice = self._fit_launches_into_lds(choice, shape, NP, ntask, gbytes,
                                             gbytes_oc)
        rank_of = np.empty(len(choice), dtype=np.int64)
        by_rank = np.lexsort((-cost, choice))
        # class pairs of equal (variant, cost) share a rank: their jobs stay
        # in job order, as if every job had been sorted by itself
        step = np.ones(len(choice), dtype=np.int64)
        step[1:] = (choice[by_rank[1:]] != choice[by_rank[:-1]]) | \
            (cost[by_rank[1:]] != cost[by_rank[:-1]])
        rank_of[by_rank] = np.cumsum(step) - 1
        if sel is None:
            order_all = by_rank.astype(np.uint32)   # (lexsort is stable)
            members = np.ones(len(choice), dtype=np.int64)
        elif self.native:
            # stable counting sort of the jobs by the rank of their class pair
            from ...hip import hostlib
            rank_of_key = np.full(sel.nc * sel.nc, -1, dtype=np.int32)
            rank_of_key[sel.upk] = rank_of
            order_all, jobs_sorted = hostlib.order_jobs(
                sel.pk, rank_of_key, int(rank_of.max()) + 1, jobs)
            members = sel.members
        else:
            rank = rank_of[sel.sel]
            rank = rank.astype(np.uint16 if len(choice) <= 0xFFFF
                               else np.uint32)
            order_all = np.argsort(rank, kind='stable').astype(np.uint32)
            members = sel.members
        used = sorted(set(choice.tolist()))
        launches, cursor = [], 0
        for k in used:
            v = self.variants[k]
            idx = np.flatnonzero(choice == k)      # class pairs (or jobs)
            count = int(members[idx].sum())
            if v == GENERAL:
                # one workgroup per pair, CG vectors + U in global scratch
                # (rows N <= padded rows NP)
                per_wg = int(((3 * NP[idx] + ntask[idx]) * C).max())
                geo = dict(ucap=per_wg, gcap=0, dynamic_lds=0, grid=None,
                           threads=GENERAL_THREADS, per_wg=per_wg)
            elif v == MFMA:
                # one wave per pair; dynamic LDS: the two images
                gcap = int(-(-gbytes[idx].max() // 16) * 16)
                geo = dict(ucap=0, gcap=gcap, dynamic_lds=2 * gcap, grid=count,
                           threads=64)
            elif v == STREAM:
                # one to 256 workgroups per pair; scratch [x | r | p | Ap |
                # diag (| second solution)] (N <= NP reals each); LDS: image
                # of B | staged rows of p | partial sums
                per_wg = int((6 if C == 2 else 5) * NP[idx].max())
                dyn = int(-(-gbytes[idx].max() // 16) * 16)
                # (the pairs' costs in launch order, largest first: `prepare`
                # picks the workgroups per pair from them)
                # (a tuple: launch descriptions are compared as values)
                costs = tuple(np.sort(np.repeat(cost[idx], members[idx])
                                      .astype(np.float64))[::-1].tolist())
                geo = dict(ucap=per_wg, gcap=dyn, dynamic_lds=dyn, costs=costs,
                           grid=None, threads=STREAM_THREADS, per_wg=per_wg)
            elif isinstance(v, OCVariant):
                # one pair per workgroup; dynamic LDS: p | row sums | row map
                # | two images (mgk_oc.h)
                pcap = int(self._pcap(NP[idx].max()))
                gcap = int(-(-gbytes_oc[idx].max() // 16) * 16)
                dyn = int(self._oc_lds(v, C, nodal, pcap, gcap)[1])
                dense = False
                if v.S == 0:
                    # on-the-fly variants: the dense n x n edge-record arrays
                    # of both graphs (mgk_oc.h DENSE), sized for the largest
                    # graph of the call -- when they fit (F_DENSE tells the
                    # kernel that they are there)
                    extra = self._dense_bytes(dgraphs, int(nmax[idx].max()))
                    if extra and dyn + extra + 4096 <= LDS_LIMIT:
                        # (+ 4 cells of p: the last trip of a row of the
                        # dense product reads up to three cells past it)
                        pcap += 4
                        dyn += extra + 4 * C * self.rsize
                        dense = True
                geo = dict(
                    ucap=pcap, gcap=gcap, dynamic_lds=dyn,
                    grid=int(max(1, -(-count // self.jobs_per_unit))),
                    threads=64 * v.W, tab=gtab, dense=dense)
            else:
                wpb = WPB1 if v.W == 1 else 1
                # Many small workgroups (jobs_per_unit pairs per wave, default
                # one) rather than one persistent grid: the hardware
                # dispatcher then balances the load whatever the achieved
                # residency is, and a launch of few jobs (a rare variant, one
                # rank's shard of a multi-GPU run) still covers the chip.
                # Measured: 1 pair per wave = 8 per wave + 1 % on 500 500
                # pairs, + 28 % on 61 000.
                grid = int(max(1, -(-count // (wpb * self.jobs_per_unit))))
                ucap = int(self._ucap(ntask[idx].max()))
                gcap = int(-(-gbytes[idx].max() // 16) * 16)
                dyn = int(self._two_stage_lds(v, C, ucap, gcap,
                                              tab_bytes)[1])
                geo = dict(ucap=ucap, gcap=gcap, dynamic_lds=dyn, grid=grid,
                           threads=64 * v.W * wpb)
            launches.append(dict(variant=v, k=k, offset=cursor, count=count,
                                 **geo))
            cursor += count
        out = Partition((jobs, used, order_all, launches))
        out.jobs_sorted, out.merge_map = jobs_sorted, applied
        return out

    def _launch_lds(self, v, shape, NP, ntask, gbytes, gbytes_oc):
        """LDS of a workgroup -- static and dynamic, `lds_bytes` -- of ONE
        launch of variant `v` over the given class pairs (or jobs): the
        regions are sized for the largest vector and the largest image among
        them -- two maxima that need not belong to one pair."""
        if isinstance(v, OCVariant):
            return int(self.lds_bytes(v, shape.C, int(NP.max()),
                                      int(gbytes_oc.max()),
                                      nodal=shape.nodal))
        return int(self.lds_bytes(v, shape.C, int(ntask.max()),
                                  int(gbytes.max()), shape.tab_bytes))

    def _fit_launches_into_lds(self, choice, shape, NP, ntask, gbytes,
                               gbytes_oc):
        """Every pair was given a variant whose LDS regions hold IT; a launch
        sizes its regions for the largest vector and the largest graph image
        among its pairs, and the two can come from different pairs: the sum
        went 0.5 KB over the 160 KB of a CU for the 16-wave double variant
        with LDS-resident slot values on 45...62-node graphs, and 2.4 KB over
        for the 16-wave two-stage variant (64 KB of it static) on a list of
        170 mixed graphs -- invalid launches, scripts/fuzz_parity.py seeds 23
        and 51.  Pairs that hold one of the two maxima of such a launch leave
        for the general solver until the launch fits."""
        fallback = None
        for k in sorted(set(choice.tolist())):
            v = self.variants[k]
            if k < 0 or v in (GENERAL, STREAM, MFMA):
                continue
            while True:
                idx = np.flatnonzero(choice == k)
                if not len(idx) or self._launch_lds(
                        v, shape, NP[idx], ntask[idx], gbytes[idx],
                        gbytes_oc[idx]) <= LDS_LIMIT:
                    break
                if fallback is None:
                    if shape.oc_only or GENERAL not in self.variants:
                        raise NotOwnerComputes(
                            f'the pairs of variant {v} do not fit the LDS '
                            'of a compute unit together and the general '
                            'solver is not available to this call')
                    fallback = self.variants.index(GENERAL)
                big_p = NP[idx] if isinstance(v, OCVariant) else ntask[idx]
                big_g = gbytes_oc[idx] if isinstance(v, OCVariant) \
                    else gbytes[idx]
                # drop whichever maximum frees more bytes per pair dropped
                cand = []
                for key in (big_p, big_g):
                    out = idx[key == key.max()]
                    keep = np.setdiff1d(idx, out)
                    after = self._launch_lds(
                        v, shape, NP[keep], ntask[keep], gbytes[keep],
                        gbytes_oc[keep]) if len(keep) else 0
                    cand.append((after, len(out), out))
                after, _, out = min(cand, key=lambda c: (c[0], c[1]))
                choice = choice.copy()
                choice[out] = fallback
        return choice
