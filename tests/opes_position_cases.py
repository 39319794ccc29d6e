"""Cases in which the GEOMETRY of the deposit block decides the answer (tests/test_opes_position_f64_host.py proves on the CPU that each
takes the path it names, tests/test_gpu_opes_position_f64.py runs them on opes_deposit_f64_kernel and opes_step_f64_kernel): which of
the 256 threads holds a search's winner (its lane, its wave, its stride k = t, t + 256, ...), where two bit-equal distances sit in the
butterfly, in the four LDS slots and in one thread's strides, which partial sums a pair term travels through, table sizes at the edges
of a wave and of a stride, and a chain that runs `store` and `move` between barriers hundreds of times.

The LATTICE table of n kernels: column 0 holds i + 0.1 (u - 0.5), the other columns 0, widths 0.3 (0.9 + 0.2 u) per column, heights
0.5 + u, no period; cutoff 5, threshold 1, capacity 600.  Neighbours are about 3.3 widths apart (q = 11: no merge) and share pair
terms of about 5e-3, so one term lost from S is some 1e9 bounds.

A `Case` is one table and ONE deposit, with what must come out stated independently of the host twin: the counts, the exact height of
every slot that takes a kernel (a fold of IEEE additions in the order of the deposit) and the slots the oracle's history must show.
`reference(case)` runs the host twin and the oracle once per case and keeps them."""

import math

import torch

import opes_deposit_cases as cases
import opes_deposit_oracle as oracle
import opes_run_cases as rc

F64 = torch.float64
CAP, CUTOFF, THRESHOLD = 600, 5.0, 1.0
FAR, FAR_WIDTH, NEW_HEIGHT = -100.0, 0.6, 0.5
# 9/16: FAR + OFFSET is exact, so a kernel OFFSET away in column 0 and one OFFSET away in column 1 are at bit-equal q (0.55 is not
# representable next to -100: the two q would differ in the last places and no tie rule would be asked)
OFFSET = 0.5625
TIE_PAIRS = [(0, 1), (3, 35), (63, 64), (10, 200), (200, 260), (255, 256), (7, 263), (263, 519), (300, 511)]
TRIPLE = (200, 260, 519)
SIZES = [0, 1, 2, 63, 64, 65, 255, 256, 257, 511, 512, 513]
_REFERENCE = {}


def lattice_table(n, d, seed=0):
    g = torch.Generator().manual_seed(52000 + 10 * n + d + seed)
    centers = torch.zeros(n, d, dtype=F64)
    centers[:, 0] = torch.arange(n, dtype=F64) + 0.1 * (torch.rand(n, dtype=F64, generator=g) - 0.5)
    sigma = 0.3 * (0.9 + 0.2 * torch.rand(n, d, dtype=F64, generator=g))
    heights = 0.5 + torch.rand(n, dtype=F64, generator=g)
    return centers, sigma, heights


class Case(object):
    """`table`, `new`: (centers, sigma, heights); `counts`: (n, merges, refused) after the deposit; `heights`: {slot: exact height};
    `takers`: the taker slot of every new kernel's FIRST search in order (None: appended); `tie`: None, "exact" (the first search's two
    best are bit-equal), "near" (one ulp apart) or "all" (a tie in every search); `chains`: the chain rounds the oracle must record."""

    def __init__(self, label, d, table, new, counts, heights, takers, capacity=CAP, threshold=THRESHOLD, tie=None, chains=0):
        self.label, self.d, self.table, self.new, self.counts, self.heights, self.takers = label, d, table, new, counts, heights, takers
        self.capacity, self.threshold, self.tie, self.chains = capacity, threshold, tie, chains

    @property
    def n0(self):
        return self.table[0].shape[0]


def _next_to(table, slots, heights):
    """Kernel i 0.1 from the centre of slot slots[i] in column 0, with that slot's widths."""
    centers = table[0][slots].clone()
    centers[:, 0] += 0.1
    return centers, table[1][slots].clone(), heights


def _fold(table, slots, heights):
    """{slot: its height after taking the kernels that name it, added one after the other}."""
    out = {}
    for slot, h in zip(slots, heights.tolist()):
        out[slot] = out.get(slot, float(table[2][slot])) + h
    return out


# ---------------------------------------------------------------------------------------------- 1. a winner at every position
def every_position(d):
    """520 new kernels in one deposit, kernel i next to slot perm[i]: every thread, wave and stride holds a winner once."""
    table = lattice_table(520, d)
    g = torch.Generator().manual_seed(610 + d)
    perm = torch.randperm(520, generator=g).tolist()
    new = _next_to(table, perm, 0.5 + torch.rand(520, dtype=F64, generator=g))
    return Case("every_position_d%d" % d, d, table, new, (520, 520, 0), _fold(table, perm, new[2]), perm)


# ---------------------------------------------------------------------------------------------- 2. exact ties and near ties
def _far_row(d, column, offset):
    row = torch.zeros(d, dtype=F64)
    row[0] = FAR
    row[column] += offset
    return row


def tie(mode, pair, d):
    """Slots a < b of the 520-kernel table moved next to FAR with widths 0.6, and one new kernel at FAR.  plain: a at +0.5, b at -0.5;
    mirror: the signs swapped; columns: a OFFSET away in column 0, b in column 1; near: plain with b one ulp nearer, so b must win."""
    a, b = pair
    centers, sigma, heights = lattice_table(520, d)
    if mode == "columns":
        centers[a], centers[b] = _far_row(d, 0, OFFSET), _far_row(d, 1, OFFSET)
    else:
        sign = -1.0 if mode == "mirror" else 1.0
        centers[a], centers[b] = _far_row(d, 0, 0.5 * sign), _far_row(d, 0, -0.5 * sign)
        if mode == "near":
            centers[b, 0] = math.nextafter(float(centers[b, 0]), FAR)
    sigma[a], sigma[b] = FAR_WIDTH, FAR_WIDTH
    taker = b if mode == "near" else a
    new = (_far_row(d, 0, 0.0)[None], torch.full((1, d), FAR_WIDTH, dtype=F64), torch.tensor([NEW_HEIGHT], dtype=F64))
    table = (centers, sigma, heights)
    expect = {a: float(heights[a]), b: float(heights[b])}
    expect[taker] += NEW_HEIGHT
    return Case("tie_%s_%d_%d_d%d" % (mode, a, b, d), d, table, new, (520, 1, 0), expect, [taker], tie="near" if mode == "near" else "exact")


def triple_tie():
    """Three slots OFFSET from FAR in columns 0, 1 and 2: the first must take the kernel; the other two then tie again, past the threshold."""
    d = 8
    centers, sigma, heights = lattice_table(520, d)
    for column, slot in enumerate(TRIPLE):
        centers[slot], sigma[slot] = _far_row(d, column, OFFSET), FAR_WIDTH
    new = (_far_row(d, 0, 0.0)[None], torch.full((1, d), FAR_WIDTH, dtype=F64), torch.tensor([NEW_HEIGHT], dtype=F64))
    expect = {slot: float(heights[slot]) for slot in TRIPLE}
    expect[TRIPLE[0]] += NEW_HEIGHT
    return Case("tie_triple_d8", d, (centers, sigma, heights), new, (520, 1, 0), expect, [TRIPLE[0]], tie="all")


def tie_cases():
    out = [tie(mode, pair, d) for d in (1, 8) for mode in ("plain", "mirror", "near") for pair in TIE_PAIRS]
    return out + [tie("columns", pair, 8) for pair in TIE_PAIRS] + [triple_tie()]


# ---------------------------------------------------------------------------------------------- 3. table-size edges
def size_edge(n0, d):
    """Four kernels in one deposit: next to slot 0, slot n0 - 1 and slot n0 // 2 (where there are such slots) and a fresh one."""
    table = lattice_table(n0, d)
    slots = [0, n0 - 1, n0 // 2] if n0 else []
    g = torch.Generator().manual_seed(730 + 10 * n0 + d)
    h = 0.5 + torch.rand(len(slots) + 1, dtype=F64, generator=g)
    near = _next_to(table, slots, h[:-1])
    fresh = torch.zeros(1, d, dtype=F64)
    fresh[0, 0] = n0 + 4.0
    new = (torch.cat([near[0], fresh]), torch.cat([near[1], torch.full((1, d), 0.3, dtype=F64)]), h)
    expect = _fold(table, slots, h[:-1])
    expect[n0] = float(h[-1])
    return Case("size_%d_d%d" % (n0, d), d, table, new, (n0 + 1, len(slots), 0), expect, slots + [None])


# ---------------------------------------------------------------------------------------------- 4. a chain through the whole table
def whole_table_chain(d):
    """300 kernels under a threshold of 1000 widths: one new kernel next to slot 150 and the table collapses into one kernel, 299 of the
    300 merges being chain rounds that store, move the last row into the hole and search again."""
    table = lattice_table(300, d)
    new = _next_to(table, [150], torch.tensor([1.0], dtype=F64))
    case = Case("chain_d%d" % d, d, table, new, (1, 300, 0), {}, [150], capacity=320, threshold=1e3, chains=299)
    case.total_height = math.fsum(table[2].tolist() + [1.0])       # what slot 0 holds in the end
    return case


# ---------------------------------------------------------------------------------------------- the references
def reference(case):
    """(S of the table before, the host twin after the deposit, the oracle after it), once per case."""
    if case.label not in _REFERENCE:
        total0 = cases.brute_force_S(*case.table, None, CUTOFF)
        host = cases.HostTable(case.capacity, case.d, None, CUTOFF, case.threshold).fill(*case.table, total0).deposit(*case.new)
        ref = oracle.Oracle(case.capacity, case.d, None, CUTOFF, case.threshold).fill(*case.table).deposit(*case.new)
        _REFERENCE[case.label] = (total0, host, ref)
    return _REFERENCE[case.label]


def assert_takes_its_path(case):
    """On the oracle and the host twin alone: the counts, the takers of every first search, the chain rounds, the margins of every
    search that is no tie on purpose, the exact heights, and the twin's table and S against the oracle and the brute force."""
    _, host, ref = reference(case)
    assert host.counts() == ref.counts() == case.counts, (case.label, host.counts(), ref.counts(), case.counts)
    firsts = [h[1] if h[0] == "merge" else None for h in ref.history if h[0] in ("merge", "append")]
    assert firsts == case.takers, (case.label, firsts[:8], case.takers[:8])
    assert sum(1 for h in ref.history if h[0] == "chain") == case.chains and ref.refused == 0, case.label
    assert min([m[0] for m in ref.margins], default=math.inf) >= 1e-9, case.label       # an empty table is not searched
    gaps = [m[1] for m in ref.margins] or [math.inf]
    if case.tie == "exact":
        assert gaps[0] == 0.0 and min(gaps[1:]) >= 1e-9, (case.label, gaps)
    elif case.tie == "near":
        assert 0.0 < gaps[0] < 1e-12 and min(gaps[1:]) >= 1e-9, (case.label, gaps)
    elif case.tie == "all":
        assert gaps[0] == 0.0 and len(gaps) == 2, (case.label, gaps)
    else:
        assert min(gaps) >= 1e-9, (case.label, min(gaps))
    n = ref.n
    for slot, h in case.heights.items():
        assert float(host.heights[slot]) == h, (case.label, slot)
    cases.assert_tables_close(n, (host.centers, host.sigma, host.heights), (ref.centers, ref.sigma, ref.heights), case.label)
    brute = cases.brute_force_S(host.centers[:n], host.sigma[:n], host.heights[:n], None, CUTOFF)
    ratio = abs(float(host.state[1]) - brute) / (cases.S_BOUND * max(1.0, ref.A))
    assert ratio <= 1.0, (case.label, float(host.state[1]), brute, ref.A)
    return ratio, ref


# ---------------------------------------------------------------------------------------------- 6. a step with many walkers
WALKER_COUNTS = [65, 257, 300]


def invalid_walkers(W):
    """(the walker whose V is NaN, the one whose y is NaN, the one whose exp overflows): wave 2 and the second stride where W reaches
    them, else the last walker (wave 1, or lane 0 of the second stride) and a lane in the middle of wave 0."""
    nan_v = 130 if W > 130 else W - 1
    nan_y = 259 if W > 259 else (256 if W > 256 else 33)
    return nan_v, nan_y, 0


def many_walkers(W):
    """A step of W walkers, d = 1, on the 60-kernel lattice table from a run that has not started: the outputs are fresh lattice points
    (all appended), V in [-3, 0), three walkers invalid.  Returns (table, y [W, 1], V [W], the invalid walkers, sigma0 [1])."""
    table = lattice_table(60, 1)
    g = torch.Generator().manual_seed(860 + W)
    y = (65.0 + torch.arange(W, dtype=F64) + 0.1 * (torch.rand(W, dtype=F64, generator=g) - 0.5)).reshape(W, 1)
    V = -3.0 * torch.rand(W, dtype=F64, generator=g)
    bad = invalid_walkers(W)
    V[bad[0]], y[bad[1], 0], V[bad[2]] = math.nan, math.nan, 1000.0
    return table, y, V, bad, rc.sigma0_row(1)


def host_walker_run(W):
    """The host twin's step of `many_walkers(W)`: (HostRun, the case)."""
    case = many_walkers(W)
    table, y, V, _, sigma0 = case
    host = rc.HostRun(CAP, 1, None, CUTOFF, THRESHOLD, sigma0, None, False)
    host.table.fill(*table, cases.brute_force_S(*table, None, CUTOFF))
    host.step(y, V)
    return host, case


def walker_sums(W):
    """(valid walkers, sum of exp(beta V), sum of its squares) over the valid walkers by math.fsum."""
    _, _, V, bad, _ = many_walkers(W)
    w = [math.exp(rc.BETA * v) for a, v in enumerate(V.tolist()) if a not in bad]
    return len(w), math.fsum(w), math.fsum(x * x for x in w)


# ---------------------------------------------------------------------------------------------- 5. the density at every d
def density_case(d):
    """300 kernels in [-1, 1)^d under `mixed_period`, widths near 0.3 sqrt(d) per kernel (so that q does not grow with d and most kernels
    lie inside the cutoff), and 5 points, each 0.1 from a kernel's centre.  Returns (points, centers, heights, sigma, period)."""
    g = torch.Generator().manual_seed(940 + d)
    centers = 2.0 * torch.rand(300, d, dtype=F64, generator=g) - 1.0
    heights = 0.5 + torch.rand(300, dtype=F64, generator=g)
    sigma = 0.3 * math.sqrt(d) * (0.8 + 0.4 * torch.rand(300, d, dtype=F64, generator=g))
    points = centers[[0, 77, 150, 223, 299]] + 0.1
    return points, centers, heights, sigma, cases.mixed_period(d)
