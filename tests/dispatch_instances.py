"""The host-side dispatch ladders of the mid- and large-frame kernels, restated in Python, and the table of their instances.

Frames the lane kernels do not take are served by ahead-of-time template families; an `if` ladder on the frame's size picks one
instance per plan (molann_amd/csrc/molann_host_launch.inc: launch_pre; molann_capi.inc: launch_wave_bwd; molann_host_jit.inc:
group_vjp_geometry; molann_host_create.inc: choose_ring).  Every instance is separately compiled code with its own tail, so a test
that means to cover a family has to reach every instance, at the sizes where its tail differs: the first size of its range (the
register kernels: one atom in the last four register slots; the ring: one window in the last LDS-DMA instruction) and the last
(every register slot full; the last instruction one window short of full).

This module has no GPU code and imports nothing but the standard library:

* the arithmetic of each ladder (`regs_wu`, `batch_ub`, `lane_serves_alignment`, `compact_windows`, `ring_nd`, `ring_nb`, `wave_pre`,
  `group_bwd_b`, `group_vjp_b`) and the names `last_launch_info` prints (`*_name`);
* `ring_plan(n_win)`: the touched atoms of a frame whose compact image has exactly `n_win` windows;
* `TABLE`: every instance of the seven ladders with its range, the edges a test must run and the way to reach each edge - the plan
  shape and, where the default route never gets there, the documented product switch - or the reason why nothing reaches it.

tests/test_dispatch_instances_host.py holds the table against the macro lists of the C++ sources; tests/test_gpu_dispatch_instances.py
runs every reachable (instance, edge)."""

import collections

REGS_MAX_ATOMS = 24 * 512                                   # frames_align_regs_kernel / frames_align_bwd_regs_kernel: 8 waves x 64 lanes x 24 atoms
BATCH_MAX_ATOMS = 384                                       # frames_align_batch_kernel
LDS_BYTES = 163840
FB_STRIDE = 65
RING_BUCKETS = (1, 2, 3, 4, 6, 8, 10, 12, 14, 16, 18, 20, 22, 24, 26, 28, 30, 32)


def _ceil_div(a, b):
    return -(-a // b)


def _ceil_to(a, b):
    return _ceil_div(a, b) * b


# ---- who serves AlignmentLayer.forward and its gradient ---------------------------------------------------------------------
def lane_geometry_ok(tile_bytes, cols):
    """lane_geometry (molann_host_plan.inc): a wave's dense tile + staging rows, at least four waves per CU in blocks of <= 64 KiB."""
    per_wave = _ceil_to(tile_bytes, 16) + _ceil_to(cols * FB_STRIDE * 4, 16)
    best = 0
    for wpb in (4, 3, 2, 1):
        if wpb * per_wave > 65536:
            continue
        best = max(best, min(32, wpb * (LDS_BYTES // (wpb * per_wave))))
    return best >= 4


def lane_serves_alignment(n_inp, n_align):
    """geom[1] of choose_family: the lane kernel's `align_out` form takes the frame (its tables hold <= 64 alignment entries)."""
    return 0 < n_align <= 64 and n_inp * 768 <= 65536 and lane_geometry_ok(64 * n_inp * 12, 1)


def lane_serves_dense_gradient(n_inp, n_align):
    """geom[0] of the plan AlignmentLayer.forward makes under autograd (one position item per atom: 3 n_inp feature columns)."""
    return n_align <= 64 and n_inp * 768 <= 65536 and 3 * n_inp <= 128 and lane_geometry_ok(64 * n_inp * 12, 3 * n_inp)


def regs_wu(n_inp):
    """(W, U) of frames_align_regs_kernel and frames_align_bwd_regs_kernel: the fewest data waves with <= 24 atoms per thread, the
    atoms per thread in fours; None beyond 12 288 atoms."""
    if not 1 <= n_inp <= REGS_MAX_ATOMS:
        return None
    w = 1
    while _ceil_div(n_inp, 64 * w) > 24:
        w *= 2
    return w, _ceil_div(_ceil_div(n_inp, 64 * w), 4)


def batch_ub(n_inp):
    """(U, B) of frames_align_batch_kernel: rounds of the most frames (16, 8, 4) with B n_inp <= 1536 atoms; None beyond 384 atoms."""
    if not 1 <= n_inp <= BATCH_MAX_ATOMS:
        return None
    nb = 16
    while nb > 4 and nb * n_inp > 1536:
        nb //= 2
    per_lane = _ceil_div(nb * n_inp, 64)
    return (2 if per_lane <= 8 else (4 if per_lane <= 16 else 6)), nb


def regs_name(wu):
    return "frames_align_regs_kernel<W=%d,U=%d>" % wu


def bwd_regs_name(wu):
    return "frames_align_bwd_regs_kernel<W=%d,U=%d>" % wu


def batch_name(ub):
    return "frames_align_batch_kernel<U=%d,B=%d>" % ub


def align_forward_name(n_inp, n_align, no_align_batch=False, no_ring=False):
    """What last_launch_info names after AlignmentLayer.forward (molann_align_f32 -> launch_pre, mode 1)."""
    if lane_serves_alignment(n_inp, n_align):
        return "frames_lane_kernel<0,align_out>"            # (or its plan-specialised twin, molann_lane_jit<align_out>)
    if not no_ring and n_inp <= BATCH_MAX_ATOMS and not no_align_batch:
        return batch_name(batch_ub(n_inp))
    if not no_ring and n_inp <= REGS_MAX_ATOMS:
        return regs_name(regs_wu(n_inp))
    return "frames_wave_kernel<pre=0>"


def align_backward_name(n_inp, n_align):
    """What last_launch_info names after the dense gradient of AlignmentLayer.forward (distinct alignment atoms)."""
    if lane_serves_dense_gradient(n_inp, n_align):
        return "lane"
    if n_inp <= REGS_MAX_ATOMS:
        return bwd_regs_name(regs_wu(n_inp))
    return "frames_wave_bwd"


# ---- frames_ring_kernel ------------------------------------------------------------------------------------------------------
def compact_windows(slot_atoms, n_inp):
    """compact_windows (molann_host_jit.inc): first dword of each 16-byte window of the frame's compact image - a greedy cover of the
    touched dwords, the last window clamped to the frame's end, an odd number of windows."""
    frame_dw = 3 * n_inp
    used = [False] * frame_dw
    for a in slot_atoms:
        used[3 * a] = used[3 * a + 1] = used[3 * a + 2] = True
    win = []
    for d in range(frame_dw):
        if not used[d] or (win and d < win[-1] + 4):
            continue
        win.append(min(d, frame_dw - 4))
    if not win:
        win.append(0)
    if len(win) % 2 == 0:
        win.append(win[-1])
    return win


def ring_nd(n_win):
    """choose_ring's bucket: LDS-DMA instructions per frame, the first of the list with 64 ND >= the window count; 0: not served."""
    for b in RING_BUCKETS:
        if 64 * b >= n_win:
            return b
    return 0


def ring_nb(nd, n_align, ring_batch=None):
    """Frames per ring entry (launch_pre): with an alignment as many as keep an entry within 8 KB; MOLANN_RING_BATCH caps it.
    ND = 3 takes two frames per entry whether or not the plan has an alignment: without the switch <ND=3> alone is never chosen."""
    nb = 8 // nd if (n_align > 0 and nd <= 4) else 1
    if nd == 3:
        nb = 2
    if ring_batch is not None and 1 <= ring_batch < nb:
        nb = 4 if ring_batch >= 4 else (2 if ring_batch >= 2 else 1)
    if nd * nb > 8:
        nb = 1
    return nb


def ring_name(nd, nb):
    return "frames_ring_kernel<ND=%d>" % nd if nb == 1 else "frames_ring_kernel<ND=%d,B=%d>" % (nd, nb)


def ring_window_range(nd):
    """(first, last) window count of bucket ND.  compact_windows makes every count odd, so the largest is 64 ND - 1: the last
    LDS-DMA instruction of a frame is never full."""
    prev = ([0] + list(RING_BUCKETS))[RING_BUCKETS.index(nd)]
    return 64 * prev + 1, 64 * nd - 1


RING_FEWEST_WINDOWS = 25


def ring_plan(n_win):
    """(n_inp, touched atoms, in frame order) of a frame whose compact image has exactly n_win windows (n_win odd).  Every other
    atom of a frame of 2 n_win - 1 atoms: one window per atom, the first window holds atom 0 and the last - clamped to the frame's
    end - the frame's last atom.  The ring serves plans the lane kernels refuse, which touch more than 32 atoms of more than 52: 33
    adjacent atoms at the end of a 53-atom frame make the fewest windows such a plan can have, RING_FEWEST_WINDOWS."""
    if n_win % 2 == 0 or n_win < RING_FEWEST_WINDOWS:
        raise ValueError("no plan of the ring kernel has %d windows" % n_win)
    if n_win == RING_FEWEST_WINDOWS:
        return 53, list(range(20, 53))
    if n_win < 33:
        raise ValueError("window counts between %d and 33 are not constructed here" % RING_FEWEST_WINDOWS)
    return 2 * n_win - 1, list(range(0, 2 * n_win - 1, 2))


# ---- the small ladders -------------------------------------------------------------------------------------------------------
def wave_pre(n_items, mode=0, wave_pre_env=None):
    """frames_wave_kernel<pre>: item rounds loaded with the alignment atoms; MOLANN_WAVE_PRE (read once per process) overrides."""
    pre = 0 if (mode == 1 or n_items <= 64) else (2 if n_items <= 128 else 4)
    if wave_pre_env is not None and wave_pre_env >= 0:
        pre = wave_pre_env
    return 4 if pre >= 4 else (2 if pre >= 2 else pre)


def wave_name(pre):
    return "frames_wave_kernel<pre=%d>" % pre


def group_bwd_b(n_items):
    """frames_group_bwd_kernel<B>: frames per wave and round, at most 256 items per round; None: one frame (the gather kernel)."""
    nb = 8
    while nb > 1 and nb * n_items > 256:
        nb //= 2
    return nb if nb > 1 else None


def group_bwd_name(b):
    return "frames_group_bwd_kernel<B=%d>" % b


def group_vjp_b(n_items):
    """molann_group_vjp<B>: the first B group_vjp_geometry tries (it halves B further only where 160 KiB of LDS do not hold the
    plan's tables at one wave per block)."""
    b = 8
    while b > 2 and b * n_items > 256:
        b //= 2
    return b


def group_vjp_name(b):
    return "molann_group_vjp<B=%d>" % b


# ---- the table ---------------------------------------------------------------------------------------------------------------
# An edge: the size that selects the instance (atoms, windows or items), which end of the range it is, the environment the route
# needs ({} = the default route) and the shape of the plan in words.
Edge = collections.namedtuple("Edge", "size end env how")
# An instance: ladder, the name last_launch_info prints, its template arguments, the range of sizes the ladder's arithmetic gives
# it, the edges to run (empty: unreachable) and the reason where nothing reaches it.
Instance = collections.namedtuple("Instance", "ladder name args lo hi edges unreachable")

NO_BATCH = {"MOLANN_NO_ALIGN_BATCH": "1"}
NO_RING = {"MOLANN_NO_RING": "1"}
BIG_ALIGN = "an alignment set of 65 entries (atoms named more than once): past the lane kernel's tables"
FIRST_BEYOND_LANE = 53                                      # lane_serves_alignment holds up to 52 atoms
SMALL_LADDER_ATOMS = 60                                     # the frame of the small ladders' cases (more than 32 atoms touched: no lane plan)
FIRST_DENSE_GRADIENT = 27                                   # lane_serves_dense_gradient holds up to 26 atoms (a 64-frame tile + 78 staging rows)


def _ranges(fn, top):
    """{instance: (lo, hi)} of a ladder over sizes 1..top, and the sizes in order (to check that the ranges tile)."""
    out = collections.OrderedDict()
    for n in range(1, top + 1):
        k = fn(n)
        lo, hi = out.get(k, (n, n))
        out[k] = (min(lo, n), max(hi, n))
    return out


def _align_regs_instances():
    rows = []
    for (w, u), (lo, hi) in _ranges(regs_wu, REGS_MAX_ATOMS).items():
        assert hi == 64 * w * 4 * u                         # the last size of a range is the exactly-full one
        edges = []
        for size, end in ((max(lo, FIRST_BEYOND_LANE), "first"), (hi, "full")):
            if size <= BATCH_MAX_ATOMS:
                edges.append(Edge(size, end, NO_BATCH, "AlignmentLayer.forward of %d atoms with MOLANN_NO_ALIGN_BATCH=1" % size))
            else:
                edges.append(Edge(size, end, {}, "AlignmentLayer.forward of %d atoms" % size))
        rows.append(Instance("ALIGN_REGS_CASE", regs_name((w, u)), (w, u), lo, hi, tuple(edges), None))
    return rows


def _align_bwd_instances():
    rows = []
    for (w, u), (lo, hi) in _ranges(regs_wu, REGS_MAX_ATOMS).items():
        edges = tuple(Edge(size, end, {}, "gradient of AlignmentLayer.forward of %d atoms" % size)
                      for size, end in ((max(lo, FIRST_DENSE_GRADIENT), "first"), (hi, "full")))
        rows.append(Instance("ALIGN_BWD_CASE", bwd_regs_name((w, u)), (w, u), lo, hi, edges, None))
    return rows


def _align_batch_instances():
    rows = []
    for (u, b), (lo, hi) in _ranges(batch_ub, BATCH_MAX_ATOMS).items():
        assert b * hi == 64 * 4 * u                         # full: the round's atoms fill every register slot of the data wave
        edges = []
        for size, end in ((max(lo, 4), "first"), (hi, "full")):
            if size < FIRST_BEYOND_LANE:
                edges.append(Edge(size, end, {}, "AlignmentLayer.forward of %d atoms, %s" % (size, BIG_ALIGN)))
            else:
                edges.append(Edge(size, end, {}, "AlignmentLayer.forward of %d atoms" % size))
        rows.append(Instance("ALIGN_BATCH_CASE", batch_name((u, b)), (u, b), lo, hi, tuple(edges), None))
    return rows


def _ring_instances():
    rows = []
    for nd in RING_BUCKETS:
        lo, hi = ring_window_range(nd)
        first = max(lo, RING_FEWEST_WINDOWS)
        for nb in (8, 4, 2, 1):
            if nd * nb > 8 and nb > 1:
                continue
            if nd == 3 and nb == 4:                         # (no such instance: 3 x 4 KB entries would pass 8 KB)
                continue
            default_nb = ring_nb(nd, 1)
            if nb == default_nb:
                env, how = {}, "features behind an alignment"
            elif nb == 1:
                env, how = {"MOLANN_RING_BATCH": "1"}, "features without an alignment; behind one with MOLANN_RING_BATCH=1"
            else:
                env, how = {"MOLANN_RING_BATCH": str(nb)}, "features behind an alignment with MOLANN_RING_BATCH=%d" % nb
            if nd >= 6 or (nd, nb) == (3, 2):
                how = "features with and without an alignment"
            if (nd, nb) == (3, 1):
                how = "features with and without an alignment, both with MOLANN_RING_BATCH=1"
            edges = tuple(Edge(size, end, env, "%d windows: %s" % (size, how)) for size, end in ((first, "first"), (hi, "last")))
            rows.append(Instance("LAUNCH_RING", ring_name(nd, nb), (nd, nb), lo, hi, edges, None))
    return rows


def _small_instances():
    # item counts: both sides of every threshold; an instance with one threshold only gets the other end of its range (B = 8 and
    # pre = 0: a single item), or a size past its last preloaded round (pre = 4: 256 items are four rounds) / a second size (B = 2)
    rows = []
    for b, lo, hi in ((8, 1, 32), (4, 33, 64), (2, 65, 128)):
        edges = tuple(Edge(size, end, {}, "backward of %d feature items on %d atoms behind a 40-atom alignment" % (size, SMALL_LADDER_ATOMS))
                      for size, end in ((lo, "first"), (hi, "last")))
        rows.append(Instance("LAUNCH_GROUP_BWD", group_bwd_name(b), (b,), lo, hi, edges, None))
    for pre, lo, hi in ((0, 1, 64), (2, 65, 128), (4, 129, None)):
        edges = tuple(Edge(size, end, NO_RING, "features of %d items on %d atoms with MOLANN_NO_RING=1" % (size, SMALL_LADDER_ATOMS))
                      for size, end in ((lo, "first"), (hi or 257, "last" if hi else "past")))
        rows.append(Instance("LAUNCH_WAVE", wave_name(pre), (pre,), lo, hi, edges, None))
    switch = dict(NO_RING, MOLANN_WAVE_PRE="1")              # (read once per process: such a case runs in a process of its own)
    rows.append(Instance("LAUNCH_WAVE", wave_name(1), (1,), None, None,
                         tuple(Edge(size, "switch", switch, "features of %d items in a process started with MOLANN_WAVE_PRE=1 and MOLANN_NO_RING=1" % size)
                               for size in (64, 65)), None))
    for b, lo, hi in ((8, 1, 32), (4, 33, 64), (2, 65, None)):
        edges = tuple(Edge(size, end, {}, "values and forces of %d feature items on %d atoms behind a 40-atom alignment" % (size, SMALL_LADDER_ATOMS))
                      for size, end in ((lo, "first"), (hi or 128, "last" if hi else "past")))
        rows.append(Instance("molann_group_vjp", group_vjp_name(b), (b,), lo, hi, edges, None))
    return rows


TABLE = tuple(_align_regs_instances() + _align_bwd_instances() + _align_batch_instances() + _ring_instances() + _small_instances())
LADDERS = ("ALIGN_REGS_CASE", "ALIGN_BWD_CASE", "ALIGN_BATCH_CASE", "LAUNCH_RING", "LAUNCH_GROUP_BWD", "LAUNCH_WAVE", "molann_group_vjp")


def align_set_sizes(instance, edge):
    """Alignment set sizes a case runs: 3 atoms and half the frame (at most 400 forward, 300 backward: the sizes of
    test_large_frame_alignment_in_registers and test_dense_alignment_gradient); 65 entries where only that reaches the instance."""
    if BIG_ALIGN in edge.how:
        return [65]
    return [3, min(300 if instance.ladder == "ALIGN_BWD_CASE" else 400, edge.size // 2)]


def instances(ladder):
    return [i for i in TABLE if i.ladder == ladder]


def cases(ladder):
    """[(instance, edge)] of a ladder's reachable instances."""
    return [(i, e) for i in instances(ladder) for e in i.edges]


def case_id(instance, edge):
    return "%s-%s%d" % (instance.name.split("_kernel")[-1].replace("molann_group_vjp", "").strip("<>").replace("=", "").replace(",", "_"),
                        edge.end, edge.size)
