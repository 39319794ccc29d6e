"""tests/dispatch_instances.py against the host code it restates: the table of instances equals the macro invocation lists of
molann_amd/csrc/*.inc (an instance added to a ladder without a case in the table fails here), the ranges tile the frame sizes, and
the restated arithmetic gives each listed instance at both ends of its range and its neighbour one step beyond.  No GPU."""

import os
import re

import pytest

import dispatch_instances as di

CSRC = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "molann_amd", "csrc")


def _read(name):
    with open(os.path.join(CSRC, name)) as f:
        return f.read()


def _invocations(text, macro):
    """The argument tuples of every invocation of `macro` (its #define has names, not numbers, for arguments)."""
    return [tuple(int(v) for v in m.split(",")) for m in re.findall(r"\b%s\(([\d, ]+)\)" % macro, text)]


LAUNCH, CAPI, JIT, CREATE = (_read(n) for n in ("molann_host_launch.inc", "molann_capi.inc", "molann_host_jit.inc", "molann_host_create.inc"))


def _group_vjp_instances():
    """The frames per round group_vjp_geometry tries: from b0 (halved while a round has more than 256 items) down to its floor."""
    m = re.search(r"int b0 = (\d+);\s*while \(b0 > (\d+) && \(long\)b0 \* n_items > (\d+)\) b0 /= 2;\s*for \(int b = b0; b >= (\d+); b /= 2\)", JIT)
    assert m, "group_vjp_geometry no longer has the form this test reads"
    top, floor_, per_round, floor2 = (int(v) for v in m.groups())
    assert floor_ == floor2 and per_round == 256
    out, b = [], top
    while b >= floor_:
        out.append((b,))
        b //= 2
    return out


SOURCES = {
    "ALIGN_REGS_CASE": lambda: _invocations(LAUNCH, "ALIGN_REGS_CASE"),
    "ALIGN_BWD_CASE": lambda: _invocations(CAPI, "ALIGN_BWD_CASE"),
    "ALIGN_BATCH_CASE": lambda: _invocations(LAUNCH, "ALIGN_BATCH_CASE"),
    "LAUNCH_RING": lambda: _invocations(LAUNCH, "LAUNCH_RING"),
    "LAUNCH_GROUP_BWD": lambda: _invocations(CAPI, "LAUNCH_GROUP_BWD"),
    "LAUNCH_WAVE": lambda: _invocations(LAUNCH, "LAUNCH_WAVE"),
    "molann_group_vjp": _group_vjp_instances,
}


@pytest.mark.parametrize("ladder", di.LADDERS)
def test_table_equals_the_dispatch_list(ladder):
    listed = SOURCES[ladder]()
    assert listed and len(set(listed)) == len(listed), (ladder, listed)
    table = [i.args for i in di.instances(ladder)]
    assert len(set(table)) == len(table), (ladder, table)
    assert set(table) == set(listed), (ladder, "only in the table", sorted(set(table) - set(listed)), "only in the source", sorted(set(listed) - set(table)))


def test_the_ladders_are_the_seven_of_the_sources():
    assert set(di.LADDERS) == set(SOURCES) == {i.ladder for i in di.TABLE}
    assert len(_invocations(LAUNCH, "ALIGN_REGS_CASE")) == 15 and len(_invocations(CAPI, "ALIGN_BWD_CASE")) == 15
    assert len(_invocations(LAUNCH, "ALIGN_BATCH_CASE")) == 7 and len(_invocations(LAUNCH, "LAUNCH_RING")) == 25


def test_every_instance_has_both_edges_or_a_reason():
    """Taking an instance's case out of the table fails here (or above, when the whole instance goes)."""
    names = [i.name for i in di.TABLE]
    assert len(set(names)) == len(names)
    for i in di.TABLE:
        if i.unreachable is not None:
            assert not i.edges and len(i.unreachable) > 20, i
            continue
        assert len(i.edges) == 2 and i.edges[0].size != i.edges[1].size, i
        for e in i.edges:
            assert e.how and isinstance(e.env, dict), (i, e)
            if i.lo is not None:
                assert i.lo <= e.size and (i.hi is None or e.size <= i.hi), (i, e)
    # the register and batch kernels: the last size of a range is the exactly-full one and is an edge; the first size is an edge
    # unless the lane kernel takes such frames (then the first size beyond it)
    for i in di.instances("ALIGN_REGS_CASE") + di.instances("ALIGN_BWD_CASE"):
        w, u = i.args
        assert i.hi == 64 * w * 4 * u and i.edges[1].size == i.hi and i.edges[1].end == "full", i
        first = di.FIRST_BEYOND_LANE if i.ladder == "ALIGN_REGS_CASE" else di.FIRST_DENSE_GRADIENT
        assert i.edges[0].size == max(i.lo, first), i
    for i in di.instances("ALIGN_BATCH_CASE"):
        u, b = i.args
        assert b * i.hi == 64 * 4 * u and i.edges[1].size == i.hi and i.edges[0].size == max(i.lo, 4), i
    for i in di.instances("LAUNCH_RING"):
        nd, nb = i.args
        assert (i.lo, i.hi) == di.ring_window_range(nd) and i.hi == 64 * nd - 1, i
        assert [e.size for e in i.edges] == [max(i.lo, di.RING_FEWEST_WINDOWS), i.hi], i


def test_constants_of_the_ladders():
    """The numbers the restated ladders share with the sources."""
    assert "p->n_inp <= 384 && getenv(\"MOLANN_NO_ALIGN_BATCH\") == nullptr" in LAUNCH and di.BATCH_MAX_ATOMS == 384
    assert LAUNCH.count("p->n_inp <= 24 * 512") == 1 and CAPI.count("p->n_inp <= 24 * 512") == 1 and di.REGS_MAX_ATOMS == 24 * 512
    assert LAUNCH.count("(p->n_inp + 64 * W - 1) / (64 * W) > 24") == 1 and CAPI.count("(p->n_inp + 64 * W - 1) / (64 * W) > 24") == 1
    assert "while (nb > 4 && nb * p->n_inp > 1536) nb /= 2;" in LAUNCH
    assert "const int units = per_lane <= 8 ? 2 : (per_lane <= 16 ? 4 : 6);" in LAUNCH
    m = re.search(r"static const int buckets\[\] = \{([\d, ]+)\};", CREATE)
    assert m and tuple(int(v) for v in m.group(1).split(",")) == di.RING_BUCKETS
    assert {nd for nd, _ in _invocations(LAUNCH, "LAUNCH_RING")} == set(di.RING_BUCKETS)
    assert "int nb = (p->n_align > 0 && nd <= 4) ? 8 / nd : 1;" in LAUNCH and "if (nd == 3) nb = 2;" in LAUNCH
    assert "int pre = (mode == 1 || p->n_items <= 64) ? 0 : (p->n_items <= 128 ? 2 : 4);" in LAUNCH
    assert "while (nb > 1 && (long)nb * p->n_items > 256) nb /= 2;" in CAPI
    assert "const bool lane_tables_fit = d->n_align <= 64 && (long)d->n_inp * 768 <= 65536;" in CREATE


@pytest.mark.parametrize("ladder,fn,top", [("ALIGN_REGS_CASE", di.regs_wu, di.REGS_MAX_ATOMS), ("ALIGN_BWD_CASE", di.regs_wu, di.REGS_MAX_ATOMS),
                                           ("ALIGN_BATCH_CASE", di.batch_ub, di.BATCH_MAX_ATOMS)])
def test_ranges_tile_the_frame_sizes(ladder, fn, top):
    rows = sorted(di.instances(ladder), key=lambda i: i.lo)
    assert rows[0].lo == 1 and rows[-1].hi == top
    for a, b in zip(rows, rows[1:]):
        assert b.lo == a.hi + 1, (a, b)                     # no gap, no overlap
    assert fn(0) is None and fn(top + 1) is None
    for k, i in enumerate(rows):
        assert fn(i.lo) == i.args and fn(i.hi) == i.args, i
        assert fn(i.lo - 1) == (rows[k - 1].args if k else None), i
        assert fn(i.hi + 1) == (rows[k + 1].args if k + 1 < len(rows) else None), i
        assert all(fn(n) == i.args for n in range(i.lo, i.hi + 1, 7)), i


def test_register_ranges_are_the_documented_ones():
    got = {i.args: (i.lo, i.hi) for i in di.instances("ALIGN_REGS_CASE")}
    assert got == {(1, 1): (1, 256), (1, 2): (257, 512), (1, 3): (513, 768), (1, 4): (769, 1024), (1, 5): (1025, 1280), (1, 6): (1281, 1536),
                   (2, 4): (1537, 2048), (2, 5): (2049, 2560), (2, 6): (2561, 3072), (4, 4): (3073, 4096), (4, 5): (4097, 5120),
                   (4, 6): (5121, 6144), (8, 4): (6145, 8192), (8, 5): (8193, 10240), (8, 6): (10241, 12288)}
    assert got == {i.args: (i.lo, i.hi) for i in di.instances("ALIGN_BWD_CASE")}
    assert {i.args: (i.lo, i.hi) for i in di.instances("ALIGN_BATCH_CASE")} == {
        (2, 16): (1, 32), (4, 16): (33, 64), (6, 16): (65, 96), (4, 8): (97, 128), (6, 8): (129, 192), (4, 4): (193, 256), (6, 4): (257, 384)}


def test_alignment_routes_reach_the_listed_instance():
    """With the edge's switches and each alignment set size the GPU cases use, the restated route names the instance; without the
    switch (or with a small alignment set where a large one is the way) it names another kernel."""
    for ladder in ("ALIGN_REGS_CASE", "ALIGN_BATCH_CASE"):
        for i, e in di.cases(ladder):
            for n_al in di.align_set_sizes(i, e):
                assert di.align_forward_name(e.size, n_al, no_align_batch="MOLANN_NO_ALIGN_BATCH" in e.env) == i.name, (i, e, n_al)
            if e.env:
                assert di.align_forward_name(e.size, 3) != i.name, (i, e)
            if di.BIG_ALIGN in e.how:
                assert di.align_forward_name(e.size, 3) == "frames_lane_kernel<0,align_out>", (i, e)
    for i, e in di.cases("ALIGN_BWD_CASE"):
        for n_al in di.align_set_sizes(i, e):
            assert di.align_backward_name(e.size, n_al) == i.name, (i, e, n_al)
    # the lane kernel's reach: what makes 53 and 27 atoms the first sizes of the mid-frame kernels
    assert di.lane_serves_alignment(52, 26) and not di.lane_serves_alignment(53, 26) and not di.lane_serves_alignment(32, 65)
    assert di.lane_serves_dense_gradient(26, 13) and not di.lane_serves_dense_gradient(27, 13)
    assert di.align_forward_name(12289, 3) == "frames_wave_kernel<pre=0>" and di.align_backward_name(12289, 3) == "frames_wave_bwd"
    assert di.align_forward_name(700, 3, no_ring=True) == "frames_wave_kernel<pre=0>"


def test_ring_window_counts_select_the_listed_instance():
    for i, e in di.cases("LAUNCH_RING"):
        nd, nb = i.args
        n_inp, touched = di.ring_plan(e.size)
        win = di.compact_windows(touched, n_inp)
        assert len(win) == e.size and len(set(win)) == e.size, (i, e)
        assert win[-1] == 3 * n_inp - 4 and touched[-1] == n_inp - 1, (i, e)       # the last window is the clamped one, on the last atom
        assert win[0] == 3 * touched[0], (i, e)
        assert di.ring_nd(e.size) == nd, (i, e)
        batch = int(e.env["MOLANN_RING_BATCH"]) if "MOLANN_RING_BATCH" in e.env else None
        assert di.ring_nb(nd, 40, batch) == nb, (i, e)
        assert di.ring_nb(nd, 0, None) == (2 if nd == 3 else 1) and di.ring_nb(nd, 0, 1) == 1
    for k, nd in enumerate(di.RING_BUCKETS):
        lo, hi = di.ring_window_range(nd)
        assert di.ring_nd(lo) == nd and di.ring_nd(hi) == nd and di.ring_nd(hi + 1) == nd           # 64 ND itself: an even count, never made
        if k:
            assert di.ring_nd(lo - 1) == di.RING_BUCKETS[k - 1]
        assert di.ring_nd(hi + 2) == (di.RING_BUCKETS[k + 1] if k + 1 < len(di.RING_BUCKETS) else 0)
    assert len(di.compact_windows([0, 2], 8)) == 3          # an even cover gets its last window twice
    with pytest.raises(ValueError):
        di.ring_plan(64)


def test_small_ladders_select_the_listed_instance():
    for i, e in di.cases("LAUNCH_GROUP_BWD"):
        assert di.group_bwd_name(di.group_bwd_b(e.size)) == i.name, (i, e)
    assert [di.group_bwd_b(n) for n in (32, 33, 64, 65, 128, 129)] == [8, 4, 4, 2, 2, None]
    for i, e in di.cases("LAUNCH_WAVE"):
        env = int(e.env["MOLANN_WAVE_PRE"]) if "MOLANN_WAVE_PRE" in e.env else None
        assert di.wave_name(di.wave_pre(e.size, 0, env)) == i.name, (i, e)
    assert [di.wave_pre(n) for n in (64, 65, 128, 129)] == [0, 2, 2, 4] and di.wave_pre(500, mode=1) == 0
    assert [di.wave_pre(10, 0, v) for v in (0, 1, 2, 3, 4, 9)] == [0, 1, 2, 2, 4, 4]
    for i, e in di.cases("molann_group_vjp"):
        assert di.group_vjp_name(di.group_vjp_b(e.size)) == i.name, (i, e)
    assert [di.group_vjp_b(n) for n in (32, 33, 64, 65, 1000)] == [8, 4, 4, 2, 2]
    # both sides of every threshold are edges
    for ladder, sizes in (("LAUNCH_GROUP_BWD", {32, 33, 64, 65, 128}), ("LAUNCH_WAVE", {64, 65, 128, 129}), ("molann_group_vjp", {32, 33, 64, 65})):
        assert sizes <= {e.size for _, e in di.cases(ladder)}, ladder
