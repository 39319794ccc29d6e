"""tests/lane_rounds.py without a GPU: the launch infos it reads, the tile model against the dealing written another way, the size rule's
own promises for every ring the float32 lane kernels are launched with, the base of 251 frames in every lane of every slot, and the
comparer on float32 stand-ins - a correct per-frame function passes, planted ring faults that no batch of one generation per block
shows are named with their place in the ring.  This is what shows that tests/test_gpu_lane_rounds.py can fail."""

import math

import pytest
import torch

import f64_rounds as fr
import lane_rounds as lr

RING_INFOS = [
    ("molann_lane_jit<NL=2> (plan-specialised; 14 consumer waves + 2 loader, ring of 16 tiles) grid=256 block=1024 lds=160000",
     lr.Ring("molann_lane_jit<NL=2>", 14, 2, 16, 256, 1024)),
    ("molann_lane_jit<align_out> (plan-specialised; 3 consumer waves + 1 loader, ring of 5 tiles) grid=7 block=256 lds=99",
     lr.Ring("molann_lane_jit<align_out>", 3, 1, 5, 7, 256)),
    ("molann_lane_jit<NL=3,wide> (plan-specialised; 8 consumer waves + 2 loader, ring of 9 tiles, 41 KB of weights resident) grid=256 block=640 lds=1",
     lr.Ring("molann_lane_jit<NL=3,wide>", 8, 2, 9, 256, 640)),
    ("molann_bwd_ring (plan-specialised; 6 consumer waves + 2 loader, ring of 12 tiles) grid=256 block=512 lds=5 + reduce_rows_kernel",
     lr.Ring("molann_bwd_ring", 6, 2, 12, 256, 512)),
    ("molann_bwd_ring<values> (plan-specialised; 6 consumer waves + 2 loader, ring of 12 tiles) grid=1 block=512 lds=5",
     lr.Ring("molann_bwd_ring<values>", 6, 2, 12, 1, 512)),
]


def test_the_base_and_the_comparer_are_the_float64_files():
    assert lr.BASE == fr.BASE == 251 and lr.repeated is fr.repeated and lr.wrong_frames is fr.wrong_frames


@pytest.mark.parametrize("info,want", RING_INFOS, ids=[w.kind for _, w in RING_INFOS])
def test_ring_launch_infos_are_read(info, want):
    assert lr.geometry(info) == want and lr.units_of(want) == want.grid


def test_ahead_of_time_launch_infos_are_read():
    g = lr.geometry("frames_lane_kernel<2,features_regs> grid=2048 block=128 lds=20480")
    assert g == lr.Stride("frames_lane_kernel<2,features_regs>", 2048, 128, 2, 64, False) and lr.units_of(g) == 4096
    assert lr.geometry("mlp_lane_kernel<NL=2> grid=1024 block=256 lds=3")[1:] == (1024, 256, 4, 64, False)
    assert lr.geometry("mlp_mfma_kernel<f32> grid=1024 block=256 lds=3")[1:] == (1024, 256, 4, 16, False)
    chain = ("molann_lane_jit<NL=0> (plan-specialised; 14 consumer waves + 2 loader, r || molann_mlp_bwd (plan-specialised) grid=256 block=256"
             " + reduce_rows_kerne || molann_lane_bwd (plan-specialised) grid=512 block=256 || chunks of 1048576 frames")
    found = lr.geometries(chain)                      # the first kernel's geometry is cut off by the info's 72 characters per launch
    assert [g.kind for g in found] == ["molann_mlp_bwd", "molann_lane_bwd"] and found[0].by_block and not found[1].by_block
    assert (found[0].grid, found[0].waves, found[1].grid, found[1].waves) == (256, 4, 512, 4)
    with pytest.raises(AssertionError):
        lr.geometry(chain)
    with pytest.raises(AssertionError):
        lr.geometry("frames_wave_kernel<pre=0> grid=8 block=256 mode=0")


@pytest.mark.parametrize("grid", [1, 2, 255, 256, 1024])
def test_every_tile_goes_to_exactly_one_block(grid):
    nslot = 4
    counts = sorted({1, max(1, grid - 1), grid, grid + 1, 2 * grid - 1, 3 * grid + 7, grid * (2 * nslot + 1) + max(1, grid // 3)})
    for n_tiles in counts:
        for ragged in (1, 37, 64):
            n = 64 * (n_tiles - 1) + ragged
            model = lr.tile_model(n, grid, nslot)
            assert model.n_tiles == n_tiles and sorted(model) == list(range(grid))
            assert sorted(t for tiles in model.values() for t in tiles) == list(range(n_tiles))
            # the dealing written another way: tile t -> block t mod grid, as that block's (t div grid)-th
            assert all(tiles == list(range(b, n_tiles, grid)) for b, tiles in model.items())
            assert max(len(v) for v in model.values()) - min(len(v) for v in model.values()) <= 1
            for f in {0, 63, 64, n // 2, n - 1}:
                if f < n:
                    b, k, slot, gen, lane = model.where(f)
                    assert model[b][k] == f // 64 and lane == f % 64 and (slot, gen) == (k % nslot, k // nslot)
    with pytest.raises(AssertionError):
        model.where(n)


@pytest.mark.parametrize("nload", [1, 2])
@pytest.mark.parametrize("nslot", list(range(2, 17)))
def test_the_size_rule_keeps_its_promises(nslot, nload):
    for grid in (2, 256, 304):
        s = lr.batch_size(grid, nslot)
        G = s.generations
        assert G == 2 and s.n_tiles == grid * (G * nslot + 1) + s.extra and s.n == 64 * (s.n_tiles - 1) + 37 <= 1 << 21
        assert math.gcd(251, 64 * grid * nslot) == 1 and 1 <= s.extra < grid
        model = lr.tile_model(s.n, grid, nslot)
        sizes = [len(model[b]) for b in range(grid)]
        assert set(sizes) == {G * nslot + 1, G * nslot + 2}, "some blocks own one tile more than others, none two"
        assert min(sizes) // nslot == G == lr.full_generations(s.n, grid, nslot), "every block fills its ring twice"
        last = s.n_tiles - 1
        b, k, slot, gen, lane = model.where(s.n - 1)
        assert model[b][-1] == last and k == len(model[b]) - 1, "the ragged tile is its block's last"
        assert gen == G and lane == 36 and slot == k % nslot == 1, "and lies in the third generation, counting from zero"
        assert len(model[b]) == max(sizes) and b == s.extra - 1
        # every block is in generation G when the launch ends, none beyond it
        assert {model.where(64 * model[bb][-1])[3] for bb in range(grid)} == {G}
        # the loaders share a block's tiles; in the blocks with the smaller count the second loader has none in the last generation
        for n_b in set(sizes):
            parts = lr.loader_tiles(n_b, nload)
            assert sorted(n for p in parts for n in p) == list(range(n_b)) and all(p == list(range(j, n_b, nload)) for j, p in enumerate(parts))


def test_the_size_rule_refuses_what_it_cannot_keep():
    with pytest.raises(AssertionError):
        lr.batch_size(1024, 16)                       # beyond 2^21 frames: fail, never fewer generations
    with pytest.raises(AssertionError):
        lr.batch_size(251, 4)                         # copies of the base would line up with the blocks
    with pytest.raises(AssertionError):
        lr.batch_size(1, 4)                           # one block has no neighbours
    with pytest.raises(AssertionError):
        lr.batch_size(256, 1)


@pytest.mark.parametrize("units,tiles", [((4096,), (64,)), ((2048,), (64,)), ((4096,), (16,)), ((1024, 256, 2048), (64, 64, 64)),
                                         ((4096, 1024, 256, 2048), (64, 64, 64, 64)), ((6,), (64,))])
def test_the_size_rule_of_the_grid_stride_kernels(units, tiles):
    s = lr.stride_size(units, tiles)
    assert s.n == 64 * (s.n_tiles - 1) + 37 and s.nslot == 1
    for u, t in zip(units, tiles):
        n_t = -(-s.n // t)
        iterations = [len(range(w, n_t, u)) for w in range(u)]          # the kernels' loop, literally
        assert min(iterations) >= 2 and max(iterations) == min(iterations) + 1, (u, t, min(iterations), max(iterations))
        assert lr.full_generations(s.n, u, 1, t) == min(iterations)
        assert s.n % t != 0, "the last tile is ragged"
    lead = max(u * t // 64 for u, t in zip(units, tiles))
    assert s.n_tiles == 2 * lead + s.extra and s.n_tiles // lead == 2, "the widest kernel runs two full iterations and part of a third"


@pytest.mark.parametrize("grid,nslot", [(2, 2), (5, 3), (256, 16), (256, 9), (304, 11)])
def test_every_lane_of_every_slot_and_generation_sees_several_base_frames(grid, nslot):
    s = lr.batch_size(grid, nslot)
    f = torch.arange(s.n)
    t, lane = f // 64, f % 64
    k = t // grid                                      # the tile's number in its block: slot k % nslot, generation k // nslot
    key = k * 64 + lane
    n_keys = int(key.max()) + 1
    lo = torch.full((n_keys,), 10 ** 6).scatter_reduce(0, key, f % lr.BASE, "amin")
    hi = torch.full((n_keys,), -1).scatter_reduce(0, key, f % lr.BASE, "amax")
    blocks = torch.zeros(n_keys, dtype=torch.long).scatter_add(0, key, torch.ones_like(key))     # how many blocks run this (tile, lane)
    assert int((blocks > 0).sum()) == 64 * (s.generations * nslot + 1) + (64 if s.extra > 1 else 37)
    several = blocks >= 2
    assert bool((hi[several] > lo[several]).all()), "a (slot, generation, lane) that only ever sees one base frame"
    if grid >= 4:                                      # (fewer blocks: the longer blocks' last tile, or its lanes past 37, run in one block only)
        assert s.extra >= 3 and bool(several[blocks > 0].all())


def test_a_nan_with_another_payload_is_a_wrong_row():
    base = torch.randn((lr.BASE, 5), generator=torch.Generator().manual_seed(3), dtype=torch.float32)
    base[17, 2] = float("nan")
    long = lr.repeated(base, 1000).clone()
    assert lr.wrong_frames({"out": long}, {"out": base}) == []
    bits = long.view(torch.int32)
    assert bits[17 + 2 * lr.BASE, 2] == bits[17, 2] and math.isnan(float(long[17 + 2 * lr.BASE, 2]))
    bits[17 + 2 * lr.BASE, 2] ^= 0x5                  # still NaN, another payload
    assert math.isnan(float(long[17 + 2 * lr.BASE, 2]))
    assert lr.wrong_frames({"out": long}, {"out": base}) == [17 + 2 * lr.BASE]


# ---- the comparer on stand-ins of a ring -------------------------------------------------------------------------------------------
GRID, NSLOT = 5, 3
W = torch.randn((6, 4), generator=torch.Generator().manual_seed(5), dtype=torch.float32)


def _g(rows):
    return torch.tanh(rows @ W) + 2.0


def correct(x, grid=GRID):
    return {"out": _g(x)}


def refills_a_slot_one_generation_early(x, grid=GRID):
    """done[s] is not waited for: the consumers of lanes 60 .. 63 of a block's tile n find the block's tile n + NSLOT in the slot"""
    out = _g(x).clone()
    model = lr.tile_model(x.shape[0], grid, NSLOT)
    for b, tiles in model.items():
        for n, t in enumerate(tiles):
            if n + NSLOT < len(tiles):
                src = 64 * tiles[n + NSLOT]
                for lane in range(60, 64):
                    if src + lane < x.shape[0]:
                        out[64 * t + lane] = _g(x[src + lane:src + lane + 1])[0]
    return {"out": out}


def ragged_tile_keeps_the_slots_old_rows(x, grid=GRID):
    """the ragged tile in a reused slot: the lanes past its end are live from the slot's previous tile and overwrite that tile's rows"""
    out = _g(x).clone()
    model = lr.tile_model(x.shape[0], grid, NSLOT)
    live = x.shape[0] - 64 * (model.n_tiles - 1)
    b, n, slot, gen, _ = model.where(x.shape[0] - 1)
    if gen > 0 and live < 64:
        prev = model[b][n - NSLOT]
        out[64 * prev + live:64 * prev + 64] = 0.0
    return {"out": out}


def the_longer_blocks_drop_their_last_tile(x, grid=GRID):
    """n_b computed as the smallest block's: the blocks that own one tile more never store it"""
    out = _g(x).clone()
    model = lr.tile_model(x.shape[0], grid, NSLOT)
    shortest = min(len(v) for v in model.values())
    for tiles in model.values():
        for t in tiles[shortest:]:
            out[64 * t:64 * t + 64] = float("nan")
    return {"out": out}


FAULTS = [refills_a_slot_one_generation_early, ragged_tile_keeps_the_slots_old_rows, the_longer_blocks_drop_their_last_tile]


def _batches():
    s = lr.batch_size(GRID, NSLOT)
    base = torch.randn((lr.BASE, 6), generator=torch.Generator().manual_seed(9), dtype=torch.float32)
    return s, base, lr.repeated(base, s.n)


def test_a_correct_function_passes():
    s, base, x = _batches()
    assert x.shape[0] == s.n == 64 * (GRID * 7 + s.extra - 1) + 37 and s.extra == 3
    assert lr.wrong_frames(correct(x), correct(base)) == []
    assert lr.explain([], GRID, NSLOT, s.n) == "no frame wrong"


@pytest.mark.parametrize("fault", FAULTS, ids=[f.__name__ for f in FAULTS])
def test_a_planted_ring_fault_is_named_with_its_place(fault):
    s, base, x = _batches()
    one_generation = x[:64 * GRID * NSLOT]            # every block fills its ring once, evenly, no ragged tile: what the shorter tests run
    got, want = fault(one_generation), correct(one_generation)
    assert torch.equal(got["out"].view(torch.int32), want["out"].view(torch.int32)), "visible within one generation"
    got = fault(base, grid=-(-lr.BASE // 64))
    assert torch.equal(got["out"].view(torch.int32), correct(base)["out"].view(torch.int32)), "visible in the base launch"
    wrong = lr.wrong_frames(fault(x), correct(base))
    assert wrong
    model = lr.tile_model(s.n, GRID, NSLOT)
    where = [model.where(f) for f in wrong]
    text = lr.explain(wrong, GRID, NSLOT, s.n)
    assert text.startswith("%d frames wrong (grid %d, ring of %d" % (len(wrong), GRID, NSLOT))
    assert "frame %d: block %d, tile %d of the block, slot %d, generation %d, lane %d" % ((wrong[0],) + where[0]) in text
    if fault is refills_a_slot_one_generation_early:
        assert {w[4] for w in where} == {60, 61, 62, 63} and {w[3] for w in where} == {0, 1}
        assert len(wrong) == 4 * sum(max(0, len(t) - NSLOT) for t in model.values()) - 4      # (the ragged source tile has no lanes 60 .. 63)
    elif fault is ragged_tile_keeps_the_slots_old_rows:
        assert wrong == list(range(64 * model[s.extra - 1][-1 - NSLOT] + 37, 64 * model[s.extra - 1][-1 - NSLOT] + 64))
        assert {w[3] for w in where} == {s.generations - 1} and {w[2] for w in where} == {1}
    else:
        assert {w[0] for w in where} == set(range(s.extra)) and {w[1] for w in where} == {s.generations * NSLOT + 1}
        assert len(wrong) == 64 * (s.extra - 1) + 37
