"""tests/f64_rounds.py without a GPU: the size rule against a literal model of the kernels' grid-stride loop, for every geometry the
float64 one-launch kernels are launched with, and the comparer on torch stand-ins - a correct per-frame function passes, three
planted faults, each bit-identical to it on a batch of one round per block, are named with their first wrong frame in a later round.
This is what shows that tests/test_gpu_f64_rounds.py can fail."""

import math

import pytest
import torch

import f64_rounds as fr
import test_gpu_frame_isolation as fi

# (lanes per frame, block): the four lane groups at four waves per block, and the stepped-down blocks of two waves and of one
GEOMETRIES = [(8, 256), (16, 256), (32, 256), (64, 256), (64, 128), (64, 64)]


def test_the_base_is_the_isolation_files():
    assert fr.BASE == fi.BASE == 251


def test_the_launch_info_is_read_by_the_isolation_files_pattern():
    info = "frames_value_opes_f64_kernel (values + opes in one launch; 16 lanes per frame) grid=2432 block=256 lds=6144"
    assert fr.geometry(info, fi.GEOMETRY) == (2432, 256, 16)
    found, chunk, unread = fi._geometry(info, 10 ** 6, None)
    assert found == [("frames_value_opes_f64_kernel", 2432, 16, 1, 10 ** 6 // (2432 * 16))] and chunk is None and not unread
    with pytest.raises(AssertionError):
        fr.geometry("frames_lane_kernel grid=8 block=256", fi.GEOMETRY)


@pytest.mark.parametrize("cus", [256, 304])
@pytest.mark.parametrize("lanes,block", GEOMETRIES)
def test_the_size_rule_on_a_model_of_the_loop(lanes, block, cus):
    grid = 8 * cus
    r = fr.batch_size(grid, block, lanes)
    per_block, per_wave, waves = block // lanes, 64 // lanes, block // 64
    assert r.per_block == per_block and r.n == 3 * grid * per_block + r.tail and math.gcd(fr.BASE, grid * per_block) == 1
    frames = fr.loop_model(r.n, grid, per_block)
    assert sorted(f for v in frames.values() for f in v) == list(range(r.n))              # every frame once
    step = grid * per_block
    assert all(v == list(range(v[0], r.n, step)) for v in frames.values() if v)
    # every block: at least three rounds in every slot; fr.rounds_run says the same
    assert min(len(v) for v in frames.values()) >= 3 and fr.rounds_run(r.n, grid, per_block) == 3
    last = max(len(v) for v in frames.values())
    assert last == 4
    live = sorted((b, s // per_wave, s % per_wave) for (b, s), v in frames.items() if len(v) == last)
    assert live == sorted(r.live) and len(live) == r.tail
    assert all(fr.frame_of(r, slot, 3) == frames[(slot[0], slot[1] * per_wave + slot[2])][3] for slot in r.live)
    blocks = {b for b, _, _ in live}
    assert blocks == {0}, "a block other than the first is still in the loop"
    per = dict(((b, w), sum(1 for bb, ww, _ in live if (bb, ww) == (b, w))) for b in blocks for w in range(waves))
    if lanes < 64:                                    # a wave in which some but not all lane groups still have a frame
        assert any(0 < c < per_wave for c in per.values()), per
        assert "partial" in r.classes and 0 < per[r.classes["partial"][:2]] < per_wave
    if waves > 1:                                     # an idle wave next to a busy one
        assert any(per[(b, w)] > 0 and per[(b, w + 1)] == 0 for b in blocks for w in range(waves - 1)), per
    if "full" in r.classes:
        assert per[r.classes["full"][:2]] == per_wave
    assert set(r.classes.values()) <= set(r.live) and r.classes


# ---- the comparer on stand-ins -------------------------------------------------------------------------------------------------------
GRID, BLOCK, LANES = 5, 256, 8
PB = BLOCK // LANES
W = torch.randn((6, 3), generator=torch.Generator().manual_seed(5), dtype=torch.float64)


def _g(rows):
    return torch.tanh(rows @ W) + 2.0                 # never zero: adding 0.0 to it changes no bit


def correct(x, grid=GRID, per_block=PB):
    return {"out": _g(x), "e": _g(x).sum(1)}


def _by_slot(x, grid, per_block, rule):
    """The loop's model with a per-slot rule(out, frames of the slot, rows of x)"""
    out = _g(x).clone()
    for (b, s), frames in fr.loop_model(x.shape[0], grid, per_block).items():
        rule(out, b, s, frames)
    return {"out": out, "e": out.sum(1)}


def keeps_its_accumulator(x, grid=GRID, per_block=PB):
    """acc is cleared once, above the loop: a slot's frame gets its own value on top of the slot's earlier ones"""
    def rule(out, b, s, frames):
        acc = torch.zeros(3, dtype=x.dtype)
        for f in frames:
            own = out[f].clone()
            out[f] = acc + own
            acc = acc + own
    return _by_slot(x, grid, per_block, rule)


def reads_its_row_an_iteration_late(x, grid=GRID, per_block=PB):
    """the row pointer is advanced after the frame's rows are read: from the second iteration on a slot reads its previous frame's"""
    def rule(out, b, s, frames):
        for prev, f in zip(frames, frames[1:]):
            out[f] = _g(x[prev:prev + 1])[0]
    return _by_slot(x, grid, per_block, rule)


def idle_slots_leave_early(x, grid=GRID, per_block=PB):
    """a slot without a frame in the launch's last round leaves the loop before its last frame's final store is complete"""
    frames_of = fr.loop_model(x.shape[0], grid, per_block)
    last = max(len(v) for v in frames_of.values())

    def rule(out, b, s, frames):
        if len(frames) < last and len(frames) > 1:
            out[frames[-1], 2] = 0.0
    return _by_slot(x, grid, per_block, rule)


FAULTS = [keeps_its_accumulator, reads_its_row_an_iteration_late, idle_slots_leave_early]


def _batches():
    r = fr.batch_size(GRID, BLOCK, LANES)
    base = torch.randn((fr.BASE, 6), generator=torch.Generator().manual_seed(9), dtype=torch.float64)
    return r, base, fr.repeated(base, r.n)


def test_a_correct_function_passes():
    r, base, x = _batches()
    assert x.shape[0] == r.n == 3 * GRID * PB + 9 and torch.equal(x[fr.BASE:], base[:r.n - fr.BASE])
    assert fr.wrong_frames(correct(x), correct(base)) == []
    for slices in (1, 3, 1000):
        assert fr.wrong_frames(correct(x), correct(base), slices=slices) == []
    nan = correct(x)
    nan["out"][7, 1] = float("nan")                   # NaN in both is equal; NaN in one is not
    want = correct(base)
    assert fr.wrong_frames(nan, want) == [7]
    want["out"][7, 1] = float("nan")
    assert fr.wrong_frames(nan, want, names=["out"]) == sorted(set(range(7 + fr.BASE, r.n, fr.BASE)))


@pytest.mark.parametrize("fault", FAULTS, ids=[f.__name__ for f in FAULTS])
def test_a_planted_fault_is_named(fault):
    r, base, x = _batches()
    one_round = x[:GRID * PB - 3]                     # a ragged single round: what every shorter test runs
    got, want = fault(one_round), correct(one_round)
    assert all(torch.equal(got[k].view(torch.int64), want[k].view(torch.int64)) for k in want), "visible in one round"
    got, want = fault(base, grid=-(-fr.BASE // PB)), correct(base)
    assert all(torch.equal(got[k].view(torch.int64), want[k].view(torch.int64)) for k in want), "visible in the base launch"
    wrong = fr.wrong_frames(fault(x), correct(base))
    assert wrong and wrong[0] >= GRID * PB, wrong[:5]
    if fault is idle_slots_leave_early:               # exactly the third round's frames of the slots idle in the fourth
        assert wrong == list(range(2 * GRID * PB + r.tail, 3 * GRID * PB))
    else:                                             # every frame past the first round
        assert wrong == list(range(GRID * PB, r.n))
    for name in ("out", "e"):
        assert fr.wrong_frames(fault(x), correct(base), names=[name]) == wrong
