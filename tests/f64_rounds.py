"""The grid-stride loop of the float64 one-launch kernels, past one round per block: the batch size that gets every block through three
full rounds and a ragged fourth, and the comparison of such a launch with one launch of the frames it repeats.

The ten kernels run a frame in a group of G lanes, block / G frames per block and round (slot = thread / G, wave = thread / 64), and
step `for (f = block * per_block + slot; f < n; f += grid * per_block)`.  A frame's LDS rows and its slot's registers pass from one
iteration to the next; a batch of one round per block - every batch of the entries' own tests - never iterates.

  geometry(info)            (grid, block, G) of a launch info, read by test_gpu_frame_isolation's GEOMETRY pattern
  tail_of(block, G)         frames of the ragged last round
  batch_size(grid, ...)     N = 3 grid per_block + tail, and what the last round looks like (Rounds)
  loop_model(n, grid, pb)   {(block, slot): its frames in order} - the loop above, literally
  wrong_frames(long, base)  the frames of a long launch on a repeated base batch whose rows are not the base launch's, bit for bit

No GPU is needed to import or use this module."""

import collections
import math
import re

import torch

import isolation as iso

BASE = 251                  # test_gpu_frame_isolation's prime; asserted equal where both are imported
ROUNDS = 3                  # full rounds of every block before the ragged one

Rounds = collections.namedtuple("Rounds", "n grid block lanes per_block tail live classes")


def geometry_pattern(table):
    """The (pattern, reader) of test_gpu_frame_isolation.GEOMETRY that reads "(values + ...; G lanes per frame) grid= block="."""
    rows = [(p, r) for p, r in table if "lanes per frame" in p]
    assert len(rows) == 1, rows
    return rows[0]


def geometry(info, table):
    """(grid, block, lanes per frame) of a one-kernel launch info, by the isolation file's own pattern"""
    pattern, read = geometry_pattern(table)
    m = re.search(pattern, info)
    assert m and info.count("_kernel") == 1, info
    grid, per_block, ring = read(m)
    lanes, block = int(m.group(2)), int(m.group(4))
    assert ring == 1 and per_block * lanes == block and block % 64 == 0 and 64 % lanes == 0, info
    return grid, block, lanes


def tail_of(block, lanes):
    """Frames of the fourth round, all in block 0 (tail < per_block wherever per_block > 1): with several frames per wave and several
    waves per block, wave 0 full, one group of wave 1 live and the other waves idle; otherwise one frame - a wave with one live group
    of several, or a busy wave next to an idle one, or (one frame per block) one block a round ahead of the others."""
    per_wave, waves = 64 // lanes, block // 64
    return per_wave + 1 if per_wave > 1 and waves > 1 else 1


def batch_size(grid, block, lanes, base=BASE):
    """Rounds for a saturated grid: n, the live (block, wave, group) slots of the last round and one slot of each live class -
    "full" (every group of its wave live) and "partial" (some groups of its wave idle)."""
    per_block, per_wave = block // lanes, 64 // lanes
    tail = tail_of(block, lanes)
    n = ROUNDS * grid * per_block + tail
    assert math.gcd(base, grid * per_block) == 1, ("copies of the base line up with the blocks", base, grid, per_block)
    live = [(s // per_block, (s % per_block) // per_wave, s % per_wave) for s in range(tail)]
    by_wave = collections.Counter((b, w) for b, w, _ in live)
    classes = {}
    for b, w, g in live:
        classes.setdefault("full" if by_wave[(b, w)] == per_wave else "partial", (b, w, g))
    return Rounds(n, grid, block, lanes, per_block, tail, live, classes)


def frame_of(r, slot, rnd):
    """The frame that (block, wave, group) `slot` of Rounds r runs in round `rnd`"""
    b, w, g = slot
    return rnd * r.grid * r.per_block + b * r.per_block + w * (64 // r.lanes) + g


def rounds_run(n, grid, per_block):
    """Full rounds that every block of a launch of n frames runs"""
    return n // (grid * per_block)


def loop_model(n, grid, per_block):
    """{(block, slot): [frames in the order the slot runs them]}: the kernels' loop, literally"""
    frames = {}
    for b in range(grid):
        for s in range(per_block):
            mine, f = [], b * per_block + s
            while f < n:
                mine.append(f)
                f += grid * per_block
            frames[(b, s)] = mine
    return frames


def repeated(base, n):
    """n frames: the base batch repeated along its first dimension (on its device)"""
    reps = [1] * base.dim()
    reps[0] = -(-n // base.shape[0])
    return base.repeat(reps)[:n].contiguous()


def wrong_frames(long, base, names=None, slices=16):
    """Sorted frames f of the long launch with a row, in any output of `names`, that is not row f mod BASE of the base launch bit for
    bit.  Rows are compared as integers (NaN != NaN must hide nothing), `slices` frames' ranges at a time: the largest temporary is a
    slice of the output, never the output."""
    bad = set()
    for name in (names if names is not None else sorted(base)):
        a, b = long[name], base[name]
        assert a.dtype == b.dtype and a.shape[1:] == b.shape[1:] and a.device == b.device, (name, a.shape, b.shape)
        n, nb = a.shape[0], b.shape[0]
        ia, ib = iso._bits(a.contiguous()).reshape(n, -1), iso._bits(b.contiguous()).reshape(nb, -1)
        step = max(nb, -(-n // slices))
        for s in range(0, n, step):
            e = min(n, s + step)
            want = ib[torch.arange(s, e, device=a.device) % nb]
            bad |= set(((ia[s:e] != want).any(1).nonzero().flatten() + s).tolist())
    return sorted(bad)
