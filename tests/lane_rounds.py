"""The float32 lane-per-frame kernels past one ring generation (or one grid-stride iteration) per block: the batch size that takes every
block through two full generations and a ragged, uneven third, a literal model of how the tiles are dealt, and the words that say where
in the ring a wrong frame lies.  The comparison itself is tests/f64_rounds.py's (`repeated`, `wrong_frames`, BASE = 251).

The ring kernels (molann_lane_jit in all its builds, molann_bwd_ring; molann_ring.inc): a tile is 64 frames, one per lane.  Block b of
`grid` takes the tiles ring_tile(block_tiles(n_tiles, b, grid), n) = b + n grid, n = 0 .. n_b - 1 (TILE_GROUP = 1).  Its n-th tile lives
in slot n % NSLOT at generation n / NSLOT: loader n % NLOAD refills the slot only after done[slot] >= generation, a consumer reads it only
after ready[slot] >= generation + 1, and the consumers take n from an LDS counter.  grid = min(n_tiles, CUs x blocks per CU), so a block
reaches generation 1 only beyond 64 x grid x NSLOT frames.

The ahead-of-time kernels (frames_lane_kernel, mlp_lane_kernel, mlp_mfma_kernel, molann_lane_bwd) stride
`for (t = block * wpb + wave; t < n_tiles; t += grid * wpb)`: the same dealing with a wave in a block's place, one slot, and "iteration"
for "generation".  molann_mlp_bwd deals the tiles b + k grid to block b and hands them to its waves through an atomic counter.

  geometry(info) / geometries(info)   Ring(kind, ncons, nload, nslot, grid, block) / Stride(kind, grid, block, waves, tile) of a launch info
  tile_model(n_frames, grid, nslot)   {block: [tiles in order]} with .where(frame) -> (block, n, slot, generation, lane)
  batch_size(grid, nslot, gens=2)     n_tiles = grid (gens nslot + 1) + extra, n = 64 (n_tiles - 1) + 37            (a ring)
  stride_size(units, tiles, its=2)    the same shape for grid-stride kernels: `its` full iterations of every wave, a ragged uneven one more
  explain(frames, grid, nslot)        wrong frame numbers -> "(block, n-th tile, slot, generation, lane)"

No GPU is needed to import or use this module."""

import collections
import math
import re

from f64_rounds import BASE, repeated, wrong_frames     # noqa: F401  (re-exported: the tests take them from here)

TILE = 64
RAGGED = 37                                  # live lanes of the last tile
MAX_FRAMES = 1 << 21
GENERATIONS = 2

Ring = collections.namedtuple("Ring", "kind ncons nload nslot grid block")
Stride = collections.namedtuple("Stride", "kind grid block waves tile by_block")
Size = collections.namedtuple("Size", "n n_tiles extra grid nslot generations")

_RING = re.compile(r"(molann_lane_jit<[^>]*>|molann_bwd_ring(?:<values>)?) \(plan-specialised; (\d+) consumer waves \+ (\d+) loader, "
                   r"ring of (\d+) tiles[^)]*\) grid=(\d+) block=(\d+)")
_STRIDE = re.compile(r"(frames_lane_kernel<[^>]*>|mlp_lane_kernel<[^>]*>|mlp_mfma_kernel<[^>]*>|molann_mlp_bwd|molann_lane_bwd)"
                     r"(?: \(plan-specialised\))? grid=(\d+) block=(\d+)")
# frames per wave and iteration: mlp_mfma_kernel steps over blocks of 16 rows (molann_dev_mlp.inc: `rb < n_blocks`, n_blocks = ceil(n / 16)),
# every other kernel of the family over 64-frame tiles
_TILE_OF = {"mlp_mfma_kernel": 16}


def geometries(info):
    """Every lane-family launch an info names, in the order it names them.  Waves per block: block / 64 for frames_lane_kernel
    (molann_host_launch.inc: `dim3 block(64 * wpb)`), mlp_lane_kernel and mlp_mfma_kernel (`dim3(64 * wpb)`), molann_lane_bwd
    (`64 * g.wpb`) and molann_mlp_bwd (`64 * p->mbwd_wpb`), whose waves take their block's tiles from a counter (by_block)."""
    found = []
    for m in _RING.finditer(info):
        r = Ring(m.group(1), *[int(m.group(i)) for i in range(2, 7)])
        assert r.block == 64 * (r.ncons + r.nload) and r.nslot >= 1 and r.grid >= 1, info
        found.append((m.start(), r))
    for m in _STRIDE.finditer(info):
        kind, grid, block = m.group(1), int(m.group(2)), int(m.group(3))
        assert block % 64 == 0 and grid >= 1, info
        found.append((m.start(), Stride(kind, grid, block, block // 64, _TILE_OF.get(kind.split("<")[0], TILE), kind == "molann_mlp_bwd")))
    return [g for _, g in sorted(found, key=lambda p: p[0])]


def geometry(info):
    """The one lane-family launch of an info: Ring(kind, ncons, nload, nslot, grid, block) or Stride(kind, grid, block, ...)"""
    found = geometries(info)
    assert len(found) == 1, (info, found)
    return found[0]


def units_of(g):
    """What deals the tiles: the blocks of a ring kernel, the waves of a grid-stride kernel"""
    return g.grid if isinstance(g, Ring) else g.grid * g.waves


class TileModel(dict):
    """{block: [tiles in order]}; `where(frame)` names the frame's place in the ring"""

    def __init__(self, n_frames, grid, nslot):
        dict.__init__(self)
        self.n_frames, self.grid, self.nslot = int(n_frames), int(grid), int(nslot)
        self.n_tiles = (self.n_frames + TILE - 1) // TILE
        for b in range(self.grid):
            t_base, t_step, n_b = block_tiles(self.n_tiles, b, self.grid)
            self[b] = [ring_tile(t_base, t_step, n) for n in range(n_b)]

    def where(self, frame):
        """(block, n, slot, generation, lane) of a frame: the block's n-th tile, in slot n % nslot at generation n / nslot"""
        assert 0 <= frame < self.n_frames, (frame, self.n_frames)
        t, lane = divmod(int(frame), TILE)
        b = t % self.grid
        n = (t - b) // self.grid
        assert self[b][n] == t, (frame, b, n)
        return b, n, n % self.nslot, n // self.nslot, lane


def block_tiles(n_tiles, block, grid, tile_group=1):
    """molann_ring.inc's block_tiles, line by line: (t_base, t_step, n_b)"""
    t_base = block * tile_group
    t_step = grid * tile_group
    full = (n_tiles - tile_group - t_base) // t_step + 1 if n_tiles - tile_group - t_base >= 0 else 0
    first = t_base + full * t_step
    partial = n_tiles - first if first < n_tiles else 0
    return t_base, t_step, full * tile_group + partial


def ring_tile(t_base, t_step, n):
    """molann_ring.inc's ring_tile for TILE_GROUP = 1"""
    return t_base + n * t_step


def tile_model(n_frames, grid, nslot):
    return TileModel(n_frames, grid, nslot)


def loader_tiles(n_b, nload):
    """[n of loader 0, n of loader 1, ...]: loader j takes the block's tiles n = j, j + NLOAD, ... (ring_loader)"""
    return [list(range(j, n_b, nload)) for j in range(nload)]


def _extra(grid):
    """Blocks that own one tile more: about a third of them, at least three where there are four blocks (so that every lane of the extra
    tile, those past the ragged tile's 37 too, runs in two blocks or more and sees more than one base frame), never all"""
    assert grid >= 2, ("one block cannot own more tiles than its neighbours", grid)
    return max(min(3, grid - 1), grid // 3)


def _sized(n_tiles, extra, grid, nslot, generations, base):
    n = TILE * (n_tiles - 1) + RAGGED
    assert math.gcd(base, TILE * grid * nslot) == 1, ("copies of the base line up with the ring", base, grid, nslot)
    assert n <= MAX_FRAMES, ("this geometry needs more than 2^21 frames", n, grid, nslot, generations)
    return Size(n, n_tiles, extra, grid, nslot, generations)


def batch_size(grid, nslot, generations=GENERATIONS, base=BASE):
    """A ring of nslot >= 2 tiles: every block owns generations x nslot + 1 tiles, the first `extra` blocks one more, so every block
    fills its ring `generations` times and goes on into generation `generations`; the ragged last tile (37 frames) is the last tile of
    block extra - 1, the second of that generation there."""
    assert nslot >= 2, ("a ring of one slot: use stride_size", nslot)
    extra = _extra(grid)
    return _sized(grid * (generations * nslot + 1) + extra, extra, grid, nslot, generations, base)


def stride_size(units, tiles=(TILE,), iterations=GENERATIONS, base=BASE):
    """Grid-stride kernels launched on the same batch, `units[k]` waves (or blocks) dealing tiles of `tiles[k]` frames: the kernel with
    the most frames per iteration runs `iterations` full iterations in every wave and an uneven ragged one more; the others run at least
    as many, and `extra` is the first choice that leaves every one of them uneven (its tile count no multiple of its units)."""
    units, tiles = list(units), list(tiles)
    assert len(units) == len(tiles) and all(TILE % t == 0 for t in tiles), (units, tiles)
    per = [-(-u * t // TILE) for u, t in zip(units, tiles)]       # 64-frame tiles per full iteration
    lead = max(per)
    for extra in range(_extra(lead), lead):
        n_tiles = lead * iterations + extra
        n = TILE * (n_tiles - 1) + RAGGED
        counts = [-(-n // t) for t in tiles]
        if all(c % u != 0 and c // u >= iterations for c, u in zip(counts, units)):
            for u, t in zip(units, tiles):
                assert math.gcd(base, t * u) == 1, ("copies of the base line up with the grid", base, u, t)
            return _sized(n_tiles, extra, lead, 1, iterations, base)
    raise AssertionError(("no uneven size for these kernels", units, tiles))


def full_generations(n_frames, grid, nslot, tile=TILE):
    """Generations (iterations: nslot = 1) that EVERY block of the launch fills completely"""
    n_tiles = -(-n_frames // tile)
    return (n_tiles // grid) // nslot


def explain(frames, grid, nslot, n_frames, limit=8):
    """"N frames wrong; frame f: block b, its n-th tile, slot s, generation g, lane l; ..." for an assertion message"""
    frames = list(frames)
    if not frames:
        return "no frame wrong"
    model = tile_model(n_frames, grid, nslot)
    where = [(f,) + model.where(f) for f in frames[:limit]]
    gens = collections.Counter(model.where(f)[3] for f in frames[:4096])
    text = "; ".join("frame %d: block %d, tile %d of the block, slot %d, generation %d, lane %d" % w for w in where)
    return "%d frames wrong (grid %d, ring of %d; by generation, first 4096: %s); %s%s" % (
        len(frames), grid, nslot, dict(sorted(gens.items())), text, "; ..." if len(frames) > limit else "")
