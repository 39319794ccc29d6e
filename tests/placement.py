"""An arena of guarded buffers: what a caller's own arrays look like to a kernel.

An MD engine hands the C ABI pointers into the middle of its position and force arrays: 4-byte aligned (8 for float64), rarely 16,
with somebody else's data on both sides.  A fresh torch allocation is 256-byte aligned and has nothing next to it that a test
looks at, so neither the narrow-load / narrow-store paths nor a store one element past an output are seen by tests that use one.

`Arena(device)` owns one large tensor per dtype, viewed as int32 and filled with SENTINEL - a bit pattern that reads as NaN in
float32 and, paired, as NaN in float64.  `carve(name, shape, dtype, offset_elems)` returns a contiguous view whose address is
`offset_elems * itemsize` past a 256-byte boundary, between two guard bands of the sentinel; a band is at least 64 rows of the
buffer and never less than 4 KiB, so a kernel that overruns by a whole tile still lands inside the arena: the failure is an
assertion, never a fault.  `check()` names every buffer whose leading or trailing band no longer holds the sentinel (compared as
integers: NaN != NaN would hide nothing here, but a float comparison would).  Inputs are carved the same way (`data=`): a kernel
that reads past an input and uses what it read poisons its own outputs with NaN, and `inputs_changed()` names every input that was
written.  `refill(name)` puts the sentinel back into an output, `put(name, values)` known values into a buffer that is accumulated
into.  No GPU is needed to import or use this module."""

import torch

SENTINEL = 0x7FF8DEAD                                      # float32: NaN; two of them as a float64: NaN
BOUNDARY = 256                                             # bytes: what torch's allocator gives, and more than any kernel's widest access
MIN_BAND = 4096                                            # bytes
BAND_ROWS = 64
RESET_MARGIN = 8 << 20                                     # bytes past the last band that `reset` refills as well


def bits(t):
    """The integer view of a float tensor (float32 -> int32, float64 -> int64), for comparisons bit for bit."""
    return t.view({4: torch.int32, 8: torch.int64}[t.element_size()]) if t.is_floating_point() else t


def same_bits(a, b):
    return a.shape == b.shape and a.dtype == b.dtype and bool(torch.equal(bits(a), bits(b)))


def _round_up(v, m):
    return -(-v // m) * m


class _Buffer(object):
    __slots__ = ("name", "view", "words", "lead", "trail", "kept")

    def __init__(self, name, view, words, lead, trail):
        self.name, self.view, self.words, self.lead, self.trail, self.kept = name, view, words, lead, trail, None


class Arena(object):
    def __init__(self, device, capacity=64 << 20):
        """`capacity`: bytes per dtype, allocated when the dtype is first carved."""
        self.device, self.capacity = torch.device(device), _round_up(int(capacity), BOUNDARY)
        self._store = {}                                   # dtype -> [int32 tensor whose element 0 sits on a boundary, cursor in bytes]
        self.buffers = {}

    def _words(self, dtype, need):
        if dtype not in self._store:
            raw = torch.empty(self.capacity // 4 + BOUNDARY // 4, dtype=torch.int32, device=self.device)
            skip = (-raw.data_ptr() % BOUNDARY) // 4
            words = raw[skip:skip + self.capacity // 4]
            words.fill_(SENTINEL)
            self._store[dtype] = [words, 0]
        words, cursor = self._store[dtype]
        if cursor + need > self.capacity:
            raise MemoryError("arena of %d bytes per dtype is full: %d more wanted at %d" % (self.capacity, need, cursor))
        return words, cursor

    def reset(self):
        """Forget every buffer and put the sentinel back wherever a buffer or a band was."""
        for entry in self._store.values():
            entry[0][:(entry[1] + RESET_MARGIN) // 4].fill_(SENTINEL)     # nothing past the last trailing band was handed out
            entry[1] = 0
        self.buffers = {}

    def carve(self, name, shape, dtype, offset_elems=0, data=None, row_dims=None):
        """A contiguous view of `shape` at `offset_elems` elements past a boundary, between two guard bands.  With `data` the view is
        an input: it holds a copy of data, and `inputs_changed()` compares it with that copy.  Without, it holds the sentinel.  A row -
        the bands are 64 of them - is the last `row_dims` dimensions (by default all but the first: a frame's worth)."""
        if name in self.buffers:
            raise KeyError("buffer %r carved twice" % name)
        shape = tuple(int(s) for s in shape)
        item = torch.empty(0, dtype=dtype).element_size()
        if item % 4:
            raise TypeError("the arena holds 4- and 8-byte types, not %s" % dtype)
        numel = 1
        for s in shape:
            numel *= s
        row = item
        for d in shape[1:] if row_dims is None else shape[len(shape) - row_dims:]:
            row *= d
        band = _round_up(max(MIN_BAND, BAND_ROWS * row), BOUNDARY)
        start = band + int(offset_elems) * item            # the leading band holds the offset as well
        end = start + numel * item
        total = _round_up(end + band, BOUNDARY)
        words, cursor = self._words(dtype, total)
        w = lambda lo, hi: words[(cursor + lo) // 4:(cursor + hi) // 4]     # noqa: E731
        body = w(start, end)
        view = body.view(dtype).view(shape) if numel else torch.empty(shape, dtype=dtype, device=self.device)
        buf = _Buffer(name, view, body, w(0, start), w(end, total))
        if data is not None:
            view.copy_(data.to(self.device, dtype).reshape(shape))
            buf.kept = body.clone()
        self._store[dtype][1] = cursor + total
        self.buffers[name] = buf
        if numel:
            assert view.is_contiguous() and (view.data_ptr() - int(offset_elems) * item) % BOUNDARY == 0, (name, view.data_ptr())
        return view

    def refill(self, *names):
        """The sentinel back into these outputs (all buffers that are no inputs when none is named)."""
        for name in names or [n for n, b in self.buffers.items() if b.kept is None]:
            self.buffers[name].words.fill_(SENTINEL)

    def put(self, name, values):
        """Known values into a buffer that a kernel accumulates into."""
        b = self.buffers[name]
        b.view.copy_(values.to(self.device, b.view.dtype).reshape(b.view.shape))

    def holds_sentinel(self, name):
        """True when every word of the buffer is still the sentinel: nothing was stored into it."""
        return bool((self.buffers[name].words == SENTINEL).all())

    def check(self):
        """["name (leading band)", "name (trailing band)", ...] of every guard band that differs from the sentinel."""
        bad = []
        for name, b in self.buffers.items():
            for side, band in (("leading", b.lead), ("trailing", b.trail)):
                if not bool((band == SENTINEL).all()):
                    at = int((band != SENTINEL).nonzero()[0 if side == "trailing" else -1])
                    gap = at if side == "trailing" else band.numel() - 1 - at
                    bad.append("%s (%s band, nearest damaged word %d words from the buffer)" % (name, side, gap))
        return bad

    def inputs_changed(self):
        """Names of the inputs that no longer hold, bit for bit, what was put in."""
        return [name for name, b in self.buffers.items() if b.kept is not None and not bool(torch.equal(b.words, b.kept))]


def offsets(placement, names, wide=4):
    """{name: offset in elements} of a call's buffers.  `placement`: an int k (every buffer at k), "mixedA" or "mixedB" (every buffer
    of the call at another residue, the second the first rotated).  `wide` is 16 bytes in elements: 4 for float32, 2 for float64."""
    if isinstance(placement, int):
        return dict((n, placement) for n in names)
    shift = {"mixedA": 1, "mixedB": 3}[placement]          # float32: x 1, next 2, 3, 0, ... / x 3, 0, 1, 2, ...; float64: 1, 0, ... / 0, 1, ...
    if wide == 2:
        shift = {"mixedA": 1, "mixedB": 0}[placement]
    return dict((n, (i + shift) % wide) for i, n in enumerate(names))
