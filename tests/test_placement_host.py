"""The check checks: tests/placement.py on CPU tensors.  The guard bands must report a one-element write on either side of a
buffer by name, pass when nothing was touched, and an input band that is read must poison what consumes it."""

import pytest
import torch

import placement as pl


@pytest.mark.parametrize("dtype", [torch.float32, torch.float64])
def test_carve_gives_the_requested_residues(dtype):
    arena = pl.Arena("cpu", capacity=1 << 20)
    item = 4 if dtype == torch.float32 else 8
    for k in range(16 // item + 2):
        v = arena.carve("b%d" % k, (5, 7), dtype, k)
        assert v.is_contiguous() and v.shape == (5, 7) and v.dtype == dtype
        assert v.data_ptr() % 256 == (k * item) % 256 and v.data_ptr() % 16 == (k * item) % 16
        assert bool(torch.isnan(v).all())                  # the sentinel reads as NaN in both types
    assert arena.check() == [] and arena.inputs_changed() == []


def test_bands_are_64_rows_and_at_least_4_kib():
    arena = pl.Arena("cpu", capacity=8 << 20)
    arena.carve("small", (3, 2), torch.float32, 1)
    arena.carve("rows", (4, 500, 3), torch.float64, 1)
    arena.carve("flat", (9,), torch.float32, 3)
    for name, least in (("small", 4096), ("rows", 64 * 500 * 3 * 8), ("flat", 4096)):
        b = arena.buffers[name]
        assert b.lead.numel() * 4 >= least and b.trail.numel() * 4 >= least, name


@pytest.mark.parametrize("dtype", [torch.float32, torch.float64])
@pytest.mark.parametrize("side", ["after", "before"])
def test_a_one_element_overrun_is_reported_by_name(dtype, side):
    arena = pl.Arena("cpu", capacity=1 << 20)
    arena.carve("x", (6, 5, 3), dtype, 1, data=torch.arange(90.0).view(6, 5, 3))
    out = arena.carve("out", (6, 7), dtype, 3 if dtype == torch.float32 else 1)
    arena.carve("other", (6, 7), dtype, 2 if dtype == torch.float32 else 0)
    assert arena.check() == []
    # one element past the end / before the start, written the way a kernel's tail store would: through the same storage
    flat = torch.empty(0, dtype=dtype).set_(out.untyped_storage(), out.storage_offset() - 1, (out.numel() + 2,), (1,))
    flat[-1 if side == "after" else 0] = 1.0
    bad = arena.check()
    assert len(bad) == 1 and bad[0].startswith("out (%s band" % ("trailing" if side == "after" else "leading")), bad
    assert "0 words from the buffer" in bad[0]
    assert arena.inputs_changed() == []
    assert arena.holds_sentinel("out")                     # the buffer itself was not touched


def test_a_sentinel_shaped_write_cannot_hide_and_a_float_compare_is_not_used():
    """The bands are compared as integers: another NaN than the sentinel's is damage."""
    arena = pl.Arena("cpu", capacity=1 << 20)
    out = arena.carve("out", (4, 3), torch.float32, 2)
    torch.empty(0, dtype=torch.float32).set_(out.untyped_storage(), out.storage_offset() + out.numel(), (1,), (1,))[0] = float("nan")
    assert [b.split(" ")[0] for b in arena.check()] == ["out"]


def test_an_untouched_arena_passes_and_outputs_can_be_refilled():
    arena = pl.Arena("cpu", capacity=1 << 20)
    x = arena.carve("x", (4, 3), torch.float32, 1, data=torch.ones(4, 3))
    out = arena.carve("out", (4, 3), torch.float32, 2)
    acc = arena.carve("acc", (10,), torch.float32, 3)
    out.copy_(x * 2.0)
    arena.put("acc", torch.arange(10.0))
    assert arena.check() == [] and arena.inputs_changed() == []
    assert not arena.holds_sentinel("out") and bool((acc == torch.arange(10.0)).all())
    arena.refill("out")
    assert arena.holds_sentinel("out") and bool(torch.isnan(out).all())
    x[1, 1] = 5.0
    assert arena.inputs_changed() == ["x"]
    arena.reset()
    assert arena.buffers == {} and arena.check() == []


@pytest.mark.parametrize("dtype", [torch.float32, torch.float64])
def test_reading_an_input_band_poisons_what_consumes_it(dtype):
    arena = pl.Arena("cpu", capacity=1 << 20)
    x = arena.carve("x", (8, 3), dtype, 1, data=torch.ones(8, 3))
    assert bool(torch.isfinite(x.sum()))
    for first in (-1, 1):                                  # one element before, one past the end
        wide = torch.empty(0, dtype=dtype).set_(x.untyped_storage(), x.storage_offset() + min(first, 0), (x.numel() + 1,), (1,))
        assert bool(torch.isnan(wide.sum())) and bool(torch.isnan((wide * 0.0).max()))


def test_offsets_cover_every_residue():
    names = ["x", "g", "out", "gx", "gp"]
    assert pl.offsets(2, names) == dict((n, 2) for n in names)
    a, b = pl.offsets("mixedA", names), pl.offsets("mixedB", names)
    assert [a[n] for n in names] == [1, 2, 3, 0, 1] and [b[n] for n in names] == [3, 0, 1, 2, 3]
    a, b = pl.offsets("mixedA", names, wide=2), pl.offsets("mixedB", names, wide=2)
    assert [a[n] for n in names] == [1, 0, 1, 0, 1] and [b[n] for n in names] == [0, 1, 0, 1, 0]


def test_same_bits_tells_nan_payloads_and_signed_zeros_apart():
    a = torch.tensor([0.0, float("nan")])
    assert pl.same_bits(a, a.clone())
    assert not pl.same_bits(a, torch.tensor([-0.0, float("nan")]))
    assert not pl.same_bits(torch.zeros(2), torch.zeros(2, dtype=torch.float64))
