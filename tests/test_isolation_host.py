"""tests/isolation.py on torch stand-ins for a kernel: a correct one passes the checker, three planted leaks - each invisible on
finite data - are caught with the leaking frames named.  This is what shows that tests/test_gpu_frame_isolation.py can fail."""

import types

import pytest
import torch

import isolation as iso
from molann_amd import workloads as wl

N, TILE, D, K = 200, 64, 6, 8
BAD_A, BAD_B = (0, 63, N - 1), (1, 64, 100, N - 2)


def _weights():
    g = torch.Generator().manual_seed(3)
    w1 = torch.zeros(K, K, dtype=torch.float64)
    w1[:D] = torch.randn((D, K), generator=g, dtype=torch.float64)        # K-padding: the rows of the padded k's are zeros
    return w1, torch.randn((K, 3), generator=g, dtype=torch.float64)


W1, W2 = _weights()


def correct(f):
    pad = torch.zeros((f.shape[0], K), dtype=f.dtype)
    pad[:, :D] = f
    return {"out": torch.tanh(pad @ W1) @ W2}


def leaks_the_next_row(f):
    out = correct(f)["out"]
    out[:-1] += 0.0 * f[1:].sum(1, keepdim=True)
    return {"out": out}


def leaks_the_last_row_into_the_last_tile(f):
    out = correct(f)["out"]
    first = (f.shape[0] - 1) // TILE * TILE
    out[first:] += 0.0 * f[-1].sum()                          # "clamped rows" of a short tile multiplied away, not selected away
    return {"out": out}


def fills_the_staging_buffer_once(f, every_tile=False):
    """A head on tiles of 64 rows through one staging buffer [64, K]: a tile writes its D feature columns, the hidden layer goes back
    into the same rows (all K columns), the padded columns meet the zero rows of W1 in the next tile."""
    n = f.shape[0]
    out = torch.empty((n, 3), dtype=f.dtype)
    staging = torch.zeros((TILE, K), dtype=f.dtype)
    for t0 in range(0, n, TILE):
        m = min(TILE, n - t0)
        if every_tile:
            staging.zero_()
        staging[:m, :D] = f[t0:t0 + m]
        staging[:m] = torch.tanh(staging[:m] @ W1)
        out[t0:t0 + m] = staging[:m] @ W2
    return {"out": out}


def _f(seed=1):
    return {"f": torch.randn((N, D), generator=torch.Generator().manual_seed(seed), dtype=torch.float64)}


def _run(kernel, bad, kind="mixed"):
    clean, data = kernel(_f()["f"]), iso.poison(_f(), bad, kind)
    got = kernel(data["f"])
    return clean, got


def test_the_stand_ins_agree_on_finite_data():
    f = _f()["f"]
    want = correct(f)["out"]
    for kernel in (leaks_the_next_row, leaks_the_last_row_into_the_last_tile, fills_the_staging_buffer_once,
                   lambda a: fills_the_staging_buffer_once(a, every_tile=True)):
        assert torch.equal(kernel(f)["out"], want)           # the planted leaks are invisible to any test on finite data


@pytest.mark.parametrize("kind", iso.KINDS)
def test_a_correct_kernel_passes(kind):
    for kernel in (correct, lambda a: fills_the_staging_buffer_once(a, every_tile=True)):
        for bad in (BAD_A, BAD_B):
            clean, got = _run(kernel, bad, kind)
            assert iso.keep_rows_equal(clean, got, bad, ["out"]) == []
            assert iso.leaking_frames(clean, got, bad, ["out"]) == []
            if kind == "nan":
                assert not bool(torch.isfinite(got["out"][list(bad)]).any())


@pytest.mark.parametrize("kernel,leaks", [
    (leaks_the_next_row, {BAD_A: [62, N - 2], BAD_B: [0, 63, 99, N - 3]}),
    (leaks_the_last_row_into_the_last_tile, {BAD_A: list(range(192, N - 1)), BAD_B: []}),
    (fills_the_staging_buffer_once, {BAD_A: [64, 127, 128, 191, 192], BAD_B: [65, 128, 129, 164, 192, 193]}),
])
def test_planted_leaks_are_named(kernel, leaks):
    found = False
    for bad, frames in leaks.items():
        clean, got = _run(kernel, bad, "nan")
        assert iso.leaking_frames(clean, got, bad, ["out"]) == frames, (kernel.__name__, bad)
        complaints = iso.keep_rows_equal(clean, got, bad, ["out"])
        assert bool(complaints) == bool(frames)
        if frames:
            found = True
            assert complaints[0].startswith("out: frame %d element 0 changed from " % frames[0]), complaints[0]
            assert complaints[-1] == "out: %d elements in %d kept frames changed" % (3 * len(frames), len(frames)), complaints[-1]
    assert found


def test_the_comparison_is_on_bits():
    a = {"out": torch.tensor([[0.0, 1.0], [float("nan"), 2.0]])}
    b = {"out": torch.tensor([[-0.0, 1.0], [float("nan"), 2.0]])}
    assert iso.keep_rows_equal(a, a, [], ["out"]) == []                     # a kept NaN with the same bits is no change
    bad = iso.keep_rows_equal(a, b, [], ["out"])
    assert len(bad) == 2 and "frame 0 element 0" in bad[0]                  # -0.0 == 0.0 as floats
    assert iso.keep_rows_equal(a, b, [0], ["out"]) == []
    assert iso.keep_rows_equal(a, {"out": b["out"].double()}, [], ["out"])[0].startswith("out: shape or type changed")
    assert iso.keep_rows_equal({"grad_params": a["out"]}, {"grad_params": b["out"]}, [], ["grad_params"]) == []      # a sum over frames


def test_poison():
    g = torch.Generator().manual_seed(2)
    bufs = {"x": torch.randn((9, 5, 3), generator=g), "v": torch.randn((2, 9, 5, 3), generator=g), "grad_out": torch.randn((9, 4), generator=g),
            "W0": torch.randn((4, 4), generator=g), "centers": torch.randn((9, 4), generator=g), "kappa": torch.randn(4, generator=g)}
    where = {"x": 3 * 2 + iso.COORD, "v": 3 * 2 + iso.COORD, "grad_out": 3}
    out = iso.poison(bufs, [1, 4, 8], "mixed", where=where)
    for shared in ("W0", "centers", "kappa"):                               # [9, 4] as well, but no per-frame input
        assert out[shared] is bufs[shared]
    assert bool(torch.isfinite(bufs["x"]).all())                            # copies
    for name, t in (("x", out["x"]), ("v", out["v"].movedim(1, 0)), ("grad_out", out["grad_out"])):
        rows, ref = t.reshape(9, -1), bufs[name].movedim(iso.frame_dim(name), 0).reshape(9, -1)
        nonfinite = (~torch.isfinite(rows)).nonzero().tolist()
        assert nonfinite == [[1, where[name]], [4, where[name]], [8, where[name]]], (name, nonfinite)
        assert bool(torch.isinf(rows[1, where[name]])) and float(rows[1, where[name]]) > 0 and bool(torch.isnan(rows[4, where[name]]))
        keep = torch.isfinite(rows)
        assert torch.equal(rows[keep], ref[keep])
    assert bool(torch.isnan(out["v"][0, 4, 2, iso.COORD])) and bool(torch.isfinite(out["v"][1]).all())       # tangent 0 alone
    assert int(torch.isnan(iso.poison(bufs, [1, 4], "nan", only=("x",))["x"]).sum()) == 2
    assert bool(torch.isfinite(iso.poison(bufs, [1, 4], "nan", only=("x",))["grad_out"]).all())
    assert int(torch.isinf(iso.poison(bufs, torch.tensor([1, 4]), "inf")["x"]).sum()) == 2
    mask = torch.zeros(9, dtype=torch.bool)
    mask[[0, 2]] = True
    assert (~torch.isfinite(iso.poison(bufs, mask, "nan")["x"])).nonzero()[:, 0].tolist() == [0, 2]
    with pytest.raises(ValueError):
        iso.poison(bufs, [0], "zero")
    with pytest.raises(AssertionError):
        iso.poison(bufs, [9], "nan")


def test_chosen_atom():
    items = [(wl.BOND, [7, 2]), (wl.ANGLE, [5, 3, 2])]
    assert iso.chosen_atom([0, 1, 2, 3], items) == 2                        # the first item atom that is aligned on
    assert iso.chosen_atom([0, 1], items) == 7 and iso.chosen_atom(None, items) == 7
    assert iso.chosen_atom([4, 0, 1], []) == 4


def _cx(align=(0, 1, 2, 3), dims=None):
    items = [(wl.ANGLE, [1, 4, 5]), (wl.DIHEDRAL, [4, 6, 7, 8]), (wl.BOND, [1, 4]), (wl.BOND, [9, 6]), (wl.POSITION, [0, 2])]
    return types.SimpleNamespace(items=items, align=None if align is None else list(align), n_inp=10, dims=dims)


def test_dependent_elements():
    cx = _cx()                                               # columns: angle 0, dihedral 1-2, bonds 3 and 4, positions 5-10
    shapes = {"out": (7, 11), "grad_x": (7, 10, 3)}
    m = iso.dependent_elements(cx, "features", 1, shapes)
    assert m["out"].nonzero().flatten().tolist() == [0, 3, 5, 6, 7, 8, 9, 10]       # its items; the positions through the centroid
    m = iso.dependent_elements(cx, "features_backward", 1, shapes)
    assert m["grad_x"].any(1).nonzero().flatten().tolist() == [1, 4, 5] and bool(m["grad_x"][[1, 4, 5]].all())
    assert not bool(m["out"].any())
    cx_free = _cx(align=None)
    m = iso.dependent_elements(cx_free, "features", 9, shapes, value="inf")
    assert m["out"].nonzero().flatten().tolist() == [4]
    m = iso.dependent_elements(cx_free, "features_backward", 9, shapes, value="inf")                  # g r / |r| with |r| = inf
    assert m["grad_x"].nonzero().tolist() == [[6, iso.COORD], [9, iso.COORD]]
    m = iso.dependent_elements(cx_free, "features_backward", 9, shapes, value="nan")                  # |r| = NaN: the whole rows
    assert m["grad_x"].all(1).nonzero().flatten().tolist() == [6, 9] and int(m["grad_x"].sum()) == 6
    assert iso.dependent_elements(cx_free, "features", 0, shapes)["out"].nonzero().flatten().tolist() == [5, 6, 7]
    assert not bool(iso.dependent_elements(cx_free, "features_backward", 0, shapes)["grad_x"].any())  # dx of a raw position is g
    # behind a head: every output, every item atom's row
    cxh = _cx(dims=[11, 16, 4])
    hs = {"out": (7, 4), "grad_x": (7, 10, 3), "energy": (7,), "grad_params": (300,)}
    m = iso.dependent_elements(cxh, "value_and_restraint_f64", 1, hs)
    assert set(m) == {"out", "grad_x", "energy"} and bool(m["out"].all()) and bool(m["energy"].all())
    assert m["grad_x"].all(1).nonzero().flatten().tolist() == [0, 1, 2, 4, 5]
    m = iso.dependent_elements(cxh, "value_and_restraint_f64", 9, hs, value="inf")                    # tanh(inf) = 1: nothing is owed
    assert not any(bool(v.any()) for v in m.values())
    m = iso.dependent_elements(cxh, "value_and_restraint_f64", None, hs, buffer="center", element=2)
    assert bool(m["energy"].all()) and not bool(m["out"].any())
    assert m["grad_x"].all(1).nonzero().flatten().tolist() == [0, 1, 2, 4, 5, 6, 7, 8, 9]
    m = iso.dependent_elements(cx, "features_backward", None, shapes, buffer="grad_f", element=2, value="inf")
    assert m["grad_x"].all(1).nonzero().flatten().tolist() == [4, 6, 7, 8]
    m = iso.dependent_elements(cx, "features_backward", None, shapes, buffer="grad_f", element=9)
    assert m["grad_x"].all(1).nonzero().flatten().tolist() == [2]
    # tangents: [T, N, d], the frame second
    js = {"out": (7, 11), "tangent_out": (2, 7, 11)}
    m = iso.dependent_elements(cx, "features_jvp", 4, js, buffer="v")
    assert m["tangent_out"].shape == (2, 11) and m["tangent_out"][0].nonzero().flatten().tolist() == [0, 1, 2, 3]
    assert not bool(m["tangent_out"][1].any()) and not bool(m["out"].any())
    m = iso.dependent_elements(cx, "features_jvp", 4, js)
    assert bool(m["tangent_out"][:, [0, 1, 2, 3]].all()) and m["out"].nonzero().flatten().tolist() == [0, 1, 2, 3]
    # the alignment alone, and a head alone
    m = iso.dependent_elements(cx, "align", 1, {"out": (7, 10, 3)})
    assert bool(m["out"].all())
    only_positions = types.SimpleNamespace(items=[(wl.POSITION, list(range(10)))], align=[0, 1, 2, 3], n_inp=10, dims=None)
    m = iso.dependent_elements(only_positions, "backward_x", 1, {"grad_x": (7, 10, 3)})             # the solver's identity: nothing is owed
    assert not bool(m["grad_x"].any())
    assert bool(iso.dependent_elements(only_positions, "features", 1, {"out": (7, 30)})["out"].all())
    m = iso.dependent_elements(types.SimpleNamespace(items=[], align=None, n_inp=6, dims=[6, 8, 3]), "mlp_backward", None,
                               {"grad_f": (7, 6), "grad_params": (83,)}, buffer="f")
    assert bool(m["grad_f"].all()) and "grad_params" not in m
    got = {"out": torch.zeros((7, 11))}
    got["out"][3] = float("nan")
    masks = iso.dependent_elements(cx, "features", 1, {"out": (7, 11)})
    assert iso.not_non_finite(got, masks, [3]) == []
    bad = iso.not_non_finite(got, masks, [2, 3])
    assert len(bad) == 1 and bad[0].startswith("out: frame 2 has 8 finite dependent elements (the first: 0 = 0.0)")
