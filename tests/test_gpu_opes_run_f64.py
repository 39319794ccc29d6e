"""A whole OPES step on the device with no read-back: frames_value_opes_table_f64_kernel (`MolANN.value_and_opes_table`: the bias from
the table's state in device memory) and opes_step_f64_kernel (`molann_amd.bias.OpesRun.deposit`: this step's kernels formed from the
bias launch's outputs and deposited).

  bias   `value_and_opes_table` against `value_and_opes` called with n and norm = S / n taken from `read_state()`: torch.equal on y,
         bias and dx - the walk, the transform and every sum's order are the same code.
  step   the device against its host twin `molann_selftest_opes_step_f64` on tests/opes_run_cases.py's scenarios (held against the
         oracle on the host by tests/test_opes_run_f64_host.py): counts and slots equal, rows and scalars within that module's 1e-12
         bounds - the device's exp and pow may differ from the host's by an ulp; how many cases came out bit for bit is printed.
  loop   bias then deposit, 30 steps of 4 walkers on C3's preprocessing behind a [d_feat, 32, 2] tanh head: the eager loop against
         the CPU loop of the host twins, and one captured graph of the two launches, replayed, against the eager loop's bits."""

import math

import pytest
import torch

import isolation
import opes_deposit_cases as cases
import opes_run_cases as rc
import opes_run_oracle as run_oracle
import placement as pl
import test_gpu_random_backward as rb
import test_gpu_value_and_hills_f64 as vh
import test_gpu_value_and_vjp_f64 as vv
from molann_amd import _capi, ann, workloads as wl
from molann_amd import bias as mbias

pytestmark = pytest.mark.gpu
F64 = torch.float64
NAN, INF = float("nan"), float("inf")
CPU = torch.device("cpu")
KERNEL = "frames_value_opes_table_f64_kernel"
CAP, CUTOFF, THRESHOLD = 600, 5.0, 1.0
_BITS = {"same": 0, "cases": 0}


# ---------------------------------------------------------------------------------------------- the bias from the table's state
def _outputs(model, x, d):
    """The model's outputs of x, by the new call on an empty table."""
    empty = mbias.OpesTable(1, d, x.device)
    y = model.value_and_opes_table(x, empty, rc.SCALE, rc.EPSILON)[0]
    torch.cuda.synchronize()
    return y


def _filled_table(dev, y_tab, n_live, capacity, period, cutoff, seed):
    """A table of `n_live` kernels next to the outputs `y_tab` (rows reused in turn, a width of noise on each), widths 0.2-0.5 of the
    outputs' spread, heights 0.5-1.5, S recomputed on the device; the dead rows are NaN."""
    d = y_tab.shape[1]
    t = mbias.OpesTable(capacity, d, dev, period=period, cutoff=cutoff, threshold=THRESHOLD)
    for v in (t.centers, t.sigma, t.heights):
        v.fill_(NAN)
    if n_live:
        g = torch.Generator().manual_seed(seed)
        spread = y_tab.std(dim=0).cpu() + 0.05 if y_tab.shape[0] > 1 else torch.full((d,), 0.3, dtype=F64)
        sigma = spread * (0.2 + 0.3 * torch.rand(n_live, d, dtype=F64, generator=g))
        rows = y_tab.cpu()[torch.arange(n_live) % y_tab.shape[0]]
        t.centers[:n_live] = (rows + sigma * torch.randn(n_live, d, dtype=F64, generator=g)).to(dev)
        t.sigma[:n_live], t.heights[:n_live] = sigma.to(dev), (0.5 + torch.rand(n_live, dtype=F64, generator=g)).to(dev)
        t.state[0] = float(n_live)
        t.recompute_sum(n=n_live)
    return t


def _same_as_value_and_opes(model, x, table, what):
    n, total, _, _ = table.read_state()
    got = model.value_and_opes_table(x, table, rc.SCALE, rc.EPSILON)
    torch.cuda.synchronize()
    info = vh._info(model)
    assert info.startswith(KERNEL + " (values + opes from the table's state in one launch; ") and info.count("_kernel") == 1, info
    want = model.value_and_opes(x, table.centers[:n], table.heights[:n], table.sigma[:n], rc.SCALE, total / n if n else 1.0, rc.EPSILON, table.cutoff,
                                table.period)
    torch.cuda.synchronize()
    assert len(got) == 3 and all(torch.equal(a, b) for a, b in zip(got, want)), what
    assert [tuple(v.shape) for v in got] == [(x.shape[0], table.d), (x.shape[0],), tuple(x.shape)]
    return got, info


@pytest.mark.parametrize("n_inp,lanes", [(7, 8), (12, 16), (30, 32), (40, 64)])
@pytest.mark.parametrize("aligned", [True, False], ids=["aligned", "no_alignment"])
@pytest.mark.parametrize("head", [True, False], ids=["head", "features"])
def test_lane_groups(n_inp, lanes, aligned, head, hip_device):
    """Every lane-group width, with and without an alignment and a head, 1 and 65 frames, 40 live kernels under a capacity of 64 (a lane
    with several kernels, with one, with none), output 0 periodic, cutoff 5."""
    case = vh._small_case(n_inp, aligned, head)
    model = case.build(hip_device).double().requires_grad_(False)
    d_out = case.mlp[-1] if head else case.d_feat()
    if head:       # the head's widest layer input (the 12 feature columns) asks for at least 16 lanes
        lanes = max(lanes, 16)
    period = torch.zeros(d_out, dtype=F64)
    period[0] = 1.3
    y_tab = _outputs(model, case.frames(65, seed=900 + n_inp, dev=CPU).double().to(hip_device), d_out)
    table = _filled_table(hip_device, y_tab, 40, 64, period, CUTOFF, n_inp)
    for n in (1, 65):
        x = case.frames(n, seed=n_inp + n, dev=CPU).double().to(hip_device)
        (y, v, dx), info = _same_as_value_and_opes(model, x, table, (case.name, aligned, head, n))
        assert "%d lanes per frame" % lanes in info, info
        assert bool(torch.isfinite(v).all()) and float((v - rc.SCALE * math.log(rc.EPSILON)).abs().max()) > 0.0 and float(dx.abs().max()) > 0.0


@pytest.mark.parametrize("name,n", [("P1", 9), ("C4", 3)])
def test_larger_frames(name, n, hip_device):
    w, model, _ = vv._shared(name, hip_device)
    d = w.out_dim()
    y_tab = _outputs(model, w.make_frames(17 if name == "C4" else 65, seed=8).double().to(hip_device), d)
    table = _filled_table(hip_device, y_tab, 75, 100, vh._period_row(d, 1.1, 3), 4.0, 60)
    (_, v, dx), _ = _same_as_value_and_opes(model, w.make_frames(n, seed=7).double().to(hip_device), table, name)
    assert bool(torch.isfinite(v).all()) and float(dx.abs().max()) > 0.0


@pytest.mark.parametrize("n", [1, 65])
@pytest.mark.parametrize("n_live", [0, 1, 300])
def test_table_sizes(n_live, n, hip_device):
    """C3 (8 outputs): no kernel yet, one, 300 under a capacity of 600, with and without a cutoff.  Without kernels the bias is scale
    log(epsilon) and dx exactly 0 while every table tensor holds NaN: nothing of the table is read."""
    w, model, _ = vv._shared("C3", hip_device)
    d = w.out_dim()
    x = w.make_frames(n, seed=21 + n).double().to(hip_device)
    y_tab = _outputs(model, w.make_frames(65, seed=22).double().to(hip_device), d)
    for cutoff in (None, 4.0):
        table = _filled_table(hip_device, y_tab, n_live, CAP, vh._period_row(d, 1.1, 3), cutoff, 23 + n_live)
        (y, v, dx), _ = _same_as_value_and_opes(model, x, table, (n_live, n, cutoff))
        if n_live == 0:
            assert bool(torch.isnan(table.centers).all()) and bool(torch.isnan(table.sigma).all()) and bool(torch.isnan(table.heights).all())
            assert bool((v == rc.SCALE * math.log(rc.EPSILON)).all()) and float(dx.abs().max()) == 0.0
            assert torch.equal(y, model.value_and_vjp(x, torch.zeros_like(y))[0])
        else:
            assert bool(torch.isfinite(v).all()) and float(dx.abs().max()) > 0.0
    # a count the table cannot hold is held to it: NaN and -1 read as no kernel, capacity + 5 as the whole table
    if n_live == 300 and n == 1:
        full = _filled_table(hip_device, y_tab, CAP, CAP, None, 4.0, 29)
        want = model.value_and_opes(x, full.centers, full.heights, full.sigma, rc.SCALE, full.read_state()[1] / CAP, rc.EPSILON, 4.0)
        for n0, kernels in ((NAN, 0), (-1.0, 0), (CAP + 5.0, CAP)):
            full.state[0] = n0
            got = model.value_and_opes_table(x, full, rc.SCALE, rc.EPSILON)
            if kernels:
                assert all(torch.equal(a, b) for a, b in zip(got, want)), n0
            else:
                assert bool((got[1] == rc.SCALE * math.log(rc.EPSILON)).all()) and float(got[2].abs().max()) == 0.0, n0


def test_two_calls_and_the_callers_buffers(hip_device):
    w, model, _ = vv._shared("C3", hip_device)
    d = w.out_dim()
    x = w.make_frames(65, seed=31).double().to(hip_device)
    table = _filled_table(hip_device, _outputs(model, x, d), 45, 64, None, CUTOFF, 32)
    a = model.value_and_opes_table(x, table, rc.SCALE, rc.EPSILON)
    into = (torch.full((65, d), NAN, dtype=F64, device=hip_device), torch.full((65,), NAN, dtype=F64, device=hip_device), torch.full_like(x, NAN))
    b = model.value_and_opes_table(x, table, rc.SCALE, rc.EPSILON, into=into)
    assert all(u is v for u, v in zip(b, into)) and all(pl.same_bits(u, v) for u, v in zip(a, b))
    empty = model.value_and_opes_table(x[:0], table, rc.SCALE, rc.EPSILON)
    assert [tuple(t.shape) for t in empty] == [(0, d), (0,), (0, w.n_atoms, 3)]
    with pytest.raises(ValueError, match="columns"):
        model.value_and_opes_table(x, mbias.OpesTable(8, d - 1, hip_device), rc.SCALE, rc.EPSILON)
    with pytest.raises(TypeError, match="OpesTable"):
        model.value_and_opes_table(x, (table.centers, table.heights), rc.SCALE, rc.EPSILON)
    with pytest.raises(ValueError, match="epsilon"):
        model.value_and_opes_table(x, table, rc.SCALE, 0.0)
    with pytest.raises(TypeError, match="float64"):
        model.value_and_opes_table(x.float(), table, rc.SCALE, rc.EPSILON)


def test_offset_caller_buffers_inside_guard_bands_and_the_operators(tmp_path, hip_device):
    """The C entry on buffers carved out of an arena, every one at another residue of 16 bytes, between guard bands: the outputs have
    the bits of the ctypes call on fresh tensors, no band and no input is written; the dispatcher operators give those bits too."""
    import warnings
    w, model, _ = vv._shared("C3", hip_device)
    n, d, H, cap = 65, w.out_dim(), 45, 50
    x = w.make_frames(n, seed=55).double().to(hip_device)
    period = vh._period_row(d, 1.1, 2).to(hip_device)
    t = _filled_table(hip_device, _outputs(model, x, d), H, cap, period, 4.0, 56)
    entry, lins = model._fast_state(x)["entry"](), [m for m in model.ann_layers if isinstance(m, torch.nn.Linear)]
    extra = (t.centers, t.heights, t.sigma, t.state, t.period, rc.SCALE, rc.EPSILON, 4.0)
    fresh = ann._one_launch_ctypes(ann._OPES_TABLE, entry, x, extra, None, None, (n, w.n_atoms, 3), d, lins, rb._align_layer(model))
    torch.cuda.synchronize()
    assert entry.plan.last_launch_info().startswith(KERNEL)
    arena = pl.Arena(hip_device, capacity=8 << 20)
    inputs = (("x", x), ("centers", t.centers), ("heights", t.heights), ("sigma", t.sigma), ("state", t.state), ("period", period))
    outputs = (("out", (n, d)), ("bias", (n,)), ("grad_x", (n, w.n_atoms, 3)))
    views = {}
    for i, (name, data) in enumerate(inputs):
        views[name] = arena.carve(name, data.shape, F64, (i + 1) % 2, data=data)
    for i, (name, shape) in enumerate(outputs):
        views[name] = arena.carve(name, shape, F64, i % 2)
    assert len(set(v.data_ptr() % 16 for v in views.values())) == 2
    with torch.cuda.device(hip_device):
        W, B = [lin.weight.detach().contiguous() for lin in lins], [lin.bias.detach().contiguous() for lin in lins]
        code = _capi.lib().molann_value_and_opes_table_f64(entry.plan._handle, views["x"].data_ptr(), n, *_capi._layer_pointers(W, B),
                                                           views["centers"].data_ptr(), views["heights"].data_ptr(), views["sigma"].data_ptr(), cap,
                                                           views["state"].data_ptr(), views["period"].data_ptr(), rc.SCALE, rc.EPSILON, 4.0,
                                                           views["out"].data_ptr(), views["bias"].data_ptr(), views["grad_x"].data_ptr(),
                                                           torch.cuda.current_stream().cuda_stream)
        torch.cuda.synchronize()
    assert code == 0
    assert arena.check() == [] and arena.inputs_changed() == []
    assert all(pl.same_bits(views[name], want) for (name, _), want in zip(outputs, fresh))
    assert bool(torch.isfinite(fresh[2]).all()) and float(fresh[2].abs().max()) > 0.0
    # the scripted model's operators
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        torch.jit.script(model).save(str(tmp_path / "c3_f64.pt"))
    loaded = torch.jit.load(str(tmp_path / "c3_f64.pt"), map_location=hip_device)
    ws, bs = [lin.weight for lin in loaded.linears.children()], [lin.bias for lin in loaded.linears.children()]
    desc = list(loaded.desc)
    handle = torch.ops.molann.register_desc(desc)
    by_handle = torch.ops.molann.value_and_opes_table_h(x, handle, loaded.ref_x, ws, bs, t.centers, t.heights, t.sigma, t.state, period, rc.SCALE,
                                                        rc.EPSILON, 4.0, [])
    by_desc = torch.ops.molann.value_and_opes_table(x, desc, loaded.ref_x, ws, bs, t.centers, t.heights, t.sigma, t.state, period, rc.SCALE, rc.EPSILON,
                                                    4.0, [])
    torch.cuda.synchronize()
    info = torch.ops.molann.launch_info(desc, hip_device.index)
    assert info.count(KERNEL) == 1 and info.count("_kernel") == 1, info
    assert all(torch.equal(a, b) for a, b in zip(by_handle, fresh)) and all(torch.equal(a, b) for a, b in zip(by_desc, fresh))
    with pytest.raises(ValueError, match="cutoff"):
        torch.ops.molann.value_and_opes_table(x, desc, loaded.ref_x, ws, bs, t.centers, t.heights, t.sigma, t.state, period, rc.SCALE, rc.EPSILON, 0.0, [])
    with pytest.raises(ValueError, match="state"):
        torch.ops.molann.value_and_opes_table(x, desc, loaded.ref_x, ws, bs, t.centers, t.heights, t.sigma, t.state[:3], period, rc.SCALE, rc.EPSILON,
                                              4.0, [])


def test_the_bias_entrys_return_codes(hip_device):
    """The family's order - plan, n, NULL, alignment, items - then capacity and the three scalars, each MOLANN_E_DESC; nothing is
    launched on a refusal."""
    x = wl.get_workload("C3").make_frames(3, seed=91).double().to(hip_device)
    with torch.cuda.device(hip_device):
        p = _capi.Plan(22, features=[(wl.BOND, [0, 1])])
        pa = _capi.Plan(22, align_idx=[0, 1, 2, 3], ref_x=torch.zeros(4, 3))     # no items: nothing to bias
        assert p.supports_value_and_opes_table_f64() and not pa.supports_value_and_opes_table_f64()
        new = lambda *shape: torch.full(shape, NAN, dtype=F64, device=hip_device)       # noqa: E731
        y, v, dx = new(3, 1), new(3), new(3, 22, 3)
        one = torch.ones(4, dtype=F64, device=hip_device)          # a table of one kernel at 1 with width 1, state (1, 1, 1, 1)
        L, stream = _capi.lib(), torch.cuda.current_stream().cuda_stream
        good = dict(plan=p, centers=one.data_ptr(), heights=one.data_ptr(), sigma=one.data_ptr(), capacity=1, state=one.data_ptr(), period=None,
                    scale=2.25, epsilon=1e-3, cutoff=4.0)

        def raw(**changes):
            a = dict(good, **changes)
            return L.molann_value_and_opes_table_f64(a["plan"]._handle if a["plan"] is not None else None, x.data_ptr(), 3, None, None, a["centers"],
                                                     a["heights"], a["sigma"], a["capacity"], a["state"], a["period"], a["scale"], a["epsilon"], a["cutoff"],
                                                     y.data_ptr(), v.data_ptr(), dx.data_ptr(), stream)

        bad = [dict(capacity=0), dict(capacity=-3), dict(scale=NAN), dict(scale=INF), dict(epsilon=NAN), dict(epsilon=INF), dict(epsilon=0.0),
               dict(epsilon=-1e-3), dict(cutoff=NAN), dict(cutoff=0.0), dict(cutoff=-4.0)]
        for change in bad:
            assert raw(**change) == _capi.E_DESC, change
            # what comes before keeps its code
            assert raw(plan=None, **change) == _capi.E_NULL and raw(plan=pa, **change) == _capi.E_STAGE, change
            for name in ("centers", "heights", "sigma", "state"):
                assert raw(**dict(change, **{name: None})) == _capi.E_NULL, (change, name)
                assert raw(**dict(change, **{name: one.data_ptr() + 4})) == _capi.E_ALIGNMENT, (change, name)
            assert raw(period=one.data_ptr() + 4, **change) == _capi.E_ALIGNMENT
        # n_frames == 0 returns before anything is looked at
        assert L.molann_value_and_opes_table_f64(p._handle, None, 0, None, None, None, None, None, 0, None, None, NAN, -1.0, 0.0, None, None, None, stream) == 0
        torch.cuda.synchronize()
        assert all(bool(torch.isnan(t).all()) for t in (y, v, dx)), "a refusal launched"
        assert raw() == 0 and raw(scale=-2.25) == 0 and raw(cutoff=INF) == 0
        torch.cuda.synchronize()
        assert p.last_launch_info().startswith(KERNEL)
        bond = (x[:, 0] - x[:, 1]).norm(dim=1)
        assert float((y[:, 0] - bond).abs().max()) <= 1e-12
        assert float((v - 2.25 * torch.log(torch.exp(-0.5 * (bond - 1.0) ** 2) + 1e-3)).abs().max()) <= 1e-12      # norm = S / n = 1


# ---------------------------------------------------------------------------------------------- the step against its host twin
def _device_run(dev, sc, n0, capacity=CAP):
    period, table, y, V, sigma0, sigma_min = sc
    d = y.shape[1]
    t = mbias.OpesTable(capacity, d, dev, period=period, cutoff=CUTOFF, threshold=THRESHOLD)
    t.centers[:n0], t.sigma[:n0], t.heights[:n0] = (v.to(dev) for v in table)
    t.state[:2] = torch.tensor([float(n0), cases.brute_force_S(*table, period, CUTOFF)], dtype=F64).to(dev)
    run = mbias.OpesRun(_NoModel(), t, rc.KT, rc.BIASFACTOR, rc.BARRIER, sigma0, sigma_min)
    run.run[:3] = torch.tensor(rc.RUN0, dtype=F64).to(dev)
    return t, run


class _NoModel(object):
    def value_and_opes_table(self, *args, **kwargs):
        raise AssertionError("the step tests deposit only")


def _snapshot(t, run):
    torch.cuda.synchronize()
    return tuple(v.cpu() for v in (t.centers, t.sigma, t.heights, t.state, run.run))


def _device_steps(dev, n0, d, width):
    sc = rc.step_scenario(n0, d)
    t, run = _device_run(dev, sc, n0)
    y, V = sc[2].to(dev), sc[3].to(dev)
    for i in range(0, y.shape[0], width):
        assert run.deposit(y[i:i + width], V[i:i + width]) is None
    return _snapshot(t, run)


@pytest.mark.parametrize("width", [1, 4])
@pytest.mark.parametrize("d", [1, 8])
@pytest.mark.parametrize("n0", [60, 520])
def test_the_step_matches_its_host_twin(n0, d, width, hip_device):
    host, _ = rc.host_scenario_run(n0, d, width)
    got = _device_steps(hip_device, n0, d, width)
    worst, bits = rc.assert_same_run(got, host.snapshot(), (n0, d, width))
    _BITS["cases"] += 1
    _BITS["same"] += 1 if bits else 0
    print("n0 %d d %d W %d: worst error / bound %.3g, %s; so far %d of %d cases bit for bit"
          % (n0, d, width, worst, "the host's bits" if bits else "exp or pow an ulp off", _BITS["same"], _BITS["cases"]))
    assert int(got[3][0]) > n0 and float(got[4][0]) == rc.RUN0[0] + 16


@pytest.mark.parametrize("fixed_sigma,with_min", [(True, False), (True, True), (False, False)])
def test_fixed_widths_and_no_floor_match_the_host_twin(fixed_sigma, with_min, hip_device):
    dev, n0, d = hip_device, 60, 8
    period, table, y, V, sigma0, sigma_min = rc.step_scenario(n0, d)
    sigma_min = sigma_min if with_min else None
    total0 = cases.brute_force_S(*table, period, CUTOFF)
    host = rc.HostRun(CAP, d, period, CUTOFF, THRESHOLD, sigma0, sigma_min, fixed_sigma)
    host.table.fill(*table, total0)
    t = mbias.OpesTable(CAP, d, dev, period=period, cutoff=CUTOFF, threshold=THRESHOLD)
    t.centers[:n0], t.sigma[:n0], t.heights[:n0] = (v.to(dev) for v in table)
    t.state[:2] = torch.tensor([float(n0), total0], dtype=F64).to(dev)
    run = mbias.OpesRun(_NoModel(), t, rc.KT, rc.BIASFACTOR, rc.BARRIER, sigma0, sigma_min, fixed_sigma)
    for i in range(0, 16, 4):
        host.step(y[i:i + 4], V[i:i + 4])
        run.deposit(y[i:i + 4].to(dev), V[i:i + 4].to(dev))
    got = _snapshot(t, run)
    rc.assert_same_run(got, host.snapshot(), (fixed_sigma, with_min))
    assert (float(got[4][4]) == 1.0) == fixed_sigma and float(got[4][0]) == 16.0
    if fixed_sigma:       # sigma0 is above the floor: the new kernels keep sigma0 and their heights are the weights
        assert run.read_run()["sigma_scale"] == 1.0


def test_two_runs_give_the_same_bits(hip_device):
    a, b = _device_steps(hip_device, 520, 8, 4), _device_steps(hip_device, 520, 8, 4)
    assert all(pl.same_bits(u, v) for u, v in zip(a, b))


@pytest.mark.parametrize("bad", ["nan_V", "inf_V", "overflow_V", "nan_y"])
def test_an_invalid_walker_behaves_as_on_the_host(bad, hip_device):
    dev, n0, d = hip_device, 60, 8
    sc = rc.step_scenario(n0, d)
    y, V = sc[2][:4].clone(), sc[3][:4].clone()
    if bad == "nan_y":
        y[2, 3] = NAN
    else:
        V[2] = {"nan_V": NAN, "inf_V": INF, "overflow_V": 1000.0}[bad]
    host = rc.HostRun(CAP, d, sc[0], CUTOFF, THRESHOLD, sc[4], sc[5], False)
    host.table.fill(*sc[1], cases.brute_force_S(*sc[1], sc[0], CUTOFF))
    host.run[:3] = torch.tensor(rc.RUN0, dtype=F64)
    host.step(y, V)
    t, run = _device_run(dev, sc, n0)
    run.deposit(y.to(dev), V.to(dev))
    got = _snapshot(t, run)
    rc.assert_same_run(got, host.snapshot(), bad)
    assert int(got[3][3]) == 1 and float(got[4][0]) == rc.RUN0[0] + 3 and bool(torch.isfinite(got[4]).all()) and bool(torch.isfinite(got[3]).all())
    # a step of that walker alone changes nothing but the count of the refused
    t, run = _device_run(dev, sc, n0)
    before = _snapshot(t, run)
    run.deposit(y[2:3].to(dev), V[2:3].to(dev))
    after = _snapshot(t, run)
    assert pl.same_bits(after[4][:3], before[4][:3]) and float(after[3][3]) == 1.0 and pl.same_bits(after[3][:3], before[3][:3])
    assert all(pl.same_bits(u, v) for u, v in zip(after[:3], before[:3]))


@pytest.mark.parametrize("offset", [0, 1])
def test_guard_bands_around_every_buffer_of_the_step(offset, hip_device):
    """The table, state, run, y, V and the width rows in an arena of guard bands, the table FULL after the run (capacity = n0 + 3): nothing
    before a buffer, nothing after its last row, the inputs as they were, and the host twin's run."""
    dev, n0, d = hip_device, 60, 8
    period, table, y, V, sigma0, sigma_min = rc.step_scenario(n0, d)
    cap = n0 + 3
    arena = pl.Arena(dev, capacity=4 << 20)
    centers, sigma = arena.carve("centers", (cap, d), F64, offset), arena.carve("sigma", (cap, d), F64, offset)
    heights, state = arena.carve("heights", (cap,), F64, offset, row_dims=0), arena.carve("state", (4,), F64, offset, row_dims=0)
    run = arena.carve("run", (8,), F64, offset, row_dims=0)
    per = arena.carve("period", (d,), F64, offset, data=period, row_dims=0)
    yy, vv_ = arena.carve("y", y.shape, F64, offset, data=y), arena.carve("V", V.shape, F64, offset, data=V, row_dims=0)
    s0 = arena.carve("sigma0", (d,), F64, offset, data=sigma0, row_dims=0)
    smin = arena.carve("sigma_min", (d,), F64, offset, data=sigma_min, row_dims=0)
    centers.zero_(), sigma.zero_(), heights.zero_(), run.zero_()
    centers[:n0], sigma[:n0], heights[:n0] = (v.to(dev) for v in table)
    total0 = cases.brute_force_S(*table, period, CUTOFF)
    state.copy_(torch.tensor([float(n0), total0, 0.0, 0.0], dtype=F64))
    run[:3] = torch.tensor(rc.RUN0, dtype=F64).to(dev)
    host = rc.HostRun(cap, d, period, CUTOFF, THRESHOLD, sigma0, sigma_min, False)
    host.table.fill(*table, total0)
    host.run[:3] = torch.tensor(rc.RUN0, dtype=F64)
    host.step(y, V)
    with torch.cuda.device(dev):
        _capi.opes_step_f64(centers, sigma, heights, state, run, per, yy, vv_, s0, smin, rc.BETA, THRESHOLD, CUTOFF, False)
    torch.cuda.synchronize()
    assert arena.check() == [] and arena.inputs_changed() == []
    got = tuple(v.cpu() for v in (centers, sigma, heights, state, run))
    rc.assert_same_run(got, host.snapshot(), offset)
    assert int(got[3][0]) == cap and int(got[3][3]) > 0, got[3]


def test_the_step_operator_gives_the_ctypes_bits(hip_device):
    from molann_amd import script
    script.load_ops()
    dev, n0, d = hip_device, 520, 8
    want = _device_steps(dev, n0, d, 4)
    sc = rc.step_scenario(n0, d)
    t, run = _device_run(dev, sc, n0)
    y, V = sc[2].to(dev), sc[3].to(dev)
    for i in range(0, 16, 4):
        torch.ops.molann.opes_step(t.centers, t.sigma, t.heights, t.state, run.run, t.period, y[i:i + 4], V[i:i + 4], run.sigma0, run.sigma_min, rc.BETA,
                                   THRESHOLD, CUTOFF, False)
    assert all(pl.same_bits(u, v) for u, v in zip(_snapshot(t, run), want))
    with pytest.raises(ValueError, match="beta"):
        torch.ops.molann.opes_step(t.centers, t.sigma, t.heights, t.state, run.run, t.period, y[:4], V[:4], run.sigma0, None, 0.0, THRESHOLD, CUTOFF, True)
    with pytest.raises(ValueError, match="run"):
        torch.ops.molann.opes_step(t.centers, t.sigma, t.heights, t.state, run.run[:4], t.period, y[:4], V[:4], run.sigma0, None, 1.0, THRESHOLD, CUTOFF, True)


# ---------------------------------------------------------------------------------------------- the loop
STEPS, WALKERS, LOOP_CAP = 30, 4, 128
_LOOP = {}


def _loop_model(dev):
    if "model" not in _LOOP:
        w, model, _ = vv._workload("C3", dev, head=[32, 2], act=torch.nn.Tanh())
        xs = [w.make_frames(WALKERS, seed=500 + i).double().to(dev) for i in range(STEPS)]
        y_all = torch.cat([_outputs(model, x, 2) for x in xs]).cpu()
        sigma0 = 0.35 * y_all.std(dim=0)
        _LOOP.update(model=model, w=w, xs=xs, y_all=y_all, sigma0=sigma0, sigma_min=0.6 * sigma0,
                     period=torch.tensor([0.0, 4.0 * float(y_all[:, 1].abs().max())], dtype=F64))
    return _LOOP


def _new_run(dev):
    L = _loop_model(dev)
    table = mbias.OpesTable(LOOP_CAP, 2, dev, period=L["period"], cutoff=CUTOFF, threshold=THRESHOLD)
    return mbias.OpesRun(L["model"], table, rc.KT, rc.BIASFACTOR, rc.BARRIER, L["sigma0"], L["sigma_min"])


def _eager_loop(dev):
    """The eager loop, once: per step (y, V, dx) and the table, state and run after it, all on the CPU."""
    if "eager" not in _LOOP:
        L = _loop_model(dev)
        run = _new_run(dev)
        steps = []
        for x in L["xs"]:
            y, v, dx = run.bias(x)
            run.deposit(y, v)
            steps.append(tuple(t.cpu() for t in (y, v, dx)) + (_snapshot(run.table, run),))
        _LOOP["eager"] = steps
    return _LOOP["eager"]


def test_the_eager_loop_against_the_cpu_loop_of_the_host_twins(hip_device):
    L, eager = _loop_model(hip_device), _eager_loop(hip_device)
    host = rc.HostRun(LOOP_CAP, 2, L["period"], CUTOFF, THRESHOLD, L["sigma0"], L["sigma_min"], False)
    ref = run_oracle.RunOracle(LOOP_CAP, 2, L["period"], CUTOFF, THRESHOLD, rc.KT, rc.BIASFACTOR, rc.BARRIER, L["sigma0"], L["sigma_min"], False)
    worst_v = worst = 0.0
    for i, (y, v, dx, after) in enumerate(eager):
        assert torch.equal(y, L["y_all"][WALKERS * i:WALKERS * (i + 1)])      # the outputs do not depend on the table
        hv, _ = host.bias(y)
        # the device sums P lane by lane, the host in one sequence: at most 128 positive terms, each an exp at 1-2 ulp
        worst_v = max(worst_v, float(((v - hv).abs() / (rc.BOUND * torch.clamp(hv.abs(), min=1.0))).max()))
        host.step(y, hv)
        ref.step(y, hv)
        ratio, _ = rc.assert_same_run(after, host.snapshot(), "step %d" % i)
        worst = max(worst, ratio)
    print("30 steps of 4 walkers: n %d merges %d refused %d; worst error / bound: bias %.3g, table and scalars %.3g"
          % (host.table.counts() + (worst_v, worst)))
    assert worst_v <= 1.0
    # conditions on the inputs, on the oracle alone: every decision clear of the threshold and of its runner-up; merges and appends
    # both happen, the widths are rescaled
    assert ref.table.counts() == host.table.counts()
    assert min(m[0] for m in ref.table.margins) >= 1e-9 and min(m[1] for m in ref.table.margins) >= 1e-9
    assert ref.table.merges > 0 and ref.table.n > 8 and ref.table.refused == 0 and ref.sigma_scale < 1.0
    print("sigma_min held a width up in %d of %d steps; sigma_scale %.4g, neff %.4g" % (ref.bound_steps, STEPS, ref.sigma_scale, ref.neff))
    assert float(eager[-1][2].abs().max()) > 0.0 and float(eager[0][2].abs().max()) == 0.0


def test_one_captured_graph_replays_the_loop_and_reads_device_memory(hip_device):
    dev = hip_device
    L, eager = _loop_model(dev), _eager_loop(dev)
    run = _new_run(dev)
    t = run.table
    x_static = L["xs"][0].clone()
    into = (torch.empty(WALKERS, 2, dtype=F64, device=dev), torch.empty(WALKERS, dtype=F64, device=dev), torch.empty_like(x_static))
    side = torch.cuda.Stream(device=dev)
    side.wait_stream(torch.cuda.current_stream(dev))
    with torch.cuda.stream(side):               # a step outside the capture: plans, libraries and caches are made here
        run.deposit(*run.bias(x_static, into=into)[:2])
    torch.cuda.current_stream(dev).wait_stream(side)
    torch.cuda.synchronize()
    for v in (t.centers, t.sigma, t.heights, t.state, run.run):
        v.zero_()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):               # one stream, two launches in a chain
        run.deposit(*run.bias(x_static, into=into)[:2])
    torch.cuda.synchronize()
    assert float(t.state.abs().max()) == 0.0 and float(run.run.abs().max()) == 0.0, "the capture ran the launches"
    for i, (x, (y, v, dx, after)) in enumerate(zip(L["xs"], eager)):
        x_static.copy_(x)
        graph.replay()
        got = tuple(u.cpu() for u in into)
        assert all(pl.same_bits(a, b) for a, b in zip(got, (y, v, dx))), "step %d: y, V or dx" % i
        assert all(pl.same_bits(a, b) for a, b in zip(_snapshot(t, run), after)), "step %d: table, state or run" % i
    # another table and state under the same graph: the launches read device memory, nothing was baked in at capture
    last = tuple(u.cpu() for u in into)
    snap = eager[9][3]
    for dst, src in zip((t.centers, t.sigma, t.heights, t.state, run.run), snap):
        dst.copy_(src.to(dev))
    x_static.copy_(L["xs"][10])
    graph.replay()
    got = tuple(u.cpu() for u in into)
    assert all(pl.same_bits(a, b) for a, b in zip(got, eager[10][:3])) and not pl.same_bits(got[1], last[1])
    assert all(pl.same_bits(a, b) for a, b in zip(_snapshot(t, run), eager[10][3]))


def test_a_nan_walker_changes_no_other_walkers_outputs(hip_device):
    dev = hip_device
    L, eager = _loop_model(dev), _eager_loop(dev)
    run = _new_run(dev)
    for dst, src in zip((run.table.centers, run.table.sigma, run.table.heights, run.table.state, run.run), eager[19][3]):
        dst.copy_(src.to(dev))
    x = L["xs"][20]
    clean = dict(zip(("y", "V", "dx"), run.bias(x)))
    assert all(pl.same_bits(clean[k].cpu(), want) for k, want in zip(("y", "V", "dx"), eager[20][:3]))
    bad_x = isolation.poison({"x": x}, [2], "nan", where={"x": 3 * isolation.chosen_atom([a - 1 for a in L["w"].align],
                                                                                       [(ty, [a - 1 for a in at]) for ty, at in L["w"].features])
                                                          + isolation.COORD})["x"]
    poisoned = dict(zip(("y", "V", "dx"), run.bias(bad_x)))
    torch.cuda.synchronize()
    assert isolation.keep_rows_equal(clean, poisoned, [2], ("y", "V", "dx")) == []
    assert not bool(torch.isfinite(poisoned["V"][2])) and bool(torch.isnan(poisoned["dx"][2]).any())
    # and the step refuses that walker alone
    run.deposit(poisoned["y"], poisoned["V"])
    state, scalars = run.table.read_state(), run.read_run()
    assert state[3] == 1 and scalars["counter"] == WALKERS * 20 + 3 and math.isfinite(scalars["neff"]) and math.isfinite(state[1])
    assert set(scalars) == {"counter", "sum_w", "sum_w2", "neff", "sigma_scale", "rct"}
