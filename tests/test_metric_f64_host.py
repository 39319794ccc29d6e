"""The float64 value-and-metric entry points on the host (no GPU): the two symbols are declared, exported and bound and answer a null
plan with MOLANN_E_NULL; MolANN.value_and_metric and PreprocessingANN.value_and_metric exist, refuse a CPU tensor with the
NotImplementedError that names the route that remains (value_and_jacobian and the einsum), and their argument checks - one function
for both methods, run before anything touches a device - refuse wrong `weights` and `into`."""

import os

import pytest
import torch

from molann_amd import _capi, ann, workloads as wl
from molann_amd.ann import MolANN, PreprocessingANN

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SYMBOLS = ["molann_value_and_metric_f64", "molann_plan_supports_value_and_metric_f64"]
EINSUM = r'value_and_jacobian and torch\.einsum\("fkai,a,flai->fkl", jac, w, jac\)'


@pytest.mark.parametrize("name", SYMBOLS)
def test_symbol_declared_exported_and_bound(name):
    header = open(os.path.join(ROOT, "include", "molann_hip.h")).read()
    assert name + "(" in header, name
    fn = getattr(_capi.lib(), name)
    assert fn.argtypes is not None and len(fn.argtypes) == (9 if name == SYMBOLS[0] else 1), name
    assert name in _capi.declared_symbols()


def test_null_plan():
    L = _capi.lib()
    assert L.molann_plan_supports_value_and_metric_f64(None) == _capi.E_NULL
    assert L.molann_value_and_metric_f64(None, None, 1, None, None, None, None, None, None) == _capi.E_NULL
    assert L.molann_value_and_metric_f64(None, None, 0, None, None, None, None, None, None) == _capi.E_NULL


def test_plan_methods_exist():
    assert callable(_capi.Plan.supports_value_and_metric_f64) and callable(_capi.Plan.value_and_metric_f64)
    assert callable(MolANN.value_and_metric) and callable(PreprocessingANN.value_and_metric)
    for method in (MolANN.value_and_metric, PreprocessingANN.value_and_metric):
        doc = " ".join(method.__doc__.split())
        assert "sum_a w_a |grad_a y_k|^2 = dF_k G dF_k^T" in doc, doc


def test_cpu_tensor_names_the_einsum_route():
    w = wl.get_workload("C3")
    model = wl.build_model(w, torch.device("cpu"), 0).double().requires_grad_(False)
    x = w.make_frames(3, seed=1).double()
    with pytest.raises(NotImplementedError, match=EINSUM):
        model.value_and_metric(x)
    with pytest.raises(NotImplementedError, match=EINSUM):
        model.preprocessing_layer.value_and_metric(x)
    with pytest.raises(NotImplementedError, match=EINSUM):
        model.value_and_metric(x, weights=torch.ones(w.n_atoms, dtype=torch.float64))


def test_weights_and_into_are_checked_before_any_device_call():
    """ann._check_metric_args is what both methods call before the plan is looked up; tensors on the meta device stand for 'another
    device' here."""
    n, n_inp, d = 5, 22, 8
    x = torch.zeros((n, n_inp, 3), dtype=torch.float64)
    y, M = torch.zeros((n, d), dtype=torch.float64), torch.zeros((n, d, d), dtype=torch.float64)
    check = lambda weights=None, into=None: ann._check_metric_args("value_and_metric", x, n_inp, d, weights, into)
    w = torch.linspace(0.5, 2.0, n_inp, dtype=torch.float64)
    assert check() == (None, None, None)
    got = check(w, (y, M))
    assert torch.equal(got[0], w) and got[1] is y and got[2] is M
    assert check(w.reshape(n_inp, 1))[0].shape == (n_inp,)
    for bad in (w.float(), w.to(torch.int64), [1.0] * n_inp, 1.0):
        with pytest.raises(TypeError, match="weights"):
            check(bad)
    for bad in (w[:-1], torch.ones(n_inp + 1, dtype=torch.float64), torch.ones((n, n_inp), dtype=torch.float64),
                torch.ones(n_inp, dtype=torch.float64, device="meta")):
        with pytest.raises(ValueError, match="weights"):
            check(bad)
    for bad in ((y,), (y, M, M), (y, None), [y.numpy(), M]):
        with pytest.raises(TypeError, match="into"):
            check(into=bad)
    for bad in ((y.float(), M), (y, M.float())):
        with pytest.raises(TypeError, match="float64"):
            check(into=bad)
    for bad in ((y[:4], M), (y, M[:, :-1]), (y, M[:, :, :-1]), (y.t(), M), (y, torch.zeros((n, d, 2 * d), dtype=torch.float64)[:, :, ::2]),
                (y.to("meta"), M), (y, M.to("meta")), (y, torch.zeros((n, d, n_inp, 3), dtype=torch.float64))):
        with pytest.raises(ValueError, match="into"):
            check(into=bad)
