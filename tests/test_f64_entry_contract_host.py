"""The refusals of the float64 one-launch methods that need no GPU: a CPU tensor is refused by every one of them with the
NotImplementedError that names the route that remains, and the `into` check they share refuses tensors on another device (the meta
device stands for one here) before anything touches a device."""

import pytest
import torch

from molann_amd import ann, workloads as wl


def test_cpu_tensor_names_the_route_that_remains():
    w = wl.get_workload("C3")
    model = wl.build_model(w, torch.device("cpu"), 0).double().requires_grad_(False)
    x = w.make_frames(3, seed=1).double()
    g = torch.ones((3, w.out_dim()), dtype=torch.float64)
    with pytest.raises(NotImplementedError, match="served by one fused plan on a HIP device"):
        model.value_and_vjp(x, g)
    with pytest.raises(NotImplementedError, match=r"value_and_vjp on x\.expand\(d_out, -1, -1\) with torch\.eye\(d_out\)"):
        model.value_and_jacobian(x)
    with pytest.raises(NotImplementedError, match=r"value_and_jacobian and torch\.einsum"):
        model.value_and_metric(x)
    with pytest.raises(NotImplementedError, match=r"value_and_jacobian and torch\.einsum"):
        model.preprocessing_layer.value_and_metric(x)
    with pytest.raises(NotImplementedError):
        model.value_and_jacobian(x, into=(g, g))                       # the gate comes before `into`


@pytest.mark.parametrize("second_shape,pair", [((5, 22, 3), "(y, dx)"), ((5, 8, 22, 3), "(y, jac)"), ((5, 8, 8), "(y, M)")])
def test_into_on_another_device_is_refused_before_any_device_call(second_shape, pair):
    x = torch.zeros((5, 22, 3), dtype=torch.float64)
    y, second = torch.zeros((5, 8), dtype=torch.float64), torch.zeros(second_shape, dtype=torch.float64)
    check = lambda into: ann._check_into("name", x, into, torch.float64, 8, second_shape, pair)       # noqa: E731
    assert check(None) == (None, None)
    got = check((y, second))
    assert got[0] is y and got[1] is second
    assert check([y, second.reshape(-1)])[1].dim() == 1                # the element count is what counts
    for bad in ((y.to("meta"), second), (y, second.to("meta")), (y[:4], second), (y, second[:, :-1]), (y.t(), second)):
        with pytest.raises(ValueError, match="into"):
            check(bad)
    for bad in ((y,), (y, second, second), (y, None)):
        with pytest.raises(TypeError, match=r"pair of tensors \(y, "):
            check(bad)
    for bad in ((y.float(), second), (y, second.float())):
        with pytest.raises(TypeError, match="float64"):
            check(bad)
