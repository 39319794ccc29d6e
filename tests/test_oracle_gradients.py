"""The float64 oracle's autograd against the reference's own (tests/golden/grad_*.npz and grad2_*.npz): the GPU tests use torch
autograd through the oracle as their stand-in on fresh batches, so its gradients are tied to the reference's here, centred and
assigned (uncentred) references alike.  No GPU."""

import glob
import os

import numpy as np
import pytest
import torch

from golden_util import GOLDEN_DIR
from molann_amd import workloads as wl
from oracle import molann_oracle as mo

GRAD = sorted(os.path.basename(p)[:-4] for p in glob.glob(os.path.join(GOLDEN_DIR, "grad_*.npz")))
GRAD2 = sorted(os.path.basename(p)[:-4] for p in glob.glob(os.path.join(GOLDEN_DIR, "grad2_*.npz")))


def _oracle_model(d):
    """(forward(x, params), params as float64 leaves) of a grad_* / grad2_* case: input group = all atoms."""
    xyz = d["ref_xyz"] if "ref_xyz" in d else wl.ALA_DIPEPTIDE_XYZ
    al, ref_x = None, None
    if "align_numbers" in d:
        al = [a - 1 for a in d["align_numbers"].tolist()]
        ref_x = torch.from_numpy(d["ref_x"]).double() if "ref_x_assigned" in d else mo.center_reference(torch.from_numpy(xyz[al])).double()
    ptr = d["feat_ptr"]
    feats = [(int(t), [a - 1 for a in d["feat_numbers"][ptr[i]:ptr[i + 1]].tolist()]) for i, t in enumerate(d["feat_types"].tolist())]
    uav = bool(d["use_angle_value"])
    n_lin = len(d["mlp_dims"]) - 1 if "mlp_dims" in d else 0
    params = [torch.from_numpy(d[k % i]).double().requires_grad_(True) for i in range(n_lin) for k in ("W%d", "b%d")]

    def forward(x):
        if not feats:
            return mo.align_forward(x, al, ref_x)
        if not params:
            return mo.preprocessing_forward(x, feats, uav, al, ref_x)
        return mo.molann_forward(x, feats, params[0::2], params[1::2], uav, al, ref_x)
    return forward, params


def _rel(got, want):
    return float(np.abs(got - want).max()) / max(1e-12, float(np.abs(want).max()))


def test_gradient_fixtures_are_there():
    assert {"grad_features_C3p_shift", "grad_molann_L1_raw", "grad_align_A5_shift", "grad_features_P2_raw"} <= set(GRAD)
    assert "grad2_features_C3p_shift" in GRAD2
    for name in ("grad_features_C3p_shift", "grad_molann_L1_raw", "grad_align_A5_shift", "grad_features_P2_raw"):
        d = np.load(os.path.join(GOLDEN_DIR, name + ".npz"))
        assert bool(d["ref_x_assigned"])
        assert float(np.abs(d["ref_x"].astype(np.float64).mean(axis=0)).max()) > 1.0      # really off centre


@pytest.mark.parametrize("name", GRAD)
def test_oracle_gradient_matches_reference_autograd(name):
    d = np.load(os.path.join(GOLDEN_DIR, name + ".npz"))
    forward, params = _oracle_model(d)
    x = torch.from_numpy(d["x"]).double().requires_grad_(True)
    out = forward(x)
    assert _rel(out.detach().numpy(), d["out_f64"]) <= 1e-9
    (out * torch.from_numpy(d["G"]).double()).sum().backward()
    assert _rel(x.grad.numpy(), d["gx_f64"]) <= 1e-9, name
    for i, p in enumerate(params):
        assert _rel(p.grad.numpy(), d["gp%d_f64" % i]) <= 1e-9, (name, i)


@pytest.mark.parametrize("name", GRAD2)
def test_oracle_second_order_matches_reference_autograd(name):
    d = np.load(os.path.join(GOLDEN_DIR, name + ".npz"))
    forward, params = _oracle_model(d)
    x = torch.from_numpy(d["x"]).double().requires_grad_(True)
    (F,) = torch.autograd.grad((forward(x) * torch.from_numpy(d["G"]).double()).sum(), x, create_graph=True)
    assert _rel(F.detach().numpy(), d["F_f64"]) <= 1e-9
    (F * F).sum().backward()
    assert _rel(x.grad.numpy(), d["gx2_f64"]) <= 1e-9, name
    for i, p in enumerate(params):
        want = d["gp2_%d_f64" % i]
        if np.abs(want).max() > 0:
            assert _rel(p.grad.numpy(), want) <= 1e-9, (name, i)
