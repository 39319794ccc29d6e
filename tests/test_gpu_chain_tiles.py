"""State carried from one iteration of a persistent loop to the next, at batch sizes where it is used:

* molann_mlp_chain with more tiles than blocks (csrc/molann_mlp_jit.inc).  Streamed heads keep a ring of NSLAB LDS slab buffers
  whose prefetch runs on across a block's tiles (the stream wraps, the buffer index and the counted waits carry over); the
  resident build copies the stream once and walks it for every tile.  A block runs a second tile only when n_tiles > grid.
* The unfused forward of a wave-per-frame plan past two workspace chunks (molann_forward_packed_f32): from the third chunk on a
  half is reused, after the main stream has waited for the side stream's MLP that read it.

The forward of one frame does not depend on where it sits in the batch, so every row must match, bit for bit, the same plan run
in pieces where each block runs one tile (or each piece fits one chunk).  Sampled rows are also held to a float64 MLP / the float64
oracle (fp32) or to the bf16 arithmetic model (bf16)."""

import re

import numpy as np
import pytest
import torch

from build_util import workload_model
from molann_amd import _capi, workloads as wl
from molann_amd.ann import AlignmentLayer, FeatureLayer, MolANN, PreprocessingANN, create_sequential_nn, last_launch_info
from molann_amd.atomgroup import Universe
from molann_amd.feature import Feature
from oracle import molann_oracle as mo
from test_gpu_mid_frames import _oracle_rows
from test_gpu_mlp_chain import ACTS, _emulate, _params, _plan

pytestmark = pytest.mark.gpu

_CHAIN = re.compile(r"molann_mlp_chain<(bf16|f32),FB=(\d+)(,resident)?> \(plan-specialised(?:; (\d) slab buffers)?\) grid=(\d+) block=(\d+)")


def _chain_info(info):
    m = _CHAIN.search(info)
    assert m, info
    nslab = 1 if m.group(3) else int(m.group(4))
    fb, grid, block = int(m.group(2)), int(m.group(5)), int(m.group(6))
    return nslab, grid, 16 * (block // 64) * fb


def _f64_mlp(f, ws, bs, act):
    h = f.cpu().double()
    for i, (w, b) in enumerate(zip(ws, bs)):
        h = h @ w.cpu().double().T + b.cpu().double()
        if i + 1 < len(ws):
            h = ACTS[act](h)
    return h


def _sample_rows(n, tile, grid, n_tiles, seed):
    """First and last 16 rows of the tiles of blocks 0, 1, grid / 2 and grid - 1 in the first and the last round, the whole last
    tile, and 200 random rows."""
    rows = set()
    rounds = -(-n_tiles // grid)
    for b in (0, 1, grid // 2, grid - 1):
        for r in (0, rounds - 1):
            t = b + r * grid
            if t < n_tiles:
                rows |= set(range(t * tile, min(t * tile + 16, n))) | set(range(max(0, (t + 1) * tile - 16), min((t + 1) * tile, n)))
    rows |= set(range((n_tiles - 1) * tile, n))
    rows |= set(np.random.default_rng(seed).choice(n, size=200, replace=False).tolist())
    return torch.tensor(sorted(rows))


def _check_rows(out, f, idx, ws, bs, act, bf16):
    got = out[idx.to(out.device)].cpu().double()
    fs = f[idx.to(f.device)]
    want = _emulate(fs, ws, bs, act).double() if bf16 else _f64_mlp(fs, ws, bs, act)
    scale = max(1.0, float(want.abs().max()))
    err = float((got - want).abs().max())
    assert err <= (4e-3 if bf16 else 1e-5) * scale, (err, scale)
    return err


@pytest.mark.parametrize("dims,precision,want_nslab", [
    ([341, 512, 256, 16], _capi.MLP_BF16, 4),   # C5's head: 624 KB, slabs of 38 KB, a pair and a lone P
    ([341, 512, 256, 16], _capi.MLP_F32, 4),    # 1.2 MB
    ([700, 64, 8], _capi.MLP_F32, 3),           # 180 KB, slabs of 45 KB
    ([960, 64, 8], _capi.MLP_F32, 2),           # 244 KB, slabs of 61 KB
    ([960, 40], _capi.MLP_F32, 2),              # 180 KB, one layer: a lone P only
    ([126, 64, 32, 2], _capi.MLP_F32, 1),       # P2's head, resident
    ([85, 128, 64, 8], _capi.MLP_F32, 1),       # C4's head, resident
], ids=["C5-bf16", "C5-f32", "700-f32", "960x64-f32", "960x40-f32", "P2-f32", "C4-f32"])
def test_chain_kernel_with_several_tiles_per_block(dims, precision, want_nslab, hip_device):
    """n_tiles = grid + 1, 2 grid, 2 grid + 1 and 3 grid - 1, the last tile five frames short: every row against the same plan run
    in pieces of grid tiles, sampled rows against the reference; then new weights and the largest batch again."""
    act = _capi.ACT_TANH
    bf16 = precision == _capi.MLP_BF16
    plan = _plan(dims, act, n_inp=max(128, dims[0] // 3 + 4), precision=precision)
    ws, bs = _params(dims, hip_device, 5)
    plan.update_mlp(ws, bs)
    gen = torch.Generator(device=hip_device).manual_seed(dims[0])
    probe = torch.randn(1, dims[0], device=hip_device, generator=gen)
    plan.mlp_packed(probe, torch.empty(1, dims[-1], device=hip_device))
    nslab, _, tile = _chain_info(plan.last_launch_info())
    assert nslab == want_nslab, plan.last_launch_info()
    # the grid: one block per CU, at most
    n_probe = (2 * torch.cuda.get_device_properties(hip_device).multi_processor_count + 1) * tile
    f = torch.randn(n_probe, dims[0], device=hip_device, generator=gen)
    plan.mlp_packed(f, torch.empty(n_probe, dims[-1], device=hip_device))
    _, grid, tile2 = _chain_info(plan.last_launch_info())
    assert tile2 == tile and grid < n_probe // tile, plan.last_launch_info()
    counts = (grid + 1, 2 * grid, 2 * grid + 1, 3 * grid - 1)
    n_max = counts[-1] * tile - 5
    f = torch.randn(n_max, dims[0], device=hip_device, generator=gen)

    def run(n):
        out = torch.full((n, dims[-1]), float("nan"), device=hip_device)
        plan.mlp_packed(f[:n], out)
        info = plan.last_launch_info()
        pieces = torch.full((n, dims[-1]), float("nan"), device=hip_device)
        for s in range(0, n, grid * tile):
            e = min(s + grid * tile, n)
            plan.mlp_packed(f[s:e], pieces[s:e])
        torch.cuda.synchronize()
        return out, pieces, info

    for k, n_tiles in enumerate(counts):
        n = n_tiles * tile - 5
        out, pieces, info = run(n)
        nslab, g, _ = _chain_info(info)
        assert g == grid and n_tiles > grid and nslab == want_nslab, info
        assert torch.equal(out, pieces), float((out - pieces).abs().nan_to_num(float("inf")).max())
        err = _check_rows(out, f, _sample_rows(n, tile, grid, n_tiles, k), ws, bs, act, bf16)
        print("%s %s: %s, grid %d, tile %d, %d frames = %d tiles, up to %d per block; max err %.3g"
              % (dims, "bf16" if bf16 else "f32", "resident" if nslab == 1 else "%d slab buffers" % nslab, grid, tile, n, n_tiles,
                 -(-n_tiles // grid), err))
    # the stream is re-read: new weights, the largest batch again
    ws, bs = _params(dims, hip_device, 6)
    plan.update_mlp(ws, bs)
    out, pieces, _ = run(n)
    assert torch.equal(out, pieces)
    _check_rows(out, f, _sample_rows(n, tile, grid, counts[-1], 9), ws, bs, act, bf16)


def _pieces_within_chunks(model, x, wf):
    """The model on pieces of half a chunk (a multiple of 64 frames) that never cross a chunk boundary."""
    step = (wf // 2) & ~63
    ys = []
    for c in range(0, x.shape[0], wf):
        for s in range(c, min(c + wf, x.shape[0]), step):
            ys.append(model(x[s:min(s + step, c + wf)]))
    return torch.cat(ys)


def _boundary_rows(n, wf):
    rows = set(range(0, 64)) | set(range(n - 64, n))
    for c in range(wf, n, wf):
        rows |= set(range(c - 64, min(c + 64, n)))
    return torch.tensor(sorted(rows))


def _chunked_forward_checks(model, x, x2, wf, oracle_rows):
    """Batches of 2 wf + 65 and 3 wf + 1 frames (x, x2: 3 wf + 1 each): whole batch against pieces inside chunks, rows around every
    boundary against `oracle_rows`, then the two 3-chunk batches from two streams back to back."""
    for n in (2 * wf + 65, 3 * wf + 1):
        with torch.no_grad():
            y = model(x[:n])
            info = last_launch_info(model)
            pieces = _pieces_within_chunks(model, x[:n], wf)
        torch.cuda.synchronize()
        assert "chunk=%d" % wf in info, info
        assert torch.equal(y, pieces), float((y - pieces).abs().nan_to_num(float("inf")).max())
        idx = _boundary_rows(n, wf)
        err = oracle_rows(x[idx.to(x.device)].cpu(), y[idx.to(y.device)].cpu().double())
        print("%d frames in chunks of %d (%d chunks): max err %.3g on %d rows" % (n, wf, -(-n // wf), err, len(idx)))
    with torch.no_grad():
        want2 = model(x2)
    torch.cuda.synchronize()
    s1, s2 = torch.cuda.Stream(), torch.cuda.Stream()
    with torch.no_grad():
        with torch.cuda.stream(s1):
            a = model(x)
        with torch.cuda.stream(s2):
            b = model(x2)
        with torch.cuda.stream(s1):
            c = model(x2)
    torch.cuda.synchronize()
    assert torch.equal(a, y) and torch.equal(b, want2) and torch.equal(c, want2)


def _chunk_size(model, x):
    with torch.no_grad():
        model(x[:70])
    info = last_launch_info(model)
    m = re.search(r"chunk=(\d+)", info)
    assert m and ("frames_ring_kernel" in info or "frames_wave_kernel" in info), info
    return int(m.group(1)), info


def test_p2_forward_reuses_both_workspace_halves(hip_device):
    """P2 (166 atoms, positions of the 42 aligned atoms, MLP [126,64,32,2]) at 2 and 3 chunks and a bit."""
    w = wl.get_workload("P2")
    model = workload_model(w, hip_device).requires_grad_(False)
    x = w.make_frames(70, device=hip_device, seed=1)
    wf, info = _chunk_size(model, x)
    x = w.make_frames(3 * wf + 1, device=hip_device, seed=2)
    x2 = w.make_frames(3 * wf + 1, device=hip_device, seed=3)

    def oracle_rows(xs, got):
        err = float((got - _oracle_rows(w, model, xs)[1]).abs().max())
        assert err <= 1e-5, err
        return err

    _chunked_forward_checks(model, x, x2, wf, oracle_rows)


def _streamed_head_plan(dims_tail, precision, device, seed=7):
    """400-atom chain, Kabsch on 24 atoms, the aligned positions of 320 atoms (d = 960)."""
    rng = np.random.default_rng(seed)
    xyz = np.cumsum(rng.normal(size=(400, 3)) * 0.6, axis=0).astype(np.float32)
    xyz -= xyz.mean(axis=0)
    u = Universe(xyz)
    align = sorted(rng.choice(400, size=24, replace=False).tolist())
    pos = sorted(rng.choice(400, size=320, replace=False).tolist())
    feats = [Feature("pos", "position", u.atoms_by_number([a + 1 for a in pos]))]
    pp = PreprocessingANN(AlignmentLayer(u.atoms_by_number([a + 1 for a in align]), u.atoms), FeatureLayer(feats, u.atoms, False))
    torch.manual_seed(seed)
    model = MolANN(pp, create_sequential_nn([pp.output_dimension()] + dims_tail), mlp_precision=precision)
    return xyz, [(wl.POSITION, pos)], align, model.to(device).requires_grad_(False)


def _frames(xyz, n, device, seed):
    g = torch.Generator(device=device).manual_seed(seed)
    return (torch.from_numpy(xyz).to(device).unsqueeze(0) + 0.2 * torch.randn((n, xyz.shape[0], 3), generator=g, device=device)).contiguous()


@pytest.mark.parametrize("dims_tail,precision", [([64, 8], "f32"), ([128, 8], "bf16")], ids=["960x64x8-f32", "960x128x8-bf16"])
def test_streamed_head_forward_reuses_both_workspace_halves(dims_tail, precision, hip_device):
    """A wave-per-frame plan whose head streams its weights ([960,64,8] fp32: 244 KB; [960,128,8] bf16: 244 KB) and whose chunk is
    small (d = 960: about 70 000 frames), at 2 and 3 chunks and a bit."""
    xyz, spec, align, model = _streamed_head_plan(dims_tail, precision, hip_device)
    assert model.preprocessing_layer.output_dimension() == 960
    wf, info = _chunk_size(model, _frames(xyz, 70, hip_device, 1))
    assert "molann_mlp_chain<%s" % precision in info and ",resident" not in info and "slab buffers" in info, info
    assert wf < 80000, wf        # three chunks stay under 1 GB of frames
    x = _frames(xyz, 3 * wf + 1, hip_device, 2)
    x2 = _frames(xyz, 3 * wf + 1, hip_device, 3)
    lins = [m for m in model.ann_layers if isinstance(m, torch.nn.Linear)]
    ref_x = mo.center_reference(torch.from_numpy(xyz[align])).double()

    def oracle_rows(xs, got):
        if precision == "bf16":   # the bf16 arithmetic model on the kernel's own features
            with torch.no_grad():
                feat = model.preprocessing_layer(xs.to(hip_device))
            want = _emulate(feat, [l.weight.detach() for l in lins], [l.bias.detach() for l in lins], _capi.ACT_TANH).double()
            tol = 4e-3 * max(1.0, float(want.abs().max()))
        else:
            want = mo.molann_forward(xs.double(), spec, [l.weight.detach().cpu().double() for l in lins],
                                     [l.bias.detach().cpu().double() for l in lins], False, align, ref_x)
            tol = 1e-5 * max(1.0, float(want.abs().max()))
        err = float((got - want).abs().max())
        assert err <= tol, (err, tol)
        return err

    _chunked_forward_checks(model, x, x2, wf, oracle_rows)
