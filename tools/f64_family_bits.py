#!/usr/bin/env python3
"""The bits of the eight float64 value-and-bias kernels, written to a file or held against one: the check that a change to their
shared frame loop (frame_value_term_loop_f64, molann_dev_vjp_f64.inc) or to a term's pieces changes no output bit.

    python tools/f64_family_bits.py --write parent.npz          # on a build of the commit to compare with
    python tools/f64_family_bits.py --against parent.npz        # on the new build: exit 1 on the first tensor that differs
    python tools/f64_family_bits.py --lib PATH/libmolann_hip.so --write parent.npz      # another build of the library, same tree

Entries: value_and_restraint, value_and_hills, value_and_grid, value_and_bias, value_and_opes, value_and_opes_table and value_and_bias
with ``opes=`` an `Opes` or an `OpesFromTable`.  Models: the small cases of the entries' own lane-group tests (`small_case`), 7, 12, 30 and 40
atoms - lane groups of 8, 16, 32 and 64; a head asks for at least 16 - with and without a head, with and without an alignment.  67
frames from a fixed seed (two full blocks of a lane group of 8 and a ragged one), frame 5 with a NaN coordinate.  Term variants: the
restraint absent, plain, or with periods, flat bottoms and a centre per frame; 0 and 37 hills or kernels; one sigma row or one per
hill; the table absent or present with a periodic axis; a table state with n = 0 and n = 37.  y, the energies and grad_x are kept as
int64 views: NaN payloads and the sign of zero count."""
import argparse
import os
import re
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import numpy as np  # noqa: E402
import torch  # noqa: E402

F64 = torch.float64
N_FRAMES, NAN_FRAME, N_ROWS = 67, 5, 37
SIZES = (7, 12, 30, 40)
LANES = (8, 16, 32, 64)
SCALE, EPSILON, CUTOFF = 2.25, 1e-3, 4.0
ENTRIES = ("restraint", "hills", "grid", "bias", "opes", "bias_opes", "opes_table", "bias_opes_table")


def _rand(g, *shape):
    return torch.rand(shape, generator=g, dtype=F64)


class Terms(object):
    """Everything the eight entries take, from one seed, laid out over the model's outputs; y_tab: NaN-free outputs of the model"""

    def __init__(self, y_tab, dev, seed):
        from molann_amd import bias as mb
        g = torch.Generator().manual_seed(seed)
        y = y_tab.cpu()
        d = y.shape[1]
        on = lambda t: t.to(dev).contiguous()       # noqa: E731
        spread = y.std(dim=0) + 0.05
        self.d, self.dev = d, dev
        # restraint: plain (one centre row) and full (a centre per frame, every second output periodic, flat bottoms)
        self.kappa = on(5.0 + 20.0 * _rand(g, d))
        self.center = on(y.mean(dim=0))
        self.center_rows = on(y[torch.arange(N_FRAMES) % y.shape[0]] + 0.3 * spread * torch.randn(N_FRAMES, d, generator=g, dtype=F64))
        period = torch.zeros(d, dtype=F64)
        period[::2] = 1.3
        self.period, self.flat = on(period), on(0.2 * spread * _rand(g, d))
        # hills / kernels on the columns hc (all outputs for the single entries), a table on gc
        self.hc = tuple(range(d)) if d <= 2 else (d - 1, 0, 2)
        self.gc = (1, 0) if d <= 2 else (1, 3)
        self.rows, self.rows_c = self._rows(y, spread, range(d), g, on), self._rows(y, spread, self.hc, g, on)
        self.grid = self._grid(y, range(min(d, 2)), g, on)
        self.grid_c = self._grid(y, self.gc, g, on)
        self.mb = mb

    @staticmethod
    def _rows(y, spread, cols, g, on):
        cols = list(cols)
        k = len(cols)
        sig = spread[cols] * (0.2 + 0.3 * _rand(g, N_ROWS, k))
        centers = y[torch.arange(N_ROWS) % y.shape[0]][:, cols] + sig * torch.randn(N_ROWS, k, generator=g, dtype=F64)
        period = torch.zeros(k, dtype=F64)
        period[0] = 1.3
        return dict(centers=on(centers), heights=on(0.5 + _rand(g, N_ROWS)), sigma_rows=on(sig), sigma=on(sig[0]), period=on(period), k=k)

    @staticmethod
    def _grid(y, cols, g, on):
        cols = list(cols)
        shape, periodic = (5, 6)[:len(cols)], [False, True][:len(cols)]
        lo, hi = y[:, cols].min(dim=0).values, y[:, cols].max(dim=0).values
        spacing = [float(hi[k] - lo[k]) / (n if per else n - 1) for k, (n, per) in enumerate(zip(shape, periodic))]
        return dict(table=on(torch.randn(shape, generator=g, dtype=F64)), lower=[float(v) for v in lo], spacing=spacing, periodic=periodic)

    def restraint(self, kind):
        if kind == "none":
            return None
        if kind == "plain":
            return self.mb.Restraint(self.center, self.kappa)
        return self.mb.Restraint(self.center_rows, self.kappa, self.period, self.flat)

    def table(self, rows, n_live):
        """An OpesTable with capacity N_ROWS + 19 whose first n_live rows are `rows`; the dead rows NaN; S set, not summed"""
        t = self.mb.OpesTable(N_ROWS + 19, rows["k"], self.dev, period=rows["period"], cutoff=CUTOFF)
        for v in (t.centers, t.sigma, t.heights):
            v.fill_(float("nan"))
        if n_live:
            t.centers[:n_live], t.sigma[:n_live], t.heights[:n_live] = rows["centers"][:n_live], rows["sigma_rows"][:n_live], rows["heights"][:n_live]
            t.state[0], t.state[1] = float(n_live), 0.02 * n_live * float(rows["heights"][:n_live].sum())
        return t


def _variants(entry, model, x, T):
    """[(name, call)] of an entry: call() -> (y, energies, grad_x)"""
    mb = T.mb
    out = []
    tables = [("n%d_%s" % (n, s), n, s) for n, s in ((0, "shared"), (N_ROWS, "shared"), (N_ROWS, "rows"))]

    def rows_of(R, n, s):
        return R["centers"][:n], R["heights"][:n], (R["sigma_rows"][:n] if s == "rows" else R["sigma"])

    if entry == "restraint":
        for kind in ("plain", "full"):
            r = T.restraint(kind)
            out.append((kind, lambda r=r: model.value_and_restraint(x, r.center, r.kappa, r.period, r.flat)))
    elif entry in ("hills", "opes") and T.d <= 8:
        for name, n, s in tables:
            c, h, sg = rows_of(T.rows, n, s)
            if entry == "hills":
                out.append((name, lambda c=c, h=h, sg=sg: model.value_and_hills(x, c, h, sg, T.rows["period"])))
            else:
                norm = 0.02 * max(float(h.sum()), 1.0)
                out.append((name, lambda c=c, h=h, sg=sg, norm=norm: model.value_and_opes(x, c, h, sg, SCALE, norm, EPSILON, CUTOFF, T.rows["period"])))
    elif entry == "grid" and T.d <= 2:
        G = T.grid
        out.append(("periodic_axis", lambda: model.value_and_grid(x, G["table"], G["lower"], G["spacing"], G["periodic"])))
    elif entry == "opes_table" and T.d <= 8:
        for n in (0, N_ROWS):
            t = T.table(T.rows, n)
            out.append(("state_n%d" % n, lambda t=t: model.value_and_opes_table(x, t, SCALE, EPSILON)))
    elif entry in ("bias", "bias_opes", "bias_opes_table"):
        G = mb.Grid(T.grid_c["table"], T.grid_c["lower"], T.grid_c["spacing"], T.grid_c["periodic"], columns=T.gc)
        R = T.rows_c
        for rk, (name, n, s), grid in (("none", tables[1], G), ("full", tables[2], G), ("full", tables[0], None), ("plain", tables[2], None),
                                      ("none", tables[0], G)):
            r = T.restraint(rk)
            label = "r_%s-%s-%s" % (rk, name, "table" if grid is not None else "no_table")
            c, h, sg = rows_of(R, n, s)
            if entry == "bias":
                H = mb.Hills(c, h, sg, R["period"], columns=T.hc)
                out.append((label, lambda r=r, H=H, grid=grid: model.value_and_bias(x, restraint=r, hills=H, grid=grid)))
                if rk == "full" and grid is not None:
                    out.append(("r_full-no_hills-table", lambda r=r, grid=grid: model.value_and_bias(x, restraint=r, grid=grid)))
            elif entry == "bias_opes":
                O = mb.Opes(c, h, sg, SCALE, 0.02 * max(float(h.sum()), 1.0), EPSILON, CUTOFF, R["period"], columns=T.hc)
                out.append((label, lambda r=r, O=O, grid=grid: model.value_and_bias(x, restraint=r, grid=grid, opes=O)))
            elif s == "rows" or n == 0:         # a table holds a sigma row per kernel
                O = mb.OpesFromTable(T.table(R, n), SCALE, EPSILON, columns=T.hc)
                out.append((label.replace("-n", "-state_n"), lambda r=r, O=O, grid=grid: model.value_and_bias(x, restraint=r, grid=grid, opes=O)))
    return out


def small_case(n_inp, aligned, head, two_outputs):
    """The small model of the entries' lane-group tests, as a `Case` of tests/test_gpu_random_backward.py: a chain of n_inp atoms; two
    dihedrals sharing atoms 2 and 3, an angle and a bond on their atoms and, behind a head, the positions of atoms 4 and 6 (12 feature
    columns, a [12, 5, 2] tanh head); atoms 0, 2, 4, 6 aligned or no alignment; the atoms from 7 on untouched.  two_outputs (the
    table's entry, at most 3 outputs): without a head only the angle and the bond."""
    from molann_amd import workloads as wl
    from test_gpu_random_backward import Case
    feats = [(wl.DIHEDRAL, [0, 1, 2, 3]), (wl.DIHEDRAL, [2, 3, 4, 5]), (wl.ANGLE, [3, 4, 5]), (wl.BOND, [0, 5])]
    if head:
        feats.append((wl.POSITION, [4, 6]))
    elif two_outputs:
        feats = feats[2:]
    case = Case("bits%d" % n_inp, wl.synthetic_chain(n_atoms=n_inp, step=1.4, seed=3), feats, align=[0, 2, 4, 6] if aligned else None)
    if head:
        case.mlp = [case.d_feat(), 5, 2]
    return case


def run(dev):
    """{key: int64 array} of every case, and {entry: lane groups seen}"""
    from molann_amd import ann
    results, seen = {}, dict((e, set()) for e in ENTRIES)
    for n_inp in SIZES:
        for head in (True, False):
            for aligned in (True, False):
                for entry in ENTRIES:
                    case = small_case(n_inp, aligned, head, entry == "grid")
                    model = case.build(dev).double().requires_grad_(False)
                    x = case.frames(N_FRAMES, seed=1000 + n_inp, dev=torch.device("cpu")).double()
                    x_tab = case.frames(65, seed=2000 + n_inp, dev=torch.device("cpu")).double().to(dev)
                    x[NAN_FRAME, 0, 1] = float("nan")
                    x = x.to(dev)
                    with torch.no_grad():
                        y_tab = model(x_tab)
                    T = Terms(y_tab, dev, seed=3000 + n_inp + 10 * head + aligned)
                    for name, call in _variants(entry, model, x, T):
                        out = call()
                        torch.cuda.synchronize()
                        info = model.last_launch_info() if isinstance(model, ann.MolANN) else ann.last_launch_info(model)
                        m = re.search(r"(\d+) lanes per frame", info)
                        want = "frames_value_%s_f64_kernel" % entry
                        assert m and want in info and info.count("_kernel") == 1, (entry, name, info)
                        lanes = int(m.group(1))
                        seen[entry].add(lanes)
                        if not bool(torch.isnan(out[2][NAN_FRAME]).any()):
                            print("f64_family_bits: note: %s %s atoms=%d: the NaN frame's gradient is finite" % (entry, name, n_inp))
                        for tensor, t in zip(("y", "energies", "grad_x"), out):
                            key = "%s|atoms=%d|%s|%s|%s|G=%d|%s" % (entry, n_inp, "head" if head else "features",
                                                                  "aligned" if aligned else "no_alignment", name, lanes, tensor)
                            assert key not in results, key
                            results[key] = t.detach().contiguous().cpu().numpy().view(np.int64).copy()
    return results, seen


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--write", default="", help="write every case's bits to this .npz")
    ap.add_argument("--against", default="", help="compare every case's bits with this .npz; exit 1 on the first difference")
    ap.add_argument("--lib", default="", help="load this libmolann_hip.so instead of the tree's")
    args = ap.parse_args()
    if bool(args.write) == bool(args.against):
        ap.error("one of --write and --against")
    from molann_amd import _capi
    if args.lib:
        _capi.LIB_PATH = os.path.abspath(args.lib)
    results, seen = run(torch.device("cuda:0"))
    with open("/proc/self/maps") as maps:       # the build that ran: one library, the one asked for
        loaded = sorted(set(line.split()[-1] for line in maps if "libmolann_hip" in line))
    print("f64_family_bits: ran %s" % ", ".join(loaded))
    assert loaded == [os.path.realpath(_capi.LIB_PATH)], (loaded, _capi.LIB_PATH)
    for entry, lanes in seen.items():
        assert tuple(sorted(lanes)) == LANES, (entry, "lane groups", sorted(lanes))
    launches = len(results) // 3
    if args.write:
        np.savez_compressed(args.write, **results)
        print("f64_family_bits: wrote %d tensors of %d launches to %s" % (len(results), launches, args.write))
        return 0
    ref = np.load(args.against)
    if sorted(ref.files) != sorted(results):
        print("f64_family_bits: the cases differ: %s" % sorted(set(ref.files) ^ set(results))[:8])
        return 1
    for key in results:
        a, b = ref[key], results[key]
        if a.shape != b.shape or not np.array_equal(a, b):
            entry, _, _, _, _, lanes, tensor = key.split("|")
            bad = int((a != b).sum()) if a.shape == b.shape else -1
            print("f64_family_bits: DIFFERENT entry=%s %s tensor=%s (%d of %d words)   [%s]" % (entry, lanes, tensor, bad, a.size, key))
            return 1
    print("f64_family_bits: %d tensors of %d launches equal %s bit for bit (every entry at G = 8, 16, 32, 64)" % (len(results), launches, args.against))
    return 0


if __name__ == "__main__":
    sys.exit(main())
