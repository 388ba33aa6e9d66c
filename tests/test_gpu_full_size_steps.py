"""The pair steps bench.py times, at the size it times them, against the CPU oracle driven step by step with the same
config and inputs (oracle/edm_oracle.c: ora_bias_pair_loop, the reference fix's per-pair loop; the batched fix's order
through pre_add_hill, every force, ora_bias_add_hill_list, post_add_hill).  The kernels' forms that only run at these
sizes -- the XCD remap of the short force pass's workgroups, its LDS-staged rows of the counts, the LDS-window pass with
pairs below the window, the pair list's per-atom pass over many workgroups -- are held to the oracle here, not only to
each other.

1. W1 as bench.py runs it (1 M pairs, 4096 hills ahead of the first step, six hill steps; the limiter as bench.py sets
   it, and binding on every step), through both array entries of the reference order and the batch order.
2. The LDS-window force pass (k_pair_forces_ordered_win) without segments: 2 M pairs, walls inside the grid, pairs
   below the window and beyond the walls, a second add_hill on ~70 % of the pairs, the limiter binding.
3. The reference-order pass on W2's 38.8 M pairs, one hill step.
4. The LJ melt from positions as bench.py builds it: 32 000 atoms, ~1.13 M list entries, device RNG, both orders.

Every case asserts which force-pass form ran (edm_hip_bias_get "ordered_window_passes").  Tolerances are those of
tests/test_gpu_fuzz_pairfix.py.  The whole module takes about ten seconds on one MI355X."""
import gc

import numpy as np
import pytest

import edm_amd.hip as H
import edm_amd.workloads as W
from oracle import binding as B

import pairfix_cases as PF
from test_gpu_parity import _parse_hills, close

pytestmark = pytest.mark.gpu

# bench.CFG (bench.py is not imported: it is a script with its own start-up)
BENCH_CFG = ("tempering 0\nhill_prefactor 0.5\nhill_density 250\ndimension 1\nbox_low 0\nbox_high 2.8\n"
             "bias_spacing 0.00025\nbias_sigma 0.025\n")
# tests/k1o_window_worker.py's config: walls at 0.2 and 2.7 inside a grid of 0 to 2.8 (outward copy nodes exist); here
# with a limiter that binds on every hill step (~50 to ~200 hills deferred, none skipped)
WINDOW_CFG = BENCH_CFG.replace("box_low 0\nbox_high 2.8\n", "box_low 0.2\nbox_high 2.7\n") + "bias_per_step 0.3\n"
LIMITER_KEYS = ("overflow_left", "overflow_right", "b_skip_hill_add", "hills_added", "steps")
SLICE = 1 << 22


@pytest.fixture(scope="module", autouse=True)
def _gpu():
    H.require_gpu()
    yield


def _make(cls, text, workdir, tag, *lib):
    cfg = str(workdir / ("%s.edm" % tag))
    hills = str(workdir / ("HILLS_%s" % tag))
    with open(cfg, "w") as fh:
        fh.write(text + "hills_filename %s\nhistogram_filename %s.hist\n" % (hills, hills))
    b = cls(*lib, cfg)
    b.setup(1.0, 1.0)
    b.subdivide([0.0], [2.8], [0.0], [2.8], [0], [0.3])
    return b, hills


def _forces(fg, fo, scale, what):
    bad = np.abs(fg - fo) > 1e-8 * np.abs(fo) + 1e-9 * scale
    assert not bad.any(), "%s: %d/%d forces differ, worst %g of %g" % (what, bad.sum(), len(fo), np.abs(fg - fo).max(), scale)


def _energy(eg, eo, what):
    assert abs(eg - eo) <= 1e-9 * abs(eo) + 1e-12, "%s: energy %.17g, oracle %.17g" % (what, eg, eo)


def _limiter(g, o, what):
    got, want = [int(g.get(k)) for k in LIMITER_KEYS], [int(o.get(k)) for k in LIMITER_KEYS]
    assert got == want, "%s: limiter state %s, oracle %s %s" % (what, got, want, LIMITER_KEYS)
    assert abs(g.get("cum_bias") - o.get("cum_bias")) <= 1e-9 * max(abs(o.get("cum_bias")), 1e-300), (what, g.get("cum_bias"),
                                                                                                      o.get("cum_bias"))


def _step_checks(g, o, eg, eo, fg, fo, what):
    _forces(fg, fo, max(np.abs(fo).max(), 1e-300), what)
    _energy(eg, eo, what)
    _limiter(g, o, what)


def _grid_and_histogram(g, o, what):
    v, _ = g.gauss.download()
    ov = o.gauss.grid.values
    assert np.allclose(v, ov, rtol=1e-9, atol=1e-12 * np.abs(ov).max()), what + ": grid"
    assert np.array_equal(g.hist.values, o.hist.values), what + ": histogram"
    assert int(g.get("ord_gate_giveups")) == 0, what


def _same_hills(got_path, want_path):
    """the HILLS events of a run, in order, against the oracle's (read after both objects are gone: their logs drained)"""
    got, want = _parse_hills(got_path + "_0"), _parse_hills(want_path + "_0")
    assert len(got) == len(want) > 0, (len(got), len(want))
    for a, w in zip(got, want):
        assert a[:3] == w[:3], (a, w)
        close(a[3:], w[3:], rtol=0, atol=2e-8, what="HILLS line")
    return want


def _to_host_slice(d, p0, p1):
    out = np.empty(p1 - p0, d.dtype)
    if p1 > p0:
        H.check(H.lib().edm_hip_memcpy_d2h(out.ctypes.data, d.ptr + p0 * d.dtype.itemsize, out.nbytes))
    return out


def _oracle_batch_order(o, r, xs, us, est):
    """the batched fix's hill step on the oracle: pre_add_hill, every force on the bias it leaves, the add_hill calls in
    order, post_add_hill -> (energy, forces)"""
    o.pre_add_hill(est)
    e, f, _ = o.pair_loop(r, np.zeros(len(r), dtype=np.int32), np.zeros(0), 0, est)
    o.add_hill_list(xs, us)
    o.post_add_hill()
    return e, f


# ---- 1. W1 as bench.py times it ------------------------------------------------------------------------------------
@pytest.mark.parametrize("limiter", ["bench", "binding"])
def test_w1_steps_vs_oracle(limiter, workdir, oracle_lib):
    """bench.py's W1: 4096 hills of 1e-3 first, then the same 1 M pairs and uniforms on every step, est = 2 n.
    `binding` (bias_per_step 0.1): ~52 hills a step, 75 to 124 deferred, b_skip_hill_add in turn."""
    text = BENCH_CFG + ("bias_per_step 0.1\n" if limiter == "binding" else "")
    dev, hills_dev = _make(H.Bias, text, workdir, "dev")
    host, hills_host = _make(H.Bias, text, workdir, "host")
    batch, hills_batch = _make(H.Bias, text, workdir, "batch")
    ora, hills_ora = _make(B.Bias, text, workdir, "ora", oracle_lib)
    ora_b, hills_ora_b = _make(B.Bias, text, workdir, "ora_batch", oracle_lib)
    hills0 = W.pair_distances(4096, 2).reshape(-1, 1)
    for obj in (dev, host, batch, ora, ora_b):
        obj.gauss.add_values(hills0, 1e-3)
    n = W.W1_PAIRS
    r, u = W.pair_distances(n, 1), W.uniform(3, n)
    first = np.arange(n, dtype=np.int32)
    est = 2 * n
    d_r, d_u, d_first = H.DeviceArray.from_host(r), H.DeviceArray.from_host(u), H.DeviceArray.from_host(first)
    d_f, d_fb = H.DeviceArray.zeros((n,)), H.DeviceArray.zeros((n,))
    # the LAMMPS fix's path: page-locked host arrays
    p_r, p_u, p_f, p_first = H.pinned_array(n), H.pinned_array(n), H.pinned_array(n), H.pinned_array(n, np.int32)
    p_r[:], p_u[:], p_first[:] = r, u, first
    zeros = np.zeros(n, dtype=np.int32)
    skipped = 0
    for step in range(6):
        what = "%s step %d" % (limiter, step)
        eo, fo, nc = ora.pair_loop(r, zeros, u, 1, est)
        assert nc == n
        eg = dev.pair_step_ordered_device(d_r, d_f, d_first, n, d_r, d_u, n, est)
        fg = d_f.to_host()
        _step_checks(dev, ora, eg, eo, fg, fo, what + " (device arrays)")
        p_f[:] = 0.0
        eh = host.pair_step_ordered_host(p_r, p_f, p_first, p_r, p_u, est)
        assert np.array_equal(p_f, fg), what + ": the host-array entry's forces differ from the device-array entry's"
        assert abs(eh - eg) <= 1e-12 * abs(eg), (what, eh, eg)
        _limiter(host, ora, what + " (host arrays)")
        eob, fob = _oracle_batch_order(ora_b, r, r, u, est)
        egb = batch.pair_step_device(d_r, d_fb, n, d_r, d_u, n, est)
        _step_checks(batch, ora_b, egb, eob, d_fb.to_host(), fob, what + " (batch order)")
        skipped += int(ora.get("b_skip_hill_add"))
        # W1 is below the window form's size: every pass is the short kernel's
        for obj in (dev, host):
            assert int(obj.get("ordered_window_passes")) == 0, what
            if not ora.get("b_skip_hill_add"):
                assert int(obj.get("ordered_segments")) == 1, what
    assert skipped == (3 if limiter == "binding" else 0), skipped
    _grid_and_histogram(dev, ora, limiter + ", device arrays")
    _grid_and_histogram(host, ora, limiter + ", host arrays")
    _grid_and_histogram(batch, ora_b, limiter + ", batch order")
    del obj, dev, host, batch, ora, ora_b   # (a GPU object writes its last batch's HILLS lines when it is destroyed)
    gc.collect()
    events = _same_hills(hills_dev, hills_ora)
    _same_hills(hills_host, hills_ora)
    _same_hills(hills_batch, hills_ora_b)
    if limiter == "binding":
        assert sum(ev[1] == "u" for ev in events) >= 3, "the limiter must cut a hill short on the steps it deposits"


# ---- 2. the LDS-window force pass without segments -----------------------------------------------------------------
def test_window_form_steps_vs_oracle(workdir, oracle_lib):
    """2 000 003 pairs (odd), every 1001st at 0.1 -- below the window's first node and outside the walls; a second
    add_hill on ~70 % of the pairs; hill, hill, forces only, hill"""
    g, hills_g = _make(H.Bias, WINDOW_CFG, workdir, "win")
    o, hills_o = _make(B.Bias, WINDOW_CFG, workdir, "win_ora", oracle_lib)
    n = 2000003
    r = W.pair_distances(n, 5)
    r[::1001] = 0.1
    d_r = H.DeviceArray.from_host(r)
    d_f = H.DeviceArray.zeros((n,))
    last = 2 * n
    deferred = 0
    for step, hill in enumerate([1, 1, 0, 1]):
        what = "window step %d" % step
        second = (W.uniform(61000 + 10 * step, n) < 0.7).astype(np.int32)
        ru = W.uniform(61001 + 10 * step, 2 * n)
        passes = int(g.get("ordered_window_passes"))
        eo, fo, nc = o.pair_loop(r, second, ru, hill, last)
        if hill:
            xs, us = PF.staged_samples(r, second, ru)
            assert len(xs) == nc
            eg = g.pair_step_ordered_device(d_r, d_f, H.DeviceArray.from_host(PF.first_calls(second)), n,
                                            H.DeviceArray.from_host(xs), H.DeviceArray.from_host(us), nc, est=last)
            last = nc
            assert int(g.get("ordered_segments")) == 1, what
            assert int(g.get("ordered_window_passes")) == passes + 1, what + ": the force pass must be the window form"
            deferred += int(o.get("overflow_right")) > int(o.get("overflow_left"))
        else:
            eg = g.pair_forces_device(d_r, d_f, n)
            assert int(g.get("ordered_window_passes")) == passes, what
        _step_checks(g, o, eg, eo, d_f.to_host(), fo, what)
    assert deferred == 3, "the limiter must bind on every hill step"
    _grid_and_histogram(g, o, "window")
    del g, o
    gc.collect()
    _same_hills(hills_g, hills_o)


# ---- 3. W2's 38.8 M pairs through the reference-order pass ---------------------------------------------------------
def test_w2_reference_order_step_vs_oracle(workdir, oracle_lib):
    """one hill step in the headline's form at W2's size: the distances are the samples, pair k's call is sample k,
    est = 2 n.  Host memory stays near 1.5 GB: the forces are compared in slices."""
    g, hills_g = _make(H.Bias, BENCH_CFG, workdir, "w2")
    o, hills_o = _make(B.Bias, BENCH_CFG, workdir, "w2_ora", oracle_lib)
    n = W.W2_PAIRS
    r = W.pair_distances(n, 11)
    u = W.uniform(12, n)
    d_r, d_u = H.DeviceArray.from_host(r), H.DeviceArray.from_host(u)
    d_first = H.DeviceArray.from_host(np.arange(n, dtype=np.int32))
    d_f = H.DeviceArray.zeros((n,))
    eg = g.pair_step_ordered_device(d_r, d_f, d_first, n, d_r, d_u, n, 2 * n)
    assert int(g.get("ordered_window_passes")) == 1 and int(g.get("ordered_segments")) == 1
    d_first.free()
    d_u.free()
    d_r.free()
    eo, fo, nc = o.pair_loop(r, np.zeros(n, dtype=np.int32), u, 1, 2 * n)
    del r, u
    gc.collect()
    assert nc == n
    scale = np.abs(fo).max()
    for p0 in range(0, n, SLICE):
        p1 = min(n, p0 + SLICE)
        _forces(_to_host_slice(d_f, p0, p1), fo[p0:p1], scale, "W2 pairs [%d, %d)" % (p0, p1))
    _energy(eg, eo, "W2")
    _limiter(g, o, "W2")
    assert int(o.get("hills_added")) > 50
    _grid_and_histogram(g, o, "W2")
    d_f.free()
    del fo, g, o
    gc.collect()
    _same_hills(hills_g, hills_o)


# ---- 4. the LJ melt from positions, as bench.py builds it ----------------------------------------------------------
def close_pairs(xa, cut):
    """every pair i < j of the points xa [n, 3] with |x_i - x_j| <= cut, sorted by (i, j): cKDTree.query_pairs's list,
    from a cell list"""
    lo = xa.min(axis=0)
    nc = np.maximum(((xa.max(axis=0) - lo) // cut).astype(np.int64) + 1, 1)
    c3 = np.minimum(((xa - lo) // cut).astype(np.int64), nc - 1)
    cid = (c3[:, 0] * nc[1] + c3[:, 1]) * nc[2] + c3[:, 2]
    order = np.argsort(cid, kind="stable")
    start = np.searchsorted(cid[order], np.arange(nc.prod() + 1))
    pi, pj = [], []
    for cx in range(nc[0]):
        for cy in range(nc[1]):
            for cz in range(nc[2]):
                k = (cx * nc[1] + cy) * nc[2] + cz
                me = order[start[k]:start[k + 1]]
                if not len(me):
                    continue
                nb = np.concatenate([order[start[q]:start[q + 1]]
                                     for q in ((x * nc[1] + y) * nc[2] + z
                                               for x in range(max(cx - 1, 0), min(cx + 2, nc[0]))
                                               for y in range(max(cy - 1, 0), min(cy + 2, nc[1]))
                                               for z in range(max(cz - 1, 0), min(cz + 2, nc[2])))])
                d = xa[me][:, None, :] - xa[nb][None, :, :]
                ii, jj = np.nonzero(((d * d).sum(axis=2) <= cut * cut) & (me[:, None] < nb[None, :]))
                pi.append(me[ii])
                pj.append(nb[jj])
    pi, pj = np.concatenate(pi), np.concatenate(pj)
    o = np.lexsort((pj, pi))
    return np.stack([pi[o], pj[o]], axis=1).astype(np.int32)


def test_close_pairs_on_a_small_box():
    """the cell list against all pairs by brute force (and cKDTree where scipy is installed)"""
    xa = W.uniform(8, 3 * 600).reshape(600, 3) * 9.0
    d = xa[:, None, :] - xa[None, :, :]
    i, j = np.nonzero(np.triu((d * d).sum(axis=2) <= 2.8 * 2.8, k=1))
    assert np.array_equal(close_pairs(xa, 2.8), np.stack([i, j], axis=1))


@pytest.mark.parametrize("reference_order", [1, 0], ids=["reference_order", "batch_order"])
def test_lj_melt_from_positions_vs_oracle(reference_order, workdir, oracle_lib):
    """32 000 atoms at the LJ-melt density, every pair closer than 2.8 (~1.13 M entries), all atoms owned, one type,
    device RNG seeded 777; three hill steps with the previous step's call count as est, as in bench.py, then a step
    without hills"""
    na = 32000
    box = (na / 0.8442) ** (1.0 / 3.0)
    xa = W.uniform(5, 3 * na).reshape(na, 3) * box
    pr = close_pairs(xa, 2.8)
    try:
        from scipy.spatial import cKDTree
    except ImportError:
        pass
    else:
        q = cKDTree(xa).query_pairs(2.8, output_type="ndarray")
        assert np.array_equal(pr, q[np.lexsort((q[:, 1], q[:, 0]))]), "the cell list's pairs differ from cKDTree's"
    P = len(pr)
    assert P > 1000000
    g, hills_g = _make(H.Bias, BENCH_CFG, workdir, "lj%d" % reference_order)
    o, hills_o = _make(B.Bias, BENCH_CFG, workdir, "lj%d_ora" % reference_order, oracle_lib)
    g.set_device_rng(True, 777)
    g.set("reference_order", reference_order)
    g.pair_list_upload(pr[:, 0], pr[:, 1], np.ones(na, dtype=np.int32))
    d_xa = H.DeviceArray.from_host(xa)
    dvec = xa[pr[:, 0]] - xa[pr[:, 1]]
    r = np.sqrt((dvec ** 2).sum(axis=1))
    dvec = dvec * (1.0 / r)[:, None]
    ones = np.ones(P, dtype=np.int32)
    K, M = 0x632BE59BD9B4E019, (1 << 64) - 1
    calls = 2 * P
    for step, hill in enumerate([1, 1, 1, 0]):
        what = "LJ order %d step %d" % (reference_order, step)
        d_fa = H.DeviceArray.zeros((na, 3))
        eg, nc = g.pair_list_step_device(na, 1, 1, d_xa, d_fa, bool(hill), calls)
        if not hill:
            eo, fo, _ = o.pair_loop(r, ones, np.zeros(0), 0, calls)
        elif reference_order:
            eo, fo, nco = o.pair_loop(r, ones, W.uniform((777 + step * K) & M, 2 * P), 1, calls)
            assert nc == nco == 2 * P, (what, nc, nco)
        else:
            eo, fo = _oracle_batch_order(o, r, np.repeat(r, 2), W.uniform((777 + step * K) & M, 2 * P), calls)
            assert nc == 2 * P, (what, nc)
        if hill:
            calls = nc
        fa = np.zeros((na, 3))
        np.add.at(fa, pr[:, 0], dvec * fo[:, None])
        np.add.at(fa, pr[:, 1], -dvec * fo[:, None])
        fg = d_fa.to_host()
        bad = np.abs(fg - fa) > 1e-8 * np.abs(fa) + 1e-9 * np.abs(fa).max()
        assert not bad.any(), "%s: %d/%d atom force components differ, worst %g" % (what, bad.sum(), fa.size, np.abs(fg - fa).max())
        _energy(eg, eo, what)
        _limiter(g, o, what)
        # (the list's force pass has a kernel of its own: never the pair array's window form)
        assert int(g.get("ordered_window_passes")) == 0
    assert int(o.get("hills_added")) > 0
    _grid_and_histogram(g, o, "LJ order %d" % reference_order)
    del g, o
    gc.collect()
    _same_hills(hills_g, hills_o)
