"""fix edm_pair in the REFERENCE'S order on steps with more hills than one force pass holds (16 384): the batch's hills
are cut into segments, each segment's record pass starts from the records the previous one left, and each segment's
force pass covers the pairs whose hill count lies in it (OrderedForcesArgs::sel_off, edm_bias.cpp:
ordered_segments_enqueue).  All-samples deposition -- every add_hill call deposits, the reference's default -- reaches
that size at ~10 000 pairs.

* Beyond the cap, both array entries against the oracle driven in the reference's own per-pair loop (bias_pair_loop);
  local tempering, whose hill path takes at most 12 288 hills a step, in forced segments below it.
* Forced small segments (edm_hip_bias_set "ordered_segment_hills") reproduce the reference's goldens, with forces bit
  for bit those of one pass.
* The device-resident pair list in segments, against the oracle and bit for bit against one pass.
* A long pair array in segments of 2048 hills: the LDS-window force form per segment equals the short form and the
  oracle.
"""
import math
import os
import subprocess
import sys

import numpy as np
import pytest

import edm_amd.hip as H
import edm_amd.workloads as W
from oracle import binding as B

import golden_util as GU
import pairfix_cases as PF
from test_gpu_parity import _parse_hills, close

pytestmark = pytest.mark.gpu

CAP = 16384   # hills of one force pass (ORD_MAX_HILLS): the default segment

_ALL = PF.PAIRFIX["all_samples"]
_WALLS = PF.PAIRFIX["walls_inside"]
BEYOND = {
    # the all_samples grid with ~34 000 add_hill calls per hill step: three segments
    "all_samples": dict(_ALL, n=20000, nmax=34000, steps=[1, 1, 0, 1]),
    # walls strictly inside the grid (boundary duplication on real nodes), no hill_density, no binding limiter
    "walls_inside": dict(_WALLS, cfg=_WALLS["cfg"].replace("hill_density 120\n", "").replace("bias_per_step 0.2", "bias_per_step 100.0"),
                         n=10500, nmax=18000, steps=[1, 1, 0, 1]),
    # the limiter binds at hill 17 278 of the first step (second segment): 610 hills go to the overflow buffer, which
    # the next hill step's pre_add_hill flushes
    "limiter_binds": dict(_ALL, cfg=_ALL["cfg"].replace("bias_per_step 100.0", "bias_per_step 0.48"), n=10500, nmax=18000,
                          steps=[1, 0, 1]),
    # heights that read the bias under construction: their hill path takes at most EDM_TAIL_CAP = 12 288 hills a step
    # (batch order too), so ~11 900 hills in forced segments of 4096
    "local_tempering": dict(PF.PAIRFIX["local_tempering"], n=7000, nmax=12000, steps=[1, 1, 0, 1], seg=4096),
}
LIMITER_SEED = 777   # (limiter_binds: the inputs the bias_per_step above was chosen for)

# the long-array case (worker: ordered_segments_worker.py): past PAIR_LDS_THRESHOLD, ~2.55 M hills
LONG = dict(_ALL, n=1500003, nmax=2600000)


def inputs(spec, name, step):
    """(r[n], second[n], uniforms[2 n]) as pairfix_cases.pairfix_inputs draws them, for the cases of this file"""
    seed = LIMITER_SEED if name == "limiter_binds" and step == 0 else 31000 + 100 * sorted(list(BEYOND) + ["long"]).index(name) + step
    n = spec["n"]
    u = W.uniform(seed, n)
    r = np.cbrt(u * (spec["r_hi"] ** 3 - spec["r_lo"] ** 3) + spec["r_lo"] ** 3)
    second = (W.uniform(seed + 31, n) < 0.7).astype(np.int32)
    return r, second, W.uniform(seed + 57, 2 * n)


@pytest.fixture(scope="module", autouse=True)
def _gpu():
    H.require_gpu()
    yield


def _make(cls, spec, name, workdir, tag, *lib):
    cfg = str(workdir / ("%s_%s.edm" % (name, tag)))
    hills = str(workdir / ("HILLS_%s_%s" % (name, tag)))
    with open(cfg, "w") as fh:
        fh.write(spec["cfg"] + "\nhills_filename %s\nhistogram_filename %s.hist\n" % (hills, hills))
    b = cls(*lib, cfg)
    b.setup(1.0, 1.0)
    b.subdivide([spec["lo"]], [spec["hi"]], [spec["lo"]], [spec["hi"]], [0], [spec["skin"]])
    return b, hills


def _ordered_step(b, entry, r, second, ru, est):
    """one hill step through pair_step_ordered_host / _device: (energy, forces, add_hill calls)"""
    xs, us = PF.staged_samples(r, second, ru)
    first = PF.first_calls(second)
    if entry == "host":
        f = np.zeros(len(r))
        e = b.pair_step_ordered_host(r, f, first, xs, us, est=est)
        return e, f, len(xs)
    d_r, d_f, d_first = H.DeviceArray.from_host(r), H.DeviceArray.zeros((len(r),)), H.DeviceArray.from_host(first)
    d_x, d_u = H.DeviceArray.from_host(xs), H.DeviceArray.from_host(us)
    e = b.pair_step_ordered_device(d_r, d_f, d_first, len(r), d_x, d_u, len(xs), est=est)
    return e, d_f.to_host(), len(xs)


def _plain_forces(b, r):
    d_r, d_f = H.DeviceArray.from_host(r), H.DeviceArray.zeros((len(r),))
    e = b.pair_forces_device(d_r, d_f, len(r))
    return e, d_f.to_host()


def _same_hills(got_path, want_path):
    got, want = _parse_hills(got_path), _parse_hills(want_path)
    assert len(got) == len(want)
    for a, w in zip(got, want):
        assert a[:3] == w[:3], (a, w)
        close(a[3:], w[3:], rtol=0, atol=2e-8, what="HILLS line")
    return want


@pytest.mark.parametrize("entry", ["host", "device"])
@pytest.mark.parametrize("name", sorted(BEYOND))
def test_beyond_the_cap_against_the_oracle(name, entry, workdir, oracle_lib):
    spec = BEYOND[name]
    gpu, hills_gpu = _make(H.Bias, spec, name, workdir, entry)
    ora, hills_ora = _make(B.Bias, spec, name, workdir, "oracle_" + entry, oracle_lib)
    seg = spec.get("seg", CAP)
    if seg != CAP:
        gpu.set("ordered_segment_hills", seg)
    last = spec["nmax"]
    segmented = 0
    for step, hill in enumerate(spec["steps"]):
        r, second, ru = inputs(spec, name, step)
        e_o, f_o, nc_o = ora.pair_loop(r, second, ru, hill, last)
        if hill:
            e, f, nc = _ordered_step(gpu, entry, r, second, ru, last)
            assert nc == nc_o
            last = nc
            skipped = int(ora.get("b_skip_hill_add"))
            want_segments = 0 if skipped else math.ceil(nc / seg)   # (all samples: every call is a hill of the batch)
            assert int(gpu.get("ordered_segments")) == want_segments, (step, nc)
            segmented += want_segments > 1
        else:
            e, f = _plain_forces(gpu, r)
        scale = np.abs(f_o).max()
        close(f, f_o, rtol=1e-8, atol=1e-10 * scale, what="%s step %d: forces" % (name, step))
        close(e, e_o, rtol=1e-9, atol=1e-12, what="%s step %d: energy" % (name, step))
        close(gpu.get("cum_bias"), ora.get("cum_bias"), rtol=1e-9, atol=1e-15, what="cum_bias")
        for k in ("hills_added", "overflow_left", "overflow_right", "b_skip_hill_add"):
            assert int(gpu.get(k)) == int(ora.get(k)), (step, k)
    assert segmented >= 1
    v, d = gpu.gauss.download()
    og = ora.gauss.grid
    close(v, og.values, rtol=1e-9, atol=1e-13 * np.abs(og.values).max(), what="grid")
    close(d, og.derivs, rtol=1e-9, atol=1e-11 * max(np.abs(og.derivs).max(), 1e-300), what="derivs")
    assert np.array_equal(gpu.hist.values, ora.hist.values)
    del gpu, ora
    events = _same_hills(hills_gpu + "_0", hills_ora + "_0")
    if name == "limiter_binds":
        # the oracle's own log: the limiter's undo hill of the first step comes after the first segment's hills
        undo = [ev for ev in events if ev[0] == 0 and ev[1] == "u"]
        assert len(undo) == 1 and undo[0][2] > CAP, undo


def _hill_count(name):
    """hills of the first step of a PAIRFIX scenario (its golden log's 'h' lines)"""
    return sum(1 for ev in _parse_hills(os.path.join(GU.GOLDEN, "pairfix_%s.hills.txt" % name)) if ev[0] == 0 and ev[1] == "h")


@pytest.mark.parametrize("name", sorted(PF.PAIRFIX))
def test_forced_small_segments_reproduce_the_goldens(name, workdir):
    spec = PF.PAIRFIX[name]
    gold = np.load(os.path.join(GU.GOLDEN, "pairfix_%s.npz" % name), allow_pickle=False)
    nh0 = _hill_count(name)
    for seg in sorted({1, 7, 64, max(1, nh0 - 1)}):
        cut, hills_cut = _make(H.Bias, spec, name, workdir, "seg%d" % seg)
        one, _ = _make(H.Bias, spec, name, workdir, "one%d" % seg)
        cut.set("ordered_segment_hills", seg)
        assert int(cut.get("ordered_segment_hills")) == seg
        last = spec["nmax"]
        for step, hill in enumerate(spec["steps"]):
            r, second, ru = PF.pairfix_inputs(name, step)
            want_f, want_e = gold["force"][step], gold["energy"][step]
            scale = np.abs(want_f).max()
            if hill:
                e, f, nc = _ordered_step(cut, "host", r, second, ru, last)
                e1, f1, _ = _ordered_step(one, "host", r, second, ru, last)
                last = nc
                if not int(cut.get("b_skip_hill_add")):
                    assert int(one.get("ordered_segments")) == 1
                    assert int(cut.get("ordered_segments")) >= (2 if seg < nh0 // 2 else 1), (seg, step)
                assert np.array_equal(f, f1), "%s S=%d step %d: segments change the forces" % (name, seg, step)
                close(e, e1, rtol=1e-12, atol=1e-15, what="energy (another summation order)")
            else:
                e, f = _plain_forces(cut, r)
            close(f, want_f, rtol=1e-8, atol=1e-10 * scale, what="%s S=%d step %d: forces" % (name, seg, step))
            close(e, want_e, rtol=1e-10, atol=1e-12, what="%s S=%d step %d: energy" % (name, seg, step))
            close(cut.get("cum_bias"), gold["cum_bias"][step], rtol=1e-10, what="cum_bias")
            got = [int(cut.get("overflow_left")), int(cut.get("overflow_right")), int(cut.get("b_skip_hill_add"))]
            assert got == list(gold["overflow"][step])
        v, d = cut.gauss.download()
        close(v, gold["grid_values"], rtol=1e-9, atol=1e-13 * np.abs(gold["grid_values"]).max(), what="grid")
        close(d, gold["grid_derivs"], rtol=1e-9, atol=1e-11 * max(np.abs(gold["grid_derivs"]).max(), 1e-300), what="derivs")
        assert np.array_equal(cut.hist.values, gold["hist"])
        del cut, one
        _same_hills(hills_cut + "_0", os.path.join(GU.GOLDEN, "pairfix_%s.hills.txt" % name))


def _half_list(rng, nall, nlocal, box, cut):
    """positions and a half list in neighbour-list order: for owned i, its neighbours j > i within `cut`"""
    x = rng.uniform(0, box, (nall, 3))
    pi, pj = [], []
    for i in range(nlocal):
        d2 = ((x[i + 1:] - x[i]) ** 2).sum(axis=1)
        js = np.nonzero(d2 < cut * cut)[0] + i + 1
        pi.append(np.full(len(js), i, dtype=np.int32))
        pj.append(js.astype(np.int32))
    return x, np.concatenate(pi), np.concatenate(pj)


LIST_CFG = ("tempering 0\nhill_prefactor 0.3\nbias_per_step 100.0\ndimension 1\nbox_low 0\nbox_high 2.8\n"
            "bias_spacing 0.001\nbias_sigma 0.05\n")


def test_pair_list_beyond_the_cap_against_the_oracle(oracle_lib, workdir):
    """pair_list_step with reference_order 1, device RNG, all-samples deposition, two atom types and ghost atoms:
    ~20 000 add_hill calls per hill step, two segments"""
    cfgs = {}
    for tag in ("gpu", "ora"):
        cfgs[tag] = str(workdir / (tag + ".edm"))
        open(cfgs[tag], "w").write(LIST_CFG + "hills_filename %s/HILLS_%s\nhistogram_filename %s/HIST_%s\n" % (workdir, tag, workdir, tag))
    b = H.Bias(cfgs["gpu"])
    o = B.Bias(oracle_lib, cfgs["ora"])
    for x in (b, o):
        x.setup(1.0, 1.0)
        x.subdivide([0], [2.8], [0], [2.8], [0], [0.3])
    b.set_device_rng(True, 4243)
    b.set("reference_order", 1)
    rng = np.random.default_rng(11)
    nall, nlocal = 2600, 2000
    types = rng.integers(1, 3, nall).astype(np.int32)
    itype, jtype = 1, 2
    est = 30000
    segmented = 0
    for step, hill in enumerate([1, 0, 1]):
        x, pi, pj = _half_list(rng, nall, nlocal, 15.0, 2.8)
        d_fd = H.DeviceArray.zeros((nall, 3))
        b.pair_list_upload(pi, pj, types)
        e, ncalls = b.pair_list_step_device(nlocal, itype, jtype, H.DeviceArray.from_host(x), d_fd, hill, est)
        fd = d_fd.to_host()
        if hill:
            o.pre_add_hill(est)
        E, fref, calls = 0.0, np.zeros((nall, 3)), 0
        for i, j in zip(pi.tolist(), pj.tolist()):
            ti, tj = types[i], types[j]
            if not ((ti == itype and tj == jtype) or (ti == jtype and tj == itype)):
                continue
            dvec = x[i] - x[j]
            r = np.sqrt((dvec ** 2).sum())
            dvec = dvec * (1.0 / r)
            ev, fv = o.update_force([r])
            E += ev
            fref[i] += dvec * fv[0]
            if j < nlocal:
                fref[j] -= dvec * fv[0]
            if hill:
                for _ in range(2 if j < nlocal else 1):   # (all samples: the uniform is not read)
                    o.add_hill([r], 0.5)
                    calls += 1
        if hill:
            o.post_add_hill()
            assert ncalls == calls and calls > CAP, (step, ncalls, calls)
            est = calls
            assert int(b.get("ordered_segments")) == math.ceil(calls / CAP)
            segmented += 1
            close(b.get("cum_bias"), o.get("cum_bias"), rtol=1e-9, what="cum_bias")
            for k in ("overflow_left", "overflow_right", "b_skip_hill_add", "hills_added"):
                assert int(b.get(k)) == int(o.get(k)), (step, k)
        close(e, E, rtol=1e-9, atol=1e-13, what="energy step %d" % step)
        close(fd, fref, rtol=1e-8, atol=1e-11 * max(np.abs(fref).max(), 1e-300), what="forces step %d" % step)
        assert not fd[nlocal:].any(), "newton off: ghost atoms receive no force"
    assert segmented == 2
    v, _ = b.gauss.download()
    og = o.gauss.grid
    close(v, og.values, rtol=1e-9, atol=1e-13 * np.abs(og.values).max(), what="grid")
    assert np.array_equal(b.hist.values, o.hist.values)


@pytest.mark.parametrize("seg", [7, 64])
def test_pair_list_segments_equal_one_pass(seg, workdir):
    """the same list and positions through forced segments and through one pass: per-atom forces bit for bit"""
    out = []
    for tag, s in (("one", 0), ("cut", seg)):
        cfg = str(workdir / ("%s.edm" % tag))
        open(cfg, "w").write(LIST_CFG + "hills_filename %s/H_%s\nhistogram_filename %s/HIST_%s\n" % (workdir, tag, workdir, tag))
        b = H.Bias(cfg)
        b.setup(1.0, 1.0)
        b.subdivide([0], [2.8], [0], [2.8], [0], [0.3])
        b.set_device_rng(True, 99)
        b.set("reference_order", 1)
        b.set("ordered_segment_hills", s)
        rng = np.random.default_rng(21)
        nall, nlocal = 500, 400
        types = rng.integers(1, 3, nall).astype(np.int32)
        res = []
        est = 3000
        for step in range(3):
            x, pi, pj = _half_list(rng, nall, nlocal, 9.0, 2.8)
            d_fd = H.DeviceArray.zeros((nall, 3))
            b.pair_list_upload(pi, pj, types)
            e, nc = b.pair_list_step_device(nlocal, 1, 2, H.DeviceArray.from_host(x), d_fd, True, est)
            est = nc
            res.append((e, d_fd.to_host(), int(b.get("ordered_segments")), nc))
        out.append(res)
    for (e1, f1, s1, nc), (e2, f2, s2, _) in zip(*out):
        assert s1 == 1 and s2 == math.ceil(nc / seg), (s1, s2, nc)
        assert np.array_equal(f1, f2), "segments change the per-atom forces"
        close(e2, e1, rtol=1e-12, atol=0, what="energy")


def test_long_pair_array_in_segments(workdir, oracle_lib):
    """1.5 M pairs (the LDS-window form's size), ~2.55 M hills in segments of 2048: the window form per segment equals
    the short-array kernel (EDM_HIP_TEST_FORCE=no_k1o_window, a worker process: the token is read once per process)
    bit for bit, and the oracle's per-pair loop"""
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    out = {}
    for tag, token in (("window", None), ("short", "no_k1o_window")):
        env = dict(os.environ, PYTHONPATH=root + os.pathsep + os.path.join(root, "tests"))
        env.pop("EDM_HIP_TEST_FORCE", None)
        if token:
            env["EDM_HIP_TEST_FORCE"] = token
        p = subprocess.run([sys.executable, os.path.join(root, "tests", "ordered_segments_worker.py"), str(workdir)],
                           capture_output=True, text=True, env=env, timeout=600)
        assert p.returncode == 0, p.stdout[-2000:] + p.stderr[-2000:]
        line = [ln for ln in p.stdout.splitlines() if ln.startswith("RESULT")][-1].split()
        out[tag] = (line[1], float(line[2]), int(line[3]), int(line[4]))
    assert out["window"][0] == out["short"][0], "the window form's forces differ from the short form's"
    close(out["short"][1], out["window"][1], rtol=1e-12, atol=0, what="energies (another summation order)")
    ncalls = out["window"][3]
    assert out["window"][2] == math.ceil(ncalls / 2048) and out["window"][2] > 1000
    f = np.load(str(workdir / "segments_window.npy"))
    ora, _ = _make(B.Bias, LONG, "long", workdir, "oracle", oracle_lib)
    r, second, ru = inputs(LONG, "long", 0)
    e_o, f_o, nc_o = ora.pair_loop(r, second, ru, 1, LONG["nmax"])
    assert nc_o == ncalls
    close(f, f_o, rtol=1e-8, atol=1e-10 * np.abs(f_o).max(), what="forces vs the oracle")
    close(out["window"][1], e_o, rtol=1e-9, atol=1e-12, what="energy vs the oracle")


def test_segment_size_argument(workdir):
    spec = PF.PAIRFIX["w1_density"]
    b, _ = _make(H.Bias, spec, "w1_density", workdir, "args")
    assert int(b.get("ordered_segment_hills")) == 0 and int(b.get("ordered_segments")) == 0
    for bad in (-1, CAP + 1, 1e9):
        with pytest.raises(H.EdmHipError):
            b.set("ordered_segment_hills", bad)
    assert int(b.get("ordered_segment_hills")) == 0
    b.set("ordered_segment_hills", CAP)
    b.set("ordered_segment_hills", 0)
    # a step at or below the cap: one pass, as before
    r, second, ru = PF.pairfix_inputs("w1_density", 0)
    _ordered_step(b, "device", r, second, ru, spec["nmax"])
    assert int(b.get("ordered_segments")) == 1
