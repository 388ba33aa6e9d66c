"""Development aid: one all-samples hill step of fix edm_pair on the W1 geometry (C1D grid, bias_spacing 0.00025, bias_sigma
0.025, 1 048 576 pairs, no hill_density: every add_hill call deposits, ~1.8 M hills) in the reference's order -- its
force pass in segments of S hills, for a few S -- and, on the same inputs, in batch order (edm_hip_bias_pair_step).
Wall-clock milliseconds per step (the call returns with the energy: the step is complete), median of the timed steps."""
import json
import os
import sys
import tempfile
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tests"))
import edm_amd.hip as H
import edm_amd.workloads as W
import pairfix_cases as PF

H.require_gpu()
STEPS, WARMUP = int(os.environ.get("STEPS", "5")), 2
tmpdir = tempfile.mkdtemp()
n = 1 << 20
u = W.uniform(1, n)
r = np.cbrt(u * (2.8 ** 3 - 0.85 ** 3) + 0.85 ** 3)
second = (W.uniform(2, n) < 0.7).astype(np.int32)
xs, us = PF.staged_samples(r, second, W.uniform(3, 2 * n))
first = PF.first_calls(second)
ns = len(xs)
d_r, d_f, d_first = H.DeviceArray.from_host(r), H.DeviceArray.zeros((n,)), H.DeviceArray.from_host(first)
d_x, d_u = H.DeviceArray.from_host(xs), H.DeviceArray.from_host(us)


def bias(tag):
    cfg = os.path.join(tmpdir, tag + ".edm")
    with open(cfg, "w") as fh:
        fh.write("tempering 0\nhill_prefactor 0.5\nbias_per_step 1000.0\ndimension 1\nbox_low 0\nbox_high 2.8\n"
                 "bias_spacing 0.00025\nbias_sigma 0.025\nhills_filename %s.H\nhistogram_filename %s.hist\n" % (cfg, cfg))
    b = H.Bias(cfg)
    b.setup(1.0, 1.0)
    b.subdivide([0.0], [2.8], [0.0], [2.8], [0], [0.3])
    return b


def timed(step):
    ms = []
    for i in range(WARMUP + STEPS):
        t0 = time.perf_counter()
        step()
        if i >= WARMUP:
            ms.append((time.perf_counter() - t0) * 1e3)
    return float(np.median(ms))


out = {"pairs": n, "hills": ns}
for seg in (2048, 4096, 16384):
    b = bias("ref%d" % seg)
    b.set("ordered_segment_hills", seg)
    out["reference_order_ms_S%d" % seg] = timed(lambda: b.pair_step_ordered_device(d_r, d_f, d_first, n, d_x, d_u, ns, est=ns))
    out["segments_S%d" % seg] = int(b.get("ordered_segments"))
    del b
b = bias("batch")
out["batch_order_ms"] = timed(lambda: b.pair_step_device(d_r, d_f, n, d_x, d_u, ns, est=ns))
print(json.dumps(out))
