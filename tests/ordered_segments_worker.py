"""Worker of tests/test_gpu_pairfix_order_segments.py::test_long_pair_array_in_segments: one all-samples hill step in the
reference's order on a pair array long enough for the LDS-window force pass (k_pair_forces_ordered_win), its hills cut
into segments of 2048 -- or, with EDM_HIP_TEST_FORCE=no_k1o_window in the environment, the short-array kernel on the
same segments.  Writes the forces to <workdir>/segments_<tag>.npy."""
import hashlib
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import edm_amd.hip as H

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import test_gpu_pairfix_order_segments as T

workdir = sys.argv[1]
tag = os.environ.get("EDM_HIP_TEST_FORCE") or "window"
H.require_gpu()
spec = T.LONG
cfg = os.path.join(workdir, "long_%s.edm" % tag)
with open(cfg, "w") as fh:
    fh.write(spec["cfg"] + "\nhills_filename %s.H\nhistogram_filename %s.hist\n" % (cfg, cfg))
b = H.Bias(cfg)
b.setup(1.0, 1.0)
b.subdivide([spec["lo"]], [spec["hi"]], [spec["lo"]], [spec["hi"]], [0], [spec["skin"]])
b.set("ordered_segment_hills", 2048)
r, second, ru = T.inputs(spec, "long", 0)
xs, us = T.PF.staged_samples(r, second, ru)
first = T.PF.first_calls(second)
n = len(r)
d_r, d_first, d_f = H.DeviceArray.from_host(r), H.DeviceArray.from_host(first), H.DeviceArray.zeros((n,))
d_x, d_u = H.DeviceArray.from_host(xs), H.DeviceArray.from_host(us)
e = b.pair_step_ordered_device(d_r, d_f, d_first, n, d_x, d_u, len(xs), est=spec["nmax"])
f = d_f.to_host()
np.save(os.path.join(workdir, "segments_%s.npy" % tag), f)
print("RESULT", hashlib.sha256(f.tobytes()).hexdigest(), "%.17g" % e, int(b.get("ordered_segments")), len(xs))
