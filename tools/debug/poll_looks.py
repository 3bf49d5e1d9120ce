"""How many looks (round trips to memory) the polls of the resident half-step's head need, at configs[1]: the counts of a
-DLCF_POLL_LOOKS build of the library (never shipped; see lcf_hip.hip), run with LCF_HIP_LIB=<that build> on the GPU box.
Prints one JSON line: polls that were over after 1, 2, 3 and more looks, their shares, and the mean looks per poll.
    python tools/debug/poll_looks.py [label] [walkers=1024] [steps=1000]"""
import ctypes as C
import json
import os
import sys

sys.path.insert(0, os.getcwd())
import bench  # noqa: E402
from lightcurve_fitting_amd import engine as E  # noqa: E402

label = sys.argv[1] if len(sys.argv) > 1 else 'build'
nw = int(sys.argv[2]) if len(sys.argv) > 2 else 1024
nst = int(sys.argv[3]) if len(sys.argv) > 3 else 1000
model, lc, priors = bench.build_problem(0)
eng = model.engine_for(lc, priors=priors)
s = E.NativeSampler(eng, nw, 7)
s.set_state(bench.initial_walkers(nw))
s.run(0, 200, 'random', False)
lib = E.load_library()
out = (C.c_ulonglong * 4)()
lib.lcf_debug_read_poll_looks.argtypes = [C.c_void_p, C.c_int]
assert lib.lcf_debug_read_poll_looks(out, 1) == 0
s.run(200, nst, 'random', False)
assert lib.lcf_debug_read_poll_looks(out, 0) == 0
one, two, more, looks = (int(v) for v in out)
polls = one + two + more
print(json.dumps(dict(build=label, walkers=nw, steps=nst, kernel=s.last_run_kernel(), polls=polls, expected_polls=nw * nst,
                      looks_1=one, looks_2=two, looks_3_or_more=more, looks_total=looks,
                      share_1=round(one / polls, 4), share_2=round(two / polls, 4), share_3_or_more=round(more / polls, 4),
                      mean_looks_per_poll=round(looks / polls, 4), us_per_half_step=round(1e3 * s.last_run_ms() / (2 * nst), 3))))
