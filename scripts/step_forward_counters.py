"""bench.py with the forward form's counters read after every EPS.Solve: python scripts/step_forward_counters.py --gpus 1 --steps 300 --warmup 60
prints bench.py's JSON line on standard output and one line FORWARD COUNTERS {...} on standard error - the counters of the solver's basis as the last solve left them (they
accumulate over the solves of one EPS) - and the reason of the last refusal, if any. A bench run must show aborted = 0."""
import os, sys
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import slepc_amd as ks
import bench

last = {}
solve = ks.EPS.Solve


def solve_and_read(self, *a, **kw):
    r = solve(self, *a, **kw)
    last[id(self)] = self.GetBV().step_forward_stats()
    return r


ks.EPS.Solve = solve_and_read
try:
    bench.main()
finally:
    for st in last.values():
        print("FORWARD COUNTERS", st, file=sys.stderr)
