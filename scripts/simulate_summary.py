"""Throughput of the fused summary sampler (mmhn_simulate_summary) against the materialised one (mmhn_simulate,
incl. the download), and one long summary run.
python scripts/simulate_summary.py [n_mut] [n_sim] [long n_sim]   (defaults 20, 10^7, 10^9)"""
import os, sys, time
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
from metmhn_amd import Engine, synthetic

n = int(sys.argv[1]) if len(sys.argv) > 1 else 20
ns = int(float(sys.argv[2])) if len(sys.argv) > 2 else 10_000_000
nl = int(float(sys.argv[3])) if len(sys.argv) > 3 else 1_000_000_000
lt, dp, dm = synthetic.random_params(n)
e = Engine(n)
e.simulate(lt, dp, dm, 1000, 1)
e.simulate_summary(lt, dp, dm, 1000, 1)


def best(f, reps=3):
    ts = []
    for _ in range(reps):
        t0 = time.perf_counter(); f(); ts.append(time.perf_counter() - t0)
    return min(ts), float(np.median(ts))


td, tdm = best(lambda: e.simulate(lt, dp, dm, ns, 2))
ts, tsm = best(lambda: e.simulate_summary(lt, dp, dm, ns, 2))
print(f"n_mut={n}, {ns} samples: simulate_dat {ns / td / 1e6:.1f} M samples/s (best of 3; median {ns / tdm / 1e6:.1f}), "
      f"simulate_summary {ns / ts / 1e6:.1f} M samples/s (median {ns / tsm / 1e6:.1f})", flush=True)
if nl > 0:
    t0 = time.perf_counter(); c = e.simulate_summary(lt, dp, dm, nl, 3); tl = time.perf_counter() - t0
    print(f"simulate_summary {nl} samples: {tl:.2f} s ({nl / tl / 1e6:.1f} M samples/s), seeded {c[1] / c[0]:.4f}", flush=True)
