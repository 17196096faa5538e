"""Rate of the fleet deployment loop (sim2sim.FleetInfer) with a latency set, against the loop of the same job
without one -- and, with ``--parent_root``, against a checkout of the parent commit in that job.

    python tools/fleet_latency_rate.py [--out profiles/fleet_latency_rate.txt] [--parent_root ../parent]

The method is tools/fleet_record_rate.py's: for N = 1, 1,024 and 4,096 robots on the flat scene, replayed
graphs of ``chunk`` control periods, HIP events around ``reps`` replays after a warm-up replay, every
measurement from the loop's start state (FleetInfer.restart), median [min, max] of ``repeat``. Eight graphs per
N, measured by turns within every repeat:

  off              FleetInfer._periods, nothing configured: the parent's four launches a period
  zero action      an all-zero latency table through duck_fleet_actuate_delayed: four launches a period, no draw,
                   and the robots move exactly as with the latency off (the same physics work)
  zero both        the same with duck_fleet_sense_delay enqueued as well: five launches a period
  action           an action delay drawn per robot and period over 0..2, no IMU delay: four launches a period,
                   duck_fleet_actuate_delayed in duck_fleet_actuate's place
  both             the same with an IMU delay drawn over 0..2: five launches a period (with a drawn delay the
                   robots move otherwise, so these two periods hold other physics work as well)
  actuate alone    duck_fleet_actuate back to back with itself (a graph of ``chunk`` launches of it)
  delayed alone    duck_fleet_actuate_delayed back to back with itself, both delays drawn
  sense alone      duck_fleet_sense_delay back to back with itself, both delays drawn

``--parent_root`` names a built checkout of the parent commit: its tools/fleet_rate.py is run there as a child
process before this commit's graphs and again after them, and the period with the latency off is checked
against the [min, max] those two runs report, widened by the difference between the two runs' medians.
"""

import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

from open_duck_playground_amd import native  # noqa: E402
from open_duck_playground_amd.sim2sim import FleetInfer, command_grid  # noqa: E402
from tools.fleet_rate_common import (Report, capture, export_policy, parent_run, parent_verdict, parse,  # noqa: E402
                                     parser, replay_seconds, spread)


def main() -> int:
    args = parse("fleet_latency_rate.py", parser())
    say, path = Report(), export_policy()
    chunk, reps, rep = args.chunk, args.reps, args.repeat
    say(f"fleet_latency_rate: flat_terrain, {torch.cuda.get_device_name(0)}, build {native.lib().duck_build_id().decode()[:12]}")
    say(f"graphs of {chunk} control periods, {reps} replays timed with HIP events after a warm-up replay, "
        f"median [min, max] of {rep}, the graphs of one N measured by turns")
    say("latency: delays drawn per robot and period over 0..2 (every lane evaluates the threefry block), seed 1")
    say()
    say(f"{'robots':>7} {'off us':>22} {'zero action us':>22} {'added us':>9} {'zero both us':>22} {'added us':>9} "
        f"{'action us':>22} {'added us':>9} {'both us':>22} {'added us':>9} "
        f"{'actuate alone us':>17} {'delayed alone us':>17} {'sense alone us':>15}")
    cells = command_grid("3x3x3")
    off_period, runs = {}, []
    if args.parent_root:
        runs.append(parent_run(args))
    for n in [int(v) for v in args.sizes.split(",")]:
        def fleet(action, sense):
            f = FleetInfer("flat_terrain", path, n, device=args.device)
            f.set_commands(cells[np.arange(n) % len(cells)])
            f.set_latency(action, sense, seed=1)
            assert f.latent() == (action != 0) and f.lat_sense == (sense != 0)
            return f

        def zero(sense):
            f = fleet(0, 0)
            f._load_latency(np.zeros((n, 4), np.int32), 1)
            f.lat_sense = sense
            return f

        fleets = [fleet(0, 0), zero(False), zero(True), fleet((0, 2), 0), fleet((0, 2), (0, 2))]
        plain, both = fleets[0], fleets[4]

        def alone(call):
            def body():
                for _ in range(chunk):
                    call()
            return body

        graphs = [(f, capture(f, lambda f=f: f._periods(chunk))) for f in fleets] + \
            [(plain, capture(plain, alone(plain.actuate))), (both, capture(both, alone(both.actuate_delayed))),
             (both, capture(both, alone(both.sense_delay)))]
        times = [[] for _ in graphs]
        for _ in range(rep):
            for k, (f, g) in enumerate(graphs):
                times[k].append(replay_seconds(f, g, reps) / chunk * 1e6)
        off, zact, ztwo, act, two, a_alone, d_alone, s_alone = (spread(t) for t in times)
        off_period[n] = off
        fmt = lambda s: f"{s[0]:>8.1f} [{s[1]:.1f}, {s[2]:.1f}]"  # noqa: E731
        say(f"{n:>7} {fmt(off):>22} {fmt(zact):>22} {zact[0] - off[0]:>+9.1f} {fmt(ztwo):>22} {ztwo[0] - off[0]:>+9.1f} "
            f"{fmt(act):>22} {act[0] - off[0]:>+9.1f} {fmt(two):>22} {two[0] - off[0]:>+9.1f} "
            f"{a_alone[0]:>17.1f} {d_alone[0]:>17.1f} {s_alone[0]:>15.1f}")
        del fleets, plain, both, graphs
    if args.parent_root:
        runs.append(parent_run(args))
        parent_verdict(say, runs, off_period, "period with the latency off")
    say.write(args.out)
    return 0


if __name__ == "__main__":
    raise SystemExit(main())
